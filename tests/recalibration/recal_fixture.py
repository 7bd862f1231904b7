"""The seeded detection sets of the recalibration tests: the issue's fixture (recal_ref.fixture) as result dicts with ground truth, the
partitions ground-truth matching gives on them (known by construction, so the host path needs no GPU), and the host-only
fit -> apply -> measure chain whose improvement ratios the end-to-end bar rests on."""
import numpy as np
import torch

from pod_compare_amd import compute_calibration_errors as cce
from pod_compare_amd import evaluation_utils as ev
from pod_compare_amd import recalibration as rc
from tests.recalibration import recal_ref as ref

K = 7
CMAP = {i + 1: i for i in range(K)}                  # the BDD map: category id -> contiguous class
T = np.array([[1.0, 0, 0, 0], [0, 1.0, 0, 0], [-1.0, 0, 1.0, 0], [0, -1.0, 0, 1.0]])


def detection_set(n_m: int = 300, n_fp: int = 100, n_images: int = 40, seed: int = 36):
    """-> (predicted, gt, links): result dicts, a COCO ground-truth dict, links[i] = the annotation index of predicted[i]'s ground truth
    or -1 for a false positive.  A result file can carry labels only as one-hot rows (matched) and zero rows (false positives), so a
    detection has ONE active class whose logit is over-confident by the fixture's factor 2 (label ~ Bernoulli(sigmoid(x / 2))): label 1 makes
    it a matched detection of that class, label 0 a false positive.  The other columns score below the clamp.  Box residuals and sigmas
    are the fixture's."""
    fx = ref.fixture(n_m, n_fp, K, seed)
    rng = fx["rng"]
    pool = 8 * (n_m + n_fp)
    x = rng.normal(-2.0, 3.0, size=(pool, K)) - 20.0           # the inactive columns: scores below the clamp, never a positive label
    active = rng.integers(0, K, size=pool)
    xa = rng.normal(3.0, 3.0, size=pool)                       # N(3, 3^2): three of four labels positive, as 300 / 100 asks
    x[np.arange(pool), active] = xa
    lab = np.zeros(x.shape, dtype=bool)
    lab[np.arange(pool), active] = rng.uniform(size=pool) < 1.0 / (1.0 + np.exp(-xa / 2.0))
    one, none = np.flatnonzero(lab.sum(1) == 1)[:n_m], np.flatnonzero(lab.sum(1) == 0)[:n_fp]
    assert one.size == n_m and none.size == n_fp
    p = (1.0 / (1.0 + np.exp(-x))).astype(np.float32)
    ids = [100 + 3 * i for i in range(n_images)]
    predicted, anns, links = [], [], []
    for r in range(n_m + n_fp):
        matched = r < n_m
        img = ids[r % n_images] if matched else ids[(r - n_m) % n_images]
        slot = r // n_images if matched else (n_m + n_images - 1) // n_images + (r - n_m) // n_images
        x0, y0 = 100.0 + 1200.0 * (slot % 4), 100.0 + 1200.0 * (slot // 4)
        box = np.array([x0, y0, x0 + 800.0, y0 + 800.0])
        row = p[one[r]] if matched else p[none[r - n_m]]
        sigma = fx["sigma"][r] if matched else rng.uniform(1.0, 6.0, size=4)
        mean = box - (fx["resid"][r] if matched else 0.0)
        cov = T @ np.diag(sigma ** 2) @ T.T
        if matched:
            cls = int(np.flatnonzero(lab[one[r]])[0])
            anns.append({"id": len(anns) + 1, "image_id": img, "category_id": cls + 1, "bbox": [x0, y0, 800.0, 800.0], "area": 640000.0, "iscrowd": 0})
        links.append(len(anns) - 1 if matched else -1)
        f32 = lambda v: [float(np.float32(a)) for a in v]
        predicted.append({"image_id": img, "category_id": int(np.argmax(row)) + 1, "bbox": f32([mean[0], mean[1], mean[2] - mean[0], mean[3] - mean[1]]),
                          "score": float(row.max()), "cls_prob": f32(row), "bbox_covar": [f32(c) for c in cov]})
    order = np.argsort([d["image_id"] for d in predicted], kind="stable")          # a result file lists image by image
    predicted, links = [predicted[i] for i in order], [links[i] for i in order]
    gt = {"images": [{"id": i, "width": 5000, "height": 4000} for i in ids], "annotations": anns}
    return predicted, gt, links


def restrict(predicted, gt, links, keep):
    sel = [i for i, d in enumerate(predicted) if d["image_id"] in keep]
    sub = {"images": [im for im in gt["images"] if im["id"] in keep], "annotations": gt["annotations"]}
    return [predicted[i] for i in sel], sub, [links[i] for i in sel]


def partitions(predicted, gt, links):
    """The dict match_predictions_to_groundtruth returns on a detection_set, from the links alone (CPU tensors): every matched detection a
    true positive beside its ground truth, no duplicates, the rest false positives (the row order inside a partition is the detections':
    no metric depends on it)."""
    pred = ev.eval_predictions_preprocess(predicted, 0.0, device="cpu")
    seen, at = {}, []
    for d in predicted:
        at.append((d["image_id"], seen.get(d["image_id"], 0)))
        seen[d["image_id"]] = at[-1][1] + 1
    pick = lambda name, i: pred[name][at[i][0]][at[i][1]]
    tp = [i for i, l in enumerate(links) if l >= 0]
    fp = [i for i, l in enumerate(links) if l < 0]
    stack = lambda name, rows, shape: torch.stack([pick(name, i) for i in rows]) if rows else torch.zeros(shape)
    part = lambda rows: {"predicted_box_means": stack("predicted_boxes", rows, (0, 4)), "predicted_box_covariances": stack("predicted_covar_mats", rows, (0, 4, 4)),
                         "predicted_cls_probs": stack("predicted_cls_probs", rows, (0, K))}
    t = part(tp)
    boxes = np.array([gt["annotations"][links[i]]["bbox"] for i in tp], dtype=np.float64).reshape(-1, 4)
    boxes[:, 2:] += boxes[:, :2]                                                   # XYWH -> XYXY, as eval_gt_preprocess
    t["gt_box_means"] = torch.from_numpy(boxes).to(torch.float32)
    t["gt_cat_idxs"] = torch.tensor([[float(gt["annotations"][links[i]]["category_id"])] for i in tp], dtype=torch.float32).reshape(-1, 1)
    d = part([])
    d["gt_box_means"], d["gt_cat_idxs"] = torch.zeros((0, 4)), torch.zeros((0, 1))
    return {"true_positives": t, "duplicates": d, "false_positives": part(fp), "false_negatives": {"gt_box_means": torch.zeros((0, 4)), "gt_cat_idxs": torch.zeros((0, 1))}}


def host_fit(matched, reg: str = "moment"):
    """The restatement's fit on a partition dict -> (beta, scales (1, 4))."""
    tp, fp = matched["true_positives"], matched["false_positives"]
    conv = np.array([CMAP[int(c)] for c in tp["gt_cat_idxs"].reshape(-1).tolist()], dtype=np.int64)
    probs = np.concatenate([tp["predicted_cls_probs"].numpy(), fp["predicted_cls_probs"].numpy()])
    onehot = np.zeros(probs.shape, dtype=np.uint8)
    onehot[np.arange(conv.size), conv] = 1
    beta, _ = ref.fit_temperature(probs.reshape(-1), onehot.reshape(-1))
    z, seg, _ = ref.reg_z(tp["predicted_box_means"].numpy(), tp["predicted_box_covariances"].numpy(), tp["gt_box_means"].numpy())
    zg, seg_off = ref.group(z, seg, 4)
    if reg == "moment":
        scales = ref.moment_scales(*ref.moment(zg, seg_off))
    else:
        grid = ref.grid_scales()
        scales = [grid[j] for j in ref.ece_fit(zg, seg_off)[1]]
    return beta, [scales]


def host_apply(predicted, beta, scales):
    """The restatement's apply on result dicts (packed and unpacked as apply_to_results does)."""
    rec, counts, k, place = rc.pack_results(predicted)
    out = ref.apply_records(rec.numpy(), counts.numpy(), k, beta, scales)
    res = []
    for inst, (r, s) in zip(predicted, place):
        row = out[r, s].tolist()
        res.append(dict(inst, score=row[4], cls_prob=row[6:6 + k], bbox_covar=[row[6 + k + 4 * a:6 + k + 4 * a + 4] for a in range(4)]))
    return res


def measure(matched):
    """(reg expected calibration error, cls marginal calibration error) by the package's host function."""
    torch.manual_seed(0)
    res = cce.calibration_errors(matched, dict(CMAP))
    return res["reg_expected_calibration_error"], res["cls_marginal_calibration_error"]


def host_ratios(reg: str = "moment", n_m: int = 300, n_fp: int = 100):
    """Fit on fold 0/2 with the restatement, apply to the complement, measure before / after: ((ece_before, ece_after), (mce_before, mce_after))."""
    predicted, gt, links = detection_set(n_m, n_fp)
    ids = [im["id"] for im in gt["images"]]
    fit_part = restrict(predicted, gt, links, rc.fold_image_ids(ids, 0, 2))
    test_part = restrict(predicted, gt, links, rc.fold_image_ids(ids, 0, 2, complement=True))
    beta, scales = host_fit(partitions(*fit_part), reg)
    before = measure(partitions(*test_part))
    after = measure(partitions(host_apply(test_part[0], beta, scales), test_part[1], test_part[2]))
    return (before[0], after[0]), (before[1], after[1]), beta, scales


if __name__ == "__main__":
    for reg in ("moment", "ece"):
        ece, mce, beta, scales = host_ratios(reg)
        print("%s: beta %.4f scales %s | reg ECE %.5f -> %.5f (x%.2f) | cls MCE %.5f -> %.5f (x%.2f)"
              % (reg, beta, [round(s, 4) for s in scales[0]], ece[0], ece[1], ece[0] / ece[1], mce[0], mce[1], mce[0] / mce[1]))
