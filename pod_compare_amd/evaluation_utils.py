"""Ground-truth matching and proper scoring rules on the GPU, with the reference's names.

Mirrors core/evaluation_tools/evaluation_utils.py (EU) `match_predictions_to_groundtruth` and
core/evaluation_tools/scoring_rules.py (SR) `compute_reg_scores`, `compute_reg_scores_fn`,
`retinanet_compute_cls_scores`: same arguments (dicts keyed by image id), same nested result dict of tensors, same
row order (prediction-dict key order, then ground-truth order, true positive = highest max class probability).
The reference re-concatenates its result tensors inside a Python loop over every ground-truth box (EU:222-360);
here one kernel launch labels the whole data set and the partitions are gathered with index tensors on the device.

Beside the reference's rules: `reg_proper_scores` (energy score and CRPS per row, kernel pod_reg_scores, K33) and `brier_rows` -- bounded
proper scoring rules scoring_rules.py does not define.  A partition that carries their per-row tensors ("energy_score", "crps",
"brier_score") gets their means under the mask from `compute_reg_scores` / `retinanet_compute_cls_scores`; one that does not gets what
the reference returns.

`pdq_scores` (with `pdq_pair_quality` and `pdq_assign` under it) is PDQ, the probability-based detection quality, on the kernels of K34
(include/pod_mi355x.h has the definition): the metric the reference's README leaves to a separate CPU tool.
"""
import math
from typing import Dict

import torch

from . import hip

MATCH_MAX_DET = 128


def match_predictions_to_groundtruth(predicted_box_means: Dict, predicted_cls_probs: Dict, predicted_box_covariances: Dict,
                                     gt_box_means: Dict, gt_cat_idxs: Dict, iou_min: float = 0.1, iou_correct: float = 0.7,
                                     device="cuda"):
    """EU:191-367."""
    lib = hip.load()
    dev = torch.device(device)
    keys = list(predicted_box_means.keys())
    f = lambda t: t.to(dev, torch.float32)
    k = next(iter(predicted_cls_probs.values())).shape[1] if keys else 0          # no prediction: empty (0, 0) probabilities, as the oracle's
    pb = torch.cat([f(predicted_box_means[i]).reshape(-1, 4) for i in keys]) if keys else torch.zeros((0, 4), device=dev)
    pp = torch.cat([f(predicted_cls_probs[i]).reshape(-1, k) for i in keys]) if keys else torch.zeros((0, k), device=dev)
    pc = torch.cat([f(predicted_box_covariances[i]).reshape(-1, 4, 4) for i in keys]) if keys else torch.zeros((0, 4, 4), device=dev)
    nd = [int(predicted_box_means[i].shape[0]) for i in keys]
    ng = [int(gt_box_means[i].shape[0]) if i in gt_box_means else 0 for i in keys]
    if any(n > MATCH_MAX_DET for n in nd):
        raise hip.PodError("more than {} detections in one image".format(MATCH_MAX_DET))
    has_gt = [i for i in keys if i in gt_box_means]
    gb = torch.cat([f(gt_box_means[i]).reshape(-1, 4) for i in has_gt]) if has_gt else torch.zeros((0, 4), device=dev)
    gc = torch.cat([f(gt_cat_idxs[i]).reshape(-1, 1) for i in has_gt]) if has_gt else torch.zeros((0, 1), device=dev)
    i32 = lambda x: torch.tensor(x, dtype=torch.int32, device=dev)
    det_off = i32([0] + torch.tensor(nd).cumsum(0).tolist() if nd else [0])
    gt_off = i32([0] + torch.tensor(ng).cumsum(0).tolist() if ng else [0])
    det_img = torch.repeat_interleave(torch.arange(len(keys), dtype=torch.int32, device=dev), i32(nd).long()) if nd else i32([])
    gt_img = torch.repeat_interleave(torch.arange(len(keys), dtype=torch.int32, device=dev), i32(ng).long()) if ng else i32([])
    D, G = int(pb.shape[0]), int(gb.shape[0])
    gt_fn = torch.zeros(max(G, 1), dtype=torch.int32, device=dev)
    cnt = torch.zeros(max(G, 1), dtype=torch.int32, device=dev)
    midx = torch.zeros((max(G, 1), MATCH_MAX_DET), dtype=torch.int32, device=dev)
    miou = torch.zeros((max(G, 1), MATCH_MAX_DET), dtype=torch.float32, device=dev)
    det_fp = torch.zeros(max(D, 1), dtype=torch.int32, device=dev)
    P = hip.ptr
    pb, pp, gb = pb.contiguous(), pp.contiguous(), gb.contiguous()
    hip.check(lib.pod_match_groundtruth(P(pb), P(pp), P(det_off), P(det_img.contiguous()), D, P(gb), P(gt_off), P(gt_img.contiguous()), G,
                                        max(k, 1), float(iou_min), float(iou_correct), P(gt_fn), P(cnt), P(midx), P(miou), P(det_fp),
                                        hip.current_stream()), "pod_match_groundtruth")
    gt_fn, cnt, midx, miou, det_fp = gt_fn[:G], cnt[:G], midx[:G], miou[:G], det_fp[:D]
    rank = torch.arange(MATCH_MAX_DET, device=dev)[None, :]
    tp_g = (cnt > 0).nonzero().squeeze(1)
    tp_d = midx[tp_g, 0].long()
    dup_mask = (rank >= 1) & (rank < cnt[:, None])
    dup_g, dup_r = dup_mask.nonzero(as_tuple=True)                    # row-major: ground-truth order, then rank
    dup_d = midx[dup_g, dup_r].long()
    fp_d = det_fp.bool().nonzero().squeeze(1)
    fn_g = gt_fn.bool().nonzero().squeeze(1)
    part = lambda d, g, iou: {"predicted_box_means": pb[d], "predicted_box_covariances": pc[d], "predicted_cls_probs": pp[d],
                              "gt_box_means": gb[g], "gt_cat_idxs": gc[g], "iou_with_ground_truth": iou}
    return {"true_positives": part(tp_d, tp_g, miou[tp_g, 0]),
            "duplicates": part(dup_d, dup_g, miou[dup_g, dup_r]),
            "false_positives": {"predicted_box_means": pb[fp_d], "predicted_box_covariances": pc[fp_d], "predicted_cls_probs": pp[fp_d]},
            "false_negatives": {"gt_box_means": gb[fn_g], "gt_cat_idxs": gc[fn_g]}}


def reg_proper_scores(means: torch.Tensor, covs: torch.Tensor, gt: torch.Tensor, num_samples: int = 1000, seed: int = 0,
                      energy: bool = True, crps: bool = True) -> Dict:
    """Per-row energy score ("energy_score") and CRPS ("crps") of N(mean, cov + 1e-2 I) at the ground truth, fp32, from ONE launch of
    pod_reg_scores (include/pod_mi355x.h, K33; the reference defines neither rule).  Row i draws under (seed, i) alone: a row's score
    depends neither on the number of rows nor on the other rows."""
    n = int(means.shape[0])
    out = {}
    if energy:
        out["energy_score"] = torch.empty(n, dtype=torch.float32, device=means.device)
    if crps:
        out["crps"] = torch.empty(n, dtype=torch.float32, device=means.device)
    if not out:
        raise ValueError("reg_proper_scores: neither rule asked for")
    if n == 0:
        return out
    f = lambda t: t.to(torch.float32).contiguous()
    means, covs, gt = f(means), f(covs), f(gt)
    with torch.cuda.device(means.device):
        hip.check(hip.load().pod_reg_scores(hip.ptr(means), hip.ptr(covs), hip.ptr(gt), n, int(num_samples), int(seed) & 0xFFFFFFFFFFFFFFFF,
                                            None, None, hip.ptr(out.get("energy_score")), hip.ptr(out.get("crps")), hip.current_stream()),
                  "pod_reg_scores")
    return out


def brier_rows(p: torch.Tensor) -> torch.Tensor:
    """Per-row Brier score of the binary vector [p, 1 - p] against [1, 0] -- the multilabel formulation retinanet_compute_cls_scores uses
    for the ignorance score (SR:6-42): (1 - p)^2 + (1 - p)^2."""
    q = 1.0 - p
    return 2.0 * q * q


def _row_score_means(input_matches: Dict, valid_idxs: torch.Tensor, names) -> Dict:
    """Means of the per-row tensors `input_matches` carries, under the mask: fp32 rows, the mean taken in fp64; None on an empty mask."""
    out = {}
    for name in names:
        if name in input_matches:
            rows = input_matches[name][valid_idxs]
            out[name + "_mean"] = float(rows.double().mean()) if rows.shape[0] else None
    return out


def compute_reg_scores(input_matches: Dict, valid_idxs: torch.Tensor) -> Dict:
    """SR:45-81: ignorance (NLL of N(mean, cov + 1e-2 I) at the ground truth, kernel pod_reg_nll) and MSE; and, where the partition carries
    the per-row tensors "energy_score" / "crps" (reg_proper_scores on the WHOLE partition), their means under the mask."""
    means = input_matches["predicted_box_means"][valid_idxs].contiguous()
    covs = input_matches["predicted_box_covariances"][valid_idxs].contiguous()
    gt = input_matches["gt_box_means"][valid_idxs].contiguous()
    extra = _row_score_means(input_matches, valid_idxs, ("energy_score", "crps"))
    if means.shape[0] == 0:
        return dict({"ignorance_score_mean": None, "mean_squared_error": None}, **extra)
    lib = hip.load()
    nll = torch.empty(means.shape[0], dtype=torch.float32, device=means.device)
    hip.check(lib.pod_reg_nll(hip.ptr(means), hip.ptr(covs), hip.ptr(gt), means.shape[0], hip.ptr(nll), hip.current_stream()), "pod_reg_nll")
    return dict({"ignorance_score_mean": float(nll.mean()), "mean_squared_error": float(((means - gt) ** 2).mean())}, **extra)


def compute_reg_scores_fn(false_positives: Dict, valid_idxs: torch.Tensor) -> Dict:
    """SR:84-114: mean differential entropy of N(mean, cov + 1e-2 I) = 0.5 log det(2 pi e Sigma)."""
    covs = false_positives["predicted_box_covariances"][valid_idxs]
    if covs.shape[0] == 0:
        return {"total_entropy_mean": None}
    # Sigma is formed in fp32, as SR:100-101 and pod_reg_nll form it (the sum rounds where a variance is >~ 1e5 * 1e-2), then scored in fp64
    sig = (covs.float() + 1e-2 * torch.eye(4, dtype=torch.float32, device=covs.device)).double()
    ent = 0.5 * torch.logdet(sig) + 2.0 * (1.0 + math.log(2.0 * math.pi))
    return {"total_entropy_mean": float(ent.mean())}


def retinanet_compute_cls_scores(input_matches: Dict, valid_idxs: torch.Tensor) -> Dict:
    """SR:6-42: mean of -log p(correct) in the multilabel formulation."""
    p = input_matches["predicted_score_of_gt_category"][valid_idxs]
    extra = _row_score_means(input_matches, valid_idxs, ("brier_score",))          # where the partition carries brier_rows of its rows
    if p.shape[0] == 0:
        return dict({"ignorance_score_mean": None}, **extra)
    return dict({"ignorance_score_mean": float((-torch.log(p)).mean())}, **extra)


PDQ_P_MIN = 0.0027
PDQ_PLANES = ("pPDQ", "q_spatial", "q_label", "q_fg", "q_bg")


class PdqTables:
    """The host tables of a pod_pdq_* call -- frames (n, 2) = (W, H), detection, ground-truth and pair offsets -- as contiguous CPU tensors,
    and the device workspace the calls copy them into."""

    def __init__(self, frames, det_counts, gt_counts, device):
        n = len(det_counts)
        if len(gt_counts) != n or len(frames) != n:
            raise ValueError("pdq: one frame, one detection count and one ground-truth count per image")
        if any(c > hip.POD_PDQ_MAX_SIDE for c in list(det_counts) + list(gt_counts)):
            raise hip.PodError("more than {} detections or ground truths in one image".format(hip.POD_PDQ_MAX_SIDE))
        cum = lambda xs: torch.tensor([0] + list(xs), dtype=torch.int64).cumsum(0)
        self.n_images = n
        self.frames = torch.tensor([[int(w), int(h)] for w, h in frames], dtype=torch.int32).reshape(n, 2).contiguous()
        self.det_off = cum(det_counts).to(torch.int32).contiguous()
        self.gt_off = cum(gt_counts).to(torch.int32).contiguous()
        self.pair_off = cum([d * g for d, g in zip(det_counts, gt_counts)]).contiguous()
        self.n_det, self.n_gt, self.n_pairs = int(self.det_off[-1]), int(self.gt_off[-1]), int(self.pair_off[-1])
        self.device = torch.device(device)
        self.workspace = torch.empty(max(int(hip.load().pod_pdq_workspace_bytes(n)), 8), dtype=torch.uint8, device=self.device)

    def pair_matrix(self, plane: torch.Tensor, m: int) -> torch.Tensor:
        """Image m's (G, D) view of one plane of n_pairs values."""
        G, D = int(self.gt_off[m + 1] - self.gt_off[m]), int(self.det_off[m + 1] - self.det_off[m])
        return plane[int(self.pair_off[m]):int(self.pair_off[m + 1])].view(G, D)


def pdq_pair_quality(tables: PdqTables, means: torch.Tensor, covs: torch.Tensor, probs: torch.Tensor, gt_boxes: torch.Tensor,
                     gt_classes: torch.Tensor, p_min: float = PDQ_P_MIN, sums: bool = False):
    """pod_pdq_pairs (K34): packed detections (D_total, 4) / (D_total, 4, 4) / (D_total, K) and ground truths (G_total, 4) / int (G_total,)
    on the device -> (quality (5, n_pairs) fp64 in PDQ_PLANES' order, det_invalid (D_total,) int32[, sums (2, n_pairs) fp64])."""
    dev = tables.device
    f = lambda t, shape: t.to(dev, torch.float32).reshape(shape).contiguous()
    K = int(probs.shape[1]) if probs.dim() == 2 and probs.shape[0] else 1
    means, covs, probs, gt_boxes = f(means, (-1, 4)), f(covs, (-1, 4, 4)), f(probs, (-1, K)), f(gt_boxes, (-1, 4))
    gt_classes = gt_classes.to(dev, torch.int32).reshape(-1).contiguous()
    if means.shape[0] != tables.n_det or covs.shape[0] != tables.n_det or probs.shape[0] != tables.n_det or \
            gt_boxes.shape[0] != tables.n_gt or gt_classes.shape[0] != tables.n_gt:
        raise ValueError("pdq: the packed arrays do not have the tables' row counts")
    quality = torch.zeros((5, tables.n_pairs), dtype=torch.float64, device=dev)
    invalid = torch.zeros(tables.n_det, dtype=torch.int32, device=dev)
    s = torch.zeros((2, tables.n_pairs), dtype=torch.float64, device=dev) if sums else None
    P = hip.ptr
    with torch.cuda.device(dev):
        hip.check(hip.load().pod_pdq_pairs(tables.frames.data_ptr(), tables.det_off.data_ptr(), tables.gt_off.data_ptr(), tables.pair_off.data_ptr(),
                                           tables.n_images, P(means), P(covs), P(probs), K, P(gt_boxes), P(gt_classes), float(p_min),
                                           P(tables.workspace), P(quality), P(s), P(invalid), hip.current_stream()), "pod_pdq_pairs")
    return (quality, invalid, s) if sums else (quality, invalid)


def pdq_assign(tables: PdqTables, quality: torch.Tensor):
    """pod_pdq_assign (K34): per image the maximum-weight assignment on plane 0 of `quality` -> (gt_match (G_total,) int32: the detection
    inside its image or -1, counts (n_images, 3) int32 = TP, FP, FN, image_sums (n_images, 5) fp64 over the true positives)."""
    dev = tables.device
    quality = quality.to(dev, torch.float64).contiguous()
    if tuple(quality.shape) != (5, tables.n_pairs):
        raise ValueError("pdq: quality must be the (5, n_pairs) planes of the tables")
    match = torch.full((tables.n_gt,), -1, dtype=torch.int32, device=dev)
    counts = torch.zeros((tables.n_images, 3), dtype=torch.int32, device=dev)
    image_sums = torch.zeros((tables.n_images, 5), dtype=torch.float64, device=dev)
    P = hip.ptr
    with torch.cuda.device(dev):
        hip.check(hip.load().pod_pdq_assign(tables.det_off.data_ptr(), tables.gt_off.data_ptr(), tables.pair_off.data_ptr(), tables.n_images,
                                            P(quality), P(tables.workspace), P(match), P(counts), P(image_sums), hip.current_stream()), "pod_pdq_assign")
    return match, counts, image_sums


def pdq_scores(pred: Dict, gt: Dict, frame_sizes: Dict, cat_mapping: Dict[int, int], p_min: float = PDQ_P_MIN, device="cuda") -> Dict:
    """PDQ of a data set (include/pod_mi355x.h, K34).  pred: what `eval_predictions_preprocess` returns (already filtered by the minimum
    allowed score); gt: what `eval_gt_preprocess` returns; frame_sizes: image id -> (width, height), in the order the images are added
    up; cat_mapping: the ground truth's category id -> the model's contiguous class.  An image on one side only counts (its detections
    are false positives, its ground truths false negatives); one without a frame size raises.  One launch scores every (ground truth,
    detection) pair of the data set, one assigns every image; the totals are added on the host in image order, in fp64.
    -> {"PDQ", "avg_pPDQ", "avg_spatial", "avg_label", "avg_fg", "avg_bg", "TP", "FP", "FN", "invalid_detections", "num_images", "p_min"}."""
    dev = torch.device(device)
    boxes, probs, covs = pred["predicted_boxes"], pred["predicted_cls_probs"], pred["predicted_covar_mats"]
    gboxes, gcats = gt["gt_boxes"], gt["gt_cat_idxs"]
    missing = [i for i in list(boxes) + list(gboxes) if i not in frame_sizes]
    if missing:
        raise ValueError("pdq: no frame size for image {!r}".format(missing[0]))
    ids = [i for i in frame_sizes if i in boxes or i in gboxes]
    nd = [int(boxes[i].shape[0]) if i in boxes else 0 for i in ids]
    ng = [int(gboxes[i].shape[0]) if i in gboxes else 0 for i in ids]
    tables = PdqTables([frame_sizes[i] for i in ids], nd, ng, dev)
    K = next((int(probs[i].shape[1]) for i in ids if i in probs), 1)
    cat = lambda ts, shape: torch.cat([t.to(dev, torch.float32).reshape(shape) for t in ts]) if ts else torch.zeros((0,) + tuple(shape[1:]), device=dev)
    means = cat([boxes[i] for i in ids if i in boxes], (-1, 4))
    cov = cat([covs[i] for i in ids if i in boxes], (-1, 4, 4))
    prob = cat([probs[i] for i in ids if i in boxes], (-1, K))
    gb = cat([gboxes[i] for i in ids if i in gboxes], (-1, 4))
    gc = torch.tensor([cat_mapping[int(c)] for i in ids if i in gboxes for c in gcats[i].reshape(-1).tolist()], dtype=torch.int32, device=dev)
    res = {"PDQ": 0.0, "avg_pPDQ": 0.0, "avg_spatial": 0.0, "avg_label": 0.0, "avg_fg": 0.0, "avg_bg": 0.0, "TP": 0, "FP": sum(nd), "FN": sum(ng),
           "invalid_detections": 0, "num_images": len(ids), "p_min": float(p_min)}
    if not ids:
        return res
    quality, invalid = pdq_pair_quality(tables, means, cov, prob, gb, gc, p_min)
    _, counts, image_sums = pdq_assign(tables, quality)
    tp, fp, fn = (int(v) for v in counts.sum(0).tolist())
    totals = [0.0] * 5
    for row in image_sums.cpu().tolist():          # image order, fp64
        totals = [a + b for a, b in zip(totals, row)]
    res.update({"TP": tp, "FP": fp, "FN": fn, "invalid_detections": int(invalid.sum()), "PDQ": totals[0] / (tp + fp + fn) if tp + fp + fn else 0.0})
    if tp:
        res.update({k: t / tp for k, t in zip(("avg_pPDQ", "avg_spatial", "avg_label", "avg_fg", "avg_bg"), totals)})
    return res


def eval_predictions_preprocess(predicted_instances, min_allowed_score: float = 0.0, is_odd: bool = False, device="cpu"):
    """EU:19-73 (SURVEY f-2, the on-disk result format read back): list of `instances_to_json` dicts -> per-image tensors.
    XYWH boxes back to XYXY; covariances back through T' = [[1,0,0,0],[0,1,0,0],[1,0,1,0],[0,1,0,1]] (the inverse of
    covar_xyxy_to_xywh's T), detections with category_id == -1 (unless `is_odd`) or max cls_prob < min_allowed_score
    dropped.  Vectorised per image instead of one torch.cat per detection."""
    from collections import defaultdict
    rows = defaultdict(list)
    for inst in predicted_instances:
        top = max(inst["cls_prob"])
        if (not is_odd and inst["category_id"] == -1) or top < min_allowed_score:
            continue
        rows[inst["image_id"]].append(inst)
    tinv = torch.tensor([[1.0, 0, 0, 0], [0, 1.0, 0, 0], [1.0, 0, 1.0, 0], [0, 1.0, 0.0, 1.0]], dtype=torch.float64)
    boxes, probs, covs = {}, {}, {}
    for image_id, insts in rows.items():
        b = torch.tensor([i["bbox"] for i in insts], dtype=torch.float64)
        b[:, 2] += b[:, 0]
        b[:, 3] += b[:, 1]
        c = torch.tensor([i["bbox_covar"] for i in insts], dtype=torch.float64)
        boxes[image_id] = b.to(torch.float32).to(device)
        probs[image_id] = torch.tensor([i["cls_prob"] for i in insts], dtype=torch.float32, device=device)
        covs[image_id] = (tinv @ c @ tinv.t()).to(torch.float32).to(device)
    return {"predicted_boxes": boxes, "predicted_cls_probs": probs, "predicted_covar_mats": covs}


def eval_gt_preprocess(gt_instances, device="cpu"):
    """EU:76-92: COCO annotations -> per-image XYXY boxes and (n,1) category ids."""
    from collections import defaultdict
    rows = defaultdict(list)
    for g in gt_instances:
        rows[g["image_id"]].append(g)
    boxes, cats = {}, {}
    for image_id, gs in rows.items():
        b = torch.tensor([g["bbox"] for g in gs], dtype=torch.float64)
        b[:, 2] += b[:, 0]
        b[:, 3] += b[:, 1]
        boxes[image_id] = b.to(torch.float32).to(device)
        cats[image_id] = torch.tensor([[g["category_id"]] for g in gs], dtype=torch.float32, device=device)
    return {"gt_boxes": boxes, "gt_cat_idxs": cats}


def planted_ground_truth(planted_boxes: torch.Tensor, planted_classes: torch.Tensor, image_size, out_size):
    """Planted boxes (network-input pixels, synthetic.planted_head_outputs) as ground truth at the output resolution:
    scaled like the detections (IU:394-403) and clipped to the frame; category ids are class + 1 (BDD ids 1..7)."""
    sx, sy = out_size[1] / image_size[1], out_size[0] / image_size[0]
    b = planted_boxes.to(torch.float32) * torch.tensor([sx, sy, sx, sy], dtype=torch.float32, device=planted_boxes.device)
    b[:, 0::2] = b[:, 0::2].clamp(0.0, float(out_size[1]))
    b[:, 1::2] = b[:, 1::2].clamp(0.0, float(out_size[0]))
    return b, (planted_classes.to(torch.float32) + 1.0).reshape(-1, 1)


def score_against_planted(detections, heads, image_size, out_size, iou_min: float = 0.1, iou_correct: float = 0.7, device="cuda") -> Dict:
    """End-to-end "NLL parity" number of the metric: detections of the path (`DeviceDetections`, one per image) matched to
    the planted ground truth of their inputs (EU:191-367, the offline evaluation's defaults iou_min 0.1 / iou_correct 0.7),
    then SR:68-74 on the true positives.  Returns {"nll", "mse", true_positives, duplicates, false_positives,
    false_negatives}."""
    pb, pp, pc, gb, gc = {}, {}, {}, {}, {}
    for i, (det, h) in enumerate(zip(detections, heads)):
        m = det.count()
        pb[i], pp[i], pc[i] = det.boxes[:m], det.probs[:m], det.cov[:m]
        gb[i], gc[i] = planted_ground_truth(h.planted_boxes, h.planted_classes, image_size, out_size)
    res = match_predictions_to_groundtruth(pb, pp, pc, gb, gc, iou_min, iou_correct, device=device)
    tp = res["true_positives"]
    valid = torch.ones(tp["predicted_box_means"].shape[0], dtype=torch.bool, device=tp["predicted_box_means"].device)
    reg = compute_reg_scores(tp, valid)
    return {"nll": reg["ignorance_score_mean"], "mse": reg["mean_squared_error"],
            "true_positives": int(tp["predicted_box_means"].shape[0]), "duplicates": int(res["duplicates"]["predicted_box_means"].shape[0]),
            "false_positives": int(res["false_positives"]["predicted_box_means"].shape[0]),
            "false_negatives": int(res["false_negatives"]["gt_box_means"].shape[0])}
