"""Host side of the calibration pass (csrc/k18_calibration.hip, C ABI pod_calib_*): compute_calibration_errors.calibration_errors
(CE:86-297) with its O(detections) work on the GPU.

The kernels compute the per-detection keys (classification entropy, MVN entropy), the regression cdf bin counts, the
minimum-uncertainty errors and the marginal calibration error's sorted bins; the host keeps the O(classes x 4 x 14) tail with the
host function's own torch expressions, and draws the randperms on the CPU generator in the host function's order (cls then reg,
class by class), so a seeded run shuffles identically.  No CPU fallback: a missing library raises.
"""
import ctypes
from typing import Dict

import numpy as np
import torch

from . import hip

_STEP = 1 / 15.0


def _edges():
    """CE:253-256: the `i + step` of `for i in torch.arange(0.0, 1.0 - step, step)`, fp32 0-d tensors, in loop order."""
    return [i + _STEP for i in torch.arange(0.0, 1.0 - _STEP, _STEP)]


def marginal_calibration_error_gpu(scores: torch.Tensor, labels: torch.Tensor, num_bins: int = 15) -> float:
    """compute_calibration_errors.marginal_calibration_error on the GPU.  scores: device fp32 in [0, 1], labels: device int64 in {0, 1},
    equally many.  Sorted scores, their distinct count (the host chooses the discrete path below n / 4), bin starts, per-bin fp64 sums
    and the debiased L2 terms in bin order on the device; the host computes the <= 15 equal-mass edges from the 28 sorted values
    they depend on, with the restatement's numpy expressions."""
    lib = hip.load()
    scores = scores.reshape(-1).to(torch.float32).contiguous()
    labels = labels.reshape(-1).to(torch.int64).contiguous()
    n = int(scores.numel())
    if n == 0 or labels.numel() != n:
        raise ValueError("probs and labels: equally many, at least one")
    if n >= 2 ** 31:
        raise ValueError("more than 2^31 - 1 scores")
    dev = scores.device
    stream = hip.current_stream()
    P = hip.ptr
    ws = torch.empty(max(int(lib.pod_calib_marginal_sort_workspace_bytes(n)), 1), dtype=torch.uint8, device=dev)
    srt = torch.empty(n, dtype=torch.float64, device=dev)
    order = torch.empty(n, dtype=torch.int32, device=dev)
    hip.check(lib.pod_calib_marginal_sort(P(scores), n, P(ws), P(srt), P(order), stream), "pod_calib_marginal_sort")
    n_blk = -(-n // hip.POD_CALIB_BLOCK)
    blk_cnt = torch.empty(n_blk, dtype=torch.int32, device=dev)
    hip.check(lib.pod_calib_marginal_bins(P(srt), n, None, 0, P(blk_cnt), stream), "pod_calib_marginal_bins")
    cnt = blk_cnt.cpu().numpy().astype(np.int64)
    if int(cnt.sum()) < n / 4.0:                                        # discrete scores: one bin per value
        edges = np.zeros(0, dtype=np.float64)
    else:
        nb = min(num_bins, n)
        each, extras = divmod(n, nb)                                    # np.array_split's section sizes
        div = np.cumsum([0] + extras * [each + 1] + (nb - extras) * [each])
        at = torch.as_tensor(np.stack([div[1:-1] - 1, div[1:-1]], 1).reshape(-1), dtype=torch.int64, device=dev)
        v = srt[at].cpu().numpy().reshape(-1, 2)
        edges = [(v[i, 0] + v[i, 1]) / 2.0 for i in range(nb - 1)] + [1.0]
        edges = np.array(sorted(set(edges)), dtype=np.float64)
        e = (ctypes.c_double * len(edges))(*edges.tolist())
        hip.check(lib.pod_calib_marginal_bins(P(srt), n, e, len(edges), P(blk_cnt), stream), "pod_calib_marginal_bins")
        cnt = blk_cnt.cpu().numpy().astype(np.int64)
    n_bins = int(cnt.sum())
    blk_off = torch.as_tensor(np.concatenate([[0], np.cumsum(cnt)[:-1]]), dtype=torch.int64, device=dev)
    ws2 = torch.empty(max(int(lib.pod_calib_marginal_error_workspace_bytes(n_bins)), 1), dtype=torch.uint8, device=dev)
    total = torch.empty(1, dtype=torch.float64, device=dev)
    e = (ctypes.c_double * max(len(edges), 1))(*edges.tolist())
    hip.check(lib.pod_calib_marginal_error(P(srt), P(order), P(labels), n, e if len(edges) else None, len(edges), P(blk_off), n_bins, P(ws2),
                                           P(total), stream), "pod_calib_marginal_error")
    return float(max(float(total.item()), 0.0) ** 0.5)


def calibration_errors_gpu(matched: dict, cat_mapping_dict: Dict[int, int], marginal_fn=None) -> dict:
    """compute_calibration_errors.calibration_errors (CE:86-297) with the calibration pass on the GPU: the same dict, the same
    randperm draws.  marginal_fn=None: the marginal calibration error on the GPU (marginal_calibration_error_gpu); else
    `marginal_fn(probs, labels)` on the host arrays, as the host function calls it."""
    return calibration_pass(matched, cat_mapping_dict, marginal_fn)[0]


def calibration_pass(matched: dict, cat_mapping_dict: Dict[int, int], marginal_fn=None):
    """(calibration_errors_gpu's dict, per-class details): {"cls_min_u", "reg_min_u": [class] fp64, "counts": [class][4][14] the
    "cdf < edge" counts, "totals": [class][4], "reg_ece", "reg_mce": [class][4] fp32} in the map's class order."""
    lib = hip.load()
    dev = torch.device("cuda", torch.cuda.current_device())
    parts = {k: matched[k] for k in ("true_positives", "duplicates", "false_positives")}
    tp, dup, fp = parts["true_positives"], parts["duplicates"], parts["false_positives"]
    f32 = lambda t, *shape: t.to(dev, torch.float32).reshape(*shape)
    k1 = int(tp["predicted_cls_probs"].shape[1])
    values = [int(c) for c in cat_mapping_dict.values()]
    if any(c < 0 or c >= hip.POD_MAX_CLASSES for c in values) or k1 < 2:
        raise ValueError("contiguous class ids must lie in [0, {}) and the scores need a background column".format(hip.POD_MAX_CLASSES))
    n_tp, n_dup, n_fp = (int(p["predicted_cls_probs"].shape[0]) for p in (tp, dup, fp))
    n_m, n = n_tp + n_dup, n_tp + n_dup + n_fp
    gt_ids = torch.cat((tp["gt_cat_idxs"].reshape(-1), dup["gt_cat_idxs"].reshape(-1))).to(dev)
    ids = [int(c) for c in torch.unique(gt_ids.long()).tolist()]
    for c in ids:                                                                                     # CE:86-103 (KeyError as the host)
        cat_mapping_dict[c]
    lut = torch.zeros(max(ids + [0]) + 1, dtype=torch.int64, device=dev)
    for c in ids:
        lut[c] = int(cat_mapping_dict[c])
    conv = lut[gt_ids.long()] if n_m else torch.zeros(0, dtype=torch.int64, device=dev)
    probs = torch.cat((f32(tp["predicted_cls_probs"], -1, k1), f32(dup["predicted_cls_probs"], -1, k1), f32(fp["predicted_cls_probs"], -1, k1))).contiguous()
    cov = torch.cat([f32(p["predicted_box_covariances"], -1, 4, 4) for p in (tp, dup, fp)]).contiguous()
    means = torch.cat([f32(p["predicted_box_means"], -1, 4) for p in (tp, dup)]).contiguous()
    gt = torch.cat([f32(p["gt_box_means"], -1, 4) for p in (tp, dup)]).contiguous()

    scores = probs.reshape(-1)                                                                        # CE:117-131
    onehot = torch.cat((torch.nn.functional.one_hot(conv, k1).reshape(-1), torch.zeros(n_fp * k1, dtype=torch.int64, device=dev)))
    out = {"cls_marginal_inputs": (scores.cpu().numpy(), onehot.cpu().numpy())}
    if marginal_fn is None:
        out["cls_marginal_calibration_error"] = marginal_calibration_error_gpu(scores, onehot)
    else:
        out["cls_marginal_calibration_error"] = float(marginal_fn(*out["cls_marginal_inputs"]))
    out = {"cls_marginal_calibration_error": out["cls_marginal_calibration_error"], "cls_marginal_inputs": out["cls_marginal_inputs"]}

    stream = hip.current_stream()
    P = hip.ptr
    gt_class = conv.to(torch.int32).contiguous()
    cls_ent = torch.empty(max(n, 1), dtype=torch.float32, device=dev)
    reg_ent = torch.empty(max(n, 1), dtype=torch.float32, device=dev)
    det_class = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
    class_count = torch.empty(hip.POD_MAX_CLASSES, dtype=torch.int32, device=dev)
    hip.check(lib.pod_calib_keys(P(probs), k1, P(cov), P(gt_class), n_m, n, P(cls_ent), P(reg_ent), P(det_class), P(class_count), stream),
              "pod_calib_keys")
    edges = _edges()
    e = (ctypes.c_float * len(edges))(*[float(x) for x in edges])
    counts = torch.empty((hip.POD_MAX_CLASSES, 4, len(edges) + 1), dtype=torch.int32, device=dev)
    hip.check(lib.pod_calib_reg_counts(P(means), P(cov), P(gt), P(det_class), n_m, e, len(edges), P(counts), stream), "pod_calib_reg_counts")

    per_class = class_count.cpu().numpy().astype(np.int64)
    class_off = torch.as_tensor(np.concatenate([[0], np.cumsum(per_class)[:-1]]), dtype=torch.int32, device=dev)
    perms, seg_class, sizes = [], [], []
    for c in values:                                                                                  # the host function's draw order
        for which in (0, 1):                                                                          # cls, then reg
            perms.append(torch.randperm(int(per_class[c])))
            seg_class.append(2 * c + which)
            sizes.append(int(per_class[c]))
    seg_off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    n_pos, max_seg = int(seg_off[-1]), max(sizes + [0])
    perm = torch.cat(perms).to(dev, torch.int64) if n_pos else torch.zeros(1, dtype=torch.int64, device=dev)
    min_err = torch.empty(max(len(sizes), 1), dtype=torch.float64, device=dev)
    ws = torch.empty(max(int(lib.pod_calib_min_uncertainty_workspace_bytes(n, n_pos)), 1), dtype=torch.uint8, device=dev)
    t_seg_off = torch.as_tensor(seg_off, device=dev)
    t_seg_class = torch.as_tensor(seg_class, dtype=torch.int32, device=dev)
    hip.check(lib.pod_calib_min_uncertainty(P(cls_ent), P(reg_ent), P(det_class), n, n_tp, P(class_off), P(t_seg_off), P(t_seg_class), len(sizes),
                                            max_seg, n_pos, P(perm), P(ws), P(min_err), stream), "pod_calib_min_uncertainty")
    min_err = min_err.cpu()
    hist = counts.cpu().to(torch.int64).cumsum(2)                                                     # "cdf < edge i" = bins 0 .. i
    cls_min_u, reg_min_u, reg_ece, reg_mce = [], [], [], []
    for j, c in enumerate(values):                                                                    # CE:206-261's tail, the host's expressions
        cls_min_u.append(min_err[2 * j].double())
        reg_min_u.append(min_err[2 * j + 1].double())
        ece_c, mce_c = [], []
        for d in range(4):
            m = int(hist[c, d, -1])
            errs = []
            for i, edge in enumerate(edges):
                frac = torch.tensor(float(hist[c, d, i]), dtype=torch.float32) / m
                errs.append((frac - edge) ** 2)
            errs = torch.stack(errs)
            mce_c.append(errs.max())
            ece_c.append(errs.mean())
        reg_mce.append(torch.stack(mce_c))
        reg_ece.append(torch.stack(ece_c))

    def nanmean(ts):
        t = torch.stack(ts, 0).double()
        return float(t[~torch.isnan(t)].mean())
    out.update({"reg_expected_calibration_error": nanmean(reg_ece), "reg_maximum_calibration_error": nanmean(reg_mce),
                "cls_minimum_uncertainty_error": nanmean(cls_min_u), "reg_minimum_uncertainty_error": nanmean(reg_min_u)})
    details = {"cls_min_u": torch.stack(cls_min_u).numpy(), "reg_min_u": torch.stack(reg_min_u).numpy(),
               "counts": hist[values][:, :, :-1].numpy(), "totals": hist[values][:, :, -1].numpy(),
               "reg_ece": torch.stack(reg_ece).numpy(), "reg_mce": torch.stack(reg_mce).numpy()}
    return out, details


def keys_gpu(matched: dict, cat_mapping_dict: Dict[int, int]):
    """The per-detection keys of pod_calib_keys for the rows (true positives, duplicates, false positives): (cls_entropy, reg_entropy,
    det_class) as CPU tensors -- for tests that hold the GPU's own keys against the host formula."""
    lib = hip.load()
    dev = torch.device("cuda", torch.cuda.current_device())
    tp, dup, fp = matched["true_positives"], matched["duplicates"], matched["false_positives"]
    k1 = int(tp["predicted_cls_probs"].shape[1])
    conv = torch.as_tensor([cat_mapping_dict[int(c)] for c in torch.cat((tp["gt_cat_idxs"].reshape(-1), dup["gt_cat_idxs"].reshape(-1))).tolist()],
                           dtype=torch.int32, device=dev)
    probs = torch.cat([p["predicted_cls_probs"].to(dev, torch.float32).reshape(-1, k1) for p in (tp, dup, fp)]).contiguous()
    cov = torch.cat([p["predicted_box_covariances"].to(dev, torch.float32).reshape(-1, 4, 4) for p in (tp, dup, fp)]).contiguous()
    n_m, n = int(conv.numel()), int(probs.shape[0])
    cls_ent = torch.empty(max(n, 1), dtype=torch.float32, device=dev)
    reg_ent = torch.empty(max(n, 1), dtype=torch.float32, device=dev)
    det_class = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
    class_count = torch.empty(hip.POD_MAX_CLASSES, dtype=torch.int32, device=dev)
    P = hip.ptr
    hip.check(lib.pod_calib_keys(P(probs), k1, P(cov), P(conv), n_m, n, P(cls_ent), P(reg_ent), P(det_class), P(class_count),
                                 hip.current_stream()), "pod_calib_keys")
    return cls_ent[:n].cpu(), reg_ent[:n].cpu(), det_class[:n].cpu()
