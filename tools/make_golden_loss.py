"""Writes tests/golden/train_loss_r1161.npz: the reference's own training losses on a small two-image problem.

    python tools/make_golden_loss.py [--out tests/golden/train_loss_r1161.npz]

The reference module `probabilistic_modeling.probabilistic_retinanet` is imported where it lies (oracle/refimport.py) and its
`ProbabilisticRetinaNet.losses` (PR:168-333) is called UNBOUND on a small attribute holder carrying what `losses` reads.  Three names of the
imported module are replaced for the call: `sigmoid_focal_loss_jit` and `smooth_l1_loss` (fvcore is absent; the stand-in raises) by fvcore's
public definitions restated below, and `get_event_storage` by a sink.  The normals `Normal.rsample` draws (PR:245-246) come from a seeded
numpy Philox stream and are recorded, as oracle/make_golden.py records PI:289-297's.  The anchor labels (detectron2 RetinaNet.label_anchors,
not part of the reference tree) are restated here with the stand-in's pairwise_iou.

The file holds arrays and JSON metadata only: the inputs in the reference's (N, R, C) layout, anchors, ground truth, labels, the
recorded normals and, per case, both losses and the moving normaliser.  Inputs are fp32 values; the reference runs on their fp64 copies.
"""
import argparse
import importlib
import json
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle.refimport import load_reference  # noqa: E402
from pod_compare_amd import anchors as _anchors, synthetic  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "train_loss_r1161.npz")
FRAME = (64, 96)
NUM_CLASSES, NUM_SAMPLES, ANNEALING_STEP = 7, 3, 80000
GT_BOXES = [[10, 8, 44, 40], [50, 20, 90, 60], [2, 2, 14, 10], [30, 30, 36, 62], [10, 8, 44, 40]]
GT_CLASSES = [0, 3, 6, 2, 5]
SEED, EPS_SEED = 2101, 2102
CASES = (("plain", False, 0), ("var_step0", True, 0), ("var_mid", True, ANNEALING_STEP // 2), ("var_annealed", True, ANNEALING_STEP))


def sigmoid_focal_loss(inputs, targets, alpha=-1, gamma=2, reduction="none"):
    """fvcore.nn.sigmoid_focal_loss (public definition)."""
    p = torch.sigmoid(inputs)
    ce_loss = F.binary_cross_entropy_with_logits(inputs, targets, reduction="none")
    p_t = p * targets + (1 - p) * (1 - targets)
    loss = ce_loss * ((1 - p_t) ** gamma)
    if alpha >= 0:
        loss = (alpha * targets + (1 - alpha) * (1 - targets)) * loss
    return loss.mean() if reduction == "mean" else loss.sum() if reduction == "sum" else loss


def smooth_l1_loss(input, target, beta, reduction="none"):
    """fvcore.nn.smooth_l1_loss (public definition)."""
    if beta < 1e-5:
        loss = torch.abs(input - target)
    else:
        n = torch.abs(input - target)
        loss = torch.where(n < beta, 0.5 * n ** 2 / beta, n - 0.5 * beta)
    return loss.mean() if reduction == "mean" else loss.sum() if reduction == "sum" else loss


def label_anchors(anchors, gt_boxes, gt_classes, num_classes, thresholds=(0.4, 0.5)):
    """detectron2 RetinaNet.label_anchors + Matcher(thresholds, [0, -1, 1], allow_low_quality_matches=True) for one image (public
    behaviour).  Returns (labels int64 (R,), matched box index (R,), matched boxes (R, 4))."""
    from detectron2.structures import Boxes, pairwise_iou
    if len(gt_boxes) == 0:
        r = anchors.shape[0]
        return torch.full((r,), num_classes, dtype=torch.int64), torch.zeros(r, dtype=torch.int64), torch.zeros_like(anchors)
    q = pairwise_iou(Boxes(gt_boxes), Boxes(anchors))
    vals, idx = q.max(dim=0)
    match = torch.zeros_like(idx)
    match[(vals >= thresholds[0]) & (vals < thresholds[1])] = -1
    match[vals >= thresholds[1]] = 1
    best, _ = q.max(dim=1)
    match[torch.nonzero(q == best[:, None])[:, 1]] = 1
    labels = gt_classes[idx].clone()
    labels[match == 0] = num_classes
    labels[match == -1] = -1
    return labels, idx, gt_boxes[idx]


def make_inputs():
    shapes = _anchors.level_shapes(*_anchors.padded_size(*FRAME))
    anchors = _anchors.grid_anchors(shapes)
    r = sum(a.shape[0] for a in anchors)
    rng = synthetic.SeededNormals(SEED)
    n = 2
    return shapes, anchors, dict(cls=rng.randn(n, r, NUM_CLASSES) * 2.0 - 2.0, delta=rng.randn(n, r, 4) * 0.5,
                                 cls_var=rng.randn(n, r, NUM_CLASSES) - 1.0, reg_var=rng.randn(n, r, 4) * 4.0)


def build():
    load_reference()
    pr = importlib.import_module("probabilistic_modeling.probabilistic_retinanet")
    from detectron2.modeling.box_regression import Box2BoxTransform
    from detectron2.structures import Boxes
    shapes, anchors, x = make_inputs()
    flat = torch.cat(anchors)
    gts = [(torch.tensor(GT_BOXES, dtype=torch.float32), torch.tensor(GT_CLASSES, dtype=torch.int64)),
           (torch.zeros((0, 4)), torch.zeros((0,), dtype=torch.int64))]
    lab = [label_anchors(flat, b, c, NUM_CLASSES) for b, c in gts]
    labels = torch.stack([l[0] for l in lab])
    matched_boxes = [l[2].double() for l in lab]

    eps_src = synthetic.SeededNormals(EPS_SEED)
    eps_log = []

    def std_normal(shape, dtype, device):
        t = eps_src(shape)
        eps_log.append(t)
        return t.to(dtype)

    import torch.distributions.normal as normal_mod
    saved = (pr.sigmoid_focal_loss_jit, pr.smooth_l1_loss, pr.get_event_storage, normal_mod._standard_normal)
    pr.sigmoid_focal_loss_jit, pr.smooth_l1_loss = sigmoid_focal_loss, smooth_l1_loss
    pr.get_event_storage = lambda: SimpleNamespace(put_scalar=lambda *a, **k: None)
    normal_mod._standard_normal = std_normal
    out = {"anchors": flat.numpy(), "gt_boxes": gts[0][0].numpy(), "gt_classes": gts[0][1].numpy().astype(np.int32),
           "labels": labels.numpy().astype(np.int32), "matched_gt": torch.stack([l[1] for l in lab]).numpy().astype(np.int32)}
    for k, v in x.items():
        out[k] = v.numpy()
    cases = {}
    try:
        for name, var, step in CASES:
            eps_src = synthetic.SeededNormals(EPS_SEED)          # every case replays the same stream
            first = len(eps_log)
            holder = SimpleNamespace(num_classes=NUM_CLASSES, box2box_transform=Box2BoxTransform(weights=(1.0, 1.0, 1.0, 1.0)),
                                     loss_normalizer=100, loss_normalizer_momentum=0.9, focal_loss_alpha=0.25, focal_loss_gamma=2.0,
                                     smooth_l1_beta=0.0, compute_cls_var=var, cls_var_loss="loss_attenuation" if var else "none",
                                     cls_var_num_samples=NUM_SAMPLES, compute_bbox_cov=var,
                                     bbox_cov_loss="negative_log_likelihood" if var else "none", bbox_cov_type="diagonal",
                                     current_step=step, annealing_step=ANNEALING_STEP)
            with torch.no_grad():
                res = pr.ProbabilisticRetinaNet.losses(holder, [Boxes(a) for a in anchors], list(labels), matched_boxes,
                                                       [x["cls"].double()], [x["delta"].double()],
                                                       [x["cls_var"].double()] if var else None, [x["reg_var"].double()] if var else None)
            drawn = eps_log[first:]
            assert len(drawn) == (1 if var else 0), len(drawn)
            if var:
                if "eps" in out:
                    assert np.array_equal(out["eps"], drawn[0].numpy())
                out["eps"] = drawn[0].numpy()                     # (S, valid anchors, K): the reference's compact layout
            out["loss_cls_" + name] = np.float64(res["loss_cls"])
            out["loss_box_reg_" + name] = np.float64(res["loss_box_reg"])
            cases[name] = dict(variance_heads=var, current_step=step, loss_normalizer=float(holder.loss_normalizer))
    finally:
        pr.sigmoid_focal_loss_jit, pr.smooth_l1_loss, pr.get_event_storage, normal_mod._standard_normal = saved
    meta = dict(kind="train_loss", frame=list(FRAME), shapes=[list(s) for s in shapes], num_classes=NUM_CLASSES, num_anchors=9,
                cls_var_num_samples=NUM_SAMPLES, annealing_step=ANNEALING_STEP, focal_loss_alpha=0.25, focal_loss_gamma=2.0,
                smooth_l1_beta=0.0, box_reg_weights=[1.0, 1.0, 1.0, 1.0], initial_loss_normalizer=100.0, loss_normalizer_momentum=0.9,
                seed=SEED, eps_seed=EPS_SEED, cases=cases)
    out["meta"] = np.array(json.dumps(meta, sort_keys=True))
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=OUT)
    args = ap.parse_args(argv)
    arrays = build()
    np.savez_compressed(args.out, **arrays)
    print(args.out, os.path.getsize(args.out), "bytes", len(arrays), "arrays")


if __name__ == "__main__":
    main()
