"""Times pod_reg_score_loss (K27, both kinds) beside pod_train_loss (K21) at the training shape: 720 x 1280 frames padded for the FPN,
SOLVER.IMS_PER_BATCH = 4, BBOX_COV_LOSS.NUM_SAMPLES = 1000, CLS_VAR_LOSS.NUM_SAMPLES = 10, seeded random head outputs and a seeded
ground-truth set whose positive count is printed.  Every figure is the median over WINDOWS windows of CALLS launches enqueued back to back
from the C entry between two device events (so the device, not Python, sets the pace), after a warm-up window.

    python tools/score_loss_bench.py [--out profiles/score_losses.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pod_compare_amd import anchors as _anchors, hip, losses      # noqa: E402

WINDOWS, CALLS = 10, 20
K, A, S, M, BATCH = 7, 9, 10, 1000, 4


def ground_truth(image: int, h: int, w: int, boxes: int = 12):
    g = torch.Generator().manual_seed(100 + image)
    side = torch.exp(torch.rand(boxes, 2, generator=g) * 2.8 + 3.2)            # 25 .. 400 px
    cx, cy = torch.rand(boxes, generator=g) * w, torch.rand(boxes, generator=g) * h
    b = torch.stack((cx - side[:, 0] / 2, cy - side[:, 1] / 2, cx + side[:, 0] / 2, cy + side[:, 1] / 2), dim=1)
    b = torch.stack((b[:, 0].clamp(0, w - 2), b[:, 1].clamp(0, h - 2), b[:, 2].clamp(2, w), b[:, 3].clamp(2, h)), dim=1)
    return b, torch.randint(0, K, (boxes,), generator=g)


def timed(call, stream_sync):
    for _ in range(CALLS):
        call()
    stream_sync()
    out = []
    for _ in range(WINDOWS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(CALLS):
            call()
        e1.record()
        stream_sync()
        out.append(e0.elapsed_time(e1) / CALLS)
    return {"median_ms": statistics.median(out), "min_ms": min(out), "max_ms": max(out), "launches": WINDOWS * CALLS}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default="")
    ap.add_argument("--device", default="cuda:0")
    args = ap.parse_args(argv)
    dev = torch.device(args.device)
    torch.cuda.set_device(dev)
    ph, pw = _anchors.padded_size(720, 1280)
    shapes = _anchors.level_shapes(ph, pw)
    level_anchors = _anchors.grid_anchors(shapes, device=dev)
    R = sum(h * w * A for h, w in shapes)
    g = torch.Generator().manual_seed(27)
    plane = lambda c, scale, shift=0.0: [(torch.randn(BATCH, A * c, h, w, generator=g) * scale + shift).to(dev) for h, w in shapes]
    cls, delta, cls_var, reg_var = plane(K, 1.0, -4.0), plane(4, 0.5), plane(K, 1.0), plane(4, 2.0)
    gts = [ground_truth(i, 720, 1280) for i in range(BATCH)]
    labels, matched, num_pos = losses.label_anchors(level_anchors, [b for b, _ in gts], [c for _, c in gts], K)
    gt = torch.cat([b for b, _ in gts]).to(dev)
    w = torch.tensor([0.1 / 300, 0.5 / 300, 0.5 / 300], device=dev)
    lib = hip.load()
    stream = hip.current_stream()
    sync = lambda: torch.cuda.current_stream().synchronize()
    result = {"frame": [720, 1280], "padded": [ph, pw], "images": BATCH, "anchors_per_image": R, "positives_per_image": num_pos.cpu().tolist(),
              "positives": int(num_pos.sum()), "boxes_per_image": 12, "num_samples": M, "cls_samples": S, "windows": WINDOWS, "calls_per_window": CALLS}

    def grad_planes(with_reg_var):
        planes = [[torch.empty_like(t) for t in ts] for ts in (cls, cls_var, delta, reg_var)]
        arr = (hip.PodLevelGrad * hip.POD_MAX_LEVELS)()
        for l in range(len(shapes)):
            arr[l].cls, arr[l].cls_var, arr[l].delta = planes[0][l].data_ptr(), planes[1][l].data_ptr(), planes[2][l].data_ptr()
            arr[l].reg_var = planes[3][l].data_ptr() if with_reg_var else None
        return planes, arr

    # pod_train_loss: as the NLL runs it (with the reg_var planes), and as the first launch of the two-launch composition (without)
    for name, rv in (("pod_train_loss, NLL (reg_var planes)", reg_var), ("pod_train_loss, first of two launches (no reg_var)", None)):
        cfg, lv, a, _ = losses._launch_inputs(cls, delta, cls_var, rv, labels, matched, gt, level_anchors, A, K, (1.0, 1.0, 1.0, 1.0), S, 3, None)
        keep, garr = grad_planes(rv is not None)
        partials = torch.empty(int(lib.pod_train_loss_partials(cfg, lv)), dtype=torch.float64, device=dev)
        sums = torch.empty(4, dtype=torch.float64, device=dev)
        call = lambda: hip.check(lib.pod_train_loss(cfg, lv, garr, hip.ptr(labels), hip.ptr(matched), hip.ptr(gt), int(gt.shape[0]), hip.ptr(a), R, 0.25,
                                                    2.0, 0.0, None, None, hip.ptr(w), hip.ptr(partials), hip.ptr(sums), stream), "pod_train_loss")
        result[name] = timed(call, sync)
    # pod_reg_score_loss on the planes of the launch above
    cfg, lv, a, _ = losses._launch_inputs(cls, delta, cls_var, reg_var, labels, matched, gt, level_anchors, A, K, (1.0, 1.0, 1.0, 1.0), S, 3, None)
    keep, garr = grad_planes(True)
    for l in range(len(shapes)):
        keep[2][l].zero_()                      # (the launch adds to the delta planes: start them finite)
    partials = torch.empty(int(lib.pod_reg_score_partials(cfg, lv)), dtype=torch.float64, device=dev)
    total = torch.empty(1, dtype=torch.float64, device=dev)
    for name, kind in (("pod_reg_score_loss, energy_loss", hip.POD_REG_LOSS_ENERGY), ("pod_reg_score_loss, second_moment_matching", hip.POD_REG_LOSS_MOMENTS)):
        for tag, grads in ((" with gradients", garr), (" value only", None)):
            call = lambda: hip.check(lib.pod_reg_score_loss(cfg, lv, grads, hip.ptr(labels), hip.ptr(matched), hip.ptr(gt), int(gt.shape[0]), hip.ptr(a), R,
                                                            kind, M, 0.0, None, None, hip.ptr(w) if grads is not None else None, hip.ptr(partials),
                                                            hip.ptr(total), stream), "pod_reg_score_loss")
            result[name + tag] = timed(call, sync)
            result[name + tag]["sum"] = float(total.cpu()[0])
    print(json.dumps(result, indent=1))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
    return result


if __name__ == "__main__":
    main()
