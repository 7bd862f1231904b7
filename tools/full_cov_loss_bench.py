"""Times pod_full_cov_loss (K28, its three kinds) beside pod_reg_score_loss (K27) on the diagonal slice of the same inputs, at the headline
training frame: 768 x 1344, 2 images, BBOX_COV_LOSS.NUM_SAMPLES = 1000, seeded random head outputs, and seeded labels at the positive
density of the loss fixture (81 positives among its 2 x 1161 anchors), each positive matched to one of 12 seeded boxes.  Every figure is
the median over WINDOWS windows of CALLS launches enqueued back to back from the C entry between two device events (so the device, not
Python, sets the pace), after a warm-up window.

    python tools/full_cov_loss_bench.py [--out profiles/full_cov_losses.json]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pod_compare_amd import anchors as _anchors, hip, losses      # noqa: E402
from tools.score_loss_bench import CALLS, WINDOWS, ground_truth, timed      # noqa: E402

K, A, M, BATCH = 7, 9, 1000, 2
FRAME = (768, 1344)
DENSITY = 81.0 / (2 * 1161)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default="")
    ap.add_argument("--device", default="cuda:0")
    args = ap.parse_args(argv)
    dev = torch.device(args.device)
    torch.cuda.set_device(dev)
    ph, pw = _anchors.padded_size(*FRAME)
    shapes = _anchors.level_shapes(ph, pw)
    level_anchors = _anchors.grid_anchors(shapes, device=dev)
    R = sum(h * w * A for h, w in shapes)
    g = torch.Generator().manual_seed(28)
    plane = lambda c, scale, shift=0.0: [(torch.randn(BATCH, A * c, h, w, generator=g) * scale + shift).to(dev) for h, w in shapes]
    cls, delta, full = plane(K, 1.0, -4.0), plane(4, 0.5), plane(10, 0.5)
    # the diagonal slice of the same inputs: channels a * 10 + (0 .. 3) of every anchor shape a
    diag = [t.view(BATCH, A, 10, *t.shape[2:])[:, :, :4].reshape(BATCH, A * 4, *t.shape[2:]).contiguous() for t in full]
    gt, _ = ground_truth(0, *FRAME)
    positive = torch.rand((BATCH, R), generator=g) < DENSITY
    labels = torch.where(positive, torch.randint(0, K, (BATCH, R), generator=g), torch.full((BATCH, R), K)).to(torch.int32).to(dev)
    matched = torch.randint(0, int(gt.shape[0]), (BATCH, R), generator=g).to(torch.int32).to(dev)
    gt = gt.to(dev)
    w = torch.tensor([0.1 / 300, 0.5 / 300, 0.5 / 300], device=dev)
    lib = hip.load()
    stream = hip.current_stream()
    sync = lambda: torch.cuda.current_stream().synchronize()
    result = {"frame": list(FRAME), "padded": [ph, pw], "images": BATCH, "anchors_per_image": R, "positives_per_image": positive.sum(1).tolist(),
              "positives": int(positive.sum()), "num_samples": M, "windows": WINDOWS, "calls_per_window": CALLS}
    entries = (("pod_full_cov_loss", lib.pod_full_cov_loss, lib.pod_full_cov_partials, full,
                (("negative_log_likelihood", hip.POD_FULL_COV_NLL), ("second_moment_matching", hip.POD_FULL_COV_MOMENTS),
                 ("energy_loss", hip.POD_FULL_COV_ENERGY))),
               ("pod_reg_score_loss (diagonal slice)", lib.pod_reg_score_loss, lib.pod_reg_score_partials, diag,
                (("second_moment_matching", hip.POD_REG_LOSS_MOMENTS), ("energy_loss", hip.POD_REG_LOSS_ENERGY))))
    for entry, fn, n_partials, reg_var, kinds in entries:
        cfg, lv, a, _ = losses._launch_inputs(cls, delta, None, reg_var, labels, matched, gt, level_anchors, A, K, (1.0, 1.0, 1.0, 1.0), 0, 3, None)
        g_delta, g_reg_var = [torch.zeros_like(t) for t in delta], [torch.empty_like(t) for t in reg_var]      # (the launch adds to the delta planes)
        garr = (hip.PodLevelGrad * hip.POD_MAX_LEVELS)()
        for l in range(len(shapes)):
            garr[l].delta, garr[l].reg_var = g_delta[l].data_ptr(), g_reg_var[l].data_ptr()
        partials = torch.empty(int(n_partials(cfg, lv)), dtype=torch.float64, device=dev)
        total = torch.empty(1, dtype=torch.float64, device=dev)
        for name, kind in kinds:
            for tag, grads in ((" with gradients", garr), (" value only", None)):
                call = lambda: hip.check(fn(cfg, lv, grads, hip.ptr(labels), hip.ptr(matched), hip.ptr(gt), int(gt.shape[0]), hip.ptr(a), R, kind, M, 0.0,
                                            None, None, hip.ptr(w) if grads is not None else None, hip.ptr(partials), hip.ptr(total), stream), entry)
                key = "%s, %s%s" % (entry, name, tag)
                result[key] = timed(call, sync)
                result[key]["sum"] = float(total.cpu()[0])
    print(json.dumps(result, indent=1))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
    return result


if __name__ == "__main__":
    main()
