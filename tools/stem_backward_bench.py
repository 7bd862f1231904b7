"""Times K30's two entries at the BDD training shape: 720 x 1280 uint8 frames padded to 736 x 1280, SOLVER.IMS_PER_BATCH = 4 -- the stem's
output is 368 x 640 x 64 per image, the pool's 184 x 320 x 64.  pod_maxpool3x3s2_backward_cl per image (one launch) and over the batch
(four launches under one record, as the trainer issues them), pod_stem7x7_wgrad over the batch's stacked frames (its two launches).  Every
figure is the median over WINDOWS windows of CALLS calls enqueued back to back from the C entry between two device events (so the device,
not Python, sets the pace), after a warm-up window; beside each the bytes the call must move and what they would take at 8 TB/s.  No
threshold is applied here.

    python tools/stem_backward_bench.py [--out profiles/stem_backward.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pod_compare_amd import amax, anchors as _anchors, conv1x1, hip      # noqa: E402

WINDOWS, CALLS = 10, 20
BATCH, HBM_TBS = 4, 8.0


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
    return {"median_ms": statistics.median(out), "min_ms": min(out), "max_ms": max(out), "calls": WINDOWS * CALLS}


def against_hbm(entry: dict, nbytes: int) -> dict:
    floor_ms = nbytes / (HBM_TBS * 1e12) * 1e3
    entry.update(bytes=nbytes, hbm_floor_ms=floor_ms, fraction_of_hbm=floor_ms / entry["median_ms"])
    return entry


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default="")
    ap.add_argument("--device", default="cuda:0")
    args = ap.parse_args(argv)
    dev = torch.device(args.device)
    torch.cuda.set_device(dev)
    hi, wi = 720, 1280
    ph, pw = _anchors.padded_size(hi, wi)
    h, w = (ph - 1) // 2 + 1, (pw - 1) // 2 + 1
    hq, wq = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    g = torch.Generator().manual_seed(30)
    frames = torch.randint(0, 256, (BATCH, 3, hi, wi), generator=g, dtype=torch.uint8).to(dev)
    mean, std = torch.tensor([103.530, 116.280, 123.675], device=dev), torch.tensor([57.375, 57.120, 58.395], device=dev)
    s = torch.relu(torch.randn((BATCH * h * w, 64), generator=g)).to(dev)              # about half zeros, as a ReLU leaves them
    dp = torch.randn((BATCH * hq * wq, 64), generator=g).to(dev)
    ds = torch.empty_like(s)
    lib, stream = hip.load(), hip.current_stream()
    sync = lambda: torch.cuda.current_stream().synchronize()
    result = {"frame": [hi, wi], "padded": [ph, pw], "images": BATCH, "stem_map": [h, w], "pooled_map": [hq, wq], "windows": WINDOWS, "calls_per_window": CALLS}

    rec = amax.word(dev)
    rows = lambda t, b: t[b * (t.shape[0] // BATCH):(b + 1) * (t.shape[0] // BATCH)]

    def pool(images):
        for b in range(images):
            hip.check(lib.pod_maxpool3x3s2_backward_cl(rows(s, b).data_ptr(), rows(dp, b).data_ptr(), rows(ds, b).data_ptr(), h, w, 64, rec.data_ptr(), stream),
                      "pod_maxpool3x3s2_backward_cl")
    per_image = (2 * h * w + hq * wq) * 64 * 4                                       # s and dS once each, dP once
    result["pod_maxpool3x3s2_backward_cl, one image"] = against_hbm(timed(lambda: pool(1), sync), per_image)
    result["pod_maxpool3x3s2_backward_cl, the batch (4 launches)"] = against_hbm(timed(lambda: pool(BATCH), sync), BATCH * per_image)

    n = int(lib.pod_stem7x7_wgrad_partials(BATCH, hi, wi, ph, pw))
    partials = torch.empty(n, dtype=torch.float32, device=dev)
    dW = torch.empty((64, 3, 7, 7), dtype=torch.float32, device=dev)
    bound = conv1x1.normalised_input_bound(frames, mean, std, {})
    ds_rec = amax.of(ds)
    call = lambda: hip.check(lib.pod_stem7x7_wgrad(frames.data_ptr(), 1, BATCH, hi, wi, mean.data_ptr(), std.data_ptr(), ds.data_ptr(), ph, pw, bound.data_ptr(),
                                                   ds_rec.data_ptr(), dW.data_ptr(), partials.data_ptr(), stream), "pod_stem7x7_wgrad")
    result["pod_stem7x7_wgrad, the batch"] = against_hbm(timed(call, sync), BATCH * (h * w * 64 * 4 + 3 * hi * wi))     # dS once plus the uint8 frames
    result["pod_stem7x7_wgrad, the batch"].update(slices=n // (64 * 192), partial_bytes=4 * n)
    print(json.dumps(result, indent=1))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
    return result


if __name__ == "__main__":
    main()
