"""What the corruptions (K35, pod_corrupt_frame_u8) cost.

1. Device time of every (name, severity) on one 720 x 1280 frame (seeded random bytes; the arithmetic does not depend on the content).
   CALLS calls of the C entry, buffers allocated beforehand, are captured into one HIP graph and the graph is replayed between two device
   events: the figure is device time per call, free of the host's enqueue cost.  One warm-up replay, then REPEATS replays: median, minimum
   and maximum.  K20 (the loader's resize, 720 x 1280 -> 750 x 1333) is timed the same way beside them, for scale.
2. apply_net from files on cfg2 (retinanet_R_50_FPN_1x_reg_cls_var + bayes_od): --images JPEG frames of 1280 x 720 written under a
   temporary directory, run with --resize-on-gpu three ways -- no corruption, contrast severity 3, defocus_blur severity 5 -- taking turns,
   --rounds times each; the `inference loop:` line's images/s after the first flush, median and range over the rounds.

    python tools/corruption_bench.py [--out profiles/corruptions.json] [--md profiles/corruptions.md] [--images 600] [--rounds 2]
"""
import argparse
import ctypes
import json
import os
import re
import shutil
import statistics
import subprocess
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
from pod_compare_amd import corruptions, hip, resize      # noqa: E402

H, W, CALLS, REPEATS = 720, 1280, 20, 9
FROM_FILES = (("none", []), ("contrast 3", ["--corruption", "contrast", "--severity", "3"]),
              ("defocus_blur 5", ["--corruption", "defocus_blur", "--severity", "5"]))


def replayed(enqueue):
    """Median / min / max device time in microseconds of one call of `enqueue`, CALLS of them replayed as one graph."""
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        enqueue()
        s.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            for _ in range(CALLS):
                enqueue()
        g.replay()
        s.synchronize()
        out = []
        for _ in range(REPEATS):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            g.replay()
            e1.record(s)
            s.synchronize()
            out.append(1000.0 * e0.elapsed_time(e1) / CALLS)
    return {"median_us": statistics.median(out), "min_us": min(out), "max_us": max(out)}


def kernel_times(dev):
    lib = hip.load()
    frame = torch.from_numpy(np.random.default_rng(35).integers(0, 256, size=(H, W, 3), dtype=np.uint8)).to(dev)
    out = torch.empty_like(frame)
    rows = {}
    for name in corruptions.NAMES:
        for severity in (1, 2, 3, 4, 5):
            rec = corruptions.record(name, severity, corruptions.corruption_key(0, 1), frame.device)
            need = int(lib.pod_corrupt_scratch_bytes(rec.kind, H, W))
            scratch = torch.empty((need // 8 + 1,), dtype=torch.int64, device=dev)

            def enqueue():
                hip.check(lib.pod_corrupt_frame_u8(frame.data_ptr(), H, W, 3 * W, out.data_ptr(), 3 * W, ctypes.byref(rec),
                                                   scratch.data_ptr() if need else None, need, hip.current_stream()), "pod_corrupt_frame_u8")
            rows["%s %d" % (name, severity)] = r = replayed(enqueue)
            print("%-16s %d: %8.1f us (%.1f - %.1f)" % (name, severity, r["median_us"], r["min_us"], r["max_us"]), flush=True)
    resize.resize_frame_u8(frame, 800, 1333)
    rows["K20 resize 720x1280 -> 750x1333"] = r = replayed(lambda: resize.resize_frame_u8(frame, 800, 1333))
    print("K20 resize        : %8.1f us (%.1f - %.1f)" % (r["median_us"], r["min_us"], r["max_us"]), flush=True)
    return rows


def from_files(n, rounds):
    from PIL import Image
    rates = {k: [] for k, _ in FROM_FILES}
    with tempfile.TemporaryDirectory(prefix="pod_corruption_bench") as root:
        rng = np.random.default_rng(0)
        yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
        images = [{"id": k + 1, "file_name": "%05d.jpg" % k, "height": H, "width": W} for k in range(n)]
        for k in range(min(n, 16)):  # smooth content with a little noise, as tools/loader_bench.py writes; 16 different frames, then copies
            f = rng.uniform(0.002, 0.02, size=6)
            img = np.stack([127 + 120 * np.sin(f[2 * c] * xx + k) * np.cos(f[2 * c + 1] * yy) for c in range(3)], axis=-1)
            img += rng.normal(0, 4, size=img.shape)
            Image.fromarray(np.clip(img, 0, 255).astype(np.uint8)).save(os.path.join(root, "%05d.jpg" % k), quality=90)
        for k in range(16, n):
            shutil.copyfile(os.path.join(root, "%05d.jpg" % (k % 16)), os.path.join(root, "%05d.jpg" % k))
        with open(os.path.join(root, "set.json"), "w") as fp:
            json.dump({"images": images}, fp)
        cfg2 = ["--config-file", "pod_compare_amd/configs/BDD-Detection/retinanet/retinanet_R_50_FPN_1x_reg_cls_var.yaml",
                "--inference-config", "pod_compare_amd/configs/Inference/bayes_od.yaml"]
        for _ in range(rounds):
            for label, extra in FROM_FILES:
                cmd = [sys.executable, "-m", "pod_compare_amd.apply_net", "--coco-json", os.path.join(root, "set.json"), "--image-root", root,
                       "--random-init", "--resize-on-gpu", "--output", os.path.join(root, "out.json")] + cfg2 + extra
                r = subprocess.run(cmd, cwd=HERE, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=900)
                m = re.search(r"inference loop: .* = ([0-9.]+) images/s; ([0-9.]+) images/s after the first flush", r.stdout)
                if r.returncode != 0 or m is None:
                    raise RuntimeError("apply_net failed (%d):\n%s" % (r.returncode, r.stdout[-2000:]))
                rates[label].append(float(m.group(2)))
                print("from files, %-15s: %.1f images/s after the first flush (%.1f over the whole loop)" % (label, float(m.group(2)), float(m.group(1))), flush=True)
    return {k: {"median_images_per_s": statistics.median(v), "min": min(v), "max": max(v), "runs": v} for k, v in rates.items()}


def markdown(res):
    k, f = res["kernel_us"], res["from_files"]
    per_image_us = 1e6 / f["none"]["median_images_per_s"]
    lines = ["# Corruptions on the GPU (K35, `apply_net --corruption`): measurements", "",
             "`tools/corruption_bench.py`, one MI355X (%s), one session." % res["device"], "",
             "## Device time per call on a 720 x 1280 frame", "",
             "%d calls of `pod_corrupt_frame_u8` replayed as one HIP graph between two device events, one warm-up replay, %d timed replays: median "
             "(minimum - maximum) in microseconds per call.  `contrast` is three launches, `gaussian_blur` two, the others one." % (CALLS, REPEATS), "",
             "| name | severity 1 | 2 | 3 | 4 | 5 |", "|---|---|---|---|---|---|"]
    for name in corruptions.NAMES:
        cells = ["%.1f (%.1f - %.1f)" % (k["%s %d" % (name, s)]["median_us"], k["%s %d" % (name, s)]["min_us"], k["%s %d" % (name, s)]["max_us"]) for s in (1, 2, 3, 4, 5)]
        lines.append("| `%s` | %s |" % (name, " | ".join(cells)))
    r = k["K20 resize 720x1280 -> 750x1333"]
    lines += ["", "For scale, K20 (`resize.resize_frame_u8`, the output's allocation inside the graph's pool) the same way: %.1f (%.1f - %.1f)." % (r["median_us"], r["min_us"], r["max_us"]), "",
              "## `apply_net` from %d JPEG files of 1280 x 720, cfg2, `--resize-on-gpu`" % res["images"], "",
              "Images/s after the first flush, %d run(s) each, taking turns; 16 host CPUs decode." % res["rounds"], "",
              "| corruption | median | range |", "|---|---|---|"]
    for label, _ in FROM_FILES:
        lines.append("| %s | %.1f | %.1f - %.1f |" % (label, f[label]["median_images_per_s"], f[label]["min"], f[label]["max"]))
    over = sorted(((v["median_us"], n) for n, v in k.items() if not n.startswith("K20") and v["median_us"] > 0.1 * per_image_us), reverse=True)
    lines += ["", "An image of the uncorrupted run takes %.0f us (1 / the median rate).  Kinds above a tenth of that: %s." % (
        per_image_us, ", ".join("`%s` (%.0f us)" % (n, t) for t, n in over) if over else "none")]
    return "\n".join(lines) + "\n"


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default="")
    ap.add_argument("--md", default="")
    ap.add_argument("--images", type=int, default=600)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--device", default="cuda:0")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("corruption_bench.py measures on the GPU: none found")
    dev = torch.device(args.device)
    torch.cuda.set_device(dev)
    res = {"frame": [H, W], "calls_per_replay": CALLS, "replays": REPEATS, "device": torch.cuda.get_device_name(dev), "images": args.images, "rounds": args.rounds}
    res["kernel_us"] = kernel_times(dev)
    torch.cuda.synchronize()
    res["from_files"] = from_files(args.images, args.rounds)
    for path, text in ((args.out, json.dumps(res, indent=1) + "\n"), (args.md, markdown(res))):
        if path:
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
            with open(path, "w") as f:
                f.write(text)
    return res


if __name__ == "__main__":
    main()
