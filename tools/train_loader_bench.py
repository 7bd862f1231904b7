"""GPU box: what train_head --train-loader and K31 cost, as profiles/train_loader.md reports it.
    python tools/train_loader_bench.py <out.txt> [--frames 32] [--iters 4 20] [--repeats 3] [--workers 8]

(a) K31 against K20: one pod_train_batch_u8 launch on four decoded 720 x 1280 frames at short edges drawn from 640..800, with flips,
    against what the parent does for the same frames -- four pod_resize_frame_u8 launches and a .flip(-1) where mirrored -- by device
    events, the two alternating, `--repeats` rounds of 50 calls each behind a warm-up round.
(b) step time and frames per second of `train_head --train-backbone --fused-step` on synthetic 720 x 1280 JPEGs (MIN_SIZE_TRAIN 720,
    IMS_PER_BATCH 4): --train-loader with the host loader, with --batch-on-gpu, and the parent's command line without the flag.  A
    variant runs at both iteration counts of --iters; the step time is the difference of the two wall times (set-up, model build and
    warm-up cancel) over the difference of the counts.  The variants alternate inside a repeat.
(c) the host time the main loop waits for the loader in each: the time inside next() of the Prefetched iterator, per step, by the same
    difference.  One untimed run of every variant comes first.
Every figure is printed with the spread over the repeats (min .. max)."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pod_compare_amd import anchors, apply_net, resize, train_batch, train_head  # noqa: E402


def spread(xs):
    return "%.4g (%.4g .. %.4g, n = %d)" % (statistics.median(xs), min(xs), max(xs), len(xs))


def kernel_bench(repeats, say):
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    frames = [torch.randint(0, 256, (720, 1280, 3), generator=g, dtype=torch.uint8).to(dev) for _ in range(4)]
    edges = [int(torch.randint(640, 801, (), generator=g)) for _ in range(4)]
    flips = [True, False, True, True]
    sizes = [anchors.resize_shortest_edge(720, 1280, e, 1333) for e in edges]

    def parent():
        out = [resize.resize_frame_u8(f, e, 1333) for f, e in zip(frames, edges)]
        return [o.flip(-1) if fl else o for o, fl in zip(out, flips)]

    def k31():
        return train_batch.train_batch_u8(frames, sizes, flips)

    assert all(torch.equal(a, b) for a, b in zip(parent(), k31()))
    times = {"parent": [], "k31": []}
    for r in range(repeats + 1):
        for name, fn in (("parent", parent), ("k31", k31)):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            for _ in range(50):
                fn()
            b.record()
            torch.cuda.synchronize()
            if r:                                        # round 0 warms up
                times[name].append(a.elapsed_time(b) / 50 * 1e3)
    say("(a) four 720 x 1280 frames -> short edges %s, flips %s; microseconds per batch, device events over 50 calls" % (edges, flips))
    say("    parent (4 x pod_resize_frame_u8 + .flip(-1)): %s" % spread(times["parent"]))
    say("    K31    (1 x pod_train_batch_u8):              %s" % spread(times["k31"]))
    say("    ratio parent / K31 of the medians: %.2f" % (statistics.median(times["parent"]) / statistics.median(times["k31"])))


class TimedPrefetched(apply_net.Prefetched):
    waited = 0.0

    def __iter__(self):
        it = super().__iter__()
        while True:
            t0 = time.perf_counter()
            try:
                item = next(it)
            except StopIteration:
                return
            finally:
                TimedPrefetched.waited += time.perf_counter() - t0
            yield item


def write_frames(root, n):
    from PIL import Image
    rng = np.random.default_rng(0)
    yy, xx = np.mgrid[0:720, 0:1280].astype(np.float32)
    images, anns = [], []
    for k in range(n):
        f = rng.uniform(0.002, 0.02, size=6)
        img = np.stack([127 + 120 * np.sin(f[2 * c] * xx + k) * np.cos(f[2 * c + 1] * yy) for c in range(3)], axis=-1) + rng.normal(0, 4, size=(720, 1280, 3))
        Image.fromarray(np.clip(img, 0, 255).astype(np.uint8)).save(os.path.join(root, "%05d.jpg" % k), quality=90)
        images.append({"id": k + 1, "file_name": "%05d.jpg" % k, "height": 720, "width": 1280})
        for j in range(3):
            anns.append({"id": 3 * k + j + 1, "image_id": k + 1, "category_id": 1 + (k + j) % 3, "bbox": [100 + 300 * j, 200 + 7 * (k % 20), 180, 140], "iscrowd": 0})
    json.dump({"images": images, "annotations": anns}, open(os.path.join(root, "gt.json"), "w"))


def step_bench(n_frames, iters, repeats, workers, say):
    train_head.Prefetched = TimedPrefetched
    base = os.path.join(ROOT, "pod_compare_amd/configs/BDD-Detection/retinanet/retinanet_R_50_FPN_1x.yaml")
    variants = {"--train-loader": ["--train-loader"], "--train-loader --batch-on-gpu": ["--train-loader", "--batch-on-gpu"],
                "parent (no flag, 720 / 1333 through the TEST keys)": ["--min-size-test", "720", "--max-size-test", "1333"]}
    with tempfile.TemporaryDirectory() as root:
        write_frames(root, n_frames)
        figures = {name: {"step": [], "wait": []} for name in variants}

        def run(flags, n):
            train_head.main(["--config-file", base, "--coco-json", os.path.join(root, "gt.json"), "--image-root", root, "--random-init",
                             "--output-dir", os.path.join(root, "out"), "--max-iter", str(n), "--log-period", "0", "--loader-workers", str(workers),
                             "--train-backbone", "--fused-step"] + flags)
            torch.cuda.synchronize()

        for flags in variants.values():                  # untimed: code objects, filter splits, pinned tables, the files in the page cache
            run(flags, iters[0])
        for r in range(repeats):
            for name, flags in variants.items():
                wall, wait = [], []
                for n in iters:
                    TimedPrefetched.waited = 0.0
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    run(flags, n)
                    wall.append(time.perf_counter() - t0)
                    wait.append(TimedPrefetched.waited)
                figures[name]["step"].append((wall[1] - wall[0]) / (iters[1] - iters[0]))
                figures[name]["wait"].append((wait[1] - wait[0]) / (iters[1] - iters[0]))
    say("(b), (c) %d JPEG frames of 720 x 1280, IMS_PER_BATCH 4, MIN_SIZE_TRAIN 720, --train-backbone --fused-step, %d loader threads; per step, from "
        "runs of %d and %d iterations" % (n_frames, workers, iters[0], iters[1]))
    for name, f in figures.items():
        say("    %s" % name)
        say("        step time  s: %s" % spread(f["step"]))
        say("        frames / s  : %s" % spread([4.0 / s for s in f["step"]]))
        say("        loader wait s: %s" % spread(f["wait"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--iters", type=int, nargs=2, default=[4, 20])
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--workers", type=int, default=8)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("train_loader_bench measures on the GPU: no GPU here, nothing measured")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fp:
        def say(line):
            print(line, flush=True)
            fp.write(line + "\n")
            fp.flush()
        kernel_bench(args.repeats, say)
        step_bench(args.frames, args.iters, args.repeats, args.workers, say)


if __name__ == "__main__":
    main()
