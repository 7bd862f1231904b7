"""What the gradient bucket costs (profiles/data_parallel.md): pod_grad_pack (K26) back to back on the --train-backbone parameter set, and the
optimiser's section of a world-1 --data-parallel step (pack + tail + pod_sgd_step from the bucket) beside the plain --fused-step section,
alternating step by step in ONE process.  The set-up is profiles/sgd_step.md's: retinanet_R_50_FPN_1x, random initialisation, four frames
of 720 x 1280 (uint8 noise, three boxes each), learning rate 0 (the untrained loss overflows at the config's rate; at rate 0 the launches
are the same and nothing moves).  GPU only.

    python tools/data_parallel_bench.py [--height 720 --width 1280 --batch 4 --warmup 3 --steps 8] [--out data_parallel_bench.json]"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from pod_compare_amd import hip, losses, train_head  # noqa: E402
from pod_compare_amd.config import setup_config  # noqa: E402
from pod_compare_amd.probabilistic_inference import build_model  # noqa: E402

YAML = os.path.join(ROOT, "pod_compare_amd", "configs/BDD-Detection/retinanet/retinanet_R_50_FPN_1x.yaml")


def make_trainer(data_parallel: bool, dev: str):
    cfg = setup_config(YAML, "", 0)
    cfg.MODEL.DEVICE = dev
    torch.manual_seed(0)
    model = build_model(cfg, save_dir=None, load_weights=False)
    cpu_cfg = cfg.clone()
    cpu_cfg.MODEL.DEVICE = "cpu"
    torch.manual_seed(0)
    shadow = build_model(cpu_cfg, save_dir=None, load_weights=False, fold=False)
    model.loss_state = losses.ProbabilisticLosses(num_classes=cfg.MODEL.RETINANET.NUM_CLASSES, cls_var_num_samples=cfg.MODEL.PROBABILISTIC_MODELING.CLS_VAR_LOSS.NUM_SAMPLES,
                                                  annealing_step=int(cfg.SOLVER.STEPS[1]))
    return train_head.HeadTrainer(model, base_lr=0.0, warmup_iters=0, train_backbone=True, shadow=shadow, fused_step=True,
                                  data_parallel=(0, 1, None) if data_parallel else None)


def stats(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU: there is no CPU figure"
    dev = "cuda:0"
    torch.cuda.set_device(0)
    g = torch.Generator().manual_seed(1)
    images = [torch.randint(0, 256, (3, args.height, args.width), generator=g, dtype=torch.uint8).to(dev) for _ in range(args.batch)]
    H, W = args.height, args.width
    gb = [torch.tensor([[0.1 * W, 0.1 * H, 0.3 * W, 0.4 * H], [0.5 * W, 0.3 * H, 0.9 * W, 0.8 * H], [0.4 * W, 0.5 * H, 0.5 * W, 0.7 * H]]) for _ in images]
    gc = [torch.tensor([1, 4, 2]) for _ in images]
    trainers = {"fused": make_trainer(False, dev), "data_parallel": make_trainer(True, dev)}
    section = {k: {"device_ms": [], "host_ms": []} for k in trainers}
    whole = {k: [] for k in trainers}

    def one_step(name, timed_section):
        tr = trainers[name]
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        ev[0].record()
        feats, padded = tr.features(images)
        tr.forward_backward(feats, padded, (H, W), gb, gc)
        if timed_section:
            torch.cuda.synchronize()                   # the device starts the section idle: the events time the section alone
        ev[1].record()
        t0 = time.perf_counter()
        if tr.bucket is not None:
            tr.reduce_gradients()
        tr.optimizer_step(tr.lr)
        t1 = time.perf_counter()
        ev[2].record()
        tr.advance()
        ev[3].record()
        torch.cuda.synchronize()
        return ev[1].elapsed_time(ev[2]), 1e3 * (t1 - t0), ev[0].elapsed_time(ev[3])

    for timed_section in (True, False):
        for i in range(args.warmup + args.steps):
            for name in trainers:                       # alternating: fused, data_parallel, fused, ...
                d, h, w = one_step(name, timed_section)
                if i >= args.warmup:
                    if timed_section:
                        section[name]["device_ms"].append(d)
                        section[name]["host_ms"].append(h)
                    else:
                        whole[name].append(w)
    # the kernel: 20 calls back to back from the C entry on one unchanged table
    b = trainers["data_parallel"].bucket
    torch.cuda.synchronize()
    lib, table = hip.load(), b.table.begin()
    for d, e in zip(table, b.entries):
        d.grad = e.w.data_ptr()                         # any fp32 tensor of the size: the weights stand in for gradients that were cleared
    call = lambda: hip.check(lib.pod_grad_pack(table, *b.table.launch_args(), *b.pack_args(), 1.0, hip.current_stream()), "pod_grad_pack")
    reps, per_call, host_call = 20, [], []
    for r in range(2 + 6):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        t0 = time.perf_counter()
        for _ in range(reps):
            call()
        t1 = time.perf_counter()
        e1.record()
        torch.cuda.synchronize()
        if r >= 2:
            per_call.append(e0.elapsed_time(e1) / reps)
            host_call.append(1e3 * (t1 - t0) / reps)
    elements = sum(e.w.numel() for e in b.entries)
    out = {"frames": [args.batch, H, W], "tensors": len(b.entries), "elements": elements, "bucket_floats": b.floats, "chunks": b.table.n_chunks,
           "pack_bytes": 8 * elements, "pack_ms_per_call": stats(per_call), "pack_host_ms_per_call": stats(host_call),
           "pack_TBps": 8 * elements / (statistics.median(per_call) * 1e-3) / 1e12,
           "section": {k: {m: stats(v) for m, v in s.items()} for k, s in section.items()}, "whole_step_ms": {k: stats(v) for k, v in whole.items()},
           "peak_memory_GB": torch.cuda.max_memory_allocated() / 1e9, "warmup": args.warmup, "steps": args.steps}
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
