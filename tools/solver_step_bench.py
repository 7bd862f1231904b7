"""What the solver's step costs (profiles/solver_step.md): pod_sgd_step (K25) and pod_sgd_step_solver (K29) back to back from the C entry on
the --train-backbone parameter set of retinanet_R_50_FPN_1x (78 tensors, 36.2 M elements, the table of profiles/sgd_step.md), in ONE
process, the variants taking turns repetition by repetition:

    pod_sgd_step | pod_sgd_step_solver with the default record | with two groups | with clipping by value | with full_model clipping and the guard

Learning rate 0 and the weights standing in for the gradients (the launches and the bytes are a real step's; nothing moves but the
momentum).  A repetition is `--calls` calls behind one another between two device events.  The requirement the tool states: the default
record is no slower than pod_sgd_step by more than the spread (maximum - minimum) pod_sgd_step shows between its own repetitions.  GPU only.

    python tools/solver_step_bench.py [--calls 20 --warmup 2 --reps 6] [--out solver_step_bench.json]"""
import argparse
import ctypes
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
from pod_compare_amd.sgd_step import SolverSettings  # noqa: E402

YAML = os.path.join(ROOT, "pod_compare_amd", "configs/BDD-Detection/retinanet/retinanet_R_50_FPN_1x.yaml")


def make_trainer(dev: str):
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
    # (any settings that are not the default ones: the optimiser then owns a group array and a workspace)
    return train_head.HeadTrainer(model, base_lr=0.0, warmup_iters=0, train_backbone=True, shadow=shadow, fused_step=True,
                                  solver=SolverSettings(clip_type="full_model", guard_nonfinite=True))


def stats(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "spread": max(xs) - min(xs)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=6)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU: there is no CPU figure"
    torch.cuda.set_device(0)
    fused = make_trainer("cuda:0").fused
    lib, table = hip.load(), fused.table.begin()
    for d, e in zip(table, fused.entries):
        d.grad = e.w.data_ptr()                         # any fp32 tensor of the size: the weights stand in for the gradients
    launch = fused.table.launch_args()
    loss = torch.tensor([0.5, 0.25], device="cuda:0")

    def record(clip=hip.POD_SGD_CLIP_OFF, guard=0, n_groups=1):
        r = hip.PodSgdSolver()
        r.n_groups, r.clip_type, r.guard, r.momentum, r.clip_value = n_groups, clip, guard, fused.mu, 1.0
        for g in range(n_groups):
            r.lr[g], r.wd[g] = 0.0, fused.weight_decay
        if guard:
            r.watch[0], r.watch[1] = loss[0:1].data_ptr(), loss[1:2].data_ptr()
        return r

    def solver_call(rec):
        return lambda: hip.check(lib.pod_sgd_step_solver(table, *launch, fused._group_host, fused._group_dev.data_ptr(), ctypes.byref(rec),
                                                         fused._workspace.data_ptr(), hip.current_stream()), "pod_sgd_step_solver")
    variants = {
        "pod_sgd_step": lambda: hip.check(lib.pod_sgd_step(table, *launch, 0.0, fused.mu, fused.weight_decay, hip.current_stream()), "pod_sgd_step"),
        "solver_default": solver_call(record()),
        "solver_two_groups": solver_call(record(n_groups=2)),      # (every tensor in group 0: the step reads group[t] and the rates it indexes)
        "solver_value": solver_call(record(hip.POD_SGD_CLIP_VALUE)),
        "solver_full_model_guard": solver_call(record(hip.POD_SGD_CLIP_FULL_MODEL, 1)),
    }
    per_call = {k: [] for k in variants}
    host_call = {k: [] for k in variants}
    for r in range(args.warmup + args.reps):
        for name, call in variants.items():             # taking turns: every variant sees the same minutes of the card
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            t0 = time.perf_counter()
            for _ in range(args.calls):
                call()
            t1 = time.perf_counter()
            e1.record()
            torch.cuda.synchronize()
            if r >= args.warmup:
                per_call[name].append(e0.elapsed_time(e1) / args.calls)
                host_call[name].append(1e3 * (t1 - t0) / args.calls)
    status = fused.status()
    assert status["bad_steps"] == 0 and not status["poisoned"], status
    elements = sum(e.w.numel() for e in fused.entries)
    folded = sum(e.w.numel() for e in fused.entries if e.folded is not None)
    step_bytes = 20 * elements + 4 * folded             # g, w, m read, w, m written; the folded filter written too
    reduce_bytes = 4 * elements                         # the gradients once more (s of the folded entries is per channel: noise)
    ms = {k: stats(v) for k, v in per_call.items()}
    base, default = ms["pod_sgd_step"], ms["solver_default"]
    out = {"tensors": len(fused.entries), "elements": elements, "folded_elements": folded, "chunks": fused.table.n_chunks, "calls": args.calls, "reps": args.reps,
           "step_bytes": step_bytes, "reduce_bytes": reduce_bytes, "ms_per_call": ms, "host_ms_per_call": {k: stats(v) for k, v in host_call.items()},
           "TBps": {k: (step_bytes + (reduce_bytes if k == "solver_full_model_guard" else 0)) / (v["median"] * 1e-3) / 1e12 for k, v in ms.items()},
           "default_minus_sgd_step_ms": default["median"] - base["median"], "sgd_step_spread_ms": base["spread"],
           "default_within_spread": default["median"] - base["median"] <= base["spread"], "last_norm": status["last_norm"]}
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
