"""Times the comparison pass (probabilistic_inference.build_comparison) against the same configs run one predictor at a time, at the
BASELINE shape: synthetic 1280 x 720 frames, network input 750 x 1333, random-init weights, the forwards replayed as HIP graphs as
apply_net replays them, ONE stream (the two sides are then the same schedule but for what is shared).

Two sets of configs on the reg_cls_var_dropout model:
  * six: standard_nms, anchor_statistics, bayes_od, bayes_od_mc_dropout, mc_dropout_ensembles_pre_nms / post_nms (10 MC runs);
  * bench: the inference sides of bench.py's configs 1, 2 and 4 -- bayes_od, bayes_od_mc_dropout, ensembles_pre_nms (5 members).
For each: every config's predictor alone (the sum is "separately"), the same predictors taking turns frame by frame, then the
comparison over the same frames ("shared"): the median over WINDOWS windows of IMAGES frames after WARMUP, milliseconds per image from
the host clock around a device synchronisation, and the windows' spread; the post-processing launches per image (4 per front, 1 tail
launch for standard NMS, 2 for the fusing modes; the post-NMS merges counted from their member loop), model evaluations per image, and
the peak of torch's allocator.  The expectation checked: shared <= the sum over families of the slowest member's own time + a tail
(measured as bayes_od's share beyond standard_nms) per further config.

    python tools/compare_pass_bench.py [--out profiles/compare_pass.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pod_compare_amd import comparison, config, modeling, synthetic      # noqa: E402
from pod_compare_amd.probabilistic_inference import build_comparison, build_model, build_predictor      # noqa: E402

CONFIGS = os.path.join(os.path.dirname(os.path.abspath(config.__file__)), "configs")
MODEL = os.path.join(CONFIGS, "BDD-Detection", "retinanet", "retinanet_R_50_FPN_1x_reg_cls_var_dropout.yaml")
SETS = {"six": ("standard_nms", "anchor_statistics", "bayes_od", "bayes_od_mc_dropout", "mc_dropout_ensembles_pre_nms", "mc_dropout_ensembles_post_nms"),
        "bench": ("bayes_od", "bayes_od_mc_dropout", "ensembles_pre_nms")}
IMAGES, WARMUP, FRAMES, WINDOWS = 50, 8, 5, 5


def cfg_of(name, dev):
    cfg = config.setup_config(MODEL, os.path.join(CONFIGS, "Inference", name + ".yaml"))
    cfg.MODEL.WEIGHTS, cfg.OUTPUT_DIR, cfg.MODEL.DEVICE = "", "", dev
    return cfg


def graphs(*ms):
    for m in ms:
        m.enable_graphs(True)
        m.graph_after_seen = 2


def timed(call, inputs):
    """ms per image, the median of WINDOWS windows of IMAGES calls after WARMUP (eager forwards, then the captures); the spread of the
    windows (max - min); the allocator's peak during them."""
    with torch.no_grad():
        for i in range(WARMUP):
            call(inputs[i % FRAMES])
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        out = []
        for _ in range(WINDOWS):
            t = time.perf_counter()
            for i in range(IMAGES):
                call(inputs[i % FRAMES])
            torch.cuda.synchronize()
            out.append(1e3 * (time.perf_counter() - t) / IMAGES)
        return statistics.median(out), max(out) - min(out), torch.cuda.max_memory_allocated() / 2 ** 20


def tail_launches(cfg) -> int:
    return 1 if cfg.PROBABILISTIC_INFERENCE.INFERENCE_MODE not in ("bayes_od", "anchor_statistics") else 2


def own_launches(cfg, members) -> int:
    """Post-processing launches of a config's own run: one front + its tail; post-NMS: per member K1f, K2, gather, decode, NMS, append,
    then the merge's two launches, the second NMS and K7."""
    if comparison.is_post_nms(cfg):
        return 6 * members + 4
    return 4 + tail_launches(cfg)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default="")
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--sets", nargs="+", default=["six", "bench"], choices=sorted(SETS))      # (six first: no ensemble member resident yet)
    args = ap.parse_args(argv)
    torch.cuda.set_device(torch.device(args.device))
    torch.manual_seed(0)
    model = build_model(cfg_of("standard_nms", args.device), load_weights=False)
    members = []
    res = {"images": IMAGES, "windows": WINDOWS, "warmup": WARMUP, "frame": [720, 1280], "streams": 1}
    inputs = []
    for i in range(FRAMES):
        frame = synthetic.synthetic_frame(i, device=args.device)
        inputs.append([{"image": modeling.resize_test_image(frame, 800, 1333), "height": 720, "width": 1280, "image_id": i}])
    for name in args.sets:
        cfgs = [cfg_of(n, args.device) for n in SETS[name]]
        if any(c.PROBABILISTIC_INFERENCE.INFERENCE_MODE == "ensembles" for c in cfgs) and not members:
            for seed in cfgs[0].PROBABILISTIC_INFERENCE.ENSEMBLES.RANDOM_SEED_NUMS:
                torch.manual_seed(int(seed))
                members.append(build_model(cfgs[0], load_weights=False))
        graphs(model, *members)
        one, alone = {}, []
        for n, cfg in zip(SETS[name], cfgs):
            p = build_predictor(cfg, model=model, model_list=members or None)
            p.return_device, p.sparse_bbox_tower = True, True
            alone.append(p)
            n_members = len(members) if cfg.PROBABILISTIC_INFERENCE.INFERENCE_MODE == "ensembles" else p.num_mc_dropout_runs
            ms, spread, peak = timed(p, inputs)
            one[n] = {"ms_per_image": ms, "window_spread_ms": spread, "peak_MiB": peak, "postprocessing_launches": own_launches(cfg, n_members)}
            model._drop_graphs()
        # the same predictors taking turns on every frame: the comparison's order of forwards with nothing shared (what alternating between
        # graphs and models costs by itself -- their filters displace each other in the last-level cache -- is in this figure, not in the sum)
        turns_ms, turns_spread, _ = timed(lambda im: [p(im) for p in alone], inputs)
        model._drop_graphs()
        cmp = build_comparison(cfgs, model=model, model_list=members or None)
        cmp.return_device, cmp.sparse_bbox_tower = True, True
        ms, spread, peak = timed(cmp, inputs)
        fams = cmp.families
        launches = 0
        for f in fams:
            for s in f.subfamilies:
                if s.kind == "merged":
                    launches += 4 + sum(tail_launches(cfgs[i]) for i in s.members)
                else:
                    launches += sum(own_launches(cfgs[i], len(members) if f.key[0] == "ensembles" else f.key[2]) for i in s.members)
        slowest = sum(max(one[SETS[name][i]]["ms_per_image"] for i in f.members) for f in fams)
        tail_ms = max(0.0, one["bayes_od"]["ms_per_image"] - one.get("standard_nms", one["bayes_od"])["ms_per_image"])
        bound = slowest + tail_ms * sum(len(f.members) - 1 for f in fams)
        res[name] = {"configs": list(SETS[name]), "separately": one, "separately_ms_per_image": sum(v["ms_per_image"] for v in one.values()),
                     "separately_postprocessing_launches": sum(v["postprocessing_launches"] for v in one.values()),
                     "separately_taking_turns_ms_per_image": turns_ms, "separately_taking_turns_window_spread_ms": turns_spread,
                     "shared_ms_per_image": ms, "shared_window_spread_ms": spread, "shared_peak_MiB": peak, "shared_postprocessing_launches": launches,
                     "families": [{"key": list(map(str, f.key)), "configs": [SETS[name][i] for i in f.members], "fronts": len(f.subfamilies)} for f in fams],
                     "model_evaluations_per_image": {"separately": len(cfgs), "shared": len(fams)},
                     "expectation_ms_per_image": bound, "expectation_met": ms <= bound}
        model._drop_graphs()
    print(json.dumps(res, indent=1))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
    return res


if __name__ == "__main__":
    main()
