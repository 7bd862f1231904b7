"""Times K32 (pod_retinanet_infer_image: detectron2's RetinaNet.inference + detector_postprocess for one image) at the BASELINE geometry --
a 750 x 1333 network input padded to 768 x 1344, R = 193 374 anchors, K = 7 classes -- against a torch restatement of the same routine on
the same device, and reports what the scoring pass achieves against HBM peak.

What is timed, each as the median over WINDOWS windows of CALLS calls between two device events, after a warm-up window.  The scoring
pass takes microseconds, less than Python needs to enqueue it, so its calls are captured ONCE into a HIP graph of SETS (score, memset)
pairs and the windows replay that graph: the device, not Python, sets the pace.  The longer chains are enqueued from Python back to back.
  * pod_retinanet_score alone (+ the memset that re-zeroes its counters).  Its algorithmic traffic is ONE read of the logits, 4 * R * K
    bytes = 5.4 MB -- which a 256 MB last-level cache would serve from the second call on.  So the calls ROTATE through SETS seeded inputs,
    SETS * 5.4 MB > 2 x the cache: every call reads its logits from HBM.  bytes / time is given against the 8.0 TB/s specification and the
    6.29 TB/s a float4 copy has been measured to reach on an MI355X.  The same call on ONE input (cache-resident) is
    given beside it: the difference is what HBM costs.
  * pod_retinanet_infer_image, the five launches of one image, rotating through the same inputs.
  * the torch restatement on the device: per level flatten().sigmoid_(), sort(descending=True), [:topk], the threshold, // K, % K, the
    delta gather and apply_deltas; the level concatenation.  It stops BEFORE the NMS: torchvision is not a dependency of this project,
    and a host-driven greedy NMS would time the host.  The K32 figure to set beside it is `score + topk + decode`, timed stage by stage.
Logits are N(-5.2, 1.6): 2 % of the (anchor, class) pairs pass the 0.05 threshold, 27 000 of 1.35 M, every level but the last two beyond
topk = 1000.

    python tools/retinanet_inference_bench.py [--out profiles/train_eval.json]
"""
import argparse
import json
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pod_compare_amd import anchors as _anchors, hip      # noqa: E402
from pod_compare_amd.retinanet_inference import InferenceParams, RetinaNetInference      # noqa: E402

K, A = 7, 9
FRAME, OUT = (750, 1333), (720, 1280)
WINDOWS, CALLS, SETS = 10, 960, 96         # 96 x 5.4 MB = 520 MB of logits in rotation
HBM_SPEC, HBM_COPY = 8.0e12, 6.29e12
SCALE_CLAMP = math.log(1000.0 / 16)


def timed(call, sync, calls=0):
    CALLS = calls or globals()["CALLS"]
    for i in range(min(CALLS, 2 * SETS)):
        call(i)
    sync()
    out = []
    for _ in range(WINDOWS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(CALLS):
            call(i)
        e1.record()
        sync()
        out.append(e0.elapsed_time(e1) / CALLS)
    return {"median_ms": statistics.median(out), "min_ms": min(out), "max_ms": max(out), "calls": WINDOWS * CALLS}


def graphed(body, dev):
    """`body(i)` for i < SETS captured into one HIP graph; returns call(i) for `timed`: every SETS-th call replays the graph."""
    body(0)
    torch.cuda.current_stream().synchronize()
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side, capture_error_mode="thread_local"):
        for i in range(SETS):
            body(i)
    torch.cuda.current_stream().wait_stream(side)
    return lambda i: graph.replay() if i % SETS == 0 else None


def torch_restatement(cls, delta, anchors, topk=1000, thresh=0.05):
    """inference_single_image up to the level concatenation, as detectron2 writes it, on the tensors' device."""
    boxes_all, scores_all, classes_all = [], [], []
    for c, d, a in zip(cls, delta, anchors):
        AK, H, W = c.shape[-3:]
        prob = c.reshape(AK // K, K, H, W).permute(2, 3, 0, 1).flatten().sigmoid_()
        dl = d.reshape(AK // K, 4, H, W).permute(2, 3, 0, 1).reshape(-1, 4)
        num_topk = min(topk, prob.numel())
        predicted_prob, topk_idxs = prob.sort(descending=True)
        predicted_prob, topk_idxs = predicted_prob[:num_topk], topk_idxs[:num_topk]
        keep = predicted_prob > thresh
        predicted_prob, topk_idxs = predicted_prob[keep], topk_idxs[keep]
        anchor_idxs, classes = topk_idxs // K, topk_idxs % K
        dsel, asel = dl[anchor_idxs], a[anchor_idxs]
        w, h = asel[:, 2] - asel[:, 0], asel[:, 3] - asel[:, 1]
        cx, cy = asel[:, 0] + 0.5 * w, asel[:, 1] + 0.5 * h
        pcx, pcy = dsel[:, 0] * w + cx, dsel[:, 1] * h + cy
        pw, ph = torch.exp(dsel[:, 2].clamp(max=SCALE_CLAMP)) * w, torch.exp(dsel[:, 3].clamp(max=SCALE_CLAMP)) * h
        boxes_all.append(torch.stack((pcx - 0.5 * pw, pcy - 0.5 * ph, pcx + 0.5 * pw, pcy + 0.5 * ph), dim=1))
        scores_all.append(predicted_prob)
        classes_all.append(classes)
    return torch.cat(boxes_all), torch.cat(scores_all), torch.cat(classes_all)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default="")
    ap.add_argument("--device", default="cuda:0")
    args = ap.parse_args(argv)
    dev = torch.device(args.device)
    torch.cuda.set_device(dev)
    shapes = _anchors.level_shapes(*_anchors.padded_size(*FRAME))
    anchors = _anchors.grid_anchors(shapes, device=dev)
    R = sum(h * w * A for h, w in shapes)
    assert R == 193374, R
    g = torch.Generator(device=dev).manual_seed(32)
    cls_sets = [[torch.randn(A * K, h, w, device=dev, generator=g) * 1.6 - 5.2 for h, w in shapes] for _ in range(SETS)]
    delta = [torch.randn(A * 4, h, w, device=dev, generator=g) * 0.3 for h, w in shapes]
    ri = RetinaNetInference(shapes, anchors, InferenceParams(num_classes=K, num_anchors=A), device=dev)
    levels = [ri.levels(c, delta) for c in cls_sets]
    keep_alive = list(cls_sets)
    lib = hip.load()
    sync = lambda: torch.cuda.current_stream().synchronize()
    P = hip.ptr
    out = ri.new_detections()

    def score(lv):
        hip.check(lib.pod_retinanet_score(ri.cfg, lv, P(ri.cand_keys), P(ri.cand_count), hip.current_stream()), "pod_retinanet_score")

    def reset():
        hip.check(lib.pod_reset_counters(P(ri.counters), int(ri.counters.numel()), hip.current_stream()), "pod_reset_counters")

    def score_reset(i, rotate=True):
        score(levels[i % SETS if rotate else 0])
        reset()

    def three_stages(i):
        lv = levels[i % SETS]
        score(lv)
        ri.topk(lv)
        ri.decode(lv)

    score(levels[0])
    sync()
    above = ri.cand_count.cpu().tolist()
    reset()
    res = {"geometry": {"frame": list(FRAME), "levels": [list(s) for s in shapes], "anchors": R, "classes": K, "entries": R * K},
           "candidates_per_level_set0": above, "windows": WINDOWS, "calls_per_window": CALLS, "input_sets_in_rotation": SETS,
           "logit_bytes_per_image": 4 * R * K}
    res["reset_counters_alone"] = timed(graphed(lambda i: reset(), dev), sync)
    res["score_rotating_inputs"] = timed(graphed(score_reset, dev), sync)
    res["score_one_input_cache_resident"] = timed(graphed(lambda i: score_reset(i, rotate=False), dev), sync)
    t = (res["score_rotating_inputs"]["median_ms"] - res["reset_counters_alone"]["median_ms"]) * 1e-3
    res["score_bytes_per_second"] = 4 * R * K / t
    res["score_fraction_of_hbm_spec_8.0TBps"] = res["score_bytes_per_second"] / HBM_SPEC
    res["score_fraction_of_float4_copy_6.29TBps"] = res["score_bytes_per_second"] / HBM_COPY
    res["score_topk_decode"] = timed(three_stages, sync)
    res["infer_image"] = timed(lambda i: ri.infer_levels(levels[i % SETS], FRAME, OUT, out), sync)
    res["detections_last_image"] = int(out.n.item())
    with torch.no_grad():
        res["torch_restatement_before_nms"] = timed(lambda i: torch_restatement(cls_sets[i % SETS], delta, anchors), sync, calls=SETS)
        # the two agree on what they select (the restatement's sort is unstable: equal sets, and equal order where no two scores are equal)
        b, s, c = torch_restatement(cls_sets[0], delta, anchors)
        three_stages(0)
        sync()
        n = int(ri.n_total.item())
        res["selected_k32"], res["selected_torch"] = n, int(s.numel())
        res["max_abs_box_difference"] = float((ri.boxes[:n] - b).abs().max()) if n == s.numel() and bool((ri.classes[:n].long() == c).all()) else None
    print(json.dumps(res, indent=1))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
    del keep_alive
    return res


if __name__ == "__main__":
    main()
