"""Times the tail kernels (K2..K7) separately with HIP events on BASELINE-size planted inputs: tail_only.py [planted|worst].
tail_only.py streamed: K2 alone on the two shapes that reach its streamed key source, which the product geometry never does."""
import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from pod_compare_amd import hotpath, synthetic, anchors as A, hip
N = 10; dev = torch.device("cuda", 0)
synth = sys.argv[1] if len(sys.argv) > 1 else "planted"
def timeit(name, fn, iters=30):
    for _ in range(3): fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    torch.cuda._sleep(2_000_000)
    for a, b in ev:
        a.record(); fn(); b.record()
    torch.cuda.synchronize()
    ms = sorted(a.elapsed_time(b) for a, b in ev)
    print("%-22s avg %.2f us  min %.2f" % (name, 1e3 * sum(ms) / len(ms), 1e3 * ms[0]))
if synth == "streamed":
    for counts, topk in (([300000, 40000], 1000), ([2049, 40000], 1025)):     # slices beyond 16 384 keys; 2048 survivors per slice
        c2, l2 = hip.PodConfig(), (hip.PodLevel * len(counts))()
        c2.n_levels, c2.topk = len(counts), topk
        for l in range(len(counts)):
            l2[l].anchor_base = sum(counts[:l])
        g = torch.Generator().manual_seed(1)
        scores = torch.rand(sum(counts), generator=g) * 0.95 + 0.05
        saved = ((scores.view(torch.int32).to(torch.int64) << 32) | (0xFFFFFFFF - torch.arange(sum(counts)))).to(dev)
        keys, cnt = saved.clone(), torch.tensor(counts + [0] * len(counts), dtype=torch.int32, device=dev)
        out = [torch.zeros(n, dtype=t, device=dev) for n, t in ((len(counts) * topk, torch.int64), (len(counts), torch.int32),
                                                                 (len(counts) * topk, torch.int64), (len(counts) * topk, torch.int32), (1, torch.int32))]
        def k2s():
            keys.copy_(saved)                                                   # a big level's slices are compacted in place
            hip.load().pod_level_topk(c2, l2, hip.ptr(keys), hip.ptr(cnt), *[hip.ptr(o) for o in out], hip.current_stream())
        timeit("restore %s" % counts, lambda: keys.copy_(saved))
        timeit("K2 topk + restore k=%d" % topk, k2s)
    sys.exit(0)
padded = A.padded_size(*A.resize_shortest_edge(720, 1280))
h = synthetic.planted_head_outputs(padded, N, seed=1000, num_boxes=24, mode=synth, device=dev)
hp = hotpath.HotPath(h.shapes, h.anchors, hotpath.PathParams(), n_runs=N, has_cls_var=True, cov_dims=4, device=dev)
P, st, lib, cfg = hip.ptr, hip.current_stream(), hp.lib, hp.cfg
lv = hp.candidates(h.cls, h.delta, h.cls_var, h.reg_var, None)
hp.decode(lv, None); hp.nms(); torch.cuda.synchronize()
print("n =", int(hp.n_total), "keep =", int(hp.n_keep))
# K2 consumes (zeroes) the per-level counts: rebuild the candidate lists first, then put the counts back before each launch
hip.check(lib.pod_mc_merge_score(cfg, lv, P(hp.mean_cls), P(hp.mean_cls_var), None, None, P(hp.cand_keys), P(hp.cand_count), P(hp.maybe_bits), st), "k1")
hip.check(lib.pod_score_maybe(cfg, lv, P(hp.mean_cls), P(hp.mean_cls_var), P(hp.maybe_bits), P(hp.cand_keys), P(hp.cand_count), P(hp.probs_dense), st), "k1b")
saved_counts = hp.counters.clone()
saved_keys = hp.cand_keys.clone()          # a big level's slices are compacted in place
def restore():
    hp.counters.copy_(saved_counts)
    hp.cand_keys.copy_(saved_keys)
timeit("restore (2 copies)", restore)
def k2():
    restore()
    lib.pod_level_topk(cfg, lv, P(hp.cand_keys), P(hp.cand_count), P(hp.sel_keys), P(hp.sel_count), P(hp.cat_keys), P(hp.cat_level), P(hp.n_total), st)
timeit("K2 topk + restore", k2)
timeit("K2b gather", lambda: lib.pod_gather_candidates(cfg, lv, P(hp.anchors), P(hp.cat_keys), P(hp.cat_level), P(hp.n_total), P(hp.cand_count), P(hp.probs_dense), P(hp.cand_anchor_idx), P(hp.cand_level), P(hp.cand_score), P(hp.cand_class), P(hp.cand_probs), P(hp.cand_delta), P(hp.cand_reg_var), P(hp.cand_anchor), P(hp.cand_run_delta), st))
timeit("K3 decode_cov", lambda: hp.decode(lv, None))
timeit("K4 nms", lambda: hp.nms())
timeit("K5+K7 bayes_od", lambda: hp.postprocess("bayes_od", (750, 1333), (720, 1280)))
timeit("K7 std", lambda: hp.finalize(hp.keep, hp.n_keep, hp.boxes, hp.cov, hp.cand_score, hp.cand_class, hp.cand_probs, (750, 1333), (720, 1280)))
