"""GPU box: sha-256 of what the merge-and-score family (k1_mc_merge_score.hip, k1f_merge_score_fused.hip) writes on seeded inputs: run it
with two builds of the library (POD_MI355X_LIB=...) to compare them bit for bit across processes.  One digest per case and form; a digest
covers the per-level counts, the per-level sorted candidate keys, probs_dense (pre-filled with -1) and the merged planes the form stores.
Cases: the nine shape / run / K / variance rows of test_fused_merge_score_equals_the_two_launch_form x both quirks, and two dense_box_merge
cases (box_role in both K1 kernels).  Forms: K1 dense scoring, K1 prune + K1b (variance head only), K1f with planes, K1f without."""
import hashlib
import sys
import torch
sys.path.insert(0, ".")
from pod_compare_amd import hip, hotpath, synthetic  # noqa: E402

P = hip.ptr


def digest(hp, planes):
    torch.cuda.synchronize()
    counts = hp.cand_count.cpu().tolist()
    h = hashlib.sha256(repr(counts).encode())
    for b, c in zip(hp.anchor_base, counts):
        h.update(torch.sort(hp.cand_keys[b:b + c].cpu())[0].numpy().tobytes())
    for t in [hp.probs_dense] + list(planes):
        if t is not None:
            h.update(t.cpu().numpy().tobytes())
    hip.check(hp.lib.pod_reset_counters(P(hp.counters), 8, hip.current_stream()), "reset")
    return h.hexdigest()[:24]


def prepare(hp, planes):
    hip.check(hp.lib.pod_reset_counters(P(hp.counters), 8, hip.current_stream()), "reset")
    if hp.probs_dense is not None:
        hp.probs_dense.fill_(-1.0)
    for t in planes:
        if t is not None:
            t.fill_(float("nan"))


def two_launch(hp, lv, prune):
    st, planes = hip.current_stream(), (hp.mean_cls, hp.mean_cls_var, hp.mean_delta, hp.mean_reg_var)
    prepare(hp, planes)
    hip.check(hp.lib.pod_mc_merge_score(hp.cfg, lv, P(hp.mean_cls), P(hp.mean_cls_var), P(hp.mean_delta), P(hp.mean_reg_var),
                                        P(hp.cand_keys), P(hp.cand_count), P(hp.maybe_bits) if prune else None, st), "k1")
    if prune:
        hip.check(hp.lib.pod_score_maybe(hp.cfg, lv, P(hp.mean_cls), P(hp.mean_cls_var), P(hp.maybe_bits), P(hp.cand_keys), P(hp.cand_count),
                                         P(hp.probs_dense), st), "k1b")
    return digest(hp, planes)


def fused(hp, lv, store):
    planes = (hp.mean_cls, hp.mean_cls_var) if store else ()
    prepare(hp, planes)
    hip.check(hp.lib.pod_merge_score_fused(hp.cfg, lv, P(hp.mean_cls) if store else None, P(hp.mean_cls_var) if store else None, P(hp.cand_keys),
                                           P(hp.cand_count), P(hp.probs_dense), hip.current_stream()), "k1f")
    return digest(hp, planes)


# (mode, runs, K, padded, variance head, dense_box_merge)
ROWS = [("planted", 10, 7, (384, 512), True), ("worst", 3, 7, (384, 512), True), ("planted", 1, 7, (384, 512), True),
        ("planted", 2, 12, (384, 512), True), ("worst", 2, 3, (160, 224), True), ("planted", 5, 7, (96, 352), True),
        ("planted", 1, 7, (384, 512), False), ("planted", 4, 7, (160, 224), False), ("worst", 1, 7, (96, 352), False)]
CASES = [r + (False, q) for r in ROWS for q in (True, False)] + [("planted", 6, 7, (384, 512), True, True, True), ("planted", 3, 7, (96, 352), True, True, False)]
for mode, runs, K, padded, cls_var, dense, quirk in CASES:
    ho = synthetic.planted_head_outputs(padded, runs, seed=77 + runs, num_boxes=12, mode=mode, num_classes=K, with_cls_var=cls_var).to("cuda")
    params = hotpath.PathParams(num_classes=ho.num_classes, num_anchors=ho.num_anchors, merge_quirk=quirk)
    hp = hotpath.HotPath(ho.shapes, ho.anchors, params, n_runs=runs, has_cls_var=cls_var, cov_dims=4, device="cuda", dense_box_merge=dense)
    hp._begin_draw(3)
    lv = hp._levels(ho.cls, ho.delta, ho.cls_var, ho.reg_var, None)
    out = [("k1 dense", two_launch(hp, lv, False))]
    if cls_var:
        out.append(("k1 prune + k1b", two_launch(hp, lv, True)))
    out += [("k1f planes", fused(hp, lv, runs > 1)), ("k1f", fused(hp, lv, False))]
    for form, d in out:
        print("%-7s N %2d K %2d %3dx%3d var %d box %d quirk %d  %-14s %s" % (mode, runs, K, padded[0], padded[1], cls_var, dense, quirk, form, d))
