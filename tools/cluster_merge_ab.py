"""GPU box: compare two builds of the library on the cluster-merge kernels (K5 bayes_fuse, K6 anchor_stats and the post-NMS
ensemble merge), bit for bit and by launch time:

    POD_MI355X_LIB=<lib> python tools/cluster_merge_ab.py [--time] [--full]

Hashes (always): every case runs through HotPath.run / PostNmsEnsemble.run in eps-replay mode; per case one sha256 over the merged
rows (m_* below n_keep, or the ensemble's c_* below n_seeds) and one over the DeviceDetections fields below n_det.  Two builds that
print the same table computed the same bits.  Cases: the four BayesOD merge combinations and the two anchor_statistics forms of
tests/test_hip_edge_cases.py (765 candidates), and every fixture of tests/golden that runs bayes_od, anchor_statistics or a
post-NMS merge (--full adds the full-size ones).
--time: HIP events around each single launch of pod_bayes_fuse (both box modes), pod_anchor_stats_merge and pod_ensemble_merge
on the workspace a case left behind, 300 launches after 30 of warm-up, five repeats: median per repeat, then their median and range."""
import hashlib
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pod_compare_amd import hip, hotpath, synthetic  # noqa: E402
from pod_compare_amd.probabilistic_inference import run_slice  # noqa: E402
from tests.helpers import Golden, fixture_id, fixture_paths  # noqa: E402

BOX_MODES, CLS_MODES = ("bayesian_inference", "covariance_intersection"), ("max_score", "bayesian_inference")


def sha(tensors) -> str:
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()[:16]


def make_path(ho, topk=1000):
    params = hotpath.PathParams(num_classes=ho.num_classes, num_anchors=ho.num_anchors, topk_candidates=topk)
    cov_dims = 0 if ho.reg_var is None else ho.reg_var[0].shape[1] // ho.num_anchors
    return hotpath.HotPath(ho.shapes, ho.anchors, params, n_runs=ho.num_runs, has_cls_var=ho.cls_var is not None, cov_dims=cov_dims, device="cuda")


def det_hash(det):
    m = det.count()
    return m, sha([det.boxes[:m], det.cov[:m], det.scores[:m], det.classes[:m], det.probs[:m], det.records[:m]])


def run_pre_nms(ho, mode, image, out, eps, topk=1000, **kw):
    hp = make_path(ho, topk)
    hd = ho.to("cuda")
    det = hp.run(mode, hd.cls, hd.delta, hd.cls_var, hd.reg_var, image_size=image, out_size=out, eps_fn=eps, **kw)
    nk = int(hp.n_keep.item())
    merged = sha([hp.m_boxes[:nk], hp.m_cov[:nk], hp.m_scores[:nk], hp.m_classes[:nk], hp.m_probs[:nk]])
    return hp, (int(hp.n_total.item()), nk, merged) + det_hash(det)


def run_post_nms(ho, image, out, eps, topk=1000):
    """eps None: native draws with a fixed key (the timing inputs; the hashed cases replay eps)."""
    hd = ho.to("cuda")
    members = [run_slice(hd, r) for r in range(ho.num_runs)]
    hp = make_path(members[0], topk)
    ens = hotpath.PostNmsEnsemble(hp, len(members))
    det = ens.run([(m.cls, m.delta, m.cls_var, m.reg_var) for m in members], image_size=image, out_size=out, eps_fn=eps,
                  draw_id=0 if eps is None else None)
    ns = int(ens.n_seeds.item())
    merged = sha([ens.c_boxes[:ns], ens.c_cov[:ns], ens.c_scores[:ns], ens.c_classes[:ns], ens.c_probs[:ns]])
    return ens, (int(ens.total.item()), ns, merged) + det_hash(det)


def launch_times(name, launch, repeats=5, warm=30, n=300):
    meds = []
    for _ in range(repeats):
        for _ in range(warm):
            launch()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
        for a, b in ev:
            a.record()
            launch()
            b.record()
        torch.cuda.synchronize()
        meds.append(statistics.median(a.elapsed_time(b) * 1e3 for a, b in ev))
    print("time | %-44s | median %7.2f us | repeats %7.2f .. %7.2f" % (name, statistics.median(meds), min(meds), max(meds)), flush=True)


def time_path(tag, hp):
    """Single launches on what hp.run left in the workspace (candidates, keep list)."""
    lib, cfg, P, st = hp.lib, hp.cfg, hip.ptr, hip.current_stream()
    outs = (P(hp.m_boxes), P(hp.m_cov), P(hp.m_scores), P(hp.m_classes), P(hp.m_probs))
    if hp.has_covariance:
        for bm in (0, 1):
            launch_times("%s pod_bayes_fuse box_mode=%d" % (tag, bm), lambda: hip.check(lib.pod_bayes_fuse(
                cfg, P(hp.n_total), P(hp.keep), P(hp.n_keep), P(hp.boxes), P(hp.cov), P(hp.cand_score), P(hp.cand_class), P(hp.cand_probs),
                bm, 1, *outs, st), "pod_bayes_fuse"))
    cov = P(hp.cov) if hp.has_covariance else None
    launch_times("%s pod_anchor_stats_merge" % tag, lambda: hip.check(lib.pod_anchor_stats_merge(
        cfg, P(hp.n_total), P(hp.keep), P(hp.n_keep), P(hp.boxes), cov, P(hp.cand_class), P(hp.cand_probs), *outs, st), "pod_anchor_stats_merge"))


def time_ensemble(tag, ens):
    hp, P, st = ens.hp, hip.ptr, hip.current_stream()
    launch_times("%s pod_ensemble_merge" % tag, lambda: hip.check(hp.lib.pod_ensemble_merge(
        hp.cfg, P(ens.total), ens.cap, P(ens.m_boxes), P(ens.m_cov), P(ens.m_classes), P(ens.m_probs), P(ens.seeds), P(ens.n_seeds),
        P(ens.c_boxes), P(ens.c_cov), P(ens.c_scores), P(ens.c_classes), P(ens.c_probs), st), "pod_ensemble_merge"))


def main():
    timing, full = "--time" in sys.argv, "--full" in sys.argv or "--time" in sys.argv
    print("library:", hip.library_path())
    print("hash | case | candidates | centres | merged rows | detections | DeviceDetections")
    row = lambda name, r: print("hash | %s | %d | %d | %s | %d | %s" % ((name,) + r), flush=True)
    size = (256, 320)
    ho = synthetic.planted_head_outputs(size, 3, seed=5, num_boxes=40)
    timed = []
    for bm in BOX_MODES:
        for cm in CLS_MODES:
            hp, r = run_pre_nms(ho, "bayes_od", size, size, synthetic.SeededNormals(5), box_merge_mode=bm, cls_merge_mode=cm)
            row("bayes_od %s / %s" % (bm, cm), r)
            if (bm, cm) == (BOX_MODES[0], CLS_MODES[0]):
                timed.append(("n=%d" % r[0], hp))      # the launches are timed on this run's candidates and keep list
    hp, r = run_pre_nms(ho, "anchor_statistics", size, size, synthetic.SeededNormals(5))
    row("anchor_statistics 3 runs, variance heads", r)
    plain = synthetic.planted_head_outputs(size, 1, seed=5, num_boxes=40, with_cls_var=False, with_reg_var=False)
    hp, r = run_pre_nms(plain, "anchor_statistics", size, size, synthetic.SeededNormals(5))
    row("anchor_statistics 1 run, no variance head", r)
    timed.append(("n=%d plain" % r[0], hp))
    full3 = None
    for path in fixture_paths():
        g = Golden(path)
        s = g.spec
        if "/full_" in path and not full:
            continue
        image, out = tuple(g.meta["image"]), tuple(g.meta["out"])
        if s.get("post_nms"):
            _, r = run_post_nms(g.head_outputs(), image, out, g.eps_source(), g.meta["topk"])
        elif s["mode"] in ("bayes_od", "anchor_statistics"):
            hp, r = run_pre_nms(g.head_outputs(), s["mode"], image, out, g.eps_source(), g.meta["topk"],
                                box_merge_mode=s.get("box_merge", "bayesian_inference"), cls_merge_mode=s.get("cls_merge", "max_score"))
            if fixture_id(path).startswith("full_cfg3"):
                timed.append(("full_cfg3 n=%d" % r[0], hp))
                full3 = (g.head_outputs(), image, out)
        else:
            continue
        row(fixture_id(path), r)
    if timing:
        for tag, hp in timed:
            time_path(tag, hp)
        for tag, (mho, image, out) in (("n=765 case, 3 members", (ho, size, size)), ("full_cfg3, 10 members", full3)):
            ens, r = run_post_nms(mho, image, out, None)
            time_ensemble("%s: m=%d, %d seeds" % (tag, r[0], r[1]), ens)


if __name__ == "__main__":
    main()
