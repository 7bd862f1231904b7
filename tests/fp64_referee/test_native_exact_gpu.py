"""The HIP chain K3 .. K7 held to the fp64 referee (tests/fp64_referee/f64_ref.py), not to the fp32 oracle's own rounding.

The rule, for candidate boxes, candidate covariances, final boxes and final covariances alike (gpu_common.hold): the HIP result's
normalised error against the fp64 evaluation is at most 2x the fp32 oracle's over the same entries, in max and in rms, plus
4 fp32 ulps.  The margin is over a measurement of the REFERENCE: it admits another equally good fp32 association (another expf,
contracted multiply-adds, a lane-wise block order); a one-pass E[x^2] - E[x]^2, a dropped cascade level or a mean taken in another
order is worse by orders of magnitude at 1 300-pixel coordinates.  Figures: profiles/fp64_referee.md (GPU section)."""
import os

import pytest
import torch

from oracle import pod_oracle as po
from pod_compare_amd import hotpath, synthetic
from pod_compare_amd.probabilistic_inference import run_slice
from tests.helpers import GOLDEN, Golden, fixture_id, fixture_paths
from tests.test_hip_parity import canonical_perm, make_path, run_hip
from tests.fp64_referee import f64_ref as fr
from tests.fp64_referee import runs
from tests.fp64_referee.gpu_common import hold, hold_records

pytestmark = pytest.mark.gpu

PRE_NMS = [p for p in fixture_paths() if "post_nms" not in p]
POST_NMS = [p for p in fixture_paths() if "post_nms" in p]
NATIVE = ["cfg3_bayes_od_mc10_s31", "full_cov_standard_nms_s121", "full_worst_cfg3_bayes_od_mc10_s1006"]


def hold_final(det, run, c64):
    m = det.count()
    assert m == len(run.det) == c64.det.boxes.shape[0]
    hold("final boxes", "box", det.boxes[:m], run.det.pred_boxes, c64.det.boxes)
    hold("final cov", "cov", det.cov[:m], run.det.pred_boxes_covariance, c64.det.cov)
    hold_records(det, m, det.K)


@pytest.mark.parametrize("path", PRE_NMS, ids=fixture_id)
def test_replay_chain_is_as_close_to_fp64_as_the_reference(path):
    """eps-replay mode (k2 gather + k3_decode_cov + K4 .. K7) on every pre-NMS fixture, the full-size ones included."""
    g, p, run, levels, modes, c64 = runs.golden_run(path)
    hp, det = run_hip(g)
    aw, cand = run.aw[0], c64.cand[0]
    n = int(hp.n_total.item())
    assert n == aw.boxes.shape[0] and hp.sel_count.cpu().tolist() == aw.level_counts
    # the `same` positions of test_hip_indices_bit_exact: where the tie convention left a candidate (and its replayed normals) in place
    perm = canonical_perm(aw.anchor_idx, aw.scores, aw.level_counts)
    assert torch.equal(hp.cand_anchor_idx[:n].cpu().long(), aw.anchor_idx[perm])
    same = perm == torch.arange(n)
    assert int(same.sum()) >= n - 16
    hold("candidate boxes", "box", hp.boxes[:n].cpu()[same], aw.boxes[same], cand.boxes[same])
    if aw.cov is not None:
        hold("candidate cov", "cov", hp.cov[:n].cpu()[same], aw.cov[same], cand.cov[same])
    hold_final(det, run, c64)


@pytest.mark.parametrize("path", POST_NMS, ids=fixture_id)
def test_post_nms_ensemble_is_as_close_to_fp64_as_the_reference(path):
    """PostNmsEnsemble: every member's kept rows (K3 + the append), then the ensemble merge, the second NMS and K7."""
    g, p, run, levels, modes, c64 = runs.golden_run(path)
    hd = g.head_outputs().to("cuda")
    members = [run_slice(hd, r) for r in range(hd.num_runs)]
    hp = make_path(members[0], g.meta["topk"])
    ens = hotpath.PostNmsEnsemble(hp, len(members))
    det = ens.run([(m.cls, m.delta, m.cls_var, m.reg_var) for m in members], image_size=tuple(g.meta["image"]), out_size=tuple(g.meta["out"]),
                  eps_fn=g.eps_source())
    kept32 = [(aw.boxes[d.keep], aw.cov[d.keep], aw.classes[d.keep]) for aw, d in zip(run.aw, run.decisions)]
    kept64 = [(c.boxes[d.keep], c.cov[d.keep]) for c, d in zip(c64.cand, run.decisions)]
    total = int(ens.total.item())
    assert total == sum(x[0].shape[0] for x in kept32)
    assert torch.equal(ens.m_classes[:total].cpu().long(), torch.cat([x[2] for x in kept32]))
    hold("member rows, boxes", "box", ens.m_boxes[:total], torch.cat([x[0] for x in kept32]), torch.cat([x[0] for x in kept64]))
    hold("member rows, cov", "cov", ens.m_cov[:total], torch.cat([x[1] for x in kept32]), torch.cat([x[1] for x in kept64]))
    hold_final(det, run, c64)


class _ClsThenZeros:
    """The dumped classification normals, then zeros for the box draws (the candidate selection does not depend on them)."""

    def __init__(self, eps_cls):
        self.eps_cls, self.pos = list(eps_cls), 0

    def __call__(self, shape):
        if self.pos < len(self.eps_cls):
            t = self.eps_cls[self.pos]
            self.pos += 1
            assert tuple(t.shape) == tuple(shape)
            return t
        return torch.zeros(tuple(shape))


def native_against_fp64(hp, ho, mode, p, image, out, draw_id, modes=None, slack=4):
    """The product path on its own in-kernel draws (k23_gather_decode): the draws are dumped, as
    test_product_kernels_equal_oracle_on_their_own_draws does, the oracle and the referee run on them, and the rule is applied where
    the candidate lists coincide (all but `slack` candidates must)."""
    modes = modes or {}
    hd = ho.to("cuda")
    det = hp.run(mode, hd.cls, hd.delta, hd.cls_var, hd.reg_var, image_size=image, out_size=out, draw_id=draw_id, **modes)
    m = det.count()
    n = int(hp.n_total.item())
    nat = dict(level=hp.cand_level[:n].cpu().long(), idx=hp.cand_anchor_idx[:n].cpu().long(), boxes=hp.boxes[:n].cpu().clone(),
               cov=hp.cov[:n].cpu().clone() if hp.has_covariance else None)
    final_b, final_c = det.boxes[:m].cpu().clone(), det.cov[:m].cpu().clone()
    eps_cls = [t.cpu() for t in hp.dump_cls_normals(draw_id)] if hp.has_cls_var else []
    rl = [synthetic.to_reference_layout(ho, r) for r in range(ho.num_runs)]
    first = po.anchorwise_inference(rl[0] if len(rl) == 1 else None, p, run_outputs=rl if len(rl) > 1 else None, eps_fn=_ClsThenZeros(eps_cls))
    ref_level = torch.repeat_interleave(torch.arange(len(first.level_counts)), torch.tensor(first.level_counts))
    eps = list(eps_cls)
    if hp.cov_dims > 0:
        eps.append(hp.dump_box_normals(draw_id, torch.tensor(hp.anchor_base)[ref_level] + first.anchor_idx).cpu())
    run, levels = runs.staged(mode, rl, p, image, out, po.ReplayEps(eps), modes)
    c64 = fr.referee_chain(run, mode, torch.float64, p.box_weights, levels, image_size=image, out_size=out, **modes)
    aw, cand = run.aw[0], c64.cand[0]
    assert torch.equal(aw.anchor_idx, first.anchor_idx)
    nat_key = {(int(l), int(i)): k for k, (l, i) in enumerate(zip(nat["level"], nat["idx"]))}
    ref_key = {(int(l), int(i)): k for k, (l, i) in enumerate(zip(ref_level, aw.anchor_idx))}
    common = [k for k in nat_key if k in ref_key]
    assert n >= 100 and len(common) >= max(len(nat_key), len(ref_key)) - slack, (n, len(ref_key), len(common))
    a, b = torch.tensor([nat_key[k] for k in common]), torch.tensor([ref_key[k] for k in common])
    hold("candidate boxes", "box", nat["boxes"][a], aw.boxes[b], cand.boxes[b])
    if aw.cov is not None:
        hold("candidate cov", "cov", nat["cov"][a], aw.cov[b], cand.cov[b])
    # detections: only where the lists coincide entirely (a candidate at the threshold on one side alone changes clusters)
    if torch.equal(a, b) and len(common) == len(nat_key) == len(ref_key):
        assert m == len(run.det)
        hold("final boxes", "box", final_b, run.det.pred_boxes, c64.det.boxes)
        hold("final cov", "cov", final_c, run.det.pred_boxes_covariance, c64.det.cov)
    return n


@pytest.mark.parametrize("name", NATIVE)
def test_native_chain_is_as_close_to_fp64_as_the_reference(name):
    """k23_gather_decode's two shapes: four wavefronts per candidate (n <= K23_SMALL_MAX; D = 4 with MC runs, D = 10) and one
    wavefront per candidate (n = 4 594)."""
    g = Golden(os.path.join(GOLDEN, name + ".npz"))
    ho = g.head_outputs()
    hp = make_path(ho, g.meta["topk"])
    s = g.spec
    p = po.PathParams(num_classes=ho.num_classes, topk_candidates=g.meta["topk"])
    modes = dict(box_merge_mode=s.get("box_merge", "bayesian_inference"), cls_merge_mode=s.get("cls_merge", "max_score"))
    n = native_against_fp64(hp, ho, s["mode"], p, tuple(g.meta["image"]), tuple(g.meta["out"]), 0, modes)
    assert (n > 1024) == name.startswith("full_worst")


# ---- K3 off its workload size ---------------------------------------------------------------------------------------------------
# prop_num_samples: one sample pair (2), the 16-row block edge (15, 16, 17), cascade_combine's 256-row flush (255, 256, 257), the
# reference's 1000 (tail block of 8), all 64 lanes (1023, 1024).  Runs: 1 (no epistemic pass), 2, 17, 64 = POD_MAX_RUNS (every lane
# of the epistemic pass).  Heads: D = 4, D = 10, no reg_var head (deterministic decode + epistemic part only; S is not read).
S_ALL = (2, 15, 16, 17, 255, 256, 257, 1000, 1023, 1024)
K3_CASES = ([(s, 1, 4) for s in S_ALL] + [(s, 2, 10) for s in (2, 16, 17, 256, 257, 1000, 1024)] + [(s, 17, 4) for s in (15, 255, 1023)] +
            [(s, 64, 4) for s in (2, 1000, 1024)] + [(17, 64, 10), (15, 1, 10), (1023, 1, 10)] + [(1000, r, 0) for r in (2, 17, 64)])
K3_NATIVE = [(2, 2, 4), (17, 1, 10), (257, 17, 4), (1023, 2, 10), (1000, 64, 4)]
FRAME = (96, 128)


def _k3_setup(S, n_runs, D):
    ho = synthetic.planted_head_outputs(FRAME, n_runs, seed=500 + n_runs, num_boxes=24, with_reg_var=D > 0, cov_dims=max(D, 4))
    params = hotpath.PathParams(num_classes=ho.num_classes, num_anchors=ho.num_anchors, prop_num_samples=S)
    hp = hotpath.HotPath(ho.shapes, ho.anchors, params, n_runs=n_runs, has_cls_var=True, cov_dims=D, device="cuda")
    return ho, hp, po.PathParams(num_classes=ho.num_classes, prop_num_samples=S)


@pytest.mark.parametrize("S,n_runs,D", K3_CASES)
def test_k3_replay_off_its_workload_size(S, n_runs, D):
    ho, hp, p = _k3_setup(S, n_runs, D)
    hd = ho.to("cuda")
    det = hp.run("standard_nms", hd.cls, hd.delta, hd.cls_var, hd.reg_var, image_size=FRAME, out_size=FRAME, eps_fn=synthetic.SeededNormals(S + n_runs))
    rl = [synthetic.to_reference_layout(ho, r) for r in range(n_runs)]
    run, levels = runs.staged("standard_nms", rl, p, FRAME, FRAME, synthetic.SeededNormals(S + n_runs))
    c64 = fr.referee_chain(run, "standard_nms", torch.float64, p.box_weights, levels, image_size=FRAME, out_size=FRAME)
    aw, cand = run.aw[0], c64.cand[0]
    n = int(hp.n_total.item())
    assert n == aw.boxes.shape[0] and n >= 100
    perm = canonical_perm(aw.anchor_idx, aw.scores, aw.level_counts)
    assert torch.equal(hp.cand_anchor_idx[:n].cpu().long(), aw.anchor_idx[perm])
    same = perm == torch.arange(n)
    assert int(same.sum()) >= n - 16
    hold("candidate boxes", "box", hp.boxes[:n].cpu()[same], aw.boxes[same], cand.boxes[same])
    assert (aw.cov is None) == (D == 0 and n_runs == 1)
    if aw.cov is not None:
        hold("candidate cov", "cov", hp.cov[:n].cpu()[same], aw.cov[same], cand.cov[same])
    hold_final(det, run, c64)


@pytest.mark.parametrize("S,n_runs,D", K3_NATIVE)
def test_k23_native_off_its_workload_size(S, n_runs, D):
    """The fused gather + decode (four wavefronts fill the samples, one sums them) at odd sample counts and run counts."""
    ho, hp, p = _k3_setup(S, n_runs, D)
    native_against_fp64(hp, ho, "standard_nms", p, FRAME, FRAME, 7)
