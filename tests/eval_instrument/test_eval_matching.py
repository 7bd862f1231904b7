"""pod_match_groundtruth (k_match_gt, k_match_det) and its host mirror against a brute-force referee, at the smallest shapes at which
they can go wrong: both lane trips of k_match_gt, 128 hits on one box, score ties, IoUs exactly on a threshold and one ulp beside it,
shared detections, image offsets, empty tensors, K != 7, thousands of blocks.

CPU (unmarked): the referees themselves -- match_ref against the oracle (and through it the reference's recorded output), the cases'
intended outcomes, no seeded pair within 1e-5 of a threshold, the fp32 threshold facts, nll_ref against the reference's own fp32
MultivariateNormal where that one is accurate.
GPU: (a) the C ABI's raw outputs into sentinel-filled buffers, integers equal, IoUs bit-equal, nothing written past `count`;
(b) evaluation_utils.match_predictions_to_groundtruth's four partitions torch.equal to the oracle's."""
import numpy as np
import pytest
import torch

from oracle import pod_oracle as po
from tests.eval_instrument import instrument_ref as ir
from tests.test_eval_matching import check, load

ALL = sorted(ir.CASES)


# ---------------------------------------------------------------------------------------------------------------------------------
# CPU: the referees
# ---------------------------------------------------------------------------------------------------------------------------------

def test_match_ref_equals_oracle_and_recorded_reference_output():
    z, pb, pp, pc, gb, gc = load()
    p = ir.pack(pb, pp, pc, gb, gc)
    res = ir.partitions(p, ir.match_ref(p.det_boxes, p.det_probs, p.det_off, p.gt_boxes, p.gt_off, 0.1, 0.7))
    want = po.match_predictions_to_groundtruth(pb, pp, pc, gb, gc, 0.1, 0.7)
    for part in want:
        for name, ref in want[part].items():
            assert tuple(res[part][name].shape) == tuple(ref.shape) and torch.equal(res[part][name].double(), ref.double()), (part, name)
    check(res, z)
    assert min(ir.part_counts(res)) > 0


@pytest.mark.parametrize("name", ALL)
def test_match_ref_equals_oracle(name):
    c, p, raw, want = ir.case(name)
    ir.assert_partitions_equal(ir.partitions(p, raw), want, name)
    print(name, "TP / duplicates / FP / FN:", ir.part_counts(want), "pairs:", ir.undecided_pairs(p.det_boxes, p.det_off, p.gt_boxes, p.gt_off, 0.1, 0.7)[1])


@pytest.mark.parametrize("name", sorted(ir.SEEDED))
def test_seeded_sets_have_no_undecided_pair(name):
    """A condition on the inputs, not a tolerance: with it, exact equality is owed by every correct implementation."""
    c, p, raw, want = ir.case(name)
    close, total = ir.undecided_pairs(p.det_boxes, p.det_off, p.gt_boxes, p.gt_off, 0.1, 0.7)
    print(name, "undecided", close, "of", total)
    assert close == 0 and total > 0
    if name.startswith("mixed"):
        assert total == 6276 and min(ir.part_counts(want)) > 0, (total, ir.part_counts(want))
    if name == "many_images":
        # thousands of k_match_gt blocks; 1500 images x 10 detections on average are 57 k_match_det blocks of 256
        assert p.gt_boxes.shape[0] > 2000 and p.det_boxes.shape[0] > 50 * 256, (p.gt_boxes.shape, p.det_boxes.shape)


def test_undecided_pairs_counts_a_pair_on_the_threshold():
    c, p, raw, want = ir.case("thresholds_exact")
    assert ir.undecided_pairs(p.det_boxes, p.det_off, p.gt_boxes, p.gt_off, 0.1, 0.7) == (6, 6)


def test_threshold_facts_fp32():
    f = np.float32
    assert f(70) / f(100) == f(0.7) and f(10) / f(100) == f(0.1)
    iou = ir.iou_f32(np.array([[0, 0, 10, 10]], f), np.stack(ir.threshold_boxes()))[0]
    assert iou.dtype == f
    assert iou[0] == f(0.7) and iou[1] > f(0.7) and iou[2] < f(0.7)
    assert iou[3] == f(0.1) and iou[4] > f(0.1) and iou[5] < f(0.1)
    assert iou[1] - f(0.7) <= 2 * np.spacing(f(0.7)) and f(0.7) - iou[2] <= 2 * np.spacing(f(0.7))         # neighbours, not strangers
    assert iou[4] - f(0.1) <= 2 * np.spacing(f(0.1)) and f(0.1) - iou[5] <= 2 * np.spacing(f(0.1))
    assert iou[4] < f(0.1) + f(1e-6)                     # a threshold padded by 1e-6 would take this one for missed


def test_cases_are_what_they_claim():
    raw = lambda n: ir.case(n)[2]
    r = raw("thresholds_exact")          # >= 0.7 hits; <= 0.1 is missed, for the box and for the detection
    assert r["gt_match_count"].tolist() == [1, 1, 0, 0, 0, 0] and r["gt_fn"].tolist() == [0, 0, 0, 1, 0, 1] and r["det_fp"].tolist() == [0, 0, 0, 1, 0, 1]
    r, p = raw("lane_trips"), ir.case("lane_trips")[1]
    assert r["gt_fn"].tolist() == [1] + [0] * 14 and r["gt_match_count"].tolist() == [0] + [1, 0] * 7
    assert [i[0] for i in r["gt_match_idx"] if i] == [int(p.det_off[m + 1]) - 1 for m in range(1, 15, 2)]
    assert int(r["det_fp"].sum()) == p.det_boxes.shape[0] - 14
    for n in ("all_hit_128_distinct", "all_hit_128_quantised"):
        r, p = raw(n), ir.case(n)[1]
        sc = p.det_probs.max(1)[r["gt_match_idx"][0]]
        assert r["gt_match_count"].tolist() == [128] and sorted(r["gt_match_idx"][0]) == list(range(128))
        assert all(sc[i] > sc[i + 1] or (sc[i] == sc[i + 1] and r["gt_match_idx"][0][i] < r["gt_match_idx"][0][i + 1]) for i in range(127))
        assert (len(set(sc.tolist())) == 128) == (n == "all_hit_128_distinct") and len(set(sc.tolist())) >= 8
    r = raw("shared_detection")
    assert r["gt_match_idx"] == [[0], [0]] and r["det_fp"].tolist() == [0, 1] and r["gt_fn"].tolist() == [0, 0]
    r = raw("cross_image")
    assert r["gt_match_count"].tolist() == [1, 1, 0, 0, 0, 0, 1, 1] and r["gt_fn"].tolist() == [0, 0, 1, 1, 1, 1, 0, 0] and r["det_fp"].tolist() == r["gt_fn"].tolist()
    r = raw("degenerate")
    assert r["gt_match_count"].tolist() == [0] * 4 and r["gt_fn"].tolist() == [1] * 4 and r["det_fp"].tolist() == [1] * 5
    p = ir.case("empties")[1]
    assert p.det_off.tolist() == [0, 1, 3, 3, 4] and p.gt_off.tolist() == [0, 0, 0, 2, 3]
    assert ir.part_counts(ir.case("empties")[3]) == (1, 0, 3, 2)
    for k in ir.CLASS_COUNTS:
        p = ir.case("class_counts_K%d" % k)[1]
        assert p.K == k and int((p.det_probs.argmax(1) == k - 1).sum()) >= p.det_boxes.shape[0] // 3


@pytest.mark.parametrize("family", ir.NLL_FAMILIES)
def test_nll_ref_against_the_fp32_reference(family):
    """Every family has cond(Sigma) <= 1e6 (asserted: the fp64 factorisation's error is then <= 1e-9); where the reference's fp32
    MultivariateNormal is accurate (wishart) the two agree within 1e-4.  Its deviation elsewhere is printed, not asserted: it is the
    reason the kernel is judged by nll_ref and not by it."""
    means, covs, gt = ir.nll_family(family, 257)
    cond = float(ir.nll_cond(covs).max())
    ref = ir.nll_ref(means, covs, gt)
    assert cond <= ir.NLL_COND_MAX and bool(torch.isfinite(ref).all()), cond
    for n in ir.NLL_SIZES + ((ir.NLL_LARGE,) if family == "wishart" else ()):          # every set the GPU tests use
        assert float(ir.nll_cond(ir.nll_family(family, n)[1]).max()) <= ir.NLL_COND_MAX, (family, n)
    try:
        dev = float((po.reg_nll(means, covs, gt).double() - ref).abs().max())
    except ValueError as e:                # torch's fp32 factorisation can refuse a covariance this ill-conditioned outright
        dev = "refused (%s)" % str(e).splitlines()[0][:60]
    print("%-8s cond(Sigma) <= %.3g, max |ref| %.4g, fp32 MultivariateNormal - fp64: %s" % (family, cond, float(ref.abs().max()), dev))
    if family == "wishart":
        assert dev <= 1e-4, dev


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------------------

def run_abi(p: ir.Packed, iou_min=0.1, iou_correct=0.7):
    """pod_match_groundtruth into buffers filled with the sentinel; returns them whole, on the host."""
    from pod_compare_amd import hip
    lib = hip.load()
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    D, G = p.det_boxes.shape[0], p.gt_boxes.shape[0]
    db, dp, do, di, gb, go, gi = (dev(a) for a in (p.det_boxes, p.det_probs, p.det_off, p.det_img, p.gt_boxes, p.gt_off, p.gt_img))
    full = lambda shape, dt: torch.full(shape, ir.SENTINEL, dtype=dt, device="cuda")
    out = {"gt_fn": full((max(G, 1),), torch.int32), "gt_match_count": full((max(G, 1),), torch.int32),
           "gt_match_idx": full((max(G, 1), ir.MATCH_MAX_DET), torch.int32), "gt_match_iou": full((max(G, 1), ir.MATCH_MAX_DET), torch.float32),
           "det_fp": full((max(D, 1),), torch.int32)}
    P = hip.ptr
    hip.check(lib.pod_match_groundtruth(P(db), P(dp), P(do), P(di), D, P(gb), P(go), P(gi), G, max(p.K, 1), float(iou_min), float(iou_correct),
                                        P(out["gt_fn"]), P(out["gt_match_count"]), P(out["gt_match_idx"]), P(out["gt_match_iou"]),
                                        P(out["det_fp"]), hip.current_stream()), "pod_match_groundtruth")
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


@pytest.mark.gpu
@pytest.mark.parametrize("name", ALL)
def test_abi_raw_outputs(name):
    c, p, raw, want = ir.case(name)
    got = run_abi(p)
    D, G = p.det_boxes.shape[0], p.gt_boxes.shape[0]
    assert got["gt_fn"][:G].tolist() == raw["gt_fn"].tolist(), name
    assert got["gt_match_count"][:G].tolist() == raw["gt_match_count"].tolist(), name
    assert got["det_fp"][:D].tolist() == raw["det_fp"].tolist(), name
    for k, n in (("gt_fn", G), ("gt_match_count", G), ("det_fp", D)):          # nothing written past the rows that exist
        assert (got[k][n:] == ir.SENTINEL).all(), (name, k)
    for g in range(G):
        n = int(raw["gt_match_count"][g])
        assert got["gt_match_idx"][g, :n].tolist() == raw["gt_match_idx"][g], (name, g)
        assert got["gt_match_iou"][g, :n].view(np.int32).tolist() == raw["gt_match_iou"][g].view(np.int32).tolist(), (name, g)      # bit-equal
    rank = np.arange(ir.MATCH_MAX_DET)[None, :]
    past = rank >= np.concatenate([raw["gt_match_count"], np.zeros(max(G, 1) - G, np.int32)])[:, None]
    assert (got["gt_match_idx"][past] == ir.SENTINEL).all() and (got["gt_match_iou"][past] == np.float32(ir.SENTINEL)).all(), name


@pytest.mark.gpu
@pytest.mark.parametrize("name", ALL)
def test_mirror_partitions(name):
    from pod_compare_amd import evaluation_utils as ev
    c, p, raw, want = ir.case(name)
    res = ev.match_predictions_to_groundtruth(c["pb"], c["pp"], c["pc"], c["gb"], c["gc"], 0.1, 0.7)
    ir.assert_partitions_equal(res, want, name)


@pytest.mark.gpu
def test_limit_129_detections_raise_before_any_launch():
    from pod_compare_amd import evaluation_utils as ev, hip
    c = ir.case_limit(129)
    with pytest.raises(hip.PodError, match="more than 128 detections"):
        ev.match_predictions_to_groundtruth(c["pb"], c["pp"], c["pc"], c["gb"], c["gc"], 0.1, 0.7)
