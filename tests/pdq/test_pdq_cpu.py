"""PDQ (K34) without a GPU: the referee against 40-digit arithmetic, the restated assignment against brute force, the entry points'
argument checks on the built library, and the untouched surface -- compute_pdq's arguments, and apply_net's evaluation without --pdq."""
import ctypes
import math

import numpy as np
import pytest
import torch

from pod_compare_amd import apply_net, build, compute_pdq, hip
from tests.pdq import fixtures as fx
from tests.pdq import pdq_ref as pr

RHOS = (0.0, 0.3, -0.3, 0.7, -0.7, 0.9, -0.9, 0.99, -0.99)
GRID = (-7.5, -2.5, 0.5, 3.5, 7.5)


@pytest.fixture(scope="module")
def lib():
    build.build_library()
    return hip.load()


# ---- the referee against 40-digit arithmetic ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mp():
    mp = pytest.importorskip("mpmath")
    mp.mp.dps = 40
    return mp


def mp_phi(mp, x):
    return mp.erfc(-mp.mpf(float(x)) / mp.sqrt(2)) / 2


def mp_integral(mp, h, k, rho):
    if rho == 0.0:
        return mp.mpf(0)
    h, k = mp.mpf(float(h)), mp.mpf(float(k))
    f = lambda t: mp.exp(-(h * h + k * k - 2 * h * k * mp.sin(t)) / (2 * mp.cos(t) ** 2))
    return mp.quad(f, mp.linspace(0, mp.asin(mp.mpf(float(rho))), 5)) / (2 * mp.pi)


def mp_phi2_pair(mp, h, k, rho):
    """(Phi2(h, k; rho), 1 - Phi2(h, k; rho)) at 40 digits; the complement through Phi2(-h, -k; rho), whose integral is the same."""
    i = mp_integral(mp, h, k, rho)
    return mp_phi(mp, h) * mp_phi(mp, k) + i, mp_phi(mp, -h) + mp_phi(mp, -k) - (mp_phi(mp, -h) * mp_phi(mp, -k) + i)


def test_referee_phi2_and_complement_against_mpmath(mp):
    """Phi2 absolutely, the complement form relatively wherever it exceeds 1e-15.  Bounds: Phi2 is a sum of two terms of size <= 1, each a
    few roundings: 4 ulp of 1 = 8.9e-16; the complement is three erfc values and a quadrature sum, 64 ulp = 1.4e-14 relative."""
    worst_abs, worst_rel = 0.0, 0.0
    for rho in RHOS:
        for h in GRID:
            for k in GRID:
                want, want_c = mp_phi2_pair(mp, h, k, rho)
                worst_abs = max(worst_abs, abs(float(float(pr.phi2(h, k, rho)) - want)))
                if want_c > 1e-15:
                    worst_rel = max(worst_rel, abs(float((float(pr.phi2_complement(h, k, rho)) - want_c) / want_c)))
    print("PDQ_REFEREE phi2 worst |err| = %.3g, complement worst relative err = %.3g" % (worst_abs, worst_rel))
    assert worst_abs <= 4 * 2.0 ** -52 and worst_rel <= 64 * 2.0 ** -52


def test_referee_pixels_of_the_fixtures_against_mpmath(mp):
    """log P and log max(Q, small) of the referee on pixels of the fixtures' segments (forty per detection, spread over T_j: a full
    40-digit pass over every pixel takes minutes) stay within pdq_ref.REFEREE_PIXEL_ERR -- the figure the kernel's bound is eight times."""
    worst = 0.0
    cases = [(fx.jittered(), j) for j in range(3)] + [(fx.edge_cases(), j) for j in (3, 4, 5)]
    for im, j in cases:
        W, H = im["frame"]
        P, Q = pr.pixel_probs(im["means"][j], im["covs"][j], W, H)
        mu, sd, rho, _ = pr.corner_blocks(im["means"][j], im["covs"][j])
        vs, us = np.nonzero(P >= pr.P_MIN)
        for t in np.linspace(0, len(vs) - 1, 40).astype(int):
            u, v = int(us[t]), int(vs[t])
            cx, cy = u + 0.5, v + 0.5
            A, Ac = mp_phi2_pair(mp, (cx - mu[0]) / sd[0], (cy - mu[1]) / sd[1], rho[0])
            B, Bc = mp_phi2_pair(mp, (mu[2] - cx) / sd[2], (mu[3] - cy) / sd[3], rho[1])
            lp, lq = mp.log(A * B), mp.log(max(Ac + A * Bc, mp.mpf(pr.SMALL)))
            worst = max(worst, abs(float(math.log(P[v, u]) - lp)), abs(float(math.log(max(Q[v, u], pr.SMALL)) - lq)))
    print("PDQ_REFEREE worst per-pixel |log err| on %d detections x 40 pixels = %.3g (REFEREE_PIXEL_ERR %.3g)" % (len(cases), worst, pr.REFEREE_PIXEL_ERR))
    assert worst <= pr.REFEREE_PIXEL_ERR
    assert pr.KERNEL_PIXEL_BOUND == max(8.0 * pr.REFEREE_PIXEL_ERR, 1e-13)


# ---- the assignment ----------------------------------------------------------------------------------------------------------------
def _total(q, match):
    return sum(q[i, j] for i, j in enumerate(match) if j >= 0)


@pytest.mark.parametrize("shape", [(1, 1), (2, 2), (3, 5), (5, 3), (4, 4), (7, 6), (6, 7), (7, 7)])
def test_restated_assignment_is_optimal_by_brute_force(shape):
    rng = np.random.default_rng(shape[0] * 10 + shape[1])
    for trial in range(4):
        q = rng.uniform(size=shape)
        if trial == 1:
            q[rng.uniform(size=shape) < 0.5] = 0.0          # pairs that can never be true positives
        if trial == 2:
            q = np.round(q * 3) / 3                          # ties
        match = pr.assign_ref(q)
        hits = match[match >= 0]
        assert len(set(hits.tolist())) == len(hits) and all(q[i, j] > 0 for i, j in enumerate(match) if j >= 0)
        assert _total(q, match) == pytest.approx(pr.assign_brute(q), abs=1e-12)


def test_restated_assignment_agrees_with_scipy_on_the_total():
    opt = pytest.importorskip("scipy.optimize")
    rng = np.random.default_rng(5)
    for shape in ((7, 7), (20, 30), (30, 20), (64, 65)):
        q = rng.uniform(size=shape) * (rng.uniform(size=shape) < 0.7)
        r, c = opt.linear_sum_assignment(q, maximize=True)
        assert _total(q, pr.assign_ref(q)) == pytest.approx(float(q[r, c].sum()), abs=1e-10)


def test_restated_assignment_edge_matrices():
    assert pr.assign_ref(np.zeros((3, 4))).tolist() == [-1, -1, -1]
    assert pr.assign_ref(np.full((4, 4), 0.5)).tolist() == [0, 1, 2, 3]          # all equal: the lowest-index rule
    assert pr.assign_ref(np.zeros((0, 3))).tolist() == [] and pr.assign_ref(np.zeros((2, 0))).tolist() == [-1, -1]
    assert pr.image_totals({k: np.ones((2, 3)) for k in pr.PLANES}, np.array([2, -1])) == ((1, 2, 1), [1.0] * 5)


# ---- the entry points --------------------------------------------------------------------------------------------------------------
def _tables(frames, nd, ng, pair=None):
    i32 = lambda xs: (ctypes.c_int32 * len(xs))(*xs)
    cum = lambda xs: [0] + np.cumsum(xs).tolist()
    pair = cum([d * g for d, g in zip(nd, ng)]) if pair is None else pair
    return i32([v for f in frames for v in f]), i32(cum(nd)), i32(cum(ng)), (ctypes.c_int64 * len(pair))(*pair)


def test_pod_pdq_entries_reject_invalid_arguments_without_a_gpu(lib):
    """Every rejection include/pod_mi355x.h lists returns POD_E_INVALID before anything is enqueued: the rejected calls carry detections, so
    an accepted one would launch.  Calls with nothing to do return POD_OK with nothing launched."""
    buf = ctypes.create_string_buffer(128)
    X = (ctypes.addressof(buf) + 63) & ~63           # 8-byte aligned, never dereferenced on these paths
    assert lib.pod_pdq_workspace_bytes(0) >= 8 and lib.pod_pdq_workspace_bytes(3) >= 4 * (6 + 4 + 4) + 8 * 4 and lib.pod_pdq_workspace_bytes(-1) == 0

    def pairs(frames=((96, 64),), nd=(3,), ng=(2,), pair=None, K=7, p_min=0.0027, n=None, null=(), ws=X, quality=X, sums=None):
        fr, do, go, po = _tables(frames, nd, ng, pair)
        args = [fr, do, go, po, len(nd) if n is None else n, X, X, X, K, X, X, p_min, ws, quality, sums, None, None]
        for i in null:
            args[i] = None
        return lib.pod_pdq_pairs(*args)

    assert pairs(nd=(0,), ng=(2,)) == 0 and pairs(frames=(), nd=(), ng=()) == 0          # no detection, no image: nothing launched
    for bad in (dict(null=(0,)), dict(null=(1,)), dict(null=(2,)), dict(null=(3,)), dict(null=(5,)), dict(null=(6,)), dict(null=(7,)), dict(null=(9,)),
                dict(null=(10,)), dict(quality=None), dict(ws=None), dict(n=-1), dict(K=0), dict(K=hip.POD_MAX_CLASSES + 1), dict(nd=(hip.POD_PDQ_MAX_SIDE + 1,)),
                dict(ng=(hip.POD_PDQ_MAX_SIDE + 1,)), dict(frames=((0, 64),)), dict(frames=((96, 0),)), dict(frames=((96, -3),)),
                dict(frames=((hip.POD_PDQ_MAX_FRAME + 1, 64),)), dict(p_min=0.0), dict(p_min=1.0), dict(p_min=-0.1), dict(p_min=float("nan")),
                dict(pair=[0, 5]), dict(pair=[1, 7]), dict(ws=X + 4), dict(quality=X + 4), dict(sums=X + 4)):
        assert pairs(**bad) == -1, bad
    two = dict(frames=((96, 64), (97, 61)))
    assert pairs(nd=(3, 2), ng=(2, 1), pair=[0, 6, 7], **two) == -1          # pair_off is not the running sum of G D
    do = (ctypes.c_int32 * 3)(0, 3, 2)                                        # detection offsets that decrease
    fr, _, go, po = _tables(two["frames"], (3, 2), (2, 1))
    assert lib.pod_pdq_pairs(fr, do, go, po, 2, X, X, X, 7, X, X, 0.0027, X, X, None, None, None) == -1

    def assign(nd=(3,), ng=(2,), pair=None, n=None, null=(), ws=X, quality=X, sums=X):
        _, do, go, po = _tables([(1, 1)] * len(nd), nd, ng, pair)
        args = [do, go, po, len(nd) if n is None else n, quality, ws, X, X, sums, None]
        for i in null:
            args[i] = None
        return lib.pod_pdq_assign(*args)

    assert assign(nd=(), ng=()) == 0
    for bad in (dict(null=(0,)), dict(null=(1,)), dict(null=(2,)), dict(null=(6,)), dict(null=(7,)), dict(quality=None), dict(ws=None), dict(sums=None),
                dict(n=-1), dict(nd=(hip.POD_PDQ_MAX_SIDE + 1,)), dict(ng=(hip.POD_PDQ_MAX_SIDE + 1,)), dict(nd=(257,), ng=(257,)), dict(pair=[0, 5]),
                dict(ws=X + 4), dict(quality=X + 4), dict(sums=X + 4)):
        assert assign(**bad) == -1, bad


def test_header_binding_and_build_list_carry_k34():
    from tests.test_abi_cpu import declared_symbols
    for name in ("pod_pdq_workspace_bytes", "pod_pdq_pairs", "pod_pdq_assign"):
        assert name in hip.EXPORTS and name in declared_symbols()
    assert "pod_pdq_workspace_bytes" in hip._SIZE_QUERIES and "k34_pdq.hip" in build.SOURCES
    header = open(next(h for h in build.HEADERS if h.endswith("pod_mi355x.h"))).read()
    assert "#define POD_PDQ_MAX_SIDE   %d" % hip.POD_PDQ_MAX_SIDE in header and "#define POD_PDQ_MAX_FRAME  %d" % hip.POD_PDQ_MAX_FRAME in header
    assert "please use the official PDQ code" in header and hip.POD_ABI_VERSION == 18


# ---- the untouched surface ---------------------------------------------------------------------------------------------------------
def test_compute_pdq_arguments():
    a = compute_pdq.build_parser().parse_args(["--results", "r.json", "--gt", "g.json"])
    assert (a.results, a.binary_results, a.gt, a.min_allowed_score, a.map_results, a.p_min) == ("r.json", "", "g.json", None, "", 0.0027)
    assert (a.train_dataset, a.test_dataset, a.device) == ("bdd_train", "bdd_val", "cuda")
    a = compute_pdq.build_parser().parse_args(["--binary-results", "r.podr", "--gt", "g.json", "--p-min", "0.01", "--min-allowed-score", "0.3",
                                               "--test-dataset", "kitti_val", "--map-results", "m.txt"])
    assert (a.binary_results, a.p_min, a.min_allowed_score, a.test_dataset, a.map_results) == ("r.podr", 0.01, 0.3, "kitti_val", "m.txt")
    with pytest.raises(SystemExit):
        compute_pdq.build_parser().parse_args(["--results", "r.json"])          # --gt is required
    with pytest.raises(SystemExit):
        compute_pdq.main(["--gt", "g.json"])                                     # one of the two result files
    with pytest.raises(SystemExit):
        compute_pdq.main(["--gt", "g.json", "--results", "r.json", "--p-min", "1.5"])
    res = {"PDQ": 0.25, "avg_pPDQ": 0.5, "avg_spatial": 0.4, "avg_label": 0.7, "avg_fg": 0.6, "avg_bg": 0.8, "TP": 3, "FP": 2, "FN": 1, "invalid_detections": 1}
    lines = compute_pdq.format_table(res).split("\n")
    assert len({len(l) for l in lines}) == 1
    assert [c.strip() for c in lines[3].strip("|").split("|")] == ["0.2500", "0.5000", "0.4000", "0.7000", "0.6000", "0.8000", "3", "2", "1", "1"]


class StubEval:
    """evaluation_utils with pdq_scores recorded: the packing above it runs for real on the CPU."""
    def __init__(self):
        from pod_compare_amd import evaluation_utils
        self._ev, self.calls = evaluation_utils, []

    def __getattr__(self, name):
        return getattr(self._ev, name)

    def pdq_scores(self, pred, gt, frame_sizes, cat_mapping, p_min, device):
        self.calls.append((pred, gt, frame_sizes, cat_mapping, p_min, device))
        return {"PDQ": 0.0}


def test_pdq_of_results_reads_frames_threshold_and_category_map():
    gt = {"images": [{"id": 4, "width": 96, "height": 64}, {"id": 9, "width": 97, "height": 61}],
          "annotations": [{"image_id": 4, "bbox": [1.0, 2.0, 10.0, 20.0], "category_id": 2}]}
    det = lambda score, img: {"image_id": img, "category_id": 1, "bbox": [1.0, 2.0, 3.0, 4.0], "score": score, "cls_prob": [score, 1.0 - score],
                              "bbox_covar": np.eye(4).tolist()}
    ev = StubEval()
    compute_pdq.pdq_of_results([det(0.9, 4), det(0.6, 9), det(0.7, 9)], gt, {1: 0, 2: 3}, 0.65, 0.01, "cpu", ev=ev)
    pred, truth, frames, cmap, p_min, device = ev.calls[0]
    assert frames == {4: (96, 64), 9: (97, 61)} and cmap == {1: 0, 2: 3} and p_min == 0.01 and device == "cpu"
    assert {k: int(v.shape[0]) for k, v in pred["predicted_boxes"].items()} == {4: 1, 9: 1}          # 0.6 fell under the threshold
    assert truth["gt_boxes"][4].tolist() == [[1.0, 2.0, 11.0, 22.0]]


PARENT_RESULT_KEYS = {"ap", "pm", "ce", "min_allowed_score", "map_results"}
PARENT_COMPARISON_HEADER = ["Inference Config", "AP", "AP50", "AP75", "TP Cls NLL", "TP Reg NLL", "FP Cls NLL", "FP Reg Entropy", "Cls MCE", "Reg ECE",
                            "Reg MaxCE", "Cls MUE", "Reg MUE"]


def _stub_evaluators(monkeypatch, tmp_path):
    import json
    from pod_compare_amd import compute_average_precision as cap
    from pod_compare_amd import compute_calibration_errors as cce
    from pod_compare_amd import compute_probabilistic_metrics as cpm
    (tmp_path / "r.json").write_text("[]")
    (tmp_path / "gt.json").write_text(json.dumps({"images": [], "annotations": []}))
    pm = {"average": {k: {"ignorance_score_mean": 1.0, "total_entropy_mean": 2.0} for k in
                      ("true_positives_cls_analysis", "true_positives_reg_analysis", "false_positives_cls_analysis", "false_positives_reg_analysis")}}
    monkeypatch.setattr(torch.cuda, "set_device", lambda d: None)
    monkeypatch.setattr(cap, "coco_average_precision", lambda *a, **k: {"stats": [0.5] * 12, "optimal_score_threshold": 0.0})
    monkeypatch.setattr(cap, "write_map_results", lambda *a: None)
    monkeypatch.setattr(cpm, "probabilistic_metrics", lambda *a, **k: pm)
    monkeypatch.setattr(cpm, "format_table", lambda r: "")
    monkeypatch.setattr(cce, "calibration_errors_of_results", lambda *a, **k: {"cls_marginal_calibration_error_source": "", "cls_marginal_calibration_error": 0.1})
    monkeypatch.setattr(cce, "format_table", lambda r: "")
    return str(tmp_path / "r.json"), str(tmp_path / "gt.json")


def test_evaluation_without_pdq_is_the_parents(monkeypatch, tmp_path, capsys):
    """Without the flag the result has the parent's keys, comparison.txt the parent's header, and no PDQ function is reached."""
    files = _stub_evaluators(monkeypatch, tmp_path)
    reached = []
    monkeypatch.setattr(compute_pdq, "pdq_of_results", lambda *a, **k: reached.append(a) or {"PDQ": 0.125, "avg_pPDQ": 0.5, "avg_spatial": 0.5, "avg_label": 0.5,
                                                                                           "avg_fg": 0.5, "avg_bg": 0.5, "TP": 1, "FP": 2, "FN": 3, "invalid_detections": 0})
    plain = apply_net.evaluate_results(*files, min_allowed_score=0.0, device="cpu")
    assert set(plain) == PARENT_RESULT_KEYS and not reached
    header = lambda table: [c.strip() for c in table.split("\n")[1].strip("|").split("|")]
    assert header(apply_net.format_comparison_table(["a"], [plain])) == PARENT_COMPARISON_HEADER
    out = capsys.readouterr().out
    assert "PDQ" not in out
    with_pdq = apply_net.evaluate_results(*files, min_allowed_score=0.25, device="cpu", pdq=True, p_min=0.01)
    assert set(with_pdq) == PARENT_RESULT_KEYS | {"pdq"} and len(reached) == 1
    assert reached[0][3:] == (0.25, 0.01, "cpu") and reached[0][2] == apply_net.evaluation_category_map("bdd_train", "bdd_val")
    assert "avg pPDQ" in capsys.readouterr().out
    table = apply_net.format_comparison_table(["a", "b"], [with_pdq, plain])
    assert header(table) == PARENT_COMPARISON_HEADER + ["PDQ"]
    rows = [[c.strip() for c in l.strip("|").split("|")] for l in table.split("\n")[3:5]]
    assert rows[0][-1] == "0.1250" and rows[1][-1] == "-"


def test_apply_net_flags_reach_evaluate_results(monkeypatch):
    import argparse
    ns = argparse.Namespace(scoring_rules=["nll"], energy_samples=1000, pdq=False, p_min=0.0027)
    assert apply_net._scoring_rule_options(ns) == {}
    ns.pdq, ns.p_min = True, 0.01
    assert apply_net._scoring_rule_options(ns) == {"pdq": True, "p_min": 0.01}
    ns.scoring_rules = ["nll", "crps"]
    assert apply_net._scoring_rule_options(ns) == {"scoring_rules": ("nll", "crps"), "energy_samples": 1000, "pdq": True, "p_min": 0.01}
    seen = {}
    monkeypatch.setattr(apply_net, "evaluate_results", lambda *a, **k: seen.update(k) or "done")
    monkeypatch.setattr(apply_net, "has_ground_truth", lambda p: True)
    assert apply_net.main(["--eval-only", "--pdq", "--p-min", "0.02", "--coco-json", "gt.json", "--output", "r.json"]) == "done"
    assert seen["pdq"] is True and seen["p_min"] == 0.02
    seen.clear()
    apply_net.main(["--eval-only", "--coco-json", "gt.json", "--output", "r.json"])
    assert "pdq" not in seen and "p_min" not in seen


def test_fixture_frames_and_cases():
    ims = fx.all_images()
    assert [im["frame"] for im in ims[:3]] == [(96, 64), (97, 61), (96, 64)] and ims[-1]["frame"][0] > 256
    assert len(ims[3]["gt_boxes"]) == 0 and len(ims[4]["means"]) == 0 and len(ims[5]["gt_boxes"]) == 70
    assert not pr.corner_blocks(ims[2]["means"][1], ims[2]["covs"][1])[3] and not pr.corner_blocks(ims[2]["means"][3], ims[2]["covs"][3])[3]
    for j, sign in ((4, 1.0), (5, -1.0)):          # rho beyond the clamp, both signs
        cov = ims[1]["covs"][j]
        assert abs(cov[1, 0] / math.sqrt((cov[0, 0] + 0.01) * (cov[1, 1] + 0.01))) > pr.RHO_MAX
        assert pr.corner_blocks(ims[1]["means"][j], cov)[2].tolist() == [sign * pr.RHO_MAX] * 2
