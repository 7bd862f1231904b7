"""The evaluation's bounded scoring rules without a GPU: pod_reg_scores' entry checks, the closed-form anchor of the energy score on the
host restatement of the draws, and the Python plumbing -- the default call is today's call, the per-class masks only select."""
import ctypes

import numpy as np
import pytest
import torch

from pod_compare_amd import apply_net, build, hip
from pod_compare_amd import compute_probabilistic_metrics as pm
from pod_compare_amd import evaluation_utils as ev_hip
from tests.eval_instrument import instrument_ref as ir
from tests.eval_scores import scores_ref as sr


@pytest.fixture(scope="module")
def lib():
    build.build_library()
    return hip.load()


# ---- the entry point ---------------------------------------------------------------------------------------------------------------
def test_pod_reg_scores_rejects_invalid_arguments_without_a_gpu(lib):
    """Every rejection include/pod_mi355x.h lists returns POD_E_INVALID before anything is launched; every rejected call differs from a
    valid one in exactly the arguments under test.  n == 0 is accepted, and the checks come before that exit."""
    buf = ctypes.create_string_buffer(128)
    X = (ctypes.addressof(buf) + 63) & ~63           # 64-byte aligned, never dereferenced on these paths
    M4 = X + 4                                       # misaligned for 16 bytes
    base = [X, X, X, 0, 1000, 7, None, None, X, X, None]          # means, covs, gt, n, num_samples, seed, eps_in, eps_out, energy, crps, stream
    call = lambda *pairs: lib.pod_reg_scores(*[dict(pairs).get(i, v) for i, v in enumerate(base)])
    assert call() == 0
    assert call((6, X), (7, X)) == 0 and call((8, None)) == 0 and call((9, None)) == 0
    assert call((4, 1)) == 0 and call((4, hip.POD_MAX_REG_SAMPLES)) == 0
    assert call((8, None), (4, 0)) == 0 and call((8, None), (4, -5)) == 0          # energy null: num_samples is ignored
    for bad in ([(0, None)], [(1, None)], [(2, None)], [(8, None), (9, None)], [(3, -1)], [(4, 0)], [(4, -1)], [(4, hip.POD_MAX_REG_SAMPLES + 1)],
                [(8, None), (6, X)], [(8, None), (7, X)], [(6, M4)], [(7, M4)]):
        assert call(*bad) == -1, bad
        if bad != [(3, -1)]:
            assert call((3, 5), *bad) == -1, bad          # the same with rows to score: refused before any launch


def test_the_stream_word_is_its_own():
    assert sr.STREAM_EVAL_SCORE not in rr_streams() and sr.STREAM_EVAL_SCORE == int.from_bytes(b"evs\0", "big")
    src = open(build.HEADERS[0]).read()
    assert "STREAM_EVAL_SCORE = 0x%08xu" % sr.STREAM_EVAL_SCORE in src


def rr_streams():
    from tests.rng import rng_ref as rr
    return set(rr.STREAMS.values())


def test_draw_addresses_are_distinct_and_differ_from_the_training_stream():
    from tests.rng import rng_ref as rr
    rows = np.arange(5)
    ctr, comp = sr.eval_score_addr(rows, 129)
    assert rr.count_collisions((ctr, comp)) == 0
    assert rr.count_collisions((ctr, comp), rr.reg_score_addr(rows, np.zeros(5, dtype=np.int64), 129)) == 0
    w, _ = sr.eval_score_normals(11, rows, 6)
    w27, _ = rr.reg_score_normals(11, rows, np.zeros(5, dtype=np.int64), 6)
    assert not np.array_equal(w, w27)


# ---- the referee -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def anchor_eps():
    return sr.host_normals(sr.ANCHOR_SEED, np.arange(sr.ANCHOR_N), sr.ANCHOR_M)


@pytest.mark.parametrize("variance", sr.ANCHOR_VARIANCES)
def test_energy_referee_meets_the_closed_form_on_the_host_draws(anchor_eps, variance):
    """Sigma = s^2 I, gt = mean: E ES = 0.550631 s.  The mean over 4096 rows of the referee, on the host restatement of the kernel's draws
    under the seed the GPU test uses, lies within 5 standard errors (from the rows' own deviation) of it."""
    assert abs(sr.ENERGY_UNIT - 0.550631) < 5e-7
    assert float(anchor_eps.abs().max()) < 4.9 and abs(float(anchor_eps.double().mean())) < 5e-3
    means, covs, gt = sr.anchor_case(variance)
    mean, want, se, dev = sr.anchor_deviation(sr.energy_ref(means, covs, gt, anchor_eps), variance)
    print("ENERGY_ANCHOR host variance=%g mean=%.6f closed_form=%.6f standard_error=%.3g deviation=%+.2f standard errors" % (variance, mean, want, se, dev))
    assert abs(dev) <= sr.ANCHOR_SIGMAS


def test_crps_referee_against_quadrature_and_brier():
    """The closed form against its definition, the integral of (F(x) - 1[x >= y])^2, by a fine trapezoid rule; Brier at its corners."""
    means = torch.tensor([[0.0, 1.0, -2.0, 300.0]])
    gt = torch.tensor([[0.5, 1.0, 4.0, 297.0]])
    covs = torch.diag(torch.tensor([0.99, 3.99, 0.24, 24.99])).unsqueeze(0)
    x = torch.linspace(-60.0, 60.0, 2_400_001, dtype=torch.float64)
    want = 0.0
    for j in range(4):
        sd = float(covs[0, j, j] + 1e-2) ** 0.5
        y = float(gt[0, j] - means[0, j])
        cdf = 0.5 * (1.0 + torch.special.erf(x / (sd * 2.0 ** 0.5)))
        want += float(torch.trapezoid((cdf - (x >= y).double()) ** 2, x)) / 4.0
    got = float(sr.crps_ref(means, covs, gt))
    assert abs(got - want) <= 1e-4 * want, (got, want)
    assert sr.brier_rows(torch.tensor([1.0, 0.0, 0.5])).tolist() == [0.0, 2.0, 0.5]
    assert torch.equal(ev_hip.brier_rows(torch.tensor([1.0, 0.0, 0.5, 0.25])), torch.tensor([0.0, 2.0, 0.5, 1.125]))


# ---- the plumbing ------------------------------------------------------------------------------------------------------------------
class CpuEval:
    """The functions the driver needs on the CPU: instrument_ref's matching and NLL; the per-row means are evaluation_utils' own."""
    eval_predictions_preprocess = staticmethod(ev_hip.eval_predictions_preprocess)
    eval_gt_preprocess = staticmethod(ev_hip.eval_gt_preprocess)
    calls = []

    @staticmethod
    def match_predictions_to_groundtruth(pb, pp, pc, gb, gc, iou_min, iou_correct, device="cpu"):
        p = ir.pack(pb, pp, pc, gb, gc)
        return ir.partitions(p, ir.match_ref(p.det_boxes, p.det_probs, p.det_off, p.gt_boxes, p.gt_off, iou_min, iou_correct))

    @staticmethod
    def compute_reg_scores(m, valid):
        CpuEval.calls.append("compute_reg_scores")
        if int(valid.sum()) == 0:
            return {"ignorance_score_mean": None, "mean_squared_error": None}
        a, c, g = m["predicted_box_means"][valid], m["predicted_box_covariances"][valid], m["gt_box_means"][valid]
        return {"ignorance_score_mean": float(ir.nll_ref(a, c, g).mean()), "mean_squared_error": float(((a - g) ** 2).mean())}

    @staticmethod
    def compute_reg_scores_fn(m, valid):
        CpuEval.calls.append("compute_reg_scores_fn")
        c = m["predicted_box_covariances"][valid]
        return {"total_entropy_mean": float(ir.entropy_ref(c).mean()) if c.shape[0] else None}

    @staticmethod
    def retinanet_compute_cls_scores(m, valid):
        CpuEval.calls.append("retinanet_compute_cls_scores")
        p = m["predicted_score_of_gt_category"][valid]
        return {"ignorance_score_mean": float((-torch.log(p)).mean()) if p.shape[0] else None}

    def __getattr__(self, name):          # (instances only: the class itself has no such hook)
        raise AssertionError("the default call reached for ev.%s" % name)


def test_default_call_is_todays_call_and_unknown_rules_raise():
    predicted, gt = sr.result_set()
    CpuEval.calls.clear()
    classes = (0, 1, 2, 3, 4, 5, 6)
    a = pm.probabilistic_metrics(predicted, gt, device="cpu", ev=CpuEval(), classes=classes)
    n_calls = len(CpuEval.calls)
    b = pm.probabilistic_metrics(predicted, gt, device="cpu", ev=CpuEval(), classes=classes, scoring_rules=("nll",))
    assert a == b and len(CpuEval.calls) == 2 * n_calls == 2 * 4 * len(classes)
    assert a["counts"]["true_positives"] > 10 and a["counts"]["false_positives"] > 10
    assert set(a["average"]["true_positives_reg_analysis"]) == {"ignorance_score_mean", "mean_squared_error"}
    assert set(a["average"]["true_positives_cls_analysis"]) == set(a["average"]["false_positives_cls_analysis"]) == {"ignorance_score_mean"}
    table = pm.format_table(a)
    lines = table.split("\n")
    assert len(lines) == 7 and all(l.count("|") == 5 for l in lines[1:2] + lines[3:6]) and "Brier" not in table and "Energy" not in table and "CRPS" not in table
    assert [c.strip() for c in lines[1].strip("|").split("|")] == ["Output Type", "Number of Instances", "Cls Ignorance Score", "Reg Ignorance Score"]
    for bad in (("nll", "energi"), ("mse",), ("nll", "energy", "Brier")):
        with pytest.raises(ValueError) as e:
            pm.probabilistic_metrics(predicted, gt, device="cpu", ev=CpuEval(), scoring_rules=bad)
        assert repr([r for r in bad if r not in pm.SCORING_RULES][0]) in str(e.value)


def test_brier_needs_no_kernel_and_fills_its_column():
    """scoring_rules = (nll, brier) on the CPU: the driver attaches brier_rows to the true and false positives; the means are the masked
    means of those rows; the table gains ONE column with a `-` for the false negatives."""
    predicted, gt = sr.result_set()

    class Ev(CpuEval):
        brier_rows = staticmethod(ev_hip.brier_rows)
        retinanet_compute_cls_scores = staticmethod(ev_hip.retinanet_compute_cls_scores)
        seen = {}

        @staticmethod
        def match_predictions_to_groundtruth(*a, **k):
            Ev.seen = CpuEval.match_predictions_to_groundtruth(*a, **k)
            return Ev.seen

    classes = (0, 2, 5)
    res = pm.probabilistic_metrics(predicted, gt, device="cpu", ev=Ev(), classes=classes, scoring_rules=("brier", "nll"))
    base = pm.probabilistic_metrics(predicted, gt, device="cpu", ev=CpuEval(), classes=classes)
    for cls in classes:
        for part, mask_key in (("true_positives", "gt_converted_cat_idxs"), ("false_positives", "predicted_cat_idxs")):
            m = Ev.seen[part]
            rows = sr.brier_rows(m["predicted_score_of_gt_category"])[m[mask_key] == cls]
            got = res["per_class"][cls][part + "_cls_analysis"]
            assert set(got) == {"ignorance_score_mean", "brier_score_mean"}
            assert got["brier_score_mean"] == pytest.approx(float(rows.mean()), rel=1e-6) if rows.numel() else got["brier_score_mean"] is None
            assert got["ignorance_score_mean"] == pytest.approx(base["per_class"][cls][part + "_cls_analysis"]["ignorance_score_mean"], rel=1e-6)
        assert res["per_class"][cls]["true_positives_reg_analysis"] == base["per_class"][cls]["true_positives_reg_analysis"]
    assert "brier_score" not in Ev.seen["duplicates"] and "brier_score" not in Ev.seen["false_negatives"]
    lines = pm.format_table(res).split("\n")
    cells = [[c.strip() for c in l.strip("|").split("|")] for l in (lines[1], lines[3], lines[4], lines[5])]
    assert cells[0][4:] == ["Cls Brier Score"] and cells[3][4:] == ["-"] and len({len(l) for l in lines}) == 1
    assert cells[1][4] == "%.4f" % res["average"]["true_positives_cls_analysis"]["brier_score_mean"]
    assert cells[2][4] == "%.4f" % res["average"]["false_positives_cls_analysis"]["brier_score_mean"]
    old = pm.format_table(base).split("\n")
    assert [c[:4] for c in cells] == [[x.strip() for x in old[i].strip("|").split("|")] for i in (1, 3, 4, 5)]


def test_per_class_means_are_the_masked_means_of_the_attached_rows():
    """evaluation_utils' two functions on a partition that carries per-row tensors: fp64 means under the mask, None on an empty mask, and
    no new key without the tensors.  (The NLL half of compute_reg_scores needs the GPU: the empty mask stops before it.)"""
    g = torch.Generator().manual_seed(3)
    n = 37
    part = {"predicted_box_means": torch.zeros(n, 4), "predicted_box_covariances": torch.eye(4).expand(n, 4, 4), "gt_box_means": torch.zeros(n, 4),
            "predicted_score_of_gt_category": 0.05 + 0.9 * torch.rand(n, generator=g)}
    none = torch.zeros(n, dtype=torch.bool)
    mask = torch.rand(n, generator=g) < 0.4
    assert ev_hip.compute_reg_scores(part, none) == {"ignorance_score_mean": None, "mean_squared_error": None}
    assert set(ev_hip.retinanet_compute_cls_scores(part, mask)) == {"ignorance_score_mean"}
    part["energy_score"], part["crps"] = torch.rand(n, generator=g), torch.rand(n, generator=g)
    part["brier_score"] = ev_hip.brier_rows(part["predicted_score_of_gt_category"])
    assert ev_hip.compute_reg_scores(part, none) == {"ignorance_score_mean": None, "mean_squared_error": None, "energy_score_mean": None, "crps_mean": None}
    assert ev_hip.retinanet_compute_cls_scores(part, none) == {"ignorance_score_mean": None, "brier_score_mean": None}
    got = ev_hip.retinanet_compute_cls_scores(part, mask)
    assert got["brier_score_mean"] == float(part["brier_score"][mask].double().mean())
    assert got["ignorance_score_mean"] == float((-torch.log(part["predicted_score_of_gt_category"][mask])).mean())
    means = ev_hip._row_score_means(part, mask, ("energy_score", "crps"))
    assert means == {"energy_score_mean": float(part["energy_score"][mask].double().mean()), "crps_mean": float(part["crps"][mask].double().mean())}
    del part["crps"]
    assert ev_hip.compute_reg_scores(part, none) == {"ignorance_score_mean": None, "mean_squared_error": None, "energy_score_mean": None}


# ---- the commands ------------------------------------------------------------------------------------------------------------------
def canned(extra):
    pm_avg = {"true_positives_cls_analysis": {"ignorance_score_mean": 0.5}, "true_positives_reg_analysis": {"ignorance_score_mean": 12.25, "mean_squared_error": 1.0},
              "false_positives_cls_analysis": {"ignorance_score_mean": 2.0}, "false_positives_reg_analysis": {"total_entropy_mean": 9.87654}}
    if extra:
        pm_avg["true_positives_cls_analysis"]["brier_score_mean"] = 0.125
        pm_avg["false_positives_cls_analysis"]["brier_score_mean"] = None
        pm_avg["true_positives_reg_analysis"]["energy_score_mean"] = 3.14159
    return {"ap": {"stats": [0.1, 0.5, 0.25] + [0.0] * 9, "optimal_score_threshold": 0.3}, "pm": {"average": pm_avg, "counts": {}},
            "ce": {"cls_marginal_calibration_error": 0.0123, "reg_expected_calibration_error": 0.04, "reg_maximum_calibration_error": 0.2,
                   "cls_minimum_uncertainty_error": 0.11111, "reg_minimum_uncertainty_error": 0.3}}


def test_comparison_table_appends_only_the_columns_asked_for():
    plain = apply_net.format_comparison_table(["a", "b"], [canned(False), canned(False)])
    assert "Brier" not in plain and "Energy" not in plain and "CRPS" not in plain
    table = apply_net.format_comparison_table(["a", "b"], [canned(True), canned(False)])
    lines = table.split("\n")
    cells = [[c.strip() for c in l.strip("|").split("|")] for l in (lines[1], lines[3], lines[4])]
    head = [c.strip() for c in plain.split("\n")[1].strip("|").split("|")]
    assert cells[0] == head + ["TP Cls Brier", "FP Cls Brier", "TP Reg Energy"] and len({len(l) for l in lines}) == 1
    assert cells[1][len(head):] == ["0.1250", "-", "3.1416"] and cells[2][len(head):] == ["-", "-", "-"]
    assert [c[1:len(head)] for c in cells[1:]] == [[c.strip() for c in l.strip("|").split("|")][1:] for l in plain.split("\n")[3:5]]


def test_commands_pass_the_options_on(tmp_path, monkeypatch):
    import json
    from pod_compare_amd import compute_average_precision as cap
    from pod_compare_amd import compute_calibration_errors as cce
    gt = tmp_path / "gt.json"
    gt.write_text(json.dumps({"images": [], "annotations": []}))
    (tmp_path / "r.json").write_text("[]")
    # apply_net --eval-only -> evaluate_results
    calls = []
    monkeypatch.setattr(apply_net, "evaluate_results", lambda *a, **k: calls.append(k) or {})
    common = ["--eval-only", "--coco-json", str(gt), "--output", str(tmp_path / "r.json")]
    apply_net.main(common)
    apply_net.main(common + ["--scoring-rules", "nll", "energy", "brier", "--energy-samples", "64", "--random-seed", "9"])
    assert "scoring_rules" not in calls[0] and "energy_samples" not in calls[0]
    assert calls[1]["scoring_rules"] == ("nll", "energy", "brier") and calls[1]["energy_samples"] == 64 and calls[1]["seed"] == 9
    monkeypatch.undo()
    # evaluate_results -> probabilistic_metrics
    seen = []
    monkeypatch.setattr(torch.cuda, "set_device", lambda d: None)
    monkeypatch.setattr(cap, "coco_average_precision", lambda *a, **k: {"stats": [0.0] * 12, "optimal_score_threshold": 0.0})
    monkeypatch.setattr(cap, "format_summary", lambda s: "")
    monkeypatch.setattr(cap, "write_map_results", lambda *a: None)
    monkeypatch.setattr(cce, "calibration_errors_of_results", lambda *a, **k: {"cls_marginal_calibration_error_source": ""})
    monkeypatch.setattr(cce, "format_table", lambda r: "")
    monkeypatch.setattr(pm, "probabilistic_metrics", lambda *a, **k: seen.append(k) or {})
    monkeypatch.setattr(pm, "format_table", lambda r: "")
    apply_net.evaluate_results(str(tmp_path / "r.json"), str(gt), min_allowed_score=0.0, seed=4)
    apply_net.evaluate_results(str(tmp_path / "r.json"), str(gt), min_allowed_score=0.0, seed=4, scoring_rules=("nll", "crps"), energy_samples=17)
    assert set(seen[0]) == {"cat_mapping_dict", "min_allowed_score", "device"}
    assert seen[1]["scoring_rules"] == ("nll", "crps") and seen[1]["energy_samples"] == 17 and seen[1]["seed"] == 4
    monkeypatch.undo()
    # compute_probabilistic_metrics' own command line
    seen.clear()
    monkeypatch.setattr(pm, "probabilistic_metrics", lambda *a, **k: seen.append(k) or {})
    monkeypatch.setattr(pm, "format_table", lambda r: "")
    base = ["--results", str(tmp_path / "r.json"), "--gt", str(gt), "--min-allowed-score", "0"]
    pm.main(base)
    pm.main(base + ["--scoring-rules", "nll", "crps", "energy", "--energy-samples", "33", "--seed", "21"])
    assert seen[0]["scoring_rules"] == ("nll",) and seen[0]["energy_samples"] == 1000 and seen[0]["seed"] == 0
    assert seen[1]["scoring_rules"] == ("nll", "crps", "energy") and seen[1]["energy_samples"] == 33 and seen[1]["seed"] == 21
    with pytest.raises(SystemExit):
        pm.main(base + ["--scoring-rules", "nll", "energi"])
