"""compute_probabilistic_metrics with scoring_rules = (nll, energy, crps, brier), end to end on the HIP kernels: every new mean is the mean
of the fp64 referee's rows under the driver's own masks, the old keys are the default call's, the table gains three columns, and
apply_net's evaluate_results hands the options on.  693 detections on 10 images (instrument_ref's mixed set), K = 7.

Bound of a mean: 1e-6 max(1, |ref|).  The rows meet 2^-22 max(1, |row|) = 2.4e-7 (test_nll_gpu.py) and the mean of the fp32 rows is taken in
fp64, so a mean errs by at most the rows' bound; Brier is 3 fp32 operations per row (<= 4 * 2^-24 relative).

The module shares its name with tests/test_probabilistic_metrics.py for its place in the GPU run order (tests/conftest.py: GPU_ORDER)."""
import numpy as np
import pytest
import torch

from tests.eval_instrument import instrument_ref as ir
from tests.eval_scores import gpu_common as gc
from tests.eval_scores import scores_ref as sr

pytestmark = pytest.mark.gpu
CLASSES = (0, 1, 2, 3, 4, 5, 6)
M, SEED, TOL = 200, 12345, 1e-6
NEW = {"true_positives_cls_analysis": ("brier_score_mean",), "true_positives_reg_analysis": ("energy_score_mean", "crps_mean"),
       "false_positives_cls_analysis": ("brier_score_mean",), "false_positives_reg_analysis": ()}


class Recorder:
    """evaluation_utils, remembering the partitions the driver scores (the dicts it then attaches tensors to)."""
    def __init__(self):
        from pod_compare_amd import evaluation_utils
        self._ev, self.matched = evaluation_utils, None

    def __getattr__(self, name):
        return getattr(self._ev, name)

    def match_predictions_to_groundtruth(self, *a, **k):
        self.matched = self._ev.match_predictions_to_groundtruth(*a, **k)
        return self.matched


@pytest.fixture(scope="module")
def runs():
    from pod_compare_amd import compute_probabilistic_metrics as pm
    predicted, gt = sr.result_set(seed=2, nd=ir.MIXED_ND, ng=ir.MIXED_NG)
    rec = Recorder()
    full = pm.probabilistic_metrics(predicted, gt, classes=CLASSES, ev=rec, scoring_rules=("nll", "energy", "crps", "brier"), energy_samples=M, seed=SEED)
    base = pm.probabilistic_metrics(predicted, gt, classes=CLASSES)
    return predicted, gt, rec.matched, full, base


def test_new_means_equal_the_referee_under_the_same_masks(runs):
    _, _, matched, full, _ = runs
    tp, fp = matched["true_positives"], matched["false_positives"]
    n = int(tp["predicted_box_means"].shape[0])
    assert n >= 40 and int(fp["predicted_box_means"].shape[0]) >= 40
    means, covs, gt = (tp[k].cpu() for k in ("predicted_box_means", "predicted_box_covariances", "gt_box_means"))
    eps = gc.expected_normals(SEED, np.arange(n), M)          # a row draws under (seed, its position in the partition)
    ref = {"energy_score": sr.energy_ref(means, covs, gt, eps), "crps": sr.crps_ref(means, covs, gt)}
    for name, want in ref.items():
        err = gc.rel_err(tp[name].cpu(), want)
        print("PM_ROWS %-12s n = %d: max |got - ref| / max(1, |ref|) = %.3g (bound %.3g)" % (name, n, err, sr.BOUND))
        assert tp[name].dtype == torch.float32 and err <= sr.BOUND, (name, err)
    brier = {"true_positives": sr.brier_rows(tp["predicted_score_of_gt_category"].cpu()), "false_positives": sr.brier_rows(fp["predicted_score_of_gt_category"].cpu())}
    masks = {"true_positives": tp["gt_converted_cat_idxs"].cpu(), "false_positives": fp["predicted_cat_idxs"].cpu()}
    checked = 0
    for cls in CLASSES:
        for part in ("true_positives", "false_positives"):
            sel = masks[part] == cls
            rows = {"brier_score_mean": brier[part]}
            if part == "true_positives":
                rows.update(energy_score_mean=ref["energy_score"], crps_mean=ref["crps"])
            got = dict(full["per_class"][cls][part + "_cls_analysis"], **full["per_class"][cls][part + "_reg_analysis"])
            for key, r in rows.items():
                if not bool(sel.any()):
                    assert got[key] is None
                    continue
                want = float(r[sel].mean())
                assert abs(got[key] - want) <= TOL * max(1.0, abs(want)), (cls, part, key, got[key], want)
                checked += 1
    assert checked >= 4 * 5
    for key, names in NEW.items():          # the average: the nan-mean over the classes, as for the old keys
        for name in names:
            vals = [full["per_class"][c][key][name] for c in CLASSES if full["per_class"][c][key][name] is not None]
            assert full["average"][key][name] == pytest.approx(float(np.mean(vals)), rel=1e-12)


def test_old_keys_are_the_default_calls(runs):
    _, _, _, full, base = runs
    assert full["counts"] == base["counts"]
    for scope, ref in [(full["average"], base["average"])] + [(full["per_class"][c], base["per_class"][c]) for c in CLASSES]:
        assert set(scope) == set(ref)
        for key in ref:
            assert set(scope[key]) == set(ref[key]) | set(NEW[key])
            for name in ref[key]:
                assert scope[key][name] == ref[key][name], (key, name)


def test_scores_do_not_depend_on_the_class_filter(runs):
    from pod_compare_amd import compute_probabilistic_metrics as pm
    predicted, gt, _, full, _ = runs
    few = pm.probabilistic_metrics(predicted, gt, classes=(1, 3), scoring_rules=("energy", "crps", "brier"), energy_samples=M, seed=SEED)
    for cls in (1, 3):
        assert few["per_class"][cls] == full["per_class"][cls]


def test_table_has_the_three_columns(runs):
    from pod_compare_amd import compute_probabilistic_metrics as pm
    _, _, _, full, base = runs
    lines = pm.format_table(full).split("\n")
    cells = [[c.strip() for c in l.strip("|").split("|")] for l in (lines[1], lines[3], lines[4], lines[5])]
    assert len({len(l) for l in lines}) == 1
    assert cells[0][4:] == ["Cls Brier Score", "Reg Energy Score", "Reg CRPS"]
    a = full["average"]
    assert cells[1][4:] == ["%.4f" % a["true_positives_cls_analysis"]["brier_score_mean"], "%.4f" % a["true_positives_reg_analysis"]["energy_score_mean"],
                            "%.4f" % a["true_positives_reg_analysis"]["crps_mean"]]
    assert cells[2][4:] == ["%.4f" % a["false_positives_cls_analysis"]["brier_score_mean"], "-", "-"] and cells[3][4:] == ["-", "-", "-"]
    old = pm.format_table(base).split("\n")
    assert [c[:4] for c in cells] == [[x.strip() for x in old[i].strip("|").split("|")] for i in (1, 3, 4, 5)]


def test_evaluate_results_passes_the_options_through(runs, tmp_path, monkeypatch):
    """The AP and CE steps are stubbed (they have their own tests); PM runs for real on the files."""
    import json
    from pod_compare_amd import apply_net
    from pod_compare_amd import compute_average_precision as cap
    from pod_compare_amd import compute_calibration_errors as cce
    predicted, gt, _, full, base = runs
    (tmp_path / "r.json").write_text(json.dumps(predicted))
    (tmp_path / "gt.json").write_text(json.dumps({"annotations": gt}))
    monkeypatch.setattr(cap, "coco_average_precision", lambda *a, **k: {"stats": [0.0] * 12, "optimal_score_threshold": 0.0})
    monkeypatch.setattr(cap, "write_map_results", lambda *a: None)
    monkeypatch.setattr(cce, "calibration_errors_of_results", lambda *a, **k: {"cls_marginal_calibration_error_source": ""})
    monkeypatch.setattr(cce, "format_table", lambda r: "")
    args = (str(tmp_path / "r.json"), str(tmp_path / "gt.json"))
    res = apply_net.evaluate_results(*args, min_allowed_score=0.0, device="cuda:0", seed=SEED, scoring_rules=("nll", "energy", "crps", "brier"), energy_samples=M)
    plain = apply_net.evaluate_results(*args, min_allowed_score=0.0, device="cuda:0", seed=SEED)
    for cls in (1, 3):          # the driver's default classes
        assert res["pm"]["per_class"][cls] == full["per_class"][cls] and plain["pm"]["per_class"][cls] == base["per_class"][cls]
    assert "energy_score_mean" in res["pm"]["average"]["true_positives_reg_analysis"]
    assert "energy_score_mean" not in plain["pm"]["average"]["true_positives_reg_analysis"]
