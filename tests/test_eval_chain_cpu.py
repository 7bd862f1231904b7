"""The evaluation chain's host side: the test-set category maps of the three evaluators (EU:370-397) and apply_net's --eval /
--eval-only plumbing (AN:104-106), without a GPU."""
import json

import numpy as np
import pytest

from pod_compare_amd import apply_net
from pod_compare_amd import compute_average_precision as cap
from pod_compare_amd import compute_calibration_errors as ce
from pod_compare_amd import compute_probabilistic_metrics as pm


def test_evaluation_category_map():
    assert apply_net.evaluation_category_map("bdd_train", "kitti_val") == {1: 0, 2: 3}
    ident = {i: i - 1 for i in range(1, 8)}
    assert apply_net.evaluation_category_map("bdd_train", "bdd_val") == ident
    assert apply_net.evaluation_category_map("bdd_train", "lyft_val") == ident
    assert apply_net.evaluation_category_map("kitti_train", "kitti_val") == {1: 0, 2: 1}
    with pytest.raises(ValueError):
        apply_net.evaluation_category_map("kitti_train", "bdd_val")
    # the two maps agree: a model class written with category_mapping reads back as the same class
    fwd = apply_net.category_mapping("bdd_train", "kitti_val")
    back = apply_net.evaluation_category_map("bdd_train", "kitti_val")
    assert {back[d]: d for d in back} == fwd


@pytest.mark.parametrize("mod", [pm, ce, cap])
def test_evaluators_parse_the_dataset_flags(mod, tmp_path, monkeypatch):
    """--train-dataset / --test-dataset reach the category map the evaluator scores with; the defaults are BDD's."""
    from pod_compare_amd import evaluation_utils
    (tmp_path / "r.json").write_text("[]")
    (tmp_path / "gt.json").write_text(json.dumps({"annotations": [], "images": []}))
    seen = []

    class Stop(Exception):
        pass

    def fake_map(train, test):
        seen.append((train, test))
        raise Stop()

    monkeypatch.setattr(apply_net, "evaluation_category_map", fake_map)
    monkeypatch.setattr(apply_net, "category_mapping", fake_map)
    monkeypatch.setattr(evaluation_utils, "eval_predictions_preprocess", lambda *a, **k: (_ for _ in ()).throw(Stop()))
    base = ["--gt", str(tmp_path / "gt.json")]
    if mod is cap:      # AP reads the map only for binary results
        (tmp_path / "r.podr").write_bytes(b"")
        base += ["--binary-results", str(tmp_path / "r.podr")]
    else:
        base += ["--results", str(tmp_path / "r.json")]
    for extra, want in (([], ("bdd_train", "bdd_val")), (["--test-dataset", "kitti_val"], ("bdd_train", "kitti_val")),
                        (["--train-dataset", "kitti_train", "--test-dataset", "kitti_val"], ("kitti_train", "kitti_val"))):
        with pytest.raises(Stop):
            mod.main(base + extra)
        assert seen[-1] == want


def test_probabilistic_metrics_binary_results_read_with_the_test_set_map(tmp_path, monkeypatch):
    from pod_compare_amd import inference_utils
    got = []
    monkeypatch.setattr(inference_utils, "binary_results_to_json", lambda path, cmap: got.append(cmap) or [])
    monkeypatch.setattr(pm, "probabilistic_metrics", lambda *a, **k: (_ for _ in ()).throw(KeyboardInterrupt()))
    (tmp_path / "gt.json").write_text(json.dumps({"annotations": []}))
    with pytest.raises(KeyboardInterrupt):
        pm.main(["--binary-results", "x.podr", "--gt", str(tmp_path / "gt.json"), "--test-dataset", "kitti_val"])
    assert got == [{0: 1, 3: 2}]


def test_apply_net_eval_needs_ground_truth(tmp_path, capsys):
    (tmp_path / "set.json").write_text(json.dumps({"images": []}))
    for flags in (["--eval"], ["--eval-only"], ["--eval", "--coco-json", str(tmp_path / "set.json")]):
        with pytest.raises(SystemExit) as e:
            apply_net.main(flags)
        assert "ground truth" in str(e.value)
    gt = tmp_path / "gt.json"
    gt.write_text(json.dumps({"images": [], "annotations": []}))
    with pytest.raises(SystemExit) as e:
        apply_net.main(["--eval", "--coco-json", str(gt), "--ensemble-per-gpu"])
    assert "ensemble-per-gpu" in str(e.value)


def test_eval_only_builds_no_model(tmp_path, monkeypatch):
    from pod_compare_amd import probabilistic_inference
    monkeypatch.setattr(probabilistic_inference, "build_predictor", lambda *a, **k: pytest.fail("--eval-only built a model"))
    monkeypatch.setattr(probabilistic_inference, "build_model", lambda *a, **k: pytest.fail("--eval-only built a model"))
    calls = []
    monkeypatch.setattr(apply_net, "evaluate_results", lambda *a, **k: calls.append((a, k)) or {"ap": 1, "pm": 2, "ce": 3})
    gt = tmp_path / "gt.json"
    gt.write_text(json.dumps({"images": [], "annotations": []}))
    out = apply_net.main(["--eval-only", "--coco-json", str(gt), "--output", str(tmp_path / "r.json"), "--test-dataset", "kitti_val",
                          "--min-allowed-score", "0.25"])
    assert out == {"ap": 1, "pm": 2, "ce": 3}
    (a, k), = calls
    assert a[:4] == (str(tmp_path / "r.json"), str(gt), "bdd_train", "kitti_val") and k["binary"] is False and k["min_allowed_score"] == 0.25
    calls.clear()
    apply_net.main(["--eval-only", "--coco-json", str(gt), "--binary-output", str(tmp_path / "r.podr")])
    (a, k), = calls
    assert a[0] == str(tmp_path / "r.podr") and k["binary"] is True
    calls.clear()
    apply_net.main(["--eval-only", "--coco-json", str(gt), "--binary-output", str(tmp_path / "r.podr"), "--output", str(tmp_path / "r.json")])
    (a, k), = calls
    assert a[0] == str(tmp_path / "r.json") and k["binary"] is False


def test_reg_edges_match_the_host_loop():
    """The 14 regression cdf edges the GPU pass bins against are the host loop's `i + step` values."""
    import torch
    from pod_compare_amd.calibration_gpu import _edges
    step = 1 / 15.0
    want = [i + step for i in torch.arange(0.0, 1.0 - step, step)]
    got = _edges()
    assert len(got) == len(want) == 14 and all(bool(a == b) and a.dtype == torch.float32 for a, b in zip(got, want))
    assert np.all(np.diff([float(x) for x in got]) > 0)
