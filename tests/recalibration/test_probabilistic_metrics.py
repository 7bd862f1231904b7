"""Recalibration end to end on the GPU: fit on a fold, apply to the complement, measure with the package's existing host calibration
errors against the bar the host restatement sets; apply_net --eval-only --recalibration; the JSON and the sidecar path."""
import json
import os

import numpy as np
import pytest
import torch

from pod_compare_amd import apply_net
from pod_compare_amd import compute_calibration_errors as cce
from pod_compare_amd import evaluation_utils as ev
from pod_compare_amd import inference_utils as iu
from pod_compare_amd import recalibrate as cli
from pod_compare_amd import recalibration as rc
from tests.recalibration import recal_fixture as fxt

pytestmark = pytest.mark.gpu
K = 7


def gpu_measure(predicted, gt):
    """Ground-truth matching on the GPU, then the package's HOST calibration_errors on the partitions."""
    pred = ev.eval_predictions_preprocess(predicted, 0.0, device="cuda")
    g = ev.eval_gt_preprocess(gt["annotations"], device="cuda")
    matched = ev.match_predictions_to_groundtruth(pred["predicted_boxes"], pred["predicted_cls_probs"], pred["predicted_covar_mats"],
                                                  g["gt_boxes"], g["gt_cat_idxs"], 0.1, 0.7, device="cuda")
    return fxt.measure(matched), matched


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    root = tmp_path_factory.mktemp("recal")
    predicted, gt, links = fxt.detection_set(300, 100, n_images=40)
    (root / "r.json").write_text(json.dumps(predicted))
    (root / "gt.json").write_text(json.dumps(gt))
    return root, predicted, gt, links


@pytest.mark.parametrize("reg", ["moment", "ece"])
def test_fit_on_a_fold_improves_the_complement(files, reg):
    """The test that cannot pass without the feature.  The bar: at least HALF the improvement ratio the host restatement alone reaches
    on the same split (tests/recalibration/recal_fixture.host_ratios; profiles/recalibration.md has the figures) -- the factor 2 covers
    the fp32 cdf of CE:240-256 against the fp64 counts the fit uses.  before / after_gpu >= (before / after_host) / 2 is asserted as
    after_gpu <= 2 after_host, which also reads correctly where the debiased marginal error of the host's result is exactly 0."""
    root, predicted, gt, links = files
    recal_file, r2, g2 = (str(root / n) for n in ("recal_%s.json" % reg, "r2_%s.json" % reg, "g2_%s.json" % reg))
    recal = cli.main(["fit", "--results", str(root / "r.json"), "--gt", str(root / "gt.json"), "--min-allowed-score", "0", "--reg", reg,
                      "--fold", "0/2", "--output", recal_file])
    assert recal.fold == [0, 2] and recal.n_matched == 150 and recal.n_scores == 200 * K and recal.invalid == [0] * 4
    assert recal.newton_iterations <= 50 and recal.cls_objective_after < recal.cls_objective_before
    if reg == "ece":
        assert all(a <= b for a, b in zip(recal.reg_objective_after, recal.reg_objective_before))
    cli.main(["apply", "--results", str(root / "r.json"), "--recalibration", recal_file, "--output", r2, "--gt", str(root / "gt.json"), "--gt-output", g2])
    pred2, gt2 = json.load(open(r2)), json.load(open(g2))
    ids = [im["id"] for im in gt["images"]]
    held_out = rc.fold_image_ids(ids, 0, 2, complement=True)
    assert {im["id"] for im in gt2["images"]} == held_out and {d["image_id"] for d in pred2} == held_out
    raw = [d for d in predicted if d["image_id"] in held_out]
    assert len(pred2) == len(raw) == 200 and all(list(a) == list(b) and a["bbox"] == b["bbox"] and a["category_id"] == b["category_id"] for a, b in zip(raw, pred2))
    (ece0, mce0), matched = gpu_measure(raw, gt2)
    (ece1, mce1), _ = gpu_measure(pred2, gt2)
    want = fxt.partitions(*fxt.restrict(predicted, gt, links, held_out))          # the matching is what the construction says
    assert matched["true_positives"]["predicted_box_means"].shape[0] == 150 and matched["duplicates"]["predicted_box_means"].shape[0] == 0
    assert matched["false_positives"]["predicted_box_means"].shape[0] == want["false_positives"]["predicted_box_means"].shape[0] == 50
    host_ece, host_mce, host_beta, host_scales = fxt.host_ratios(reg)
    print("%s: reg ECE %.6f -> %.6f (host %.6f -> %.6f), cls MCE %.6f -> %.6f (host %.6f -> %.6f), beta %.6f (host %.6f), scales %s (host %s)"
          % (reg, ece0, ece1, host_ece[0], host_ece[1], mce0, mce1, host_mce[0], host_mce[1], recal.beta, host_beta, recal.scales, host_scales))
    # the same held-out detections under the same measure (the partitions' row order differs: a bin's mean may move in its last bits)
    assert abs(ece0 - host_ece[0]) <= 1e-9 * ece0 and abs(mce0 - host_mce[0]) <= 1e-9 * mce0
    assert ece1 < ece0 and mce1 < mce0                               # both drop
    assert ece1 <= 2.0 * host_ece[1] and mce1 <= 2.0 * host_mce[1]   # at least half the host's improvement ratio
    assert abs(recal.beta - host_beta) <= 1e-9 * host_beta and np.allclose(recal.scales, host_scales, rtol=1e-12)


def test_apply_net_eval_only_with_a_recalibration_leaves_the_raw_files(files, capsys):
    root, predicted, gt, _ = files
    run = root / "run"
    run.mkdir(exist_ok=True)
    (run / "r.json").write_text(json.dumps(predicted))
    (run / "mAP_res.txt").write_text("sentinel: a raw run's file\n")
    recal = str(root / "recal_net.json")
    cli.main(["fit", "--results", str(root / "r.json"), "--gt", str(root / "gt.json"), "--min-allowed-score", "0", "--fold", "0/1", "--output", recal])
    capsys.readouterr()
    res = apply_net.main(["--eval-only", "--coco-json", str(root / "gt.json"), "--output", str(run / "r.json"), "--min-allowed-score", "0",
                          "--recalibration", recal])
    text = capsys.readouterr().out
    assert "Average Precision" in text and "Reg Ignorance Score" in text and "Cls Marginal Calibration Error" in text      # the three tables
    assert "recalibrated: beta" in text
    assert (run / "mAP_res.txt").read_text() == "sentinel: a raw run's file\n" and os.path.exists(str(run / "mAP_res_recalibrated.txt"))
    assert res["map_results"].endswith("mAP_res_recalibrated.txt") and set(res) >= {"ap", "pm", "ce"}
    torch.manual_seed(0)
    raw = cce.calibration_errors_of_results(predicted, gt["annotations"], dict(fxt.CMAP), 0.0)
    assert res["ce"]["reg_expected_calibration_error"] < raw["reg_expected_calibration_error"]
    assert json.load(open(str(run / "r.json"))) == predicted           # the result file itself is only read


def test_json_and_sidecar_paths_agree(files):
    root, predicted, gt, _ = files
    recal = rc.Recalibration(beta=0.55, scales=[[1.0 + 0.1 * c, 0.8, 1.2, 0.9 - 0.02 * c] for c in range(K)], per_class=True, fold=None)
    recal.save(str(root / "pc.json"))
    cmap = apply_net.category_mapping("bdd_train", "bdd_val")
    rec, counts, k, _ = rc.pack_results(predicted, {v: c for c, v in cmap.items()})
    image_ids = list(dict.fromkeys(d["image_id"] for d in predicted))
    iu.write_binary_results(str(root / "r.podr"), image_ids, counts, rec, k)
    cli.main(["apply", "--results", str(root / "r.json"), "--recalibration", str(root / "pc.json"), "--output", str(root / "a.json")])
    cli.main(["apply", "--results", str(root / "r.podr"), "--binary-results", "--recalibration", str(root / "pc.json"), "--output", str(root / "b.json")])
    cli.main(["apply", "--results", str(root / "r.json"), "--recalibration", str(root / "pc.json"), "--output", str(root / "c.podr"), "--binary-output"])
    a, b = json.load(open(str(root / "a.json"))), json.load(open(str(root / "b.json")))
    c = iu.binary_results_to_json(str(root / "c.podr"), cmap)
    assert len(a) == len(predicted) and a == b == c
    assert a != predicted and [d["image_id"] for d in a] == [d["image_id"] for d in predicted]
