"""PDQ (K34) against the fp64 referee on the GPU: the per-pair sums and quantities of the fixtures, and the metric end to end through
compute_pdq.main and apply_net --eval-only --pdq, from the json and from the binary sidecar.

The bound of a sum is pdq_ref.KERNEL_PIXEL_BOUND per pixel entering it: eight times the referee's own worst per-pixel error against
40-digit arithmetic (test_pdq_cpu.py), floor 1e-13 -- the margin covers the kernel's summation order and its quadrature, nothing else.
Measured on an MI355X (profiles/pdq.md): the worst sum errs by 0.083 of its bound (1e-13 per pixel); pPDQ and the q_* by 1.1e-16.

The module shares its name with tests/test_probabilistic_metrics.py for its place in the GPU run order (tests/conftest.py: GPU_ORDER)."""
import json

import numpy as np
import pytest
import torch

from tests.pdq import fixtures as fx
from tests.pdq import gpu_common as gc
from tests.pdq import pdq_ref as pr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def kernel():
    return gc.pairs(fx.all_images())


def test_no_fixture_pixel_sits_on_a_threshold():
    """The condition on the fixtures, on the referee's own numbers: no pixel has |P - p_min| < 1e-9 and no pixel of a segment has Q within a
    factor 1 +- 1e-6 of small -- otherwise a threshold could flip between the two implementations."""
    for m, r in enumerate(gc.referee()):
        m_p, m_q = r["margins"]
        print("PDQ_FIXTURE image %d: min |P - p_min| = %.3g, min |Q / small - 1| = %.3g" % (m, m_p, m_q))
        assert m_p >= 1e-9 and m_q >= 1e-6, m


def test_pairs_meet_the_referee(kernel):
    worst_sum, worst_q, pairs, where = 0.0, 0.0, 0, ""
    for m, (got, ref) in enumerate(zip(kernel, gc.referee())):
        assert np.array_equal(got["invalid"], ref["invalid"]), m
        for name, count in (("sum_fg", "n_fg"), ("sum_bg", "n_bg")):
            err = np.abs(got[name] - ref[name])
            bound = ref[count] * pr.KERNEL_PIXEL_BOUND
            ratio = np.where(bound > 0, err / np.maximum(bound, 1e-300), np.where(err == 0, 0.0, np.inf))
            if ratio.size and float(ratio.max()) > worst_sum:
                worst_sum = float(ratio.max())
                i, j = np.unravel_index(int(ratio.argmax()), ratio.shape)
                where = "%s of image %d, ground truth %d, detection %d: %.17g vs %.17g over %d pixels" % (name, m, i, j, got[name][i, j], ref[name][i, j], ref[count][i, j])
        for name in pr.PLANES:
            if got[name].size:
                worst_q = max(worst_q, float(np.abs(got[name] - ref[name]).max()))
        pairs += got["pPDQ"].size
    print("PDQ_PAIRS %d pairs: worst |sum - ref| / (pixels * %.3g) = %.3g; worst |quality - ref| = %.3g (bound %.3g)"
          % (pairs, pr.KERNEL_PIXEL_BOUND, worst_sum, worst_q, pr.QUALITY_BOUND))
    print("PDQ_PAIRS the worst sum: " + where)
    assert pairs >= 150 and worst_sum <= 1.0 and worst_q <= pr.QUALITY_BOUND


def test_the_fixtures_exercise_what_they_claim(kernel):
    ref = gc.referee()
    assert (ref[0]["pPDQ"] > 0.05).all()                                         # jittered detections overlap their ground truth
    assert (ref[1]["pPDQ"][0, 2:] > 0).all() and ref[1]["pPDQ"][1, 0] > 0       # whole-frame, floor, both clamps; the partly visible one
    assert (ref[1]["pPDQ"][:, 1] == 0).all()                                     # wholly off the frame
    assert (ref[2]["n_i"][1] == 0).all() and (ref[2]["n_i"][2] > 0).all() and ref[2]["invalid"].tolist() == [False, True, False, True]
    assert ref[6]["n_fg"][0, 0] > 0 and ref[6]["n_bg"][1, 0] > 256               # the strip: a segment wider than one chunk of columns
    assert (kernel[5]["pPDQ"] > 0).sum() >= 3


# ---- end to end ----------------------------------------------------------------------------------------------------------------------
IDS = (11, 12, 13, 14, 15, 16)


def _records(images):
    """The fixtures as K7's records (x, y, w, h, score, class, probs, T cov T^T): what both result files are written from."""
    from pod_compare_amd import inference_utils as iu
    width = iu.record_width(fx.K)
    rec = torch.zeros((len(images), 8, width), dtype=torch.float32)
    cnt = torch.zeros(len(images), dtype=torch.int32)
    for m, im in enumerate(images):
        D = len(im["means"])
        cnt[m] = D
        if D == 0:
            continue
        b = torch.from_numpy(im["means"]).clone()
        b[:, 2:] -= b[:, :2]
        p = torch.from_numpy(im["probs"])
        rec[m, :D, 0:4], rec[m, :D, 4], rec[m, :D, 5] = b, p.max(1).values, p.argmax(1).float()
        rec[m, :D, 6:6 + fx.K] = p
        rec[m, :D, 6 + fx.K:] = iu.covar_xyxy_to_xywh(torch.from_numpy(im["covs"]).double()).float().reshape(D, 16)
    return cnt, rec


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    from pod_compare_amd import apply_net
    from pod_compare_amd import evaluation_utils as ev
    from pod_compare_amd import inference_utils as iu
    d = tmp_path_factory.mktemp("pdq")
    zr = fx.zero_rules()
    zr = dict(zr, means=zr["means"][:3], covs=zr["covs"][:3], probs=zr["probs"][:3])          # (json has no infinity)
    images = [fx.jittered(), fx.edge_cases(), zr, fx.no_ground_truth(), fx.no_detections(), fx.many_ground_truths()]
    with_det = [m for m, im in enumerate(images) if len(im["means"])]                          # image 15 is absent from the results
    cnt, rec = _records([images[m] for m in with_det])
    ids = [IDS[m] for m in with_det]
    predicted = apply_net.results_json(ids, cnt, rec, fx.K, apply_net.BDD_CAT_MAP)
    (d / "r.json").write_text(json.dumps(predicted))
    iu.write_binary_results(str(d / "r.podr"), ids, cnt, rec, fx.K)
    gt = {"images": [{"id": i, "width": im["frame"][0], "height": im["frame"][1]} for i, im in zip(IDS, images)], "annotations": []}
    for i, im in zip(IDS, images):                                                             # image 14 is absent from the annotations
        for box, c in zip(im["gt_boxes"].astype(np.float64), im["gt_classes"]):
            gt["annotations"].append({"id": len(gt["annotations"]) + 1, "image_id": i, "category_id": int(c) + 1, "iscrowd": 0,
                                      "bbox": [box[0], box[1], box[2] - box[0], box[3] - box[1]], "area": float((box[2] - box[0]) * (box[3] - box[1]))})
    (d / "gt.json").write_text(json.dumps(gt))
    # the referee takes the very fp32 values the evaluation reads back from the files
    pred = ev.eval_predictions_preprocess(predicted, 0.0)
    truth = ev.eval_gt_preprocess(gt["annotations"])
    ref_images = []
    for i, im in zip(IDS, images):
        has_d, has_g = i in pred["predicted_boxes"], i in truth["gt_boxes"]
        ref_images.append({"frame": im["frame"],
                           "means": pred["predicted_boxes"][i].numpy() if has_d else np.zeros((0, 4), np.float32),
                           "covs": pred["predicted_covar_mats"][i].numpy() if has_d else np.zeros((0, 4, 4), np.float32),
                           "probs": pred["predicted_cls_probs"][i].numpy() if has_d else np.zeros((0, fx.K), np.float32),
                           "gt_boxes": truth["gt_boxes"][i].numpy() if has_g else np.zeros((0, 4), np.float32),
                           "gt_classes": (truth["gt_cat_idxs"][i].reshape(-1).numpy().astype(np.int64) - 1) if has_g else np.zeros(0, np.int64)})
    return d, pr.dataset_ref(ref_images)


def _check(res, ref):
    for k in ("TP", "FP", "FN", "invalid_detections"):
        assert res[k] == ref[k], (k, res[k], ref[k])
    for k in ("PDQ", "avg_pPDQ", "avg_spatial", "avg_label", "avg_fg", "avg_bg"):
        assert abs(res[k] - ref[k]) <= pr.QUALITY_BOUND, (k, res[k], ref[k])


def test_compute_pdq_main_from_json_and_sidecar(files, capsys):
    from pod_compare_amd import compute_pdq
    d, ref = files
    assert ref["TP"] >= 5 and ref["FP"] >= 3 and ref["FN"] >= 60 and ref["invalid_detections"] == 1 and ref["PDQ"] > 0.0
    a = compute_pdq.main(["--results", str(d / "r.json"), "--gt", str(d / "gt.json"), "--min-allowed-score", "0.0", "--device", "cuda:0"])
    out = capsys.readouterr().out
    assert "avg pPDQ" in out and "%.4f" % a["PDQ"] in out
    b = compute_pdq.main(["--binary-results", str(d / "r.podr"), "--gt", str(d / "gt.json"), "--min-allowed-score", "0.0", "--device", "cuda:0"])
    print("PDQ_END_TO_END PDQ = %.12f (referee %.12f), TP / FP / FN = %d / %d / %d" % (a["PDQ"], ref["PDQ"], a["TP"], a["FP"], a["FN"]))
    _check(a, ref)
    assert a == b                                                   # the json and the sidecar give the same numbers
    assert a["num_images"] == 6 and a["p_min"] == 0.0027


def test_apply_net_eval_only_pdq(files, monkeypatch, capsys):
    """apply_net --eval-only --pdq: the AP, PM and CE steps are stubbed (they have their own tests), PDQ runs for real on the files."""
    from pod_compare_amd import apply_net
    from pod_compare_amd import compute_average_precision as cap
    from pod_compare_amd import compute_calibration_errors as cce
    from pod_compare_amd import compute_probabilistic_metrics as cpm
    d, ref = files
    monkeypatch.setattr(cap, "coco_average_precision", lambda *a, **k: {"stats": [0.0] * 12, "optimal_score_threshold": 0.0})
    monkeypatch.setattr(cap, "write_map_results", lambda *a: None)
    monkeypatch.setattr(cpm, "probabilistic_metrics", lambda *a, **k: {"average": {}})
    monkeypatch.setattr(cpm, "format_table", lambda r: "")
    monkeypatch.setattr(cce, "calibration_errors_of_results", lambda *a, **k: {"cls_marginal_calibration_error_source": ""})
    monkeypatch.setattr(cce, "format_table", lambda r: "")
    argv = ["--eval-only", "--coco-json", str(d / "gt.json"), "--min-allowed-score", "0.0"]
    res = apply_net.main(argv + ["--pdq", "--output", str(d / "r.json")])
    _check(res["pdq"], ref)
    assert "avg pPDQ" in capsys.readouterr().out
    side = apply_net.main(argv + ["--pdq", "--binary-output", str(d / "r.podr")])
    assert side["pdq"] == res["pdq"]
    capsys.readouterr()
    plain =apply_net.main(argv + ["--output", str(d / "r.json")])
    assert "pdq" not in plain and "avg pPDQ" not in capsys.readouterr().out
