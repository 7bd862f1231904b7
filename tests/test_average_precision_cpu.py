"""compute_average_precision (AP:16-69) on the CPU: the driver with the numpy restatement of COCOeval (tests/coco_eval_np.py)
plugged in through `impl=`, on hand-worked cases whose answers are written out here; the mAP_res.txt round trip; and the
--map-results option of compute_probabilistic_metrics / compute_calibration_errors.

pycocotools is not installed here, so these cases, not a pycocotools run, anchor the restatement that the GPU tests compare the
HIP kernels with."""
import json

import numpy as np
import pytest

from pod_compare_amd import compute_average_precision as cap
from tests import coco_eval_np as ref

EPS = np.spacing(1)
ONE = 1.0 / (1.0 + EPS)          # pr of one true positive: 1 / (0 + 1 + eps) rounds below 1
IOU_THRS, REC_THRS, _, _ = cap.coco_params()
ALL, SMALL, MEDIUM, LARGE = 0, 1, 2, 3


def t_mean(v):
    """A score entry of v at every IoU threshold, averaged the way AP:55 averages it (axis 0 of the [T, R, K, A, M] table)."""
    return np.full((10, 101, 2, 4, 3), v).mean(0)[0, 0, 0, 0]


MEAN8 = t_mean(.8)               # 0.7999999999999999


def gt(img, box, cat=1, **kw):
    return dict({"image_id": img, "category_id": cat, "bbox": list(map(float, box))}, **kw)


def det(img, box, score, cat=1):
    return {"image_id": img, "category_id": cat, "bbox": list(map(float, box)), "score": float(score)}


def run(dets, gts, cat_ids=(1,)):
    return cap.coco_average_precision(dets, gts, cat_ids=cat_ids, impl=ref.evaluate_accumulate)


def prec(res, t=slice(None), k=0, a=ALL, m=2):
    return res["precision"][t, :, k, a, m]


BIG = (0, 0, 120, 120)            # area 14400: 'large'
BIG2 = (300, 300, 110, 110)
FAR = (600, 600, 120, 120)        # no overlap with the above


def test_perfect_detections():
    res = run([det(1, BIG, .9), det(2, BIG2, .8)], [gt(1, BIG), gt(2, BIG2)])
    assert np.array_equal(prec(res), np.ones((10, 101)))           # two true positives: 2 / (2 + eps) == 1.0
    assert np.array_equal(prec(res, a=LARGE), np.ones((10, 101)))
    assert np.all(prec(res, a=SMALL) == -1) and np.all(prec(res, a=MEDIUM) == -1)   # no ground truth in those ranges
    assert np.all(res["recall"][:, 0, ALL, :] == 1.0)          # maxDets 1 / 10 / 100 cut per image: one box each
    want = [1.0, 1.0, 1.0, -1.0, -1.0, 1.0, 1.0, 1.0, 1.0, -1.0, -1.0, 1.0]
    assert res["stats"].tolist() == want


def test_false_positive_above_true_positive():
    res = run([det(1, FAR, .9), det(1, BIG, .8)], [gt(1, BIG)])
    # order FP, TP: tp [0, 1], fp [1, 1]; rc [0, 1]; pr [0, 1 / (2 + eps)] = [0, .5]; envelope [.5, .5]
    assert np.array_equal(prec(res), np.full((10, 101), .5))
    sc = res["scores"][:, :, 0, ALL, 2]
    assert np.all(sc[:, 0] == .9) and np.all(sc[:, 1:] == .8)       # searchsorted(rc, 0) = 0 -> the FP's score
    assert np.all(res["recall"][:, 0, ALL, 2] == 1.0)


def test_crowd_box_absorbs_several_detections():
    crowd = gt(1, (200, 200, 300, 300), iscrowd=1)
    dets = [det(1, BIG, .9), det(1, (210, 210, 50, 50), .8), det(1, (300, 300, 60, 60), .7)]
    res = run(dets, [gt(1, BIG), crowd])
    # the two detections inside the crowd box match it (IoU = intersection / detection area = 1) and are ignored, not FPs
    assert np.array_equal(prec(res), np.full((10, 101), ONE))
    without = run(dets, [gt(1, BIG)])
    assert np.all(prec(without)[:, 1:] == ONE) and prec(without)[0, 0] == ONE and without["precision"][0, 100, 0, 0, 2] == ONE
    assert np.all(without["scores"][:, :, 0, ALL, 2] == .9)
    assert np.array_equal(res["recall"][:, 0, ALL, 2], np.ones(10))


def test_ground_truth_ignored_by_area_range():
    small, medium = (0, 0, 20, 20), (100, 100, 50, 50)               # areas 400 ('small'), 2500 ('medium')
    res = run([det(1, medium, .9), det(1, small, .8)], [gt(1, small), gt(1, medium)])
    # medium range: the small box is ignored, so is the detection matched to it -> [TP, ignored]
    assert np.array_equal(prec(res, a=MEDIUM), np.full((10, 101), ONE))
    # small range: [ignored (matched the ignored medium box), TP]: rc [0, 1], pr [0, ONE]; the recall-0 entry takes the
    # ignored detection's score
    assert np.array_equal(prec(res, a=SMALL), np.full((10, 101), ONE))
    sc = res["scores"][:, :, 0, SMALL, 2]
    assert np.all(sc[:, 0] == .9) and np.all(sc[:, 1:] == .8)
    assert np.all(prec(res, a=LARGE) == -1)
    # an unmatched detection whose own area is out of range is ignored: a stray small box does not hurt 'medium'
    res2 = run([det(1, medium, .9), det(1, (400, 400, 10, 10), .95)], [gt(1, medium)])
    assert np.array_equal(prec(res2, a=MEDIUM), np.full((10, 101), ONE))
    assert np.array_equal(prec(res2, a=ALL), np.full((10, 101), .5))


def test_score_ties_across_images_follow_image_order():
    # image 5's detection comes first in the file, but sorted imgIds put image 2 first: order [FP (img 2), TP (img 5)]
    res = run([det(5, BIG, .5), det(2, FAR, .5)], [gt(5, BIG), gt(2, BIG)])
    want = np.where(REC_THRS <= .5, .5, 0.0)                            # rc [0, .5], pr [0, .5]
    assert np.array_equal(prec(res), np.tile(want, (10, 1)))
    assert np.all(res["recall"][:, 0, ALL, 2] == .5)


def test_score_ties_within_an_image_follow_file_order():
    res = run([det(1, FAR, .5), det(1, BIG, .5)], [gt(1, BIG)])         # [FP, TP]
    assert np.array_equal(prec(res), np.full((10, 101), .5))
    res = run([det(1, BIG, .5), det(1, FAR, .5)], [gt(1, BIG)])         # [TP, FP]: pr [ONE, .5]; rc [1, 1]
    assert np.array_equal(prec(res), np.full((10, 101), ONE))


def test_more_than_100_detections_are_truncated():
    g1, g2 = (0, 0, 120, 120), (1000, 1000, 120, 120)
    fps = [det(1, (2000 + 10 * i, 0, 120, 120), .99 - .001 * i) for i in range(99)]
    dets = fps + [det(1, g1, .5), det(1, g2, .1)]                         # the TP on g2 is detection 101: cut
    res = run(dets, [gt(1, g1), gt(1, g2)])
    assert np.all(res["recall"][:, 0, ALL, 2] == .5)                      # only g1 is found
    want = np.where(REC_THRS <= .5, 1.0 / (100 + EPS), 0.0)               # pr at the TP: 1 / (99 + 1 + eps) = .01
    assert np.array_equal(prec(res), np.tile(want, (10, 1)))
    assert np.all(res["recall"][:, 0, ALL, 1] == 0.0)                     # maxDets 10: FPs only
    assert np.all(prec(res, m=1) == 0.0)


def test_ground_truth_id_zero_reads_as_unmatched():
    """pycocotools records matches as ids: dtm = the ground truth's id, so a detection matched to the box with id 0 has
    dtm == 0 and counts as a false positive.  The box itself is taken (gtm holds the detection's id, which loadRes numbers from
    1), so a second detection cannot match it and goes to its next best box."""
    g0, g7 = (0, 0, 100, 100), (10, 0, 100, 100)
    d1, d2 = (0, 0, 100, 100), (2, 0, 100, 100)   # d1: IoU 1 with g0; d2: IoU .96 with g0, 92/108 = .852 with g7
    res = run([det(1, d1, .9), det(1, d2, .8)], [gt(1, g0, id=0), gt(1, g7, id=7)])
    # IoU .5 .. .85: [FP (id 0), TP (g7)] -> rc [0, .5], pr [0, .5]
    want = np.where(REC_THRS <= .5, .5, 0.0)
    assert np.array_equal(prec(res, t=slice(0, 8)), np.tile(want, (8, 1)))
    assert np.all(res["recall"][:8, 0, ALL, 2] == .5)
    # IoU .9, .95: d2 matches nothing -> [FP, FP]
    assert np.all(prec(res, t=slice(8, 10)) == 0.0) and np.all(res["recall"][8:, 0, ALL, 2] == 0.0)
    # with a nonzero id the same match is a true positive
    res1 = run([det(1, d1, .9), det(1, d2, .8)], [gt(1, g0, id=3), gt(1, g7, id=7)])
    assert np.array_equal(prec(res1, t=0), np.full(101, 1.0))


def test_category_without_ground_truth_stays_minus_one():
    res = run([det(1, BIG, .9), det(1, BIG2, .8, cat=3)], [gt(1, BIG)], cat_ids=(1, 3))
    assert np.all(res["precision"][:, :, 1] == -1) and np.all(res["recall"][:, 1] == -1) and np.all(res["scores"][:, :, 1] == -1)
    assert np.array_equal(prec(res), np.full((10, 101), ONE))


def test_image_without_detections():
    res = run([det(1, BIG, .9)], [gt(1, BIG), gt(2, BIG)])
    assert np.all(res["recall"][:, 0, ALL, 2] == .5)
    assert np.array_equal(prec(res), np.tile(np.where(REC_THRS <= .5, ONE, 0.0), (10, 1)))


def test_empty_result_list():
    res = run([], [gt(1, BIG), gt(2, BIG2)])
    assert np.all(prec(res) == 0.0) and np.all(res["scores"][:, :, 0, ALL, 2] == 0.0) and np.all(res["recall"][:, 0, ALL] == 0.0)
    assert np.all(prec(res, a=SMALL) == -1)
    assert res["stats"].tolist() == [0.0, 0.0, 0.0, -1.0, -1.0, 0.0, 0.0, 0.0, 0.0, -1.0, -1.0, 0.0]
    assert np.isnan(res["optimal_score_threshold"])                      # every per-class threshold is 0 and dropped


def test_f1_quirk_minus_one_precision_enters_the_mean():
    """Category 3 has no ground truth: precision -1 everywhere, so F1 = 2(-r)/(r - 1) peaks at r = .99 and the category
    contributes its score entry there, -1, to the mean."""
    res = run([det(1, BIG, .8), det(2, BIG2, .8)], [gt(1, BIG), gt(2, BIG2)], cat_ids=(1, 3))
    assert res["optimal_score_threshold"] == np.mean([MEAN8, -1.0])


def test_f1_quirk_zero_thresholds_are_dropped():
    """Category 3 has ground truth and no detections: its score entry is 0 and leaves the mean."""
    res = run([det(1, BIG, .8), det(2, BIG2, .8)], [gt(1, BIG), gt(2, BIG2), gt(1, BIG, cat=3)], cat_ids=(1, 3))
    assert res["optimal_score_threshold"] == MEAN8


def test_f1_quirk_nan_wins_argmax():
    """Category 3 has only false positives: precision 0, so F1 at recall 0 is 0/0 = NaN, and argmax returns it: the threshold is
    that category's score entry at recall 0 (its first detection's score, .7)."""
    res = run([det(1, BIG, .8), det(2, BIG2, .8), det(1, FAR, .7, cat=3)], [gt(1, BIG), gt(2, BIG2), gt(1, BIG, cat=3)],
              cat_ids=(1, 3))
    p = res["precision"].mean(0)[:, 1, 0, 2]
    with np.errstate(invalid="ignore"):
        assert np.isnan(2 * p[0] * 0.0 / (p[0] + 0.0))
    assert res["optimal_score_threshold"] == np.mean([MEAN8, t_mean(.7)])


def test_package_summary_and_threshold_match_restatement():
    rng = np.random.default_rng(7)
    gts, dets = [], []
    for img in range(12):
        for _ in range(rng.integers(0, 5)):
            x, y, w, h = rng.uniform(0, 400), rng.uniform(0, 400), rng.uniform(10, 150), rng.uniform(10, 150)
            gts.append(gt(img, (x, y, w, h), cat=int(rng.choice([1, 3])), iscrowd=int(rng.random() < .1)))
            for _ in range(rng.integers(0, 3)):
                dets.append(det(img, (x + rng.normal(0, 8), y + rng.normal(0, 8), w * rng.uniform(.8, 1.2), h * rng.uniform(.8, 1.2)),
                                round(rng.random(), 2), cat=gts[-1]["category_id"]))
    res = run(dets, gts, cat_ids=(1, 3))
    assert np.array_equal(res["stats"], ref.summarize(res["precision"], res["recall"], IOU_THRS))
    want = ref.optimal_score_threshold(res["precision"], res["scores"], REC_THRS)
    assert res["optimal_score_threshold"] == want


def test_gt_annotation_defaults_and_image_check():
    gts, dts, imgs = cap.load_annotations([det(4, (0, 0, 2, 3), .5)], [gt(4, (1, 1, 4, 5)), gt(2, (0, 0, 1, 1), id=9, area=7.0, iscrowd=1)])
    assert [(g["area"], g["iscrowd"], g["id"]) for g in gts] == [(20.0, 0, 1), (7.0, 1, 9)]
    assert dts[0]["area"] == 6.0 and dts[0]["id"] == 1 and imgs == [2, 4]
    with pytest.raises(ValueError):
        cap.load_annotations([det(4, (0, 0, 2, 3), .5)], {"images": [{"id": 2}], "annotations": []})


def _patch_hip(monkeypatch):
    from pod_compare_amd import coco_eval
    monkeypatch.setattr(coco_eval, "evaluate_accumulate", lambda *a, device=None: ref.evaluate_accumulate(*a))


def test_cli_writes_map_results_that_pm_ce_read(tmp_path, monkeypatch):
    _patch_hip(monkeypatch)
    results, gtf, out = tmp_path / "coco_instances_results.json", tmp_path / "gt.json", tmp_path / "mAP_res.txt"
    results.write_text(json.dumps([det(1, BIG, .8123456), det(2, FAR, .61), det(2, BIG2, .55)]))
    gtf.write_text(json.dumps({"images": [{"id": 1}, {"id": 2}], "annotations": [gt(1, BIG, id=1), gt(2, BIG2, id=2)]}))
    res = cap.main(["--results", str(results), "--gt", str(gtf), "--cat-ids", "1", "--output", str(out)])
    line = out.read_text()
    assert line == str(res["stats"].tolist() + [res["optimal_score_threshold"]]) + "\n"
    thr = res["optimal_score_threshold"]
    assert not np.isnan(thr)
    # PM:58-60 / CE:56-58, verbatim
    parsed = round(float(line.strip('][\n').split(', ')[-1]), 4)
    assert parsed == round(thr, 4) == cap.read_min_allowed_score(str(out))


def test_map_results_sets_pm_and_ce_min_allowed_score(tmp_path, monkeypatch):
    from pod_compare_amd import compute_calibration_errors as ce
    from pod_compare_amd import compute_probabilistic_metrics as pm
    from pod_compare_amd import evaluation_utils
    mres = tmp_path / "mAP_res.txt"
    cap.write_map_results(str(mres), np.zeros(12), 0.43218765)
    results, gtf = tmp_path / "r.json", tmp_path / "gt.json"
    results.write_text("[]")
    gtf.write_text(json.dumps({"annotations": []}))
    seen = []

    class Stop(Exception):
        pass

    def fake_pm(*a, min_allowed_score=None, **kw):
        seen.append(min_allowed_score)
        raise Stop()

    def fake_pre(predicted, min_allowed_score, device=None):
        seen.append(min_allowed_score)
        raise Stop()

    monkeypatch.setattr(pm, "probabilistic_metrics", fake_pm)
    monkeypatch.setattr(evaluation_utils, "eval_predictions_preprocess", fake_pre)
    for mod in (pm, ce):
        for extra in (["--map-results", str(mres)], [], ["--map-results", str(mres), "--min-allowed-score", "0.2"]):
            with pytest.raises(Stop):
                mod.main(["--results", str(results), "--gt", str(gtf)] + extra)
    assert seen == [0.4322, 0.0, 0.2] * 2
