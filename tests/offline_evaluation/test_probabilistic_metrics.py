"""Offline evaluation step 1, COCO average precision, on the HIP kernels (pod_coco_eval_images / pod_coco_accumulate) against the
numpy restatement of COCOeval (tests/coco_eval_np.py): precision, recall, scores, the 12 stats and the optimal-F1 threshold, bit
for bit.

The module shares its name with tests/test_probabilistic_metrics.py (step 2 of the same chain, which reads this step's threshold
through --map-results) so that the GPU run order in tests/conftest.py (GPU_ORDER, keyed by module name) gives it a place: the suite
guard (tests/test_suite_guard_cpu.py) requires one for every GPU module."""
import json
import os

import numpy as np
import pytest
import torch

from pod_compare_amd import compute_average_precision as cap
from tests import coco_eval_np as ref
from tests.coco_eval_np import synthetic_set
from tests.helpers import GOLDEN

pytestmark = pytest.mark.gpu


def check_equal(predicted, gt_json, cat_ids):
    got = cap.coco_average_precision(predicted, gt_json, cat_ids=cat_ids, device="cuda")
    iou_thrs, rec_thrs, max_dets, area_rngs = cap.coco_params()
    gts, dts, img_ids = cap.load_annotations(predicted, gt_json)
    p, r, s = ref.evaluate_accumulate(gts, dts, img_ids, list(cat_ids), iou_thrs, rec_thrs, max_dets, area_rngs)
    assert np.array_equal(got["precision"], p)
    assert np.array_equal(got["recall"], r)
    assert np.array_equal(got["scores"], s)
    stats = ref.summarize(p, r, iou_thrs)
    assert np.array_equal(got["stats"], stats)
    thr = ref.optimal_score_threshold(p, s, rec_thrs)
    assert got["optimal_score_threshold"] == thr or (np.isnan(thr) and np.isnan(got["optimal_score_threshold"]))
    return got


def test_eval_metrics_fixture():
    z = np.load(os.path.join(GOLDEN, "eval_metrics.npz"))
    predicted, gt = json.loads(str(z["predicted_json"])), json.loads(str(z["gt_json"]))
    for cat_ids in ((1, 3), tuple(range(1, 8))):
        got = check_equal(predicted, gt, cat_ids)
    assert (got["precision"] > -1).any()


def test_synthetic_2000_images_7_classes():
    gt, predicted = synthetic_set(2000, seed=2024)
    got = check_equal(predicted, gt, tuple(range(1, 8)))
    assert (got["precision"][:, :, :, 0, 2] > 0).any()


def test_global_scratch_path_and_truncation():
    """One image: 80 ground-truth boxes of one class (more than POD_COCO_LDS_GT = 64, so the IoU matrix goes through scratch),
    120 + detections (cut at 100); plus ids from 0 and crowd boxes."""
    from pod_compare_amd import hip
    gt, predicted = synthetic_set(3, seed=5)
    n_big = sum(1 for a in gt["annotations"] if a["image_id"] == gt["images"][0]["id"] and a["category_id"] == 1)
    assert n_big > hip.POD_COCO_LDS_GT
    check_equal(predicted, gt, (1, 2, 3))


def test_edge_sets():
    gt, predicted = synthetic_set(40, seed=9, big_image=False)
    check_equal([], gt, (1, 3))                                               # empty result list
    check_equal(predicted, gt, (1, 3, 42))                                    # a category nobody has
    only_dets = {"images": gt["images"], "annotations": []}
    check_equal(predicted, only_dets, (1, 3))                                 # no ground truth at all


def test_predictor_on_planted_objects():
    """Dense head tensors with planted objects -> the HIP predictor -> result JSON -> AP on the HIP kernels.  The planted boxes
    are what the head regresses to, so AP@0.5 over the planted classes must be high: sanity bound 0.5."""
    from pod_compare_amd import hotpath, synthetic
    torch.cuda.set_device(0)
    size = (384, 512)
    anns, results = [], []
    for img in range(6):
        ho = synthetic.planted_head_outputs(size, 1, seed=300 + img, num_boxes=10)
        hp = hotpath.HotPath(ho.shapes, ho.anchors, hotpath.PathParams(), n_runs=1, has_cls_var=True, cov_dims=4, device="cuda:0")
        hd = ho.to("cuda:0")
        det = hp.run("bayes_od", hd.cls, hd.delta, hd.cls_var, hd.reg_var, image_size=size, out_size=size)
        m = det.count()
        boxes, scores, classes = det.boxes[:m].double().cpu().numpy(), det.scores[:m].double().cpu().numpy(), det.classes[:m].cpu().numpy()
        for b, s, c in zip(boxes, scores, classes):
            results.append({"image_id": img, "category_id": int(c) + 1, "bbox": [b[0], b[1], b[2] - b[0], b[3] - b[1]], "score": float(s)})
        for b, c in zip(ho.planted_boxes.double().numpy(), ho.planted_classes.numpy()):
            anns.append({"id": len(anns) + 1, "image_id": img, "category_id": int(c) + 1, "bbox": [b[0], b[1], b[2] - b[0], b[3] - b[1]],
                         "area": float((b[2] - b[0]) * (b[3] - b[1])), "iscrowd": 0})
    results = json.loads(json.dumps(results))                    # through JSON, as a result file
    gt = {"images": [{"id": i} for i in range(6)], "annotations": anns}
    cats = tuple(sorted({a["category_id"] for a in anns}))
    got = check_equal(results, gt, cats)
    print("planted objects: AP@0.5 = %.4f, AP = %.4f over classes %s" % (got["stats"][1], got["stats"][0], cats))
    assert got["stats"][1] >= 0.5, got["stats"]
