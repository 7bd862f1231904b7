"""COCO average precision and the classification score at the optimal F-1 score: step 1 of the offline evaluation chain.

Mirrors /root/reference/src/offline_evaluation/compute_average_precision.py (AP:16-69): pycocotools' `COCOeval(iouType='bbox')`
with the default `Params` on a result file, `params.catIds = [1, 3]` (AP:38), the 12 `summarize()` stats, the optimal-F1 score
threshold (AP:50-59, quirks included) and `mAP_res.txt` (AP:64-68), which compute_probabilistic_metrics / compute_calibration_errors
read back with `--map-results`.

pycocotools is not a dependency.  Its two loops run as HIP kernels (csrc/k17_coco_eval.hip, C ABI pod_coco_eval_images /
pod_coco_accumulate): `evaluateImg` as one workgroup per (image, category) pair, `accumulate` as a per-category stable sort plus
one workgroup per (category, area range, max detections, IoU threshold).  All of it fp64, as numpy computes it.  `summarize` and
the F-1 threshold are a few hundred numbers and stay in numpy here.

    python -m pod_compare_amd.compute_average_precision --results coco_instances_results.json --gt val_coco_format.json
    python -m pod_compare_amd.compute_average_precision --binary-results results.podr --gt val_coco_format.json --output mAP_res.txt

Ground truth follows `COCO.loadRes` semantics: a detection's `area` is w*h, its `iscrowd` 0 and its id its 1-based position in
the result list; result image ids must be ground-truth image ids.  Extension: a ground-truth annotation without `area` or
`iscrowd` takes w*h and 0, one without `id` its 1-based position in `annotations` (the BDD converter always writes all three;
pycocotools would fail without them).  A ground truth given as a bare annotation list (no `images`) takes its image ids from
the annotations and the results.
"""
import argparse
import json
from typing import Optional, Sequence

import numpy as np

DEFAULT_CAT_IDS = (1, 3)                     # AP:38
MAX_DETS = (1, 10, 100)
AREA_LABELS = ("all", "small", "medium", "large")


def coco_params():
    """pycocotools `Params.setDetParams`: iouThrs, recThrs (numpy linspace, exactly as pycocotools builds them), maxDets, areaRng."""
    iou_thrs = np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05)) + 1, endpoint=True)
    rec_thrs = np.linspace(.0, 1.00, int(np.round((1.00 - .0) / .01)) + 1, endpoint=True)
    area_rngs = [[0 ** 2, 1e5 ** 2], [0 ** 2, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2]]
    return iou_thrs, rec_thrs, list(MAX_DETS), area_rngs


def load_annotations(predicted: Sequence[dict], gt_json):
    """(gts, dts, img_ids) as `COCO(gt)` + `loadRes(predicted)` leave them.  gt_json: a path, a COCO dict or an annotation list."""
    if isinstance(gt_json, str):
        with open(gt_json, "r") as f:
            gt_json = json.load(f)
    anns = gt_json["annotations"] if isinstance(gt_json, dict) else list(gt_json)
    gts = []
    for pos, a in enumerate(anns):
        bb = [float(v) for v in a["bbox"]]
        gts.append({"image_id": a["image_id"], "category_id": a["category_id"], "bbox": bb,
                    "area": float(a["area"]) if "area" in a else bb[2] * bb[3],
                    "iscrowd": int(a.get("iscrowd", 0)), "id": a["id"] if "id" in a else pos + 1})
    dts = []
    for pos, r in enumerate(predicted):
        bb = [float(v) for v in r["bbox"]]
        dts.append({"image_id": r["image_id"], "category_id": r["category_id"], "bbox": bb, "score": float(r["score"]),
                    "area": bb[2] * bb[3], "iscrowd": 0, "id": pos + 1})
    res_imgs = {d["image_id"] for d in dts}
    if isinstance(gt_json, dict) and "images" in gt_json:
        img_set = {im["id"] for im in gt_json["images"]}
        if not res_imgs <= img_set:
            raise ValueError("Results do not correspond to current coco set")       # loadRes's assertion
    else:
        img_set = {g["image_id"] for g in gts} | res_imgs
    return gts, dts, sorted(img_set)


def summarize(precision: np.ndarray, recall: np.ndarray, iou_thrs: np.ndarray, max_dets=MAX_DETS) -> np.ndarray:
    """COCOeval.summarize: mean over the entries > -1 of the selected slice, -1 when there are none."""
    def stat(ap, iou_thr=None, area=0, max_det=100):
        m = list(max_dets).index(max_det)
        s = precision if ap else recall
        if iou_thr is not None:
            s = s[np.where(iou_thr == iou_thrs)[0]]
        s = s[:, :, :, area, m] if ap else s[:, :, area, m]
        v = s[s > -1]
        return -1.0 if v.size == 0 else float(np.mean(v))
    return np.array([stat(1), stat(1, iou_thr=.5), stat(1, iou_thr=.75), stat(1, area=1), stat(1, area=2), stat(1, area=3),
                     stat(0, max_det=max_dets[0]), stat(0, max_det=max_dets[1]), stat(0, max_det=max_dets[2]),
                     stat(0, area=1), stat(0, area=2), stat(0, area=3)], dtype=np.float64)


def optimal_score_threshold(precision: np.ndarray, scores: np.ndarray, rec_thrs: np.ndarray) -> float:
    """AP:50-59 as written: per class, the F-1 over recall thresholds of the IoU-mean precision (area 'all', 100 detections);
    argmax takes the first NaN (p = r = 0 gives 0/0) when there is one; -1 precision entries take part in the mean over IoU
    thresholds; the per-class score thresholds that are 0 are dropped before the mean over classes (NaN if all are)."""
    with np.errstate(invalid="ignore", divide="ignore"):
        p = precision.mean(0)[:, :, 0, 2]
        r = np.expand_dims(rec_thrs, 1)
        f1 = 2 * (p * r) / (p + r)
        best = f1.argmax(0)
        sc = scores.mean(0)[:, :, 0, 2]
        thr = np.array([sc[b, i] for i, b in enumerate(best)], dtype=np.float64)
        thr = thr[thr != 0]
        return float(thr.mean()) if thr.size else float("nan")


def coco_average_precision(predicted: Sequence[dict], gt_json, cat_ids: Sequence[int] = DEFAULT_CAT_IDS, device="cuda",
                           impl=None) -> dict:
    """AP:35-59.  predicted: the dicts of coco_instances_results.json; gt_json: COCO ground truth (path, dict or annotation list).
    impl: `f(gts, dts, img_ids, cat_ids, iou_thrs, rec_thrs, max_dets, area_rngs) -> (precision, recall, scores)` replacing the
    HIP evaluate + accumulate (tests plug a numpy restatement in here).  Returns {"stats", "precision", "recall", "scores",
    "optimal_score_threshold"} with pycocotools' array layouts [T, R, K, A, M] / [T, K, A, M]."""
    iou_thrs, rec_thrs, max_dets, area_rngs = coco_params()
    gts, dts, img_ids = load_annotations(predicted, gt_json)
    cat_ids = [int(c) for c in cat_ids]
    if impl is None:
        from .coco_eval import evaluate_accumulate
        precision, recall, scores = evaluate_accumulate(gts, dts, img_ids, cat_ids, iou_thrs, rec_thrs, max_dets, area_rngs, device=device)
    else:
        precision, recall, scores = impl(gts, dts, img_ids, cat_ids, iou_thrs, rec_thrs, max_dets, area_rngs)
    stats = summarize(precision, recall, iou_thrs, max_dets)
    return {"stats": stats, "precision": precision, "recall": recall, "scores": scores,
            "optimal_score_threshold": optimal_score_threshold(precision, scores, rec_thrs)}


def format_summary(stats: np.ndarray) -> str:
    """COCOeval.summarize's printout."""
    rows = [(1, "0.50:0.95", "all", 100), (1, "0.50", "all", 100), (1, "0.75", "all", 100), (1, "0.50:0.95", "small", 100),
            (1, "0.50:0.95", "medium", 100), (1, "0.50:0.95", "large", 100), (0, "0.50:0.95", "all", 1), (0, "0.50:0.95", "all", 10),
            (0, "0.50:0.95", "all", 100), (0, "0.50:0.95", "small", 100), (0, "0.50:0.95", "medium", 100), (0, "0.50:0.95", "large", 100)]
    out = []
    for (ap, iou, area, md), v in zip(rows, stats):
        title, short = ("Average Precision", "(AP)") if ap else ("Average Recall", "(AR)")
        out.append(" {:<18} {} @[ IoU={:<9} | area={:>6s} | maxDets={:>3d} ] = {:0.3f}".format(title, short, iou, area, md, v))
    return "\n".join(out)


def write_map_results(path: str, stats: np.ndarray, threshold: float) -> None:
    """AP:64-68: `print(stats.tolist() + [thr], file=f)` (the threshold as a plain float, so the line parses as AP's did)."""
    with open(path, "w") as f:
        print(np.asarray(stats, dtype=np.float64).tolist() + [float(threshold)], file=f)


def read_min_allowed_score(path: str) -> float:
    """PM:58-60 / CE:56-58: the last entry of mAP_res.txt, rounded to 4 decimals."""
    with open(path, "r") as f:
        min_allowed_score = f.read().strip('][\n').split(', ')[-1]
    return round(float(min_allowed_score), 4)


def resolve_min_allowed_score(min_allowed_score: Optional[float], map_results: str = "") -> float:
    """PM:50-65 / CE:50-62: an explicit threshold wins; else the one in mAP_res.txt; else 0.0 (the reference's fallback, which it
    calls "not recommended")."""
    if min_allowed_score is not None:
        return float(min_allowed_score)
    if map_results:
        return read_min_allowed_score(map_results)
    return 0.0


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--results", default="", help="coco_instances_results.json written by apply_net (AN:100-102)")
    ap.add_argument("--binary-results", default="", help="the binary sidecar instead (inference_utils.write_binary_results)")
    ap.add_argument("--gt", required=True, help="COCO-format ground truth json")
    ap.add_argument("--cat-ids", default=",".join(str(c) for c in DEFAULT_CAT_IDS), help="evaluated category ids (AP:38: 1,3)")
    ap.add_argument("--output", default="", help="write mAP_res.txt here (AP:64-68)")
    ap.add_argument("--device", default="cuda")
    from .apply_net import add_dataset_arguments, category_mapping
    add_dataset_arguments(ap)
    args = ap.parse_args(argv)
    if bool(args.results) == bool(args.binary_results):
        ap.error("give exactly one of --results / --binary-results")
    if args.binary_results:
        from .inference_utils import binary_results_to_json
        predicted = binary_results_to_json(args.binary_results, category_mapping(args.train_dataset, args.test_dataset))
    else:
        with open(args.results, "r") as f:
            predicted = json.load(f)
    cat_ids = [int(c) for c in args.cat_ids.split(",") if c.strip()]
    res = coco_average_precision(predicted, args.gt, cat_ids=cat_ids, device=args.device)
    print(format_summary(res["stats"]))
    print("Classification Score at Optimal F-1 Score: {}".format(res["optimal_score_threshold"]))
    if args.output:
        write_map_results(args.output, res["stats"], res["optimal_score_threshold"])
    return res


if __name__ == "__main__":
    main()
