"""PDQ, the probability-based detection quality of Hall et al., from a result file, on the GPU.

The reference does not implement PDQ: its README sends the user to a separate CPU tool ("For evaluating with PDQ, please use the official
PDQ code"), which reads neither the binary sidecar nor the KITTI / BDD category maps.  Here the metric is defined by this project
(include/pod_mi355x.h, K34, and DESIGN.md: box segments instead of masks, pixel centres, a fixed quadrature, a stated complement form), so
numbers are comparable with that tool's only up to those choices.  Results + ground truth -> per (ground truth, detection) pair the spatial
and label quality from the detection's two corner Gaussians (kernel pod_pdq_pairs) -> per image the maximum-weight assignment (kernel
pod_pdq_assign) -> PDQ = sum of the true positives' pPDQ / (TP + FP + FN).

    python -m pod_compare_amd.compute_pdq --results coco_instances_results.json --gt val_coco_format.json
    python -m pod_compare_amd.compute_pdq --binary-results results.podr --gt val_coco_format.json --map-results mAP_res.txt
    python -m pod_compare_amd.compute_pdq --results kitti_results.json --gt kitti_val.json --test-dataset kitti_val --p-min 0.01

Frame sizes come from the ground-truth json's `images` (width, height).  Detections are filtered by the minimum allowed score as
compute_probabilistic_metrics filters them.
"""
import argparse
import json
from typing import Dict, Optional, Sequence

PDQ_KEYS = ("PDQ", "avg_pPDQ", "avg_spatial", "avg_label", "avg_fg", "avg_bg")
P_MIN = 0.0027


def pdq_of_results(predicted_instances: Sequence[dict], gt: dict, cat_mapping_dict: Optional[Dict[int, int]] = None,
                   min_allowed_score: float = 0.0, p_min: float = P_MIN, device="cuda", ev=None) -> dict:
    """predicted_instances: the dicts of coco_instances_results.json; gt: the ground-truth json (its `images` give the frame sizes, its
    `annotations` the boxes); cat_mapping_dict: dataset category id -> contiguous id.  -> evaluation_utils.pdq_scores' dict."""
    if ev is None:
        from . import evaluation_utils as ev
    if cat_mapping_dict is None:
        from .compute_probabilistic_metrics import BDD_DATASET_ID_TO_CONTIGUOUS as cat_mapping_dict
    frame_sizes = {im["id"]: (int(im["width"]), int(im["height"])) for im in gt["images"]}
    pred = ev.eval_predictions_preprocess(predicted_instances, min_allowed_score, device=device)
    truth = ev.eval_gt_preprocess(gt["annotations"], device=device)
    return ev.pdq_scores(pred, truth, frame_sizes, cat_mapping_dict, p_min, device)


def format_table(res: dict) -> str:
    rows = [("PDQ", "avg pPDQ", "avg Spatial", "avg Label", "avg FG", "avg BG", "TP", "FP", "FN", "Invalid"),
            tuple("%.4f" % res[k] for k in PDQ_KEYS) + tuple(str(res[k]) for k in ("TP", "FP", "FN", "invalid_detections"))]
    w = [max(len(r[i]) for r in rows) for i in range(len(rows[0]))]
    line = "+" + "+".join("-" * (x + 2) for x in w) + "+"
    body = ["| " + " | ".join(r[i].center(w[i]) for i in range(len(r))) + " |" for r in rows]
    return "\n".join([line, body[0], line, body[1], line])


def add_pdq_arguments(ap) -> None:
    ap.add_argument("--p-min", type=float, default=P_MIN, help="PDQ: a pixel belongs to a detection's segment when P(pixel in box) >= this")


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser()
    ap.add_argument("--results", default="", help="coco_instances_results.json written by apply_net (AN:100-102)")
    ap.add_argument("--binary-results", default="", help="the binary sidecar instead (inference_utils.write_binary_results)")
    ap.add_argument("--gt", required=True, help="COCO-format ground truth json (its `images` and `annotations`)")
    ap.add_argument("--min-allowed-score", type=float, default=None, help="score threshold of the detections (default: from --map-results, else 0.0)")
    ap.add_argument("--map-results", default="", help="mAP_res.txt of compute_average_precision: its optimal-F1 score threshold, rounded to 4 decimals, is the min allowed score (PM:50-65)")
    ap.add_argument("--device", default="cuda")
    add_pdq_arguments(ap)
    from .apply_net import add_dataset_arguments
    add_dataset_arguments(ap)
    return ap


def main(argv=None):
    args = build_parser().parse_args(argv)
    if bool(args.results) == bool(args.binary_results):
        raise SystemExit("one of --results and --binary-results")
    if not 0.0 < args.p_min < 1.0:
        raise SystemExit("--p-min must lie in (0, 1)")
    from .apply_net import category_mapping, evaluation_category_map
    from .compute_average_precision import resolve_min_allowed_score
    args.min_allowed_score = resolve_min_allowed_score(args.min_allowed_score, args.map_results)
    if args.binary_results:
        from .inference_utils import binary_results_to_json
        predicted = binary_results_to_json(args.binary_results, category_mapping(args.train_dataset, args.test_dataset))
    else:
        with open(args.results, "r") as f:
            predicted = json.load(f)
    with open(args.gt, "r") as f:
        gt = json.load(f)
    res = pdq_of_results(predicted, gt, evaluation_category_map(args.train_dataset, args.test_dataset), args.min_allowed_score, args.p_min, args.device)
    print(format_table(res))
    return res


if __name__ == "__main__":
    main()
