"""Fit a recalibration on one fold of a validation set and apply it to the rest (recalibration.py, csrc/k36_recalibrate.hip).

    python -m pod_compare_amd.recalibrate fit --results coco_instances_results.json --gt val_coco_format.json --map-results mAP_res.txt \\
        --reg ece --fold 0/2 --output recal.json
    python -m pod_compare_amd.recalibrate apply --results coco_instances_results.json --recalibration recal.json --output recalibrated.json \\
        --gt val_coco_format.json --gt-output val_complement.json

`fit` matches the fold's detections to its ground truth on the GPU (pod_match_groundtruth), fits one temperature and per-coordinate
variance scales (K36) and writes a small JSON of settings.  `apply` transforms a result file -- JSON or the binary sidecar -- on the GPU and
writes, by default, only the images outside the fit fold, with the ground truth restricted to the same images when asked: every
evaluator of the package then runs unchanged on the pair.
"""
import argparse
import json

import torch

from . import recalibration as rc


def _load_results(path: str, binary: bool, train_dataset: str, test_dataset: str):
    """-> (result dicts or None, (ids, counts, records, K) or None)."""
    if binary:
        from .inference_utils import read_binary_results
        return None, read_binary_results(path)
    with open(path, "r") as f:
        return json.load(f), None


def _class_of_category(train_dataset: str, test_dataset: str):
    from .apply_net import category_mapping
    ids_of = category_mapping(train_dataset, test_dataset)
    return {v: k for k, v in ids_of.items()} if len(set(ids_of.values())) == len(ids_of) else None


def fit_main(args) -> rc.Recalibration:
    from . import evaluation_utils as ev
    from .apply_net import category_mapping, evaluation_category_map
    from .compute_average_precision import resolve_min_allowed_score
    k, n = rc.parse_fold(args.fold)
    thr = resolve_min_allowed_score(args.min_allowed_score, args.map_results)
    predicted, table = _load_results(args.results, args.binary_results, args.train_dataset, args.test_dataset)
    if predicted is None:
        from .apply_net import results_json
        ids, counts, rec, K = table
        predicted = results_json(ids, counts, rec, K, category_mapping(args.train_dataset, args.test_dataset))
    with open(args.gt, "r") as f:
        gt = json.load(f)
    keep = rc.fold_image_ids([im["id"] for im in gt["images"]], k, n)
    predicted = [d for d in predicted if d["image_id"] in keep]
    annotations = [a for a in gt["annotations"] if a["image_id"] in keep]
    dev = args.device
    pred = ev.eval_predictions_preprocess(predicted, thr, device=dev)
    g = ev.eval_gt_preprocess(annotations, device=dev)
    matched = ev.match_predictions_to_groundtruth(pred["predicted_boxes"], pred["predicted_cls_probs"], pred["predicted_covar_mats"],
                                                  g["gt_boxes"], g["gt_cat_idxs"], args.iou_min, args.iou_correct, device=dev)
    recal = rc.fit_recalibration(matched, evaluation_category_map(args.train_dataset, args.test_dataset), cls=args.cls, reg=args.reg,
                                 per_class_reg=args.per_class_reg, device=dev, fold=(k, n), min_allowed_score=thr)
    recal.save(args.output)
    print(rc.format_table(recal))
    print("wrote %s (%d images of %d in fold %d/%d)" % (args.output, len(keep), len(set(im["id"] for im in gt["images"])), k, n))
    return recal


def apply_main(args) -> dict:
    from .apply_net import category_mapping, results_json
    from .inference_utils import write_binary_results
    recal = rc.Recalibration.load(args.recalibration)
    fold = rc.parse_fold(args.fold) if args.fold else (tuple(recal.fold) if recal.fold is not None else None)
    complement = args.complement if args.complement is not None else (recal.fold is not None and not args.fold)
    predicted, table = _load_results(args.results, args.binary_results, args.train_dataset, args.test_dataset)
    gt = None
    if args.gt:
        with open(args.gt, "r") as f:
            gt = json.load(f)
    keep = None
    if fold is not None:
        if gt is None:
            raise SystemExit("--fold (or a recalibration file that records one) ranks the images of the ground truth: give --gt")
        keep = rc.fold_image_ids([im["id"] for im in gt["images"]], fold[0], fold[1], complement=bool(complement))
    dev = torch.device(args.device)
    if table is None:
        if keep is not None:
            predicted = [d for d in predicted if d["image_id"] in keep]
        cls_of = _class_of_category(args.train_dataset, args.test_dataset)
        if args.binary_output:
            rec, counts, K, _ = rc.pack_results(predicted, cls_of)
            ids = list(dict.fromkeys(d["image_id"] for d in predicted))
        else:
            out = rc.apply_to_results(predicted, recal, cls_of, device=dev)
    else:
        ids, counts, rec, K = table
        if keep is not None:
            rows = [r for r, i in enumerate(ids) if i in keep]
            ids, counts, rec = [ids[r] for r in rows], counts[rows], rec[rows]
    if table is not None or args.binary_output:
        rec = rc.apply_to_records(rec.to(dev), counts.to(dev), K, recal).cpu()
        if args.binary_output:
            write_binary_results(args.output, ids, counts, rec, K)
        else:
            out = results_json(ids, counts, rec, K, category_mapping(args.train_dataset, args.test_dataset))
    if not args.binary_output:
        with open(args.output, "w") as f:
            json.dump(out, f, indent=4, separators=(",", ": "))
    n_images = len(keep) if keep is not None else None
    if args.gt_output:
        if gt is None:
            raise SystemExit("--gt-output restricts --gt: give --gt")
        sub = dict(gt)
        if keep is not None:
            sub["images"] = [im for im in gt["images"] if im["id"] in keep]
            sub["annotations"] = [a for a in gt["annotations"] if a["image_id"] in keep]
        with open(args.gt_output, "w") as f:
            json.dump(sub, f)
    print("wrote %s%s" % (args.output, "" if n_images is None else " (%d images%s)" % (n_images, ", the fit fold's complement" if complement else "")))
    return {"output": args.output, "images": sorted(keep) if keep is not None else None}


def build_parser() -> argparse.ArgumentParser:
    from .apply_net import add_dataset_arguments
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest="command", required=True)
    fit = sub.add_parser("fit", help="fit a temperature and variance scales on one fold")
    fit.add_argument("--results", required=True, help="coco_instances_results.json, or with --binary-results its binary sidecar")
    fit.add_argument("--binary-results", action="store_true", help="--results is the binary sidecar (inference_utils.write_binary_results)")
    fit.add_argument("--gt", required=True, help="COCO-format ground truth json (`images` and `annotations`)")
    fit.add_argument("--map-results", default="", help="mAP_res.txt: its optimal-F1 score threshold is the min allowed score (CE:50-62)")
    fit.add_argument("--min-allowed-score", type=float, default=None)
    fit.add_argument("--iou-min", type=float, default=0.1)
    fit.add_argument("--iou-correct", type=float, default=0.7)
    fit.add_argument("--cls", default="temperature", help="temperature | none (per_class is refused: it could change the arg-max class)")
    fit.add_argument("--reg", default="moment", choices=("moment", "ece", "none"))
    fit.add_argument("--per-class-reg", action="store_true", help="one row of variance scales per class instead of one for all")
    fit.add_argument("--fold", default="0/2", help="k/n: fit on the images whose rank among the ground truth's sorted image ids is = k (mod n); 0/1: all")
    fit.add_argument("--output", required=True, help="the recalibration file (JSON, settings only)")
    fit.add_argument("--device", default="cuda")
    add_dataset_arguments(fit)
    app = sub.add_parser("apply", help="apply a fitted recalibration to a result file")
    app.add_argument("--results", required=True)
    app.add_argument("--binary-results", action="store_true", help="--results is the binary sidecar")
    app.add_argument("--recalibration", required=True, help="the file `fit` wrote")
    app.add_argument("--output", required=True)
    app.add_argument("--binary-output", action="store_true", help="write --output as a binary sidecar")
    app.add_argument("--gt", default="", help="the ground truth json: needed to rank the images of a fold")
    app.add_argument("--gt-output", default="", help="write --gt restricted to the images of --output here")
    app.add_argument("--fold", default="", help="k/n (default: the fold the file records, if any)")
    app.add_argument("--complement", dest="complement", action="store_true", default=None,
                     help="write the images OUTSIDE the fold (the default when the fold is the one the file records)")
    app.add_argument("--no-complement", dest="complement", action="store_false", help="write the fold's own images")
    app.add_argument("--device", default="cuda")
    add_dataset_arguments(app)
    return ap


def main(argv=None):
    args = build_parser().parse_args(argv)
    try:
        return fit_main(args) if args.command == "fit" else apply_main(args)
    except ValueError as e:
        raise SystemExit(str(e))


if __name__ == "__main__":
    main()
