"""Evaluation while training, as train_net.py runs it: the test loader and the evaluator of the reference's Trainer
(/root/reference/src/train_net.py:29-76: build_test_loader, build_evaluator -> COCOEvaluator, `Trainer.test`, `verify_results`).

    evaluate_model(model, cfg, coco_json, image_root, output_dir)  ->  {"bbox": {"AP", "AP50", "AP75", "APs", "APm", "APl", "AP-<class>" ...}}

The test loader is build_detection_test_loader's behaviour: every image of the json in file order, ResizeShortestEdge(INPUT.MIN_SIZE_TEST,
MAX_SIZE_TEST), no flip, read ahead on DATALOADER.NUM_WORKERS threads (apply_net.CocoImages / Prefetched).  The model is the TRAINER'S OWN
object in eval mode -- dropout is the identity, the folded filters the trainer refolds after a step are the ones read, no second copy of
the weights and no checkpoint round trip.  In eval mode the reference model runs detectron2's RetinaNet.inference + detector_postprocess
(probabilistic_retinanet.py:156-166), not the probabilistic post-processing: every image goes through K32
(pod_compare_amd/retinanet_inference.py).  The results go to <output_dir>/inference/coco_instances_results.json as COCOEvaluator writes
them (image_id, category_id through the reverse of the contiguous-id map, bbox XYWH, score), bbox AP comes from the K17 kernels
(coco_eval.evaluate_accumulate), in COCOEvaluator's units: x 100, -1 where COCOeval has nothing to average.

Evaluation reads the model and writes nothing the trainer's determinism rests on: not the loss state's Philox draw counters, the flip and
plan generators, the sampler position or the momentum buffers; training mode is restored afterwards.

Data-parallel: rank r evaluates images r, r + world, ... (apply_net.shard_indices), the records are gathered to every rank
(data_parallel.gather_objects), rank 0 writes and scores, the other ranks return {} as detectron2's inference_on_dataset does.  A frame's
detections are a function of the frame alone, so the file's bytes do not depend on the world size.
"""
import json
import math
import os
from typing import Callable, Dict, List, Optional, Sequence

import numpy as np
import torch

from .apply_net import THING_CLASSES, CocoImages, Prefetched, _family, evaluation_category_map, shard_indices
from .compute_average_precision import coco_params, load_annotations, summarize

METRICS = ("AP", "AP50", "AP75", "APs", "APm", "APl")          # COCOEvaluator._derive_coco_results, iou_type "bbox"


def results_path(output_dir: str) -> str:
    """COCOEvaluator's file: DefaultTrainer hands it OUTPUT_DIR/inference."""
    return os.path.join(output_dir, "inference", "coco_instances_results.json")


def instances_to_records(image_id, boxes: torch.Tensor, scores: torch.Tensor, classes: torch.Tensor, reverse_map: Dict[int, int]) -> List[dict]:
    """detectron2's instances_to_coco_json for boxes: XYXY -> XYWH (w = x2 - x1, h = y2 - y1, in fp32), Python floats, the category id of
    the test data set.  A class the test set does not annotate (a BDD model on KITTI) has no id there and is dropped."""
    b = boxes.detach().to("cpu", torch.float32).clone()
    if b.numel():
        b[:, 2] -= b[:, 0]
        b[:, 3] -= b[:, 1]
    out = []
    for box, s, c in zip(b.tolist(), scores.detach().cpu().tolist(), classes.detach().cpu().tolist()):
        if int(c) in reverse_map:
            out.append({"image_id": image_id, "category_id": reverse_map[int(c)], "bbox": box, "score": s})
    return out


def derive_coco_results(stats: Optional[Sequence[float]], precision: Optional[np.ndarray], class_names: Sequence[str]) -> Dict[str, float]:
    """COCOEvaluator._derive_coco_results for bbox: the first six of COCOeval.stats x 100 and, per category, the mean over IoU thresholds
    and recall thresholds of precision[:, :, k, area "all", maxDets 100] x 100; -1 where there is nothing to average (stats is None: no
    predictions at all)."""
    if stats is None:
        return {m: -1.0 for m in METRICS}
    res = {m: float(stats[i] * 100) if stats[i] >= 0 else -1.0 for i, m in enumerate(METRICS)}
    if precision is not None and len(class_names) > 0:
        assert precision.shape[2] == len(class_names), (precision.shape, len(class_names))
        for k, name in enumerate(class_names):
            p = precision[:, :, k, 0, -1]
            p = p[p > -1]
            res["AP-" + name] = float(np.mean(p) * 100) if p.size else -1.0
    return res


def copypaste_lines(results: Dict[str, Dict[str, float]]) -> List[str]:
    """detectron2's print_csv_format: per task the metrics without a '-' in their name, values with four decimals."""
    lines = []
    for task, res in results.items():
        important = [(k, v) for k, v in res.items() if "-" not in k]
        lines.append("copypaste: Task: {}".format(task))
        lines.append("copypaste: " + ",".join(k for k, _ in important))
        lines.append("copypaste: " + ",".join("{0:.4f}".format(v) for _, v in important))
    return lines


def verify_results(cfg, results: Dict[str, Dict[str, float]], say: Callable = print) -> bool:
    """detectron2's verify_results: every (task, metric, expected, tolerance) of TEST.EXPECTED_RESULTS must be present, finite and within
    `tolerance` of `expected` (|actual - expected| <= tolerance passes).  No expectations: True.  A failure exits the process with status
    1, as detectron2's does."""
    expected = list(cfg.TEST.get("EXPECTED_RESULTS", []) or [])
    if not expected:
        return True
    ok = True
    for task, metric, value, tolerance in expected:
        actual = results.get(task, {}).get(metric, None)
        if actual is None or not math.isfinite(actual) or abs(actual - float(value)) > float(tolerance):
            ok = False
    if not ok:
        say("Result verification failed!")
        say("Expected Results: " + str(expected))
        say("Actual Results: " + json.dumps({t: dict(r) for t, r in results.items()}))
        raise SystemExit(1)
    say("Results verification passed.")
    return ok


def inference_params(cfg, num_anchors: int):
    from .retinanet_inference import InferenceParams
    r = cfg.MODEL.RETINANET
    return InferenceParams(num_classes=int(r.NUM_CLASSES), num_anchors=int(num_anchors), topk_candidates=int(r.TOPK_CANDIDATES_TEST),
                           score_thresh=float(r.SCORE_THRESH_TEST), nms_thresh=float(r.NMS_THRESH_TEST),
                           max_detections=int(cfg.TEST.DETECTIONS_PER_IMAGE), box_weights=tuple(float(v) for v in r.BBOX_REG_WEIGHTS))


def score_results(records: List[dict], coco_json: str, train_dataset: str, test_dataset: str, device="cuda", impl=None) -> Dict[str, float]:
    """COCOEvaluator._eval_predictions for bbox: COCOeval over every category of the test set (the json's `categories`; a json without the
    list: the test set's own ids) -> derive_coco_results.  impl: the seam of compute_average_precision (None: the K17 kernels)."""
    names = THING_CLASSES[_family(test_dataset)]
    with open(coco_json, "r") as f:
        gt = json.load(f)
    cat_ids = sorted(int(c["id"]) for c in gt["categories"]) if gt.get("categories") else list(range(1, len(names) + 1))
    by_id = {int(c["id"]): c["name"] for c in gt.get("categories", [])}
    class_names = [by_id.get(c, names[c - 1] if 1 <= c <= len(names) else str(c)) for c in cat_ids]
    if not records:
        return derive_coco_results(None, None, class_names)
    iou_thrs, rec_thrs, max_dets, area_rngs = coco_params()
    gts, dts, img_ids = load_annotations(records, gt)
    if impl is None:
        from .coco_eval import evaluate_accumulate
        precision, recall, _ = evaluate_accumulate(gts, dts, img_ids, cat_ids, iou_thrs, rec_thrs, max_dets, area_rngs, device=device)
    else:
        precision, recall, _ = impl(gts, dts, img_ids, cat_ids, iou_thrs, rec_thrs, max_dets, area_rngs)
    return derive_coco_results(summarize(precision, recall, iou_thrs, max_dets), precision, class_names)


def evaluate_model(model, cfg, coco_json: str, image_root: str, output_dir: str, train_dataset: str = "bdd_train", test_dataset: str = "bdd_val",
                   workers: Optional[int] = None, rank: int = 0, world: int = 1, group=None, say: Callable = print, on_image=None) -> dict:
    """`Trainer.test(cfg, model)` for one validation set.  Returns {"bbox": {...}} on rank 0 and {} on every other rank.
    on_image(index, entry, head outputs, detections): called per image after its detections are on the host (tests)."""
    from .retinanet_inference import RetinaNetInference
    dataset = CocoImages(coco_json, image_root, cfg.INPUT.MIN_SIZE_TEST, cfg.INPUT.MAX_SIZE_TEST)
    workers = int(cfg.DATALOADER.NUM_WORKERS) if workers is None else int(workers)
    reverse_map = {v: k for k, v in evaluation_category_map(train_dataset, test_dataset).items()}
    params = inference_params(cfg, model.num_anchors)
    dev = model.device
    paths: Dict[tuple, RetinaNetInference] = {}
    was_training = model.training
    model.eval()
    per_image = []                                    # (index, records)
    try:
        with torch.no_grad(), torch.cuda.device(dev):
            for i, d in Prefetched(dataset, shard_indices(len(dataset), rank, world), workers=workers):
                image = d["image"].to(dev, non_blocking=True)
                out = model(image, mc_dropout=False)                 # eval mode: one run, dropout the identity
                key = tuple(tuple(s) for s in out.shapes)
                path = paths.get(key)
                if path is None:
                    path = paths[key] = RetinaNetInference(out.shapes, out.anchors, params, device=dev)
                cls, delta = [t.contiguous() for t in out.cls], [t.contiguous() for t in out.delta]
                det = path.infer_image((cls, delta), tuple(image.shape[-2:]), (d["height"], d["width"]))
                boxes, scores, classes, _ = det.trimmed()            # the one read-back of an image
                per_image.append((i, instances_to_records(d["image_id"], boxes, scores, classes, reverse_map)))
                if on_image is not None:
                    on_image(i, d, out, (boxes, scores, classes))
    finally:
        model.train(was_training)
    if world > 1:
        from .data_parallel import gather_objects
        per_image = [e for part in gather_objects(per_image, world, group) for e in part]
    if rank != 0:
        return {}
    records = [r for _, recs in sorted(per_image, key=lambda e: e[0]) for r in recs]          # file order, whatever the world size
    path = results_path(output_dir)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        f.write(json.dumps(records))
        f.flush()
    results = {"bbox": score_results(records, coco_json, train_dataset, test_dataset, device=dev)}
    say("Evaluation results for bbox: " + ", ".join("{} {:.3f}".format(k, v) for k, v in results["bbox"].items() if "-" not in k), flush=True)
    for line in copypaste_lines(results):
        say(line, flush=True)
    return results


def ap_line(iteration: int, results: dict) -> str:
    """The line a training log carries behind the loss line of an evaluated iteration."""
    b = results.get("bbox", {})
    return "iter %d  bbox AP %.4f  AP50 %.4f  AP75 %.4f" % (iteration, b.get("AP", -1.0), b.get("AP50", -1.0), b.get("AP75", -1.0))
