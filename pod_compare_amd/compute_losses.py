"""Validation loss of a checkpoint: the reference's training objective (PR:129-130, PR:168-333) over a labelled COCO-format data set.

    python -m pod_compare_amd.compute_losses --coco-json <gt.json> --image-root <dir> --data-dir <checkpoints root> \
        --config-file <model.yaml> [--iteration N] [--train-mode]

Per image: the loader, the model construction and the category maps are apply_net's (imported, unchanged); the ground-truth boxes are
XYWH -> XYXY, scaled by the loader's resize factors, `iscrowd` boxes dropped, dataset category ids mapped to the model's contiguous ones
(annotations of a category the model does not have are dropped); the forward runs with dropout off (--train-mode: on, as the
reference's training forward); the anchors are labelled and the losses evaluated on the GPU (K21; K27 for the covariance term of
--bbox-cov-loss energy_loss / second_moment_matching; K28 for every name with --bbox-cov-type full) with the normaliser
max(1, positives of the image) and the annealing weight of --iteration (default SOLVER.STEPS[1]: annealing complete).  An image
without annotations counts as all-background.  Prints and returns the data-set means of loss_cls, loss_box_reg and positives per image.
"""
import argparse
import json
import os
from typing import Dict, List

import torch

from . import losses
from .apply_net import CocoImages, Prefetched, add_dataset_arguments, evaluation_category_map


def image_ground_truth(annotations: List[dict], cat_map: Dict[int, int], scale_x: float, scale_y: float):
    """COCO annotations of one image -> ((G, 4) XYXY fp32 boxes in network-input pixels, (G,) int64 contiguous classes)."""
    boxes, classes = [], []
    for a in annotations:
        if a.get("iscrowd", 0) or a["category_id"] not in cat_map:
            continue
        x, y, w, h = (float(v) for v in a["bbox"])
        boxes.append([x * scale_x, y * scale_y, (x + w) * scale_x, (y + h) * scale_y])
        classes.append(cat_map[a["category_id"]])
    return torch.tensor(boxes, dtype=torch.float32).reshape(-1, 4), torch.tensor(classes, dtype=torch.int64)


def covariance_overrides(cfg, args):
    """--bbox-cov-loss / --bbox-cov-type / --bbox-cov-samples set their BBOX_COV_LOSS keys (compute_losses and train_head alike); returns
    that node of the config."""
    cov = cfg.MODEL.PROBABILISTIC_MODELING.BBOX_COV_LOSS
    if args.bbox_cov_loss is not None:
        cov.NAME = args.bbox_cov_loss
    if args.bbox_cov_type is not None:
        cov.COVARIANCE_TYPE = args.bbox_cov_type
    if args.bbox_cov_samples > 0:
        cov.NUM_SAMPLES = args.bbox_cov_samples
    return cov


def arg_parser():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    here = os.path.dirname(os.path.abspath(__file__))
    ap.add_argument("--config-file", default=os.path.join(here, "configs/BDD-Detection/retinanet/retinanet_R_50_FPN_1x_reg_cls_var_dropout.yaml"))
    ap.add_argument("--inference-config", default="", help="optional; only merged into the config (the losses read none of its keys)")
    ap.add_argument("--coco-json", required=True, help="COCO-format ground truth: `images` and `annotations`")
    ap.add_argument("--image-root", required=True, help="directory of the files named in --coco-json")
    add_dataset_arguments(ap)
    ap.add_argument("--data-dir", default="", help="the reference's core.data_dir(): the checkpoint of OUTPUT_DIR under it is loaded (as apply_net)")
    ap.add_argument("--weights", default=None, help="overrides MODEL.WEIGHTS")
    ap.add_argument("--random-init", action="store_true", help="clear MODEL.WEIGHTS / OUTPUT_DIR and keep the seeded random initialisation")
    ap.add_argument("--random-seed", type=int, default=0)
    ap.add_argument("--iteration", type=int, default=-1, help="the training iteration the annealing weight is taken at (PR:320-321); default SOLVER.STEPS[1]")
    ap.add_argument("--bbox-cov-loss", default=None, choices=losses.BBOX_COV_LOSSES,
                    help="overrides MODEL.PROBABILISTIC_MODELING.BBOX_COV_LOSS.NAME: the covariance term of loss_box_reg -- energy_loss on any "
                         "checkpoint with the covariance head is its validation energy score, whatever it was trained under")
    ap.add_argument("--bbox-cov-type", default=None, choices=("diagonal", "full"),
                    help="overrides BBOX_COV_LOSS.COVARIANCE_TYPE: the head the checkpoint is loaded into (`full`: ten covariance channels, K28)")
    ap.add_argument("--bbox-cov-samples", type=int, default=0, help="overrides BBOX_COV_LOSS.NUM_SAMPLES, the energy loss's samples per positive anchor")
    ap.add_argument("--train-mode", action="store_true", help="dropout active in the head subnets, as in the reference's training forward")
    ap.add_argument("--min-size-test", type=int, default=0, help="overrides INPUT.MIN_SIZE_TEST")
    ap.add_argument("--max-size-test", type=int, default=0, help="overrides INPUT.MAX_SIZE_TEST")
    ap.add_argument("--loader-workers", type=int, default=-1, help="host threads of the loader; -1 = the config's value")
    ap.add_argument("--device", default="cuda:0")
    return ap


def main(argv=None):
    from .config import setup_config
    from .probabilistic_inference import build_model
    args = arg_parser().parse_args(argv)
    cfg = setup_config(args.config_file, args.inference_config, args.random_seed, data_dir=args.data_dir, is_testing=bool(args.data_dir))
    if args.weights is not None:
        cfg.MODEL.WEIGHTS = args.weights
    if args.random_init:
        cfg.MODEL.WEIGHTS, cfg.OUTPUT_DIR = "", ""
    if args.min_size_test > 0:
        cfg.INPUT.MIN_SIZE_TEST = args.min_size_test
    if args.max_size_test > 0:
        cfg.INPUT.MAX_SIZE_TEST = args.max_size_test
    cfg.MODEL.DEVICE = args.device
    cov = covariance_overrides(cfg, args)
    dev = torch.device(args.device)
    torch.cuda.set_device(dev)
    torch.manual_seed(args.random_seed)
    with open(args.coco_json, "r") as f:
        gt = json.load(f)
    if "annotations" not in gt:
        raise SystemExit("--coco-json needs `annotations`: the losses are evaluated against ground truth")
    by_image: Dict[object, List[dict]] = {}
    for a in gt["annotations"]:
        by_image.setdefault(a["image_id"], []).append(a)
    cat_map = evaluation_category_map(args.train_dataset, args.test_dataset)
    dataset = CocoImages(args.coco_json, args.image_root, cfg.INPUT.MIN_SIZE_TEST, cfg.INPUT.MAX_SIZE_TEST)
    model = build_model(cfg)
    K = cfg.MODEL.RETINANET.NUM_CLASSES
    anneal = int(cfg.SOLVER.STEPS[1])
    crit = losses.ProbabilisticLosses(num_classes=K, cls_var_num_samples=cfg.MODEL.PROBABILISTIC_MODELING.CLS_VAR_LOSS.NUM_SAMPLES,
                                      smooth_l1_beta=float(cfg.MODEL.RETINANET.get("SMOOTH_L1_LOSS_BETA", 0.0)),
                                      box_reg_weights=tuple(cfg.MODEL.RETINANET.BBOX_REG_WEIGHTS), annealing_step=anneal, seed=args.random_seed,
                                      bbox_cov_loss=cov.NAME, bbox_cov_num_samples=int(cov.NUM_SAMPLES))
    crit.current_step = anneal if args.iteration < 0 else args.iteration
    workers = args.loader_workers if args.loader_workers >= 0 else int(cfg.DATALOADER.NUM_WORKERS)
    total = torch.zeros(3, dtype=torch.float64, device=dev)          # loss_cls, loss_box_reg, positives: summed on the device
    n = 0
    with torch.no_grad():
        for i, d in Prefetched(dataset, range(len(dataset)), workers=workers):
            image = d["image"].to(dev, non_blocking=True)
            sy, sx = image.shape[1] / float(d["height"]), image.shape[2] / float(d["width"])
            boxes, classes = image_ground_truth(by_image.get(d["image_id"], []), cat_map, sx, sy)
            out = model(image, mc_dropout=bool(args.train_mode))
            labels, matched, num_pos = losses.label_anchors(out.anchors, [boxes], [classes], K)
            res = crit(out, labels, matched, boxes.to(dev), normalizer=num_pos[0].clamp(min=1))
            total += torch.stack((res["loss_cls"].double(), res["loss_box_reg"].double(), num_pos[0].double()))
            n += 1
    mean = (total / max(n, 1)).cpu().tolist()
    result = {"images": n, "loss_cls": mean[0], "loss_box_reg": mean[1], "positives_per_image": mean[2], "iteration": int(crit.current_step),
              "annealing_weight": losses.annealing_weight(crit.current_step, anneal), "train_mode": bool(args.train_mode),
              "bbox_cov_loss": str(cov.NAME), "bbox_cov_type": str(cov.COVARIANCE_TYPE)}
    print("%d images: loss_cls %.6f  loss_box_reg %.6f  positives per image %.2f  (iteration %d, covariance-loss weight %.4f%s)" % (
        n, result["loss_cls"], result["loss_box_reg"], result["positives_per_image"], result["iteration"], result["annealing_weight"],
        ", dropout on" if args.train_mode else ""))
    return result


if __name__ == "__main__":
    main()
