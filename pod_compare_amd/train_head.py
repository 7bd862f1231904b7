"""Fine-tunes the HEAD of a ProbabilisticRetinaNet -- with --train-fpn the FPN with it, with --train-backbone res3 - res5 too -- on the GPU.

    python -m pod_compare_amd.train_head --coco-json <gt.json> --image-root <dir> --data-dir <checkpoints root> \
        --config-file <model.yaml> [--weights <checkpoint>] [--max-iter N] [--log-period N] [--train-fpn | --train-backbone]

The head's part of train_net.py's loop: per step SOLVER.IMS_PER_BATCH frames of ONE resized shape (the sampler batches frames of equal
shape together; a shape's frames wait until a batch of them is complete), the frozen backbone + FPN per image under no_grad through the
existing forward, head.forward_train on the stacked features (pod_compare_amd/head_train.py), model.losses (K21; `current_step`
advanced every iteration as PR:146 does), backward() through the head's HIP backward (K22), torch.optim.SGD (momentum, weight decay)
under detectron2's WarmupMultiStepLR; the solver settings are SOLVER.*.  Checkpoints carry detectron2's names
(checkpoint.to_detectron2_state_dict) and go to OUTPUT_DIR with a `last_checkpoint` file, every SOLVER.CHECKPOINT_PERIOD iterations and
at the end: `apply_net --data-dir` loads them.  A checkpoint without variance predictors (retinanet_R_50_FPN_1x) under a config that has
them fine-tunes into one that does: the predictors the file lacks start from their seeded initialisation.

--train-fpn: the FPN's eight convolutions join the parameters.  The backbone still runs per image under no_grad, up to c3 - c5; the FPN
then runs with a backward pass of its own (pod_compare_amd/fpn_train.py: K22 for its output convolutions, K23 for the laterals, p6 / p7
and the top-down path), fed by the feature gradient the head's backward hands down, and a checkpoint carries the FPN that moved.

--train-backbone (implies --train-fpn): every parameter detectron2 trains at MODEL.BACKBONE.FREEZE_AT = 2 moves.  The stem and res2 run
per image under no_grad (resnet_train.res2_maps); res3 - res5 run with a backward pass of their own (pod_compare_amd/resnet_train.py: K24
for the 1x1 weight gradients and the stride-2 scatter, K22 for the 3x3 ones), fed by the gradient the FPN's backward hands below its
laterals and p6.  The device model computes with FrozenBN folded, W' = W s; the optimiser holds the unfolded W (W.grad = s dW'), so
momentum and weight decay act on what the reference's act on, and conv.weight is refolded from W after every step.  A checkpoint carries
W.  Only FREEZE_AT = 2 is supported.

Still NOT the reference's full trainer: no random flip (the frames are the loader's, resized only), no optimiser state in checkpoints
(a resumed run restarts momentum), one GPU.  The loss line is the only host read-back, on log steps only.
"""
import argparse
import bisect
import json
import os
from typing import Dict, List, Sequence

import torch

from . import checkpoint, losses
from .apply_net import CocoImages, Prefetched, add_dataset_arguments, evaluation_category_map
from .compute_losses import image_ground_truth
from .anchors import padded_size as _padded_size
from .config import setup_config
from .fpn_train import backbone_maps, fpn_convs, fpn_forward_train
from .head_train import head_convs
from .resnet_train import FoldedMasters, res2_maps, resnet_forward_train, trainable_convs, unfolded_pairs
from .probabilistic_inference import build_model


def warmup_multistep_lr(iteration: int, base_lr: float, steps: Sequence[int], gamma: float, warmup_iters: int, warmup_factor: float) -> float:
    """detectron2's WarmupMultiStepLR (linear warm-up): base_lr * w(it) * gamma ** (milestones <= it), w = warmup_factor (1 - a) + a with
    a = it / warmup_iters below warmup_iters, 1 from there on."""
    w = 1.0
    if iteration < warmup_iters:
        a = iteration / float(warmup_iters)
        w = warmup_factor * (1.0 - a) + a
    return base_lr * w * gamma ** bisect.bisect_right(list(steps), iteration)


class HeadTrainer:
    """The step function of train_head: optimiser, schedule and the iteration count around model.head.forward_train + model.losses."""

    def __init__(self, model, base_lr: float = 0.001, momentum: float = 0.9, weight_decay: float = 1e-4, steps: Sequence[int] = (60000, 80000),
                 gamma: float = 0.1, warmup_iters: int = 1000, warmup_factor: float = 1e-3, iteration: int = 0, train_fpn: bool = False,
                 train_backbone: bool = False, shadow=None):
        """train_backbone: res3 - res5 train too (and the FPN: it lies between them and the head); `shadow`, the same model unfolded, gives
        the master weights and FrozenBN scales (resnet_train.FoldedMasters)."""
        self.model, self.train_backbone = model, bool(train_backbone)
        self.train_fpn = bool(train_fpn) or self.train_backbone
        self.params = [p for c in head_convs(model.head) for p in (c.weight, c.bias)]
        if self.train_fpn:
            self.params += [p for c in fpn_convs(model.fpn) for p in (c.weight, c.bias)]
        for p in model.parameters():
            p.requires_grad_(False)               # what is frozen (the backbone; the FPN unless train_fpn) has no backward pass here
        for p in self.params:
            p.requires_grad_(True)
        self.masters = None
        if self.train_backbone:
            if shadow is None:
                raise ValueError("train_backbone needs `shadow`, the unfolded model: the optimiser holds its conv weights, not the folded ones")
            self.masters = FoldedMasters(trainable_convs(model.bottom_up), unfolded_pairs(shadow.bottom_up))
            self.params += self.masters.params
        self.schedule = dict(base_lr=float(base_lr), steps=tuple(int(s) for s in steps), gamma=float(gamma), warmup_iters=int(warmup_iters),
                             warmup_factor=float(warmup_factor))
        self.opt = torch.optim.SGD(self.params, lr=float(base_lr), momentum=float(momentum), weight_decay=float(weight_decay))
        self.iteration = int(iteration)

    def features(self, images: Sequence[torch.Tensor]):
        """The frozen backbone + FPN per image -> (per-level (B, 256, H, W) features, padded (h, w)).  train_fpn: only the backbone is
        frozen; the FPN runs on the batch's c3 - c5 with grad (fpn_train.fpn_forward_train)."""
        per_image, padded = [], None
        if self.train_backbone:
            # the stem and res2 frozen, per image; res3 - res5 and the FPN on the batch with grad
            res2 = [res2_maps(self.model, im) for im in images]
            padded = _padded_size(int(images[0].shape[-2]), int(images[0].shape[-1]))
            return fpn_forward_train(self.model.fpn, resnet_forward_train(self.model.bottom_up, res2)), padded
        if self.train_fpn:
            for im in images:
                maps, pad = backbone_maps(self.model, im)
                if padded is not None and tuple(pad) != tuple(padded):
                    raise ValueError("a batch holds frames of one padded size, got {} and {}".format(padded, pad))
                padded = tuple(pad)
                per_image.append(maps)
            return fpn_forward_train(self.model.fpn, per_image), padded
        with torch.no_grad():
            for im in images:
                feats, pad = self.model._trunk_eager(im)
                if padded is not None and tuple(pad) != tuple(padded):
                    raise ValueError("a batch holds frames of one padded size, got {} and {}".format(padded, pad))
                padded = tuple(pad)
                per_image.append(feats)
            stacked = [torch.cat([f[l] for f in per_image]).contiguous() for l in range(len(per_image[0]))]
        return stacked, padded

    def step(self, feats, padded, image_hw, gt_boxes, gt_classes, eps=None, normalizer=None) -> Dict[str, torch.Tensor]:
        """One iteration on the stacked features of a batch; returns the losses (device scalars)."""
        lr = warmup_multistep_lr(self.iteration, **self.schedule)
        for g in self.opt.param_groups:
            g["lr"] = lr
        out = self.model.head.forward_train(feats, self.model.anchors_for(tuple(padded)), image_hw)
        res = self.model.losses(out, gt_boxes, gt_classes, eps=eps, normalizer=normalizer)
        self.opt.zero_grad(set_to_none=True)
        (res["loss_cls"] + res["loss_box_reg"]).backward()
        if self.masters is not None:
            self.masters.collect_grads()          # W.grad = s dW': the optimiser steps the unfolded weights
        self.opt.step()                           # bumps the weights' versions: the filters and HIP graphs derived from them are rebuilt
        if self.masters is not None:
            self.masters.refold()                 # conv.weight = W s, in place
        self.model.loss_state.current_step += 1   # PR:146
        self.iteration += 1
        return res


def save_checkpoint(model, shadow, out_dir: str, name: str, iteration: int, train_fpn: bool = False, train_backbone: bool = False, masters=None) -> str:
    """`shadow`: the same model unfolded (conv + FrozenBN pairs) on the CPU -- the form detectron2's names describe; it receives the
    trained head (train_fpn: and the trained FPN, which has no norm to unfold; train_backbone: and the master weights of res3 - res5,
    `masters` = the trainer's FoldedMasters) and is written as <out_dir>/<name>.pth, named in <out_dir>/last_checkpoint."""
    os.makedirs(out_dir, exist_ok=True)
    pairs = list(zip(head_convs(shadow.head), head_convs(model.head)))
    if train_fpn or train_backbone:
        pairs += list(zip(fpn_convs(shadow.fpn), fpn_convs(model.fpn)))
    if train_backbone:
        if masters is None:
            raise ValueError("save_checkpoint(train_backbone=True) needs the trainer's master weights (HeadTrainer.masters)")
        masters.copy_to(unfolded_pairs(shadow.bottom_up))
    with torch.no_grad():
        for dst, src in pairs:
            dst.weight.copy_(src.weight.detach().cpu())
            dst.bias.copy_(src.bias.detach().cpu())
    path = os.path.join(out_dir, name + ".pth")
    torch.save({"model": checkpoint.to_detectron2_state_dict(shadow, with_dropout_entries=model.use_dropout), "iteration": int(iteration)}, path)
    with open(os.path.join(out_dir, "last_checkpoint"), "w") as f:
        f.write(name + ".pth")
    return path


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0],
                                 epilog="A step takes SOLVER.IMS_PER_BATCH frames of ONE resized shape: the sampler batches frames of equal shape "
                                        "together, in data-set order; frames of a shape wait until a batch of them is complete.  Only the head "
                                        "trains, and with --train-fpn the FPN; the ResNet stays frozen unless --train-backbone is given.")
    here = os.path.dirname(os.path.abspath(__file__))
    ap.add_argument("--config-file", default=os.path.join(here, "configs/BDD-Detection/retinanet/retinanet_R_50_FPN_1x_reg_cls_var_dropout.yaml"))
    ap.add_argument("--coco-json", required=True, help="COCO-format ground truth: `images` and `annotations`")
    ap.add_argument("--image-root", required=True, help="directory of the files named in --coco-json")
    add_dataset_arguments(ap)
    ap.add_argument("--data-dir", default="", help="the reference's core.data_dir(): checkpoints go to OUTPUT_DIR under it; its last_checkpoint, if any, is resumed from")
    ap.add_argument("--output-dir", default="", help="overrides OUTPUT_DIR")
    ap.add_argument("--weights", default=None, help="overrides MODEL.WEIGHTS (the checkpoint to fine-tune)")
    ap.add_argument("--random-init", action="store_true", help="load nothing: keep the seeded random initialisation")
    ap.add_argument("--random-seed", type=int, default=0)
    ap.add_argument("--max-iter", type=int, default=-1, help="overrides SOLVER.MAX_ITER")
    ap.add_argument("--log-period", type=int, default=20, help="a loss line every this many iterations (the only host read-back); 0: none")
    ap.add_argument("--min-size-test", type=int, default=0, help="overrides INPUT.MIN_SIZE_TEST")
    ap.add_argument("--max-size-test", type=int, default=0, help="overrides INPUT.MAX_SIZE_TEST")
    ap.add_argument("--loader-workers", type=int, default=-1, help="host threads of the loader; -1 = the config's value")
    ap.add_argument("--train-fpn", action="store_true", help="train the FPN's eight convolutions together with the head (the ResNet stays frozen)")
    ap.add_argument("--train-backbone", action="store_true", help="train res3 - res5 of the ResNet too, as detectron2 does at MODEL.BACKBONE.FREEZE_AT = 2 "
                                                                  "(implies --train-fpn; the stem and res2 stay frozen)")
    ap.add_argument("--device", default="cuda:0")
    args = ap.parse_args(argv)
    cfg = setup_config(args.config_file, "", args.random_seed, data_dir=args.data_dir)
    if args.output_dir:
        cfg.OUTPUT_DIR = args.output_dir
    if args.weights is not None:
        cfg.MODEL.WEIGHTS = args.weights
    if args.min_size_test > 0:
        cfg.INPUT.MIN_SIZE_TEST = args.min_size_test
    if args.max_size_test > 0:
        cfg.INPUT.MAX_SIZE_TEST = args.max_size_test
    cfg.MODEL.DEVICE = args.device
    freeze_at = cfg.MODEL.BACKBONE.get("FREEZE_AT", 2)
    if int(freeze_at) != 2:
        raise SystemExit("MODEL.BACKBONE.FREEZE_AT = {} is not supported: the stem and res2 are frozen and res3 - res5 train (detectron2's "
                         "default, FREEZE_AT = 2), or with neither --train-backbone nor --train-fpn only the head does".format(freeze_at))
    train_fpn = args.train_fpn or args.train_backbone
    dev = torch.device(args.device)
    torch.cuda.set_device(dev)
    with open(args.coco_json, "r") as f:
        gt = json.load(f)
    if "annotations" not in gt:
        raise SystemExit("--coco-json needs `annotations`: the head is trained against ground truth")
    by_image: Dict[object, List[dict]] = {}
    for a in gt["annotations"]:
        by_image.setdefault(a["image_id"], []).append(a)
    cat_map = evaluation_category_map(args.train_dataset, args.test_dataset)
    dataset = CocoImages(args.coco_json, args.image_root, cfg.INPUT.MIN_SIZE_TEST, cfg.INPUT.MAX_SIZE_TEST)
    # the model twice from one seed: on the device with FrozenBN folded (what runs), and unfolded on the CPU (what a checkpoint describes)
    load = not args.random_init
    torch.manual_seed(args.random_seed)
    model = build_model(cfg, load_weights=load)
    cpu_cfg = cfg.clone()
    cpu_cfg.MODEL.DEVICE = "cpu"
    torch.manual_seed(args.random_seed)
    shadow = build_model(cpu_cfg, load_weights=load, fold=False)
    torch.manual_seed(args.random_seed)
    s, K = cfg.SOLVER, cfg.MODEL.RETINANET.NUM_CLASSES
    model.loss_state = losses.ProbabilisticLosses(num_classes=K, cls_var_num_samples=cfg.MODEL.PROBABILISTIC_MODELING.CLS_VAR_LOSS.NUM_SAMPLES,
                                                  smooth_l1_beta=float(cfg.MODEL.RETINANET.get("SMOOTH_L1_LOSS_BETA", 0.0)),
                                                  box_reg_weights=tuple(cfg.MODEL.RETINANET.BBOX_REG_WEIGHTS), annealing_step=int(s.STEPS[1]),
                                                  seed=args.random_seed)
    trainer = HeadTrainer(model, base_lr=s.BASE_LR, momentum=s.MOMENTUM, weight_decay=s.WEIGHT_DECAY, steps=s.STEPS, gamma=s.GAMMA,
                          warmup_iters=s.WARMUP_ITERS, warmup_factor=s.WARMUP_FACTOR, train_fpn=train_fpn, train_backbone=args.train_backbone,
                          shadow=shadow if args.train_backbone else None)
    saved = dict(train_fpn=train_fpn, train_backbone=args.train_backbone, masters=trainer.masters)
    max_iter = args.max_iter if args.max_iter >= 0 else int(s.MAX_ITER)
    batch, period = max(1, int(s.IMS_PER_BATCH)), int(s.CHECKPOINT_PERIOD)
    workers = args.loader_workers if args.loader_workers >= 0 else int(cfg.DATALOADER.NUM_WORKERS)
    buckets: Dict[tuple, list] = {}
    written, last_line, stalled = [], None, 0
    while trainer.iteration < max_iter:
        progressed = False
        for _, d in Prefetched(dataset, range(len(dataset)), workers=workers):
            image = d["image"].to(dev, non_blocking=True)
            sy, sx = image.shape[1] / float(d["height"]), image.shape[2] / float(d["width"])
            boxes, classes = image_ground_truth(by_image.get(d["image_id"], []), cat_map, sx, sy)
            bucket = buckets.setdefault(tuple(image.shape), [])
            bucket.append((image, boxes, classes))
            if len(bucket) < batch:
                continue
            images, gb, gc = zip(*bucket)
            bucket.clear()
            feats, padded = trainer.features(images)
            res = trainer.step(feats, padded, tuple(images[0].shape[-2:]), list(gb), list(gc))
            progressed = True
            it = trainer.iteration
            if args.log_period > 0 and (it % args.log_period == 0 or it == max_iter):
                last_line = "iter %d  loss_cls %.6f  loss_box_reg %.6f  lr %.6g" % (it, float(res["loss_cls"]), float(res["loss_box_reg"]),
                                                                                  trainer.opt.param_groups[0]["lr"])
                print(last_line, flush=True)
            if period > 0 and it % period == 0 and it < max_iter:
                written.append(save_checkpoint(model, shadow, cfg.OUTPUT_DIR, "model_%07d" % (it - 1), it, **saved))
            if it >= max_iter:
                break
        stalled = 0 if progressed else stalled + 1      # (an incomplete batch carries over into the next pass over the data set)
        if stalled >= batch:
            raise SystemExit("no batch of {} frames of one resized shape can be formed from {} frames".format(batch, len(dataset)))
    written.append(save_checkpoint(model, shadow, cfg.OUTPUT_DIR, "model_final", trainer.iteration, **saved))
    what = ", the FPN and res3 - res5" if args.train_backbone else " and the FPN" if train_fpn else ""
    print("trained the head%s for %d iterations; wrote %s" % (what, trainer.iteration, written[-1]))
    return {"iterations": trainer.iteration, "checkpoints": written, "output_dir": cfg.OUTPUT_DIR, "model": model, "last_line": last_line}


if __name__ == "__main__":
    main()
