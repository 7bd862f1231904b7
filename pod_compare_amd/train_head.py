"""Fine-tunes the HEAD of a ProbabilisticRetinaNet -- with --train-fpn the FPN with it, with --train-backbone res3 - res5 too -- on the GPU.

    python -m pod_compare_amd.train_head --coco-json <gt.json> --image-root <dir> --data-dir <checkpoints root> \
        --config-file <model.yaml> [--weights <checkpoint>] [--max-iter N] [--log-period N] [--train-fpn | --train-backbone]
        [--fused-step] [--guard-nonfinite] [--random-flip] [--resume] [--data-parallel [--backend nccl|gloo] [--share-gpu]]
        [--train-loader [--no-shuffle] [--batch-on-gpu]]
        [--val-coco-json <val.json> --val-image-root <dir> [--eval-only]]

The head's part of train_net.py's loop: per step SOLVER.IMS_PER_BATCH frames of ONE resized shape (the sampler batches frames of equal
shape together; a shape's frames wait until a batch of them is complete -- with --train-loader, below, frames of one aspect-ratio
group and any sizes), the frozen backbone + FPN per image under no_grad through the
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
W.  MODEL.BACKBONE.FREEZE_AT is honoured as detectron2 honours it: 2 (the default) is the above; 1 trains res2 too -- the stem and its
max-pool run under no_grad (resnet_train.pool_maps) and res2's three blocks join the chain --; 0 trains the stem as well, nothing runs
under no_grad: the stem and the pool get a backward pass (resnet_train.stem_forward_train, K30: the pool's backward with the stem's ReLU
gate per image, one 7x7 weight gradient over the batch's stacked frames).  3, 4 and 5 are refused, and so is a value other than 2
without --train-backbone.  A checkpoint's `trained` list names res2 and the stem when they moved, so --resume across freeze points is refused.

--fused-step: the optimiser's step is ONE launch of this project's own (K25, pod_compare_amd/sgd_step.py) in place of collect_grads + torch's
SGD + refold: the trainer owns the momentum buffers, the kernel scales a folded filter's gradient by s, steps the master and rewrites the
folded filter, and the written tensors' versions are bumped so that the derived filters are rebuilt.  Without the flag torch.optim.SGD steps.

The solver: beside BASE_LR, MOMENTUM, WEIGHT_DECAY, STEPS, GAMMA, WARMUP_ITERS and WARMUP_FACTOR, SOLVER.NESTEROV, BIAS_LR_FACTOR and
WEIGHT_DECAY_BIAS (the biases of the head's and the FPN's convolutions as a parameter group of their own), CLIP_GRADIENTS.* (`value` and
`norm` per parameter tensor, `full_model` over all of them), LR_SCHEDULER_NAME (WarmupMultiStepLR, WarmupCosineLR) and WARMUP_METHOD
(linear, constant) are honoured by both optimisers -- torch's with two parameter groups, nesterov and torch's clipping utilities, the
fused one with K29 (pod_sgd_step_solver) -- and a value this trainer does not run is refused by name before a model is built
(`solver_settings`).  A YAML that names none of them runs what ran before them, call for call.

--guard-nonfinite (implies --fused-step): detectron2's stop at the first non-finite loss, without a synchronisation per step.  The fused
step checks every tensor's gradient norm and the step's two losses on the device; a bad step, and every step after it, writes nothing,
and the next log line or checkpoint (`HeadTrainer.check_finite`) raises FloatingPointError naming the first bad iteration before
anything is written: the weights are those from before it.

--random-flip: detectron2's RandomFlip(horizontal), probability 0.5.  The draw is made in the main loop in data order from a generator
seeded with --random-seed; the frame is flipped on the device and its boxes follow HFlipTransform (`hflip_boxes`).

Every checkpoint also carries the trainer's state (`pod_trainer`: iteration, the loss state's step / draw count / normaliser, the momentum
buffers under detectron2's names, the sampler's position, the frames waiting in the shape buckets, the flip generator).  --resume
(detectron2's flag): OUTPUT_DIR/last_checkpoint's weights AND that state are restored, and the run continues where it stopped -- schedule,
annealing, momentum and data order.  A checkpoint without the state, or from a run that trained other parts, is refused.  Without --resume
the weights of last_checkpoint load as before and the run starts at iteration 0.

--data-parallel [--backend nccl|gloo] [--share-gpu] (implies --fused-step): this process is one rank of a data-parallel run, as detectron2's
launch starts them (RANK / WORLD_SIZE / LOCAL_RANK of torch.distributed.run; a process group that is already initialised is used as it
is).  Every rank walks the same index stream, flip draws and shape buckets, so the global batches are the one-rank run's; rank r takes
frames [r B / W, (r + 1) B / W) of each and decodes only those (the bucket key comes from the json's height / width).  Per step ONE
launch packs every gradient times 1 / W into a flat bucket (K26, pod_compare_amd/data_parallel.py), the two losses behind them, ONE
all-reduce sums it over the ranks and K25 steps from the bucket.  Each rank keeps its own loss state (its normaliser, its draws; seeds
--random-seed + rank); rank 0's trained tensors and momentum are broadcast once at the start; only rank 0 prints (the rank means of the
losses) and writes checkpoints, whose `pod_trainer` then carries `world` and `ranks`, every rank's loss state -- --resume continues at
the same world size only.  SOLVER.IMS_PER_BATCH must be a multiple of W.

--train-loader [--no-shuffle] [--batch-on-gpu]: the first line of train_net.py's loop, build_detection_train_loader(cfg), as a data plan
that is a pure function of the json, the config and --random-seed (pod_compare_amd/train_loader.py).  Frames without a usable annotation
are dropped (DATALOADER.FILTER_EMPTY_ANNOTATIONS); every pass is a fresh seeded permutation (TrainingSampler; --no-shuffle: file order);
per frame the short edge is drawn from INPUT.MIN_SIZE_TRAIN under MIN_SIZE_TRAIN_SAMPLING (`choice`, `range`), capped by MAX_SIZE_TRAIN,
then the flip under INPUT.RANDOM_FLIP (`horizontal`, `none`; --random-flip forces it on) -- the TEST keys are not read; batches are
grouped by aspect ratio only (DATALOADER.ASPECT_RATIO_GROUPING: w > h and the rest), so a batch holds frames of several sizes: each is run
against the batch's common padded size, anchors.padded_size of the largest height and width (ImageList.from_tensors; the stem reads
zero outside the frame after normalisation), its ground truth scaled and mirrored against its OWN size.  The frames a rank will need are
known ahead, so they are read on DATALOADER.NUM_WORKERS threads in plan order -- for a data-parallel rank too, which still takes its
slice of the one-rank run's global batches.  --batch-on-gpu: the threads only decode, and ONE launch (K31, pod_compare_amd/train_batch.py)
resizes, mirrors, flips to BGR and transposes the rank's frames; the bytes are the host path's.  The checkpoint's sampler state is then
the plan's (kind `train_loader`: the permutation generator at the start of the pass, the draw generator, the position, the waiting
entries with their draws); --resume across the two kinds of data order is refused.  Without the flag nothing of this is imported.

--val-coco-json / --val-image-root: the other two places train_net.py customises DefaultTrainer in, the test loader and the evaluator
(pod_compare_amd/train_eval.py).  The validation set -- not the training json -- is evaluated after every iteration `it` with
(it + 1) % TEST.EVAL_PERIOD == 0 (detectron2's EvalHook; 0, the default: never) and always after the last iteration: every image in file
order at INPUT.MIN_SIZE_TEST / MAX_SIZE_TEST, the trainer's own model object in eval mode (dropout the identity, the filters the step just
refolded), detectron2's RetinaNet.inference + detector_postprocess on the device (K32, pod_compare_amd/retinanet_inference.py: what the
reference model runs in eval mode, PR:156-166), OUTPUT_DIR/inference/coco_instances_results.json as COCOEvaluator writes it, bbox AP from
the K17 kernels, detectron2's `copypaste:` lines and, on a log step, an AP line behind the loss line.  After the last evaluation
TEST.EXPECTED_RESULTS is checked as detectron2's verify_results checks it.  Evaluation touches nothing a run's determinism rests on: the
checkpoints of a run with evaluation are those of the run without, to the bit.  TEST.EVAL_PERIOD > 0 without --val-coco-json is refused
before a model is built.  --eval-only: load MODEL.WEIGHTS (--weights), or OUTPUT_DIR/last_checkpoint with --resume, evaluate once, print
and return the results; no optimiser is built and --coco-json is not read.  Under --data-parallel every rank evaluates its share of the
images (apply_net.shard_indices), the records are gathered, rank 0 writes and scores; the file's bytes do not depend on the world size.

Still NOT the reference's full trainer: the all-reduce does not overlap the backward pass, and without --train-loader a data-parallel
rank reads its frames without read-ahead.  The loss line is the only host read-back, on log steps only (and a checkpoint's copies); under settings that
compute a gradient norm, or the guard, the solver's 32-byte status is read with it and before a checkpoint.
"""
import argparse
import bisect
import dataclasses
import json
import math
import os
from typing import Dict, List, Optional, Sequence

import torch

from . import checkpoint, losses
from .apply_net import CocoImages, Prefetched, add_dataset_arguments, evaluation_category_map
from .compute_losses import covariance_overrides, image_ground_truth
from .anchors import padded_size as _padded_size, resize_shortest_edge
from .config import setup_config
from .data_parallel import GradBucket, broadcast_tensors, gather_objects, rank_slice
from .fpn_train import backbone_maps, fpn_convs, fpn_forward_train
from .head_train import conv_params, head_convs
from .resnet_train import FREEZE_POINTS, FoldedMasters, pool_maps, res2_maps, resnet_forward_train, stem_forward_train, trainable_convs, unfolded_pairs
from .probabilistic_inference import build_model
from .sgd_step import LR_SCHEDULERS, WARMUP_METHODS, FusedSGD, SgdEntry, SolverSettings


def warmup_multistep_lr(iteration: int, base_lr: float, steps: Sequence[int], gamma: float, warmup_iters: int, warmup_factor: float) -> float:
    """detectron2's WarmupMultiStepLR (linear warm-up): base_lr * w(it) * gamma ** (milestones <= it), w = warmup_factor (1 - a) + a with
    a = it / warmup_iters below warmup_iters, 1 from there on."""
    w = 1.0
    if iteration < warmup_iters:
        a = iteration / float(warmup_iters)
        w = warmup_factor * (1.0 - a) + a
    return base_lr * w * gamma ** bisect.bisect_right(list(steps), iteration)


def warmup_factor_at(iteration: int, warmup_iters: int, warmup_factor: float, method: str = "linear") -> float:
    """detectron2's _get_warmup_factor_at_iter: 1 from warmup_iters on; below it `constant`: warmup_factor, `linear`: warmup_factor (1 - a) + a."""
    if iteration >= warmup_iters:
        return 1.0
    if method == "constant":
        return float(warmup_factor)
    if method != "linear":
        raise ValueError("unknown warm-up method {!r}".format(method))
    a = iteration / float(warmup_iters)
    return warmup_factor * (1.0 - a) + a


def warmup_cosine_lr(iteration: int, base_lr: float, max_iter: int, warmup_iters: int, warmup_factor: float, method: str = "linear") -> float:
    """detectron2's WarmupCosineLR: base_lr * w(it) * 0.5 (1 + cos(pi it / max_iter))."""
    return base_lr * warmup_factor_at(iteration, warmup_iters, warmup_factor, method) * 0.5 * (1.0 + math.cos(math.pi * iteration / max_iter))


def scheduled_lr(iteration: int, base_lr: float, steps: Sequence[int], gamma: float, warmup_iters: int, warmup_factor: float,
                 lr_scheduler_name: str = "WarmupMultiStepLR", warmup_method: str = "linear", max_iter: int = 0) -> float:
    """The learning rate of `iteration` for a group whose base rate is base_lr, in Python doubles as torch's LambdaLR forms it.  The default
    names give warmup_multistep_lr itself, to the bit."""
    if lr_scheduler_name == "WarmupCosineLR":
        return warmup_cosine_lr(iteration, base_lr, max(1, int(max_iter)), warmup_iters, warmup_factor, warmup_method)
    if lr_scheduler_name != "WarmupMultiStepLR":
        raise ValueError("unknown learning rate schedule {!r}".format(lr_scheduler_name))
    if warmup_method == "linear":
        return warmup_multistep_lr(iteration, base_lr, steps, gamma, warmup_iters, warmup_factor)
    return base_lr * warmup_factor_at(iteration, warmup_iters, warmup_factor, warmup_method) * gamma ** bisect.bisect_right(list(steps), iteration)


def solver_settings(cfg, guard_nonfinite: bool = False) -> SolverSettings:
    """SOLVER.* beyond what train_head always read, as SolverSettings; SystemExit naming the key for a value this trainer does not run.  A
    key that is absent has detectron2's default, which is what ran before the keys were read: clipping that is not ENABLED is "off", a
    WEIGHT_DECAY_BIAS equal to WEIGHT_DECAY is no group of its own.  WEIGHT_DECAY_NORM is accepted and has no effect (every norm is frozen)."""
    s = cfg.SOLVER
    clip = s.get("CLIP_GRADIENTS", None) or {}

    def number(key, value, positive=False):
        try:
            x = float(value)
        except (TypeError, ValueError):
            x = float("nan")
        if isinstance(value, bool) or not math.isfinite(x) or x < 0 or (positive and x == 0):
            raise SystemExit("SOLVER.{} = {!r} is not supported: a finite {} number".format(key, value, "positive" if positive else "non-negative"))
        return x

    def one_of(key, value, known):
        if value not in known:
            raise SystemExit("SOLVER.{} = {!r} is not supported: one of {}".format(key, value, ", ".join(known)))
        return value

    clip_type = one_of("CLIP_GRADIENTS.CLIP_TYPE", clip.get("CLIP_TYPE", "value"), ("value", "norm", "full_model"))
    clip_value = number("CLIP_GRADIENTS.CLIP_VALUE", clip.get("CLIP_VALUE", 1.0), positive=True)
    if float(clip.get("NORM_TYPE", 2.0)) != 2.0:
        raise SystemExit("SOLVER.CLIP_GRADIENTS.NORM_TYPE = {!r} is not supported: only the 2-norm is".format(clip.get("NORM_TYPE")))
    enabled = bool(clip.get("ENABLED", False))
    wd, wd_bias = float(s.WEIGHT_DECAY), s.get("WEIGHT_DECAY_BIAS", None)
    wd_bias = None if wd_bias is None else number("WEIGHT_DECAY_BIAS", wd_bias)
    nesterov = bool(s.get("NESTEROV", False))
    if nesterov and float(s.MOMENTUM) <= 0:
        raise SystemExit("SOLVER.NESTEROV needs SOLVER.MOMENTUM > 0, got {!r}".format(s.MOMENTUM))
    return SolverSettings(nesterov=nesterov, bias_lr_factor=number("BIAS_LR_FACTOR", s.get("BIAS_LR_FACTOR", 1.0)),
                          weight_decay_bias=None if wd_bias is None or wd_bias == wd else wd_bias,
                          clip_type=clip_type if enabled else "off", clip_value=clip_value if enabled else 1.0,
                          lr_scheduler_name=one_of("LR_SCHEDULER_NAME", s.get("LR_SCHEDULER_NAME", "WarmupMultiStepLR"), LR_SCHEDULERS),
                          warmup_method=one_of("WARMUP_METHOD", s.get("WARMUP_METHOD", "linear"), WARMUP_METHODS), guard_nonfinite=bool(guard_nonfinite))


def parameter_groups(names: Sequence[str], settings: SolverSettings) -> List[int]:
    """The group of each trained tensor by its detectron2 name: 1 for a parameter named `bias` (the head's and the FPN's convolutions have
    them; the master weights of res3 - res5 have none), 0 for a weight -- all 0 when the settings give the biases nothing of their own."""
    return [1 if settings.two_groups and n.rsplit(".", 1)[-1] == "bias" else 0 for n in names]


def hflip_boxes(boxes: torch.Tensor, width) -> torch.Tensor:
    """detectron2's HFlipTransform.apply_box on (N, 4) XYXY boxes of an image `width` pixels wide (the RESIZED width, the boxes' own
    scale): x1' = W - x2, x2' = W - x1, y unchanged -- x1' < x2' wherever x1 < x2."""
    out = boxes.clone()
    out[:, 0] = width - boxes[:, 2]
    out[:, 2] = width - boxes[:, 0]
    return out


def trained_parts(train_fpn: bool, train_backbone: bool, freeze_at: int = 2) -> List[str]:
    """What a run trains, as a checkpoint's `pod_trainer` names it (--resume compares the lists): at the default freeze point what it
    always was; "res2" and "stem" follow where MODEL.BACKBONE.FREEZE_AT lets them move."""
    parts = ["head"] + (["fpn"] if train_fpn or train_backbone else []) + (["backbone"] if train_backbone else [])
    if train_backbone:
        parts += (["res2"] if freeze_at < 2 else []) + (["stem"] if freeze_at < 1 else [])
    return parts


class HeadTrainer:
    """The step function of train_head: optimiser, schedule and the iteration count around model.head.forward_train + model.losses."""

    def __init__(self, model, base_lr: float = 0.001, momentum: float = 0.9, weight_decay: float = 1e-4, steps: Sequence[int] = (60000, 80000),
                 gamma: float = 0.1, warmup_iters: int = 1000, warmup_factor: float = 1e-3, iteration: int = 0, train_fpn: bool = False,
                 train_backbone: bool = False, shadow=None, fused_step: bool = False, data_parallel=None, solver: Optional[SolverSettings] = None,
                 guard_nonfinite: bool = False, max_iter: int = 0, freeze_at: int = 2):
        """train_backbone: res3 - res5 train too (and the FPN: it lies between them and the head); `shadow`, the same model unfolded, gives
        the master weights and FrozenBN scales (resnet_train.FoldedMasters).  freeze_at (with train_backbone): MODEL.BACKBONE.FREEZE_AT --
        2: the stem and res2 stay frozen; 1: res2 trains too; 0: and the stem.  fused_step: the optimiser's step is pod_sgd_step (K25) on
        momentum buffers the trainer owns (`self.fused`), not torch's SGD; `self.opt` is the torch.optim.SGD either way (unused when fused).
        data_parallel: (rank, world, process group or None = the default one) -- this trainer is one rank of `world`: its gradients go
        through a bucket (`self.bucket`, data_parallel.GradBucket: K26, one all-reduce) and the fused step reads the rank mean from it.
        Needs fused_step.  The loss state stays the rank's own, as under DistributedDataParallel.
        solver: the SolverSettings (solver_settings(cfg); None: the defaults, under which both optimisers are built and called as before
        the settings existed).  Torch's path honours them with two parameter groups, nesterov and torch's clipping utilities; the fused
        one with pod_sgd_step_solver (K29).  guard_nonfinite (needs fused_step): a step with a non-finite gradient or loss, and every
        step after it, writes nothing; check_finite() raises.  max_iter: WarmupCosineLR's horizon."""
        self.solver = solver if solver is not None else SolverSettings()
        if guard_nonfinite and not self.solver.guard_nonfinite:
            self.solver = dataclasses.replace(self.solver, guard_nonfinite=True)
        if self.solver.guard_nonfinite and not fused_step:
            raise ValueError("guard_nonfinite needs fused_step: the guard is the fused step's (pod_sgd_step_solver)")
        if data_parallel is not None and not fused_step:
            raise ValueError("data_parallel needs fused_step: the averaged gradients are stepped from the bucket by pod_sgd_step")
        self.model, self.train_backbone = model, bool(train_backbone)
        self.freeze_at = int(freeze_at)
        if self.freeze_at not in FREEZE_POINTS or (self.freeze_at != 2 and not self.train_backbone):
            raise ValueError("freeze_at = {}: 0, 1 or 2, and other than 2 only with train_backbone".format(freeze_at))
        self.train_fpn = bool(train_fpn) or self.train_backbone
        self.params = conv_params(head_convs(model.head))
        if self.train_fpn:
            self.params += conv_params(fpn_convs(model.fpn))
        for p in model.parameters():
            p.requires_grad_(False)               # what is frozen (the backbone; the FPN unless train_fpn) has no backward pass here
        for p in self.params:
            p.requires_grad_(True)
        self.masters = None
        if self.train_backbone:
            if shadow is None:
                raise ValueError("train_backbone needs `shadow`, the unfolded model: the optimiser holds its conv weights, not the folded ones")
            self.masters = FoldedMasters(trainable_convs(model.bottom_up, self.freeze_at), unfolded_pairs(shadow.bottom_up, self.freeze_at), self.freeze_at)
            self.params += self.masters.params
        self.schedule = dict(base_lr=float(base_lr), steps=tuple(int(s) for s in steps), gamma=float(gamma), warmup_iters=int(warmup_iters),
                             warmup_factor=float(warmup_factor))
        self.max_iter = int(max_iter)
        self.groups = parameter_groups(self.param_names(), self.solver) if self.solver.two_groups else [0] * len(self.params)
        if self.solver.plain_step:
            self.opt = torch.optim.SGD(self.params, lr=float(base_lr), momentum=float(momentum), weight_decay=float(weight_decay))
        else:                                     # detectron2's build_optimizer: the biases in a group of their own
            wd_bias = float(weight_decay) if self.solver.weight_decay_bias is None else float(self.solver.weight_decay_bias)
            by_group = [[p for p, g in zip(self.params, self.groups) if g == k] for k in (0, 1)]
            param_groups = [{"params": by_group[0]}]
            if by_group[1]:
                param_groups.append({"params": by_group[1], "lr": float(base_lr) * self.solver.bias_lr_factor, "weight_decay": wd_bias})
            self.opt = torch.optim.SGD(param_groups, lr=float(base_lr), momentum=float(momentum), weight_decay=float(weight_decay),
                                       nesterov=self.solver.nesterov)
        self._grad_norm = None                    # torch's path: the norm clip_grad_norm_ returned over the full model (a device scalar)
        self.iteration = int(iteration)
        self.momentum_mu = float(momentum)
        self.fused, self.bucket, self.rank, self.world = None, None, 0, 1
        if fused_step:
            n_plain = len(self.params) - (len(self.masters.params) if self.masters is not None else 0)
            entries = [SgdEntry(p) for p in self.params[:n_plain]]
            if self.masters is not None:
                entries += [SgdEntry(p, grad_of=c.weight, scale=s, folded=c.weight) for c, p, s in zip(self.masters.convs, self.masters.params, self.masters.scales)]
            if data_parallel is not None:
                self.rank, self.world, group = int(data_parallel[0]), int(data_parallel[1]), data_parallel[2]
                if not 0 <= self.rank < self.world:
                    raise ValueError("data_parallel: rank {} of world {}".format(self.rank, self.world))
                self.bucket = GradBucket(entries, self.world, group)
            self.fused = FusedSGD(entries, momentum=float(momentum), weight_decay=float(weight_decay), grads_from=self.bucket,
                                  solver=self.solver, groups=self.groups)
        self._lrs = self.lrs_at(self.iteration)
        self._lr = self._lrs[0]
        self._losses = None

    def lrs_at(self, iteration: int) -> List[float]:
        """The learning rate of `iteration` per parameter group: the schedule on each group's own base rate, as torch's LambdaLR forms it."""
        sch = dict(self.schedule, lr_scheduler_name=self.solver.lr_scheduler_name, warmup_method=self.solver.warmup_method, max_iter=self.max_iter)
        base = sch.pop("base_lr")
        return [scheduled_lr(iteration, b, **sch) for b in ([base, base * self.solver.bias_lr_factor] if self.solver.two_groups else [base])]

    @property
    def lr(self) -> float:
        """The learning rate of the last step taken (before the first: the one the first will take), whichever optimiser steps."""
        return self._lr

    def trained(self) -> List[str]:
        return trained_parts(self.train_fpn, self.train_backbone, self.freeze_at)

    def param_names(self) -> List[str]:
        """detectron2's name of the weight each of self.params is (a master weight: of the conv it is the unfolded filter of)."""
        local = {id(p): k for k, p in self.model.named_parameters()}
        to_d2 = {v: k for k, v in checkpoint.detectron2_to_local_keys(self.model, 3 if self.model.use_dropout else 2).items()}
        owners = list(self.params)
        if self.masters is not None:
            owners[len(owners) - len(self.masters.params):] = [c.weight for c in self.masters.convs]
        return [to_d2[local[id(p)]] for p in owners]

    def momentum_state(self) -> Dict[str, torch.Tensor]:
        """The momentum buffers on the CPU under param_names(), from whichever optimiser steps; zeros where torch's has not stepped yet
        (its first step, buf = g', is what a zero buffer gives)."""
        out = {}
        for i, (name, p) in enumerate(zip(self.param_names(), self.params)):
            buf = self.fused.buffers[i] if self.fused is not None else self.opt.state.get(p, {}).get("momentum_buffer")
            out[name] = torch.zeros(p.shape, dtype=p.dtype) if buf is None else buf.detach().cpu().clone()
        return out

    def load_momentum_state(self, state: Dict[str, torch.Tensor]) -> None:
        """Raises ValueError unless `state` holds exactly param_names(), each of its parameter's shape."""
        names = self.param_names()
        if sorted(names) != sorted(state):
            odd = sorted(set(names) ^ set(state))
            raise ValueError("the momentum buffers' names do not match the trained parameters (e.g. {})".format(odd[:3]))
        for i, (name, p) in enumerate(zip(names, self.params)):
            if tuple(state[name].shape) != tuple(p.shape):
                raise ValueError("momentum of {}: shape {} in the file, {} in the model".format(name, tuple(state[name].shape), tuple(p.shape)))
        with torch.no_grad():
            for i, (name, p) in enumerate(zip(names, self.params)):
                if self.fused is not None:
                    self.fused.buffers[i].copy_(state[name])
                else:
                    self.opt.state[p]["momentum_buffer"] = state[name].to(device=p.device, dtype=p.dtype).clone()

    def features(self, images: Sequence[torch.Tensor], padded=None):
        """The frozen backbone + FPN per image -> (per-level (B, 256, H, W) features, padded (h, w)).  train_fpn: only the backbone is
        frozen; the FPN runs on the batch's c3 - c5 with grad (fpn_train.fpn_forward_train).  padded: the batch's common padded size
        (--train-loader: anchors.padded_size of the largest height and width, detectron2's ImageList.from_tensors) -- every frame is run
        against it, whatever its own size; None: the frames are of one padded size, their own, and anything else raises."""
        per_image, common = [], None if padded is None else tuple(int(v) for v in padded)
        if self.train_backbone and self.freeze_at == 2:
            # the stem and res2 frozen, per image; res3 - res5 and the FPN on the batch with grad
            res2 = [res2_maps(self.model, im, common) for im in images]
            padded = common if common is not None else _padded_size(int(images[0].shape[-2]), int(images[0].shape[-1]))
            return fpn_forward_train(self.model.fpn, resnet_forward_train(self.model.bottom_up, res2)), padded
        if self.train_backbone:
            # FREEZE_AT 1: the stem and its pool frozen, per image; 0: they run with grad on the batch.  res2 - res5 and the FPN on the batch with grad
            maps = [pool_maps(self.model, im, common) for im in images] if self.freeze_at == 1 else stem_forward_train(self.model, images, padded=common)
            padded = common if common is not None else _padded_size(int(images[0].shape[-2]), int(images[0].shape[-1]))
            return fpn_forward_train(self.model.fpn, resnet_forward_train(self.model.bottom_up, maps, self.freeze_at)), padded
        padded = None
        if self.train_fpn:
            for im in images:
                maps, pad = backbone_maps(self.model, im, common)
                if padded is not None and tuple(pad) != tuple(padded):
                    raise ValueError("a batch holds frames of one padded size, got {} and {}".format(padded, pad))
                padded = tuple(pad)
                per_image.append(maps)
            return fpn_forward_train(self.model.fpn, per_image), padded
        with torch.no_grad():
            for im in images:
                feats, pad = self.model._trunk_eager(im, common)
                if padded is not None and tuple(pad) != tuple(padded):
                    raise ValueError("a batch holds frames of one padded size, got {} and {}".format(padded, pad))
                padded = tuple(pad)
                per_image.append(feats)
            stacked = [torch.cat([f[l] for f in per_image]).contiguous() for l in range(len(per_image[0]))]
        return stacked, padded

    def step(self, feats, padded, image_hw, gt_boxes, gt_classes, eps=None, normalizer=None) -> Dict[str, torch.Tensor]:
        """One iteration on the stacked features of a batch; returns the losses (device scalars; under data_parallel this rank's own --
        `mean_losses()` holds the rank means)."""
        res = self.forward_backward(feats, padded, image_hw, gt_boxes, gt_classes, eps=eps, normalizer=normalizer)
        if self.bucket is not None:
            self.reduce_gradients()
        self.optimizer_step(self._lr)
        self.advance()
        return res

    def forward_backward(self, feats, padded, image_hw, gt_boxes, gt_classes, eps=None, normalizer=None) -> Dict[str, torch.Tensor]:
        """The first part of a step: this iteration's learning rate, the head's forward, the losses and backward().  Leaves the gradients
        in .grad and returns the losses (device scalars)."""
        self._lrs = self.lrs_at(self.iteration)
        self._lr = self._lrs[0]
        for k, g in enumerate(self.opt.param_groups):
            g["lr"] = self._lrs[min(k, len(self._lrs) - 1)]
        out = self.model.head.forward_train(feats, self.model.anchors_for(tuple(padded)), image_hw)
        res = self.model.losses(out, gt_boxes, gt_classes, eps=eps, normalizer=normalizer)
        self.opt.zero_grad(set_to_none=True)
        (res["loss_cls"] + res["loss_box_reg"]).backward()
        self._losses = {k: v.detach() for k, v in res.items()}        # (what reduce_gradients puts into the bucket's tail)
        return res

    def reduce_gradients(self) -> None:
        """data_parallel only, between forward_backward and optimizer_step: the gradients times 1 / world into the bucket (K26, one
        launch), this rank's two losses behind them, and the one all-reduce -- after it the bucket holds the rank means."""
        if self.bucket is None:
            raise ValueError("reduce_gradients: this trainer was built without data_parallel")
        self.bucket.pack()
        self.bucket.set_tail(self._losses["loss_cls"], self._losses["loss_box_reg"])
        self.bucket.all_reduce()

    def mean_losses(self) -> Dict[str, torch.Tensor]:
        """data_parallel: the rank means of the last step's losses (device scalars, views of the bucket's tail), as detectron2's
        reduce_dict logs them."""
        return {"loss_cls": self.bucket.tail[0], "loss_box_reg": self.bucket.tail[1]}

    def advance(self) -> None:
        """The end of a step: the loss state's step (PR:146) and the iteration count."""
        self.model.loss_state.current_step += 1
        self.iteration += 1

    def optimizer_step(self, lr: float) -> None:
        """From the gradients backward() left (data_parallel: from the averaged ones in the bucket) to the stepped weights and refolded
        filters."""
        if self.fused is not None:
            if self.solver.plain_step:
                self.fused.step(lr)               # K25: s dW', the step on W and W' = W s in one launch; bumps the written tensors' versions
            else:                                 # K29: the same under the solver's settings; the guard also watches the step's two losses
                self.fused.step([lr] + self._lrs[1:], iteration=self.iteration, watch=self._watched_losses() if self.solver.computes_norm else ())
            if self.masters is not None:
                for c in self.masters.convs:
                    c.weight.grad = None          # (as collect_grads leaves them)
            return
        if self.masters is not None:
            self.masters.collect_grads()          # W.grad = s dW': the optimiser steps the unfolded weights
        self._clip_gradients()                    # (after collect_grads: what is clipped is s dW')
        self.opt.step()                           # bumps the weights' versions: the filters and HIP graphs derived from them are rebuilt
        if self.masters is not None:
            self.masters.refold()                 # conv.weight = W s, in place

    def _watched_losses(self) -> List[torch.Tensor]:
        """The step's two loss values as fp32 device scalars: the bucket's tail (the rank means) under data parallelism."""
        if self.bucket is not None:
            return [self.bucket.tail[0:1], self.bucket.tail[1:2]]
        if self._losses is None:
            return []
        return [self._losses[k].reshape(1).to(torch.float32) for k in ("loss_cls", "loss_box_reg")]

    def _clip_gradients(self) -> None:
        """Torch's path: detectron2's maybe_add_gradient_clipping -- `value` and `norm` per parameter, `full_model` once over all."""
        kind, v = self.solver.clip_type, self.solver.clip_value
        have = [p for p in self.params if p.grad is not None]
        if kind == "value":
            for p in have:
                torch.nn.utils.clip_grad_value_(p, v)
        elif kind == "norm":
            for p in have:
                torch.nn.utils.clip_grad_norm_(p, v)
        elif kind == "full_model" and have:
            self._grad_norm = torch.nn.utils.clip_grad_norm_(have, v)

    def check_finite(self) -> Optional[dict]:
        """What log steps and checkpoints call before they read back or write: under guard_nonfinite the fused step's status is read (the
        one synchronisation) and FloatingPointError raised if a step was bad -- the weights are then those from before that iteration.
        Returns the status (None where there is none)."""
        if self.fused is None or self.solver.plain_step:
            return None
        st = self.fused.status()
        if st is not None and st["poisoned"]:
            raise FloatingPointError("gradient or loss became infinite or NaN at iteration {}".format(st["first_bad_iteration"]))
        return st

    def grad_norm(self, status: Optional[dict] = None) -> Optional[float]:
        """The last step's gradient norm over the full model where one was computed (a read-back: log steps only), else None.  status: what
        check_finite() returned, if it was just called."""
        if self.fused is not None:
            if not self.solver.computes_norm:
                return None
            st = status if status is not None else self.fused.status()
            return None if st is None else st["last_norm"]
        return None if self._grad_norm is None else float(self._grad_norm)


def save_checkpoint(model, shadow, out_dir: str, name: str, iteration: int, train_fpn: bool = False, train_backbone: bool = False, masters=None,
                    trainer=None, sampler=None, random_seed: int = 0, ranks=None) -> str:
    """`shadow`: the same model unfolded (conv + FrozenBN pairs) on the CPU -- the form detectron2's names describe; it receives the
    trained head (train_fpn: and the trained FPN, which has no norm to unfold; train_backbone: and the master weights of res3 - res5,
    `masters` = the trainer's FoldedMasters) and is written as <out_dir>/<name>.pth, named in <out_dir>/last_checkpoint.  trainer: the
    file also carries `pod_trainer`, the state --resume continues from (trainer_state; `sampler`: the FrameSampler of the run; `ranks`:
    every rank's loss state, of a data-parallel run)."""
    os.makedirs(out_dir, exist_ok=True)
    pairs = list(zip(head_convs(shadow.head), head_convs(model.head)))
    if train_fpn or train_backbone:
        pairs += list(zip(fpn_convs(shadow.fpn), fpn_convs(model.fpn)))
    if train_backbone:
        if masters is None:
            raise ValueError("save_checkpoint(train_backbone=True) needs the trainer's master weights (HeadTrainer.masters)")
        masters.copy_to(unfolded_pairs(shadow.bottom_up, masters.freeze_at))
    with torch.no_grad():
        for dst, src in pairs:
            dst.weight.copy_(src.weight.detach().cpu())
            dst.bias.copy_(src.bias.detach().cpu())
    path = os.path.join(out_dir, name + ".pth")
    data = {"model": checkpoint.to_detectron2_state_dict(shadow, with_dropout_entries=model.use_dropout), "iteration": int(iteration)}
    if trainer is not None:
        data[TRAINER_KEY] = trainer_state(trainer, sampler, random_seed, ranks=ranks)
    torch.save(data, path)
    with open(os.path.join(out_dir, "last_checkpoint"), "w") as f:
        f.write(name + ".pth")
    return path


TRAINER_KEY = "pod_trainer"


class FrameSampler:
    """The data order of train_head as state: the position within the pass over the data set, the frames waiting in the shape buckets, and
    the generator of the flip draws (one draw per frame, in data order, only with random_flip)."""

    def __init__(self, batch: int, random_flip: bool = False, seed: int = 0):
        self.batch, self.random_flip = max(1, int(batch)), bool(random_flip)
        self.generator = torch.Generator().manual_seed(int(seed))
        self.buckets: Dict[tuple, list] = {}
        self.next_index, self.arrivals = 0, 0

    def draw_flip(self) -> bool:
        return bool(torch.rand((), generator=self.generator) < 0.5) if self.random_flip else False

    def add(self, index: int, flipped: bool, image, boxes, classes):
        """Files a frame under its shape; returns the (images, boxes, classes) of a batch once `batch` frames of that shape wait, else None."""
        bucket = self.buckets.setdefault(tuple(image.shape), [])
        bucket.append((self.arrivals, int(index), bool(flipped), image, boxes, classes))
        self.arrivals += 1
        if len(bucket) < self.batch:
            return None
        _, _, _, images, gb, gc = zip(*bucket)
        bucket.clear()
        return images, list(gb), list(gc)

    def add_keyed(self, key, index: int, flipped: bool):
        """`add` without the frame (data parallelism: a rank decodes only its own frames): files (index, flipped) under `key`, the shape the
        frame will have; returns the batch's [(index, flipped)] in arrival order once `batch` entries of that key wait, else None."""
        bucket = self.buckets.setdefault(tuple(key), [])
        bucket.append((self.arrivals, int(index), bool(flipped), None, None, None))
        self.arrivals += 1
        if len(bucket) < self.batch:
            return None
        out = [(e[1], e[2]) for e in bucket]
        bucket.clear()
        return out

    def state(self) -> dict:
        pending = sorted(e[:3] for b in self.buckets.values() for e in b)
        return {"next_index": int(self.next_index), "pending": [[int(i), int(f)] for _, i, f in pending], "flip_generator": self.generator.get_state().clone()}

    def load_state(self, state: dict) -> List[list]:
        """Restores position and generator; returns the pending (index, flipped) pairs, which the caller re-reads and files in order."""
        self.next_index = int(state["next_index"])
        self.generator.set_state(state["flip_generator"])
        return [[int(i), int(f)] for i, f in state["pending"]]


SAMPLER_KINDS = ("frame_sampler", "train_loader")       # FrameSampler's state carries no `kind`; train_loader.TrainPlan's names itself


def check_sampler_kind(state: Optional[dict], train_loader: bool, path: str) -> None:
    """--resume: SystemExit naming the file and both kinds unless the checkpoint's data order is of the kind this run continues."""
    if state is None:
        return
    wrote = (state.get("sampler") or {}).get("kind", SAMPLER_KINDS[0])
    runs = SAMPLER_KINDS[1 if train_loader else 0]
    if wrote != runs:
        raise SystemExit("--resume: the data order in {} is of kind `{}`, this run's is `{}`: resume it {} --train-loader".format(
            path, wrote, runs, "with" if wrote == SAMPLER_KINDS[1] else "without"))


def loss_state_of(trainer: HeadTrainer) -> dict:
    """The loss state of this trainer's model as a checkpoint holds it (a rank's own under data parallelism)."""
    ls = trainer.model.loss_state
    norm = ls.loss_normalizer
    return {"current_step": int(ls.current_step), "draws": int(ls.draws),
            "loss_normalizer": (norm.detach() if torch.is_tensor(norm) else torch.tensor(float(norm))).to("cpu", torch.float64).reshape(())}


def trainer_state(trainer: HeadTrainer, sampler: Optional[FrameSampler] = None, random_seed: int = 0, ranks: Optional[List[dict]] = None) -> dict:
    """What a run needs beside the weights to continue where it stopped -- tensors, numbers, strings, lists and dicts only (the restricted
    unpickler reads it).  ranks: a data-parallel run of more than one rank adds `world` and `ranks`, every rank's loss_state_of in rank
    order (`loss_state` is this rank's); a one-rank run writes the keys it always wrote."""
    state = {"iteration": int(trainer.iteration), "loss_state": loss_state_of(trainer),
             "momentum": trainer.momentum_state(), "momentum_mu": float(trainer.momentum_mu), "trained": trainer.trained(),
             "sampler": (sampler if sampler is not None else FrameSampler(1, seed=random_seed)).state(), "random_seed": int(random_seed)}
    if ranks is not None and len(ranks) > 1:
        state["world"], state["ranks"] = len(ranks), [dict(r) for r in ranks]
    return state


def check_world(state: dict, world: int, path: str) -> None:
    """SystemExit naming the file and both sizes unless `state` was written by a run of `world` ranks (a file without the field: by one)."""
    wrote = int(state.get("world", 1))
    if wrote != int(world) or (wrote > 1 and len(state.get("ranks", [])) != wrote):
        raise SystemExit("--resume: {} was written by a run of {} rank{}, this one has {}: resume with the same world size".format(
            path, wrote, "" if wrote == 1 else "s", int(world)))


def read_trainer_state(path: str) -> dict:
    """The `pod_trainer` entry of a checkpoint file; SystemExit naming the file if it has none."""
    data = torch.load(path, map_location="cpu", weights_only=True)
    if not isinstance(data, dict) or not isinstance(data.get(TRAINER_KEY), dict):
        raise SystemExit("--resume: {} holds no `{}` entry (weights only: written without the trainer's state, or not by train_head); "
                         "run without --resume to fine-tune from its weights at iteration 0".format(path, TRAINER_KEY))
    return data[TRAINER_KEY]


def restore_trainer(trainer: HeadTrainer, state: dict, path: str) -> None:
    """Iteration, loss state and momentum from a checkpoint's `pod_trainer`; SystemExit naming the file where it does not fit this run
    (its world size among the rest: a rank of a data-parallel run takes its own entry of `ranks`)."""
    check_world(state, trainer.world, path)
    if list(state.get("trained", [])) != trainer.trained():
        raise SystemExit("--resume: {} comes from a run that trained {}, this one trains {}: give the same --train-fpn / --train-backbone".format(
            path, " + ".join(state.get("trained", [])) or "nothing", " + ".join(trainer.trained())))
    try:
        trainer.load_momentum_state(state["momentum"])
    except ValueError as e:
        raise SystemExit("--resume: {}: {}".format(path, e))
    trainer.iteration = int(state["iteration"])
    trainer._lrs = trainer.lrs_at(trainer.iteration)
    trainer._lr = trainer._lrs[0]
    ls, own = trainer.model.loss_state, state["ranks"][trainer.rank] if trainer.world > 1 else state["loss_state"]
    ls.current_step, ls.draws = int(own["current_step"]), int(own["draws"])
    ls.loss_normalizer = float(own["loss_normalizer"])


def arg_parser():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0],
                                 epilog="A step takes SOLVER.IMS_PER_BATCH frames of ONE resized shape: the sampler batches frames of equal shape "
                                        "together, in data-set order; frames of a shape wait until a batch of them is complete -- unless "
                                        "--train-loader is given: then a batch holds frames of one aspect-ratio group, of any sizes, in "
                                        "detectron2's shuffled order at INPUT.MIN_SIZE_TRAIN, padded to one size.  Only the head "
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
    ap.add_argument("--bbox-cov-loss", default=None, choices=losses.BBOX_COV_LOSSES,
                    help="overrides MODEL.PROBABILISTIC_MODELING.BBOX_COV_LOSS.NAME: what trains the box covariance (energy_loss and "
                         "second_moment_matching run on K27).  No checkpoint records the name: with --resume it is again the config's, or this flag's")
    ap.add_argument("--bbox-cov-type", default=None, choices=("diagonal", "full"),
                    help="overrides BBOX_COV_LOSS.COVARIANCE_TYPE: `full` gives the head the ten-channel predictor of a 4 x 4 Cholesky factor, "
                         "trained on K28 under every --bbox-cov-loss name.  With --resume the type is again the config's, or this flag's; a "
                         "checkpoint of the other type is refused by its shapes")
    ap.add_argument("--bbox-cov-samples", type=int, default=0, help="overrides BBOX_COV_LOSS.NUM_SAMPLES, the energy loss's samples per positive anchor")
    ap.add_argument("--random-seed", type=int, default=0)
    ap.add_argument("--max-iter", type=int, default=-1, help="overrides SOLVER.MAX_ITER")
    ap.add_argument("--log-period", type=int, default=20, help="a loss line every this many iterations (the only host read-back); 0: none")
    ap.add_argument("--min-size-test", type=int, default=0, help="overrides INPUT.MIN_SIZE_TEST")
    ap.add_argument("--max-size-test", type=int, default=0, help="overrides INPUT.MAX_SIZE_TEST")
    ap.add_argument("--loader-workers", type=int, default=-1, help="host threads of the loader; -1 = the config's value")
    ap.add_argument("--train-fpn", action="store_true", help="train the FPN's eight convolutions together with the head (the ResNet stays frozen)")
    ap.add_argument("--train-backbone", action="store_true", help="train res3 - res5 of the ResNet too, as detectron2 does at MODEL.BACKBONE.FREEZE_AT = 2 "
                                                                  "(implies --train-fpn; the stem and res2 stay frozen unless the config's "
                                                                  "MODEL.BACKBONE.FREEZE_AT says 1: res2 trains too, or 0: and the stem)")
    ap.add_argument("--fused-step", action="store_true", help="the optimiser's step as one launch of the project's own kernel (K25) in place of "
                                                              "torch.optim.SGD and the refold passes around it")
    ap.add_argument("--guard-nonfinite", action="store_true", help="stop at the first non-finite gradient or loss as detectron2's trainer does, without a "
                                                                   "synchronisation per step: the fused step (K29) checks on the device and writes nothing "
                                                                   "from that iteration on; log steps and checkpoints read the status and raise "
                                                                   "FloatingPointError before anything is written; implies --fused-step")
    ap.add_argument("--random-flip", action="store_true", help="detectron2's RandomFlip: every frame is mirrored with probability 0.5 (drawn in "
                                                               "data order from --random-seed), its boxes with it")
    ap.add_argument("--train-loader", action="store_true", help="detectron2's training loader (pod_compare_amd/train_loader.py): frames without usable "
                                                                "annotations dropped (DATALOADER.FILTER_EMPTY_ANNOTATIONS), a seeded shuffle per pass, "
                                                                "INPUT.MIN_SIZE_TRAIN / MAX_SIZE_TRAIN / MIN_SIZE_TRAIN_SAMPLING and RANDOM_FLIP drawn per "
                                                                "frame, batches grouped by aspect ratio only (DATALOADER.ASPECT_RATIO_GROUPING) and padded "
                                                                "to one size, read ahead on the loader threads -- for a data-parallel rank too")
    ap.add_argument("--no-shuffle", action="store_true", help="--train-loader: keep the json's file order")
    ap.add_argument("--batch-on-gpu", action="store_true", help="--train-loader: the loader threads only decode; ONE launch (K31) resizes, mirrors, "
                                                                "flips to BGR and transposes the batch's frames; bit-identical to the host path")
    ap.add_argument("--resume", action="store_true", help="continue the run OUTPUT_DIR/last_checkpoint stopped in: its weights and its trainer state "
                                                          "(iteration, loss state, momentum, data position); refused if the file carries none")
    ap.add_argument("--val-coco-json", default="", help="COCO-format validation set (not the training json): evaluated every TEST.EVAL_PERIOD "
                                                        "iterations and after the last one, as detectron2's EvalHook does (train_eval.py, K32)")
    ap.add_argument("--val-image-root", default="", help="directory of the files named in --val-coco-json")
    ap.add_argument("--eval-only", action="store_true", help="train_net.py's flag: load MODEL.WEIGHTS (or OUTPUT_DIR/last_checkpoint with --resume), "
                                                             "evaluate --val-coco-json once, print and return the results; builds no optimiser")
    ap.add_argument("--data-parallel", action="store_true", help="one rank of a data-parallel run (RANK / WORLD_SIZE / LOCAL_RANK, as torch.distributed.run "
                                                                 "sets them): the rank takes its share of every batch of SOLVER.IMS_PER_BATCH frames, the "
                                                                 "gradients are averaged over the ranks through one bucket (K26) and one all-reduce; implies "
                                                                 "--fused-step")
    ap.add_argument("--backend", default="nccl", help="--data-parallel: torch.distributed backend: nccl = RCCL over xGMI (the real path); gloo for a "
                                                      "functional run, e.g. several ranks on one GPU with --share-gpu")
    ap.add_argument("--share-gpu", action="store_true", help="--data-parallel, functional check only: every rank uses cuda:0")
    ap.add_argument("--device", default="cuda:0")
    return ap


def main(argv=None):
    args = arg_parser().parse_args(argv)
    rank, world, group, own_group = 0, 1, None, False
    if args.guard_nonfinite:
        args.fused_step = True
    if args.data_parallel:
        import torch.distributed as dist
        args.fused_step = True
        if dist.is_initialized():                          # the caller's process group (and its --device) is used as it is
            rank, world = dist.get_rank(), dist.get_world_size()
        else:
            rank, world = int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))
            local_rank = 0 if args.share_gpu else int(os.environ.get("LOCAL_RANK", "0"))
            args.device = "cuda:%d" % local_rank
            if world > 1:
                if args.backend == "nccl":
                    dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))
                else:
                    dist.init_process_group(args.backend)
                own_group = True
    try:
        return _run(args, rank, world, group, bind=own_group)
    finally:
        if own_group:
            dist.destroy_process_group()


def _ground_truth(path: str) -> dict:
    with open(path, "r") as f:
        gt = json.load(f)
    if "annotations" not in gt:
        raise SystemExit("--coco-json needs `annotations`: the head is trained against ground truth")
    return gt


def _run(args, rank: int, world: int, group, bind: bool = False):
    """main behind its arguments and process group: rank `rank` of `world` (1: the one-GPU run).  bind: this process was started as a rank
    and is bound to its GPU's NUMA node, as apply_net binds its ranks (a caller that brought its own process group keeps its affinity)."""
    say = print if rank == 0 else (lambda *a, **k: None)              # only rank 0 prints and writes
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
    cov = covariance_overrides(cfg, args)
    freeze_at = cfg.MODEL.BACKBONE.get("FREEZE_AT", 2)
    if int(freeze_at) not in FREEZE_POINTS:
        raise SystemExit("MODEL.BACKBONE.FREEZE_AT = {} is not supported: with --train-backbone 2 (detectron2's default: the stem and res2 are "
                         "frozen and res3 - res5 train), 1 (res2 trains too) or 0 (and the stem); without it only 2".format(freeze_at))
    freeze_at = int(freeze_at)
    if freeze_at != 2 and not args.train_backbone:
        raise SystemExit("MODEL.BACKBONE.FREEZE_AT = {} needs --train-backbone: without it the ResNet stays frozen, which is what FREEZE_AT = 2 "
                         "(or no key) says".format(freeze_at))
    solver = solver_settings(cfg, guard_nonfinite=args.guard_nonfinite)      # (SystemExit for a key this trainer does not run, before a model is built)
    eval_period = evaluation_period(cfg, args)                               # (and for an evaluation that has no validation set)
    if args.eval_only:
        return _eval_only(args, cfg, rank, world, group, say)
    train_fpn = args.train_fpn or args.train_backbone
    # --resume: the file last_checkpoint names, if there is one (none: the run starts as without the flag, as detectron2's resume_or_load)
    resume_from = checkpoint.resolve_checkpoint(cfg.OUTPUT_DIR, "") if args.resume else ""
    resume_state = read_trainer_state(resume_from) if resume_from else None
    trains = trained_parts(train_fpn, args.train_backbone, freeze_at)
    if resume_state is not None and list(resume_state.get("trained", [])) != trains:          # (before a model is built; restore_trainer checks the rest)
        raise SystemExit("--resume: {} comes from a run that trained {}, this one trains {}: give the same --train-fpn / --train-backbone".format(
            resume_from, " + ".join(resume_state.get("trained", [])) or "nothing", " + ".join(trains)))
    if resume_state is not None:
        check_world(resume_state, world, resume_from)
    check_sampler_kind(resume_state, args.train_loader, resume_from)
    if (args.no_shuffle or args.batch_on_gpu) and not args.train_loader:
        raise SystemExit("--no-shuffle and --batch-on-gpu belong to --train-loader")
    plan, gt = None, None
    if args.train_loader:         # the whole data order from the config and the json alone: SystemExit for a key the loader does not run or a
        from . import train_loader                    # record without height / width, before a model is built
        plan_cfg = train_loader.plan_settings(cfg, random_flip=args.random_flip, shuffle=not args.no_shuffle, seed=args.random_seed)
        gt = _ground_truth(args.coco_json)
        planned = train_loader.planned_indices(gt["images"], gt["annotations"], evaluation_category_map(args.train_dataset, args.test_dataset),
                                               plan_cfg.filter_empty)
        if len(planned) < len(gt["images"]):
            say("Removed {} images with no usable annotations. {} images left.".format(len(gt["images"]) - len(planned), len(planned)), flush=True)
        plan = train_loader.TrainPlan(train_loader.frame_sizes(gt["images"], args.coco_json), planned, plan_cfg)
    first, last = rank_slice(max(1, int(cfg.SOLVER.IMS_PER_BATCH)), rank, world)           # this rank's frames of every global batch
    dev = torch.device(args.device)
    torch.cuda.set_device(dev)
    if bind:                      # enqueue + loader threads of this rank on its GPU's NUMA node (hostbind.py; POD_BIND_NUMA=0: off)
        from . import hostbind
        b = hostbind.bind_rank_to_gpu_numa(dev.index or 0)
        say("rank %d: %s pci %s numa node %s -> %s" % (rank, dev, b["pci"], b["numa_node"], b["cpus"] if b["bound"] else "not bound (%s)" % b.get("why_not", "off")))
    if gt is None:
        gt = _ground_truth(args.coco_json)
    by_image: Dict[object, List[dict]] = {}
    for a in gt["annotations"]:
        by_image.setdefault(a["image_id"], []).append(a)
    cat_map = evaluation_category_map(args.train_dataset, args.test_dataset)
    dataset = CocoImages(args.coco_json, args.image_root, cfg.INPUT.MIN_SIZE_TEST, cfg.INPUT.MAX_SIZE_TEST, device_resize=args.batch_on_gpu)
    # the model twice from one seed: on the device with FrozenBN folded (what runs), and unfolded on the CPU (what a checkpoint describes)
    load = not args.random_init or bool(resume_from)       # (a resumed run's weights are the checkpoint's, whatever the first run started from)
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
                                                  seed=args.random_seed + rank, bbox_cov_loss=cov.NAME, bbox_cov_num_samples=int(cov.NUM_SAMPLES))
    model.head.dropout_seed += rank                        # a rank's loss samples and dropout masks are its own, as detectron2 seeds its ranks
    max_iter = args.max_iter if args.max_iter >= 0 else int(s.MAX_ITER)
    trainer = HeadTrainer(model, base_lr=s.BASE_LR, momentum=s.MOMENTUM, weight_decay=s.WEIGHT_DECAY, steps=s.STEPS, gamma=s.GAMMA,
                          warmup_iters=s.WARMUP_ITERS, warmup_factor=s.WARMUP_FACTOR, train_fpn=train_fpn, train_backbone=args.train_backbone,
                          shadow=shadow if args.train_backbone else None, fused_step=args.fused_step,
                          data_parallel=(rank, world, group) if args.data_parallel else None, solver=solver, max_iter=max_iter, freeze_at=freeze_at)
    batch, period = max(1, int(s.IMS_PER_BATCH)), int(s.CHECKPOINT_PERIOD)
    workers = args.loader_workers if args.loader_workers >= 0 else int(cfg.DATALOADER.NUM_WORKERS)
    sampler = FrameSampler(batch, random_flip=args.random_flip, seed=args.random_seed)
    saved = dict(train_fpn=train_fpn, train_backbone=args.train_backbone, masters=trainer.masters, trainer=trainer,
                 sampler=sampler if plan is None else plan, random_seed=args.random_seed)

    def frame(d: dict, flipped: bool):
        """One loader entry on the device with its ground truth in network-input pixels, mirrored if the draw said so."""
        image = d["image"].to(dev, non_blocking=True)
        sy, sx = image.shape[1] / float(d["height"]), image.shape[2] / float(d["width"])
        boxes, classes = image_ground_truth(by_image.get(d["image_id"], []), cat_map, sx, sy)
        if flipped:
            image, boxes = image.flip(-1), hflip_boxes(boxes, float(image.shape[2]))
        return image, boxes, classes

    def shape_key(index: int):
        """--data-parallel: the shape frame `index` will have, from the json alone -- every rank files every frame, and decodes only its own."""
        rec = dataset.images[index]
        if "height" not in rec or "width" not in rec:
            raise SystemExit("--data-parallel: image {} of {} has no `height` / `width`: the ranks agree on the batches from the json "
                             "alone".format(rec.get("file_name", index), args.coco_json))
        return (3,) + tuple(resize_shortest_edge(int(rec["height"]), int(rec["width"]), dataset.min_size, dataset.max_size))

    def file_frame(index: int, flipped: bool, d=None):
        """Files a frame with the sampler; a complete batch comes back as this rank's (images, boxes, classes) of it."""
        if not args.data_parallel:
            return sampler.add(index, flipped, *frame(dataset[index] if d is None else d, flipped))
        ready = sampler.add_keyed(shape_key(index), index, flipped)
        if ready is None:
            return None
        images, gb, gc = zip(*[frame(dataset[i], f) for i, f in ready[first:last]])
        return images, list(gb), list(gc)

    def write(name: str, it: int):
        """A checkpoint: every rank hands in its loss state (the one collective of a checkpoint), rank 0 writes the file.  Under
        --guard-nonfinite the status is read first: after a bad step nothing is written (every rank decides alike, before the collective)."""
        trainer.check_finite()
        ranks = gather_objects(loss_state_of(trainer), world, group) if world > 1 else None
        if rank == 0:
            written.append(save_checkpoint(model, shadow, cfg.OUTPUT_DIR, name, it, ranks=ranks, **saved))

    if resume_state is not None and plan is not None:
        restore_trainer(trainer, resume_state, resume_from)
        try:
            plan.load_state(resume_state["sampler"])
        except (ValueError, KeyError) as e:
            raise SystemExit("--resume: {}: {}".format(resume_from, e))
        say("resumed %s at iteration %d" % (resume_from, trainer.iteration), flush=True)
    elif resume_state is not None:
        restore_trainer(trainer, resume_state, resume_from)
        for index, flipped in sampler.load_state(resume_state["sampler"]):       # the frames that waited in the buckets, in arrival order
            if not 0 <= index < len(dataset) or file_frame(index, bool(flipped)) is not None:
                raise SystemExit("--resume: {}: its waiting frames do not fit this data set and SOLVER.IMS_PER_BATCH".format(resume_from))
        if not 0 <= sampler.next_index < max(1, len(dataset)):
            raise SystemExit("--resume: {}: stopped at frame {} of a data set of {}".format(resume_from, sampler.next_index, len(dataset)))
        say("resumed %s at iteration %d" % (resume_from, trainer.iteration), flush=True)
    if world > 1:                 # once: every rank starts from rank 0's trained tensors (the masters and the filters folded from them) and momentum
        folded = [c.weight for c in trainer.masters.convs] if trainer.masters is not None else []
        broadcast_tensors(trainer.params + folded + trainer.fused.buffers, group)
    written, last_line, stalled = [], None, 0
    extra, evaluations = {}, []

    def evaluate(it: int):
        """Trainer.test on the validation set with the model as it stands after iteration `it`; every rank takes part, rank 0 reports."""
        from . import train_eval
        res = train_eval.evaluate_model(model, cfg, args.val_coco_json, args.val_image_root, cfg.OUTPUT_DIR, args.train_dataset, args.test_dataset,
                                        workers=workers, rank=rank, world=world, group=group, say=say)
        say(train_eval.ap_line(it, res), flush=True)
        evaluations.append((it, res))
        return res

    def after_step(res):
        """The log line and the periodic checkpoint behind a step."""
        nonlocal last_line
        it = trainer.iteration
        if args.log_period > 0 and (it % args.log_period == 0 or it == max_iter):
            norm = trainer.grad_norm(trainer.check_finite())                      # (FloatingPointError after a bad step, under --guard-nonfinite)
            shown = trainer.mean_losses() if args.data_parallel else res          # (the rank means, from the bucket's tail)
            last_line = "iter %d  loss_cls %.6f  loss_box_reg %.6f  lr %.6g" % (it, float(shown["loss_cls"]), float(shown["loss_box_reg"]),
                                                                              trainer.lr)
            if norm is not None:
                last_line += "  grad_norm %.6g" % norm
            say(last_line, flush=True)
        if eval_period > 0 and it % eval_period == 0 and it != max_iter:          # EvalHook.after_step; the last iteration's follows the loop
            evaluate(it)
        if period > 0 and it % period == 0 and it < max_iter:
            write("model_%07d" % (it - 1), it)

    if plan is not None:
        extra = _train_on_plan(args, plan, dataset, trainer, by_image, cat_map, dev, workers, first, last, max_iter, after_step)
    while trainer.iteration < max_iter:
        progressed = False
        indices = range(sampler.next_index, len(dataset))
        # --data-parallel: the index stream alone; a rank reads a frame when the batch that holds it is complete
        for index, d in (((i, None) for i in indices) if args.data_parallel else Prefetched(dataset, indices, workers=workers)):
            flipped = sampler.draw_flip()
            ready = file_frame(index, flipped, d)
            sampler.next_index = (index + 1) % len(dataset)
            if ready is None:
                continue
            images, gb, gc = ready
            feats, padded = trainer.features(images)
            res = trainer.step(feats, padded, tuple(images[0].shape[-2:]), gb, gc)
            progressed = True
            after_step(res)
            it = trainer.iteration
            if it >= max_iter:
                break
        else:
            sampler.next_index = 0
        stalled = 0 if progressed else stalled + 1      # (an incomplete batch carries over into the next pass over the data set)
        if stalled >= batch:
            raise SystemExit("no batch of {} frames of one resized shape can be formed from {} frames".format(batch, len(dataset)))
    if args.val_coco_json:                 # EvalHook.after_train, then DefaultTrainer.train's verify_results
        from . import train_eval
        extra["eval_results"] = evaluate(trainer.iteration)
        extra["evaluations"] = evaluations
        if rank == 0:
            train_eval.verify_results(cfg, extra["eval_results"], say)
    write("model_final", trainer.iteration)
    if world > 1:
        import torch.distributed as dist
        dist.barrier(group)               # no rank leaves before the final checkpoint is on disk
    what = ", the FPN and " + ("res3", "res2", "the stem, res2")[2 - freeze_at] + " - res5" if args.train_backbone else " and the FPN" if train_fpn else ""
    if rank == 0:
        print("trained the head%s for %d iterations; wrote %s" % (what, trainer.iteration, written[-1]))
    return dict({"iterations": trainer.iteration, "checkpoints": written, "output_dir": cfg.OUTPUT_DIR, "model": model, "last_line": last_line,
                 "trainer": trainer}, **extra)


def evaluation_period(cfg, args) -> int:
    """TEST.EVAL_PERIOD, checked against the flags before a model is built: SystemExit naming the key or the flag for an evaluation that
    has no validation set to run on."""
    period = cfg.TEST.get("EVAL_PERIOD", 0)
    if isinstance(period, bool) or not isinstance(period, int) or period < 0:
        raise SystemExit("TEST.EVAL_PERIOD = {!r} is not supported: a non-negative number of iterations (0: no periodic evaluation)".format(period))
    if period > 0 and not args.val_coco_json:
        raise SystemExit("TEST.EVAL_PERIOD = {} needs --val-coco-json and --val-image-root: the validation set is not the training json".format(period))
    if args.eval_only and not args.val_coco_json:
        raise SystemExit("--eval-only needs --val-coco-json and --val-image-root: the set to evaluate")
    if args.val_coco_json and not args.val_image_root:
        raise SystemExit("--val-coco-json needs --val-image-root: the directory of the files it names")
    return int(period)


def _eval_only(args, cfg, rank: int, world: int, group, say) -> dict:
    """train_net.py:67-76: build the model, resume_or_load(MODEL.WEIGHTS, resume=--resume), Trainer.test, verify_results.  No optimiser,
    no loss state, no training json."""
    from . import train_eval
    dev = torch.device(args.device)
    torch.cuda.set_device(dev)
    found = checkpoint.resolve_checkpoint(cfg.OUTPUT_DIR, "") if args.resume else ""
    torch.manual_seed(args.random_seed)
    # (--random-init evaluates the seeded initialisation unless a checkpoint is named: --weights, or last_checkpoint under --resume)
    model = build_model(cfg, save_dir="" if args.resume else None, load_weights=not args.random_init or bool(found) or args.weights is not None)
    say("evaluating %s" % (model.loaded_from or "the seeded random initialisation"), flush=True)
    workers = args.loader_workers if args.loader_workers >= 0 else int(cfg.DATALOADER.NUM_WORKERS)
    res = train_eval.evaluate_model(model, cfg, args.val_coco_json, args.val_image_root, cfg.OUTPUT_DIR, args.train_dataset, args.test_dataset,
                                    workers=workers, rank=rank, world=world, group=group, say=say)
    say(train_eval.ap_line(0, res), flush=True)
    if rank == 0:
        train_eval.verify_results(cfg, res, say)
    if world > 1:
        import torch.distributed as dist
        dist.barrier(group)
    return {"iterations": 0, "checkpoints": [], "output_dir": cfg.OUTPUT_DIR, "model": model, "last_line": None, "eval_results": res}


def _train_on_plan(args, plan, dataset, trainer, by_image, cat_map, dev, workers, first, last, max_iter, after_step) -> dict:
    """--train-loader's loop: the plan's global batches, this rank's entries [first, last) of each, read ahead pass by pass on `workers`
    threads (a batch that completes across a pass boundary belongs to the pass it completes in; the waiting entries carry over inside the
    plan).  The plan moves batch by batch, so a checkpoint's state is the position behind the last trained batch.  A frame's ground truth
    is scaled by (nw / w, nh / h) and mirrored against the frame's OWN resized width; the batch's frames are run against one padded size,
    anchors.padded_size of their largest height and width (detectron2's ImageList.from_tensors), which is also the `image_hw` handed
    to forward_train (informational).  Returns what main's result gains: the plan, the batches trained and the loader wait in seconds."""
    import time
    from . import train_loader
    frames = train_loader.PlannedFrames(dataset)
    trained, wait = [], 0.0
    while trainer.iteration < max_iter:
        ahead = plan.until_pass_end(limit=max_iter - trainer.iteration)
        stream = iter(Prefetched(frames, [e for b in ahead for e in b[first:last]], workers=workers))
        try:
            for _ in ahead:
                mine = plan.next_batch()[first:last]
                t0 = time.perf_counter()
                loaded = [next(stream)[1] for _ in mine]
                wait += time.perf_counter() - t0
                if args.batch_on_gpu:           # K31: the decoded frames -> the network inputs, one launch
                    from . import train_batch
                    images = train_batch.train_batch_u8([d["frame"].to(dev, non_blocking=True) for d in loaded], [e.size for e in mine],
                                                        [e.flipped for e in mine])
                else:                           # resized by the loader threads at the drawn size; mirrored here
                    images = [d["image"].to(dev, non_blocking=True) for d in loaded]
                    images = [im.flip(-1) if e.flipped else im for im, e in zip(images, mine)]
                gb, gc = [], []
                for d, e in zip(loaded, mine):
                    boxes, classes = image_ground_truth(by_image.get(d["image_id"], []), cat_map, e.size[1] / float(d["width"]), e.size[0] / float(d["height"]))
                    gb.append(hflip_boxes(boxes, float(e.size[1])) if e.flipped else boxes)
                    gc.append(classes)
                padded = train_loader.batch_padded_size(mine)
                feats, padded = trainer.features(images, padded=padded)
                res = trainer.step(feats, padded, tuple(padded), gb, gc)
                trained.append(mine)
                after_step(res)
                if trainer.iteration >= max_iter:
                    break
        finally:
            stream.close()
    return {"plan": plan, "trained": trained, "loader_wait": wait}


if __name__ == "__main__":
    main()
