"""The reference's training objective on the GPU (K21): anchor labelling and ProbabilisticRetinaNet.losses, PR:168-333.

    labels, matched_gt, num_pos = label_anchors(anchors, gt_boxes_per_image, gt_classes_per_image, num_classes)     # PR:129-130
    crit = ProbabilisticLosses(num_classes=7, cls_var_num_samples=10)
    out = crit(head_outputs, labels, matched_gt, gt_boxes, anchors)           # {"loss_cls", "loss_box_reg"}: device scalars, PR:333
    (out["loss_cls"] + out["loss_box_reg"]).backward()                        # gradients at the four head outputs
    crit = ProbabilisticLosses(num_classes=7, bbox_cov_loss="energy_loss", bbox_cov_num_samples=1000)          # BBOX_COV_LOSS.NAME: the
    # covariance term of loss_box_reg is the energy score (or "second_moment_matching") in place of the NLL: a second launch, K27
    # head outputs whose reg_var planes have A * 10 channels (BBOX_COV_LOSS.COVARIANCE_TYPE: full) take the same names to K28: the
    # Gaussian NLL of the 4 x 4 Cholesky factor, moment matching or the energy score of the full covariance (`covariance_route`)

Everything stays on the device: no call here reads a value back.  The convolutions have no backward pass -- the gradients stop at the
per-level head tensors (`(N, A*C, H, W)` planes, N = images), which is what a trainer of the head, or a checkpoint selection by
validation loss, needs first.  There is no CPU fallback: a missing library or a failing launch raises (hip.PodError).
"""
from typing import List, Optional, Sequence, Tuple

import torch

from . import hip

IOU_THRESHOLDS = (0.4, 0.5)          # Base-RetinaNet.yaml: MODEL.RETINANET.IOU_THRESHOLDS, labels [0, -1, 1]


def _cat_anchors(anchors) -> torch.Tensor:
    a = torch.cat(list(anchors)) if isinstance(anchors, (list, tuple)) else anchors
    return a.to(torch.float32).contiguous()


def concat_ground_truth(gt_boxes_per_image: Sequence[torch.Tensor], gt_classes_per_image: Sequence[torch.Tensor], device):
    """Per-image lists -> (gt_boxes (G, 4) fp32, gt_classes (G,) int32, gt_off (N + 1,) int32) on `device`, the concatenated form the
    kernels take (image i owns rows gt_off[i] .. gt_off[i + 1])."""
    assert len(gt_boxes_per_image) == len(gt_classes_per_image) and len(gt_boxes_per_image) >= 1
    counts = [int(b.shape[0]) for b in gt_boxes_per_image]
    for b, c in zip(gt_boxes_per_image, gt_classes_per_image):
        assert b.dim() == 2 and b.shape[1] == 4 and c.shape == (b.shape[0],), (tuple(b.shape), tuple(c.shape))
    off = [0]
    for n in counts:
        off.append(off[-1] + n)
    boxes = torch.cat([b.to(device, torch.float32).reshape(-1, 4) for b in gt_boxes_per_image]).contiguous()
    classes = torch.cat([c.to(device).reshape(-1) for c in gt_classes_per_image]).to(torch.int32).contiguous()
    return boxes, classes, torch.tensor(off, dtype=torch.int32).to(device, non_blocking=True)


def label_anchors(anchors, gt_boxes_per_image: Sequence[torch.Tensor], gt_classes_per_image: Sequence[torch.Tensor], num_classes: int,
                  iou_thresholds: Tuple[float, float] = IOU_THRESHOLDS):
    """PR:129-130 (detectron2 RetinaNet.label_anchors, Matcher with allow_low_quality_matches=True) for N images in one call.
    anchors: (R, 4) or the per-level list; gt_boxes_per_image[i]: (G_i, 4) XYXY in network-input pixels; gt_classes_per_image[i]: (G_i,).
    Returns device tensors: labels int32 (N, R) -- the class, `num_classes` for background, -1 for ignored --, matched_gt int32 (N, R)
    -- the arg-max box as a ROW OF THE CONCATENATED boxes (`concat_ground_truth`; -1 for an image without boxes) -- and num_pos int32 (N,)."""
    a = _cat_anchors(anchors)
    dev = a.device
    boxes, classes, off = concat_ground_truth(gt_boxes_per_image, gt_classes_per_image, dev)
    n, r, g = len(gt_boxes_per_image), int(a.shape[0]), int(boxes.shape[0])
    labels = torch.empty((n, r), dtype=torch.int32, device=dev)
    matched = torch.empty((n, r), dtype=torch.int32, device=dev)
    num_pos = torch.empty((n,), dtype=torch.int32, device=dev)
    scratch = torch.empty((max(g, 1),), dtype=torch.int32, device=dev)
    lib = hip.load()
    with torch.cuda.device(dev):
        hip.check(lib.pod_label_anchors(hip.ptr(a), r, hip.ptr(boxes) if g else None, hip.ptr(classes) if g else None, hip.ptr(off), n, g,
                                        int(num_classes), float(iou_thresholds[0]), float(iou_thresholds[1]), hip.ptr(labels), hip.ptr(matched),
                                        hip.ptr(num_pos), hip.ptr(scratch), hip.current_stream()), "pod_label_anchors")
    return labels, matched, num_pos


def annealing_weight(current_step: float, annealing_step: float) -> float:
    """PR:320-321: the weight of the NLL regression loss, 0 at step 0 and 1 from `annealing_step` on."""
    x = min(1.0, float(current_step) / float(annealing_step))
    return (100 ** x - 1.0) / (100.0 - 1.0)


def _launch_inputs(cls, delta, cls_var, reg_var, labels, matched_gt, gt_boxes, anchors, num_anchors: int, num_classes: int, box_weights,
                   cls_samples: int, seed: int, cov_dims: Optional[int]):
    """What pod_train_loss and pod_reg_score_loss take alike: (cfg, levels, anchors (R, 4), gt (G, 4)), every plane and index tensor checked."""
    L, n = len(cls), int(cls[0].shape[0])
    dev = cls[0].device
    D = (0 if reg_var is None else int(reg_var[0].shape[1]) // num_anchors) if cov_dims is None else int(cov_dims)
    cfg = hip.PodConfig()
    cfg.n_levels, cfg.n_runs, cfg.num_anchors, cfg.num_classes = L, n, int(num_anchors), int(num_classes)
    cfg.cov_dims, cfg.has_cls_var, cfg.cls_samples = D, int(cls_var is not None), int(cls_samples)
    for i in range(4):
        cfg.box_weights[i] = float(box_weights[i])
    cfg.philox_seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    lv = (hip.PodLevel * hip.POD_MAX_LEVELS)()
    a = _cat_anchors(anchors)
    r = int(a.shape[0])
    base = 0

    def plane(name, t, l, c, h, w_):
        if not (t.dtype == torch.float32 and t.is_contiguous() and t.device == dev and tuple(t.shape) == (n, num_anchors * c, h, w_)):
            raise hip.PodError("{}[{}]: expected contiguous fp32 {} on {}, got {} {} on {}".format(
                name, l, (n, num_anchors * c, h, w_), dev, t.dtype, tuple(t.shape), t.device))
        return t.data_ptr(), num_anchors * c * h * w_

    for l in range(L):
        h, w_ = int(cls[l].shape[2]), int(cls[l].shape[3])
        lv[l].cls, lv[l].run_stride_cls = plane("cls", cls[l], l, num_classes, h, w_)
        lv[l].delta, lv[l].run_stride_delta = plane("delta", delta[l], l, 4, h, w_)
        if cls_var is not None:
            lv[l].cls_var, _ = plane("cls_var", cls_var[l], l, num_classes, h, w_)
        if reg_var is not None and D > 0:
            lv[l].reg_var, lv[l].run_stride_reg = plane("reg_var", reg_var[l], l, D, h, w_)
        lv[l].H, lv[l].W, lv[l].anchor_base = h, w_, base
        base += h * w_ * num_anchors
    if base != r:
        raise hip.PodError("the levels hold {} anchors, `anchors` has {}".format(base, r))
    for name, t in (("labels", labels), ("matched_gt", matched_gt)):
        if not (t.dtype == torch.int32 and t.is_contiguous() and tuple(t.shape) == (n, r) and t.device == dev):
            raise hip.PodError("{}: expected contiguous int32 {} on {}".format(name, (n, r), dev))
    gt = gt_boxes.to(dev, torch.float32).reshape(-1, 4).contiguous()
    return cfg, lv, a, gt


def _weights_ok(w, dev) -> torch.Tensor:
    if w is None or w.dtype != torch.float32 or w.numel() != 3 or w.device != dev:
        raise hip.PodError("w: three fp32 weights on {} are needed with gradient planes".format(dev))
    return w.contiguous()


def train_loss_sums(cls, delta, cls_var, reg_var, labels, matched_gt, gt_boxes, anchors, num_anchors: int, num_classes: int, *,
                    box_weights=(1.0, 1.0, 1.0, 1.0), alpha: float = 0.25, gamma: float = 2.0, beta: float = 0.0, cls_samples: int = 0,
                    eps: Optional[torch.Tensor] = None, eps_out: Optional[torch.Tensor] = None, w: Optional[torch.Tensor] = None,
                    want_grads: bool = False, seed: int = 0, cov_dims: Optional[int] = None):
    """One pod_train_loss launch.  cls / delta / cls_var / reg_var: per-level lists of contiguous fp32 (N, A*C, H, W) planes (cls_var /
    reg_var None without that head).  Returns (sums double[4] = cls sum, standard regression sum, NLL regression sum, positives;
    grads = None or (g_cls, g_delta, g_cls_var, g_reg_var) per-level lists of d(w . sums[:3]) / d input)."""
    lib = hip.load()
    cfg, lv, a, gt = _launch_inputs(cls, delta, cls_var, reg_var, labels, matched_gt, gt_boxes, anchors, num_anchors, num_classes, box_weights,
                                    cls_samples, seed, cov_dims)
    L, n, dev, r, g = len(cls), int(cls[0].shape[0]), cls[0].device, int(a.shape[0]), int(gt.shape[0])
    S = int(cls_samples) if cls_var is not None else 0
    for name, t in (("eps", eps), ("eps_out", eps_out)):
        if t is not None and not (cls_var is not None and t.dtype == torch.float32 and t.is_contiguous() and t.device == dev
                                  and tuple(t.shape) == (S, n * r, num_classes)):
            raise hip.PodError("{}: expected contiguous fp32 {} on {} and a variance head".format(name, (S, n * r, num_classes), dev))
    grads = garr = None
    if want_grads:
        w = _weights_ok(w, dev)
        grads = ([torch.empty_like(t) for t in cls], [torch.empty_like(t) for t in delta],
                 None if cls_var is None else [torch.empty_like(t) for t in cls_var],
                 None if reg_var is None else [torch.empty_like(t) for t in reg_var])
        garr = (hip.PodLevelGrad * hip.POD_MAX_LEVELS)()
        for l in range(L):
            garr[l].cls, garr[l].delta = grads[0][l].data_ptr(), grads[1][l].data_ptr()
            garr[l].cls_var = None if grads[2] is None else grads[2][l].data_ptr()
            garr[l].reg_var = None if grads[3] is None else grads[3][l].data_ptr()
    n_part = int(lib.pod_train_loss_partials(cfg, lv))
    partials = torch.empty((max(n_part, 4),), dtype=torch.float64, device=dev)
    sums = torch.empty((4,), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        hip.check(lib.pod_train_loss(cfg, lv, garr, hip.ptr(labels), hip.ptr(matched_gt), hip.ptr(gt) if g else None, g, hip.ptr(a), r,
                                     float(alpha), float(gamma), float(beta), hip.ptr(eps), hip.ptr(eps_out), hip.ptr(w) if want_grads else None,
                                     hip.ptr(partials), hip.ptr(sums), hip.current_stream()), "pod_train_loss")
    return sums, grads


BBOX_COV_LOSSES = ("none", "negative_log_likelihood", "second_moment_matching", "energy_loss")      # BBOX_COV_LOSS.NAME
REG_SCORE_KINDS = {"second_moment_matching": hip.POD_REG_LOSS_MOMENTS, "energy_loss": hip.POD_REG_LOSS_ENERGY}
FULL_COV_KINDS = {"none": hip.POD_FULL_COV_NLL, "negative_log_likelihood": hip.POD_FULL_COV_NLL,          # COVARIANCE_TYPE: full (K28)
                  "second_moment_matching": hip.POD_FULL_COV_MOMENTS, "energy_loss": hip.POD_FULL_COV_ENERGY}


def _score_launch(entry: str, kind_id: int, kind: str, cls, delta, cls_var, reg_var, labels, matched_gt, gt_boxes, anchors, num_anchors, num_classes,
                  num_samples, box_weights, beta, cls_samples, eps_reg, eps_reg_out, w, grads, seed, energy: bool):
    """One launch of a covariance objective on the positive anchors, pod_reg_score_loss (K27) or pod_full_cov_loss (K28): the two take one
    argument list.  Returns (sum double[1], grads with the new reg_var planes in fourth place, or None)."""
    if reg_var is None:
        raise hip.PodError("{} needs the box covariance head (reg_var planes)".format(kind))
    lib = hip.load()
    cfg, lv, a, gt = _launch_inputs(cls, delta, cls_var, reg_var, labels, matched_gt, gt_boxes, anchors, num_anchors, num_classes, box_weights,
                                    cls_samples, seed, None)
    L, n, dev, r, g = len(cls), int(cls[0].shape[0]), cls[0].device, int(a.shape[0]), int(gt.shape[0])
    M = int(num_samples)
    for name, t in (("eps_reg", eps_reg), ("eps_reg_out", eps_reg_out)):
        if t is not None and not (energy and t.dtype == torch.float32 and t.is_contiguous() and t.device == dev
                                  and tuple(t.shape) == (M + 1, n * r, 4)):
            raise hip.PodError("{}: expected contiguous fp32 {} on {} and the energy loss".format(name, (M + 1, n * r, 4), dev))
    garr = None
    if grads is not None:
        w = _weights_ok(w, dev)
        g_reg_var = [torch.empty_like(t) for t in reg_var]
        grads = (grads[0], grads[1], grads[2], g_reg_var)
        garr = (hip.PodLevelGrad * hip.POD_MAX_LEVELS)()
        for l in range(L):
            if tuple(grads[1][l].shape) != tuple(delta[l].shape) or not grads[1][l].is_contiguous():
                raise hip.PodError("grads: delta plane {} is not laid out as delta[{}]".format(l, l))
            garr[l].delta, garr[l].reg_var = grads[1][l].data_ptr(), g_reg_var[l].data_ptr()
    n_part = int(getattr(lib, entry.replace("_loss", "_partials"))(cfg, lv))
    partials = torch.empty((max(n_part, 1),), dtype=torch.float64, device=dev)
    total = torch.empty((1,), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        hip.check(getattr(lib, entry)(cfg, lv, garr, hip.ptr(labels), hip.ptr(matched_gt), hip.ptr(gt) if g else None, g, hip.ptr(a), r,
                                      kind_id, M, float(beta), hip.ptr(eps_reg), hip.ptr(eps_reg_out),
                                      hip.ptr(w) if grads is not None else None, hip.ptr(partials), hip.ptr(total), hip.current_stream()), entry)
    return total, grads


def reg_score_sum(cls, delta, cls_var, reg_var, labels, matched_gt, gt_boxes, anchors, num_anchors: int, num_classes: int, *, kind: str,
                  num_samples: int = 1000, box_weights=(1.0, 1.0, 1.0, 1.0), beta: float = 0.0, cls_samples: int = 0,
                  eps_reg: Optional[torch.Tensor] = None, eps_reg_out: Optional[torch.Tensor] = None, w: Optional[torch.Tensor] = None,
                  grads=None, seed: int = 0):
    """One pod_reg_score_loss launch (K27): the `second_moment_matching` or `energy_loss` sum over the positive anchors, planes as
    train_loss_sums takes them.  grads: None, or train_loss_sums' planes of the SAME inputs and `w`, written earlier on this stream: the
    launch adds w[2] d sum / d delta to their delta planes in place, and the reg_var planes are allocated here.  eps_reg / eps_reg_out:
    the dense (num_samples + 1, N*R, 4) normals to replay / to receive the ones used (energy loss; tests and replay at small R only).
    Returns (sum double[1], grads with the new reg_var planes in fourth place, or None)."""
    if kind not in REG_SCORE_KINDS:
        raise ValueError("reg_score_sum: kind is one of {}, got {!r}".format(sorted(REG_SCORE_KINDS), kind))
    return _score_launch("pod_reg_score_loss", REG_SCORE_KINDS[kind], kind, cls, delta, cls_var, reg_var, labels, matched_gt, gt_boxes, anchors,
                         num_anchors, num_classes, num_samples, box_weights, beta, cls_samples, eps_reg, eps_reg_out, w, grads, seed,
                         kind == "energy_loss")


def full_cov_sum(cls, delta, cls_var, reg_var, labels, matched_gt, gt_boxes, anchors, num_anchors: int, num_classes: int, *, kind: str,
                 num_samples: int = 1000, box_weights=(1.0, 1.0, 1.0, 1.0), beta: float = 0.0, cls_samples: int = 0,
                 eps_reg: Optional[torch.Tensor] = None, eps_reg_out: Optional[torch.Tensor] = None, w: Optional[torch.Tensor] = None,
                 grads=None, seed: int = 0):
    """One pod_full_cov_loss launch (K28), as reg_score_sum is K27's: the sum the loss name `kind` selects for the FULL covariance head
    (reg_var planes of A * 10 channels) -- `none` / `negative_log_likelihood`: the Gaussian NLL, `second_moment_matching`, `energy_loss` --
    over the positive anchors.  Every argument and the result as reg_score_sum's; the reg_var planes allocated here have ten channels."""
    if kind not in FULL_COV_KINDS:
        raise ValueError("full_cov_sum: kind is one of {}, got {!r}".format(sorted(FULL_COV_KINDS), kind))
    return _score_launch("pod_full_cov_loss", FULL_COV_KINDS[kind], kind, cls, delta, cls_var, reg_var, labels, matched_gt, gt_boxes, anchors,
                         num_anchors, num_classes, num_samples, box_weights, beta, cls_samples, eps_reg, eps_reg_out, w, grads, seed,
                         kind == "energy_loss")


def covariance_route(bbox_cov_loss: str, num_anchors: int, reg_var_channels: Optional[int]):
    """Which launch evaluates the covariance term of loss_box_reg, from the loss name and the reg_var planes' channel count: (None, None)
    = pod_train_loss alone (no covariance head, or the diagonal head's NLL), else (the wrapper of the second launch, its kind).  A * 4
    channels: the diagonal head, today's paths; A * 10: the full covariance, every name through pod_full_cov_loss."""
    if bbox_cov_loss not in BBOX_COV_LOSSES:
        raise ValueError("Invalid regression loss name {!r}: BBOX_COV_LOSS.NAME is one of {}".format(bbox_cov_loss, ", ".join(BBOX_COV_LOSSES)))
    if reg_var_channels is None:
        return None, None
    if reg_var_channels == num_anchors * 4:
        return (reg_score_sum, bbox_cov_loss) if bbox_cov_loss in REG_SCORE_KINDS else (None, None)
    if reg_var_channels == num_anchors * 10:
        return full_cov_sum, bbox_cov_loss
    raise hip.PodError("reg_var planes of {} channels: {} anchor shapes have {} (COVARIANCE_TYPE diagonal) or {} (full)".format(
        reg_var_channels, num_anchors, num_anchors * 4, num_anchors * 10))


class _TrainLoss(torch.autograd.Function):
    """(loss_cls, loss_box_reg) = (w[0] cls_sum, w[1] std_reg_sum + w[2] cov_reg_sum), differentiable with respect to the per-level
    head tensors: forward is one pod_train_loss launch that also writes the gradient planes, backward scales them.  With
    `second_moment_matching` or `energy_loss`, and with the full covariance head under every name, the covariance sum and its gradients come
    from a second launch, pod_reg_score_loss or pod_full_cov_loss (`covariance_route`), on the planes the first one wrote without the
    reg_var head."""

    @staticmethod
    def forward(ctx, meta, w, *tensors):
        L, has_cv, has_rv = meta["levels"], meta["has_cls_var"], meta["has_reg_var"]
        ts = [t.detach().contiguous() for t in tensors]
        cls, delta = ts[:L], ts[L:2 * L]
        cls_var = ts[2 * L:3 * L] if has_cv else None
        reg_var = ts[(2 + has_cv) * L:(3 + has_cv) * L] if has_rv else None
        second, score = (meta.get("score_launch"), meta.get("score_kind")) if has_rv else (None, None)
        sums, grads = train_loss_sums(cls, delta, cls_var, None if second else reg_var, meta["labels"], meta["matched_gt"], meta["gt_boxes"],
                                      meta["anchors"], meta["num_anchors"], meta["num_classes"], box_weights=meta["box_weights"], alpha=meta["alpha"],
                                      gamma=meta["gamma"], beta=meta["beta"], cls_samples=meta["cls_samples"], eps=meta["eps"],
                                      eps_out=meta.get("eps_out"), w=w, want_grads=True, seed=meta["seed"])
        if second:
            total, grads = second(cls, delta, cls_var, reg_var, meta["labels"], meta["matched_gt"], meta["gt_boxes"], meta["anchors"],
                                  meta["num_anchors"], meta["num_classes"], kind=score, num_samples=meta["score_samples"],
                                  box_weights=meta["box_weights"], beta=meta["beta"], cls_samples=meta["cls_samples"],
                                  eps_reg=meta.get("eps_reg"), eps_reg_out=meta.get("eps_reg_out"), w=w, grads=grads, seed=meta["seed"])
            sums[2:3].copy_(total)
        ctx.meta = (L, has_cv, has_rv)
        ctx.planes = grads
        wd = w.double()
        meta["sums"] = sums
        loss_cls = (wd[0] * sums[0]).to(torch.float32)
        loss_reg = (wd[1] * sums[1] + wd[2] * sums[2]).to(torch.float32)
        return loss_cls, loss_reg

    @staticmethod
    def backward(ctx, g_cls, g_reg):
        L, has_cv, has_rv = ctx.meta
        p_cls, p_delta, p_cv, p_rv = ctx.planes
        out = [p * g_cls for p in p_cls] + [p * g_reg for p in p_delta]
        if has_cv:
            out += [p * g_cls for p in p_cv]
        if has_rv:
            out += [p * g_reg for p in p_rv]
        return (None, None) + tuple(out)


class ProbabilisticLosses:
    """The state and configuration ProbabilisticRetinaNet.losses reads (PR:49-50, PR:168-333; detectron2 RetinaNet's loss_normalizer = 100,
    momentum 0.9, focal alpha 0.25 / gamma 2.0, SMOOTH_L1_LOSS_BETA).  `loss_normalizer` lives on the device once the first call has
    updated it; `current_step` is the caller's to advance (the reference's forward does it after every call, PR:146)."""

    def __init__(self, num_classes: int = 7, cls_var_num_samples: int = 3, focal_loss_alpha: float = 0.25, focal_loss_gamma: float = 2.0,
                 smooth_l1_beta: float = 0.0, box_reg_weights=(1.0, 1.0, 1.0, 1.0), annealing_step: int = 80000, loss_normalizer: float = 100.0,
                 loss_normalizer_momentum: float = 0.9, seed: int = 0, bbox_cov_loss: str = "negative_log_likelihood",
                 bbox_cov_num_samples: int = 1000):
        if bbox_cov_loss not in BBOX_COV_LOSSES:          # PR:308-311
            raise ValueError("Invalid regression loss name {!r}: BBOX_COV_LOSS.NAME is one of {}".format(bbox_cov_loss, ", ".join(BBOX_COV_LOSSES)))
        self.bbox_cov_loss, self.bbox_cov_num_samples = bbox_cov_loss, int(bbox_cov_num_samples)
        self.num_classes, self.cls_var_num_samples = int(num_classes), int(cls_var_num_samples)
        self.focal_loss_alpha, self.focal_loss_gamma, self.smooth_l1_beta = float(focal_loss_alpha), float(focal_loss_gamma), float(smooth_l1_beta)
        self.box_reg_weights = tuple(float(x) for x in box_reg_weights)
        self.annealing_step, self.current_step = annealing_step, 0
        self.loss_normalizer, self.loss_normalizer_momentum = loss_normalizer, float(loss_normalizer_momentum)
        self.seed, self.draws = int(seed), 0
        self.last_sums = None          # device double[4] of the last call: cls sum, standard / covariance regression sums, positives

    def weights(self, normalizer: torch.Tensor, has_cls_var: bool, has_reg_var: bool) -> torch.Tensor:
        """Device float[3]: what multiplies the three sums (PR:268 / 282, PR:307, 319-322, 331)."""
        norm = torch.clamp(normalizer.to(torch.float64), min=1.0)
        lam = annealing_weight(self.current_step, self.annealing_step) if has_reg_var else 0.0
        s = float(self.cls_var_num_samples) if has_cls_var else 1.0
        return (torch.tensor([1.0 / s, 1.0 - lam, lam], dtype=torch.float64, device=norm.device) / norm).to(torch.float32)

    def __call__(self, head_outputs, labels: torch.Tensor, matched_gt: torch.Tensor, gt_boxes: torch.Tensor, anchors=None,
                 eps: Optional[torch.Tensor] = None, normalizer=None, eps_out: Optional[torch.Tensor] = None,
                 eps_reg: Optional[torch.Tensor] = None, eps_reg_out: Optional[torch.Tensor] = None):
        """head_outputs: synthetic.HeadOutputs whose tensors are (N images, A*C, H, W); labels / matched_gt: `label_anchors`' (N, R);
        gt_boxes: the concatenated (G, 4) boxes matched_gt indexes; anchors: default head_outputs.anchors.  eps: None (in-kernel draws,
        fresh on every call) or the dense (S, N*R, K) normals to replay.  normalizer: None = the reference's moving average (PR:201-203,
        updated here from the labels' positives, on the device), else the number or device scalar to divide by (max(1, .)).  eps_reg /
        eps_reg_out: the energy loss's dense (M + 1, N*R, 4) normals, as eps / eps_out (reg_score_sum).  With the covariance head, the
        covariance term of loss_box_reg is the one `bbox_cov_loss` names ("none": the NLL, as for every head with reg_var planes); reg_var
        planes of A * 10 channels are the full covariance (K28, `covariance_route`), any count but A * 4 and A * 10 raises."""
        ho = head_outputs
        dev = ho.cls[0].device
        K = self.num_classes
        if ho.num_classes != K:
            raise hip.PodError("head outputs have {} classes, the losses were built for {}".format(ho.num_classes, K))
        if normalizer is None:
            num_pos = ((labels >= 0) & (labels != K)).sum().to(torch.float64)
            prev = self.loss_normalizer if torch.is_tensor(self.loss_normalizer) else torch.tensor(float(self.loss_normalizer), dtype=torch.float64, device=dev)
            self.loss_normalizer = self.loss_normalizer_momentum * prev + (1 - self.loss_normalizer_momentum) * torch.clamp(num_pos, min=1.0)
            norm = self.loss_normalizer
        else:
            norm = normalizer.to(dev) if torch.is_tensor(normalizer) else torch.tensor(float(normalizer), device=dev)
        has_cv, has_rv = ho.cls_var is not None, ho.reg_var is not None
        w = self.weights(norm, has_cv, has_rv)
        second, score = covariance_route(self.bbox_cov_loss, ho.num_anchors, int(ho.reg_var[0].shape[1]) if has_rv else None)
        meta = dict(levels=len(ho.cls), has_cls_var=int(has_cv), has_reg_var=int(has_rv), labels=labels, matched_gt=matched_gt, gt_boxes=gt_boxes,
                    anchors=ho.anchors if anchors is None else anchors, num_anchors=ho.num_anchors, num_classes=K, box_weights=self.box_reg_weights,
                    alpha=self.focal_loss_alpha, gamma=self.focal_loss_gamma, beta=self.smooth_l1_beta, cls_samples=self.cls_var_num_samples,
                    eps=eps, eps_out=eps_out, seed=(self.seed & 0xFFFFFFFF) | ((self.draws & 0xFFFFFFFF) << 32),
                    score_launch=second, score_kind=score, score_samples=self.bbox_cov_num_samples,
                    eps_reg=eps_reg, eps_reg_out=eps_reg_out)
        self.draws += 1
        tensors = list(ho.cls) + list(ho.delta) + (list(ho.cls_var) if has_cv else []) + (list(ho.reg_var) if has_rv else [])
        loss_cls, loss_reg = _TrainLoss.apply(meta, w, *tensors)
        self.last_sums = meta["sums"]
        return {"loss_cls": loss_cls, "loss_box_reg": loss_reg}


def stack_head_outputs(outs: List) -> "object":
    """Single-image HeadOutputs (one run each) of ONE frame size -> one HeadOutputs whose leading dimension is the image."""
    from .synthetic import HeadOutputs
    o = outs[0]
    cat = lambda name: None if getattr(o, name) is None else [torch.cat([getattr(x, name)[l][:1] for x in outs]).contiguous() for l in range(len(o.cls))]
    return HeadOutputs(cat("cls"), cat("delta"), cat("cls_var"), cat("reg_var"), o.anchors, o.shapes, o.num_anchors, o.num_classes, o.image_size)
