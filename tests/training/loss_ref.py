"""fp64 torch restatement of the anchor labelling and of the training losses: the referee of the K21 tests.

Written from the public definitions (detectron2 Matcher / RetinaNet.label_anchors / Box2BoxTransform.get_deltas, fvcore's
sigmoid_focal_loss and smooth_l1_loss) and from what PR:168-333 does with them; tests/training/test_losses_cpu.py holds it against the
fixture the reference itself produced (tools/make_golden_loss.py).  The IoU is evaluated in fp32, in the kernel's operation order, so
that labels can be compared exactly; everything else is fp64 and differentiable."""
import json
import os

import numpy as np
import torch

from pod_compare_amd import anchors as _anchors, synthetic

FIXTURE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "golden", "train_loss_r1161.npz")
FAR_BOX = [5000.0, 5000.0, 5010.0, 5012.0]          # wholly off every anchor's reach: its best IoU is 0


def load_fixture():
    with np.load(FIXTURE, allow_pickle=False) as z:
        fx = {k: z[k] for k in z.files}
    fx["meta"] = json.loads(str(fx["meta"]))
    return fx


def iou_matrix(gt_boxes, anchors):
    """(G, R) fp32: inter / ((area_gt + area_anchor) - inter) if inter > 0 else 0."""
    g, a = gt_boxes.float(), anchors.float()
    wh = (torch.min(g[:, None, 2:], a[None, :, 2:]) - torch.max(g[:, None, :2], a[None, :, :2])).clamp(min=0)
    inter = wh[..., 0] * wh[..., 1]
    area_g = (g[:, 2] - g[:, 0]) * (g[:, 3] - g[:, 1])
    area_a = (a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1])
    return torch.where(inter > 0, inter / ((area_g[:, None] + area_a[None, :]) - inter), torch.zeros_like(inter))


def label_anchors(anchors, gt_boxes, gt_classes, num_classes, lo=0.4, hi=0.5):
    """One image -> dict(labels (R,) int64, matched (R,) int64 first arg-max or -1, unique (R,) bool: the maximum is reached once,
    match (R,) the Matcher's label before / after promotion, num_pos)."""
    r = anchors.shape[0]
    if gt_boxes.shape[0] == 0:
        return dict(labels=torch.full((r,), num_classes, dtype=torch.int64), matched=torch.full((r,), -1, dtype=torch.int64),
                    unique=torch.zeros(r, dtype=torch.bool), promoted=torch.zeros(r, dtype=torch.bool), by_threshold=torch.zeros(r, dtype=torch.int64), num_pos=0)
    q = iou_matrix(gt_boxes, anchors)
    v = q.max(dim=0).values
    hit = q == v[None, :]
    m = torch.argmax(hit.to(torch.int8), dim=0)                # first maximum = lowest box index
    lo32, hi32 = torch.tensor(lo, dtype=torch.float32), torch.tensor(hi, dtype=torch.float32)
    by_thr = torch.where(v >= hi32, 1, torch.where(v >= lo32, -1, 0))
    promoted = (q == q.max(dim=1, keepdim=True).values).any(dim=0)
    match = torch.where(promoted, torch.ones_like(by_thr), by_thr)
    labels = torch.where(match == 1, gt_classes.long()[m], torch.where(match == 0, torch.full_like(m, num_classes), torch.full_like(m, -1)))
    return dict(labels=labels, matched=m, unique=hit.sum(dim=0) == 1, promoted=promoted & (by_thr != 1), by_threshold=by_thr,
                num_pos=int(((labels >= 0) & (labels < num_classes)).sum()))


def get_deltas(src, tgt, weights=(1.0, 1.0, 1.0, 1.0)):
    sw, sh = src[..., 2] - src[..., 0], src[..., 3] - src[..., 1]
    scx, scy = src[..., 0] + 0.5 * sw, src[..., 1] + 0.5 * sh
    tw, th = tgt[..., 2] - tgt[..., 0], tgt[..., 3] - tgt[..., 1]
    tcx, tcy = tgt[..., 0] + 0.5 * tw, tgt[..., 1] + 0.5 * th
    return torch.stack((weights[0] * (tcx - scx) / sw, weights[1] * (tcy - scy) / sh, weights[2] * torch.log(tw / sw), weights[3] * torch.log(th / sh)), dim=-1)


def focal(x, t, alpha, gamma):
    p = torch.sigmoid(x)
    ce = torch.nn.functional.binary_cross_entropy_with_logits(x, t, reduction="none")
    p_t = p * t + (1 - p) * (1 - t)
    loss = ce * (1 - p_t) ** gamma
    return (alpha * t + (1 - alpha) * (1 - t)) * loss if alpha >= 0 else loss


def smooth_l1(d, beta):
    n = d.abs()
    return n if beta < 1e-5 else torch.where(n < beta, 0.5 * n ** 2 / beta, n - 0.5 * beta)


def loss_sums(cls, delta, cls_var, reg_var, labels, matched_boxes, anchors, num_classes, eps=None, alpha=0.25, gamma=2.0, beta=0.0,
              weights=(1.0, 1.0, 1.0, 1.0)):
    """cls (N, R, K), delta (N, R, 4), cls_var / reg_var like them or None: fp64.  labels (N, R) int64, matched_boxes (N, R, 4) (any box where
    the label is not a class), anchors (R, 4), eps (S, N*R, K) dense by anchor.  Returns (cls sum, standard regression sum, NLL sum, positives)."""
    valid = labels >= 0
    pos = valid & (labels != num_classes)
    target = torch.nn.functional.one_hot(labels.clamp(min=0), num_classes + 1)[..., :-1].double()
    if cls_var is None:
        cls_sum = focal(cls, target, alpha, gamma)[valid].sum()
    else:
        std = torch.sqrt(torch.exp(cls_var))
        z = cls[None] + std[None] * eps.double().view(eps.shape[0], *cls.shape)
        cls_sum = focal(z, target[None].expand_as(z), alpha, gamma)[:, valid].sum()
    tgt = get_deltas(anchors.double()[None].expand_as(matched_boxes)[pos], matched_boxes.double()[pos], weights)
    sl = smooth_l1(delta[pos] - tgt, beta)
    std_sum = sl.sum()
    nll_sum = torch.zeros((), dtype=torch.float64)
    if reg_var is not None:
        c = torch.clamp(reg_var[pos], -7.0, 7.0)
        nll_sum = (0.5 * torch.exp(-c) * sl + 0.5 * c).sum()
    return cls_sum, std_sum, nll_sum, int(pos.sum())


def annealing_lambda(step, anneal):
    return (100 ** min(1.0, step / anneal) - 1.0) / (100.0 - 1.0)


def scatter_eps(compact, valid):
    """The reference's (S, valid anchors, K) normals -> dense (S, N*R, K), zeros at the ignored anchors."""
    compact = torch.as_tensor(compact)
    dense = torch.zeros((compact.shape[0], valid.numel(), compact.shape[2]), dtype=compact.dtype)
    dense[:, valid.reshape(-1)] = compact
    return dense


def to_planes(x, shapes, num_anchors):
    """(N, R, C) level-concatenated anchor-major -> per-level (N, A*C, H, W) planes."""
    out, base = [], 0
    for h, w in shapes:
        n = h * w * num_anchors
        out.append(synthetic.nchw_from_anchor_major(x[:, base:base + n].contiguous(), h, w, num_anchors))
        base += n
    return out


def from_planes(planes, c):
    return torch.cat([synthetic.anchor_major_from_nchw(p, c) for p in planes], dim=1)


def fixture_geometry(fx):
    shapes = [tuple(s) for s in fx["meta"]["shapes"]]
    anchors = _anchors.grid_anchors(shapes)
    assert np.array_equal(torch.cat(anchors).numpy(), fx["anchors"])
    return shapes, anchors
