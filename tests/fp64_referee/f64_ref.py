"""The fp64 referee of the box arithmetic: candidate decode + moments, the cluster merges, finalize.

A restatement of the arithmetic of oracle/pod_oracle.py AFTER its discrete decisions, with the number format as a parameter:
every function computes in the dtype of the tensors it is handed (torch.float32 or torch.float64; numpy's matching dtype in the
LAPACK part).  At float32 it is the oracle's own sequence of torch / numpy calls on the same shapes, so it reproduces the oracle
bit for bit (tests/fp64_referee/test_f64_referee_cpu.py pins that on every predictor fixture); at float64 the same sequence is
the bar both the fp32 oracle and the HIP kernels are measured against (profiles/fp64_referee.md).

Inputs are the fp32 tensors both sides read (head planes -- in MC modes the fp32 merged planes, which K1 reproduces bit for bit --
anchors, replayed normals), converted ONCE to the dtype.  Every discrete decision is an argument and is never recomputed here:
the per-level top-k index sequences, the NMS keep list, the cluster membership rows, the same-class masks, the non-empty mask.
`oracle_run` / `oracle_run_post_nms` collect them from an fp32 oracle run, stage by stage.
"""
import math
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from oracle import pod_oracle as po          # the DECISIONS' source (and the fp32 side of every comparison); no arithmetic is taken from it

SCALE_CLAMP = math.log(1000.0 / 16)


# ---------------------------------------------------------------------------------------------------------------------------
# candidate stage
# ---------------------------------------------------------------------------------------------------------------------------

def merge_planes(xs: Sequence[torch.Tensor], quirk: bool) -> torch.Tensor:
    """The fp32 run merge (x0 twice and the last run never under the quirk; one divide).  An INPUT of the referee: K1's planes are
    held bit-equal to it by test_dense_merge_planes_equal_reference_merge, so both sides read these fp32 values."""
    acc = xs[0]
    for i in (range(0, len(xs) - 1) if quirk else range(1, len(xs))):
        acc = acc + xs[i]
    return acc / len(xs)


def _centre_form(anchors):
    w = anchors[:, 2] - anchors[:, 0]
    h = anchors[:, 3] - anchors[:, 1]
    return w, h, anchors[:, 0] + 0.5 * w, anchors[:, 1] + 0.5 * h


def _apply(deltas, w, h, cx, cy, weights):
    """dx, dy shift the centre by a fraction of the anchor's size; dw, dh (clamped) scale it.  `deltas`: (n,4[,S]), w..cy: (n[,S])."""
    wx, wy, ww, wh = weights
    dx, dy = deltas[:, 0::4] / wx, deltas[:, 1::4] / wy
    dw = torch.clamp(deltas[:, 2::4] / ww, max=SCALE_CLAMP)
    dh = torch.clamp(deltas[:, 3::4] / wh, max=SCALE_CLAMP)
    pcx, pcy = dx * w[:, None] + cx[:, None], dy * h[:, None] + cy[:, None]
    pw, ph = torch.exp(dw) * w[:, None], torch.exp(dh) * h[:, None]
    return pcx - 0.5 * pw, pcy - 0.5 * ph, pcx + 0.5 * pw, pcy + 0.5 * ph


def decode_boxes(deltas: torch.Tensor, anchors: torch.Tensor, weights=(1.0, 1.0, 1.0, 1.0)) -> torch.Tensor:
    """(n,4) deltas against (n,4) anchors: the deterministic decode."""
    x1, y1, x2, y2 = _apply(deltas, *_centre_form(anchors), weights)
    return torch.stack((x1, y1, x2, y2), dim=-1).reshape(deltas.shape)


def decode_sample_boxes(deltas: torch.Tensor, anchors: torch.Tensor, weights=(1.0, 1.0, 1.0, 1.0)) -> torch.Tensor:
    """(n,4,S) sampled deltas against (n,4,S) anchors."""
    out = torch.zeros_like(deltas)
    out[:, 0::4, :], out[:, 1::4, :], out[:, 2::4, :], out[:, 3::4, :] = _apply(deltas, *_centre_form(anchors), weights)
    return out


def cholesky_from_head(reg_var: torch.Tensor) -> torch.Tensor:
    """diag sqrt(exp(.)); with D = 10 the strict lower triangle in tril_indices(4,4,-1) order."""
    chol = torch.diag_embed(torch.sqrt(torch.exp(reg_var[:, 0:4])))
    if reg_var.shape[1] > 4:
        ti = torch.tril_indices(row=4, col=4, offset=-1)
        chol[:, ti[0], ti[1]] = reg_var[:, 4:]
    return chol


def mean_covariance(samples):
    """Mean over the sample axis and the unbiased two-pass covariance.  `samples`: (n,k,S), or a list of S (n,k) tensors.
    Returns (mean (n,k), cov (n,k,k), residual outer-product sum (n,k,k))."""
    if not isinstance(samples, torch.Tensor):
        samples = torch.stack(list(samples), 2)
    s = samples.shape[2]
    mean = torch.mean(samples, 2, keepdim=True)
    res = torch.transpose(torch.unsqueeze(samples - mean, 1), 1, 3)
    rss = torch.sum(torch.matmul(res, torch.transpose(res, 3, 2)), 1)
    return mean.squeeze(2), rss / (s - 1), rss


@dataclass
class LevelInputs:
    """One pyramid level, fp32, anchor-major: what the candidate stage reads."""
    delta: torch.Tensor                          # (R,4): the (merged) box deltas
    anchors: torch.Tensor                        # (R,4)
    reg_var: Optional[torch.Tensor] = None       # (R,D): the (merged) box log-variances / Cholesky entries
    run_delta: Optional[List[torch.Tensor]] = None   # per run (R,4): present when there is an epistemic part


def level_inputs(outputs: Optional[Dict], run_outputs: Optional[Sequence[Dict]], quirk: bool) -> List[LevelInputs]:
    """From the reference-layout dicts the oracle takes (pod_compare_amd.synthetic.to_reference_layout)."""
    src = outputs if run_outputs is None else run_outputs[0]
    out = []
    for lvl, anchors in enumerate(src["anchors"]):
        if run_outputs is None:
            pick = lambda key: None if src[key] is None else src[key][lvl][0]
            out.append(LevelInputs(pick("box_delta"), anchors, pick("box_reg_var")))
        else:
            merged = lambda key: None if src[key] is None else merge_planes([ro[key][lvl] for ro in run_outputs], quirk)[0]
            out.append(LevelInputs(merged("box_delta"), anchors, merged("box_reg_var"), [ro["box_delta"][lvl][0] for ro in run_outputs]))
    return out


@dataclass
class Candidates:
    boxes: torch.Tensor                          # (n,4)
    cov: Optional[torch.Tensor]                  # (n,4,4) or None
    # intermediates, for localising a failure stage by stage
    aleatoric: Optional[torch.Tensor] = None     # sample covariance alone
    epistemic: Optional[torch.Tensor] = None     # covariance over the runs' decoded boxes
    residual_sum: Optional[torch.Tensor] = None  # sum over samples of the residuals' outer products (before / (S-1))
    run_mean: Optional[torch.Tensor] = None      # mean over the runs' decoded boxes
    samples: Optional[torch.Tensor] = None       # (n,4,S) decoded samples, when asked for


def candidate_stage(levels: Sequence[LevelInputs], tops: Sequence[torch.Tensor], eps_prop: Optional[torch.Tensor], dtype,
                    weights=(1.0, 1.0, 1.0, 1.0), keep_samples: bool = False) -> Candidates:
    """From `delta = delta[top]` on.  tops[l]: the level's selected anchor indices, in candidate order (a decision).
    eps_prop: (S,n,4) fp32 normals (required when the head has reg_var and n > 0)."""
    cv = lambda t: t.to(dtype)
    lv_delta, lv_chol, lv_anchor, lv_epi, lv_rmean = [], [], [], [], []
    for lv, top in zip(levels, tops):
        anc = cv(lv.anchors)[top]
        lv_delta.append(cv(lv.delta)[top])
        lv_anchor.append(anc)
        lv_chol.append(None if lv.reg_var is None else cholesky_from_head(cv(lv.reg_var)[top]))
        if lv.run_delta is not None:
            rmean, epi, _ = mean_covariance([decode_boxes(cv(rd)[top], anc, weights) for rd in lv.run_delta])
            lv_epi.append(epi)
            lv_rmean.append(rmean)
    delta, anchors = torch.cat(lv_delta), torch.cat(lv_anchor)
    epi = torch.cat(lv_epi) if lv_epi else None
    rmean = torch.cat(lv_rmean) if lv_rmean else None
    n = delta.shape[0]
    if lv_chol[0] is None:
        return Candidates(decode_boxes(delta, anchors, weights), epi, None, epi, None, rmean)
    if n == 0:
        return Candidates(torch.zeros((0, 4), dtype=dtype), torch.zeros((0, 4, 4), dtype=dtype))
    chol = torch.cat(lv_chol)
    eps = cv(eps_prop)
    s = eps.shape[0]
    draws = delta + torch.matmul(chol, eps.unsqueeze(-1)).squeeze(-1)
    draws = torch.transpose(torch.transpose(draws, 0, 1), 1, 2)
    anc_s = torch.repeat_interleave(anchors.unsqueeze(2), s, dim=2)
    samples = decode_sample_boxes(draws, anc_s, weights)
    boxes, ale, rss = mean_covariance(samples)
    return Candidates(boxes, ale if epi is None else ale + epi, ale, epi, rss, rmean, samples if keep_samples else None)


# ---------------------------------------------------------------------------------------------------------------------------
# cluster stage
# ---------------------------------------------------------------------------------------------------------------------------

def iou_matrix(b1: torch.Tensor, b2: torch.Tensor) -> torch.Tensor:
    """Pairwise IoU (intersection > 0 guard, no +1) in the tensors' dtype: the planted tests' precondition is stated on it."""
    area = lambda b: (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    wh = (torch.min(b1[:, None, 2:], b2[:, 2:]) - torch.max(b1[:, None, :2], b2[:, :2])).clamp(min=0)
    inter = wh.prod(dim=2)
    return torch.where(inter > 0, inter / (area(b1)[:, None] + area(b2) - inter), torch.zeros(1, dtype=inter.dtype))


def bayes_fuse(means: np.ndarray, covs: np.ndarray, mode: str):
    """Product of Gaussians ("bayesian_inference") or covariance intersection; LAPACK in the arrays' dtype."""
    precs = np.linalg.inv(covs)
    if mode == "bayesian_inference":
        fused_cov = np.linalg.inv(precs.sum(0))
        fused_mean = np.matmul(precs, np.expand_dims(means, 2)).sum(0)
        fused_mean = np.squeeze(np.matmul(fused_cov, fused_mean))
    elif mode == "covariance_intersection":
        total = precs.sum(0)
        rest = total - precs
        d_i, d_tot, d_rest = np.linalg.det(precs), np.linalg.det(total), np.linalg.det(rest)
        omega = (d_tot - d_rest + d_i) / (precs.shape[0] * d_tot + (d_i - d_rest).sum(0))
        wp = np.expand_dims(omega, (1, 2)) * precs
        fused_cov = np.linalg.inv(wp.sum(0))
        fused_mean = np.matmul(fused_cov, np.matmul(wp, np.expand_dims(means, 2)).sum(0))
    else:
        raise ValueError("unknown box merge mode {}".format(mode))
    return fused_mean, fused_cov


@dataclass
class Merged:
    """Cluster-stage output rows (before finalize)."""
    boxes: torch.Tensor
    cov: torch.Tensor
    probs: torch.Tensor
    scores: torch.Tensor


@dataclass
class Decisions:
    """What the fp32 oracle run decided (pre-NMS modes)."""
    tops: List[torch.Tensor]                     # per level: selected anchor indices, candidate order
    keep: torch.Tensor                           # NMS keep list into the candidates, truncated to max_detections
    member: Optional[torch.Tensor] = None        # (len(keep), n) bool: IoU with the centre > affinity_thresh
    same: Optional[List[torch.Tensor]] = None    # per centre: bool over ITS MEMBERS, the same-class mask
    nonempty: Optional[torch.Tensor] = None      # (rows before finalize,) bool


def standard_nms_stage(boxes, cov, probs, scores, keep) -> Merged:
    c = cov[keep] if cov is not None else torch.zeros(boxes[keep].shape + (4,), dtype=boxes.dtype)
    return Merged(boxes[keep], c, probs[keep], scores[keep])


def bayes_od_stage(boxes, cov, probs, scores, d: Decisions, box_merge_mode: str, cls_merge_mode: str) -> Merged:
    out_b, out_c, out_p = [], [], []
    for row, same, centre in zip(d.member, d.same, d.keep):
        grp_pv = probs[row]
        out_p.append(grp_pv.mean(0).unsqueeze(0) if cls_merge_mode == "bayesian_inference" else probs[centre].unsqueeze(0))
        mu, c = bayes_fuse(boxes[row, :][same].numpy(), cov[row, :][same].numpy(), box_merge_mode)
        out_b.append(torch.from_numpy(np.squeeze(mu)))
        out_c.append(torch.from_numpy(c))
    if cls_merge_mode == "bayesian_inference":
        pv = torch.cat(out_p, 0)
        score = torch.max(pv, 1)[0]
    else:
        pv, score = probs[d.keep], scores[d.keep]
    return Merged(torch.stack(out_b, 0), torch.stack(out_c, 0), pv, score)


def anchor_statistics_stage(boxes, cov, probs, d: Decisions) -> Merged:
    """Per centre with >= 2 IoU members: mean, unbiased covariance of the same-class members' boxes (+ the mean of their
    covariances); otherwise the centre's own row (1e-4 I when there are no candidate covariances)."""
    has_cov = cov is not None and len(cov) > 0
    out_b, out_c, out_p = [], [], []
    for row, same, centre in zip(d.member, d.same, d.keep):
        if row.sum(0) >= 2:
            grp = boxes[row, :][same, :]
            mu = grp.mean(0)
            res = (grp - mu).unsqueeze(2)
            c = torch.sum(torch.matmul(res, torch.transpose(res, 2, 1)), 0) / max((grp.shape[0] - 1), 1.0)
            if has_cov:
                c = c + cov[row, :][same, :].mean(0)
            pv = probs[row, :][same, :].mean(0)
        else:
            mu, pv = boxes[centre], probs[centre]
            c = cov[centre] if has_cov else 1e-4 * torch.eye(4, 4, dtype=boxes.dtype)
        out_b.append(mu); out_c.append(c); out_p.append(pv)
    pv = torch.stack(out_p, 0)
    return Merged(torch.stack(out_b, 0), torch.stack(out_c, 0), pv, torch.max(pv, 1)[0])


def ensembles_stage(boxes, cov, probs, clusters: Sequence[torch.Tensor], keep2: torch.Tensor) -> Merged:
    """Black-box (post-NMS) ensemble merge: per cluster (index lists, a decision) the members' moments, then the second NMS's keep."""
    out_b, out_c, out_p = [], [], []
    for idx in clusters:
        grp, grp_cov = boxes[idx], cov[idx]
        if grp.shape[0] >= 2:
            mu = grp.mean(0)
            res = (grp - mu).unsqueeze(2)
            c = torch.sum(torch.matmul(res, torch.transpose(res, 2, 1)), 0) / (grp.shape[0] - 1)
            c = c + grp_cov.mean(0)
        else:
            mu, c = grp.mean(0), grp_cov.mean(0)
        out_b.append(mu); out_c.append(c); out_p.append(probs[idx].mean(0))
    pv = torch.stack(out_p, 0)
    score = torch.max(pv, 1)[0]
    return Merged(torch.stack(out_b, 0)[keep2], torch.stack(out_c, 0)[keep2], pv[keep2], score[keep2])


# ---------------------------------------------------------------------------------------------------------------------------
# finalize
# ---------------------------------------------------------------------------------------------------------------------------

def scale_clip(boxes: torch.Tensor, image_size, out_size) -> torch.Tensor:
    sx, sy = out_size[1] / image_size[1], out_size[0] / image_size[0]
    b = boxes.clone()
    b[:, 0::2] *= sx
    b[:, 1::2] *= sy
    return torch.stack((b[:, 0].clamp(min=0, max=out_size[1]), b[:, 1].clamp(min=0, max=out_size[0]),
                        b[:, 2].clamp(min=0, max=out_size[1]), b[:, 3].clamp(min=0, max=out_size[0])), dim=-1)


def nonempty_fp32(boxes32: torch.Tensor, image_size, out_size) -> torch.Tensor:
    """The non-empty mask as the fp32 run decides it."""
    assert boxes32.dtype == torch.float32
    b = scale_clip(boxes32, image_size, out_size)
    return ((b[:, 2] - b[:, 0]) > 0.0) & ((b[:, 3] - b[:, 1]) > 0.0)


def finalize(m: Merged, image_size, out_size, nonempty: torch.Tensor) -> Merged:
    """Scale to the output resolution, clip, drop the empty rows (a decision), cov + 1e-4 I, S cov S^T."""
    dtype = m.boxes.dtype
    sx, sy = out_size[1] / image_size[1], out_size[0] / image_size[0]
    b = scale_clip(m.boxes, image_size, out_size)
    cov = m.cov[nonempty] + 1e-4 * torch.eye(4, dtype=dtype)
    smat = torch.diag_embed(torch.as_tensor((sx, sy, sx, sy), dtype=dtype)).unsqueeze(0)
    smat = torch.repeat_interleave(smat, cov.shape[0], 0)
    cov = torch.matmul(torch.matmul(smat, cov), torch.transpose(smat, 2, 1))
    return Merged(b[nonempty], cov, m.probs[nonempty], m.scores[nonempty])


def cov_xyxy_to_xywh(cov: torch.Tensor) -> torch.Tensor:
    """T cov T^T with T taking (x1,y1,x2,y2) to (x1,y1,w,h)."""
    t = torch.as_tensor([[1.0, 0, 0, 0], [0, 1.0, 0, 0], [-1.0, 0, 1.0, 0], [0, -1.0, 0, 1.0]], dtype=cov.dtype).unsqueeze(0)
    t = torch.repeat_interleave(t, cov.shape[0], 0)
    return torch.matmul(torch.matmul(t, cov), torch.transpose(t, 2, 1))


# ---------------------------------------------------------------------------------------------------------------------------
# the fp32 oracle run and its decisions; the referee chained over them
# ---------------------------------------------------------------------------------------------------------------------------

def split_tops(aw: po.Anchorwise) -> List[torch.Tensor]:
    return list(torch.split(aw.anchor_idx, aw.level_counts))


def cluster_decisions(mode: str, boxes32, probs32, classes, keep, p: po.PathParams):
    """Membership rows and same-class masks from fp32 candidate rows (bayes_od: argmax of the probability vectors; anchor
    statistics: the candidates' classes)."""
    member = po.iou_matrix(boxes32[keep], boxes32) > p.affinity_thresh
    if mode == "bayes_od":
        cls_of = probs32.max(1)[1]
        same = [cls_of[row] == cls_of[c] for row, c in zip(member, keep)]
    else:
        same = [classes[row] == classes[c] for row, c in zip(member, keep)]
    return member, same


@dataclass
class OracleRun:
    """One fp32 oracle run, stage by stage, with what it decided."""
    aw: List[po.Anchorwise]                      # one per member (post-NMS) or a single one
    pre: po.Detections                           # before finalize
    det: po.Detections                           # final
    eps_prop: List[Optional[torch.Tensor]]       # per aw: the (S,n,4) normals it drew, or None
    decisions: List[Decisions]                   # per aw (post-NMS: tops + keep only)
    nonempty: torch.Tensor = None
    clusters: Optional[List[torch.Tensor]] = None    # post-NMS: member index lists
    keep2: Optional[torch.Tensor] = None             # post-NMS: the second NMS's keep


def _anchorwise(outputs, run_outputs, p, eps_fn):
    rec = po.RecordEps(eps_fn)
    aw = po.anchorwise_inference(outputs, p, run_outputs, rec)
    src = outputs if run_outputs is None else run_outputs[0]
    eps_prop = rec.tensors[-1] if src["box_reg_var"] is not None and aw.boxes.shape[0] > 0 else None
    return aw, eps_prop


def oracle_run(mode: str, p: po.PathParams, image_size, out_size, *, outputs=None, run_outputs=None, eps_fn,
               box_merge_mode="bayesian_inference", cls_merge_mode="max_score") -> OracleRun:
    """po.predict in its stages (the same calls in the same order), keeping what it decided on the way."""
    aw, eps_prop = _anchorwise(outputs, run_outputs, p, eps_fn)
    d = Decisions(split_tops(aw), None)
    if mode in ("standard_nms", "mc_dropout_ensembles", "ensembles"):
        pre = po.standard_nms_post(aw, image_size, p)
    elif mode == "anchor_statistics":
        pre = po.anchor_statistics_post(aw, image_size, p)
    elif mode == "bayes_od":
        pre = po.bayes_od_post(aw, image_size, p, box_merge_mode, cls_merge_mode) if aw.boxes.shape[0] else \
            po._empty_detections(image_size, p.num_classes)
    else:
        raise ValueError(mode)
    d.keep = pre.keep
    if mode in ("anchor_statistics", "bayes_od"):
        d.member, d.same = cluster_decisions(mode, aw.boxes, aw.probs, aw.classes, pre.keep, p)
    ok = nonempty_fp32(pre.pred_boxes, image_size, out_size)
    d.nonempty = ok
    return OracleRun([aw], pre, po.finalize(pre, out_size[0], out_size[1]), [eps_prop], [d], ok)


def oracle_run_post_nms(p: po.PathParams, image_size, out_size, member_outputs, eps_fn) -> OracleRun:
    """po.predict_post_nms_ensemble in its stages."""
    aws, epss, ds, dets = [], [], [], []
    for o in member_outputs:
        aw, eps_prop = _anchorwise(o, None, p, eps_fn)
        det = po.standard_nms_post(aw, image_size, p)
        aws.append(aw); epss.append(eps_prop); dets.append(det); ds.append(Decisions(split_tops(aw), det.keep))
    pre = po.black_box_ensembles_post([x.pred_boxes for x in dets], [x.pred_classes for x in dets], [x.pred_cls_probs for x in dets],
                                      [x.pred_boxes_covariance for x in dets], image_size, p)
    boxes, classes = torch.cat([x.pred_boxes for x in dets]), torch.cat([x.pred_classes for x in dets])
    iou = po.iou_matrix(boxes, boxes)
    clusters, taken = [], torch.zeros(boxes.shape[0], dtype=torch.bool)
    for i in range(boxes.shape[0]):          # the greedy sweep in index order (index 0 always seeds)
        if i != 0 and taken[i]:
            continue
        idx = torch.where((iou[i, :] >= p.affinity_thresh) & (classes == classes[i]))[0]
        clusters.append(idx)
        taken[idx] = True
    ok = nonempty_fp32(pre.pred_boxes, image_size, out_size)
    return OracleRun(aws, pre, po.finalize(pre, out_size[0], out_size[1]), epss, ds, ok, clusters, pre.keep)


@dataclass
class Chain:
    """The referee's evaluation of one run, every stage in one dtype."""
    cand: List[Candidates]
    pre: Merged
    det: Merged


def referee_chain(run: OracleRun, mode: str, dtype, weights, levels: Sequence[Sequence[LevelInputs]],
                  box_merge_mode="bayesian_inference", cls_merge_mode="max_score", image_size=None, out_size=None) -> Chain:
    """levels: per oracle Anchorwise (one, or one per post-NMS member) its LevelInputs.  Scores / probability vectors are fp32
    inputs of this chain (the class side is K1's, held to its own tests); only their means over cluster members are formed here."""
    cv = lambda t: t.to(dtype)
    cands = [candidate_stage(lv, d.tops, eps, dtype, weights) for lv, d, eps in zip(levels, run.decisions, run.eps_prop)]
    if run.clusters is not None:
        parts = [standard_nms_stage(c.boxes, c.cov, cv(aw.probs), cv(aw.scores), d.keep) for c, aw, d in zip(cands, run.aw, run.decisions)]
        pre = ensembles_stage(torch.cat([x.boxes for x in parts]), torch.cat([x.cov for x in parts]), torch.cat([x.probs for x in parts]),
                              run.clusters, run.keep2)
    else:
        c, aw, d = cands[0], run.aw[0], run.decisions[0]
        probs, scores = cv(aw.probs), cv(aw.scores)
        if len(d.keep) == 0:
            pre = Merged(torch.zeros((0, 4), dtype=dtype), torch.zeros((0, 4, 4), dtype=dtype), probs[:0], scores[:0])
        elif mode == "bayes_od":
            pre = bayes_od_stage(c.boxes, c.cov, probs, scores, d, box_merge_mode, cls_merge_mode)
        elif mode == "anchor_statistics":
            pre = anchor_statistics_stage(c.boxes, c.cov, probs, d)
        else:
            pre = standard_nms_stage(c.boxes, c.cov, probs, scores, d.keep)
    return Chain(cands, pre, finalize(pre, image_size, out_size, run.nonempty))


# ---------------------------------------------------------------------------------------------------------------------------
# error measures (profiles/fp64_referee.md states them)
# ---------------------------------------------------------------------------------------------------------------------------

FLOOR = 4 * 2.0 ** -23          # 4 fp32 ulps at the normalising scale
MARGIN = 2.0


def box_error(x, ref64):
    """|x - ref| / max(1, |ref|), element-wise."""
    ref64 = ref64.double()
    return (torch.as_tensor(x).double() - ref64).abs() / ref64.abs().clamp(min=1.0)


def cov_error(c, ref64):
    """|c - ref| / sqrt(C_ii C_jj), the diagonal taken from the fp64 matrix.  Where that is 0 (the covariance of a one-member group
    without candidate covariances is the zero matrix) only an exact 0 has no error."""
    ref64 = ref64.double()
    dg = ref64.diagonal(dim1=-2, dim2=-1)
    scale = torch.sqrt(dg.unsqueeze(-1) * dg.unsqueeze(-2))
    err = (torch.as_tensor(c).double() - ref64).abs()
    exact = torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, float("inf")))
    return torch.where(scale > 0, err / scale.clamp(min=1e-300), exact)


def bar_fractions(c, ref64):
    """Worst fraction of the element-wise bar 1e-4 max(1, |ref|) and of the per-matrix bar 1e-4 max(1, max |ref matrix|)."""
    ref64 = ref64.double()
    err = (torch.as_tensor(c).double() - ref64).abs()
    if err.numel() == 0:
        return 0.0, 0.0
    elem = err / (1e-4 * ref64.abs().clamp(min=1.0))
    if ref64.dim() >= 3:
        mat = err / (1e-4 * ref64.abs().amax(dim=(-2, -1), keepdim=True).clamp(min=1.0))
    else:
        mat = elem
    return float(elem.max()), float(mat.max())


def stats(e: torch.Tensor):
    """(worst, rms, flat index of the worst) of an error tensor."""
    if e.numel() == 0:
        return 0.0, 0.0, -1
    f = e.reshape(-1)
    return float(f.max()), float(torch.sqrt((f * f).mean())), int(f.argmax())


def within_rule(e_hip: torch.Tensor, e_ref: torch.Tensor):
    """The acceptance rule: max and rms of the HIP side's error against fp64 at most MARGIN x the fp32 oracle's over the same entries,
    plus FLOOR.  Returns (ok, figures)."""
    hm, hr, hi = stats(e_hip)
    rm, rr, _ = stats(e_ref)
    fig = dict(n=int(e_hip.numel()), hip_max=hm, ref_max=rm, hip_rms=hr, ref_rms=rr, at=hi,
               ratio_max=hm / max(rm, 1e-300), ratio_rms=hr / max(rr, 1e-300))
    return hm <= MARGIN * rm + FLOOR and hr <= MARGIN * rr + FLOOR, fig
