"""K5 (BayesOD fusion), K6 (anchor statistics) and K7 (finalize) on PLANTED clusters, against the fp64 referee.

The golden fixtures' largest cluster has a handful of members; these kernels walk the candidate rows 256 at a time and reduce across
four wavefronts, so their edges are at cluster sizes no fixture reaches.  Candidate rows are written straight into one HotPath's device
arrays (boxes, cov, cand_score, cand_class, cand_probs, n_total) and `HotPath.postprocess` runs NMS + merge + finalize on them.

Boxes are jittered copies of a few centres, built so that no IoU a decision depends on is near its threshold: every IoU of a kept
centre with a candidate differs from affinity_thresh by >= 1e-3, every IoU of two candidates from nms_thresh by the same gap, in fp32
AND fp64 -- asserted before anything runs (a precondition, not a tolerance), so membership and the keep list are the same in both
precisions.  The kernels accumulate in fp64 registers: the rule of gpu_common.hold (no further from fp64 than 2x the fp32 reference)
must hold everywhere, and for the fused covariance at condition >= 1e4 the HIP result must be the closer one outright."""
import functools

import numpy as np
import pytest
import torch

from oracle import pod_oracle as po
from pod_compare_amd import hotpath, synthetic
from tests.fp64_referee import f64_ref as fr
from tests.fp64_referee.gpu_common import hold, hold_records

pytestmark = pytest.mark.gpu

K = 7
IMAGE, OUT = (2000, 2400), (1497, 1301)          # sy = 0.7485, sx = 0.542...: non-unit, different, not representable
SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 600)   # members per cluster: wavefront edge, workgroup edge, the tid + 256 second trip
WITH_OTHERS = (1, 2, 64, 257)                    # clusters that also hold members of another class inside the IoU ball
GAP = 1e-3
P = po.PathParams(num_classes=K)


def spd(rng, n, cond):
    """n SPD 4x4 fp32 matrices of condition ~cond, variances within 1e-2 .. 1e4 px^2; after the rounding to fp32 the smallest
    eigenvalue is still at least half the intended one (re-drawn otherwise: at 1e7 fp32 rounding alone can make a matrix indefinite)."""
    out = np.empty((n, 4, 4), np.float32)
    todo = np.arange(n)
    while todo.size:
        m = todo.size
        vmax = 10.0 ** rng.uniform(min(np.log10(1e-2 * cond), 3.5), 4.0, m)     # (at 1e7 the smallest eigenvalue goes down to 3e-4)
        ev = vmax[:, None] * np.power(1.0 / cond, np.sort(np.concatenate((np.zeros((m, 1)), rng.uniform(0, 1, (m, 2)), np.ones((m, 1))), 1), 1))
        q, _ = np.linalg.qr(rng.standard_normal((m, 4, 4)))
        c = (q * ev[:, None, :]) @ q.transpose(0, 2, 1)
        c32 = ((c + c.transpose(0, 2, 1)) / 2).astype(np.float32)
        good = np.linalg.eigvalsh(c32.astype(np.float64))[:, 0] >= 0.5 * ev.min(1)
        out[todo[good]] = c32[good]
        todo = todo[~good]
    return out


class Planted:
    """Candidate rows of one planted frame (fp32 CPU tensors, rows shuffled)."""

    def __init__(self, seed, cond, layout):
        """layout: list of (x, y, w, h, members, others, outsiders, degenerate)."""
        rng = np.random.Generator(np.random.Philox(seed))
        boxes, classes, rank = [], [], []
        for ci, (x, y, w, h, members, others, outsiders, degenerate) in enumerate(layout):
            base = np.array([x, y, x + (0.0 if degenerate else w), y + h])
            cls = ci % K
            for j in range(members + others + outsiders):
                b = base + (0.0 if j == 0 else 1.0) * rng.uniform(-0.004, 0.004, 4) * np.array([w, h, w, h])
                if j >= members + others:
                    b = b + np.array([0.1 * w, 0, 0.1 * w, 0])                # IoU with the centre ~ 0.82: neither a member nor kept
                boxes.append(b)
                classes.append((cls + 1) % K if members <= j < members + others else cls)
                rank.append((j != 0, rng.uniform()))                           # the centre scores highest in its cluster
        n = len(boxes)
        order = sorted(range(n), key=lambda i: rank[i])
        score = np.empty(n)
        score[order] = 0.95 - 1e-4 * np.arange(n)                              # all distinct, all above the threshold
        perm = rng.permutation(n)
        self.n = n
        self.boxes = torch.from_numpy(np.asarray(boxes)[perm].astype(np.float32))
        self.classes = torch.from_numpy(np.asarray(classes)[perm].astype(np.int64))
        self.scores = torch.from_numpy(score[perm].astype(np.float32))
        pv = rng.uniform(0.0, 0.3, (n, K)) * score[perm][:, None]
        pv[np.arange(n), self.classes.numpy()] = self.scores.numpy()
        self.probs = torch.from_numpy(pv.astype(np.float32))
        assert torch.equal(self.probs.max(1)[1], self.classes) and torch.equal(self.probs.max(1)[0], self.scores)
        self.cov = torch.from_numpy(spd(rng, n, cond))

    def aw(self, with_cov=True):
        return po.Anchorwise(self.boxes, self.cov if with_cov else None, self.scores, self.classes, self.probs,
                             torch.zeros(self.n, dtype=torch.int64), [self.n])


def grid(k):
    """Slot k of a 200-px grid inside the frame: (x, y)."""
    return 150.0 + 200.0 * (k % 10) + 0.37 * k, 140.0 + 200.0 * (k // 10) + 0.21 * k


@functools.lru_cache(maxsize=None)
def cluster_frame(cond, degenerate=False):
    """Every cluster size, with and without other-class members and near non-members; four clusters clipped at one side of the frame
    each and one clipped to empty; for anchor statistics also a zero-width centre (its class group is empty: centre_fallback)."""
    layout = []
    for k, m in enumerate(SIZES):
        x, y = grid(2 * k)
        layout.append((x, y, 90.0 + 7 * k, 150.0 - 6 * k, m, 3 if m in WITH_OTHERS else 0, 2 if m in (2, 65, 600) else 0, False))
    layout.append(grid(19) + (100.0, 100.0, 1, 0, 0, False))                  # a singleton with nothing around it
    W, H = float(IMAGE[1]), float(IMAGE[0])
    for x, y in ((-30.0, 900.0), (1100.0, -40.0), (W - 60.0, 1300.0), (1500.0, H - 50.0), (W + 50.0, 1700.0)):
        layout.append((x, y, 100.0, 120.0, 3, 0, 0, False))
    if degenerate:
        layout.append((1900.0, 1500.0, 100.0, 100.0, 1, 0, 0, True))
    return Planted(11 + int(np.log10(cond)), cond, layout)


@functools.lru_cache(maxsize=None)
def crowded_frame():
    """More centres than max_detections: 110 two-member clusters."""
    return Planted(29, 1e4, [(100.0 + 190.0 * (k % 12) + 0.37 * k, 100.0 + 170.0 * (k // 12) + 0.21 * k, 100.0, 100.0, 2, 0, 0, False) for k in range(110)])


def assert_decisions_are_safe(pl: Planted, keep):
    for dt in (torch.float32, torch.float64):
        iou = fr.iou_matrix(pl.boxes.to(dt), pl.boxes.to(dt))
        assert float((iou - P.nms_thresh).abs().min()) >= GAP
        assert float((iou[keep] - P.affinity_thresh).abs().min()) >= GAP
    a, b = fr.iou_matrix(pl.boxes, pl.boxes), fr.iou_matrix(pl.boxes.double(), pl.boxes.double())
    assert torch.equal(a > P.nms_thresh, b > P.nms_thresh) and torch.equal(a[keep] > P.affinity_thresh, b[keep] > P.affinity_thresh)


@functools.lru_cache(maxsize=None)
def workspace(with_cov):
    ho = synthetic.planted_head_outputs((96, 128), 1, seed=1, num_boxes=2)
    params = hotpath.PathParams(num_classes=K, num_anchors=ho.num_anchors)
    return hotpath.HotPath(ho.shapes, ho.anchors, params, n_runs=1, has_cls_var=True, cov_dims=4 if with_cov else 0, device="cuda")


def plant(hp, pl: Planted):
    n = pl.n
    assert n <= hp.n_cap
    for dst in (hp.boxes, hp.cov, hp.cand_score, hp.cand_class, hp.cand_probs):
        dst.zero_()
    hp.boxes[:n].copy_(pl.boxes)
    hp.cov[:n].copy_(pl.cov)
    hp.cand_score[:n].copy_(pl.scores)
    hp.cand_class[:n].copy_(pl.classes.to(torch.int32))
    hp.cand_probs[:n].copy_(pl.probs)
    hp.n_total.fill_(n)


@functools.lru_cache(maxsize=None)
def reference(frame, args, mode, box_merge, cls_merge, with_cov=True):
    """fp32 oracle rows, its decisions and the fp64 referee's rows for one planted frame and mode; computed once."""
    pl = frame(*args)
    aw = pl.aw(with_cov)
    if mode == "bayes_od":
        pre = po.bayes_od_post(aw, IMAGE, P, box_merge, cls_merge)
    else:
        pre = po.anchor_statistics_post(aw, IMAGE, P)
    d = fr.Decisions([], pre.keep)
    d.member, d.same = fr.cluster_decisions(mode, pl.boxes, pl.probs, pl.classes, pre.keep, P)
    assert_decisions_are_safe(pl, pre.keep)
    b, c, pv, sc = pl.boxes.double(), pl.cov.double() if with_cov else None, pl.probs.double(), pl.scores.double()
    pre64 = fr.bayes_od_stage(b, c, pv, sc, d, box_merge, cls_merge) if mode == "bayes_od" else fr.anchor_statistics_stage(b, c, pv, d)
    # The non-empty mask: a clipped box is either gone entirely or at least a pixel wide and high (precondition), so the mask is the
    # same in both precisions -- as long as the fp32 rows are boxes at all: at condition 1e7 the reference's fused means are off by
    # hundreds of pixels and its own mask differs.  The mask is therefore taken from the fp64 rows, and the fp32 side is finalized
    # under it with the same arithmetic at float32 (which is po.finalize: test_f64_referee_cpu.py).
    clipped = fr.scale_clip(pre64.boxes, IMAGE, OUT)
    w, h = clipped[:, 2] - clipped[:, 0], clipped[:, 3] - clipped[:, 1]
    assert bool((((w == 0) | (w >= 1)) & ((h == 0) | (h >= 1))).all())
    ok = (w > 0) & (h > 0)
    sane = not (mode == "bayes_od" and args and args[0] >= 1e7)
    if sane:
        assert torch.equal(ok, fr.nonempty_fp32(pre.pred_boxes, IMAGE, OUT))
    det32 = fr.finalize(fr.Merged(pre.pred_boxes, pre.pred_boxes_covariance, pre.pred_cls_probs, pre.scores), IMAGE, OUT, ok)
    if sane:
        ref = po.finalize(pre, OUT[0], OUT[1])
        assert torch.equal(det32.boxes, ref.pred_boxes) and torch.equal(det32.cov, ref.pred_boxes_covariance)
    det = po.Detections(OUT, det32.boxes, det32.scores, pre.pred_classes[ok], det32.probs, det32.cov)
    return pl, pre, det, d, ok, pre64, fr.finalize(pre64, IMAGE, OUT, ok)


def run_and_hold(ref, mode, box_merge="bayesian_inference", cls_merge="max_score", with_cov=True, beat_fused=False):
    pl, pre, det, d, ok, pre64, det64 = ref
    hp = workspace(with_cov)
    plant(hp, pl)
    out = hp.postprocess(mode, IMAGE, OUT, box_merge, cls_merge)
    nk = int(hp.n_keep.item())
    assert torch.equal(hp.keep[:nk].cpu().long(), d.keep)
    assert torch.equal(hp.m_classes[:nk].cpu().long(), pre.pred_classes)
    hold("merged boxes", "box", hp.m_boxes[:nk], pre.pred_boxes, pre64.boxes)
    fig = hold("merged cov", "cov", hp.m_cov[:nk], pre.pred_boxes_covariance, pre64.cov, must_beat=beat_fused)
    hold("merged probs", "box", hp.m_probs[:nk], pre.pred_cls_probs, pre64.probs)
    m = out.count()
    assert m == int(ok.sum()) == len(det)
    assert torch.equal(out.classes[:m].cpu().long(), det.pred_classes)
    hold("final boxes", "box", out.boxes[:m], det.pred_boxes, det64.boxes)
    hold("final cov", "cov", out.cov[:m], det.pred_boxes_covariance, det64.cov)
    hold_records(out, m, K)
    return hp, pl, d, ok, out, fig


@pytest.mark.parametrize("cls_merge", ["max_score", "bayesian_inference"])
@pytest.mark.parametrize("box_merge", ["bayesian_inference", "covariance_intersection"])
@pytest.mark.parametrize("cond", [1e0, 1e4, 1e7])
def test_k5_on_planted_clusters(cond, box_merge, cls_merge):
    """1 .. 600 members per cluster, both box merges and both class merges, member covariances of condition 1, 1e4 and 1e7 (where the
    reference's fp32 LAPACK inverse loses most of its digits): K5 inverts in fp64 and must be the closer side from 1e4 on."""
    ref = reference(cluster_frame, (cond,), "bayes_od", box_merge, cls_merge)
    hp, pl, d, ok, out, fig = run_and_hold(ref, "bayes_od", box_merge, cls_merge, beat_fused=cond >= 1e4)
    sizes = sorted(int(s.sum()) for s in d.same)
    balls = [int(r.sum()) for r in d.member]
    assert set(SIZES) <= set(sizes) and {m + 3 for m in WITH_OTHERS} <= set(balls)      # other-class members inside the IoU ball
    # finalize: every side clipped once, one row clipped to empty and the rows behind it moved up
    assert int((~ok).sum()) == 1 and int((~ok).nonzero()[0]) < len(ok) - 1
    m = out.count()
    b = out.boxes[:m].cpu()
    assert bool((b[:, 0] == 0).any() and (b[:, 1] == 0).any() and (b[:, 2] == OUT[1]).any() and (b[:, 3] == OUT[0]).any())


@pytest.mark.parametrize("with_cov", [True, False])
def test_k6_on_planted_clusters(with_cov):
    """Anchor statistics with candidate covariances (their mean is added) and without (a singleton falls back to 1e-4 I); a zero-width
    centre has no member at all, itself included: the centre's own row, which finalize then drops."""
    ref = reference(cluster_frame, (1e4, True), "anchor_statistics", "", "", with_cov)
    hp, pl, d, ok, out, fig = run_and_hold(ref, "anchor_statistics", with_cov=with_cov)
    empty = [i for i, row in enumerate(d.member) if int(row.sum()) == 0]
    assert len(empty) == 1
    c = int(d.keep[empty[0]])
    assert torch.equal(hp.m_boxes[empty[0]].cpu(), pl.boxes[c])
    want = pl.cov[c] if with_cov else 1e-4 * torch.eye(4)
    assert torch.equal(hp.m_cov[empty[0]].cpu(), want)
    assert int((~ok).sum()) == 2 and not bool(ok[empty[0]])
    singles = [i for i, row in enumerate(d.member) if int(row.sum()) == 1]
    assert singles and (with_cov or all(torch.equal(hp.m_cov[i].cpu(), 1e-4 * torch.eye(4)) for i in singles))


@pytest.mark.parametrize("mode", ["bayes_od", "anchor_statistics"])
def test_max_detections_centres_at_once(mode):
    """110 clusters: the keep list is cut at max_detections and every one of the 100 workgroups has a cluster."""
    ref = reference(crowded_frame, (), mode, "bayesian_inference", "max_score")
    hp, pl, d, ok, out, fig = run_and_hold(ref, mode, beat_fused=mode == "bayes_od")
    assert len(d.keep) == P.max_detections == out.count()
