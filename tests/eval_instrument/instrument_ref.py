"""Referees for the metric's instrument, plain numpy / torch on the CPU.

  match_ref        brute-force restatement of include/pod_mi355x.h's contract for pod_match_groundtruth's raw outputs
  undecided_pairs  how many (ground truth, detection) pairs sit so close to a threshold that fp32 could decide them either way
  nll_ref          -log N(gt; mean, cov + 1e-2 I) in fp64 through torch.linalg.cholesky

and what the tests of both kernels share: the packing of per-image dicts into the C ABI's concatenated arrays, the assembly of the raw
outputs into the reference's four partitions, and the seeded case generators."""
import math
from typing import Dict, NamedTuple

import numpy as np
import torch

MATCH_MAX_DET = 128
SENTINEL = -7
LOG_2PI = math.log(2.0 * math.pi)


# ----------------------------------------------------------------------------------------------------------------------------------
# ground-truth matching
# ----------------------------------------------------------------------------------------------------------------------------------

def iou_f32(gt: np.ndarray, det: np.ndarray) -> np.ndarray:
    """(G, M) fp32 IoU, detectron2 pairwise_iou's operations in its order (oracle.pod_oracle.iou_matrix): every step one correctly
    rounded fp32 operation, inter / ((area_gt + area_det) - inter) where inter > 0, else 0."""
    gt, det = np.asarray(gt, np.float32).reshape(-1, 4), np.asarray(det, np.float32).reshape(-1, 4)
    w = np.minimum(gt[:, None, 2], det[None, :, 2]) - np.maximum(gt[:, None, 0], det[None, :, 0])
    h = np.minimum(gt[:, None, 3], det[None, :, 3]) - np.maximum(gt[:, None, 1], det[None, :, 1])
    inter = np.maximum(w, np.float32(0)) * np.maximum(h, np.float32(0))
    ag = (gt[:, 2] - gt[:, 0]) * (gt[:, 3] - gt[:, 1])
    ad = (det[:, 2] - det[:, 0]) * (det[:, 3] - det[:, 1])
    den = (ag[:, None] + ad[None, :]) - inter
    assert inter.dtype == np.float32 and den.dtype == np.float32
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(inter > 0, inter / den, np.float32(0)).astype(np.float32)


def iou_f64(gt: np.ndarray, det: np.ndarray) -> np.ndarray:
    """The same quantity of the same fp32 boxes in fp64."""
    gt, det = np.asarray(gt, np.float64).reshape(-1, 4), np.asarray(det, np.float64).reshape(-1, 4)
    w = np.minimum(gt[:, None, 2], det[None, :, 2]) - np.maximum(gt[:, None, 0], det[None, :, 0])
    h = np.minimum(gt[:, None, 3], det[None, :, 3]) - np.maximum(gt[:, None, 1], det[None, :, 1])
    inter = np.maximum(w, 0.0) * np.maximum(h, 0.0)
    ag = (gt[:, 2] - gt[:, 0]) * (gt[:, 3] - gt[:, 1])
    ad = (det[:, 2] - det[:, 0]) * (det[:, 3] - det[:, 1])
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(inter > 0, inter / (ag[:, None] + ad[None, :] - inter), 0.0)


def _images(det_off, gt_off):
    det_off, gt_off = np.asarray(det_off, np.int64), np.asarray(gt_off, np.int64)
    assert det_off.shape == gt_off.shape
    for m in range(len(det_off) - 1):
        yield int(det_off[m]), int(det_off[m + 1]), int(gt_off[m]), int(gt_off[m + 1])


def match_ref(det_boxes, det_probs, det_off, gt_boxes, gt_off, iou_min, iou_correct) -> Dict:
    """pod_match_groundtruth's raw outputs: gt_fn (G,), gt_match_count (G,), gt_match_idx / gt_match_iou as one list per ground-truth
    box (global detection indices, best first: descending max class probability, then lower detection index), det_fp (D,)."""
    det_boxes = np.asarray(det_boxes, np.float32).reshape(-1, 4)
    gt_boxes = np.asarray(gt_boxes, np.float32).reshape(-1, 4)
    det_probs = np.asarray(det_probs, np.float32)
    lo, hi = np.float32(iou_min), np.float32(iou_correct)
    D, G = det_boxes.shape[0], gt_boxes.shape[0]
    score = det_probs.max(axis=1) if D else np.zeros(0, np.float32)
    gt_fn, count, det_fp = np.zeros(G, np.int32), np.zeros(G, np.int32), np.zeros(D, np.int32)
    idx, ious = [None] * G, [None] * G
    for d0, d1, g0, g1 in _images(det_off, gt_off):
        assert d1 - d0 <= MATCH_MAX_DET
        iou = iou_f32(gt_boxes[g0:g1], det_boxes[d0:d1])
        for d in range(d0, d1):
            det_fp[d] = 1 if all(iou[g - g0, d - d0] <= lo for g in range(g0, g1)) else 0
        for g in range(g0, g1):
            row = iou[g - g0]
            gt_fn[g] = 1 if all(v <= lo for v in row) else 0
            hits = sorted((j for j in range(d1 - d0) if row[j] >= hi), key=lambda j: (-float(score[d0 + j]), j))
            count[g] = len(hits)
            idx[g] = [d0 + j for j in hits]
            ious[g] = np.array([row[j] for j in hits], np.float32)
    return {"gt_fn": gt_fn, "gt_match_count": count, "gt_match_idx": idx, "gt_match_iou": ious, "det_fp": det_fp}


def undecided_pairs(det_boxes, det_off, gt_boxes, gt_off, iou_min, iou_correct, margin=1e-5):
    """(pairs whose fp64 IoU lies within `margin` of a threshold, all pairs).  The fp32 IoU is ~8 correctly rounded operations on
    exact fp32 inputs (relative error <= ~5e-7), so a pair outside the margin is decided alike by every correct implementation."""
    det_boxes, gt_boxes = np.asarray(det_boxes, np.float32).reshape(-1, 4), np.asarray(gt_boxes, np.float32).reshape(-1, 4)
    thr = [float(np.float32(iou_min)), float(np.float32(iou_correct))]
    close = total = 0
    for d0, d1, g0, g1 in _images(det_off, gt_off):
        iou = iou_f64(gt_boxes[g0:g1], det_boxes[d0:d1])
        total += iou.size
        close += int(sum((np.abs(iou - t) <= margin).sum() for t in thr))
    return close, total


class Packed(NamedTuple):
    """A data set in the C ABI's layout: image slots are the prediction dict's keys in order; a key without ground truth owns no boxes."""
    det_boxes: np.ndarray
    det_probs: np.ndarray
    det_covs: np.ndarray
    det_off: np.ndarray
    det_img: np.ndarray
    gt_boxes: np.ndarray
    gt_cats: np.ndarray
    gt_off: np.ndarray
    gt_img: np.ndarray
    K: int


def pack(pb: Dict, pp: Dict, pc: Dict, gb: Dict, gc: Dict) -> Packed:
    keys = list(pb.keys())
    K = int(next(iter(pp.values())).shape[1]) if keys else 0          # no prediction: no class count (the oracle's (0, 0))
    f = lambda t, *s: np.asarray(t, np.float32).reshape(*s)
    cat = lambda parts, *s: np.concatenate(parts) if parts else np.zeros((0,) + s, np.float32)
    nd = [int(pb[k].shape[0]) for k in keys]
    ng = [int(gb[k].shape[0]) if k in gb else 0 for k in keys]
    off = lambda n: np.concatenate([[0], np.cumsum(n)]).astype(np.int32)
    img = lambda n: np.repeat(np.arange(len(n)), n).astype(np.int32)
    return Packed(cat([f(pb[k], -1, 4) for k in keys], 4), cat([f(pp[k], -1, K) for k in keys], K), cat([f(pc[k], -1, 4, 4) for k in keys], 4, 4),
                  off(nd), img(nd), cat([f(gb[k], -1, 4) for k in keys if k in gb], 4), cat([f(gc[k], -1, 1) for k in keys if k in gb], 1),
                  off(ng), img(ng), K)


def partitions(p: Packed, raw: Dict) -> Dict:
    """The reference's four partitions from the raw outputs: rows in ground-truth order (then rank) / detection order."""
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    G = p.gt_boxes.shape[0]
    tp_g = [g for g in range(G) if raw["gt_match_count"][g] > 0]
    tp_d = [raw["gt_match_idx"][g][0] for g in tp_g]
    tp_i = [raw["gt_match_iou"][g][0] for g in tp_g]
    dup_g = [g for g in range(G) for _ in range(1, int(raw["gt_match_count"][g]))]
    dup_d = [d for g in range(G) for d in raw["gt_match_idx"][g][1:]]
    dup_i = [v for g in range(G) for v in raw["gt_match_iou"][g][1:]]
    fp_d, fn_g = np.nonzero(raw["det_fp"])[0], np.nonzero(raw["gt_fn"])[0]
    ix = lambda l: np.asarray(l, np.int64)
    part = lambda d, g, iou: {"predicted_box_means": t(p.det_boxes[ix(d)]), "predicted_box_covariances": t(p.det_covs[ix(d)]),
                              "predicted_cls_probs": t(p.det_probs[ix(d)]), "gt_box_means": t(p.gt_boxes[ix(g)]),
                              "gt_cat_idxs": t(p.gt_cats[ix(g)]), "iou_with_ground_truth": t(np.asarray(iou, np.float32))}
    return {"true_positives": part(tp_d, tp_g, tp_i), "duplicates": part(dup_d, dup_g, dup_i),
            "false_positives": {"predicted_box_means": t(p.det_boxes[fp_d]), "predicted_box_covariances": t(p.det_covs[fp_d]),
                                "predicted_cls_probs": t(p.det_probs[fp_d])},
            "false_negatives": {"gt_box_means": t(p.gt_boxes[fn_g]), "gt_cat_idxs": t(p.gt_cats[fn_g])}}


def assert_partitions_equal(got: Dict, want: Dict, what=""):
    """torch.equal on every tensor of the four partitions, rows in the same order."""
    assert sorted(got) == sorted(want), (what, sorted(got), sorted(want))
    for part in want:
        assert sorted(got[part]) == sorted(want[part]), (what, part)
        for name, ref in want[part].items():
            val = got[part][name].cpu()
            assert tuple(val.shape) == tuple(ref.shape), (what, part, name, tuple(val.shape), tuple(ref.shape))
            assert val.dtype == ref.dtype and torch.equal(val, ref), (what, part, name)


def part_counts(res: Dict):
    return (int(res["true_positives"]["predicted_box_means"].shape[0]), int(res["duplicates"]["predicted_box_means"].shape[0]),
            int(res["false_positives"]["predicted_box_means"].shape[0]), int(res["false_negatives"]["gt_box_means"].shape[0]))


# ----------------------------------------------------------------------------------------------------------------------------------
# matching cases: name -> dict(pb, pp, pc, gb, gc[, iou_min, iou_correct]); `seeded` marks the random ones (undecided_pairs == 0)
# ----------------------------------------------------------------------------------------------------------------------------------

GT = [100.0, 100.0, 200.0, 200.0]


def _covs(rng, n):
    l = rng.standard_normal((n, 4, 4)).astype(np.float32)
    return l @ l.transpose(0, 2, 1) + np.eye(4, dtype=np.float32)


def _onehot(score, K, col=None, rng=None):
    """(n, K) probabilities whose row maximum is `score` (> 0), in column `col` (default: seeded random columns)."""
    score = np.asarray(score, np.float32)
    p = np.zeros((score.shape[0], K), np.float32)
    c = np.full(score.shape[0], col) if col is not None else rng.integers(0, K, score.shape[0])
    p[np.arange(score.shape[0]), c] = score
    return p


def _far(n):
    """n boxes that overlap neither GT nor each other's images' ground truth."""
    j = np.arange(n, dtype=np.float32)
    return np.stack([1000 + 10 * j, 1000 + 0 * j, 1008 + 10 * j, 1050 + 0 * j], 1)


def _dataset(images, K=7, seed=0):
    """images: list of (det (n, 4), score (n,) or probs (n, K), gt (g, 4) or None) -> the five dicts, keys 10, 11, ..."""
    rng = np.random.default_rng(seed)
    pb, pp, pc, gb, gc = {}, {}, {}, {}, {}
    for m, (det, sc, gt) in enumerate(images):
        key = 10 + m
        det = np.asarray(det, np.float32).reshape(-1, 4)
        sc = np.asarray(sc, np.float32)
        pb[key] = torch.from_numpy(det)
        pp[key] = torch.from_numpy(sc.reshape(-1, K) if sc.ndim == 2 else _onehot(sc, K, rng=rng))
        pc[key] = torch.from_numpy(_covs(rng, det.shape[0]))
        if gt is not None:
            gt = np.asarray(gt, np.float32).reshape(-1, 4)
            gb[key] = torch.from_numpy(gt)
            gc[key] = torch.from_numpy(rng.integers(1, K + 1, (gt.shape[0], 1)).astype(np.float32))
    return dict(pb=pb, pp=pp, pc=pc, gb=gb, gc=gc)


def case_lane_trips():
    """One box per image; nd in {0, 1, 63, 64, 65, 100, 127, 128}: the only hit / the only partial overlap is the LAST detection."""
    images = []
    for nd in (0, 1, 63, 64, 65, 100, 127, 128):
        sc = 0.1 + 0.8 * np.arange(nd, dtype=np.float32) / 128
        if nd == 0:
            images.append((np.zeros((0, 4)), sc, [GT]))
            continue
        hit, part = _far(nd), _far(nd)
        hit[-1] = [101, 100, 200, 199]                     # IoU 0.98
        part[-1] = [150, 100, 250, 200]                    # IoU 1/3: neither a hit nor missed
        images += [(hit, sc, [GT]), (part, sc, [GT])]
    return _dataset(images)


def case_all_hit_128(quantised: bool):
    rng = np.random.default_rng(128)
    gt = np.array([100.0, 100.0, 300.0, 300.0])
    det = (gt[None, :] + rng.uniform(-4.0, 4.0, (128, 4))).astype(np.float32)          # jitter <= 2 % of 200
    sc = rng.integers(1, 9, 128) / 8.0 if quantised else rng.permutation(np.arange(1, 129)) / 256.0
    return _dataset([(det, sc, [gt])], seed=128)


def threshold_boxes():
    """Against [0, 0, 10, 10]: IoU exactly 0.7f / 0.1f, and y2 moved by one nextafter step up and down."""
    out = []
    for y2 in (7.0, 1.0):
        y = np.float32(y2)
        for v in (y, np.nextafter(y, np.float32(np.inf)), np.nextafter(y, np.float32(-np.inf))):
            out.append(np.array([0, 0, 10, v], np.float32))
    return out          # [0.7, 0.7+, 0.7-, 0.1, 0.1+, 0.1-]


def case_thresholds_exact():
    return _dataset([([b], [0.5], [[0, 0, 10, 10]]) for b in threshold_boxes()])


def case_shared_detection():
    return _dataset([([GT, [400, 400, 450, 450]], [0.5, 0.9], [GT, [101, 100, 200, 200]])])


def case_cross_image():
    a, b = [100, 100, 200, 200], [300, 100, 380, 220]
    c, d = [600, 600, 700, 700], [100, 500, 220, 560]
    near = lambda x: [x[0] + 1, x[1], x[2], x[3] - 1]
    return _dataset([([near(a), near(b)], [0.9, 0.8], [a, b]),
                     ([near(a), near(b)], [0.9, 0.8], [c, d]),          # the coordinates of image 0's detections: no hit HERE
                     ([near(c), near(d)], [0.9, 0.8], [a, b]),          # the coordinates of image 0's boxes
                     ([near(c), near(d)], [0.9, 0.8], [c, d])])


def case_empties():
    e = np.zeros((0, 4), np.float32)
    return _dataset([([GT], [0.5], None), ([GT, [0, 0, 5, 5]], [0.5, 0.25], e), (e, np.zeros(0), [GT, [0, 0, 5, 5]]), ([GT], [0.5], [GT])])


def case_all_predictions_empty():
    e = np.zeros((0, 4), np.float32)
    return _dataset([(e, np.zeros(0), [GT]), (e, np.zeros(0), [GT, [0, 0, 5, 5]])])


def case_no_ground_truth_at_all():
    return _dataset([([GT], [0.5], None), ([GT, [0, 0, 5, 5]], [0.5, 0.25], None)])


def case_everything_empty():
    return dict(pb={}, pp={}, pc={}, gb={}, gc={})


def case_degenerate():
    return _dataset([([[5, 5, 5, 5]], [0.5], [[5, 5, 5, 5]]),                   # zero area on both sides: inter == 0 -> IoU 0
                     ([[5, 5, 5, 20]], [0.5], [[5, 5, 5, 20]]),                 # zero width
                     ([[8, 0, 2, 10], [8, 8, 2, 2]], [0.5, 0.6], [[0, 0, 10, 10]]),          # x2 < x1 (area < 0); both reversed (area > 0)
                     ([[0, 0, 10, 10]], [0.5], [[8, 0, 2, 10]])])


def random_set(seed, nd, ng, K=7, last_column_every=0):
    """Detections are ground-truth boxes jittered by {4 %, 25 %, 300 %} of their size (chosen at random), probabilities quantised to
    1/8 so that ties occur; every fifth key has no ground truth."""
    rng = np.random.default_rng(seed)
    images = []
    for m, (n, g) in enumerate(zip(nd, ng)):
        xy = rng.uniform(0.0, 600.0, (max(g, 1), 2))
        wh = rng.uniform(20.0, 200.0, (max(g, 1), 2))
        gt = np.concatenate([xy, xy + wh], 1)
        src = rng.integers(0, gt.shape[0], n)
        frac = rng.choice([0.04, 0.25, 3.0], n)
        size = np.concatenate([wh, wh], 1)[src]
        det = gt[src] + rng.uniform(-1.0, 1.0, (n, 4)) * frac[:, None] * size
        probs = (rng.integers(0, 8 if last_column_every else 9, (n, K)) / 8.0).astype(np.float32)
        if last_column_every:
            probs[::last_column_every, K - 1] = 1.0          # the row maximum sits in the last column (and ties with its like)
        images.append((det, probs, None if m % 5 == 4 else gt[:g]))
    return _dataset(images, K=K, seed=seed)


MIXED_ND = [1, 63, 64, 65, 100, 127, 128, 0, 17, 128]
MIXED_NG = [3, 5, 1, 8, 12, 2, 40, 4, 0, 6]
MIXED_SEEDS = (1, 2, 3)
CLASS_COUNTS = (1, 7, 80)
MANY_IMAGES = 1500


def case_many_images():
    rng = np.random.default_rng(1500)
    return random_set(1500, rng.integers(0, 21, MANY_IMAGES).tolist(), rng.integers(0, 6, MANY_IMAGES).tolist())


def case_limit(n):
    det = np.tile(np.array([GT], np.float32), (n, 1))
    return _dataset([(det, 0.1 + 0.8 * np.arange(n, dtype=np.float32) / 256, [GT])])


SEEDED = dict([("mixed_s%d" % s, (lambda s=s: random_set(s, MIXED_ND, MIXED_NG))) for s in MIXED_SEEDS] +
              [("class_counts_K%d" % k, (lambda k=k: random_set(40 + k, [5, 70, 128, 9], [2, 3, 4, 2], K=k, last_column_every=3))) for k in CLASS_COUNTS] +
              [("many_images", case_many_images)])
CASES = dict([("lane_trips", case_lane_trips), ("all_hit_128_distinct", lambda: case_all_hit_128(False)),
              ("all_hit_128_quantised", lambda: case_all_hit_128(True)), ("thresholds_exact", case_thresholds_exact),
              ("shared_detection", case_shared_detection), ("cross_image", case_cross_image), ("empties", case_empties),
              ("all_predictions_empty", case_all_predictions_empty), ("no_ground_truth_at_all", case_no_ground_truth_at_all),
              ("everything_empty", case_everything_empty), ("degenerate", case_degenerate), ("limit_128", lambda: case_limit(128))] +
             list(SEEDED.items()))
_BUILT = {}


def case(name):
    """The case's dicts, its packing, match_ref's outputs and the oracle's partitions: computed once, shared, never modified."""
    if name not in _BUILT:
        from oracle import pod_oracle as po
        c = CASES[name]()
        p = pack(c["pb"], c["pp"], c["pc"], c["gb"], c["gc"])
        raw = match_ref(p.det_boxes, p.det_probs, p.det_off, p.gt_boxes, p.gt_off, 0.1, 0.7)
        want = po.match_predictions_to_groundtruth(c["pb"], c["pp"], c["pc"], c["gb"], c["gc"], 0.1, 0.7)
        _BUILT[name] = (c, p, raw, want)
    return _BUILT[name]


# ----------------------------------------------------------------------------------------------------------------------------------
# regression NLL
# ----------------------------------------------------------------------------------------------------------------------------------

def nll_sigma(covs: torch.Tensor) -> torch.Tensor:
    """cov + 1e-2 I formed in fp32, as the reference (scoring_rules.py:68) and the kernel form it, then fp64, symmetrised from the
    lower triangle (what a Cholesky factorisation reads)."""
    sig = (covs.float() + torch.tensor(1e-2, dtype=torch.float32) * torch.eye(4, dtype=torch.float32)).double()
    low = torch.tril(sig)
    return low + torch.tril(sig, -1).transpose(-1, -2)


def nll_factor(covs: torch.Tensor) -> torch.Tensor:
    return torch.linalg.cholesky(nll_sigma(covs))


def nll_ref(means: torch.Tensor, covs: torch.Tensor, gt: torch.Tensor) -> torch.Tensor:
    """0.5 |L^-1 (gt - mean)|^2 + sum log L_ii + 2 log 2 pi, fp64."""
    L = nll_factor(covs)
    diff = (gt.double() - means.double()).unsqueeze(-1)
    y = torch.linalg.solve_triangular(L, diff, upper=False).squeeze(-1)
    return 0.5 * (y * y).sum(-1) + torch.log(torch.diagonal(L, dim1=-2, dim2=-1)).sum(-1) + 2.0 * LOG_2PI


def entropy_ref(covs: torch.Tensor) -> torch.Tensor:
    """0.5 log det(2 pi e Sigma) from nll_ref's factor."""
    L = nll_factor(covs)
    return torch.log(torch.diagonal(L, dim1=-2, dim2=-1)).sum(-1) + 2.0 * (1.0 + LOG_2PI)


def nll_cond(covs: torch.Tensor) -> torch.Tensor:
    ev = torch.linalg.eigvalsh(nll_sigma(covs))
    return ev[:, -1] / ev[:, 0]


NLL_FAMILIES = ("wishart", "zero", "cond1e6", "rank1", "huge")
NLL_SIZES = (1, 255, 256, 257)
NLL_LARGE = 70001
NLL_COND_MAX = 1e6


def _rotations(g, n):
    q, r = torch.linalg.qr(torch.randn(n, 4, 4, dtype=torch.float64, generator=g))
    return q * torch.sign(torch.diagonal(r, dim1=-2, dim2=-1)).unsqueeze(-2)


def nll_family(name: str, n: int, seed: int = 0):
    """(means, covs, gt) fp32, means ~ 300 +- 50."""
    g = torch.Generator().manual_seed(1000 * NLL_FAMILIES.index(name) + seed + n)
    rn = lambda *s: torch.randn(*s, dtype=torch.float64, generator=g)
    means = 300.0 + 50.0 * rn(n, 4)
    eye = torch.eye(4, dtype=torch.float64)
    if name == "wishart":
        l = rn(n, 4, 4)
        covs, dev = l @ l.transpose(1, 2) + 0.5 * eye, 2.0
    elif name == "zero":
        covs, dev = torch.zeros(n, 4, 4, dtype=torch.float64), 0.05
    elif name == "cond1e6":
        # fp32 rounding of the 1e4-sized entries moves the smallest eigenvalue of Sigma (1e-2) by up to ~1e-3: draw 4 n candidates and
        # keep the first n whose ROUNDED Sigma has cond <= 1e6 -- a property of the input alone, the bound the fp64 referee's error rests on
        q = _rotations(g, 4 * n + 8)
        covs = (q * torch.tensor([1e4, 1.0, 1e-2, 0.0], dtype=torch.float64)) @ q.transpose(1, 2)
        covs = 0.5 * (covs + covs.transpose(1, 2))          # exactly symmetric, so also after rounding to fp32
        covs = covs[nll_cond(covs.float()) <= NLL_COND_MAX][:n]
        assert covs.shape[0] == n
        dev = 2.0
    elif name == "rank1":
        v = rn(n, 4)
        v = v / v.norm(dim=1, keepdim=True)
        covs, dev = 100.0 * v.unsqueeze(2) * v.unsqueeze(1), 2.0
    elif name == "huge":
        l = rn(n, 4, 4)
        covs, dev = 1e6 * (l @ l.transpose(1, 2) + eye), 1e3
    else:
        raise KeyError(name)
    gt = means + dev * rn(n, 4)
    covs = 0.5 * (covs + covs.transpose(1, 2))
    return means.float(), covs.float(), gt.float()
