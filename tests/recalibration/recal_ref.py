"""fp64 numpy restatement of K36 (post-hoc recalibration), written from include/pod_mi355x.h: the referee of the GPU tests.

Sums are added in the header's order -- chunks of 256 consecutive values, a chunk's partial ((0.0 + v_0) + v_1) + ..., then the
partials in chunk order -- so that the moment sums, the residuals, the grid objectives and the covariance map can be compared bit
for bit; the temperature sums go through numpy's exp / log, which are not the device's, and are compared through the test's own bound.
"""
import math
import statistics

import numpy as np

CHUNK = 256
P_LO = 2.0 ** -30
GRID_POINTS, GRID_ONE = 1025, 512
NEWTON_TOL = 2.0 ** -40


def grid_scales():
    return [2.0 ** ((j - GRID_ONE) / 128) for j in range(GRID_POINTS)]


def quantiles():
    nd = statistics.NormalDist()
    return [nd.inv_cdf(i / 15.0) for i in range(1, 15)]


def chunk_sum(values) -> float:
    """The stated order: per 256-value chunk in index order, then the chunk partials in chunk order."""
    v = np.asarray(values, dtype=np.float64).reshape(-1)
    full = v.size // CHUNK
    partials = []
    if full:
        blk = v[:full * CHUNK].reshape(full, CHUNK)
        acc = np.zeros(full, dtype=np.float64)
        for j in range(CHUNK):                         # every chunk's running sum takes its j-th value
            acc = acc + blk[:, j]
        partials = acc.tolist()
    if v.size % CHUNK:
        a = 0.0
        for x in v[full * CHUNK:].tolist():
            a += x
        partials.append(a)
    total = 0.0
    for p in partials:
        total += p
    return total


def logit(p) -> np.ndarray:
    c = np.clip(np.asarray(p, dtype=np.float32).astype(np.float64), P_LO, 1.0 - P_LO)
    return np.log(c / (1.0 - c))


def sigmoid(t: np.ndarray):
    e = np.exp(-np.abs(t))
    d = 1.0 + e
    return np.where(t >= 0.0, 1.0 / d, e / d), e


def cls_terms(p, y, beta: float):
    """The per-score terms of L, g, h at beta."""
    x = logit(p)
    yd = np.asarray(y, dtype=np.float64)
    t = beta * x
    s, e = sigmoid(t)
    return (np.maximum(t, 0.0) + np.log1p(e)) - yd * t, (s - yd) * x, (e / ((1.0 + e) * (1.0 + e))) * (x * x)


def cls_sums(p, y, beta: float):
    return tuple(chunk_sum(t) for t in cls_terms(p, y, beta))


def fit_temperature(p, y, max_iter: int = 50):
    """Newton from beta = 1 -> (beta, iterations)."""
    beta = 1.0
    for it in range(1, max_iter + 1):
        _, g, h = cls_sums(p, y, beta)
        if not (math.isfinite(g) and math.isfinite(h)) or h == 0.0:
            raise ValueError("temperature fit failed")
        step = g / h
        beta -= step
        if abs(step) <= NEWTON_TOL * abs(beta):
            return beta, it
    raise ValueError("no convergence")


def temper(p, beta: float) -> np.ndarray:
    p = np.asarray(p, dtype=np.float32)
    if beta == 1.0:
        return p.copy()
    return sigmoid(beta * logit(p))[0].astype(np.float32)


def reg_z(means, covs, gt, det_class=None, n_class: int = 0):
    """-> z (n, 4) fp64, seg (n, 4) int32 (-1: left out), invalid (4,)."""
    means, gt = np.asarray(means, dtype=np.float32).reshape(-1, 4), np.asarray(gt, dtype=np.float32).reshape(-1, 4)
    var = np.asarray(covs, dtype=np.float32).reshape(-1, 16)[:, [0, 5, 10, 15]].astype(np.float64)
    n = means.shape[0]
    r = gt.astype(np.float64) - means.astype(np.float64)
    c = np.asarray(det_class, dtype=np.int64).reshape(-1, 1) if n_class else np.zeros((n, 1), dtype=np.int64)
    ok = (var > 0.0) & np.isfinite(var) & np.isfinite(r) & (c >= 0) & (c < max(n_class, 1))
    with np.errstate(all="ignore"):
        z = np.where(ok, r / np.sqrt(var), 0.0)
    seg = np.where(ok, 4 * c + np.arange(4)[None, :], -1).astype(np.int32)
    return z, seg, (~ok).sum(0).astype(np.int64)


def group(z, seg, n_seg: int):
    """-> zg (values grouped by segment, row order kept, left-out tail zeros), seg_off (n_seg + 1,)."""
    z, seg = np.asarray(z, dtype=np.float64).reshape(-1), np.asarray(seg).reshape(-1)
    key = np.where((seg >= 0) & (seg < n_seg), seg, n_seg)
    order = np.argsort(key, kind="stable")
    seg_off = np.searchsorted(key[order], np.arange(n_seg + 1), side="left").astype(np.int64)
    zg = z[order].copy()
    zg[seg_off[n_seg]:] = 0.0
    return zg, seg_off


def moment(zg, seg_off):
    """-> counts, sums of z^2 in the stated order."""
    n_seg = len(seg_off) - 1
    counts = np.diff(seg_off).astype(np.int64)
    sums = np.array([chunk_sum(zg[seg_off[s]:seg_off[s + 1]] ** 2) for s in range(n_seg)], dtype=np.float64)
    return counts, sums


def moment_scales(counts, sums):
    return [math.sqrt(t / c) if c else 1.0 for c, t in zip(counts.tolist(), sums.tolist())]


def ece_objectives(z_segment, scales=None, q=None) -> np.ndarray:
    """One segment: obj[j] = (sum_i (count(z < scales[j] q_i) / m - i / 15)^2) / 14, the 14 terms added in i order."""
    scales = np.asarray(grid_scales() if scales is None else scales, dtype=np.float64)
    q = np.asarray(quantiles() if q is None else q, dtype=np.float64)
    zs = np.sort(np.asarray(z_segment, dtype=np.float64))
    m = zs.size
    if m == 0:
        return np.zeros(scales.size, dtype=np.float64)
    acc = np.zeros(scales.size, dtype=np.float64)
    for i in range(1, q.size + 1):
        cnt = np.searchsorted(zs, scales * q[i - 1], side="left")
        dlt = cnt.astype(np.float64) / float(m) - float(i) / float(q.size + 1)
        acc = acc + dlt * dlt
    return acc / float(q.size)


def argmin_tie(obj, j_one: int = GRID_ONE) -> int:
    """The smallest objective; ties to the smaller |j - j_one|, then to the smaller j."""
    return min(range(len(obj)), key=lambda j: (float(obj[j]), abs(j - j_one), j))


def ece_fit(zg, seg_off, scales=None, q=None, j_one: int = GRID_ONE):
    """-> obj (n_seg, n_grid), best_j, best_obj, one_obj."""
    objs = np.stack([ece_objectives(zg[seg_off[s]:seg_off[s + 1]], scales, q) for s in range(len(seg_off) - 1)])
    best = np.array([argmin_tie(o, j_one) for o in objs], dtype=np.int32)
    return objs, best, objs[np.arange(len(best)), best], objs[:, j_one]


def apply_records(records, counts, num_classes: int, beta: float, scales) -> np.ndarray:
    """pod_recal_apply: the same operations in the same order."""
    rec = np.asarray(records, dtype=np.float32)
    n_img, max_det, W = rec.shape
    K = num_classes
    out = np.zeros_like(rec)
    scales = np.asarray(scales, dtype=np.float64).reshape(-1, 4)
    live = np.arange(max_det)[None, :] < np.asarray(counts).reshape(-1, 1)
    r = rec[live]                                       # (rows, W)
    o = r.copy()
    o[:, 4] = temper(r[:, 4], beta)
    o[:, 6:6 + K] = temper(r[:, 6:6 + K], beta)
    if scales.shape[0] > 1:
        with np.errstate(all="ignore"):
            cls = r[:, 5].astype(np.int64)
        known = (cls >= 0) & (cls < scales.shape[0])
        s = np.where(known[:, None], scales[np.clip(cls, 0, scales.shape[0] - 1)], 1.0)
    else:
        s = np.broadcast_to(scales[0], (r.shape[0], 4)).copy()
    s0, s1, s2, s3 = (s[:, k:k + 1] for k in range(4))
    m20, m31 = s2 - s0, s3 - s1
    C = r[:, 6 + K:].astype(np.float64).reshape(-1, 4, 4)
    A = np.empty_like(C)
    A[:, 0] = s0 * C[:, 0]
    A[:, 1] = s1 * C[:, 1]
    A[:, 2] = m20 * C[:, 0] + s2 * C[:, 2]
    A[:, 3] = m31 * C[:, 1] + s3 * C[:, 3]
    Cn = np.empty_like(C)
    Cn[:, :, 0] = A[:, :, 0] * s0
    Cn[:, :, 1] = A[:, :, 1] * s1
    Cn[:, :, 2] = A[:, :, 0] * m20 + A[:, :, 2] * s2
    Cn[:, :, 3] = A[:, :, 1] * m31 + A[:, :, 3] * s3
    one = np.all(s == 1.0, axis=1)
    with np.errstate(all="ignore"):
        new = Cn.reshape(-1, 16).astype(np.float32)
    o[:, 6 + K:] = np.where(one[:, None], r[:, 6 + K:], new)
    out[live] = o
    return out


# ---- the seeded fixture of the tests -------------------------------------------------------------------------------------------------

def fixture(n_m: int, n_fp: int, K: int = 7, seed: int = 36):
    """n_m matched and n_fp false-positive detections: x over-confident by 2 and y under-confident by 1.5 in the box, the class
    probabilities over-confident by a factor 2 in logit space."""
    rng = np.random.default_rng(seed)
    sigma = rng.uniform(1.0, 6.0, size=(n_m, 4))
    resid = rng.standard_normal((n_m, 4)) * sigma * np.array([2.0, 1.0 / 1.5, 2.0, 1.0 / 1.5])
    x = rng.normal(-2.0, 3.0, size=(n_m + n_fp, K))
    labels = (rng.uniform(size=x.shape) < 1.0 / (1.0 + np.exp(-x / 2.0))).astype(np.uint8)
    p = (1.0 / (1.0 + np.exp(-x))).astype(np.float32)
    return {"sigma": sigma, "resid": resid, "p": p, "labels": labels, "rng": rng}
