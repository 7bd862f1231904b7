"""The referee of tests/pdq/: PDQ as include/pod_mi355x.h (K34) and DESIGN.md define it, restated in numpy fp64 (erfc from torch: numpy has
none).  It shares no code with the kernel and differs where it may: it walks the WHOLE frame (no region of interest), integrates Phi2 with
eight panels of 32 Gauss-Legendre points whatever rho is, and sums with numpy's pairwise sums.  The assignment is restated step for step
(`assign_ref`, bit-equal by construction: additions, subtractions and comparisons) and brute-forced over permutations (`assign_brute`)."""
import itertools
import math

import numpy as np
import torch

SMALL = 1e-14
P_MIN = 0.0027
RHO_MAX = 0.99
PANELS, POINTS = 8, 32
MAX_SIDE = 256
PLANES = ("pPDQ", "q_spatial", "q_label", "q_fg", "q_bg")
# The referee's own worst error per pixel in log P / log max(Q, small) against 40-digit arithmetic, as test_pdq_cpu.py measures and asserts it
# (profiles/pdq.md has the figures).  The kernel gets eight times that per pixel entering a sum, with a floor of 1e-13 per pixel.
REFEREE_PIXEL_ERR = 1e-14
KERNEL_PIXEL_BOUND = max(8.0 * REFEREE_PIXEL_ERR, 1e-13)
QUALITY_BOUND = 1e-9

_GL_X, _GL_W = np.polynomial.legendre.leggauss(POINTS)


def erfc(x):
    return torch.special.erfc(torch.as_tensor(np.asarray(x, dtype=np.float64))).numpy()


def phi(x):
    return 0.5 * erfc(-np.asarray(x, dtype=np.float64) / math.sqrt(2.0))


def phi2_integral(h, k, rho):
    """(1 / 2 pi) int_0^{asin rho} exp(-(h^2 + k^2 - 2 h k sin t) / (2 cos^2 t)) dt for arrays h, k (broadcast) and a scalar rho."""
    h, k = np.broadcast_arrays(np.asarray(h, dtype=np.float64), np.asarray(k, dtype=np.float64))
    top = math.asin(rho)
    out = np.zeros(h.shape, dtype=np.float64)
    half = 0.5 * top / PANELS
    a, b = h * h + k * k, 2.0 * h * k
    for panel in range(PANELS):
        t = half * (2 * panel + 1) + half * _GL_X
        s, c2 = np.sin(t), np.cos(t) ** 2
        for q in range(POINTS):
            out += (_GL_W[q] * half) * np.exp(-(a - b * s[q]) / (2.0 * c2[q]))
    return out / (2.0 * math.pi)


def phi2(h, k, rho):
    return phi(h) * phi(k) + phi2_integral(h, k, rho)


def phi2_complement(h, k, rho):
    """1 - Phi2(h, k; rho), never formed as that difference: Phi(-h) + Phi(-k) - Phi2(-h, -k; rho)."""
    return phi(-np.asarray(h)) + phi(-np.asarray(k)) - phi2(-np.asarray(h), -np.asarray(k), rho)


def corner_blocks(mean, cov):
    """fp32 mean (4,), cov (4, 4) -> (mu[4], sd[4], rho[2], valid) in fp64: cov + 1e-2 I formed in fp32, the lower triangle read."""
    mean = np.asarray(mean, dtype=np.float32)
    cov = np.asarray(cov, dtype=np.float32)
    var = (np.diagonal(cov) + np.float32(1e-2)).astype(np.float64)
    mu = mean.astype(np.float64)
    valid = bool(np.all(np.isfinite(mu)) and np.all(np.isfinite(var)) and np.all(var > 0.0))
    with np.errstate(all="ignore"):
        sd = np.sqrt(var)
        r = np.array([float(cov[1, 0]) / (sd[0] * sd[1]), float(cov[3, 2]) / (sd[2] * sd[3])])
    valid = valid and bool(np.all(np.isfinite(r)))
    rho = np.clip(r, -RHO_MAX, RHO_MAX) if valid else np.zeros(2)
    return mu, sd, rho, valid


def pixel_probs(mean, cov, W, H):
    """P and Q on every pixel of the frame, (H, W) fp64 each; None, None for an invalid detection."""
    mu, sd, rho, valid = corner_blocks(mean, cov)
    if not valid:
        return None, None
    cx = (np.arange(W, dtype=np.float64) + 0.5)[None, :]
    cy = (np.arange(H, dtype=np.float64) + 0.5)[:, None]
    h1, k1 = (cx - mu[0]) / sd[0], (cy - mu[1]) / sd[1]
    h2, k2 = (mu[2] - cx) / sd[2], (mu[3] - cy) / sd[3]
    A, B = phi2(h1, k1, rho[0]), phi2(h2, k2, rho[1])
    Ac, Bc = phi2_complement(h1, k1, rho[0]), phi2_complement(h2, k2, rho[1])
    return A * B, Ac + A * Bc


def gt_segment(box, W, H):
    """(H, W) bool: the pixels whose centre lies in [x1, x2) x [y1, y2) of the fp32 box."""
    b = np.asarray(box, dtype=np.float32).astype(np.float64)
    cx = (np.arange(W, dtype=np.float64) + 0.5)[None, :]
    cy = (np.arange(H, dtype=np.float64) + 0.5)[:, None]
    return (cx >= b[0]) & (cx < b[2]) & (cy >= b[1]) & (cy < b[3])


def pair_ref(P, Q, seg, q_label, p_min=P_MIN):
    """One (ground truth, detection) pair from the detection's P, Q and the ground truth's segment -> dict of the two un-normalised sums,
    the five quantities and the pixel counts entering each sum."""
    zero = {"sum_fg": 0.0, "sum_bg": 0.0, "n_fg": 0, "n_bg": 0, "n_i": int(seg.sum()), **{k: 0.0 for k in PLANES}}
    if P is None or zero["n_i"] == 0:
        return zero
    T = P >= p_min
    if not bool((T & seg).any()):
        return zero
    n_i = zero["n_i"]
    fg_terms = np.where(T, np.log(np.maximum(P, SMALL)), math.log(SMALL))[seg]
    bg_terms = np.log(np.maximum(Q, SMALL))[T & ~seg]
    sum_fg, sum_bg = float(fg_terms.sum()), float(bg_terms.sum())
    l_fg, l_bg = -sum_fg / n_i, -sum_bg / n_i
    q_spatial = math.exp(-(l_fg + l_bg))
    return {"sum_fg": sum_fg, "sum_bg": sum_bg, "n_fg": n_i, "n_bg": int(bg_terms.size), "n_i": n_i, "pPDQ": math.sqrt(q_spatial * q_label),
            "q_spatial": q_spatial, "q_label": float(q_label), "q_fg": math.exp(-l_fg), "q_bg": math.exp(-l_bg)}


def image_ref(frame, means, covs, probs, gt_boxes, gt_classes, p_min=P_MIN):
    """All pairs of one image -> dict of (G, D) arrays (the keys of pair_ref), "invalid" (D,) bool and "margins": the smallest |P - p_min|
    and the smallest |Q / small - 1| over the pixels of every valid detection (the condition on the fixtures)."""
    W, H = frame
    G, D = len(gt_boxes), len(means)
    keys = ("sum_fg", "sum_bg", "n_fg", "n_bg", "n_i") + PLANES
    out = {k: np.zeros((G, D), dtype=np.int64 if k.startswith("n_") else np.float64) for k in keys}
    out["invalid"] = np.zeros(D, dtype=bool)
    segs = [gt_segment(b, W, H) for b in gt_boxes]
    m_p, m_q = math.inf, math.inf
    for j in range(D):
        P, Q = pixel_probs(means[j], covs[j], W, H)
        out["invalid"][j] = P is None
        if P is not None:
            m_p = min(m_p, float(np.abs(P - p_min).min()))
            m_q = min(m_q, float(np.abs(Q[P >= p_min] / SMALL - 1.0).min()) if bool((P >= p_min).any()) else math.inf)
        for i in range(G):
            c = int(gt_classes[i])
            ql = float(np.float32(probs[j][c])) if 0 <= c < len(probs[j]) else 0.0
            for k, v in pair_ref(P, Q, segs[i], ql, p_min).items():
                out[k][i, j] = v
    out["margins"] = (m_p, m_q)
    return out


def assign_ref(q):
    """The kernel's assignment, step for step: shortest augmenting paths with potentials on cost -q over the G real rows against
    n = max(G, D) columns (zero cost past D), ties to the lowest column.  q: (G, D) fp64.  -> match (G,) int: the column of a true positive
    (assigned and q > 0), else -1."""
    q = np.asarray(q, dtype=np.float64)
    G, D = q.shape
    n = max(G, D)
    cost = np.zeros((G + 1, n + 1), dtype=np.float64)
    ok = np.isfinite(q) & (q > 0.0)          # a quality that is not positive and finite counts as 0
    cost[1:, 1:D + 1] = -np.where(ok, q, 0.0)
    u, v = np.zeros(n + 1), np.zeros(n + 1)
    p, way = np.zeros(n + 1, dtype=np.int64), np.zeros(n + 1, dtype=np.int64)
    for i in range(1, G + 1):
        p[0] = i
        minv = np.full(n + 1, np.inf)
        used = np.zeros(n + 1, dtype=bool)
        j0 = 0
        while True:
            used[j0] = True
            i0 = p[j0]
            cur = (cost[i0] - u[i0]) - v
            better = ~used & (cur < minv)
            better[0] = False
            minv[better] = cur[better]
            way[better] = j0
            cand = np.where(used, np.inf, minv)
            cand[0] = np.inf
            j1 = int(np.argmin(cand))          # the first minimum: the lowest column
            delta = cand[j1]
            u[p[used]] += delta                # (the rows of the used columns are distinct)
            v[used] -= delta
            minv[~used] -= delta
            j0 = j1
            if p[j0] == 0:
                break
        while j0 != 0:
            j1 = way[j0]
            p[j0] = p[j1]
            j0 = j1
    match = np.full(G, -1, dtype=np.int64)
    for c in range(1, n + 1):
        if p[c] != 0 and c <= D and ok[p[c] - 1, c - 1]:
            match[p[c] - 1] = c - 1
    return match


def assign_brute(q):
    """The maximum total of q over all assignments of the padded square matrix, by permutations (n <= 8)."""
    q = np.asarray(q, dtype=np.float64)
    G, D = q.shape
    n = max(G, D)
    sq = np.zeros((n, n))
    sq[:G, :D] = q
    return max(sum(sq[i, perm[i]] for i in range(n)) for perm in itertools.permutations(range(n)))


def image_totals(planes, match):
    """counts (TP, FP, FN) and the five sums over the true positives in ground-truth order; planes: dict of (G, D) arrays."""
    G, D = planes["pPDQ"].shape
    s = [0.0] * 5
    tp = 0
    for i in range(G):
        if match[i] >= 0:
            tp += 1
            for k, name in enumerate(PLANES):
                s[k] += float(planes[name][i, match[i]])
    return (tp, D - tp, G - tp), s


def dataset_ref(images, p_min=P_MIN):
    """images: list of dicts frame, means, covs, probs, gt_boxes, gt_classes (numpy; empty arrays for none) -> the result dict
    evaluation_utils.pdq_scores returns."""
    tp = fp = fn = invalid = 0
    s = [0.0] * 5
    for im in images:
        r = image_ref(im["frame"], im["means"], im["covs"], im["probs"], im["gt_boxes"], im["gt_classes"], p_min)
        (a, b, c), si = image_totals(r, assign_ref(r["pPDQ"]))
        tp, fp, fn = tp + a, fp + b, fn + c
        invalid += int(r["invalid"].sum())
        s = [x + y for x, y in zip(s, si)]
    den = tp + fp + fn
    mean = lambda x: x / tp if tp else 0.0
    return {"PDQ": s[0] / den if den else 0.0, "avg_pPDQ": mean(s[0]), "avg_spatial": mean(s[1]), "avg_label": mean(s[2]), "avg_fg": mean(s[3]),
            "avg_bg": mean(s[4]), "TP": tp, "FP": fp, "FN": fn, "invalid_detections": invalid}
