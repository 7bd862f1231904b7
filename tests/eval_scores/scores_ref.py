"""Referees of tests/eval_scores/: the evaluation's bounded scoring rules (include/pod_mi355x.h, K33) in fp64 on the CPU, and the host
restatement of the kernel's draws.  Not a test.

  energy_ref          (1 / M) sum_s |(mean - gt) + L eps_s| - (1 / (2 M)) sum_s |L (eps_s - eps_{s+1})| from GIVEN fp32 normals, L the factor of
                      instrument_ref.nll_factor; the difference of the normals is taken in fp32 and then widened, as the kernel takes it
  crps_ref            the Gaussian CRPS's closed form per coordinate, averaged over the four
  brier_rows          2 (1 - p)^2
  eval_score_normals  (word, which) of every normal of rows `rows`: samples 2c and 2c + 1 of row i are components 0..3 and 4..7 of the
                      Philox4x32-10 call with counter (i, 0, c, STREAM_EVAL_SCORE)
  host_normals        those normals through rng_ref.box_muller16 (fp64), rounded to fp32: the draws without a GPU
  ENERGY_UNIT         the energy score's expectation at Sigma = s^2 I, gt = mean, per unit s
  result_set          a small result file and its ground truth for the drivers"""
import math

import numpy as np
import torch

from tests.eval_instrument import instrument_ref as ir
from tests.rng import rng_ref as rr

STREAM_EVAL_SCORE = 0x65767300          # "evs"
BOUND = 2.0 ** -22                      # per row, relative to max(1, |ref|): test_nll_gpu.py derives it
# E |X - y| - 0.5 E |X - X'| for X, X' ~ N(y, s^2 I_4): E |X - y| = s sqrt(2) Gamma(2.5) / Gamma(2), E |X - X'| = sqrt(2) times that
ENERGY_UNIT = math.sqrt(2.0) * math.gamma(2.5) / math.gamma(2.0) * (1.0 - 1.0 / math.sqrt(2.0))
# the anchor's fixed case: test_eval_scores_cpu.py shows that the host referee meets the 5-standard-error condition under this seed
ANCHOR_SEED, ANCHOR_N, ANCHOR_M, ANCHOR_VARIANCES, ANCHOR_SIGMAS = 20260133, 4096, 1000, (1.0, 25.0), 5.0


def energy_ref(means: torch.Tensor, covs: torch.Tensor, gt: torch.Tensor, eps: torch.Tensor) -> torch.Tensor:
    """eps: (M + 1, n, 4) fp32.  (n,) fp64."""
    assert eps.dtype == torch.float32 and eps.dim() == 3 and eps.shape[0] >= 2
    L = ir.nll_factor(covs)
    d = means.double() - gt.double()
    through = lambda v: torch.einsum("nij,snj->sni", L, v.double())
    u1 = d.unsqueeze(0) + through(eps[:-1])
    u2 = through(eps[:-1] - eps[1:])                      # the fp32 difference, then fp64
    return u1.norm(dim=-1).mean(0) - 0.5 * u2.norm(dim=-1).mean(0)


def crps_ref(means: torch.Tensor, covs: torch.Tensor, gt: torch.Tensor) -> torch.Tensor:
    """(n,) fp64: (1/4) sum_j sd_j [z_j (2 Phi(z_j) - 1) + 2 phi(z_j) - 1 / sqrt(pi)], sd_j^2 the diagonal of cov + 1e-2 I (fp32 sum)."""
    sd = torch.sqrt(torch.diagonal(ir.nll_sigma(covs), dim1=-2, dim2=-1))
    z = (gt.double() - means.double()) / sd
    pdf = torch.exp(-0.5 * z * z) / math.sqrt(2.0 * math.pi)
    return (sd * (z * torch.special.erf(z / math.sqrt(2.0)) + 2.0 * pdf - 1.0 / math.sqrt(math.pi))).mean(-1)


def brier_rows(p: torch.Tensor) -> torch.Tensor:
    return 2.0 * (1.0 - p.double()) ** 2


def eval_score_addr(rows, M):
    """(M + 1, n, 4): the counter (.., 4) uint32 and the component 0..7 of every normal."""
    r = np.asarray(rows, dtype=np.uint64).reshape(1, -1, 1)
    s = np.arange(M + 1, dtype=np.uint64)[:, None, None]
    j = np.arange(4, dtype=np.uint64)[None, None, :]
    comp = np.broadcast_to((s & np.uint64(1)) * np.uint64(4) + j, (M + 1, r.shape[1], 4))
    return rr._finish([r, np.uint64(0), s >> np.uint64(1)], comp, STREAM_EVAL_SCORE)


def eval_score_normals(key, rows, M):
    return rr._words(*eval_score_addr(rows, M), key)


def host_normals(key, rows, M) -> torch.Tensor:
    word, which = eval_score_normals(key, rows, M)
    n0, n1 = rr.box_muller16(word)
    return torch.from_numpy(np.where(which == 0, n0, n1).astype(np.float32))


def anchor_case(variance: float, n: int = ANCHOR_N):
    """(means, covs, gt) with cov + 1e-2 I = variance * I and gt = mean."""
    g = torch.Generator().manual_seed(7)
    means = (300.0 + 50.0 * torch.randn(n, 4, dtype=torch.float64, generator=g)).float()
    covs = ((variance - 1e-2) * torch.eye(4, dtype=torch.float64)).float().expand(n, 4, 4).contiguous()
    return means, covs, means.clone()


def anchor_deviation(rows: torch.Tensor, variance: float):
    """(mean of the rows, closed form, standard error from the rows' own sample deviation, deviation in standard errors)."""
    rows = rows.double()
    want = ENERGY_UNIT * math.sqrt(variance)
    se = float(rows.std(unbiased=True)) / math.sqrt(rows.numel())
    return float(rows.mean()), want, se, (float(rows.mean()) - want) / se


def result_set(seed=5, nd=(40, 64, 9, 30, 0, 25), ng=(6, 9, 2, 5, 3, 4), K=7):
    """(predicted instances, ground-truth annotations) in the result file's format, from instrument_ref.random_set's boxes; the class
    probabilities lie in [0.05, 0.95], so that every ignorance score is finite."""
    c = ir.random_set(seed, list(nd), list(ng), K=K)
    rng = np.random.default_rng(seed)
    xywh = lambda b: [float(b[0]), float(b[1]), float(b[2] - b[0]), float(b[3] - b[1])]
    predicted, gt = [], []
    for key in c["pb"]:
        probs = (0.05 + 0.9 * rng.random((c["pb"][key].shape[0], K))).astype(np.float32)
        for b, cov, p in zip(c["pb"][key].tolist(), c["pc"][key].tolist(), probs.tolist()):
            predicted.append({"image_id": key, "category_id": int(np.argmax(p)) + 1, "bbox": xywh(b), "score": max(p), "cls_prob": p, "bbox_covar": cov})
        if key in c["gb"]:
            for b, cat in zip(c["gb"][key].tolist(), c["gc"][key].reshape(-1).tolist()):
                gt.append({"image_id": key, "category_id": int(cat), "bbox": xywh(b)})
    return predicted, gt
