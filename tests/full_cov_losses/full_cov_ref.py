"""fp64 torch restatement of the three objectives of K28 -- the Gaussian NLL, moment matching and the energy score of the FULL box
covariance -- as include/pod_mi355x.h defines them: the referee of the K28 tests, differentiated by autograd.  The analytic derivatives the
header states are restated beside the losses (test_full_cov_losses_cpu.py holds them against autograd), and so is the count of the terms
whose sign fp32 and fp64 may decide differently: at beta = 0 one such sign moves a gradient by 2 / M or more, so a test first asserts that
it meets none.  The fixture holds four reg_var channels; the six off-diagonal ones are made here from a seed."""
import torch

from tests.score_losses import score_ref as sr
from tests.training import loss_ref as lr

K, A = sr.K, sr.A
OFF_SEED = 2803          # (2801, 2802 and 2805 do meet undecided terms at M = 1000 on this fixture)
TINY = 2.0 ** -18        # an order above fp32's worst relative error on a five-term sum
T = torch.tril_indices(4, 4, -1)          # (1,0) (2,0) (2,1) (3,0) (3,1) (3,2): channels 4 .. 9, the order cholesky_from_head reads
LOWER = torch.tril_indices(4, 4, 0)
replay_normals = sr.replay_normals


def off_diagonals(reg_var, seed=OFF_SEED):
    """(2, 1161, 4) fp32 log-variances -> the six off-diagonal channels, (2, 1161, 6) fp32: 0.5 sqrt(s_i s_j) n_k, (i, j) = T[k]."""
    n = torch.randn((2, 1161, 6), generator=torch.Generator().manual_seed(seed), dtype=torch.float32)
    s = torch.exp(0.5 * torch.clamp(reg_var.float(), -7.0, 7.0))
    return 0.5 * torch.sqrt(s[..., T[0]] * s[..., T[1]]) * n


def full_case(fx, images=(0, 1), seed=OFF_SEED, zero_off=False):
    """score_ref.fixture_case with ten reg_var channels: the fixture's four, then the seeded off-diagonals (zeros with zero_off)."""
    case = sr.fixture_case(fx, images)
    off = off_diagonals(torch.from_numpy(fx["reg_var"]), seed)[list(images)]
    case["reg_var"] = torch.cat([case["reg_var"], torch.zeros_like(off) if zero_off else off], dim=-1).contiguous()
    return case


def sl1_prime(u, beta):
    return sr.sl1_prime(u, beta)


class Referee:
    """One case in `dtype` (fp64: the referee; fp32: what the bar leaves to a kernel).  delta (N, R, 4) / rv (N, R, 10) are leaves unless
    given (then any tensors of the same shapes, e.g. a head's outputs); `std` is the standard regression sum pod_train_loss adds to the
    same delta planes."""

    def __init__(self, case, beta=0.0, weights=(1.0, 1.0, 1.0, 1.0), dtype=torch.float64, delta=None, rv=None):
        self.beta, self.dtype = beta, dtype
        self.delta = case["delta"].to(dtype).clone().requires_grad_(True) if delta is None else delta
        self.rv = case["reg_var"].to(dtype).clone().requires_grad_(True) if rv is None else rv
        assert self.rv.shape[-1] == 10
        labels, matched = case["labels"].long(), case["matched_gt"].long()
        self.pos = (labels >= 0) & (labels < K) & (matched >= 0)
        boxes = case["gt_boxes"].to(dtype)[matched.clamp(min=0)]
        anchors = case["anchors"].to(dtype)[None].expand_as(boxes)
        self.t = lr.get_deltas(anchors[self.pos], boxes[self.pos], weights)          # (P, 4)
        self.d = self.delta[self.pos] - self.t
        rvp = self.rv[self.pos]
        self.c = torch.clamp(rvp[:, :4], -7.0, 7.0)
        self.inside = ((rvp[:, :4] >= -7.0) & (rvp[:, :4] <= 7.0)).detach()
        L = torch.diag_embed(torch.exp(0.5 * self.c))
        self.L = L.index_put((torch.arange(L.shape[0])[:, None], T[0][None], T[1][None]), rvp[:, 4:])      # (P, 4, 4)
        self.std = lr.smooth_l1(self.d, beta).sum()

    def positive_normals(self, eps):
        """dense (M + 1, N*R, 4) -> (M + 1, P, 4)"""
        return eps.to(self.dtype).view(eps.shape[0], *self.pos.shape, 4)[:, self.pos]

    def chain(self, g_L):
        """d / d L (P, 4, 4) -> d / d rv (P, 10): the diagonal through L_jj = exp(0.5 clamp(rv_j)), the strict lower triangle as it is."""
        L = self.L.detach()
        diag = 0.5 * torch.diagonal(L, dim1=-2, dim2=-1) * torch.diagonal(g_L, dim1=-2, dim2=-1) * self.inside
        return torch.cat([diag, g_L[:, T[0], T[1]]], dim=-1)

    # ---- POD_FULL_COV_NLL
    def nll(self):
        y = torch.linalg.solve_triangular(self.L, self.d[..., None], upper=False)[..., 0]
        return (0.5 * (y * y).sum(-1) + 0.5 * self.c.sum(-1)).sum()

    def nll_analytic(self):
        """(d / d delta (P, 4), d / d rv (P, 10)) as the header states them."""
        L, d = self.L.detach(), self.d.detach()
        y = torch.linalg.solve_triangular(L, d[..., None], upper=False)
        q = torch.linalg.solve_triangular(L.transpose(-1, -2), y, upper=True)[..., 0]
        y = y[..., 0]
        diag = 0.5 * (1.0 - torch.diagonal(L, dim1=-2, dim2=-1) * q * y) * self.inside
        return q, torch.cat([diag, -(q[:, T[0]] * y[:, T[1]])], dim=-1)

    # ---- POD_FULL_COV_MOMENTS
    def moments(self):
        S = self.L @ self.L.transpose(-1, -2)
        E = S - self.d[:, :, None] * self.d[:, None, :]
        return lr.smooth_l1(self.d, self.beta).sum() + lr.smooth_l1(E[:, LOWER[0], LOWER[1]], self.beta).sum()

    def moments_analytic(self):
        L, d = self.L.detach(), self.d.detach()
        E = L @ L.transpose(-1, -2) - d[:, :, None] * d[:, None, :]
        m = torch.tril(sl1_prime(E, self.beta))
        G = m + m.transpose(-1, -2)                           # the symmetric extension plus the diagonal once more
        g_delta = sl1_prime(d, self.beta) - (G @ d[..., None])[..., 0]
        return g_delta, self.chain(torch.tril(G @ L))

    def moments_undecided(self):
        """(terms within TINY of a sign change relative to the sum of their terms' magnitudes, the smallest ratio)"""
        L, d = self.L.detach(), self.d.detach()
        E = (L @ L.transpose(-1, -2) - d[:, :, None] * d[:, None, :])[:, LOWER[0], LOWER[1]]
        mag = (L.abs() @ L.abs().transpose(-1, -2) + d.abs()[:, :, None] * d.abs()[:, None, :])[:, LOWER[0], LOWER[1]]
        a = E.abs() / mag
        b = d.abs() / (self.delta[self.pos].detach().abs() + self.t.abs())
        return int((a < TINY).sum() + (b < TINY).sum()), float(torch.minimum(a.min(), b.min()))

    # ---- POD_FULL_COV_ENERGY
    def _samples(self, eps, L, d):
        e = self.positive_normals(eps)
        m = e.shape[0] - 1
        de = e[:m] - e[1:]
        u1 = d[None] + torch.einsum("pjk,spk->spj", L, e[:m])
        u2 = torch.einsum("pjk,spk->spj", L, de)
        return m, e[:m], de, u1, u2

    def energy(self, eps):
        m, _, _, u1, u2 = self._samples(eps, self.L, self.d)
        return (2.0 * lr.smooth_l1(u1, self.beta).sum() - lr.smooth_l1(u2, self.beta).sum()) / m

    def energy_analytic(self, eps):
        m, e, de, u1, u2 = self._samples(eps, self.L.detach(), self.d.detach())
        p1, p2 = sl1_prime(u1, self.beta), sl1_prime(u2, self.beta)
        g_delta = (2.0 / m) * p1.sum(0)
        g_L = (2.0 / m) * torch.einsum("spj,spk->pjk", p1, e) - (1.0 / m) * torch.einsum("spj,spk->pjk", p2, de)
        return g_delta, self.chain(torch.tril(g_L))

    def energy_undecided(self, eps):
        L, d = self.L.detach(), self.d.detach()
        m, e, de, u1, u2 = self._samples(eps, L, d)
        a = u1.abs() / (d.abs()[None] + torch.einsum("pjk,spk->spj", L.abs(), e.abs()))
        mag2 = torch.einsum("pjk,spk->spj", L.abs(), de.abs())
        b = u2.abs() / mag2.clamp(min=1e-300)
        return int((a < TINY).sum() + (b < TINY).sum()), float(torch.minimum(a.min(), b.min()))

    def gradients(self, total):
        """autograd of `total` -> (d / d delta (N, R, 4), d / d rv (N, R, 10))"""
        g = torch.autograd.grad(total, (self.delta, self.rv), allow_unused=True, retain_graph=True)
        return tuple(torch.zeros_like(x) if y is None else y for x, y in zip((self.delta, self.rv), g))
