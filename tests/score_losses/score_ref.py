"""fp64 torch restatement of the two box-covariance objectives of K27, `second_moment_matching` and `energy_loss`, as
include/pod_mi355x.h defines them: the referee of the K27 tests, differentiated by autograd.  The analytic derivatives the header states are
restated beside it (test_score_losses_cpu.py holds them against autograd), and so is the count of the terms whose sign fp32 and fp64 may
decide differently: at beta = 0 one such sign moves a gradient by 4 / M, above the bar, so a test first asserts that it meets none."""
import torch

from tests.training import loss_ref as lr

K, A = 7, 9
EPS_SEED = 2703          # (2702 and 2704 do meet undecided terms on this fixture)
TINY = 2.0 ** -16


def replay_normals(m, n_rows=2 * 1161, seed=EPS_SEED):
    """The dense (M + 1, N*R, 4) fp32 normals a test replays, made on the CPU."""
    return torch.randn((m + 1, n_rows, 4), generator=torch.Generator().manual_seed(seed), dtype=torch.float32)


def fixture_case(fx, images=(0, 1)):
    """The fixture's images as a case: fp32 head outputs (N, R, C) anchor-major, labels / matched_gt int32 (N, R), the boxes."""
    idx = list(images)
    t = lambda k: torch.from_numpy(fx[k])[idx].contiguous()
    return dict(cls=t("cls"), delta=t("delta"), reg_var=t("reg_var"), labels=t("labels"), matched_gt=t("matched_gt"),
                gt_boxes=torch.from_numpy(fx["gt_boxes"]), anchors=torch.from_numpy(fx["anchors"]))


def sl1_prime(u, beta):
    return torch.sign(u) if beta < 1e-5 else torch.where(u.abs() < beta, u / beta, torch.sign(u))


class Referee:
    """One case in fp64.  delta / lv are leaves; `std` is the standard regression sum pod_train_loss adds to the same delta planes."""

    def __init__(self, case, beta=0.0, weights=(1.0, 1.0, 1.0, 1.0)):
        self.beta = beta
        self.delta = case["delta"].double().clone().requires_grad_(True)
        self.lv = case["reg_var"].double().clone().requires_grad_(True)
        labels, matched = case["labels"].long(), case["matched_gt"].long()
        self.pos = (labels >= 0) & (labels < K) & (matched >= 0)
        boxes = case["gt_boxes"].double()[matched.clamp(min=0)]
        anchors = case["anchors"].double()[None].expand_as(boxes)
        self.t = lr.get_deltas(anchors[self.pos], boxes[self.pos], weights)          # (P, 4)
        self.d = self.delta[self.pos] - self.t
        self.c = torch.clamp(self.lv[self.pos], -7.0, 7.0)
        self.inside = ((self.lv[self.pos] >= -7.0) & (self.lv[self.pos] <= 7.0)).detach()
        self.std = lr.smooth_l1(self.d, beta).sum()

    def positive_normals(self, eps):
        """dense (M + 1, N*R, 4) -> (M + 1, P, 4) fp64"""
        return eps.double().view(eps.shape[0], *self.pos.shape, 4)[:, self.pos]

    # ---- second_moment_matching
    def moments(self):
        v = torch.exp(self.c)
        return (lr.smooth_l1(self.d, self.beta) + lr.smooth_l1(v - self.d ** 2, self.beta)).sum()

    def moments_analytic(self):
        """(d / d delta, d / d lv) at the positives, (P, 4) each, as the header states them."""
        d, v = self.d.detach(), torch.exp(self.c.detach())
        m = sl1_prime(v - d ** 2, self.beta)
        return sl1_prime(d, self.beta) - 2.0 * d * m, m * v * self.inside

    def moments_undecided(self):
        d, v = self.d.detach(), torch.exp(self.c.detach())
        a = (v - d ** 2).abs() / (v + d ** 2)
        b = d.abs() / (self.delta[self.pos].detach().abs() + self.t.abs())
        return int(((a < TINY) | (b < TINY)).sum()), float(a.min()), float(b.min())

    # ---- energy_loss
    def energy(self, eps):
        e = self.positive_normals(eps)
        m = e.shape[0] - 1
        sg = torch.exp(0.5 * self.c)
        z = self.delta[self.pos][None] + sg[None] * e
        first = lr.smooth_l1(z[:m] - self.t[None], self.beta).sum()
        second = lr.smooth_l1(sg[None] * (e[:m] - e[1:]), self.beta).sum()
        return (2.0 * first - second) / m

    def energy_analytic(self, eps):
        e = self.positive_normals(eps)
        m = e.shape[0] - 1
        d, sg = self.d.detach(), torch.exp(0.5 * self.c.detach())
        p1 = sl1_prime(d[None] + sg[None] * e[:m], self.beta)
        de = e[:m] - e[1:]
        p2 = sl1_prime(sg[None] * de, self.beta)
        g_delta = (2.0 / m) * p1.sum(0)
        g_lv = 0.5 * sg * ((2.0 / m) * (p1 * e[:m]).sum(0) - (1.0 / m) * (p2 * de).sum(0)) * self.inside
        return g_delta, g_lv

    def energy_undecided(self, eps):
        e = self.positive_normals(eps)
        m = e.shape[0] - 1
        d, sg = self.d.detach(), torch.exp(0.5 * self.c.detach())
        ratio = (d[None] + sg[None] * e[:m]).abs() / (d.abs()[None] + sg[None] * e[:m].abs())
        return int(((ratio < TINY) | (e[:m] == e[1:])).sum()), float(ratio.min())

    def gradients(self, total):
        """autograd of `total` -> (d / d delta, d / d lv), (N, R, 4) each"""
        g = torch.autograd.grad(total, (self.delta, self.lv), allow_unused=True, retain_graph=True)      # (d and c are shared by every sum)
        return tuple(torch.zeros_like(self.delta) if x is None else x for x in g)
