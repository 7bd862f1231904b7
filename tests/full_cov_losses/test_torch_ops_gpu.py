"""K28 on the GPU: pod_full_cov_loss -- the Gaussian NLL, moment matching and the energy score of the full box covariance -- against the
fp64 referee and its autograd (tests/full_cov_losses/full_cov_ref.py), on the K21 fixture: a 64 x 96 frame, R = 1161, K = 7, two images
(the second without ground truth), 81 positives, 19 of their 324 diagonal log-variances outside the clamp; the six off-diagonal channels
come from seed 2803.  Bounds: the project's bar 1e-4 max(1, |ref|) (tests/helpers.py); zeros, untouched elements, draws and
repeatability exact.  Replayed normals come from seed 2703; test_full_cov_losses_cpu.py asserts that fp32 torch uses at most a quarter of
the bar on these inputs and that no term's sign is within 2^-18 of a change."""
import copy

import pytest
import torch

from pod_compare_amd import anchors as _anchors, losses, modeling
from pod_compare_amd.head_train import head_convs
from tests.full_cov_losses import full_cov_ref as fr
from tests.head_backward import hb
from tests.helpers import assert_close
from tests.training import loss_ref as lr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
K, A, R = fr.K, fr.A, 1161
KINDS = ("negative_log_likelihood", "second_moment_matching", "energy_loss")


@pytest.fixture(scope="module")
def fx():
    f = lr.load_fixture()
    f["shapes"], f["level_anchors"] = lr.fixture_geometry(f)
    return f


@pytest.fixture(scope="module")
def normals():
    made = {}
    return lambda m: made.setdefault(m, fr.replay_normals(m))


def planes(fx, x):
    return [p.to(DEV).contiguous() for p in lr.to_planes(x, fx["shapes"], A)]


def run(fx, case, kind, beta, m=0, eps=None, eps_out=None, seed=0, diagonal=False):
    """The two-launch composition on a case: pod_train_loss without the reg_var planes, then pod_full_cov_loss on its planes, w = 1
    (diagonal: pod_reg_score_loss, K27, on the four diagonal channels of the same case).  Returns dict(sums double[4] of the first launch,
    total double[1], base = the delta planes the first launch alone left, g_delta, g_reg_var), anchor-major on the CPU."""
    D = 4 if diagonal else 10
    cls, delta, reg_var = planes(fx, case["cls"]), planes(fx, case["delta"]), planes(fx, case["reg_var"][..., :D].contiguous())
    labels, matched, gb = case["labels"].to(DEV), case["matched_gt"].to(DEV), case["gt_boxes"].to(DEV)
    anchors = [a.to(DEV) for a in fx["level_anchors"]]
    w = torch.ones(3, device=DEV)
    sums, grads = losses.train_loss_sums(cls, delta, None, None, labels, matched, gb, anchors, A, K, beta=beta, w=w, want_grads=True)
    base = lr.from_planes([p.cpu() for p in grads[1]], 4)
    second = losses.reg_score_sum if diagonal else losses.full_cov_sum
    total, grads = second(cls, delta, None, reg_var, labels, matched, gb, anchors, A, K, kind=kind, num_samples=m, beta=beta,
                          eps_reg=None if eps is None else eps.to(DEV), eps_reg_out=eps_out, w=w, grads=grads, seed=seed)
    assert all(tuple(p.shape[1:2]) == (A * D,) for p in grads[3])
    return dict(sums=sums.cpu(), total=total.cpu(), base=base, g_delta=lr.from_planes([p.cpu() for p in grads[1]], 4),
                g_reg_var=lr.from_planes([p.cpu() for p in grads[3]], D))


def check_against(ref, total, got, what):
    """Value and both planes against the referee's sum `total`; exact zeros and untouched elements where no positive anchor is."""
    g_delta, g_rv = ref.gradients(ref.std + total)
    assert_close(got["sums"][1], ref.std.detach(), what + " std_reg_sum")
    print(what, "score sum", float(got["total"][0]), "ref", float(total.detach()))
    for name, x, want in (("g_delta", got["g_delta"], g_delta), ("g_reg_var", got["g_reg_var"], g_rv)):
        print(what, name, "max |ref|", float(want.abs().max()), "max |err|", float((x.double() - want).abs().max()),
              "worst fraction of the bar", float(((x.double() - want).abs() / (1e-4 * want.abs().clamp(min=1.0))).max()))
    assert_close(got["total"][0], total.detach(), what + " score sum")
    assert_close(got["g_delta"], g_delta, what + " g_delta")
    for k in range(10):
        assert_close(got["g_reg_var"][..., k], g_rv[..., k], what + " g_reg_var channel %d" % k)
    assert tuple(got["g_reg_var"].shape[-1:]) == (10,)
    assert bool((got["g_reg_var"][~ref.pos] == 0).all()) and bool((got["g_reg_var"][ref.pos] != 0).any())       # exactly 0 on all ten channels
    assert torch.equal(got["g_delta"][~ref.pos], got["base"][~ref.pos])                    # bit-equal to what pod_train_loss alone left
    assert not torch.equal(got["g_delta"][ref.pos], got["base"][ref.pos])


def check_the_clamp(ref, got):
    """The 19 out-of-clamp diagonal entries have gradient exactly 0; the off-diagonal gradients of the same anchors are not all zero."""
    at_pos = got["g_reg_var"][ref.pos]
    outside = at_pos[:, :4][~ref.inside]
    assert int((~ref.inside).sum()) == 19 and outside.numel() == 19 and bool((outside == 0).all())
    assert bool((at_pos[(~ref.inside).any(-1)][:, 4:] != 0).any())


def test_nll_equals_fp64_autograd(fx):
    case = fr.full_case(fx)
    ref = fr.Referee(case, 0.0)
    got = run(fx, case, "negative_log_likelihood", 0.0)             # (num_samples = 0: checked for the energy kind only)
    check_against(ref, ref.nll(), got, "nll")
    check_the_clamp(ref, got)
    again = run(fx, case, "none", 0.0, m=-5)                         # `none` with a covariance head is the NLL
    assert all(torch.equal(got[k], again[k]) for k in ("total", "g_delta", "g_reg_var"))


@pytest.mark.parametrize("beta", [0.0, 0.11])
def test_moment_matching_equals_fp64_autograd(fx, beta):
    case = fr.full_case(fx)
    ref = fr.Referee(case, beta)
    assert ref.moments_undecided()[0] == 0
    got = run(fx, case, "second_moment_matching", beta)
    check_against(ref, ref.moments(), got, "moments beta=%g" % beta)
    check_the_clamp(ref, got)


@pytest.mark.parametrize("beta", [0.0, 0.11])
@pytest.mark.parametrize("m", [7, 64, 1000])
def test_energy_score_equals_fp64_autograd(fx, normals, m, beta):
    """M = 7: an odd count below one wavefront; 64: the pair (63, 64) crosses the lane range; 1000: the default, a ragged last trip."""
    case, eps = fr.full_case(fx), normals(m)
    ref = fr.Referee(case, beta)
    assert ref.energy_undecided(eps)[0] == 0
    got = run(fx, case, "energy_loss", beta, m, eps)
    check_against(ref, ref.energy(eps), got, "energy M=%d beta=%g" % (m, beta))
    check_the_clamp(ref, got)


@pytest.mark.parametrize("kind", KINDS)
def test_every_anchor_positive_beside_an_image_without_positives(fx, kind):
    """Three images: the fixture's two, and image 0's head outputs labelled against the fixture's boxes plus one wholly off every
    anchor's reach -- its best IoU of 0 promotes all 1161 anchors: full positive lists in every workgroup next to image 1's empty ones."""
    gb, gc = torch.from_numpy(fx["gt_boxes"]), torch.from_numpy(fx["gt_classes"]).long()
    sets = [(gb, gc), (gb[:0], gc[:0]), (torch.cat([gb, torch.tensor([lr.FAR_BOX])]), torch.cat([gc, torch.tensor([1])]))]
    labels, matched, num_pos = losses.label_anchors([a.to(DEV) for a in fx["level_anchors"]], [b for b, _ in sets], [c for _, c in sets], K)
    assert num_pos.cpu().tolist() == [81, 0, 1161]
    case = fr.full_case(fx, images=(0, 1, 0))
    case["labels"], case["matched_gt"] = labels.cpu(), matched.cpu()
    case["gt_boxes"] = torch.cat([b for b, _ in sets])
    assert torch.equal(case["labels"][:2], torch.from_numpy(fx["labels"]))
    beta, m = 0.11, 7                                     # (a continuous derivative: no sign condition at this size)
    ref = fr.Referee(case, beta)
    assert int(ref.pos.sum()) == 81 + 1161
    eps = fr.replay_normals(m, n_rows=3 * R)
    energy = kind == "energy_loss"
    got = run(fx, case, kind, beta, m if energy else 0, eps if energy else None)
    total = ref.energy(eps) if energy else ref.nll() if kind == "negative_log_likelihood" else ref.moments()
    check_against(ref, total, got, kind + " all positive")


def test_native_draws_are_k27s_and_refereed_on_their_own_normals(fx):
    case, m, beta = fr.full_case(fx), 1000, 0.11
    ref = fr.Referee(case, beta)

    def native(seed, diagonal=False):
        eps_out = torch.full((m + 1, 2 * R, 4), float("nan"), device=DEV)
        got = run(fx, case, "energy_loss", beta, m, eps_out=eps_out, seed=seed, diagonal=diagonal)
        return got, eps_out.cpu()

    g1, e1 = native(11)
    g2, e2 = native(11)
    g3, e3 = native(12)
    assert torch.equal(g1["total"], g2["total"]) and torch.equal(e1, e2)                    # the same seed: the same bits
    assert torch.equal(g1["g_delta"], g2["g_delta"]) and torch.equal(g1["g_reg_var"], g2["g_reg_var"])
    assert not torch.equal(e1, e3) and float(g1["total"]) != float(g3["total"])            # another seed: other draws
    rows = ref.pos.reshape(-1)
    assert bool(torch.isfinite(e1).all()) and bool((e1[:, ~rows] == 0).all()) and bool((e1[:, rows] != 0).any())
    _, e27 = native(11, diagonal=True)
    assert torch.equal(e1, e27)                                                             # what pod_reg_score_loss draws under this seed
    check_against(ref, ref.energy(e1), g1, "energy on the kernel's own draws")


def test_draws_do_not_depend_on_the_batch(fx):
    """Image 0 alone gives the normals and the per-anchor gradient bits it gives inside the two-image call."""
    m, beta, seed = 64, 0.11, 5
    both, alone = fr.full_case(fx), fr.full_case(fx, images=(0,))
    e_both = torch.full((m + 1, 2 * R, 4), float("nan"), device=DEV)
    e_alone = torch.full((m + 1, R, 4), float("nan"), device=DEV)
    g_both = run(fx, both, "energy_loss", beta, m, eps_out=e_both, seed=seed)
    g_alone = run(fx, alone, "energy_loss", beta, m, eps_out=e_alone, seed=seed)
    assert torch.equal(e_both[:, :R].cpu(), e_alone.cpu()) and bool((e_alone != 0).any())
    assert torch.equal(g_both["g_delta"][0], g_alone["g_delta"][0]) and torch.equal(g_both["g_reg_var"][0], g_alone["g_reg_var"][0])
    assert torch.equal(g_both["total"], g_alone["total"])                                   # (image 1 has no positive: it adds exact zeros)


@pytest.mark.parametrize("beta", [0.0, 0.11])
def test_zero_off_diagonals_agree_with_the_referee_and_with_k27(fx, normals, beta):
    """Moment matching and the energy score at zero off-diagonals stay within the bar of the referee; the energy sum, its delta gradients
    and its four diagonal gradients within the bar of K27's on the four-channel slice (not bit-equal: the sums are formed differently)."""
    case, m = fr.full_case(fx, zero_off=True), 64
    eps = normals(m)
    ref = fr.Referee(case, beta)
    assert ref.moments_undecided()[0] == 0 and ref.energy_undecided(eps)[0] == 0
    check_against(ref, ref.moments(), run(fx, case, "second_moment_matching", beta), "moments, zero off-diagonals, beta=%g" % beta)
    got = run(fx, case, "energy_loss", beta, m, eps)
    check_against(ref, ref.energy(eps), got, "energy, zero off-diagonals, beta=%g" % beta)
    k27 = run(fx, case, "energy_loss", beta, m, eps, diagonal=True)
    assert_close(got["total"][0], k27["total"][0].double(), "energy sum against K27's")
    assert_close(got["g_delta"], k27["g_delta"].double(), "energy g_delta against K27's")
    assert_close(got["g_reg_var"][..., :4], k27["g_reg_var"].double(), "energy diagonal g_reg_var against K27's")


# ---- the head's backward at a predictor width of 90 -------------------------------------------------------------------------------
LEVELS, B, C = [(12, 20), (6, 10), (3, 5)], 2, 64          # tests/head_backward/test_torch_ops_gpu.py's plan


def test_head_backward_with_a_full_covariance_head():
    """head.forward_train on a head with bbox_cov_dims = 10, a full-covariance loss, backward(): bbox_cov's weight and bias gradients (90
    output channels, padded to 128 -- the one width besides 36 and 63 the head's backward has run at) against torch autograd of the same
    head and the referee's loss, under tests/head_backward/hb.py's bounds."""
    torch.manual_seed(0)
    head = modeling.ProbabilisticRetinaNetHead(in_channels=C, num_classes=K, dropout_rate=0.0, compute_cls_var=False, compute_bbox_cov=True,
                                               bbox_cov_dims=10)
    for conv in head_convs(head):
        torch.nn.init.normal_(conv.weight, std=0.05)
        torch.nn.init.normal_(conv.bias, std=0.1)
    head = head.to(DEV)
    assert head.bbox_cov.out_channels == 90
    g = torch.Generator().manual_seed(1)
    feats = [torch.randn((B, C, h, w), generator=g).to(DEV) for h, w in LEVELS]
    level_anchors = _anchors.grid_anchors(LEVELS)
    frame = (LEVELS[0][0] * 8, LEVELS[0][1] * 8)
    gb = torch.tensor([[10.0, 8.0, 70.0, 60.0], [90.0, 30.0, 150.0, 90.0], [40.0, 20.0, 56.0, 44.0]])
    gc = torch.tensor([1, 4, 2])
    dev_anchors = [a.to(DEV) for a in level_anchors]
    labels, matched, num_pos = losses.label_anchors(dev_anchors, [gb, gb[:1]], [gc, gc[:1]], K)
    boxes = torch.cat([gb, gb[:1]])
    assert int(num_pos.sum()) >= 8
    crit = losses.ProbabilisticLosses(num_classes=K, annealing_step=80000, bbox_cov_loss="negative_log_likelihood")
    crit.current_step = 40000
    lam, norm = lr.annealing_lambda(40000, 80000), float(num_pos.sum())
    out = head.forward_train(feats, dev_anchors, frame)
    assert [int(t.shape[1]) for t in out.reg_var] == [90] * len(LEVELS)
    res = crit(out, labels, matched, boxes.to(DEV), normalizer=norm)
    res["loss_box_reg"].backward()
    grads = {}
    for dtype in (torch.float32, torch.float64):
        h = copy.deepcopy(head).to("cpu", dtype)
        for q in h.parameters():
            q.grad = None
        delta, rv = [], []
        for f in feats:
            x = f.cpu().to(dtype)
            for conv in h.bbox_subnet:
                x = torch.relu(conv(x))
            delta.append(h.bbox_pred(x))
            rv.append(h.bbox_cov(x))
        case = dict(labels=labels.cpu(), matched_gt=matched.cpu(), gt_boxes=boxes, anchors=torch.cat(level_anchors))
        ref = fr.Referee(case, 0.0, dtype=dtype, delta=lr.from_planes(delta, 4), rv=lr.from_planes(rv, 10))
        loss = ((1.0 - lam) * ref.std + lam * ref.nll()) / norm
        loss.backward()
        grads[dtype] = (h.bbox_cov.weight.grad, h.bbox_cov.bias.grad, loss.detach())
    assert_close(float(res["loss_box_reg"].detach()), float(grads[torch.float64][2]), "loss_box_reg")
    chk = hb.Checker()
    for i, (name, got) in enumerate((("bbox_cov.weight", head.bbox_cov.weight.grad), ("bbox_cov.bias", head.bbox_cov.bias.grad))):
        assert got is not None and got.shape[0] == 90 and bool(torch.isfinite(got).all()) and bool((got != 0).any()), name
        chk.add("full covariance " + name, got, grads[torch.float32][i], grads[torch.float64][i])
    chk.finish()
