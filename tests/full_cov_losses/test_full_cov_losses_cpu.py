"""CPU side of K28: the declarations of the two entry points, their refusals (validation happens on the host before any launch), the routing
of ProbabilisticLosses by the reg_var planes' channel count, the --bbox-cov-type flag of the two commands, and the referee of the GPU tests
(tests/full_cov_losses/full_cov_ref.py) -- its analytic derivatives against its own autograd, and the two conditions its inputs must
meet for the project's bar to be a statement about the kernel: (a) the same restatement in fp32 torch uses at most a quarter of the bar,
(b) at beta = 0 no term whose sign enters a derivative lies within 2^-18 of a sign change.  No GPU."""
import ctypes

import pytest
import torch

from pod_compare_amd import build, hip, losses
from tests.helpers import assert_close
from tests.full_cov_losses import full_cov_ref as fr
from tests.training import loss_ref as lr

NAMES = ("pod_full_cov_partials", "pod_full_cov_loss")
BAR = 1e-4


@pytest.fixture(scope="module")
def fx():
    return lr.load_fixture()


def test_header_binding_and_library_carry_the_full_covariance_entry_points():
    from tests.test_abi_cpu import HEADER, declared_symbols
    header = open(HEADER).read()
    for name in NAMES:
        assert name in hip.EXPORTS and name in declared_symbols()
    assert hip.POD_ABI_VERSION == 18 and header.count("#define POD_ABI_VERSION ") == 1 and "#define POD_ABI_VERSION 18\n" in header
    for name, value in (("POD_FULL_COV_NLL", 1), ("POD_FULL_COV_MOMENTS", 2), ("POD_FULL_COV_ENERGY", 3)):
        assert getattr(hip, name) == value and any(l.split()[:3] == ["#define", name, str(value)] for l in header.splitlines()), name
    assert "k28_full_cov_loss.hip" in build.SOURCES
    lib = ctypes.CDLL(build.build_library())
    assert lib.pod_abi_version() == 18 and all(hasattr(lib, n) for n in NAMES)
    assert "pod_full_cov_partials" in hip._SIZE_QUERIES and hip.load().pod_full_cov_partials.restype is ctypes.c_int64


def test_full_covariance_entry_point_rejects_invalid_arguments_without_a_gpu():
    lib = hip.load()
    buf = ctypes.create_string_buffer(96)
    X = (ctypes.addressof(buf) + 15) & ~15           # any non-null pointer: never dereferenced on these paths
    lv = (hip.PodLevel * hip.POD_MAX_LEVELS)()
    lv[0].H, lv[0].W, lv[0].anchor_base = 2, 3, 0
    for n in ("cls", "cls_var", "delta", "reg_var"):
        setattr(lv[0], n, X)
    no_var = (hip.PodLevel * hip.POD_MAX_LEVELS)()
    no_var[0].H, no_var[0].W, no_var[0].anchor_base = 2, 3, 0
    no_var[0].cls = no_var[0].cls_var = no_var[0].delta = X
    empty = (hip.PodLevel * hip.POD_MAX_LEVELS)()
    empty[0].cls = empty[0].cls_var = empty[0].delta = empty[0].reg_var = X

    def cfg_with(**kw):
        c = hip.PodConfig()
        c.n_levels, c.n_runs, c.num_anchors, c.num_classes, c.cov_dims, c.has_cls_var, c.cls_samples = 1, 1, 9, 7, 10, 1, 3
        for k, v in kw.items():
            setattr(c, k, v)
        return c

    def full(c, R=54, labels=X, matched=X, gt=X, n_gt=1, anchors=X, partials=X, total=X, grads=None, w=None, levels=lv, kind=3, m=1000,
             beta=0.0, eps=None, eps_out=None):
        return lib.pod_full_cov_loss(c, levels, grads, labels, matched, gt, n_gt, anchors, R, kind, m, beta, eps, eps_out, w, partials, total, None)

    assert lib.pod_full_cov_partials(cfg_with(), lv) == 1 and lib.pod_full_cov_partials(cfg_with(n_runs=3), lv) == 3
    assert lib.pod_full_cov_partials(cfg_with(n_levels=0), lv) == 0 and lib.pod_full_cov_partials(None, lv) == 0
    # what pod_reg_score_loss refuses (tests/score_losses/test_score_losses_cpu.py), with the head width the other way round
    for kw in ({"n_levels": 0}, {"n_levels": hip.POD_MAX_LEVELS + 1}, {"n_runs": 0}, {"n_runs": 65536}, {"num_anchors": 0}, {"num_classes": 0},
               {"num_classes": 16}, {"cls_samples": 0}, {"cls_samples": hip.POD_MAX_CLS_SAMPLES + 1}, {"cov_dims": 4}, {"cov_dims": 0}):
        for kind in (1, 2, 3):
            assert full(cfg_with(**kw), kind=kind) == -1, (kw, kind)
    ok = cfg_with()
    for kw in ({"R": 55}, {"R": 0}, {"labels": None}, {"matched": None}, {"anchors": None}, {"partials": None}, {"total": None}, {"gt": None},
               {"n_gt": -1}, {"beta": -1.0}, {"beta": float("nan")}, {"levels": None}, {"levels": empty}):
        for kind in (1, 2, 3):
            assert full(ok, kind=kind, **kw) == -1, (kw, kind)
    assert full(None) == -1
    assert full(ok, grads=(hip.PodLevelGrad * hip.POD_MAX_LEVELS)(), w=None) == -1          # gradient planes need their weights
    # and what is this entry's own: the kind, the sample count of the energy kind alone, the reg_var planes, aligned dense normals
    for kind in (0, 4, -1):
        assert full(ok, kind=kind) == -1, kind
    for m in (0, -5, hip.POD_MAX_REG_SAMPLES + 1):          # (the energy kind only: test_torch_ops_gpu.py runs the other two with num_samples = 0)
        assert full(ok, m=m) == -1, m
    for kind in (1, 2, 3):
        assert full(ok, levels=no_var, kind=kind) == -1
    assert full(ok, eps=X + 4) == -1 and full(ok, eps_out=X + 8) == -1
    # the existing entry points keep refusing the full covariance
    assert lib.pod_reg_score_loss(ok, lv, None, X, X, X, 1, X, 54, 2, 1000, 0.0, None, None, None, X, X, None) == -1


def test_losses_route_by_the_channel_count_of_the_reg_var_planes():
    """A * 4: today's paths; A * 10: every one of the four names through pod_full_cov_loss; any other count raises, naming it."""
    kinds = {"none": hip.POD_FULL_COV_NLL, "negative_log_likelihood": hip.POD_FULL_COV_NLL,
             "second_moment_matching": hip.POD_FULL_COV_MOMENTS, "energy_loss": hip.POD_FULL_COV_ENERGY}
    assert losses.FULL_COV_KINDS == kinds
    for name in losses.BBOX_COV_LOSSES:
        crit = losses.ProbabilisticLosses(bbox_cov_loss=name)
        assert losses.covariance_route(crit.bbox_cov_loss, 9, 90) == (losses.full_cov_sum, name)
        assert losses.covariance_route(name, 3, 30) == (losses.full_cov_sum, name)
        assert losses.covariance_route(name, 9, None) == (None, None)
    assert losses.covariance_route("none", 9, 36) == (None, None) == losses.covariance_route("negative_log_likelihood", 9, 36)
    assert losses.covariance_route("energy_loss", 9, 36) == (losses.reg_score_sum, "energy_loss")
    assert losses.covariance_route("second_moment_matching", 9, 36) == (losses.reg_score_sum, "second_moment_matching")
    with pytest.raises(hip.PodError, match="63 channels"):
        losses.covariance_route("none", 9, 63)
    with pytest.raises(ValueError, match="bogus"):
        losses.covariance_route("bogus", 9, 90)
    with pytest.raises(ValueError):
        losses.full_cov_sum(None, None, None, None, None, None, None, None, 9, 7, kind="bogus")


def test_a_seven_channel_plane_raises_from_the_loss_state():
    """Through ProbabilisticLosses.__call__ on CPU tensors: the routing runs, and refuses, before any launch."""
    from pod_compare_amd import synthetic
    z = lambda c: [torch.zeros((1, c, 2, 3))]
    ho = synthetic.HeadOutputs(z(7), z(4), None, z(7), [torch.zeros((6, 4))], [(2, 3)], 1, 7, (16, 24))
    crit = losses.ProbabilisticLosses(num_classes=7)
    with pytest.raises(hip.PodError, match="7 channels"):
        crit(ho, torch.zeros((1, 6), dtype=torch.int32), torch.zeros((1, 6), dtype=torch.int32), torch.zeros((1, 4)), normalizer=1.0)
    assert crit.draws == 0


def test_the_covariance_type_flag_overrides_the_config_in_both_commands():
    from pod_compare_amd import compute_losses, train_head
    from pod_compare_amd.config import setup_config
    for mod in (train_head, compute_losses):
        ap = mod.arg_parser()
        base = ["--coco-json", "x.json", "--image-root", "."]
        args = ap.parse_args(base)
        assert args.bbox_cov_type is None
        cfg = setup_config(args.config_file, "", 0)
        cov = mod.covariance_overrides(cfg, args)
        assert cov.COVARIANCE_TYPE == "diagonal" and cov.NAME == "negative_log_likelihood"          # the YAML's, untouched
        args = ap.parse_args(base + ["--bbox-cov-type", "full", "--bbox-cov-loss", "energy_loss"])
        cov = mod.covariance_overrides(cfg, args)
        assert cov.COVARIANCE_TYPE == "full" and cov.NAME == "energy_loss"
        assert cfg.MODEL.PROBABILISTIC_MODELING.BBOX_COV_LOSS.COVARIANCE_TYPE == "full"
        cov = mod.covariance_overrides(cfg, ap.parse_args(base + ["--bbox-cov-type", "diagonal"]))
        assert cov.COVARIANCE_TYPE == "diagonal" and cov.NAME == "energy_loss"
        with pytest.raises(SystemExit):
            ap.parse_args(base + ["--bbox-cov-type", "banded"])


def test_the_full_type_gives_the_model_a_ninety_channel_predictor():
    from pod_compare_amd import modeling
    m = modeling.ProbabilisticRetinaNet(num_classes=7, bbox_cov_loss="energy_loss", bbox_cov_type="full")
    assert m.head.bbox_cov.out_channels == 90 and m.head.bbox_cov_dims == 10


# ---- the referee ---------------------------------------------------------------------------------------------------------------------
def test_the_fixture_and_its_seeded_off_diagonals(fx):
    case = fr.full_case(fx)
    assert tuple(case["reg_var"].shape) == (2, 1161, 10) and case["reg_var"].dtype == torch.float32
    assert torch.equal(case["reg_var"][..., :4], torch.from_numpy(fx["reg_var"]))
    ref = fr.Referee(case)
    assert int(ref.pos.sum()) == 81 and int((~ref.inside).sum()) == 19 and tuple(ref.L.shape) == (81, 4, 4)
    assert fr.T.t().tolist() == [[1, 0], [2, 0], [2, 1], [3, 0], [3, 1], [3, 2]]
    assert bool((torch.triu(ref.L, 1) == 0).all()) and bool((ref.L[:, fr.T[0], fr.T[1]] != 0).all())
    rvp = case["reg_var"][ref.pos].double()
    assert torch.equal(ref.L[:, 2, 1].detach(), rvp[:, 6]) and torch.equal(ref.L[:, 3, 0].detach(), rvp[:, 7])
    zero = fr.Referee(fr.full_case(fx, zero_off=True))
    assert bool((zero.L[:, fr.T[0], fr.T[1]] == 0).all())


@pytest.mark.parametrize("beta", [0.0, 0.11])
def test_referee_analytic_derivatives_equal_its_autograd(fx, beta):
    ref = fr.Referee(fr.full_case(fx), beta)
    cases = [("nll", ref.nll(), ref.nll_analytic()), ("moments", ref.moments(), ref.moments_analytic())]
    for m in (7, 64):
        eps = fr.replay_normals(m)
        cases.append(("energy M=%d" % m, ref.energy(eps), ref.energy_analytic(eps)))
    for what, total, (a_delta, a_rv) in cases:
        g_delta, g_rv = ref.gradients(total)
        assert_close(a_delta, g_delta[ref.pos], what + " d/d delta", rtol=1e-9, atol=1e-9)
        assert_close(a_rv, g_rv[ref.pos], what + " d/d rv", rtol=1e-9, atol=1e-9)
        assert bool((g_delta[~ref.pos] == 0).all()) and bool((g_rv[~ref.pos] == 0).all())
        outside = g_rv[ref.pos][:, :4][~ref.inside]
        assert outside.numel() == 19 and bool((outside == 0).all()) and bool((g_rv[ref.pos][:, 4:] != 0).any())


def fraction_of_the_bar(x32, x64):
    x64 = x64.detach().double()
    return float(((x32.detach().double() - x64).abs() / (BAR * torch.clamp(x64.abs(), min=1.0))).max())


@pytest.mark.parametrize("beta", [0.0, 0.11])
def test_condition_a_the_restatement_in_fp32_uses_a_quarter_of_the_bar(fx, beta):
    """Every value and gradient of the three kinds, M = 64 and 1000: fp32 torch against fp64 torch, at most 0.25 of 1e-4 max(1, |ref|)."""
    case = fr.full_case(fx)
    r64, r32 = fr.Referee(case, beta), fr.Referee(case, beta, dtype=torch.float32)
    sums = [("nll", lambda r: r.nll()), ("moments", lambda r: r.moments())]
    for m in (64, 1000):
        eps = fr.replay_normals(m)
        sums.append(("energy M=%d" % m, lambda r, eps=eps: r.energy(eps)))
    for what, fn in sums:
        if what == "nll" and beta:
            continue                                   # (no smooth-L1 term in it)
        t64, t32 = fn(r64), fn(r32)
        fracs = [fraction_of_the_bar(t32, t64)] + [fraction_of_the_bar(a, b) for a, b in zip(r32.gradients(r32.std + t32), r64.gradients(r64.std + t64))]
        print("condition (a) %-14s beta %.2f: fractions of the bar: value %.3f  d/d delta %.3f  d/d rv %.3f" % ((what, beta) + tuple(fracs)))
        assert max(fracs) <= 0.25, (what, fracs)


def test_condition_b_no_term_of_the_fixture_has_an_undecided_sign(fx):
    """Off-diagonal seed 2803, replayed normals of seed 2703, at the three sample counts of the GPU test, and the moment-matching terms:
    none within 2^-18 of a sign change relative to the sum of the magnitudes of its terms."""
    for zero_off in (False, True):
        ref = fr.Referee(fr.full_case(fx, zero_off=zero_off), 0.0)
        count, ratio = ref.moments_undecided()
        print("moment matching (zero off-diagonals: %s): smallest ratio %.3g" % (zero_off, ratio))
        assert count == 0
        for m in (7, 64, 1000):
            eps = fr.replay_normals(m)
            assert tuple(eps.shape) == (m + 1, 2322, 4)
            count, ratio = ref.energy_undecided(eps)
            print("energy, M = %d (zero off-diagonals: %s): smallest ratio %.3g" % (m, zero_off, ratio))
            assert count == 0, m
