"""CPU side of K27: the declarations of the two entry points, their refusals (validation happens on the host before any launch), the new
keywords of ProbabilisticLosses, and the referee of the GPU tests (tests/score_losses/score_ref.py) -- its analytic derivatives against
its own autograd, and the count of sign-undecided terms on the fixture, so that a changed fixture is caught here.  No GPU."""
import ctypes

import pytest
import torch

from pod_compare_amd import build, hip, losses
from tests.helpers import assert_close
from tests.score_losses import score_ref as sr
from tests.training import loss_ref as lr

NAMES = ("pod_reg_score_partials", "pod_reg_score_loss")


@pytest.fixture(scope="module")
def fx():
    return lr.load_fixture()


def test_header_binding_and_library_carry_the_score_entry_points():
    from tests.test_abi_cpu import HEADER, declared_symbols
    header = open(HEADER).read()
    for name in NAMES:
        assert name in hip.EXPORTS and name in declared_symbols()
    assert hip.POD_ABI_VERSION == 18 and "#define POD_ABI_VERSION 18\n" in header
    for name, value in (("POD_REG_LOSS_MOMENTS", 1), ("POD_REG_LOSS_ENERGY", 2), ("POD_MAX_REG_SAMPLES", 4096)):
        assert getattr(hip, name) == value and any(l.split()[:3] == ["#define", name, str(value)] for l in header.splitlines()), name
    assert "k27_reg_score_loss.hip" in build.SOURCES
    lib = ctypes.CDLL(build.build_library())
    assert lib.pod_abi_version() == 18 and all(hasattr(lib, n) for n in NAMES)
    assert "pod_reg_score_partials" in hip._SIZE_QUERIES and hip.load().pod_reg_score_partials.restype is ctypes.c_int64


def test_score_entry_point_rejects_invalid_arguments_without_a_gpu():
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
        c.n_levels, c.n_runs, c.num_anchors, c.num_classes, c.cov_dims, c.has_cls_var, c.cls_samples = 1, 1, 9, 7, 4, 1, 3
        for k, v in kw.items():
            setattr(c, k, v)
        return c

    def score(c, R=54, labels=X, matched=X, gt=X, n_gt=1, anchors=X, partials=X, total=X, grads=None, w=None, levels=lv, kind=2, m=1000,
              beta=0.0, eps=None, eps_out=None):
        return lib.pod_reg_score_loss(c, levels, grads, labels, matched, gt, n_gt, anchors, R, kind, m, beta, eps, eps_out, w, partials, total, None)

    assert lib.pod_reg_score_partials(cfg_with(), lv) == 1 and lib.pod_reg_score_partials(cfg_with(n_runs=3), lv) == 3
    assert lib.pod_reg_score_partials(cfg_with(n_levels=0), lv) == 0 and lib.pod_reg_score_partials(None, lv) == 0
    # what pod_train_loss refuses
    for kw in ({"n_levels": 0}, {"n_levels": hip.POD_MAX_LEVELS + 1}, {"n_runs": 0}, {"n_runs": 65536}, {"num_anchors": 0}, {"num_classes": 0},
               {"num_classes": 16}, {"cls_samples": 0}, {"cls_samples": hip.POD_MAX_CLS_SAMPLES + 1}, {"cov_dims": 10}):
        assert score(cfg_with(**kw)) == -1, kw
    ok = cfg_with()
    for kw in ({"R": 55}, {"R": 0}, {"labels": None}, {"matched": None}, {"anchors": None}, {"partials": None}, {"total": None}, {"gt": None},
               {"n_gt": -1}, {"beta": -1.0}, {"beta": float("nan")}, {"levels": None}, {"levels": empty}):
        assert score(ok, **kw) == -1, kw
    assert score(None) == -1
    assert score(ok, grads=(hip.PodLevelGrad * hip.POD_MAX_LEVELS)(), w=None) == -1          # gradient planes need their weights
    # and what is this entry's own: the diagonal head, the kind, the sample count, the reg_var planes, aligned dense normals
    assert score(cfg_with(cov_dims=0)) == -1
    for kind in (0, 3, -1):
        assert score(ok, kind=kind) == -1, kind
    for m in (0, -5, hip.POD_MAX_REG_SAMPLES + 1):
        assert score(ok, m=m) == -1, m
    assert score(ok, levels=no_var) == -1 and score(ok, levels=no_var, kind=1) == -1
    assert score(ok, eps=X + 4) == -1 and score(ok, eps_out=X + 8) == -1


def test_unknown_loss_name_raises_and_the_four_names_are_accepted():
    with pytest.raises(ValueError, match="bogus"):
        losses.ProbabilisticLosses(bbox_cov_loss="bogus")
    for name in ("none", "negative_log_likelihood", "second_moment_matching", "energy_loss"):
        crit = losses.ProbabilisticLosses(bbox_cov_loss=name, bbox_cov_num_samples=17)
        assert crit.bbox_cov_loss == name and crit.bbox_cov_num_samples == 17 and crit.draws == 0
    crit = losses.ProbabilisticLosses()
    assert crit.bbox_cov_loss == "negative_log_likelihood" and crit.bbox_cov_num_samples == 1000
    with pytest.raises(ValueError):
        losses.reg_score_sum(None, None, None, None, None, None, None, None, 9, 7, kind="negative_log_likelihood")


def test_the_model_hands_its_loss_name_and_sample_count_to_its_loss_state():
    from pod_compare_amd import config, modeling
    import inspect
    p = inspect.signature(modeling.ProbabilisticRetinaNet.__init__).parameters
    assert p["bbox_cov_loss"].default == "none" and p["bbox_cov_num_samples"].default == 1000
    assert "bbox_cov_loss=self.bbox_cov_loss" in inspect.getsource(modeling.ProbabilisticRetinaNet.losses)
    assert config.get_cfg().MODEL.PROBABILISTIC_MODELING.BBOX_COV_LOSS.NUM_SAMPLES == 1000


@pytest.mark.parametrize("beta", [0.0, 0.11])
def test_referee_analytic_derivatives_equal_its_autograd(fx, beta):
    case = sr.fixture_case(fx)
    ref = sr.Referee(case, beta)
    assert int(ref.pos.sum()) == 81 and int((~ref.inside).sum()) == 19
    g_delta, g_lv = ref.gradients(ref.moments())
    a_delta, a_lv = ref.moments_analytic()
    assert_close(a_delta, g_delta[ref.pos], "moments d/d delta", rtol=1e-12, atol=1e-12)
    assert_close(a_lv, g_lv[ref.pos], "moments d/d lv", rtol=1e-12, atol=1e-12)
    assert bool((g_delta[~ref.pos] == 0).all()) and bool((g_lv[~ref.pos] == 0).all())
    for m in (7, 64):
        eps = sr.replay_normals(m)
        g_delta, g_lv = ref.gradients(ref.energy(eps))
        a_delta, a_lv = ref.energy_analytic(eps)
        assert_close(a_delta, g_delta[ref.pos], "energy d/d delta", rtol=1e-12, atol=1e-12)
        assert_close(a_lv, g_lv[ref.pos], "energy d/d lv", rtol=1e-12, atol=1e-12)
        assert bool((g_lv[ref.pos][~ref.inside] == 0).all()) and bool((g_lv[ref.pos][ref.inside] != 0).any())


def test_no_term_of_the_fixture_has_an_undecided_sign(fx):
    """Seed 2703 at the three sample counts of the GPU test, and the moment-matching terms: none within 2^-16 of a sign change."""
    ref = sr.Referee(sr.fixture_case(fx), 0.0)
    count, a, b = ref.moments_undecided()
    print("moment matching: smallest ratios", a, b)
    assert count == 0
    for m in (7, 64, 1000):
        eps = sr.replay_normals(m)
        assert tuple(eps.shape) == (m + 1, 2322, 4)
        count, ratio = ref.energy_undecided(eps)
        print("energy, M =", m, "smallest ratio", ratio)
        assert count == 0, m
