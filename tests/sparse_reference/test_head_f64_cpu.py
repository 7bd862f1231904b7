"""The float64 referee of tests/sparse_reference/head_f64.py, pinned to what the reference's own ProbabilisticRetinaNetHead produced
(tests/golden/head_*.npz) before it judges anything.  A condition on the referee, not a measurement: within 0.1 x the 1e-4 bar of
tests/test_head_reference_gpu.py (measured: 0.7 % of that, profiles/sparse_reference.md), so that at geometries the fixtures do not have
it stands in for the reference 10 x finer than the bar it judges by; and the same code in float32 meets tests/test_head_reference.py's 2e-5."""
import pytest
import torch

from oracle import model_fixture as mf
from tests.head_fixture import VARIANT_NAMES, HeadFixture
from tests.sparse_reference import head_f64 as hf

TOL = 1e-4                       # the project's bar (tests/test_head_reference_gpu.py)
F64_BOUND = 0.1 * TOL
F32_BOUND = 2e-5                 # tests/test_head_reference.py
MC_VARIANTS = [v for v in VARIANT_NAMES if mf.VARIANTS[v]["dropout_rate"] > 0]


def worst(got, fx, prefix):
    """Largest error of a referee evaluation against the fixture, in units of the tensor's scale max(1, max |fixture|)."""
    w = 0.0
    for field in hf.FIELDS:
        if got[field] is None:
            assert not fx.present(field), field
            continue
        assert fx.present(field), field
        for l in range(len(fx.levels)):
            want = fx.t("%s_%s_l%d" % (prefix, field, l)).double()
            assert got[field][l].shape == want.shape, (field, l, got[field][l].shape, want.shape)
            w = max(w, float((got[field][l].double() - want).abs().max()) / max(1.0, float(want.abs().max())))
    return w


def evaluate(variant, mc, dtype):
    fx = HeadFixture(variant)
    v = mf.VARIANTS[variant]
    assert fx.meta["channels"] == mf.CHANNELS and (fx.meta["num_anchors"], fx.meta["num_classes"]) == (hf.NUM_ANCHORS, hf.NUM_CLASSES)
    params = hf.seeded_parameters(v, fx.meta["seed"], fx.meta["channels"])
    assert sorted(params) == sorted(fx.meta["state_keys"])                       # the restated key names are the reference's
    replay = hf.replay_of(fx.masks, fx.levels, fx.meta["channels"], fx.runs) if mc else None
    got = hf.head_f64(params, fx.features(), v, replay, fx.runs, dtype)
    return worst(got, fx, "mc" if mc else "eval")


@pytest.mark.parametrize("variant", VARIANT_NAMES)
def test_f64_referee_equals_the_reference_head_in_eval_mode(variant):
    w = evaluate(variant, False, torch.float64)
    print("\nsparse_reference: f64 referee vs fixture, eval, %s: %.3e" % (variant, w))
    assert w <= F64_BOUND, w


@pytest.mark.parametrize("variant", MC_VARIANTS)
def test_f64_referee_equals_the_reference_head_on_its_recorded_masks(variant):
    w = evaluate(variant, True, torch.float64)
    print("\nsparse_reference: f64 referee vs fixture, MC, %s: %.3e" % (variant, w))
    assert w <= F64_BOUND, w


@pytest.mark.parametrize("variant", VARIANT_NAMES)
def test_f32_evaluation_of_the_referee_meets_the_cpu_parity_bound(variant):
    w = evaluate(variant, False, torch.float32)
    print("\nsparse_reference: f32 evaluation vs fixture, eval, %s: %.3e" % (variant, w))
    assert w <= F32_BOUND, w
    if mf.VARIANTS[variant]["dropout_rate"] > 0:
        w = evaluate(variant, True, torch.float32)
        print("sparse_reference: f32 evaluation vs fixture, MC, %s: %.3e" % (variant, w))
        assert w <= F32_BOUND, w


def test_seeded_masks_do_not_depend_on_the_order_they_are_asked_for():
    a, b = hf.SeededMasks(7, 0.2), hf.SeededMasks(7, 0.2)
    x = a.get(1, 0, 2, 0, 3, (1, 64, 33, 47))
    b.get(1, 1, 0, 0, 0, (1, 64, 33, 47))
    assert torch.equal(x, b.get(1, 0, 2, 0, 3, (1, 64, 33, 47)))
    assert not torch.equal(x, a.get(1, 1, 2, 0, 3, (1, 64, 33, 47))) and not torch.equal(x, a.get(1, 0, 1, 0, 3, (1, 64, 33, 47)))
    assert abs(float(x.float().mean()) - 0.8) < 0.01
    # the copy order of HeadFixture.replay: with the last run's unused evaluations skipped (m = n - 1) an evaluation keeps its masks
    full, skip = hf.replay_of(a, [(33, 47)], 64, 3), hf.replay_of(a, [(33, 47)], 64, 3, 2)
    assert torch.equal(full(1, 2, 0, 3), skip(1, 2, 0, 3)) and torch.equal(full(1, 2, 0, 4), skip(1, 2, 0, 4))      # bbox: variance branch at n
    assert torch.equal(full(0, 2, 0, 3), skip(0, 2, 0, 2))                                                         # cls: at m
