"""The fp64 referee (tests/fp64_referee/f64_ref.py) on the CPU: pinned bit for bit to the oracle at float32 on every predictor
fixture, then the fp32 oracle measured against its float64 evaluation (the CPU section of profiles/fp64_referee.md)."""
import numpy as np
import pytest
import torch

from oracle import pod_oracle as po
from tests.helpers import fixture_id
from tests.fp64_referee import f64_ref as fr
from tests.fp64_referee import runs

SMALL_CFG = [p for p in runs.ALL if fixture_id(p).startswith("cfg")]


@pytest.mark.parametrize("path", runs.ALL, ids=fixture_id)
def test_referee_at_float32_is_the_oracle_bit_for_bit(path):
    """Same torch / numpy calls on the same shapes: boxes, covariances and final detections torch.equal, the two post-NMS
    fixtures included.  Only then is the float64 evaluation the bar."""
    g, p, run, levels, modes, _ = runs.golden_run(path)
    c32 = runs.chain(g, run, levels, modes, p, torch.float32)
    for aw, c in zip(run.aw, c32.cand):
        assert c.boxes.dtype == torch.float32 and torch.equal(c.boxes, aw.boxes)
        assert (c.cov is None) == (aw.cov is None)
        if aw.cov is not None:
            assert torch.equal(c.cov, aw.cov)
    for got, want in ((c32.pre.boxes, run.pre.pred_boxes), (c32.pre.cov, run.pre.pred_boxes_covariance), (c32.pre.scores, run.pre.scores),
                      (c32.pre.probs, run.pre.pred_cls_probs), (c32.det.boxes, run.det.pred_boxes), (c32.det.cov, run.det.pred_boxes_covariance),
                      (c32.det.scores, run.det.scores), (c32.det.probs, run.det.pred_cls_probs)):
        assert got.dtype == torch.float32 and torch.equal(got, want)
    # and the staged oracle run is po.predict itself
    s = g.spec
    kw, modes = runs.fixture_kwargs(g)
    img, out = tuple(g.meta["image"]), tuple(g.meta["out"])
    if s.get("post_nms"):
        ref = po.predict_post_nms_ensemble(p, img, out, kw, g.eps_source())
    else:
        ref = po.predict(s["mode"], p, img, out, outputs=kw[0] if s["runs"] == 1 else None, run_outputs=kw if s["runs"] > 1 else None,
                         eps_fn=g.eps_source(), **modes)
    assert torch.equal(ref.pred_boxes, run.det.pred_boxes) and torch.equal(ref.pred_boxes_covariance, run.det.pred_boxes_covariance)
    assert torch.equal(ref.pred_classes, run.det.pred_classes) and torch.equal(ref.scores, run.det.scores)
    assert torch.equal(fr.cov_xyxy_to_xywh(c32.det.cov), po.cov_xyxy_to_xywh(run.det.pred_boxes_covariance))


def test_referee_units_at_float32_equal_the_oracle_on_conditioned_inputs():
    """The cluster functions off the fixtures' handful of members: both box merges on ill-conditioned covariances, D = 10 Cholesky."""
    rng = np.random.Generator(np.random.Philox(3))
    q, _ = np.linalg.qr(rng.standard_normal((40, 4, 4)))
    ev = np.stack([np.geomspace(1e-2, 1e-2 * c, 4) for c in np.geomspace(1.0, 1e5, 40)])
    covs = (q * ev[:, None, :] @ q.transpose(0, 2, 1)).astype(np.float32)
    covs = (covs + covs.transpose(0, 2, 1)) / 2
    means = (300 + rng.standard_normal((40, 4))).astype(np.float32)
    for mode in ("bayesian_inference", "covariance_intersection"):
        a, b = fr.bayes_fuse(means, covs, mode), po.bayes_fuse(means, covs, mode)
        assert a[0].dtype == np.float32 and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        a64 = fr.bayes_fuse(means.astype(np.float64), covs.astype(np.float64), mode)
        assert a64[1].dtype == np.float64
    rv = torch.from_numpy(rng.standard_normal((9, 10)).astype(np.float32))
    assert torch.equal(fr.cholesky_from_head(rv), po.cholesky_from_head(rv))
    assert fr.cholesky_from_head(rv.double()).dtype == torch.float64
    b = torch.from_numpy((100 + 50 * rng.random((30, 2))).astype(np.float32))
    b = torch.cat((b, b + 20 + torch.from_numpy(rng.random((30, 2)).astype(np.float32))), 1)
    assert torch.equal(fr.iou_matrix(b, b), po.iou_matrix(b, b))


@pytest.mark.parametrize("name", ["cfg2_bayes_od_regclsvar_s21", "full_cov_standard_nms_s121"])
def test_the_rule_rejects_a_one_pass_covariance(name):
    """The acceptance rule the GPU tests apply (f64_ref.within_rule) has teeth: the fp32 one-pass form (sum x x^T - S m m^T) / (S - 1)
    on the very samples of the two-pass reference is further from fp64 by three orders of magnitude and is refused, while the
    reference against itself passes."""
    path = [p for p in runs.ALL if fixture_id(p) == name][0]
    g, p, run, levels, modes, c64 = runs.golden_run(path)
    c32 = fr.candidate_stage(levels[0], run.decisions[0].tops, run.eps_prop[0], torch.float32, p.box_weights, keep_samples=True)
    assert torch.equal(c32.cov, run.aw[0].cov)
    x, ref64 = c32.samples, c64.cand[0].cov
    s = x.shape[2]
    mean = x.mean(2)
    one_pass = (torch.einsum("nis,njs->nij", x, x) - s * mean[:, :, None] * mean[:, None, :]) / (s - 1)
    e_ref = fr.cov_error(c32.cov, ref64)
    ok, fig = fr.within_rule(fr.cov_error(one_pass, ref64), e_ref)
    assert not ok and fig["ratio_max"] > 100 and fig["ratio_rms"] > 100, fig
    assert fr.within_rule(e_ref, e_ref)[0]


@pytest.mark.parametrize("path", runs.ALL, ids=fixture_id)
def test_measured_reference_against_float64(path):
    """How far the fp32 oracle itself is from the exact evaluation (figures: profiles/fp64_referee.md, CPU section).  Asserted by
    direction only: over the element-wise 1e-4 bar on the two full-size fixtures named there, under it on the small cfg* fixtures,
    and under 1e-4 x max |matrix| everywhere."""
    r = runs.measure(path)
    name = fixture_id(path)
    print(name, r)
    for q in ("candidate cov", "final cov"):
        if q in r:
            assert r[q]["mat"] < 1.0, (name, q, r[q])
    if name in runs.FULL_OVER_BAR:
        assert r["candidate cov"]["elem"] > 1.0, (name, r["candidate cov"])
    if path in SMALL_CFG:
        for q in ("candidate boxes", "candidate cov", "final boxes", "final cov"):
            if q in r:
                assert r[q]["elem"] < 1.0, (name, q, r[q])
    for q in ("candidate boxes", "final boxes"):      # box means: the element-wise bar holds against fp64 on every fixture
        assert r[q]["elem"] < 1.0, (name, q, r[q])
