"""pod_reg_nll (k_reg_nll) and the scoring-rule mirrors against nll_ref, an fp64 referee, on covariances from well conditioned to
cond(Sigma) = 1e6.

Per-row bound |got - ref| <= 2^-22 max(1, |ref|): the kernel works in fp64 and rounds once to fp32 (2^-24 relative); the referee's
fp64 Cholesky factorisation errs by <= cond * 1e-15 <= 1e-9 (cond <= 1e6 is asserted in test_eval_matching.py); an fp64 emulation of
the kernel's arithmetic measured 5.5e-8 relative on every family.  The measured maxima are printed."""
import pytest
import torch

from tests.eval_instrument import instrument_ref as ir

pytestmark = pytest.mark.gpu
BOUND = 2.0 ** -22


def reg_nll(means, covs, gt):
    from pod_compare_amd import hip
    lib = hip.load()
    d = [t.cuda().contiguous() for t in (means, covs, gt)]
    n = means.shape[0]
    out = torch.full((n + 1,), float(ir.SENTINEL), device="cuda")
    hip.check(lib.pod_reg_nll(hip.ptr(d[0]), hip.ptr(d[1]), hip.ptr(d[2]), n, hip.ptr(out), hip.current_stream()), "pod_reg_nll")
    out = out.cpu()
    assert float(out[n]) == ir.SENTINEL          # nothing written past row n - 1
    return out[:n]


def rel_err(got, ref):
    return float(((got.double() - ref).abs() / ref.abs().clamp(min=1.0)).max())


@pytest.mark.parametrize("n", ir.NLL_SIZES)
@pytest.mark.parametrize("family", ir.NLL_FAMILIES)
def test_reg_nll_rows_against_fp64(family, n):
    means, covs, gt = ir.nll_family(family, n)
    ref = ir.nll_ref(means, covs, gt)
    got = reg_nll(means, covs, gt)
    err = rel_err(got, ref)
    print("pod_reg_nll %-8s n = %3d: max |got - ref| / max(1, |ref|) = %.3g (bound %.3g), max |ref| = %.4g" % (family, n, err, BOUND, float(ref.abs().max())))
    assert bool(torch.isfinite(got).all()) and err <= BOUND, (family, n, err)


@pytest.fixture(scope="module")
def large():
    means, covs, gt = ir.nll_family("wishart", ir.NLL_LARGE)
    return means, covs, gt, ir.nll_ref(means, covs, gt)


def test_reg_nll_70001_rows(large):
    means, covs, gt, ref = large
    err = rel_err(reg_nll(means, covs, gt), ref)
    print("pod_reg_nll wishart  n = %d: max |got - ref| / max(1, |ref|) = %.3g (bound %.3g)" % (ir.NLL_LARGE, err, BOUND))
    assert err <= BOUND, err


def test_reg_nll_indefinite_row_is_nan_and_alone():
    means, covs, gt = ir.nll_family("wishart", 257)
    clean = reg_nll(means, covs, gt)
    bad = covs.clone()
    q = ir._rotations(torch.Generator().manual_seed(9), 1)[0]
    bad[130] = ((q * torch.tensor([3.0, 1.0, 0.5, -0.5], dtype=torch.float64)) @ q.t()).float()          # an eigenvalue below -1e-2
    assert float(torch.linalg.eigvalsh(ir.nll_sigma(bad[130:131]))[0, 0]) < -0.4
    got = reg_nll(means, bad, gt)
    assert bool(torch.isnan(got[130]))
    keep = torch.arange(257) != 130
    assert torch.equal(got[keep], clean[keep])


def test_compute_reg_scores_70001_rows(large):
    from pod_compare_amd import evaluation_utils as ev
    means, covs, gt, ref = large
    m = {"predicted_box_means": means.cuda(), "predicted_box_covariances": covs.cuda(), "gt_box_means": gt.cuda()}
    res = ev.compute_reg_scores(m, torch.ones(ir.NLL_LARGE, dtype=torch.bool, device="cuda"))
    want = float(ref.mean())
    mse = float(((means.double() - gt.double()) ** 2).mean())
    print("compute_reg_scores: ignorance %.9g (fp64 %.9g, mean |ref| %.4g), mse %.9g (fp64 %.9g)" % (
        res["ignorance_score_mean"], want, float(ref.abs().mean()), res["mean_squared_error"], mse))
    assert abs(res["ignorance_score_mean"] - want) <= 1e-5 * max(1.0, float(ref.abs().mean()))          # an fp32 tree reduction
    assert abs(res["mean_squared_error"] - mse) <= 1e-5 * mse
    none = ev.compute_reg_scores(m, torch.zeros(ir.NLL_LARGE, dtype=torch.bool, device="cuda"))
    assert none == {"ignorance_score_mean": None, "mean_squared_error": None}


@pytest.mark.parametrize("family", ["cond1e6", "rank1"])
def test_compute_reg_scores_fn_against_the_factor(family):
    from pod_compare_amd import evaluation_utils as ev
    means, covs, gt = ir.nll_family(family, 257)
    want = float(ir.entropy_ref(covs).mean())
    got = ev.compute_reg_scores_fn({"predicted_box_covariances": covs.cuda()}, torch.ones(257, dtype=torch.bool, device="cuda"))["total_entropy_mean"]
    print("compute_reg_scores_fn %-8s: %.12g (fp64 from the factor %.12g, difference %.3g)" % (family, got, want, abs(got - want)))
    assert abs(got - want) <= 1e-9, (got, want)
    assert ev.compute_reg_scores_fn({"predicted_box_covariances": covs.cuda()}, torch.zeros(257, dtype=torch.bool, device="cuda")) == {"total_entropy_mean": None}
