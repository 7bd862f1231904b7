"""pod_reg_scores (k_eval_scores, K33) against the fp64 referees of tests/eval_scores/scores_ref.py, on instrument_ref's covariance
families.

Per-row bound |got - ref| <= 2^-22 max(1, |ref|) for both rules: the kernel works in fp64 after the fp32 normals and rounds once to fp32
(2^-24 relative); the referee's fp64 Cholesky factorisation errs by <= cond * 1e-15 <= 1e-9 on these families (cond <= 1e6 is asserted in
tests/eval_instrument/test_eval_matching.py).  The energy referee is evaluated on the kernel's OWN normals (eps_out), so no sampling error
enters; that those normals are the documented ones is test_native_exact_gpu.py's matter.  Measured on an MI355X (profiles/eval_scores.md).

The module shares its name with tests/eval_instrument/test_nll_gpu.py (the NLL of the same rows) so that the GPU run order in
tests/conftest.py (GPU_ORDER, keyed by module name) gives it a place."""
import numpy as np
import pytest
import torch

from tests.eval_instrument import instrument_ref as ir
from tests.eval_scores import gpu_common as gc
from tests.eval_scores import scores_ref as sr

pytestmark = pytest.mark.gpu

# (family, n, M): every family at more than one workgroup with a second trip of lane 0 (M = 129); the sizes around a workgroup's four rows
# and the sample counts around the lane-63 / second-trip edges on one family; the default M; the grid
CASES = [(f, 257, 129) for f in ir.NLL_FAMILIES] + \
        [("wishart", 1, 1), ("wishart", 3, 2), ("wishart", 4, 127), ("wishart", 5, 128), ("cond1e6", 1, 129), ("rank1", 3, 1), ("huge", 4, 2),
         ("zero", 5, 127), ("cond1e6", 5, 1000), ("huge", 3, 1000), ("wishart", 257, 1000), ("rank1", 257, 128), ("wishart", ir.NLL_LARGE, 16)]


@pytest.mark.parametrize("family,n,M", CASES)
def test_rows_against_fp64(family, n, M):
    means, covs, gt = ir.nll_family(family, n)
    got = gc.reg_scores(means, covs, gt, M=M, seed=1234 + M, want_eps=True)
    want_e, want_c = sr.energy_ref(means, covs, gt, got["eps"]), sr.crps_ref(means, covs, gt)
    err_e, err_c = gc.rel_err(got["energy"], want_e), gc.rel_err(got["crps"], want_c)
    print("EVAL_SCORES %-8s n = %5d M = %4d: max |got - ref| / max(1, |ref|): energy %.3g, crps %.3g (bound %.3g); max |ref| %.4g, %.4g"
          % (family, n, M, err_e, err_c, sr.BOUND, float(want_e.abs().max()), float(want_c.abs().max())))
    assert bool(torch.isfinite(got["energy"]).all()) and bool(torch.isfinite(got["crps"]).all())
    assert err_e <= sr.BOUND and err_c <= sr.BOUND, (family, n, M, err_e, err_c)
    assert float(want_c.min()) > 0.0 and float(got["crps"].min()) > 0.0          # a proper score of a continuous forecast is positive


@pytest.fixture(scope="module")
def clean():
    """257 wishart rows at M = 129 under one seed: the run the identities below compare with.  Computed once, never modified."""
    means, covs, gt = ir.nll_family("wishart", 257)
    return means, covs, gt, gc.reg_scores(means, covs, gt, M=129, seed=99, want_eps=True)


def test_replay_of_dumped_normals_gives_the_same_bits(clean):
    means, covs, gt, ref = clean
    again = gc.reg_scores(means, covs, gt, M=129, seed=5, eps_in=ref["eps"], want_eps=True)          # the seed is not read when replaying
    assert torch.equal(again["energy"], ref["energy"]) and torch.equal(again["crps"], ref["crps"]) and torch.equal(again["eps"], ref["eps"])


def test_two_launches_give_the_same_bits(clean):
    means, covs, gt, ref = clean
    again = gc.reg_scores(means, covs, gt, M=129, seed=99)
    assert torch.equal(again["energy"], ref["energy"]) and torch.equal(again["crps"], ref["crps"])
    other = gc.reg_scores(means, covs, gt, M=129, seed=100)
    assert not torch.equal(other["energy"], ref["energy"]) and torch.equal(other["crps"], ref["crps"])


@pytest.mark.parametrize("k", [1, 3, 4, 5, 130])
def test_a_prefix_of_the_rows_scores_as_alone(clean, k):
    means, covs, gt, ref = clean
    part = gc.reg_scores(means[:k], covs[:k], gt[:k], M=129, seed=99, want_eps=True)
    assert torch.equal(part["energy"], ref["energy"][:k]) and torch.equal(part["crps"], ref["crps"][:k])
    assert torch.equal(part["eps"], ref["eps"][:, :k])


def test_indefinite_row_is_nan_and_alone(clean):
    means, covs, gt, ref = clean
    bad = covs.clone()
    q = ir._rotations(torch.Generator().manual_seed(9), 1)[0]
    bad[130] = ((q * torch.tensor([3.0, 1.0, 0.5, -0.5], dtype=torch.float64)) @ q.t()).float()          # an eigenvalue below -1e-2
    assert float(torch.linalg.eigvalsh(ir.nll_sigma(bad[130:131]))[0, 0]) < -0.4
    assert float(torch.diagonal(ir.nll_sigma(bad[130:131]), dim1=-2, dim2=-1).min()) > 0.0              # its CRPS alone would be finite
    got = gc.reg_scores(means, bad, gt, M=129, seed=99)
    assert bool(torch.isnan(got["energy"][130])) and bool(torch.isnan(got["crps"][130]))
    keep = torch.arange(257) != 130
    assert torch.equal(got["energy"][keep], ref["energy"][keep]) and torch.equal(got["crps"][keep], ref["crps"][keep])


def test_either_output_may_be_null(clean):
    means, covs, gt, ref = clean
    e = gc.reg_scores(means, covs, gt, M=129, seed=99, crps=False)
    c = gc.reg_scores(means, covs, gt, M=-3, seed=99, energy=False)          # num_samples is ignored without the energy score
    assert set(e) == {"energy"} and set(c) == {"crps"}
    assert torch.equal(e["energy"], ref["energy"]) and torch.equal(c["crps"], ref["crps"])


@pytest.mark.parametrize("variance", sr.ANCHOR_VARIANCES)
def test_energy_score_meets_the_closed_form(variance):
    """Sigma = s^2 I, gt = mean: the mean of 4096 rows at M = 1000 within 5 of its standard errors of 0.550631 s -- the condition, the
    seed and the sizes of test_eval_scores_cpu.py, there on the host restatement of these draws."""
    means, covs, gt = sr.anchor_case(variance)
    got = gc.reg_scores(means, covs, gt, M=sr.ANCHOR_M, seed=sr.ANCHOR_SEED)
    mean, want, se, dev = sr.anchor_deviation(got["energy"], variance)
    print("ENERGY_ANCHOR gpu variance=%g mean=%.6f closed_form=%.6f standard_error=%.3g deviation=%+.2f standard errors" % (variance, mean, want, se, dev))
    assert abs(dev) <= sr.ANCHOR_SIGMAS
    crps_want = sr.crps_ref(means, covs, gt)
    assert gc.rel_err(got["crps"], crps_want) <= sr.BOUND
    unit = 2.0 / np.sqrt(2.0 * np.pi) - 1.0 / np.sqrt(np.pi)          # z = 0 in every coordinate: CRPS = 0.2337 s
    assert float((crps_want / np.sqrt(variance) - unit).abs().max()) <= 1e-6


def test_reg_proper_scores_is_one_launch_of_the_same_rows(clean):
    from pod_compare_amd import evaluation_utils as ev
    means, covs, gt, ref = clean
    got = ev.reg_proper_scores(means.cuda(), covs.cuda(), gt.cuda(), num_samples=129, seed=99)
    assert set(got) == {"energy_score", "crps"} and got["crps"].dtype == torch.float32 and got["crps"].is_cuda
    assert torch.equal(got["energy_score"].cpu(), ref["energy"]) and torch.equal(got["crps"].cpu(), ref["crps"])
    only = ev.reg_proper_scores(means.cuda(), covs.cuda(), gt.cuda(), num_samples=129, seed=99, crps=False)
    assert set(only) == {"energy_score"} and torch.equal(only["energy_score"].cpu(), ref["energy"])
    empty = ev.reg_proper_scores(means[:0].cuda(), covs[:0].cuda(), gt[:0].cuda())
    assert empty["energy_score"].shape == (0,) and empty["crps"].shape == (0,)
