"""torch.ops.pod_mi355x.reg_scores: the operator returns the direct call's bits and refuses what `reg_nll` refuses.  The module shares its
name with tests/test_torch_ops_gpu.py for its place in the GPU run order (tests/conftest.py: GPU_ORDER)."""
import pytest
import torch

from tests.eval_instrument import instrument_ref as ir
from tests.eval_scores import gpu_common as gc

pytestmark = pytest.mark.gpu


def test_reg_scores_operator_equals_the_direct_call():
    import pod_compare_amd.torch_ops  # noqa: F401  (registers the library)
    means, covs, gt = ir.nll_family("wishart", 5)
    want = gc.reg_scores(means, covs, gt, M=129, seed=31)
    energy, crps = torch.ops.pod_mi355x.reg_scores(means.cuda(), covs.cuda(), gt.cuda(), 129, 31)
    assert energy.dtype == crps.dtype == torch.float32 and energy.is_cuda and tuple(energy.shape) == tuple(crps.shape) == (5,)
    assert torch.equal(energy.cpu(), want["energy"]) and torch.equal(crps.cpu(), want["crps"])
    want = gc.reg_scores(means, covs, gt, M=1000, seed=0)
    energy, crps = torch.ops.pod_mi355x.reg_scores(means.cuda(), covs.cuda(), gt.cuda())          # the schema's defaults: 1000 draws, seed 0
    assert torch.equal(energy.cpu(), want["energy"]) and torch.equal(crps.cpu(), want["crps"])
    energy, crps = torch.ops.pod_mi355x.reg_scores(means[:0].cuda(), covs[:0].cuda(), gt[:0].cuda())
    assert tuple(energy.shape) == tuple(crps.shape) == (0,)


def test_reg_scores_operator_rejects_bad_arguments():
    import pod_compare_amd.torch_ops  # noqa: F401
    op = torch.ops.pod_mi355x.reg_scores
    m, c, g = torch.zeros(2, 4, device="cuda"), torch.eye(4, device="cuda").repeat(2, 1, 1), torch.zeros(2, 4, device="cuda")
    with pytest.raises(NotImplementedError):
        op(m.cpu(), c.cpu(), g.cpu())                                  # no CPU kernel
    for bad in (lambda: op(m, c.cpu(), g), lambda: op(m, c, g.cpu()),                                       # device
                lambda: op(m.double(), c, g), lambda: op(m, c.half(), g), lambda: op(m, c, g.long()),      # dtype
                lambda: op(m, c[:, :3, :3], g), lambda: op(m, c, g[:1]), lambda: op(m[:, :3], c, g), lambda: op(m, c.reshape(2, 16), g),      # shape
                lambda: op(m, c, g, 0), lambda: op(m, c, g, 4097)):                                          # num_samples
        with pytest.raises(RuntimeError):
            bad()
