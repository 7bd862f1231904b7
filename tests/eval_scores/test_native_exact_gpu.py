"""The draws of pod_reg_scores against the host restatement (scores_ref.eval_score_normals): the expected tensor is host words -> the
kernels' own box_muller16 (pod_debug_box_muller16) -> host layout, so the comparison is torch.equal -- the method of
tests/rng/test_native_exact_gpu.py, whose name this module shares for its place in the GPU run order (tests/conftest.py: GPU_ORDER)."""
import numpy as np
import pytest
import torch

from tests.eval_instrument import instrument_ref as ir
from tests.eval_scores import gpu_common as gc
from tests.rng import rng_ref as rr

pytestmark = pytest.mark.gpu
KEY = (0x9E3779B9 << 32) | 77          # both key words in use


@pytest.mark.parametrize("M", [1, 6, 127, 128, 129, 301])
def test_eval_score_draws_equal_the_host_map(M):
    """M + 1 samples per row, M odd and even; from M = 127 on a lane takes a second trip and sample 128 -- the partner of lane 63's sample
    127 -- comes from lane 0 of that trip.  Six rows: two workgroups, the second half full; the counter's first word is the row."""
    n = 6
    means, covs, gt = ir.nll_family("wishart", n)
    eps = gc.reg_scores(means, covs, gt, M=M, seed=KEY, want_eps=True)["eps"]
    assert torch.equal(eps, gc.expected_normals(KEY, np.arange(n), M))


def test_eval_score_draws_are_not_the_training_loss_draws():
    """The same key, rows and sample count on K27's stream word (rows as anchors of image 0): different normals everywhere but by chance."""
    n, M = 6, 129
    means, covs, gt = ir.nll_family("wishart", n)
    eps = gc.reg_scores(means, covs, gt, M=M, seed=KEY, want_eps=True)["eps"]
    word, which = rr.reg_score_normals(KEY, np.arange(n), np.zeros(n, dtype=np.int64), M)
    other = torch.gather(gc.gpu_box_muller(word), -1, torch.from_numpy(which.astype(np.int64))[..., None])[..., 0]
    assert other.shape == eps.shape and float((other == eps).float().mean()) < 1e-3
