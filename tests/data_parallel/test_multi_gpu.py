"""The two-rank data-parallel step of tests/data_parallel/test_ensemble_dist_gpu.py over RCCL, one GPU per rank: the bucket is reduced on the
device (host_staged is false, asserted by each rank).  RCCL refuses two ranks on one device: skipped below two GPUs."""
import pytest
import torch

from tests.data_parallel import dp

pytestmark = pytest.mark.gpu
N_GPU = torch.cuda.device_count() if torch.cuda.is_available() else 0


@pytest.mark.skipif(N_GPU < 2, reason="one GPU per rank: needs two")
def test_two_ranks_over_nccl_end_bit_equal(tmp_path):
    ranks = dp.run_two_ranks(tmp_path, backend="nccl", own_gpu=True)
    dp.assert_same_state(ranks[0], ranks[1], "rank 0 against rank 1")
    assert ranks[0]["iteration"] == 2 and all(bool(m.any()) for m in ranks[0]["momentum"])
