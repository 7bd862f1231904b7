"""Two real ranks of a data-parallel run on ONE GPU: rank 0 is the test process, rank 1 the one process that is started, the collective is
gloo's (the bucket staged through pinned host memory, because gloo cannot move device buffers; RCCL reduces it in place).  Two steps of the
small --train-backbone trainer on four frames, two per rank: both ranks end with the same bits, and those are the bits of the virtual-rank
emulation in one process (tests/data_parallel/dp.py) on the same frames."""
import pytest

from tests.data_parallel import dp

pytestmark = pytest.mark.gpu


def test_two_ranks_over_gloo_end_bit_equal_and_as_the_virtual_ranks(tmp_path):
    ranks = dp.run_two_ranks(tmp_path)                     # (each rank asserts bucket.host_staged)
    dp.assert_same_state(ranks[0], ranks[1], "rank 0 against rank 1")
    assert ranks[0]["iteration"] == 2 and all(bool(m.any()) for m in ranks[0]["momentum"])
    virtual = dp.emulate(world=2, steps=2)
    for r in range(2):
        dp.assert_same_state(ranks[r], virtual[r], "rank %d against its virtual twin" % r, loss_state=True)
