"""pod_pdq_pairs' structure on the GPU: a pair's bits depend on its detection, its ground truth, the frame and p_min alone -- not on the
batch, the order of the detections or the launch -- and the zero rules hold exactly.  (The sentinels behind every output are checked by
gpu_common.pairs on every call.)

The module shares its name with tests/test_native_exact_gpu.py for its place in the GPU run order (tests/conftest.py: GPU_ORDER)."""
import numpy as np
import pytest

from tests.pdq import fixtures as fx
from tests.pdq import gpu_common as gc
from tests.pdq import pdq_ref as pr

pytestmark = pytest.mark.gpu
KEYS = pr.PLANES + ("sum_fg", "sum_bg")


def _same_bits(a, b, cols=None):
    for k in KEYS:
        x = a[k] if cols is None else a[k][:, cols]
        assert x.tobytes() == b[k].tobytes(), k


def test_a_pairs_bits_do_not_depend_on_batch_order_or_launch():
    ims = fx.all_images()
    batch = gc.pairs(ims)
    again = gc.pairs(ims)
    for a, b in zip(batch, again):
        _same_bits(a, b)                                            # two launches
    for m in (0, 1, 2, 5, 6):
        _same_bits(gc.pairs([ims[m]])[0], batch[m])                 # alone
    three = gc.pairs([ims[5], ims[1], ims[0]])                      # in a batch of three, at other offsets
    _same_bits(three[0], batch[5])
    _same_bits(three[1], batch[1])
    _same_bits(three[2], batch[0])
    order = [4, 0, 5, 2, 1, 3]
    perm = gc.pairs([fx.permuted(ims[1], order)])[0]                # the detections permuted: the columns move with them
    _same_bits(batch[1], perm, cols=order)
    assert np.array_equal(batch[1]["invalid"][order], perm["invalid"])


def test_zero_rules_hold_exactly():
    edge, zero, many = gc.pairs([fx.edge_cases(), fx.zero_rules(), fx.many_ground_truths()])
    ref = gc.referee()
    for k in KEYS:
        assert (edge[k][:, 1] == 0.0).all(), k                      # wholly off the frame: no pixel of T on it
        assert (zero[k][1] == 0.0).all(), k                         # n_i = 0
        assert (zero[k][2] == 0.0).all(), k                         # S_i and T_j disjoint
        assert (zero[k][:, 1] == 0.0).all() and (zero[k][:, 3] == 0.0).all(), k          # invalid detections
        assert ((many[k] == 0.0) == (ref[5]["pPDQ"] == 0.0)).all(), k                      # exactly the referee's no-overlap pairs
    assert zero["invalid"].tolist() == [False, True, False, True] and not edge["invalid"].any()
    assert zero["pPDQ"][0, 0] > 0.0 and zero["pPDQ"][0, 2] > 0.0    # the invalid detection affects neither neighbour
    alone = gc.pairs([dict(fx.zero_rules(), **{k: fx.zero_rules()[k][[0, 2]] for k in ("means", "covs", "probs")})])[0]
    for k in KEYS:
        assert alone[k].tobytes() == zero[k][:, [0, 2]].tobytes(), k


def test_no_ground_truth_and_no_detections():
    a, b = gc.pairs([fx.no_ground_truth(), fx.no_detections()])
    assert a["pPDQ"].shape == (0, 2) and b["pPDQ"].shape == (2, 0) and a["invalid"].tolist() == [False, False]
    p_other = gc.pairs([fx.jittered()], p_min=0.05)[0]              # p_min is an argument: a larger one shrinks the segment
    base = gc.pairs([fx.jittered()])[0]
    assert (p_other["sum_bg"] > base["sum_bg"]).all() and (p_other["sum_fg"] <= base["sum_fg"]).all()
