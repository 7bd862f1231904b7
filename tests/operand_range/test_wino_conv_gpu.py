"""pod_wino_conv3x3_split (K12) across operand range against fp64 (ranges.py; named after tests/test_wino_conv_gpu.py for its place in
tests/conftest.py's GPU_ORDER).  Levels 9 x 13 and 5 x 7 (the second below one block), two copies, C = 32, K = 64 channels-last; K = 36 as
planes; C = 16; the form cut over its input channels at (6, 11, 128, 64); one image per level stored three times under dropout masks
(p = 0.25: a mask depends on seed and offset only, so both runs of a comparison see the same one)."""
import pytest
import torch

from tests.operand_range import ranges as R

pytestmark = pytest.mark.gpu
FORMS = [n for n in R.WINO_NAMES if n != "replicas"]


@pytest.mark.parametrize("name", R.WINO_NAMES)
def test_power_of_two_shifts_scale_the_result_exactly(name):
    """Section 1: the Winograd transforms, the fp32 accumulation, the store pass's multiply-add and the dropout gain all commute with an
    exact power of two; the filter terms U do not change with the weights' binade, only the trailer word does."""
    from pod_compare_amd.wino import WinoConv
    p = R.wino_problem(name)
    R.check_activation_shifts(R.kernel, p)
    R.check_weight_shifts(R.kernel, p)
    base = WinoConv(p.w.cuda(), None, split=True).U
    for j in R.J_SHIFTS:
        u = WinoConv((p.w * 2.0 ** j).cuda(), None, split=True).U
        assert torch.equal(u[:-8], base[:-8]) and float(u[-8:-6].view(torch.float32)) == float(base[-8:-6].view(torch.float32)) * 2.0 ** j, j


@pytest.mark.parametrize("name", FORMS)
def test_binade_edges_of_the_record(name):
    R.check_binade_edges(R.kernel, R.wino_problem(name), "K12 " + name)


def test_the_worst_gain_of_the_input_transform():
    """'gain of Bt4 (x) Bt6 < 32' (WINO_V_TOP): the largest product of absolute row sums is 2 x 10 = 20 (rows d0 - d2 and 4 t0 - 5 t2 + t4).
    One patch holds +- nextafter(16, 0) in that sign pattern in every channel: the transformed value is 20 x max, scaled to just below
    20 x 2^10 -- an f16 number.  The tile's outputs: finite, within C_BOUND of fp64."""
    gain = R.worst_rows(R.BT4, R.BT6)[2]
    assert gain == 20 < 32
    q, rows = R.worst_gain_problem(R.wino_problem("cl"))
    want, bound, _ = q.reference()
    y = R.kernel(q)
    assert bool(torch.isfinite(y).all())
    c = float(((y.double() - want).abs() / (R.EPS * bound))[rows].max())
    print("operand_range K12 worst input-transform gain (%d x max): c = %.3f over the tile, %.3f over the launch"
          % (gain, c, float(((y.double() - want).abs() / (R.EPS * bound)).max())))
    assert c <= R.BAR["wino"]


@pytest.mark.parametrize("name", FORMS)
def test_one_record_over_bright_and_dim_data(name):
    """Section 3: the second level x 2^-d under the launch's one record (a tile never leaves its level's canvas), and homogeneous data under
    a record 2^d too high.  |err| <= 32 x 2^-24 B + T,  T = gA gG (2^-33 R sum |w| + 2^-38 gB W C X)  (ranges.py derives it: the activations
    are split after the input transform, under WINO_V_TOP = 9; gG = 1.5 and gA = 57 are the filter and output transforms' gains)."""
    R.check_mixed(R.kernel, R.wino_problem(name), "K12 " + name)


@pytest.mark.parametrize("name", FORMS)
def test_ends_of_the_range(name):
    R.check_ends(R.kernel, R.wino_problem(name), "K12 " + name)
