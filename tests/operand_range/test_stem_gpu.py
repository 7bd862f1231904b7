"""pod_stem7x7_split (K14) across operand range against fp64 (ranges.py; the module is named after tests/test_stem_gpu.py for its place in
tests/conftest.py's GPU_ORDER).  Frames 17 x 33 (9 x 17 outputs: ragged 8 x 8 tiles) and 7 x 250; float input without mean / std, where
the record is the frame's own; one uint8 frame under the analytic record."""
import pytest
import torch

from tests.operand_range import ranges as R

pytestmark = pytest.mark.gpu
FRAMES = pytest.mark.parametrize("h,w", R.STEM_FRAMES)


@FRAMES
def test_power_of_two_shifts_scale_the_result_exactly(h, w):
    from pod_compare_amd.conv1x1 import Stem7x7
    for relu in (False, True):
        R.check_activation_shifts(R.kernel, R.stem_problem(h, w, relu))
    p = R.stem_problem(h, w)
    R.check_weight_shifts(R.kernel, p)
    base = Stem7x7(p.w.cuda(), None).Ws
    for j in R.J_SHIFTS:
        ws = Stem7x7((p.w * 2.0 ** j).cuda(), None).Ws
        assert torch.equal(ws[:-8], base[:-8]) and float(ws[-8:-6].view(torch.float32)) == float(p.w.abs().max()) * 2.0 ** j, j


@FRAMES
def test_binade_edges_of_the_record(h, w):
    R.check_binade_edges(R.kernel, R.stem_problem(h, w), "K14 %dx%d" % (h, w))


@FRAMES
def test_one_record_over_bright_and_dim_data(h, w):
    """Section 3 with the bar of tests/test_stem_gpu.py (c <= 8) and T = 2^-38 (R sum |w| + W sum |x|) over the taps inside the image"""
    R.check_mixed(R.kernel, R.stem_problem(h, w), "K14 %dx%d" % (h, w))


@FRAMES
def test_ends_of_the_range(h, w):
    R.check_ends(R.kernel, R.stem_problem(h, w), "K14 %dx%d" % (h, w))


def test_uint8_frame_under_its_analytic_record():
    R.check_u8_frame(R.kernel, R.stem_u8_problem(), "K14 uint8 frame under its analytic record")
