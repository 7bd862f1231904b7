"""pod_conv1x1_split (K13) across operand range against fp64: ranges.py states the properties, test_operand_range_cpu.py shows on the same
inputs that the contract of pod_split_gemm.h can meet them.  Every kernel form of C1_FORMS; maps 5 x 13 (a full 64-pixel tile + 1) and
9 x 9 at stride 2; Cout 64 and 128; with and without a residual and ReLU; one residual_up2 case; Conv3x3S2 once.

The module shares its name with tests/test_conv1x1_gpu.py so that the GPU run order in tests/conftest.py (GPU_ORDER) places it."""
import pytest
import torch

from tests.operand_range import ranges as R

pytestmark = pytest.mark.gpu
C1 = pytest.mark.parametrize("cin,splits,waves", [pytest.param(*f, id=i) for f, i in zip(R.C1_FORMS, R.C1_FORM_IDS)])


def filter_terms(w):
    """(the f16 terms of the split filter, its trailer word)"""
    from pod_compare_amd.conv1x1 import Conv1x1
    ws = Conv1x1(w.cuda(), None, 1).Ws
    return ws[:-8].cpu(), float(ws[-8:-6].view(torch.float32).cpu())


@C1
def test_activations_times_a_power_of_two_scale_the_result_exactly(cin, splits, waves):
    for p in R.c1_problems(cin, splits, waves):
        R.check_activation_shifts(R.kernel, p)


@C1
def test_weights_times_a_power_of_two_scale_the_result_exactly(cin, splits, waves):
    """... with bit-identical filter terms: only the trailer word differs"""
    for p in R.c1_problems(cin, splits, waves):
        R.check_weight_shifts(R.kernel, p)
    w = R.c1_problem(cin, splits, waves, 5, 13, 1, 128).w
    terms, trailer = filter_terms(w)
    assert trailer == float(w.abs().max())
    for j in R.J_SHIFTS:
        shifted, t = filter_terms(w * 2.0 ** j)
        assert torch.equal(shifted, terms) and t == trailer * 2.0 ** j, j


def test_conv3x3s2_scales_exactly():
    R.check_activation_shifts(R.kernel, R.c3s2_problem())
    R.check_weight_shifts(R.kernel, R.c3s2_problem())


@C1
def test_binade_edges_of_the_record(cin, splits, waves):
    for i, p in enumerate(R.c1_edge_problems(cin, splits, waves)):
        R.check_binade_edges(R.kernel, p, "K13 Cin=%d splits=%d waves=%d map %d" % (cin, splits, waves, i))


@C1
def test_one_record_over_bright_and_dim_data(cin, splits, waves):
    """Section 3: |err| <= 8 x 2^-24 B + T, T = 2^-38 (R sum_c |w| + W sum_c |x|) derived in ranges.py.  Measured on the MI355X
    (profiles/operand_range.md): the f16 matrix instructions honour denormal inputs; c stays below 3 at every d."""
    for i, p in enumerate(R.c1_edge_problems(cin, splits, waves)):
        R.check_mixed(R.kernel, p, "K13 Cin=%d splits=%d waves=%d map %d" % (cin, splits, waves, i))


@C1
def test_ends_of_the_range(cin, splits, waves):
    for i, p in enumerate(R.c1_edge_problems(cin, splits, waves)):
        R.check_ends(R.kernel, p, "K13 Cin=%d splits=%d waves=%d map %d" % (cin, splits, waves, i))
