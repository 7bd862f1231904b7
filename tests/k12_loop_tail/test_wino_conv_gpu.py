"""The end of the K loop of pod_wino_conv3x3_split (csrc/k12_wino_conv_split.hip).  A workgroup whose chunk count (16 input channels per
chunk) is a multiple of 4 runs its last four chunks as tail forms that issue nothing for data past the last chunk -- no stage loads, no
stage parks, and a last chunk that prepares no next one; every other count keeps the clamped generic path.  Same arithmetic either way:

* a convolution of C = 16 n channels and the same convolution with 16 more input channels that are zero in the activations AND in the
  weights give the same bits -- the extra chunk adds exact zeros and moves neither operand scale, so the pair runs one sum through two
  different ends of the loop (4 chunks against 5, 8 against 9, 16 against 17, ...);
* against torch's conv2d at the channel counts the model runs, whole and cut into partial sums;
* a launch's bits do not depend on what an earlier launch left in the LDS stages the tail no longer fills.

The module shares its name with tests/test_wino_conv_gpu.py (the same kernel's tests) so that the GPU run order in tests/conftest.py
(GPU_ORDER, keyed by module name) gives it a place."""
import pytest
import torch
import torch.nn.functional as F

from pod_compare_amd import amax
from pod_compare_amd.wino import WinoConv, block_table, level_pixel_offsets

pytestmark = pytest.mark.gpu
TOL = 2e-5
LEVELS, COPIES = [(17, 33), (6, 11)], 2          # partial blocks, more than one block per level, two images
ONE_MAP = [(13, 17)]


def flat(xs):
    return torch.cat([x.permute(0, 2, 3, 1).reshape(-1, x.shape[1]) for x in xs]).contiguous()


def make(levels, copies, c, k, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    w = torch.randn(k, c, 3, 3, device="cuda", generator=g) * (2.0 / (9 * c)) ** 0.5
    b = torch.randn(k, device="cuda", generator=g)
    xs = [torch.randn(copies, c, h, wd, device="cuda", generator=g) for h, wd in levels]
    return w, b, xs


def zero_chunk(w, src):
    """16 more input channels, zero in the weights and in the activations"""
    return (torch.cat([w, torch.zeros(w.shape[0], 16, 3, 3, device="cuda")], dim=1).contiguous(),
            torch.cat([src, torch.zeros(src.shape[0], 16, device="cuda")], dim=1).contiguous())


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32])
def test_a_zero_chunk_changes_no_bit(n):
    """n chunks against n + 1 chunks whose last is zero: channels-last with bias + ReLU + dropout (the masks are keyed by output element:
    the same for both) and its published abs-max record, and NCHW planes of 36 channels."""
    p, seed, offset = 0.2, 1234, 5 << 34
    table = block_table(LEVELS, COPIES, "cuda", channels=max(512, 16 * (n + 1)))      # one table for both: 528 channels behind n = 32
    for k, planes in ((64, False), (36, True)):
        w, b, xs = make(LEVELS, COPIES, 16 * n, k, seed=100 * n + k)
        src = flat(xs)
        wp, sp = zero_chunk(w, src)
        outs, records = [], []
        for ww, ss in ((w, src), (wp, sp)):
            conv = WinoConv(ww, b, split=True)
            if planes:
                dst = torch.full((level_pixel_offsets(LEVELS, COPIES)[-1] * k,), float("nan"), device="cuda")
                conv(ss, dst, table, planes=True)
            else:
                dst = torch.full((ss.shape[0], k), float("nan"), device="cuda")
                conv(ss, dst, table, relu=True, dropout_p=p, seed=seed, offset=offset)
                record = amax.of(dst)
                assert dst._pod_amax[0] is record                      # the store pass's own record
                records.append(record.clone())
            outs.append(dst)
        assert bool(torch.isfinite(outs[0]).all())
        assert torch.equal(outs[0], outs[1]), (n, planes)
        if not planes:
            assert float(records[0].max()) > 0.0
            assert torch.equal(records[0], records[1]), n


@pytest.mark.parametrize("k,planes", [(64, False), (36, True)], ids=["channels-last-64", "planes-36"])
@pytest.mark.parametrize("c", [64, 128, 256, 512])
def test_against_conv2d_at_the_models_channel_counts(c, k, planes):
    """4, 8, 16 and 32 chunks: every peeled count, within the kernel's usual bound of torch's conv2d"""
    w, b, xs = make(LEVELS, COPIES, c, k, seed=c + k)
    src, table = flat(xs), block_table(LEVELS, COPIES, "cuda")
    offs = level_pixel_offsets(LEVELS, COPIES)
    conv = WinoConv(w, b, split=True)
    if planes:
        out = conv(src, torch.full((offs[-1] * k,), float("nan"), device="cuda"), table, planes=True)
    else:
        out = conv(src, torch.full((src.shape[0], k), float("nan"), device="cuda"), table)
    for i, (x, (h, wd)) in enumerate(zip(xs, LEVELS)):
        want = F.conv2d(x, w, b, padding=1)
        if planes:
            got = out[offs[i] * k:offs[i + 1] * k].view(COPIES, k, h, wd)
        else:
            got = out[offs[i]:offs[i + 1]].view(COPIES, h, wd, k).permute(0, 3, 1, 2)
        assert bool(torch.isfinite(got).all())
        assert float((got - want).abs().max()) <= TOL * max(1.0, float(want.abs().max()))


@pytest.mark.parametrize("c,splits", [(64, 2), (128, 2), (256, 2), (256, 4), (512, 4)])
def test_partial_sums_over_the_input_channels(c, splits):
    """2, 4 and 8 chunks per workgroup set (2: the generic path, ending in chunk 1): bit-reproducible, equal to the unsplit launch to
    rounding (the bound of tests/test_wino_conv_gpu.py: test_small_maps_split_over_the_input_channels), equal to conv2d within TOL"""
    (h, wd), k = ONE_MAP[0], 64
    w, b, xs = make(ONE_MAP, 1, c, k, seed=c * splits)
    x = xs[0].relu()
    src, table = flat([x]), block_table(ONE_MAP, 1, "cuda")
    conv = WinoConv(w, b, split=True)
    want = F.conv2d(x, w, b, padding=1).relu()
    scale = max(1.0, float(want.abs().max()))
    outs = []
    for s in (1, splits, splits):
        dst = torch.full((k * h * wd,), float("nan"), device="cuda")
        conv.planes_of_one_image(src, dst, table, relu=True, n_splits=s)
        outs.append(dst.view(1, k, h, wd))
        assert float((outs[-1] - want).abs().max()) <= TOL * scale
    assert torch.equal(outs[1], outs[2])
    assert float((outs[0] - outs[1]).abs().max()) <= 4e-6 * scale


@pytest.mark.parametrize("c", [64, 128])
def test_bits_do_not_depend_on_the_launch_before(c):
    """The tail leaves stage space unparked: a C = 64 and a C = 128 launch give the same bits alone and straight behind a C = 256 launch
    of another shape on the same stream, whose workgroups left their own patches and output staging in the LDS."""
    w, b, xs = make(LEVELS, COPIES, c, 64, seed=c)
    src, table = flat(xs), block_table(LEVELS, COPIES, "cuda")
    conv = WinoConv(w, b, split=True)
    wb, bb, xb = make([(23, 40)], 3, 256, 128, seed=7)
    big, big_src, big_table = WinoConv(wb, bb, split=True), flat(xb), block_table([(23, 40)], 3, "cuda")
    big_dst = torch.empty(big_src.shape[0], 128, device="cuda")
    torch.cuda.synchronize()
    alone = conv(src, torch.full((src.shape[0], 64), float("nan"), device="cuda"), table, relu=True)
    torch.cuda.synchronize()
    behind_dst = torch.full((src.shape[0], 64), float("nan"), device="cuda")
    big(big_src, big_dst, big_table, relu=True)
    behind = conv(src, behind_dst, table, relu=True)
    assert bool(torch.isfinite(alone).all())
    assert torch.equal(alone, behind)
