"""The store passes of the Winograd convolutions (csrc/pod_wino.h: wino_store_channels_last, wino_store_planes) on the canvases where
their stepped addressing can go wrong: several images per 16x16 block, a thread's eight rows wrapping from one image into the next (a
1 x 1 map wraps on every step), grid cells beyond the image count, partial blocks -- for the fused bias + ReLU + dropout + abs-max form,
the replica form, the NCHW planes form, and a NaN accumulator.  Both kernels (pod_wino_conv3x3, pod_wino_conv3x3_split) share the
passes and run every case they have an entry for: replicas and the abs-max record exist on the split kernel only.

The module shares its name with tests/test_wino_conv_gpu.py (the same kernels' tests) so that the GPU run order in tests/conftest.py
(GPU_ORDER, keyed by module name) gives it a place."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from pod_compare_amd import amax, hip
from pod_compare_amd.wino import WinoConv, block_table, level_pixel_offsets

pytestmark = pytest.mark.gpu
TOL = 2e-5
C, K = 16, 64
GUARD = 1 << 14            # floats: 64 KB of sentinel on either side of a destination
SENTINEL = 7.0
KERNELS = pytest.mark.parametrize("split", [False, True], ids=["fp32-mfma", "f16x3"])


def flat(xs):
    return torch.cat([x.permute(0, 2, 3, 1).reshape(-1, x.shape[1]) for x in xs]).contiguous()


def make(levels, copies, k, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    w = torch.randn(k, C, 3, 3, device="cuda", generator=g) * (2.0 / (9 * C)) ** 0.5
    b = torch.randn(k, device="cuda", generator=g)
    xs = [torch.randn(copies, C, h, wd, device="cuda", generator=g) for h, wd in levels]
    return w, b, xs


def guarded(pixels, k):
    """(whole buffer, the (pixels, k) destination in its middle): sentinel everywhere"""
    whole = torch.full((2 * GUARD + pixels * k,), SENTINEL, device="cuda")
    return whole, whole[GUARD:GUARD + pixels * k].view(pixels, k)


def guards_untouched(whole):
    return bool((whole[:GUARD] == SENTINEL).all()) and bool((whole[-GUARD:] == SENTINEL).all())


def bias_act(x, b, relu, p, seed, offset):
    hip.check(hip.load().pod_bias_act(x.data_ptr(), b.data_ptr(), None, None, x.numel(), x.shape[-1], 1, 1 if relu else 0, p, seed, offset,
                                      hip.current_stream()), "pod_bias_act")
    return x


@KERNELS
@pytest.mark.parametrize("levels,copies", [([(1, 1), (2, 3), (6, 11)], 19), ([(17, 33)], 2)], ids=["19-small-maps", "partial-blocks"])
def test_fused_mask_and_abs_max_on_awkward_canvases(levels, copies, split):
    """bias + ReLU + dropout + abs-max record in the store pass == the plain convolution followed by pod_bias_act with the same seed and
    offset, bit for bit; nothing outside the destination is written; the record holds max |value before the mask| * 1 / (1 - p)."""
    p, seed, offset = 0.2, 4321, 3 << 34
    w, b, xs = make(levels, copies, K, seed=copies)
    src, table = flat(xs), block_table(levels, copies, "cuda")
    whole, dst = guarded(src.shape[0], K)
    WinoConv(w, b, split=split)(src, dst, table, relu=True, dropout_p=p, seed=seed, offset=offset)
    record = None
    if split:
        record = amax.of(dst)
        assert dst._pod_amax[0] is record and dst._pod_amax[1] == dst._version      # the store pass's own record, not pod_absmax of the masked result
        assert float(record.max()) > 0.0
    plain = WinoConv(w, None, split=split)(src, torch.empty(src.shape[0], K, device="cuda"), table)
    want = bias_act(plain.clone(), b, True, p, seed, offset)
    assert torch.equal(dst, want)
    assert guards_untouched(whole)
    dropped = float((dst == 0).float().mean())
    assert 0.45 < dropped < 0.75                                # ReLU zeroes half, dropout 20 % of the rest
    if split:
        unmasked = bias_act(plain.clone(), b, True, 0.0, 0, 0)
        scale = np.float32(1.0) / (np.float32(1.0) - np.float32(p))
        assert float(record.max()) == float(np.float32(float(unmasked.abs().max())) * scale)


@pytest.mark.parametrize("replicas", [1, 3, 19])
def test_replicas_on_small_maps(replicas):
    """The replica form (split kernel only) == the convolution followed, level by level, by pod_expand_dropout: bit for bit, down to
    the 1 x 1 map, with the guards around the destination untouched."""
    levels, p, seed, offset = [(6, 11), (3, 5), (1, 1)], 0.25, 77, 9 << 34
    w, b, xs = make(levels, 1, K, seed=11)
    src = flat(xs)
    conv = WinoConv(w, b, split=True)
    offn, off1 = level_pixel_offsets(levels, replicas), level_pixel_offsets(levels, 1)
    whole, fused = guarded(offn[-1], K)
    conv.replicas(src, fused, block_table(levels, 1, "cuda", out_copies=replicas), replicas, relu=True, dropout_p=p, seed=seed, offset=offset)
    y = conv(src, torch.empty(src.shape[0], K, device="cuda"), block_table(levels, 1, "cuda"), relu=True)
    want = torch.full((offn[-1], K), float("nan"), device="cuda")
    for i, (h, wd) in enumerate(levels):
        hip.check(hip.load().pod_expand_dropout(y[off1[i]:].data_ptr(), want[offn[i]:].data_ptr(), h * wd * K, replicas, p, seed, offset + offn[i] * K // 8, None,
                                                hip.current_stream()), "pod_expand_dropout")
    assert torch.equal(fused, want)
    assert guards_untouched(whole)


@KERNELS
@pytest.mark.parametrize("k", [36, 63])
def test_planes_of_a_subset_of_the_runs_on_small_maps(k, split):
    """NCHW planes of K real channels (the last batch of channels is partial), widths with W % 4 != 0 (scalar stores) and W % 4 == 0
    (16-byte stores), reading runs first .. first + count - 1 of 5 and writing a buffer of 4 runs whose last run keeps its sentinel."""
    levels, in_copies, first, count, out_copies = [(6, 11), (3, 5), (1, 1), (12, 20)], 5, 2, 3, 4
    w, b, xs = make(levels, in_copies, k, seed=k)
    src = flat(xs)
    offs = level_pixel_offsets(levels, out_copies)
    whole = torch.full((2 * GUARD + offs[-1] * k,), SENTINEL, device="cuda")
    out = whole[GUARD:GUARD + offs[-1] * k]
    WinoConv(w, b, split=split)(src, out, block_table(levels, count, "cuda", in_copies=in_copies, in_first=first, out_copies=out_copies), planes=True)
    for i, (x, (h, wd)) in enumerate(zip(xs, levels)):
        got = out[offs[i] * k:offs[i + 1] * k].view(out_copies, k, h, wd)
        want = F.conv2d(x[first:first + count], w, b, padding=1)
        assert float((got[:count] - want).abs().max()) <= TOL * max(1.0, float(want.abs().max()))
        assert bool((got[count:] == SENTINEL).all())
    assert guards_untouched(whole)


@pytest.mark.parametrize("relu", [True, False], ids=["relu", "no-relu"])
def test_planes_with_an_abs_max_record(relu):
    """PodWinoConv takes out_amax with k_planes > 0 (no Python call site does; the entry serves it): same planes as the launch without
    a record, and the record holds max |what was stored| -- channels past K and pixels outside every image do not count."""
    from pod_compare_amd.wino import grouped_launch
    levels, copies, k = [(6, 11), (3, 5), (1, 1), (12, 20)], 3, 36
    w, b, xs = make(levels, copies, k, seed=8)
    src, table = flat(xs), block_table(levels, copies, "cuda")
    conv = WinoConv(w, b, split=True)
    n = level_pixel_offsets(levels, copies)[-1] * k
    want = conv(src, torch.full((n,), SENTINEL, device="cuda"), table, relu=relu, planes=True)
    got = torch.full((n,), SENTINEL, device="cuda")
    grouped_launch([{"conv": conv, "src": src, "dst": got, "table": table, "planes": True, "out_amax": True}], relu=relu)
    record = amax.of(got)
    assert got._pod_amax[0] is record
    assert torch.equal(got, want)
    assert float(record.max()) == float(got.abs().max())


@KERNELS
@pytest.mark.parametrize("relu", [True, False], ids=["relu", "no-relu"])
def test_nan_accumulator_stores_what_conv_then_bias_act_stores(relu, split):
    """One NaN input pixel: the outputs that are NaN are exactly those of the plain convolution followed by pod_bias_act (behind ReLU a NaN
    is stored as 0; without, it stays NaN unless the mask drops it), and every other output is that reference's, bit for bit."""
    levels, copies, p, seed, offset = [(6, 11), (2, 3)], 3, 0.2, 99, 1 << 34
    w, b, xs = make(levels, copies, K, seed=5)
    src, table = flat(xs), block_table(levels, copies, "cuda")
    src[6 * 11 + 2 * 11 + 4] = float("nan")                       # image 1 of the first level, pixel (2, 4)
    fused = WinoConv(w, b, split=split)(src, torch.empty(src.shape[0], K, device="cuda"), table, relu=relu, dropout_p=p, seed=seed, offset=offset)
    plain = WinoConv(w, None, split=split)(src, torch.empty(src.shape[0], K, device="cuda"), table)
    assert bool(torch.isnan(plain).any())
    want = bias_act(plain, b, relu, p, seed, offset)
    assert torch.equal(torch.isnan(fused), torch.isnan(want))
    assert bool(torch.isnan(fused).any()) == (not relu)
    assert torch.equal(torch.nan_to_num(fused, nan=-1.0), torch.nan_to_num(want, nan=-1.0))
