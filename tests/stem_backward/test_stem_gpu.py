"""K30's two kernels directly (csrc/k30_stem_backward.hip through pod_compare_amd/wgrad.py): the stem's 7x7 weight gradient against
torch.nn.grad.conv2d_weight in fp64 and fp32 on the CPU, the max-pool's backward with the stem's ReLU gate against CPU autograd, and what
the entries refuse.  Measured figures: profiles/stem_backward.md."""
import pytest
import torch

from pod_compare_amd import amax, hip, wgrad
from tests.head_backward import hb
from tests.stem_backward import sb

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MEAN, STD = torch.tensor([103.530, 116.280, 123.675]), torch.tensor([57.375, 57.120, 58.395])

# (name, frame dtype, frame (hi, wi), padded (H, W), normalised on load)
CASES = [("u8_45x70_in_64x96", torch.uint8, (45, 70), (64, 96), True),       # the image edge inside a tile; both kinds of padding
         ("f32_64x96_normalised", torch.float32, (64, 96), (64, 96), False),
         ("u8_96x160_slices", torch.uint8, (96, 160), (96, 160), True),      # more than one slice per image
         ("f32_19x27_part_tiles", torch.float32, (19, 27), (19, 27), False)]  # 10 x 14 outputs: the last tile row / column is partly outside
B = 2


def _case(dtype, hw, padded, normalise, seed):
    g = torch.Generator().manual_seed(seed)
    if dtype == torch.uint8:
        frames = torch.randint(0, 256, (B, 3) + hw, generator=g, dtype=torch.uint8)
    else:
        frames = torch.randn((B, 3) + hw, generator=g) * (40.0 if normalise else 1.0)
    ho, wo = sb.out_hw(*padded)
    ds = torch.randn((B * ho * wo, 64), generator=g) * (torch.rand((B * ho * wo, 64), generator=g) < 0.5)       # about half zeros: a gate's pattern
    return frames, ds


@pytest.mark.parametrize("name,dtype,hw,padded,normalise", CASES, ids=[c[0] for c in CASES])
def test_stem_wgrad_matches_conv2d_weight(name, dtype, hw, padded, normalise):
    """dW against torch.nn.grad.conv2d_weight on the normalised, zero-padded frames, in fp64 (the reference) and fp32 (the referee), by
    hb.check's two-sided rule.  pod_stem7x7_split accepts any extent (1 <= frame <= padded <= 16384), so outputs that are no whole number of
    8 x 8 tiles exist: the 19 x 27 case (10 x 14 outputs) is the smallest kind, with part tiles along both axes."""
    frames, ds = _case(dtype, hw, padded, normalise, seed=len(name))
    mean, std = (MEAN, STD) if normalise else (None, None)
    args = (frames.to(DEV), ds.to(DEV), padded, None if mean is None else mean.to(DEV), None if std is None else std.to(DEV))
    dW = wgrad.stem7x7_wgrad(*args)
    assert tuple(dW.shape) == (64, 3, 7, 7) and dW.dtype == torch.float32 and bool(torch.isfinite(dW).all())
    assert torch.equal(dW, wgrad.stem7x7_wgrad(*args))               # fixed slices, fixed-order fp64 sum, no atomics
    n = int(hip.load().pod_stem7x7_wgrad_partials(B, hw[0], hw[1], padded[0], padded[1]))
    assert n > 0 and n % (64 * 192) == 0
    if name.endswith("slices"):
        assert n // (64 * 192) > B, "the slice-order reduce needs more than one slice per image"
    ref = {dt: sb.ref_stem_wgrad(sb.normalised_padded(frames, mean, std, padded, dt), ds, dt) for dt in (torch.float32, torch.float64)}
    hb.check("stem7x7_wgrad " + name, dW, ref[torch.float32], ref[torch.float64])


POOL_SHAPES = [(7, 9, 4), (8, 8, 64), (32, 48, 64)]


@pytest.mark.parametrize("h,w,C", POOL_SHAPES, ids=["%dx%dx%d" % s for s in POOL_SHAPES])
def test_pool_backward_equals_cpu_autograd_exactly(h, w, C):
    """s from the levels {0, 1, 2}: ties at positive values and all-zero windows both occur.  dP in multiples of 2^-10 inside (-0.5, 0.5):
    every sum of up to four terms is exact in fp32 in any order, so the comparison with the fp64 reference is torch.equal."""
    g = torch.Generator().manual_seed(h * w + C)
    s = torch.randint(0, 3, (h * w, C), generator=g).float()
    hq, wq = sb.out_hw(h, w)
    dp = torch.randint(-511, 512, (hq * wq, C), generator=g).float() / 1024.0
    ds = wgrad.maxpool3x3s2_backward_cl(s.to(DEV), dp.to(DEV), h, w)
    want = sb.ref_pool_backward(s, dp, h, w)
    assert tuple(ds.shape) == (h * w, C) and torch.equal(ds.cpu().double(), want)
    assert bool((want != 0).any()) and bool((want[s == 0] == 0).all())
    assert float(amax.of(ds).max()) == float(ds.abs().max())         # the record the pass published
    # under a caller's record, into a caller's rows (the trainer's per-image use)
    out, rec = torch.full((h * w, C), 7.0, device=DEV), amax.word(torch.device(DEV))
    assert wgrad.maxpool3x3s2_backward_cl(s.to(DEV), dp.to(DEV), h, w, out=out, record=rec) is out
    assert torch.equal(out, ds) and float(rec.max()) == float(ds.abs().max())


def test_what_the_entries_refuse_raises_before_any_launch():
    frames = torch.zeros((1, 3, 16, 16), dtype=torch.uint8)
    ds = torch.zeros((64, 64), device=DEV)
    mean, std = MEAN.to(DEV), STD.to(DEV)
    with pytest.raises(hip.PodError):                    # a frame on the CPU
        wgrad.stem7x7_wgrad(frames, ds, (16, 16), mean, std)
    with pytest.raises(hip.PodError):                    # 8 x 8 outputs are 64 rows of dS, not 63
        wgrad.stem7x7_wgrad(frames.to(DEV), ds[:63].contiguous(), (16, 16), mean, std)
    with pytest.raises(hip.PodError):                    # an extent pod_stem7x7_split refuses: the frame larger than its padded size
        wgrad.stem7x7_wgrad(frames.to(DEV), ds, (8, 16), mean, std)
    with pytest.raises(hip.PodError):                    # ... and a padded size past 16384
        wgrad.stem7x7_wgrad(frames.to(DEV), ds, (16, 16386), mean, std)
    with pytest.raises(hip.PodError):                    # a uint8 frame without mean / std
        wgrad.stem7x7_wgrad(frames.to(DEV), ds, (16, 16))
    with pytest.raises(hip.PodError):                    # C % 4 != 0
        wgrad.maxpool3x3s2_backward_cl(torch.zeros((16, 6), device=DEV), torch.zeros((4, 6), device=DEV), 4, 4)
    with pytest.raises(hip.PodError):                    # 2 x 2 pooled rows, not 3
        wgrad.maxpool3x3s2_backward_cl(torch.zeros((16, 8), device=DEV), torch.zeros((3, 8), device=DEV), 4, 4)
    with pytest.raises(hip.PodError):                    # s on the CPU
        wgrad.maxpool3x3s2_backward_cl(torch.zeros((16, 8)), torch.zeros((4, 8), device=DEV), 4, 4)
    lib = hip.load()                                     # the entries themselves: POD_E_INVALID, nothing enqueued
    assert lib.pod_stem7x7_wgrad_partials(1, 16, 16, 8, 16) == 0 and lib.pod_stem7x7_wgrad_partials(0, 16, 16, 16, 16) == 0
    assert lib.pod_stem7x7_wgrad(None, 1, 1, 16, 16, None, None, None, 16, 16, None, None, None, None, None) == -1
    assert lib.pod_maxpool3x3s2_backward_cl(None, None, None, 4, 4, 8, None, None) == -1
