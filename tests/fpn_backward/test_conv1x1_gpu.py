"""K23 (csrc/k23_fpn_backward.hip) against plain torch on the CPU: pod_conv1x1_wgrad against an fp64 dy.T @ x at the smallest shapes at
which it can go wrong -- several slices with a pixel tail and a channel-tile edge, p6's width, p7's shape at two images, a single
pixel -- repeat launches, operand range, a planted element; the two gathers on integer-valued maps, to the bit.  Measured
figures: profiles/fpn_backward.md."""
import pytest
import torch

from pod_compare_amd import amax, hip, wgrad
from tests.fpn_backward import fb
from tests.head_backward import hb

pytestmark = pytest.mark.gpu
DEV = "cuda"

#        name             pixels  C      K
CASES = {"slices_tail":  (4117,  80,    64),      # 128-pixel slices: 32 whole ones + 21 pixels; C = 80 leaves 48 of the 128-channel tile empty
         "p6_width":     (6,     18432, 64),
         "p7_two_images": (132,  2304,  256),
         # one product per element: the hardest case for the e_hip <= 4 e_f32 side.  torch's fp32 result is ONE rounding of the exact
         # product (at most 2^-24 of it), while the split leaves out the product of the two residual terms and rounds each operand's
         # second term (the planted test below adds these up); with more pixels both sides accumulate roundings and the ratio falls
         # (measured 3.92 here, below 1.8 elsewhere: profiles/fpn_backward.md).  Deterministic: seeded CPU inputs, fixed-order kernel.
         "one_pixel":    (1,     16,    64)}


def _inputs(pixels, C, K, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn((pixels, C), generator=g), torch.randn((pixels, K), generator=g)


@pytest.fixture(scope="module")
def results():
    """Every case once: inputs, the GPU result and both CPU references."""
    out = {}
    for name, (pixels, C, K) in CASES.items():
        x, dy = _inputs(pixels, C, K)
        xg, dyg = x.to(DEV), dy.to(DEV)
        dW, db = wgrad.conv1x1_wgrad(xg, dyg)
        out[name] = (xg, dyg, dW, db, fb.ref_wgrad(x, dy, torch.float32), fb.ref_wgrad(x, dy, torch.float64))
    torch.cuda.synchronize()
    return out


def test_the_first_case_spans_several_slices():
    pixels, C, K = CASES["slices_tail"]
    n = hip.load().pod_conv1x1_wgrad_partials(pixels, C, K)
    slices = (n - 2 * ((pixels + 4095) // 4096) * K) // (K * C)
    assert slices > 1 and pixels % 16 and C % 64


@pytest.mark.parametrize("name", list(CASES))
def test_weight_gradient_matches_fp64(results, name):
    _, _, dW, _, (w32, _), (w64, _) = results[name]
    assert tuple(dW.shape) == tuple(w64.shape) and bool(torch.isfinite(dW).all())
    hb.check("c1 dW " + name, dW, w32, w64)


@pytest.mark.parametrize("name", list(CASES))
def test_bias_gradient_is_the_column_sum(results, name):
    _, _, _, db, (_, b32), (_, b64) = results[name]
    assert bool(torch.isfinite(db).all())
    hb.check("c1 db " + name, db, b32, b64)


@pytest.mark.parametrize("name", list(CASES))
def test_repeat_launches_are_bit_equal(results, name):
    xg, dyg, dW, db = results[name][:4]
    dW2, db2 = wgrad.conv1x1_wgrad(xg, dyg)
    assert torch.equal(dW, dW2) and torch.equal(db, db2)
    dW3, none = wgrad.conv1x1_wgrad(xg, dyg, bias=False)
    assert none is None and torch.equal(dW, dW3)


@pytest.mark.parametrize("name", list(CASES))
def test_operand_range_scales_exactly(results, name):
    """An operand times a power of two under a correct record: the f16 terms are the same, so the result is the scaled result to the bit."""
    xg, dyg, dW, db = results[name][:4]
    dW2, db2 = wgrad.conv1x1_wgrad(xg * 2.0 ** 12, dyg)
    assert torch.equal(dW2, dW * 2.0 ** 12) and torch.equal(db2, db)
    dW3, db3 = wgrad.conv1x1_wgrad(xg, dyg * 2.0 ** -12)
    assert torch.equal(dW3, dW * 2.0 ** -12) and torch.equal(db3, db * 2.0 ** -12)


def test_planted_output_gradient_in_the_last_pixel_and_channel():
    """dY zero but for its last element: dW's last row is that pixel's row of X times it, a single product each, and every other row is
    exactly zero -- the tail's zero fill contributes nothing.  The bound on the single product x d, from the formats (pod_split_gemm.h):
    each operand's two f16 terms miss its scaled value by at most 2^-23 of it; the product of the two residual terms, which the three
    partial products leave out, is at most 2^-11 * 2^-11 = 2^-22 of x d; the partial products are exact in fp32 and two fp32 additions
    join them, 2^-24 each; unscaling, the fp64 sum of one slice and its fp32 store are exact.  2^-23 + 2^-23 + 2^-22 + 2 * 2^-24 =
    2.5 * 2^-22."""
    pixels, C, K = CASES["slices_tail"]
    x, _ = _inputs(pixels, C, K, seed=3)
    dy = torch.zeros((pixels, K))
    dy[-1, -1] = -0.7321
    dW, db = wgrad.conv1x1_wgrad(x.to(DEV), dy.to(DEV))
    dW, want = dW.cpu().double(), x[-1].double() * float(dy[-1, -1])
    print("planted: largest relative error %.3e (bound %.3e)" % (float(((dW[-1] - want).abs() / want.abs()).max()), 2.5 * 2.0 ** -22))
    assert bool(((dW[-1] - want).abs() <= 2.5 * 2.0 ** -22 * want.abs()).all()), float((dW[-1] - want).abs().max())
    assert bool((dW[:-1] == 0).all())
    assert float(db[-1]) == float(dy[-1, -1]) and bool((db[:-1] == 0).all())


def _ints(shape, g, lo=-8, hi=9):
    return torch.randint(lo, hi, shape, generator=g).float()


@pytest.mark.parametrize("h,w,C", [(5, 6, 16), (4, 7, 64)])
@pytest.mark.parametrize("with_gate", [False, True], ids=["plain", "gate"])
@pytest.mark.parametrize("with_add", [False, True], ids=["noadd", "add"])
def test_col2im_equals_autograd_through_unfold(h, w, C, with_gate, with_add):
    g = torch.Generator().manual_seed(h * 100 + w)
    ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    dcols = _ints((ho * wo, 9 * C), g)
    gate = _ints((h * w, C), g, -2, 3) if with_gate else None           # zeros among them: the gate is > 0, not >= 0
    add = _ints((h * w, C), g) if with_add else None
    want = fb.ref_col2im(dcols.double(), h, w, gate, add)
    dev = lambda t: None if t is None else t.to(DEV)
    dx = wgrad.col2im3x3s2_cl(dev(dcols), h, w, gate=dev(gate), add=dev(add))
    assert torch.equal(dx.cpu().double(), want)
    assert float(amax.of(dx).max()) == float(dx.abs().max())
    if with_add:                                                          # in place on the gradient the map already has
        buf = dev(add)
        assert wgrad.col2im3x3s2_cl(dev(dcols), h, w, gate=dev(gate), add=buf, out=buf) is buf and torch.equal(buf, dx)


def test_col2im_beyond_one_grid_trip():
    """The element-wise loop the gathers share (pod_wgrad.h), past what one trip of the grid covers: 4096 workgroups x 256 lanes =
    1 048 576 quads, and a 129 x 129 map of 256 channels has 1 065 024 -- the second trip takes the last 16 448.  Gate and add, whole map
    against the fp64 reference (about a second on the CPU), to the bit; the record is the result's abs-max."""
    h = w = 129
    C, g = 256, torch.Generator().manual_seed(129)
    assert h * w * C // 4 == 1065024 > 4096 * 256
    dcols, gate, add = _ints((65 * 65, 9 * C), g), _ints((h * w, C), g, -2, 3), _ints((h * w, C), g)
    want = fb.ref_col2im(dcols.double(), h, w, gate, add)
    dx = wgrad.col2im3x3s2_cl(dcols.to(DEV), h, w, gate=gate.to(DEV), add=add.to(DEV))
    assert torch.equal(dx.cpu().double(), want)
    assert float(amax.of(dx).max()) == float(dx.abs().max())


@pytest.mark.parametrize("h,w", [(5, 7), (4, 6)])
def test_upsample2_sum_equals_autograd_through_nearest_interpolation(h, w):
    C, g = 64, torch.Generator().manual_seed(h)
    ht, wt = (h + 1) // 2, (w + 1) // 2
    assert (ht, wt) == {(5, 7): (3, 4), (4, 6): (2, 3)}[(h, w)]
    child, add = _ints((h * w, C), g), _ints((ht * wt, C), g)
    want = fb.ref_upsample2_sum(child.double(), h, w, add)
    out = torch.empty((ht * wt, C), device=DEV)
    top = wgrad.upsample2_sum_cl(child.to(DEV), h, w, add.to(DEV), out=out)
    assert top is out and torch.equal(top.cpu().double(), want)
    assert float(amax.of(top).max()) == float(top.abs().max())
    buf = add.to(DEV)
    assert wgrad.upsample2_sum_cl(child.to(DEV), h, w, buf) is buf and torch.equal(buf, top)      # in place on `add`


def test_bad_geometry_and_cpu_tensors_raise():
    """Every refusal comes before a launch: the library's entries are not reached, or return POD_E_INVALID from their argument checks."""
    x, dy = torch.zeros((35, 16)), torch.zeros((35, 64))
    bad = [lambda: wgrad.conv1x1_wgrad(x, dy),                                                          # CPU tensors
           lambda: wgrad.conv1x1_wgrad(x.to(DEV), dy[:34].to(DEV)),                                     # pixel counts differ
           lambda: wgrad.conv1x1_wgrad(torch.zeros((35, 24), device=DEV), dy.to(DEV)),                  # C % 16
           lambda: wgrad.conv1x1_wgrad(x.to(DEV), torch.zeros((35, 96), device=DEV)),                   # K % 64
           lambda: wgrad.conv1x1_wgrad(x.to(DEV), torch.zeros((35, 576), device=DEV)),                  # K > 512
           lambda: wgrad.conv1x1_wgrad(torch.zeros((0, 16), device=DEV), torch.zeros((0, 64), device=DEV)),
           lambda: wgrad.col2im3x3s2_cl(torch.zeros((6, 144)), 4, 6),                                   # CPU
           lambda: wgrad.col2im3x3s2_cl(torch.zeros((6, 144), device=DEV), 5, 6),                       # 5 x 6 has 9 patch rows
           lambda: wgrad.col2im3x3s2_cl(torch.zeros((6, 144), device=DEV), 4, 6, gate=torch.zeros((24, 32), device=DEV)),
           lambda: wgrad.upsample2_sum_cl(torch.zeros((35, 64)), 5, 7, torch.zeros((12, 64))),          # CPU
           lambda: wgrad.upsample2_sum_cl(torch.zeros((35, 64), device=DEV), 5, 7, torch.zeros((6, 64), device=DEV)),      # the top is 3 x 4
           lambda: wgrad.upsample2_sum_cl(torch.zeros((35, 64), device=DEV), 7, 5, torch.zeros((12, 64), device=DEV), out=torch.zeros((12, 32), device=DEV))]
    for f in bad:
        with pytest.raises(hip.PodError):
            f()
