"""K22 (csrc/k22_conv3x3_wgrad.hip) against an fp64 torch.nn.grad.conv2d_weight on the CPU: the smallest shapes at which it can go
wrong -- below a tile, across 16-pixel strips and images, two levels with a padded predictor channel, the head's own channel counts,
slice boundaries, planted single elements, operand range, repeat launches -- and the ReLU + dropout gate."""
import pytest
import torch

from pod_compare_amd import amax, wgrad
from tests.head_backward import hb

pytestmark = pytest.mark.gpu
DEV = "cuda"

#        name            levels              B   C    K
CASES = {"below_tile":   ([(5, 7)],            1, 16,  64),
         "strips":       ([(17, 19)],          2, 64,  64),
         "two_levels":   ([(9, 13), (5, 7)],   2, 32,  63),
         "head_shape":   ([(17, 19)],          1, 256, 256),
         "slices_2_34":  ([(300, 20)],         1, 16,  64),      # 2 strips x 300 rows = 600 steps: 2.34 slices, one cut inside a strip
         "one_slice":    ([(256, 16)],         1, 16,  64)}      # 256 steps: exactly one slice


def _inputs(levels, B, C, K, seed=0):
    g = torch.Generator().manual_seed(seed)
    pixels, Kpad = B * sum(h * w for h, w in levels), (K + 63) // 64 * 64
    x = torch.randn((pixels, C), generator=g)
    dy = torch.zeros((pixels, Kpad))
    dy[:, :K] = torch.randn((pixels, K), generator=g)
    return x, dy


@pytest.fixture(scope="module")
def results():
    """Every case once: inputs, the GPU result and both CPU references."""
    out = {}
    for name, (levels, B, C, K) in CASES.items():
        x, dy = _inputs(levels, B, C, K)
        xg, dyg = x.to(DEV), dy.to(DEV)
        if K % 64:                      # garbage in the padded channel, under a record of the real channels
            rec = amax.of(dyg)
            dirty = dyg.clone()
            dirty[:, K:] = 1e30
            dirty[0, K:] = float("nan")
            dyg = amax.attach(dirty, rec)
        dW, db = wgrad.conv3x3_wgrad(xg, dyg, levels, B, K)
        out[name] = (xg, dyg, dW, db, hb.ref_wgrad(x, dy, levels, B, K, torch.float32), hb.ref_wgrad(x, dy, levels, B, K, torch.float64))
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("name", list(CASES))
def test_weight_gradient_matches_fp64(results, name):
    _, _, dW, _, (w32, _), (w64, _) = results[name]
    assert tuple(dW.shape) == tuple(w64.shape) and bool(torch.isfinite(dW).all())
    hb.check("dW " + name, dW, w32, w64)


@pytest.mark.parametrize("name", list(CASES))
def test_bias_gradient_is_the_column_sum(results, name):
    _, _, _, db, (_, b32), (_, b64) = results[name]
    assert bool(torch.isfinite(db).all())
    hb.check("db " + name, db, b32, b64)


@pytest.mark.parametrize("name", ["strips", "two_levels", "slices_2_34"])
def test_repeat_launches_are_bit_equal(results, name):
    levels, B, _, K = CASES[name]
    xg, dyg, dW, db = results[name][:4]
    dW2, db2 = wgrad.conv3x3_wgrad(xg, dyg, levels, B, K)
    assert torch.equal(dW, dW2) and torch.equal(db, db2)


@pytest.mark.parametrize("shift", [-20, 10])
def test_operand_range_scales_exactly(results, shift):
    """dY times a power of two under a correct record: the f16 terms are the same, so the result is the scaled result to the bit."""
    levels, B, _, K = CASES["strips"]
    xg, dyg, dW, db = results["strips"][:4]
    dW2, db2 = wgrad.conv3x3_wgrad(xg, dyg * 2.0 ** shift, levels, B, K)
    _, _, _, _, (w32, b32), (w64, b64) = results["strips"]
    hb.check("dW range 2^%d" % shift, dW2, w32 * 2.0 ** shift, w64 * 2.0 ** shift)
    hb.check("db range 2^%d" % shift, db2, b32 * 2.0 ** shift, b64 * 2.0 ** shift)
    assert torch.equal(dW2, dW * 2.0 ** shift) and torch.equal(db2, db * 2.0 ** shift)


PLANT = ([(17, 19)], 2, 32, 64)


def _planted_expect(x64, dy64, levels, B, K):
    return hb.ref_wgrad(x64, dy64, levels, B, K, torch.float64)[0]


@pytest.mark.parametrize("corner", ["top_left", "bottom_right"])
def test_planted_output_gradient(corner):
    """dY zero but for one element at an image corner: dW[k] is the shifted 3x3 window of X (zeros outside the image -- never the
    neighbouring image's pixels), a single product each; every other filter's gradient is exactly zero."""
    levels, B, C, K = PLANT
    (h, w), k = levels[0], 37
    x, _ = _inputs(levels, B, C, K, seed=3)
    dy = torch.zeros((B * h * w, K))
    p = 0 if corner == "top_left" else h * w - 1            # image 0: its last pixel is followed by image 1's first row
    dy[p, k] = -0.7321
    dW, _ = wgrad.conv3x3_wgrad(x.to(DEV), dy.to(DEV), levels, B, K)
    ref = _planted_expect(x.double(), dy.double(), levels, B, K)
    dW = dW.cpu().double()
    y0, x0 = (0, 0) if corner == "top_left" else (h - 1, w - 1)
    img = x[:h * w].view(h, w, C).double()
    for ky in range(3):
        for kx in range(3):
            yy, xx = y0 + ky - 1, x0 + kx - 1
            want = img[yy, xx] * float(dy[p, k]) if (0 <= yy < h and 0 <= xx < w) else torch.zeros(C, dtype=torch.float64)
            assert torch.equal(ref[k, :, ky, kx], want)
    assert bool(((dW[k] - ref[k]).abs() <= 2.0 ** -22 * ref[k].abs()).all()), float((dW[k] - ref[k]).abs().max())
    others = torch.ones(K, dtype=torch.bool)
    others[k] = False
    assert bool((dW[others] == 0).all())


def test_planted_input():
    """X zero but for one pixel (the last of image 0): dW[:, c] is the shifted window of dY, a single product each, zero elsewhere."""
    levels, B, C, K = PLANT
    (h, w), c = levels[0], 5
    _, dy = _inputs(levels, B, C, K, seed=4)
    x = torch.zeros((B * h * w, C))
    x[h * w - 1, c] = 1.618
    dW, _ = wgrad.conv3x3_wgrad(x.to(DEV), dy.to(DEV), levels, B, K)
    ref = _planted_expect(x.double(), dy.double(), levels, B, K)
    dW = dW.cpu().double()
    assert bool((ref[:, c, 0, :] == 0).all()) and bool((ref[:, c, :, 0] == 0).all()) and bool((ref[:, c, 1:, 1:] != 0).all())     # no row below, no pixel to the right
    assert bool(((dW[:, c] - ref[:, c]).abs() <= 2.0 ** -22 * ref[:, c].abs()).all()), float((dW[:, c] - ref[:, c]).abs().max())
    others = torch.ones(C, dtype=torch.bool)
    others[c] = False
    assert bool((dW[:, others] == 0).all())


def test_wrong_geometry_and_cpu_tensors_raise():
    from pod_compare_amd import hip
    x, dy = torch.zeros((35, 16)), torch.zeros((35, 64))
    with pytest.raises(hip.PodError):
        wgrad.conv3x3_wgrad(x, dy, [(5, 7)], 1, 64)
    with pytest.raises(hip.PodError):
        wgrad.conv3x3_wgrad(x.to(DEV), dy.to(DEV), [(5, 8)], 1, 64)
    with pytest.raises(hip.PodError):
        wgrad.conv3x3_wgrad(torch.zeros((35, 24), device=DEV), dy.to(DEV), [(5, 7)], 1, 64)


@pytest.mark.parametrize("p", [0.0, 0.1])
def test_gate_equals_autograd_through_relu_dropout(p):
    """dZ = dOut (out > 0) / (1 - p) against fp64 autograd through dropout(relu(z)) on a fixed mask; the record bounds dZ."""
    g = torch.Generator().manual_seed(7)
    z = torch.randn((1000, 64), generator=g, dtype=torch.float64, requires_grad=True)
    keep = (torch.rand((1000, 64), generator=g) >= p).double()
    out = torch.relu(z) * keep / (1.0 - p)
    d_out = torch.randn((1000, 64), generator=g)
    out.backward(d_out.double())
    d_out_g = d_out.to(DEV)
    dz = wgrad.relu_dropout_backward(out.detach().float().to(DEV), d_out_g, p, d_z=torch.empty_like(d_out_g))
    ref32 = d_out * ((out.detach() > 0).float() * (1.0 / (1.0 - p)))
    hb.check("gate p=%.1f" % p, dz, ref32, z.grad)
    assert bool(((dz == 0).cpu() == (out.detach() <= 0)).all())
    assert float(amax.of(dz).max()) == float(dz.abs().max())
    dz2 = wgrad.relu_dropout_backward(out.detach().float().to(DEV), d_out_g, p)             # in place
    assert dz2 is d_out_g and torch.equal(dz2, dz)
