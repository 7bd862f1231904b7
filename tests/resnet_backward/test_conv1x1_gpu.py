"""K24 (csrc/k24_resnet_backward.hip) against plain torch on the CPU: pod_conv1x1_wgrad_strided against an fp64 dy.T @ x[pin] at the
smallest shapes at which it can go wrong -- several slices with a tail, odd sizes in both directions and a channel-tile edge at stride 2,
res5's shortcut and conv3 at 2048 output channels, a single pixel -- against pod_conv1x1_wgrad to the bit where that kernel reaches,
repeat launches, operand range, a planted element; pod_subsample2_scatter_cl on integer-valued maps, to the bit.  Measured figures:
profiles/resnet_backward.md."""
import pytest
import torch

from pod_compare_amd import amax, hip, wgrad
from tests.head_backward import hb
from tests.resnet_backward import rb

pytestmark = pytest.mark.gpu
DEV = "cuda"

#        name              images H_in W_in stride C     K
CASES = {"slices_tail":    (3,    17,  25,  2,     80,   64),      # 3 x 9 x 13 = 351 output pixels: 128-pixel slices, two whole ones + 95; C = 80 leaves 48 of the tile empty
         "res5_shortcut":  (2,    5,   7,   2,     1024, 2048),
         "res5_conv3":     (2,    3,   4,   1,     512,  2048),
         "one_pixel":      (1,    1,   1,   2,     16,   64)}


def _inputs(images, h, w, stride, C, K, seed=0):
    g = torch.Generator().manual_seed(seed)
    ho, wo = rb.out_hw(h, w, stride)
    return torch.randn((images * h * w, C), generator=g), torch.randn((images * ho * wo, K), generator=g)


@pytest.fixture(scope="module")
def results():
    """Every case once: inputs, the GPU result and both CPU references."""
    out = {}
    for name, geo in CASES.items():
        x, dy = _inputs(*geo)
        xg, dyg = x.to(DEV), dy.to(DEV)
        dW, db = wgrad.conv1x1_wgrad_strided(xg, dyg, *geo[:4], bias=True)
        out[name] = (xg, dyg, dW, db, rb.ref_wgrad_strided(x, dy, *geo[:4], torch.float32), rb.ref_wgrad_strided(x, dy, *geo[:4], torch.float64), dy)
    torch.cuda.synchronize()
    return out


def test_the_first_case_spans_several_slices_with_a_tail():
    images, h, w, stride, C, K = CASES["slices_tail"]
    ho, wo = rb.out_hw(h, w, stride)
    pixels = images * ho * wo
    n = hip.load().pod_conv1x1_wgrad_strided_partials(images, h, w, stride, C, K)
    slices = (n - 2 * ((pixels + 4095) // 4096) * K) // (K * C)
    assert pixels == 351 and slices == 3 and pixels % 128 and pixels % 32 and h % 2 and w % 2 and C % 128


@pytest.mark.parametrize("name", list(CASES))
def test_weight_gradient_matches_fp64(results, name):
    _, _, dW, db, w32, w64, dy = results[name]
    assert tuple(dW.shape) == tuple(w64.shape) and bool(torch.isfinite(dW).all())
    hb.check("c1s dW " + name, dW, w32, w64)
    hb.check("c1s db " + name, db, dy.sum(0), dy.double().sum(0))


@pytest.mark.parametrize("name", [n for n, geo in CASES.items() if geo[5] <= 512])
def test_bit_equal_to_the_unstrided_kernel_on_the_gathered_rows(results, name):
    """The output pixel count is the same, so the slices are the same; the gather only changes where a row is read from."""
    xg, dyg, dW, db = results[name][:4]
    sub = rb.gather_rows(xg, *CASES[name][:4])
    dW1, db1 = wgrad.conv1x1_wgrad(amax.attach(sub, amax.of(xg)), dyg)          # (the scale is the whole map's, as in the strided launch)
    assert torch.equal(dW, dW1) and torch.equal(db, db1)


@pytest.mark.parametrize("name", list(CASES))
def test_repeat_launches_are_bit_equal(results, name):
    xg, dyg, dW, db = results[name][:4]
    dW2, db2 = wgrad.conv1x1_wgrad_strided(xg, dyg, *CASES[name][:4], bias=True)
    assert torch.equal(dW, dW2) and torch.equal(db, db2)
    dW3, none = wgrad.conv1x1_wgrad_strided(xg, dyg, *CASES[name][:4])
    assert none is None and torch.equal(dW, dW3)


@pytest.mark.parametrize("name", list(CASES))
def test_operand_range_scales_exactly(results, name):
    """An operand times a power of two under a correct record: the f16 terms are the same, so the result is the scaled result to the bit."""
    xg, dyg, dW = results[name][:3]
    geo = CASES[name][:4]
    assert torch.equal(wgrad.conv1x1_wgrad_strided(xg * 2.0 ** 12, dyg, *geo)[0], dW * 2.0 ** 12)
    assert torch.equal(wgrad.conv1x1_wgrad_strided(xg, dyg * 2.0 ** -12, *geo)[0], dW * 2.0 ** -12)


def test_planted_output_gradient_picks_the_row_the_stride_selects():
    """dY zero but for its last element, at stride 2: dW's last row is row pin(last) of X -- the last image's pixel (2 (Ho - 1), 2 (Wo - 1)) --
    times it, a single product each within the formats' bound (tests/fpn_backward/test_conv1x1_gpu.py derives 2.5 * 2^-22), and every
    other row is exactly zero."""
    images, h, w, stride, C, K = CASES["slices_tail"]
    ho, wo = rb.out_hw(h, w, stride)
    pin = (images - 1) * h * w + stride * (ho - 1) * w + stride * (wo - 1)
    assert pin == images * h * w - 1                       # both sizes odd: the last output pixel reads the very last input pixel ...
    x, _ = _inputs(images, h, w, stride, C, K, seed=3)
    dy = torch.zeros((images * ho * wo, K))
    dy[-1, -1] = -0.7321
    dW, _ = wgrad.conv1x1_wgrad_strided(x.to(DEV), dy.to(DEV), images, h, w, stride)
    dW, want = dW.cpu().double(), x[pin].double() * float(dy[-1, -1])
    assert bool(((dW[-1] - want).abs() <= 2.5 * 2.0 ** -22 * want.abs()).all()), float((dW[-1] - want).abs().max())
    assert bool((dW[:-1] == 0).all())
    # ... so once more at even sizes, where the last output pixel (2, 3) reads input pixel (4, 6): neither the last row of X nor row `last`
    images, h, w = 2, 6, 8
    ho, wo = rb.out_hw(h, w, 2)
    pin = (images - 1) * h * w + 2 * (ho - 1) * w + 2 * (wo - 1)
    assert pin == images * h * w - 1 - w - 1 and pin != images * ho * wo - 1
    x = torch.randn((images * h * w, C), generator=torch.Generator().manual_seed(4))
    dy = torch.zeros((images * ho * wo, K))
    dy[-1, -1] = 0.5
    dW, _ = wgrad.conv1x1_wgrad_strided(x.to(DEV), dy.to(DEV), images, h, w, 2)
    dW, want = dW.cpu().double(), x[pin].double() * 0.5
    assert bool(((dW[-1] - want).abs() <= 2.5 * 2.0 ** -22 * want.abs()).all()), float((dW[-1] - want).abs().max())
    assert bool((dW[:-1] == 0).all())


def _ints(shape, g, lo=-8, hi=9):
    return torch.randint(lo, hi, shape, generator=g).float()


@pytest.mark.parametrize("h,w,C", [(5, 6, 16), (4, 7, 64)])
@pytest.mark.parametrize("with_gate", [False, True], ids=["plain", "gate"])
@pytest.mark.parametrize("with_add", [False, True], ids=["noadd", "add"])
def test_scatter_equals_the_fp64_reference_to_the_bit(h, w, C, with_gate, with_add):
    g = torch.Generator().manual_seed(h * 100 + w)
    ho, wo = rb.out_hw(h, w, 2)
    d_small = _ints((ho * wo, C), g)
    gate = _ints((h * w, C), g, -2, 3) if with_gate else None           # zeros among them: the gate is > 0, not >= 0
    add = _ints((h * w, C), g) if with_add else None
    assert gate is None or bool((gate == 0).any())
    want = rb.ref_scatter(d_small, h, w, gate, add)
    dev = lambda t: None if t is None else t.to(DEV)
    dx = wgrad.subsample2_scatter_cl(dev(d_small), h, w, gate=dev(gate), add=dev(add))
    assert torch.equal(dx.cpu().double(), want)
    assert float(amax.of(dx).max()) == float(dx.abs().max())
    if with_add:                                                          # in place on the gradient the map already has
        buf = dev(add)
        assert wgrad.subsample2_scatter_cl(dev(d_small), h, w, gate=dev(gate), add=buf, out=buf) is buf and torch.equal(buf, dx)


def test_bad_geometry_aliases_and_cpu_tensors_raise():
    """Every refusal comes before a launch: the library's entries are not reached, or return POD_E_INVALID from their argument checks."""
    z = lambda *shape: torch.zeros(shape, device=DEV)
    one = z(1, 16)
    bad = [lambda: wgrad.conv1x1_wgrad_strided(torch.zeros((70, 16)), torch.zeros((24, 64)), 2, 5, 7, 2),     # CPU tensors
           lambda: wgrad.conv1x1_wgrad_strided(z(70, 16), z(70, 64), 2, 5, 7, 2),                              # dy has 2 x 3 x 4 rows at stride 2
           lambda: wgrad.conv1x1_wgrad_strided(z(70, 16), z(24, 64), 2, 5, 7, 1),
           lambda: wgrad.conv1x1_wgrad_strided(z(70, 16), z(12, 64), 2, 5, 7, 3),                              # stride 3
           lambda: wgrad.conv1x1_wgrad_strided(z(70, 24), z(24, 64), 2, 5, 7, 2),                              # C % 16
           lambda: wgrad.conv1x1_wgrad_strided(z(70, 16), z(24, 96), 2, 5, 7, 2),                              # K % 64
           lambda: wgrad.conv1x1_wgrad_strided(z(70, 16), z(24, 2112), 2, 5, 7, 2),                            # K > 2048
           lambda: wgrad.conv1x1_wgrad_strided(z(0, 16), z(0, 64), 0, 5, 7, 2),                                # no image
           lambda: wgrad.subsample2_scatter_cl(torch.zeros((12, 16)), 5, 7),                                   # CPU
           lambda: wgrad.subsample2_scatter_cl(z(12, 16), 5, 9),                                               # 5 x 9 selects 15 rows
           lambda: wgrad.subsample2_scatter_cl(z(12, 6), 5, 7),                                                # C % 4
           lambda: wgrad.subsample2_scatter_cl(z(12, 16), 5, 7, gate=z(35, 32)),
           lambda: wgrad.subsample2_scatter_cl(z(12, 16), 5, 7, add=z(34, 16)),
           lambda: wgrad.subsample2_scatter_cl(one, 1, 1, out=one),                                            # in place on d_small (1 x 1: the shapes agree)
           lambda: (lambda buf: wgrad.subsample2_scatter_cl(z(12, 16), 5, 7, gate=buf, out=buf))(z(35, 16))]   # the gate is dx
    for f in bad:
        with pytest.raises(hip.PodError):
            f()
