"""The operand abs-max RECORDS of the split convolutions (include/pod_mi355x.h: "operand abs-max records"): 16 slots, 32 floats apart, whose
largest slot must be >= max |x| of what the consuming launch reads.  A record that is low by less than a factor of 2 shows nothing on
ordinary data, so every stage is held to it directly:

  1. pod_absmax against x.abs().max() (a maximum has no rounding: equality);
  2. every producer's record == max |what it stored|, bit for bit: pod_conv1x1_split (all four kernel forms + the split's reduce),
     pod_reduce_partials, pod_stem7x7_split, pod_wino_reduce -- on random data, with the maximum planted at one chosen element, and with
     a value that only a pixel OUTSIDE the image would take;
  3. every consumer reads all 16 slots;
  4. a record a factor of 4 low gives non-finite outputs at the offending pixel and leaves every other pixel inside its usual bound;
  5. pod_compare_amd/amax.py's carriers on the device (of / attach / forget / produced / joined, the pool, the carry-overs of
     conv1x1.py, the stem's analytic bound);
  6. every record a real forward consumes bounds the tensor it is consumed with.

The module shares its name with tests/test_conv1x1_gpu.py so that the GPU run order in tests/conftest.py (GPU_ORDER, keyed by module
name) gives it a place beside the 1x1 convolution's own tests."""
import sys

import pytest
import torch
import torch.nn.functional as F

from pod_compare_amd import amax, hip
from pod_compare_amd.conv1x1 import Conv1x1, Conv3x3S2, Stem7x7, maxpool3x3s2_cl

pytestmark = pytest.mark.gpu
SLOTS, STRIDE, RECORD = 16, 32, 512        # include/pod_mi355x.h: POD_AMAX_SLOTS, POD_AMAX_STRIDE, POD_AMAX_FLOATS
SENTINEL = -7.0                            # what the 496 floats between the slots hold where a test watches them
EPS = 2.0 ** -24


# ---- helpers -------------------------------------------------------------------------------------------------------------------------
def gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def zeros_record():
    return torch.zeros(RECORD, device="cuda")


def slots(rec):
    assert rec.numel() == RECORD
    return rec.view(SLOTS, STRIDE)[:, 0]


def rec_max(rec):
    return float(slots(rec).max())


def absmax(t):
    return float(t.abs().max())


def published(t):
    """max of the record the launch that wrote t published: still attached under t's version, and nothing but its 16 slots written."""
    rec, version = t._pod_amax
    assert version == t._version
    assert bool((rec.view(SLOTS, STRIDE)[:, 1:] == 0).all())
    return rec_max(rec)


def full_record(v):
    return torch.full((RECORD,), float(v), device="cuda")


def one_slot_record(v, k):
    rec = zeros_record()
    rec[k * STRIDE] = float(v)
    return rec


def pod_absmax(x, rec, n=None):
    hip.check(hip.load().pod_absmax(x.data_ptr(), x.numel() if n is None else n, rec.data_ptr(), hip.current_stream()), "pod_absmax")
    return rec


# ---- 1. pod_absmax ----------------------------------------------------------------------------------------------------------------------
ABSMAX_N = [1, 2, 3, 4, 5, 7, 1023, 1024, 1025, 4 * 256 * 1024 + 5]       # the last: one float4 pass of the 1024-block grid, one more quad, a scalar tail


@pytest.mark.parametrize("n", ABSMAX_N)
def test_absmax_is_the_abs_max_wherever_it_sits(n):
    base = torch.rand(n, device="cuda", generator=gen(n)) * 2.0 - 1.0
    assert rec_max(pod_absmax(base, zeros_record())) == absmax(base)
    for at in sorted({0, n - 1, max(n - 2, 0), n // 2}):
        x = base.clone()
        x[at] = -3.5
        rec = pod_absmax(x, zeros_record())
        assert rec_max(rec) == 3.5 == absmax(x), at
        assert bool((rec.view(SLOTS, STRIDE)[:, 1:] == 0).all())


def test_absmax_of_zeros_leaves_a_zeroed_record_zero():
    for n in (5, 4096):
        rec = pod_absmax(torch.zeros(n, device="cuda"), zeros_record())
        assert bool((rec == 0).all())


@pytest.mark.parametrize("n", [7, 4 * 256 * 64 + 3])
def test_absmax_maxes_into_the_16_slots_and_writes_nothing_else(n):
    x = torch.rand(n, device="cuda", generator=gen(n)) - 0.5
    x[n // 3] = -3.5
    for before in (10.0, 1.0, 0.0):                                # larger than max |x|: kept; smaller: the overall max is still right
        rec = torch.full((RECORD,), SENTINEL, device="cuda")
        slots(rec).fill_(before)
        pod_absmax(x, rec)
        assert bool((rec.view(SLOTS, STRIDE)[:, 1:] == SENTINEL).all())
        assert bool((slots(rec) >= before).all())
        assert bool(((slots(rec) == before) | (slots(rec) <= 3.5)).all())
        assert rec_max(rec) == max(before, 3.5)


def test_absmax_of_records_joins_two_bounds():
    a, b = zeros_record(), zeros_record()
    slots(a).copy_(torch.rand(SLOTS, device="cuda", generator=gen(1)))
    slots(b).copy_(torch.rand(SLOTS, device="cuda", generator=gen(2)))
    a[11 * STRIDE], b[3 * STRIDE] = 5.0, 9.0
    w = zeros_record()
    pod_absmax(a, w)
    assert rec_max(w) == 5.0
    pod_absmax(b, w)
    assert rec_max(w) == 9.0
    pod_absmax(a, w)
    assert rec_max(w) == 9.0


@pytest.mark.parametrize("n", [6, 1025])
def test_absmax_ignores_nan_and_takes_inf_as_written(n):
    """include/pod_mi355x.h, operand abs-max records: a NaN never enters a record (fmaxf drops it); an inf does, as written."""
    x = torch.rand(n, device="cuda", generator=gen(n)) + 0.5
    x[n // 2] = -2.5
    for at in (0, n - 1, n // 3):
        x[at] = float("nan")
    finite = x[~torch.isnan(x)]
    assert rec_max(pod_absmax(x, zeros_record())) == absmax(finite) == 2.5
    assert bool((pod_absmax(torch.full((n,), float("nan"), device="cuda"), zeros_record()) == 0).all())
    for at, v in ((n - 1, float("inf")), (1, float("-inf"))):
        y = x.clone()
        y[at] = v
        assert rec_max(pod_absmax(y, zeros_record())) == float("inf")


def test_an_inf_input_takes_the_smallest_scale():
    """What the header promises of an inf in the consumed tensor: its record is inf, the launch scales by the smallest power of two, the
    products of the inf are inf / nan as they would be in fp32 -- and the tensor's finite values fall below f16's smallest number: every
    other pixel stores bias exactly."""
    cin, cout, h, w = 32, 64, 3, 5
    g = gen(3)
    wt = torch.randn(cout, cin, 1, 1, device="cuda", generator=g) * 0.2
    b = torch.randn(cout, device="cuda", generator=g)
    x = torch.randn(h * w, cin, device="cuda", generator=g)
    x[4, 7] = float("inf")
    y = Conv1x1(wt, b, 1)(x, h, w, n_splits=1, waves=1)
    assert rec_max(amax.of(x)) == float("inf")
    assert not bool(torch.isfinite(y[4]).any())
    rest = torch.cat([y[:4], y[5:]])
    assert torch.equal(rest, b.expand_as(rest))


# ---- 2. producers -----------------------------------------------------------------------------------------------------------------------
# (Cin, n_splits, waves): the four kernel forms of pod_conv1x1_split and the cut over workgroup sets, whose record is the reduce launch's
C1_FORMS = [pytest.param(48, 1, 1, id="direct-3-ksteps"), pytest.param(32, 1, 1, id="lds-1-wave"), pytest.param(128, 1, 2, id="lds-2-waves"),
            pytest.param(128, 1, 4, id="lds-4-waves"), pytest.param(64, 2, 1, id="2-splits+reduce")]
C1_MAPS = [(1, 1, 1), (5, 13, 1), (9, 9, 2)]          # (H_in, W_in, stride): 1 pixel; 65 = a full 64-pixel tile + 1; 9 x 9 at stride 2 = 5 x 5


def upsampled(top, ho, wo):
    hr, wr = (ho + 1) // 2, (wo + 1) // 2
    return top.view(hr, wr, -1).repeat_interleave(2, 0).repeat_interleave(2, 1)[:ho, :wo].reshape(ho * wo, -1).contiguous()


def c1_reference(x, wt, b, h, w, stride, residual):
    """fp64 pre-activation (P_out, Cout) and its per-element magnitude bound"""
    cin = x.shape[1]
    xs = x.view(h, w, cin)[::stride, ::stride].reshape(-1, cin).double()
    w2 = wt.view(wt.shape[0], cin).double()
    pre, bound = xs @ w2.t() + b.double(), xs.abs() @ w2.abs().t() + b.double().abs()
    if residual is not None:
        pre, bound = pre + residual.double(), bound + residual.double().abs()
    return pre, bound


def c1_run(conv, x, wt, b, h, w, relu, residual, up2, splits, waves):
    """conv(...) -> (y, fp64 pre-activation); y is held to the module's bound against fp64 (c <= 8, tests/test_conv1x1_gpu.py) so that
    'the record equals what was stored' is said of a correct output"""
    ho, wo = conv.out_hw(h, w)
    y = conv(x, h, w, relu=relu, residual=residual, residual_up2=up2, n_splits=splits, waves=waves)
    full = None if residual is None else (upsampled(residual, ho, wo) if up2 else residual)
    pre, bound = c1_reference(x, wt, b, h, w, conv.stride, full)
    want = pre.relu() if relu else pre
    assert bool(((y.double() - want).abs() <= 8.0 * EPS * bound).all())
    return y, pre


@pytest.mark.parametrize("residual", ["none", "full", "up2"])
@pytest.mark.parametrize("cin,splits,waves", C1_FORMS)
def test_conv1x1_record_is_the_max_of_what_it_stored(cin, splits, waves, residual):
    for cout in (64, 128):
        for h, w, stride in C1_MAPS:
            g = gen(cin + cout + h)
            wt = torch.randn(cout, cin, 1, 1, device="cuda", generator=g) * (2.0 / cin) ** 0.5
            b = torch.randn(cout, device="cuda", generator=g)
            x = torch.randn(h * w, cin, device="cuda", generator=g)
            conv = Conv1x1(wt, b, stride)
            ho, wo = conv.out_hw(h, w)
            rows = {"none": 0, "full": ho * wo, "up2": ((ho + 1) // 2) * ((wo + 1) // 2)}[residual]
            res = torch.randn(rows, cout, device="cuda", generator=g) * 2.0 if rows else None
            for relu in (False, True):
                y, _ = c1_run(conv, x, wt, b, h, w, relu, res, residual == "up2", splits, waves)
                assert published(y) == absmax(y), (cout, h, w, stride, relu)


def test_the_first_launch_of_a_split_publishes_nothing():
    """n_splits = 2: the record the pair of launches leaves is the one pod_reduce_partials alone writes from the same partial sums into a
    record of its own -- slot for slot -- although the partial sums hold a value four times anything stored (a large negative
    pre-activation behind the ReLU)."""
    cin, cout, h, w = 64, 128, 5, 13
    g = gen(17)
    wt = torch.randn(cout, cin, 1, 1, device="cuda", generator=g) * (2.0 / cin) ** 0.5
    wt[3] = -wt[3].abs() * 8.0
    b = torch.randn(cout, device="cuda", generator=g)
    x = torch.rand(h * w, cin, device="cuda", generator=g) * 0.75 + 0.25
    x[7] *= 64.0
    res = torch.randn(h * w, cout, device="cuda", generator=g)
    conv = Conv1x1(wt, b, 1)
    lib, s, n = hip.load(), hip.current_stream(), h * w * cout
    partials = torch.empty(2, h * w, cout, device="cuda")
    y, y2 = torch.empty(h * w, cout, device="cuda"), torch.empty(h * w, cout, device="cuda")
    rec, rec2 = zeros_record(), zeros_record()
    hip.check(lib.pod_conv1x1_split(x.data_ptr(), y.data_ptr(), conv.Ws.data_ptr(), conv.bias.data_ptr(), res.data_ptr(), h, w, h, w, 1, cin, cout, 1, 2,
                                    partials.data_ptr(), 1, amax.of(x).data_ptr(), rec.data_ptr(), s), "pod_conv1x1_split")
    hip.check(lib.pod_reduce_partials(partials.data_ptr(), 2, n, conv.bias.data_ptr(), res.data_ptr(), y2.data_ptr(), n, cout, 1, rec2.data_ptr(), s),
              "pod_reduce_partials")
    assert torch.equal(y, y2)
    assert absmax(partials) >= 2.0 * absmax(y)                    # (what a publishing first pass would leave in the record)
    assert torch.equal(rec, rec2)
    assert rec_max(rec) == absmax(y)


def plant_pixels(p_out):
    """first pixel, last valid pixel, and the two pixels astride the 64-pixel tile boundary"""
    return sorted({0, p_out - 1} | ({63, 64} if p_out > 64 else set()))


@pytest.mark.parametrize("mode", ["positive-relu", "negative-no-relu", "negative-behind-relu", "residual-alone", "negative-residual-alone"])
@pytest.mark.parametrize("cin,splits,waves", C1_FORMS)
def test_conv1x1_record_with_the_maximum_planted_at_one_element(cin, splits, waves, mode):
    """The stored tensor's abs-max sits, by construction (one pixel's input x 64 and one filter row x 8 of one sign on inputs > 0, or one
    residual element), at ONE element at least twice anything else -- checked on the fp64 reference first.  The record must be that
    element's magnitude; behind a ReLU a large negative pre-activation must not appear in it."""
    cout = 128
    relu = mode in ("positive-relu", "negative-behind-relu")
    sign = 1.0 if mode in ("positive-relu", "residual-alone") else -1.0
    for h, w, stride in ((5, 13, 1), (9, 9, 2)):
        ho, wo = (h - 1) // stride + 1, (w - 1) // stride + 1
        for p in plant_pixels(ho * wo):
            k = 0 if p in (0, 64) else cout - 1
            g = gen(cin + p)
            wt = torch.randn(cout, cin, 1, 1, device="cuda", generator=g) * (2.0 / cin) ** 0.5
            b = torch.randn(cout, device="cuda", generator=g) * 0.1
            x = torch.rand(h * w, cin, device="cuda", generator=g) * 0.75 + 0.25
            res = None
            if "residual" in mode:
                res = torch.zeros(ho * wo, cout, device="cuda")
                res[p, k] = sign * 1000.0
            else:
                wt[k] = sign * wt[k].abs() * 8.0
                x[(p // wo) * stride * w + (p % wo) * stride] *= 64.0
            y, pre = c1_run(Conv1x1(wt, b, stride), x, wt, b, h, w, relu, res, False, splits, waves)
            others = (pre.relu() if relu else pre).abs().clone()
            others[p, k] = 0.0
            if mode == "negative-behind-relu":
                assert float(pre[p, k]) <= -2.0 * float(others.max()) and float(y[p, k]) == 0.0
                assert published(y) == absmax(y) < -0.5 * float(pre[p, k])
                continue
            assert sign * float(pre[p, k]) >= 2.0 * float(others.max())
            assert int(y.abs().argmax()) == p * cout + k
            assert published(y) == sign * float(y[p, k]) == absmax(y), (h, w, p, k)


@pytest.mark.parametrize("residual", ["none", "full", "up2"])
@pytest.mark.parametrize("cin,splits,waves", C1_FORMS)
def test_conv1x1_record_takes_no_pixel_outside_the_image(cin, splits, waves, residual):
    """Inputs >= 1, weights <= 0, ONE large positive bias B: every stored value is below B, a pixel of zeros would evaluate to exactly B.
    The lanes of a ragged tile that stand outside the image re-read pixel 0 WITHOUT its residual: with a residual of -B / 2 everywhere
    such a lane holds B - s against a stored maximum of B / 2.  The record is the stored maximum."""
    cout, B = 128, 1024.0
    for h, w, stride in C1_MAPS:
        g = gen(cin + h)
        wt = -torch.rand(cout, cin, 1, 1, device="cuda", generator=g) * 0.01
        b = torch.zeros(cout, device="cuda")
        b[70] = B
        x = torch.rand(h * w, cin, device="cuda", generator=g) + 1.0
        conv = Conv1x1(wt, b, stride)
        ho, wo = conv.out_hw(h, w)
        rows = {"none": 0, "full": ho * wo, "up2": ((ho + 1) // 2) * ((wo + 1) // 2)}[residual]
        res = torch.full((rows, cout), -B / 2, device="cuda") if rows else None
        for relu in (False, True):
            y, _ = c1_run(conv, x, wt, b, h, w, relu, res, residual == "up2", splits, waves)
            assert published(y) == absmax(y), (h, w, relu)
            if residual == "none":
                assert published(y) == float(y.max()) < B
            else:
                assert published(y) < 0.75 * B


@pytest.mark.parametrize("pixels,cout", [(37, 20), (300, 20), (65, 64)])
def test_reduce_partials_alone(pixels, cout):
    """3 splits, n no multiple of 256 x 4 (37 x 20 = 740: a partial workgroup; 300 x 20: several): y is the fixed-order fp32 sum, to the bit,
    and the record its abs-max."""
    n, stride = pixels * cout, pixels * cout + 8
    g = gen(pixels)
    buf = torch.randn(3 * stride, device="cuda", generator=g)
    parts = [buf[i * stride:i * stride + n].view(pixels, cout) for i in range(3)]
    b = torch.randn(cout, device="cuda", generator=g)
    res = torch.randn(pixels, cout, device="cuda", generator=g)
    for relu in (0, 1):
        for use_b, use_r in ((True, True), (False, False), (True, False)):
            y, rec = torch.empty(pixels, cout, device="cuda"), zeros_record()
            hip.check(hip.load().pod_reduce_partials(buf.data_ptr(), 3, stride, b.data_ptr() if use_b else None, res.data_ptr() if use_r else None, y.data_ptr(), n,
                                                     cout, relu, rec.data_ptr(), hip.current_stream()), "pod_reduce_partials")
            want = (parts[0] + parts[1]) + parts[2]
            want = want + b if use_b else want
            want = want + res if use_r else want
            want = want.relu() if relu else want
            assert torch.equal(y, want)
            assert rec_max(rec) == absmax(y)
    # a maximum in the last quad of the last (partial) workgroup's range, negative, without ReLU
    buf[stride + n - 1] = -500.0
    y, rec = torch.empty(pixels, cout, device="cuda"), zeros_record()
    hip.check(hip.load().pod_reduce_partials(buf.data_ptr(), 3, stride, None, None, y.data_ptr(), n, cout, 0, rec.data_ptr(), hip.current_stream()), "pod_reduce_partials")
    assert int(y.abs().argmax()) == n - 1 and rec_max(rec) == absmax(y) > 400.0


STEM_FRAMES = [(1, 1), (17, 33), (15, 15)]            # Ho x Wo = 1 x 1, 9 x 17, 8 x 8: tiles of 8 x 8 pixels


def stem_reference(x, wt, b, padded=None):
    x = x.double().view(1, 3, x.shape[-2], x.shape[-1])
    if padded is not None:
        x = F.pad(x, (0, padded[1] - x.shape[-1], 0, padded[0] - x.shape[-2]))
    pre = F.conv2d(x, wt.double(), b.double(), stride=2, padding=3)
    bound = F.conv2d(x.abs(), wt.double().abs(), b.double().abs(), stride=2, padding=3)
    return pre[0].permute(1, 2, 0).reshape(-1, 64), bound[0].permute(1, 2, 0).reshape(-1, 64)


def stem_weights(seed):
    g = gen(seed)
    return torch.randn(64, 3, 7, 7, device="cuda", generator=g) * (2.0 / 147) ** 0.5, torch.randn(64, device="cuda", generator=g), g


@pytest.mark.parametrize("h,w", STEM_FRAMES)
@pytest.mark.parametrize("kind", ["uint8-normalised-padded", "float"])
def test_stem_record_is_the_max_of_what_it_stored(h, w, kind):
    from pod_compare_amd import anchors as A
    wt, b, g = stem_weights(h + w)
    stem = Stem7x7(wt, b)
    mean, std = torch.tensor([103.53, 116.28, 123.675], device="cuda"), torch.tensor([1.0, 57.375, 58.395], device="cuda")
    for relu in (False, True):
        if kind == "float":
            x = torch.randn(1, 3, h, w, device="cuda", generator=g) * 1.5
            y, ho, wo = stem(x, relu=relu)
            pre, bound = stem_reference(x, wt, b)
        else:
            frame = torch.randint(0, 256, (3, h, w), dtype=torch.uint8, device="cuda", generator=g)
            padded = A.padded_size(h, w)
            y, ho, wo = stem(frame, relu=relu, mean=mean, std=std, padded_hw=padded)
            pre, bound = stem_reference((frame.float() - mean.view(3, 1, 1)) / std.view(3, 1, 1), wt, b, padded)
        assert tuple(y.shape) == tuple(pre.shape) == (ho * wo, 64)
        assert bool(((y.double() - (pre.relu() if relu else pre)).abs() <= 8.0 * EPS * bound).all())
        assert published(y) == absmax(y), relu


@pytest.mark.parametrize("mode", ["positive-relu", "negative-no-relu", "negative-behind-relu"])
def test_stem_record_with_the_maximum_planted_at_one_element(mode):
    """One input pixel (2 oy, 2 ox) x 64 under a centre tap x 8 of one sign, inputs > 0: output (oy, ox) of that channel is at least twice
    anything else (checked on the fp64 reference).  First pixel, last valid pixel, and the pixels either side of the 8 x 8 tiles' corner."""
    relu = mode != "negative-no-relu"
    sign = 1.0 if mode == "positive-relu" else -1.0
    for h, w in STEM_FRAMES:
        ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
        for oy, ox in sorted({(0, 0), (ho - 1, wo - 1), (min(7, ho - 1), min(7, wo - 1)), (min(8, ho - 1), min(8, wo - 1))}):
            k = 0 if (oy, ox) == (0, 0) else 63
            wt, b, g = stem_weights(oy * 31 + ox)
            b = b * 0.1
            wt[k, :, 3, 3] = sign * wt[k, :, 3, 3].abs() * 8.0
            x = torch.rand(1, 3, h, w, device="cuda", generator=g) * 0.75 + 0.25
            x[0, :, 2 * oy, 2 * ox] *= 64.0
            y, _, _ = Stem7x7(wt, b)(x, relu=relu)
            pre, bound = stem_reference(x, wt, b)
            p = oy * wo + ox
            assert bool(((y.double() - (pre.relu() if relu else pre)).abs() <= 8.0 * EPS * bound).all())
            others = (pre.relu() if relu else pre).abs().clone()
            others[p, k] = 0.0
            if mode == "negative-behind-relu":
                assert float(pre[p, k]) <= -2.0 * float(others.max()) and float(y[p, k]) == 0.0
                assert published(y) == absmax(y) < -0.5 * float(pre[p, k])
                continue
            assert sign * float(pre[p, k]) >= 2.0 * float(others.max())
            assert int(y.abs().argmax()) == p * 64 + k
            assert published(y) == sign * float(y[p, k]) == absmax(y), (h, w, oy, ox)


@pytest.mark.parametrize("h,w", STEM_FRAMES)
def test_stem_record_takes_no_pixel_outside_the_image(h, w):
    """Inputs >= 1, weights < 0, ONE large positive bias B: every output pixel's window holds its own centre pixel, so every stored value
    is below B -- and the tile's pixels beyond Ho x Wo, whose windows hold zeros only, evaluate to exactly B."""
    B = 1024.0
    g = gen(h)
    wt = -torch.rand(64, 3, 7, 7, device="cuda", generator=g) * 0.01 - 1e-4
    b = torch.zeros(64, device="cuda")
    b[37] = B
    x = torch.rand(1, 3, h, w, device="cuda", generator=g) + 1.0
    for relu in (False, True):
        y, _, _ = Stem7x7(wt, b)(x, relu=relu)
        assert published(y) == absmax(y) == float(y.max()) < B


@pytest.mark.parametrize("hw", [65, 66, 68])
def test_wino_reduce_record(hw):
    """K = 36 real channels of Kpad = 64, 2 splits: the planes are the fixed-order sum + bias (+ ReLU) to the bit, the record their abs-max.
    HW = 65, 66: scalar plane stores (HW % 4 != 0) over a full tile plus a ragged one; HW = 68: the 16-byte stores.  As the split launch
    leaves them, the partial sums' channels past K and the bias there are zero."""
    K, Kpad = 36, 64
    g = gen(hw)
    parts = torch.randn(2, hw, Kpad, device="cuda", generator=g)
    parts[:, :, K:] = 0.0
    b = torch.zeros(Kpad, device="cuda")
    b[:K] = torch.randn(K, device="cuda", generator=g)
    for relu in (0, 1):
        for planted in (False, True):
            if planted:                                            # the last pixel of the ragged tile, the last real channel, negative
                parts[1, hw - 1, K - 1] = -300.0
            planes, rec = torch.full((K, hw), float("nan"), device="cuda"), zeros_record()
            hip.check(hip.load().pod_wino_reduce(parts.data_ptr(), 2, hw * Kpad, b.data_ptr(), planes.data_ptr(), hw, Kpad, K, relu, rec.data_ptr(),
                                                 hip.current_stream()), "pod_wino_reduce")
            want = (parts[0] + parts[1]) + b
            want = (want.relu() if relu else want)[:, :K].t()
            assert torch.equal(planes, want)
            assert rec_max(rec) == absmax(planes)
            if planted and not relu:
                assert rec_max(rec) > 250.0 and int(planes.abs().argmax()) == (K - 1) * hw + hw - 1


# ---- 3. readers use all 16 slots ------------------------------------------------------------------------------------------------------
def every_slot_alone(launch, bound):
    """launch(record) -> output: with the bound in ONE slot, whichever, bit for bit the output under a record that holds it everywhere"""
    want = launch(full_record(bound))
    assert bool(torch.isfinite(want).all())
    for k in range(SLOTS):
        assert torch.equal(launch(one_slot_record(bound, k)), want), k


@pytest.mark.parametrize("cin,waves", [pytest.param(48, 1, id="direct-3-ksteps"), pytest.param(32, 1, id="lds-1-wave"), pytest.param(128, 2, id="lds-2-waves"),
                                       pytest.param(128, 4, id="lds-4-waves")])
def test_conv1x1_reads_every_slot_of_its_input_record(cin, waves):
    cout, h, w = 64, 5, 13
    g = gen(cin)
    wt = torch.randn(cout, cin, 1, 1, device="cuda", generator=g) * (2.0 / cin) ** 0.5
    x = torch.randn(h * w, cin, device="cuda", generator=g) * 3.0
    conv = Conv1x1(wt, torch.randn(cout, device="cuda", generator=g), 1)

    def launch(rec):
        y = torch.full((h * w, cout), float("nan"), device="cuda")
        hip.check(hip.load().pod_conv1x1_split(x.data_ptr(), y.data_ptr(), conv.Ws.data_ptr(), conv.bias.data_ptr(), None, h, w, h, w, 1, cin, cout, 0, 1, None, waves,
                                               rec.data_ptr(), None, hip.current_stream()), "pod_conv1x1_split")
        return y
    every_slot_alone(launch, absmax(x))


def test_stem_reads_every_slot_of_its_input_record():
    h, w = 17, 33
    wt, b, g = stem_weights(5)
    x = torch.randn(1, 3, h, w, device="cuda", generator=g) * 3.0
    stem = Stem7x7(wt, b)

    def launch(rec):
        y = torch.full((9 * 17, 64), float("nan"), device="cuda")
        hip.check(hip.load().pod_stem7x7_split(x.data_ptr(), 0, h, w, None, None, y.data_ptr(), stem.Ws.data_ptr(), stem.bias.data_ptr(), h, w, 1, rec.data_ptr(), None,
                                               hip.current_stream()), "pod_stem7x7_split")
        return y
    every_slot_alone(launch, absmax(x))


def test_wino_split_reads_every_slot_of_its_input_record():
    from pod_compare_amd.wino import WinoConv, block_table
    from tests.test_wino_conv_gpu import _conv_desc, _launch_rc
    C, K, h, w = 32, 64, 6, 11
    g = gen(9)
    conv = WinoConv(torch.randn(K, C, 3, 3, device="cuda", generator=g) * (2.0 / (9 * C)) ** 0.5, torch.randn(K, device="cuda", generator=g), split=True)
    src = torch.randn(h * w, C, device="cuda", generator=g) * 3.0
    table = block_table([(h, w)], 1, "cuda")

    def launch(rec):
        dst = torch.full((h * w, K), float("nan"), device="cuda")
        d = _conv_desc(conv, src, dst, table)
        d.sets[0].in_amax = rec.data_ptr()
        assert _launch_rc(d) == 0
        return dst
    every_slot_alone(launch, absmax(src))


# ---- 4. the under-bound promise --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cin,waves", [pytest.param(48, 1, id="direct-3-ksteps"), pytest.param(32, 1, id="lds-1-wave")])
def test_a_record_four_times_too_low_overflows_only_the_offending_pixel(cin, waves):
    """One pixel's input is 64 x everything else and the record holds max |x| / 4.  The scale s puts the RECORD into [2^14, 2^15), so
    max |x| s >= 4 * 2^14 = 2^16 > 65504, f16's largest number: that element's first term is inf and with it every output channel of its
    pixel is non-finite (the header: 'inf / nan, never silently wrong').  Every other pixel's values are scaled below 2^11 and still meet
    the module's bound against fp64 (c <= 8, tests/test_conv1x1_gpu.py)."""
    cout, h, w, p = 64, 5, 13, 31
    g = gen(cin + 4)
    wt = torch.randn(cout, cin, 1, 1, device="cuda", generator=g) * (2.0 / cin) ** 0.5
    b = torch.randn(cout, device="cuda", generator=g)
    x = (torch.rand(h * w, cin, device="cuda", generator=g) * 0.5 + 0.5) * torch.where(torch.rand(h * w, cin, device="cuda", generator=g) < 0.5, -1.0, 1.0)
    x[p] *= 64.0
    conv = Conv1x1(wt, b, 1)
    rec = full_record(absmax(x) / 4.0)
    y = torch.full((h * w, cout), float("nan"), device="cuda")
    hip.check(hip.load().pod_conv1x1_split(x.data_ptr(), y.data_ptr(), conv.Ws.data_ptr(), conv.bias.data_ptr(), None, h, w, h, w, 1, cin, cout, 0, 1, None, waves,
                                           rec.data_ptr(), None, hip.current_stream()), "pod_conv1x1_split")
    assert not bool(torch.isfinite(y[p]).any())
    pre, bound = c1_reference(x, wt, b, h, w, 1, None)
    keep = torch.arange(h * w, device="cuda") != p
    assert bool(torch.isfinite(y[keep]).all())
    c = float(((y.double() - pre).abs() / (EPS * bound))[keep].max())
    print("c(other pixels under a record 4 x too low) = %.2f" % c)
    assert c <= 8.0


# ---- 5. pod_compare_amd/amax.py on the device ---------------------------------------------------------------------------------------------
def test_of_returns_the_attached_record_until_the_tensor_changes():
    x = torch.randn(100, 16, device="cuda", generator=gen(1))
    rec = amax.of(x)
    assert rec_max(rec) == absmax(x)
    assert amax.of(x) is rec                                       # (still what was measured: no second pod_absmax, the same record)
    x.add_(1.0)
    again = amax.of(x)
    assert again is not rec and again.data_ptr() != rec.data_ptr()
    assert rec_max(again) == absmax(x) != rec_max(rec)
    loose = full_record(100.0)
    assert amax.of(amax.attach(x, loose)) is loose                 # an attached bound is trusted as it is ...
    x.mul_(2.0)
    assert rec_max(amax.of(x)) == absmax(x)                        # ... until the next in-place op
    amax.attach(x, loose)
    amax.forget(x)
    assert not hasattr(x, "_pod_amax") and rec_max(amax.of(x)) == absmax(x)
    amax.forget(torch.zeros(4, device="cuda"))                     # (nothing attached: a no-op)


def test_produced_hands_out_a_fresh_zeroed_record_or_the_shared_one():
    buf = torch.empty(10, 8, device="cuda")
    shared = amax.word(buf.device)
    parts = [buf[:4], buf[4:]]
    for part in parts:
        part._pod_amax_shared = shared
    assert all(amax.produced(part) is shared and part._pod_amax[0] is shared and part._pod_amax[1] == part._version for part in parts)
    a, b = amax.produced(buf), amax.produced(buf)
    assert a is not shared and a.data_ptr() not in (b.data_ptr(), shared.data_ptr())
    assert buf._pod_amax[0] is b and bool((a == 0).all()) and bool((b == 0).all()) and a.numel() == b.numel() == RECORD


def test_joined_gives_the_larger_of_two_bounds():
    small, large = torch.randn(64, 8, device="cuda", generator=gen(2)), torch.randn(50, 8, device="cuda", generator=gen(3)) * 9.0
    dst = torch.cat([small, large])
    assert amax.joined(dst, small, large) is dst
    assert rec_max(amax.of(dst)) == max(absmax(small), absmax(large)) == absmax(dst)
    amax.attach(small, full_record(1000.0))                        # a source's looser bound carries over
    assert rec_max(amax.of(amax.joined(dst, large, small))) == 1000.0


def test_the_pool_rolls_over_without_handing_out_a_live_record_twice():
    live = [amax.word(torch.device("cuda")) for _ in range(2 * amax.POOL_WORDS + 3)]
    assert len({r.data_ptr() for r in live}) == len(live)
    spans = sorted((r.data_ptr(), r.data_ptr() + 4 * RECORD) for r in live)
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:]))     # no two records overlap
    assert all(r.numel() == RECORD for r in live) and bool((torch.stack(live) == 0).all())
    for i, r in enumerate(live):
        slots(r).fill_(float(i + 1))
    assert all(rec_max(r) == float(i + 1) for i, r in enumerate(live))


@pytest.mark.parametrize("h,w", [(5, 7), (1, 1), (16, 9)])
def test_the_max_pool_carries_its_input_record_over(h, w):
    x = torch.randn(h * w, 8, device="cuda", generator=gen(h)) - 1.0
    rec = amax.of(x)
    y, _, _ = maxpool3x3s2_cl(x, h, w)
    assert amax.of(y) is rec and rec_max(rec) >= absmax(y)
    x.add_(100.0)                                                  # a stale record does not travel
    y2, _, _ = maxpool3x3s2_cl(x, h, w)
    assert not hasattr(y2, "_pod_amax") and rec_max(amax.of(y2)) == absmax(y2) > 50.0


def watch_records(monkeypatch, log):
    """Wraps amax.of (every consumption of a record goes through it): log += (consumer, tensor abs-max, record max), both device scalars
    taken at that moment on the stream."""
    inner = amax.of

    def of(t):
        rec = inner(t)
        f = sys._getframe(1)
        log.append((f.f_code.co_name, t, t.abs().max(), slots(rec).max()))
        return rec
    monkeypatch.setattr(amax, "of", of)


@pytest.mark.parametrize("h,w,relu_input", [(5, 7, False), (5, 7, True), (1, 1, False), (6, 4, True)])
def test_the_patch_matrix_is_bounded_by_its_input_record(h, w, relu_input, monkeypatch):
    C, K = 16, 64
    g = gen(h * w)
    x = torch.randn(h * w, C, device="cuda", generator=g)
    x[h * w // 2, 3] = -40.0                                       # (with relu_input the patch matrix never holds it: the bound stays loose)
    wt, b = torch.randn(K, C, 3, 3, device="cuda", generator=g) * 0.1, torch.randn(K, device="cuda", generator=g)
    conv = Conv3x3S2(wt, b)
    log = []
    watch_records(monkeypatch, log)
    y, ho, wo = conv(x, h, w, relu_input=relu_input)
    cols = [(t, float(true), float(bound)) for _, t, true, bound in log if tuple(t.shape) == (ho * wo, 9 * C)]
    assert len(cols) == 1 and len(log) == 2                        # x's record (measured), then the patch matrix with that record attached
    t, true, bound = cols[0]
    assert bound == absmax(x) == 40.0 and bound >= true == absmax(t)
    assert (true < 40.0) == relu_input
    want = F.conv2d((x.relu() if relu_input else x).view(1, h, w, C).permute(0, 3, 1, 2).double(), wt.double(), b.double(), stride=2, padding=1)
    assert float((y.view(1, ho, wo, K).permute(0, 3, 1, 2).double() - want).abs().max()) <= 1e-4 * max(1.0, float(want.abs().max()))
    assert published(y) == absmax(y)


def test_the_stem_input_bound_bounds_the_normalised_frame():
    wt, b, g = stem_weights(2)
    stem = Stem7x7(wt, b)
    mean, std = torch.tensor([103.53, 116.28, 123.675], device="cuda"), torch.tensor([1.0, 57.375, 58.395], device="cuda")
    for frame in (torch.randint(0, 256, (3, 9, 14), dtype=torch.uint8, device="cuda", generator=g), torch.full((3, 2, 2), 255, dtype=torch.uint8, device="cuda"),
                  torch.zeros(3, 2, 2, dtype=torch.uint8, device="cuda"), torch.rand(3, 9, 14, device="cuda", generator=g) * 255.0,
                  torch.randn(3, 9, 14, device="cuda", generator=g) * 1000.0):
        true = absmax((frame.float() - mean.view(3, 1, 1)) / std.view(3, 1, 1))
        bound = stem._input_bound(frame, mean, std)
        assert bound.numel() == RECORD and rec_max(bound) >= true, frame.dtype
    x = torch.randn(3, 9, 14, device="cuda", generator=g)
    assert rec_max(stem._input_bound(x, None, None)) == absmax(x)  # already normalised: the frame's own record


def stale_record_case():
    from pod_compare_amd.wino import block_table
    C, K, h, w = 128, 64, 6, 11
    g = gen(4)
    wt, b = torch.randn(K, C, 3, 3, device="cuda", generator=g) * 0.1, torch.randn(K, device="cuda", generator=g)
    return wt, b, torch.randn(h * w, C, device="cuda", generator=g) * 5.0, block_table([(h, w)], 1, "cuda"), h * w, K


def test_the_fp32_mfma_launch_drops_its_destinations_record():
    """The pod_* kernels write through raw pointers and bump no version: a launch without out_amax must leave no stale record on its
    destination (pod_wino_conv3x3 has no out_amax at all)."""
    from pod_compare_amd.wino import WinoConv
    wt, b, src, table, pixels, K = stale_record_case()
    dst = torch.zeros(pixels, K, device="cuda")
    assert rec_max(amax.of(dst)) == 0.0                            # dst carries a record of its zeros
    WinoConv(wt, b, split=False)(src, dst, table)
    assert rec_max(amax.of(dst)) == absmax(dst) > 1.0


def test_the_planes_reduce_launch_drops_its_destinations_record():
    """... and so must the planes form of a split convolution, whose reduce launch (pod_wino_reduce) is given no out_amax."""
    from pod_compare_amd.wino import WinoConv
    wt, b, src, table, pixels, K = stale_record_case()
    planes = torch.zeros(K * pixels, device="cuda")
    assert rec_max(amax.of(planes)) == 0.0
    WinoConv(wt, b, split=True).planes_of_one_image(src, planes, table, n_splits=2)
    assert rec_max(amax.of(planes)) == absmax(planes) > 1.0


# ---- 6. every record a real forward consumes bounds its tensor ---------------------------------------------------------------------------
# Split launches of one eager forward of the ResNet-50-FPN RetinaNet, read off pod_compare_amd/modeling.py: the stem (1); 16 bottlenecks x
# (conv1, conv2, conv3) + 4 shortcuts (52); FPN: 3 laterals + 3 output convs + p6 + p7 (8); the head with grouped launches: 4 subnet layers
# + the predictors (5).  Every launch consumes at least one record (a grouped launch one per set), so a forward that the hooks saw
# fewer than this many consumptions of has bypassed them.
LAUNCHES_PER_FORWARD = 1 + 52 + 8 + 5
FRAME_HW = (97, 131)                                   # padded to 128 x 160: levels 16 x 20, 8 x 10, 4 x 5, 2 x 3, 1 x 2 -- every one ragged


class Consumptions:
    """Hooks on every path a record reaches a launch by -- amax.of and the stem's own Stem7x7._input_bound -- plus amax.produced and
    sparse.LiveBlocks.__call__ to know what a record was made for.  Each consumption: (site, kind, max |tensor| now, record max), device
    scalars.  kind 'exact': the record is pod_absmax's of this very tensor, or a launch's out_amax for exactly this tensor (no dropout
    mask, no sparse launch), or the record several launches shared for exactly the slices this buffer consists of -- equality is owed;
    'bound': anything carried or computed (the max-pool and im2col carry-overs, a slice under its buffer's shared record, a masked or
    sparse output, the stem's analytic bound)."""

    def __init__(self, monkeypatch):
        from pod_compare_amd import sparse
        self.log, self.keep, self.fresh, self.shared, self.live = [], [], {}, {}, None
        of, produced, input_bound, live_call = amax.of, amax.produced, Stem7x7._input_bound, sparse.LiveBlocks.__call__
        me = self

        def site(f):
            owner = f.f_locals.get("self")
            return (type(owner).__name__ + "." if owner is not None else "") + f.f_code.co_name

        def hooked_of(t):
            had = getattr(t, "_pod_amax", None)
            attached = had is not None and had[1] == t._version
            rec = of(t)
            f = sys._getframe(1)
            sparse_read = f.f_locals.get("live") is not None
            made_for = me.fresh.get(rec.data_ptr())
            parts = me.shared.get(rec.data_ptr())
            exact = (not attached) or (made_for == (t.data_ptr(), t.numel(), False)) or \
                    (parts is not None and min(p for p, _ in parts) == t.data_ptr() and sum(n for _, n in parts) == t.numel())
            where = "%s, C = %d%s" % (site(f), t.shape[-1], " (sparse)" if sparse_read else "")
            me.log.append((where, "exact" if exact and not sparse_read else "bound", me.read(t, sparse_read), slots(rec).max()))
            me.keep.append(rec)                                    # (a live record's address is never handed out again)
            return rec

        def hooked_produced(t):
            rec = produced(t)
            f = sys._getframe(1)
            loose = float(f.f_locals.get("dropout_p", 0.0) or 0.0) > 0.0 or f.f_locals.get("live") is not None
            if getattr(t, "_pod_amax_shared", None) is None:
                me.fresh[rec.data_ptr()] = (t.data_ptr(), t.numel(), loose)
                me.shared.pop(rec.data_ptr(), None)
            else:
                me.shared.setdefault(rec.data_ptr(), []).append((t.data_ptr(), t.numel()))
                me.fresh.pop(rec.data_ptr(), None)
            me.keep.append(rec)
            return rec

        def hooked_input_bound(stem, x, mean, std):
            rec = input_bound(stem, x, mean, std)
            xn = x.float() if mean is None else (x.float() - mean.view(3, 1, 1)) / std.view(3, 1, 1)
            me.log.append(("Stem7x7._input_bound [%s]" % str(x.dtype).replace("torch.", ""), "bound", xn.abs().max(), slots(rec).max()))
            return rec

        def hooked_live(lb, table, reach, in_reach=-1):
            me.live = (lb, int(reach) + 1 if in_reach < 0 else int(in_reach))
            return live_call(lb, table, reach, in_reach)

        monkeypatch.setattr(amax, "of", hooked_of)
        monkeypatch.setattr(amax, "produced", hooked_produced)
        monkeypatch.setattr(Stem7x7, "_input_bound", hooked_input_bound)
        monkeypatch.setattr(sparse.LiveBlocks, "__call__", hooked_live)

    def read(self, t, sparse_read):
        """max |t| over what the consumer reads: all of it -- or, in a sparse launch, the cells whose reach is within the launch's in_reach
        (the others are read as 0.0: they may hold another layer's values; docstring of test_sparse_tower_gives_the_dense_towers_detections)"""
        if not sparse_read:
            return t.abs().max()
        lb, in_reach = self.live
        copies = t.shape[0] // lb.cells
        assert copies * lb.cells == t.shape[0]
        ok, at = [], 0
        for h, w in lb.hp.shapes:
            ok.append((lb.reach[at:at + h * w] <= in_reach).repeat(copies))
            at += h * w
        return (t.abs().amax(dim=1) * torch.cat(ok)).max()

    def check(self, forwards):
        """-> {site: largest record / true ratio over its 'bound' consumptions}"""
        assert len(self.log) >= forwards * LAUNCHES_PER_FORWARD, len(self.log)
        true = torch.stack([e[2] for e in self.log]).cpu().tolist()
        bound = torch.stack([e[3] for e in self.log]).cpu().tolist()
        ratios, exact = {}, 0
        for (where, kind, _, _), t, b in zip(self.log, true, bound):
            assert b >= t, (where, kind, t, b)
            if kind == "exact":
                assert b == t, (where, t, b)
                exact += 1
            elif t > 0.0:
                ratios[where] = max(ratios.get(where, 1.0), b / t)
        assert exact >= forwards * 50                              # the trunk's chain of produced records, at the least
        for where in sorted(ratios):
            print("amax record / true abs-max, largest over %-52s %8.3f" % (where, ratios[where]))
        print("consumptions: %d, of which exact: %d" % (len(self.log), exact))
        return ratios


def frame_u8(seed):
    return torch.randint(0, 256, (3,) + FRAME_HW, dtype=torch.uint8, device="cuda", generator=gen(seed))


def test_every_record_of_a_plain_forward_bounds_its_tensor(monkeypatch):
    from tests.test_sparse_tower_gpu import build
    m = build(plain=True)
    seen = Consumptions(monkeypatch)
    m(frame_u8(1))
    m(frame_u8(2).float())                                         # a float frame: the stem's bound is measured + analytic
    seen.check(2)


def test_every_record_of_an_mc_dropout_forward_bounds_its_tensor(monkeypatch):
    """The variance heads, dropout 0.2, 3 MC-dropout runs: a masked output's record holds max |value before the mask| / (1 - p) -- a bound."""
    from tests.test_sparse_tower_gpu import build
    m = build(dropout_rate=0.2)
    seen = Consumptions(monkeypatch)
    m(frame_u8(3), num_mc_dropout_runs=3, mc_dropout=True, skip_unused_last_run=True)
    m(frame_u8(4), num_mc_dropout_runs=3, mc_dropout=True, skip_unused_last_run=False)
    ratios = seen.check(2)
    assert any("_launch_split" in k for k in ratios)               # (the masked layers were seen as such)


def test_every_record_of_a_sparse_tower_forward_bounds_what_the_launch_reads(monkeypatch):
    """The predictor with sparse_bbox_tower = True, MC dropout, 3 runs: the bbox tower's launches consume records too (the layer below's
    out_amax, published over its live blocks).  Each must bound the cells the sparse launch reads."""
    import os
    from pod_compare_amd import config
    from pod_compare_amd.probabilistic_inference import build_predictor
    from tests.test_sparse_tower_gpu import build
    root = os.path.join(os.path.dirname(os.path.abspath(config.__file__)), "configs")
    cfg = config.setup_config(os.path.join(root, "BDD-Detection", "retinanet", "retinanet_R_50_FPN_1x_reg_cls_var_dropout.yaml"),
                              os.path.join(root, "Inference", "bayes_od_mc_dropout.yaml"))
    cfg.MODEL.DEVICE = "cuda"
    m = build(dropout_rate=0.2)
    with torch.no_grad():                                          # (a random-init head has no candidates: let every level fill its top-k)
        m.head.cls_score.weight.mul_(40.0)
        m.head.cls_score.bias.fill_(-2.5)
    p = build_predictor(cfg, model=m)
    p.sparse_bbox_tower, p.num_mc_dropout_runs = True, 3
    seen = Consumptions(monkeypatch)
    for seed in (5, 6):                                            # the second image finds the first one's values in the tower's buffers
        out = p([{"image": frame_u8(seed), "height": FRAME_HW[0], "width": FRAME_HW[1], "image_id": seed}])
        assert len(out) > 0
    assert p._sparse_ok()
    ratios = seen.check(2)
    assert any("(sparse)" in k for k in ratios)
