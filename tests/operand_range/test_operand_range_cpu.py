"""What tests/operand_range holds the forward split convolutions to, checked without a GPU: the plain torch emulation of the split product
(ranges.emulate: x0 = f16(x s), x1 = f16(x s - x0), three partial products in fp32, the inverse scale last) satisfies every bound and
precondition of sections 1 to 4 on the very inputs the GPU modules use -- so a correct kernel can pass -- and the same emulation with an
f16 conversion that flushes denormals does not -- so the tests would notice."""
import pytest
import torch

from tests.operand_range import ranges as R

C1 = pytest.mark.parametrize("cin,splits,waves", [pytest.param(*f, id=i) for f, i in zip(R.C1_FORMS, R.C1_FORM_IDS)])


def flushing(prob, record=None):
    return R.emulate(prob, record, flush=True)


def test_the_scale_functions_restate_the_header():
    """wino_pow2_scale puts R into [2^top, 2^(top+1)) at both ends of a binade; its clamps; wino_pow2_inverse"""
    for m in (-100, -3, 0, 3, 100):
        for top in (R.SG_TOP, R.WINO_V_TOP):
            lo, hi = 2.0 ** m, float(torch.nextafter(torch.tensor(2.0 ** (m + 1)), torch.tensor(0.0)))
            s = R.pow2_scale(lo, top)
            assert s == R.pow2_scale(hi, top) == 2.0 ** (top - m) and lo * s == 2.0 ** top and hi * s < 2.0 ** (top + 1)
            assert R.pow2_inverse(s) * s == 1.0
    assert R.pow2_scale(0.0, 14) == R.pow2_scale(2.0 ** -120, 14) == 2.0 ** 127 and R.pow2_inverse(2.0 ** 127) == 0.0
    assert R.pow2_scale(float("inf"), 14) == 2.0 ** -114           # (exponent field 255: the smallest scale a record can ask for)


def test_the_winograd_gains():
    """The claim at WINO_V_TOP (csrc/k12_wino_conv_split.hip): 'gain of Bt4 (x) Bt6 < 32'.  Largest product of absolute row sums: 2 x 10."""
    ia, ib, gain = R.worst_rows(R.BT4, R.BT6)
    assert (R.row_sums(R.BT4)[ia], R.row_sums(R.BT6)[ib], gain) == (2, 10, 20) and gain < 32
    assert 2.0 ** (R.WINO_V_TOP + 1) * gain < 65504.0            # the scaled, transformed maximum stays an f16 number
    assert R.GAIN_G == 1.5 and R.GAIN_A == 57
    # the matrices are a Winograd convolution: the emulation meets C_BOUND on unit-range data (so they restate the kernel's, not just any)
    for name in R.WINO_NAMES:
        p = R.wino_problem(name)
        want, bound, _ = p.reference()
        assert float(((R.emulate(p).double() - want).abs() / (R.EPS * bound)).max()) <= R.BAR["wino"]


@C1
def test_conv1x1_emulation_meets_sections_1_to_4(cin, splits, waves):
    for p in R.c1_problems(cin, splits, waves):
        R.check_activation_shifts(R.emulate, p)
        R.check_weight_shifts(R.emulate, p)
    for i, p in enumerate(R.c1_edge_problems(cin, splits, waves)):
        label = "emulation K13 Cin=%d map %d" % (cin, i)
        R.check_binade_edges(R.emulate, p, label)
        R.check_mixed(R.emulate, p, label)
        R.check_ends(R.emulate, p, label)


def test_conv3x3s2_emulation_scales_exactly():
    R.check_activation_shifts(R.emulate, R.c3s2_problem())
    R.check_weight_shifts(R.emulate, R.c3s2_problem())


@pytest.mark.parametrize("h,w", R.STEM_FRAMES)
def test_stem_emulation_meets_sections_1_to_4(h, w):
    label = "emulation K14 %dx%d" % (h, w)
    for relu in (False, True):
        R.check_activation_shifts(R.emulate, R.stem_problem(h, w, relu))
    p = R.stem_problem(h, w)
    R.check_weight_shifts(R.emulate, p)
    R.check_binade_edges(R.emulate, p, label)
    R.check_mixed(R.emulate, p, label)
    R.check_ends(R.emulate, p, label)


def test_stem_emulation_meets_the_uint8_case():
    p = R.stem_u8_problem()
    R.check_u8_frame(lambda q, record=None: R.emulate(q, R.stem_u8_record(q)), p, "emulation K14 uint8 frame under its analytic record")


@pytest.mark.parametrize("name", R.WINO_NAMES)
def test_wino_emulation_meets_sections_1_to_4(name):
    p, label = R.wino_problem(name), "emulation K12 " + name
    R.check_activation_shifts(R.emulate, p)
    R.check_weight_shifts(R.emulate, p)
    if name == "replicas":                     # (the masks are the kernel's: the emulation has none, and sections 2 to 4 run on the other forms)
        return
    R.check_binade_edges(R.emulate, p, label)
    R.check_mixed(R.emulate, p, label)
    R.check_ends(R.emulate, p, label)


def test_wino_emulation_at_the_worst_gain():
    q, rows = R.worst_gain_problem(R.wino_problem("cl"))
    want, bound, _ = q.reference()
    y = R.emulate(q)
    assert bool(torch.isfinite(y).all())
    assert float(((y.double() - want).abs() / (R.EPS * bound))[rows].max()) <= R.BAR["wino"]


def test_k12_sharpness_figures():
    """Printed, not asserted (ranges.py, module docstring): for K12 the derived T is no tenth of c 2^-24 B at any d of the list."""
    p = R.wino_problem("cl")
    for d in R.D_SHIFTS:
        q, dim = R.mixed(p, d)
        want, B, sx = q.reference()
        small, large = R.sharpness(q, d, B, q.T(q.record_max(), sx), dim)
        print("K12 d=%d: T < c 2^-24 B / 10 on %.1f %% of the dim elements, T > 2^-24 B on %.1f %%" % (d, 100 * small, 100 * large))


# ---- an f16 unit that flushes denormals must not pass --------------------------------------------------------------------------------------
def flush_cases():
    out = [pytest.param(R.c1_edge_problems(*f)[0], id="K13-" + i) for f, i in zip(R.C1_FORMS, R.C1_FORM_IDS)]
    out += [pytest.param(R.stem_problem(*f), id="K14-%dx%d" % f) for f in R.STEM_FRAMES]
    return out + [pytest.param(R.wino_problem(n), id="K12-" + n) for n in ("cl", "planes", "c16")]


@pytest.mark.parametrize("prob", flush_cases())
def test_flushing_f16_denormals_fails_section_3_at_d_24(prob):
    """With .half() flushing, the d = 24 case fails: by the bound itself wherever the errors of a dot product, which add like sqrt(Cin),
    outgrow T, which adds like Cin (every form but K13 at Cin = 128) -- and by the comparison with the first-term-only evaluation in
    every form of K13 and K14; K12, whose activation scale is 5 binades lower, loses the first terms too at d = 24 and fails that
    comparison at d = 18."""
    with pytest.raises(AssertionError):
        R.check_mixed(flushing, prob, "flushing", ds=(24,))
    figures = R.check_mixed(flushing, prob, "flushing", enforce=False, ds=(24,), second_terms=False)
    violated = max(figures.values()) > R.BAR[prob.kind]
    if not (prob.kind == "c1" and prob.w.shape[1] >= 128):
        assert violated, figures
    with pytest.raises(AssertionError, match="second terms"):
        R.check_mixed(flushing, prob, "flushing", enforce=False, ds=(18 if prob.kind == "wino" else 24,))
    for d in (18, 30):                     # (and every form of K13 and K14 fails the bound a binade group to either side)
        if prob.kind != "wino":
            assert max(R.check_mixed(flushing, prob, "flushing", enforce=False, ds=(d,), second_terms=False).values()) > R.BAR[prob.kind], d
