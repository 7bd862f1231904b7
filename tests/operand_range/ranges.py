"""Operand range of the forward split convolutions (K12 pod_wino_conv3x3_split, K13 pod_conv1x1_split, K14 pod_stem7x7_split): the
inputs, the fp64 references and the properties, written once.  A property takes `run(problem, record=None) -> (pixels, K) fp32 on the
CPU`: the GPU modules pass the kernels' wrappers, test_operand_range_cpu.py passes `emulate` below, so that what the kernels are held to
is shown, without a GPU, to be satisfiable -- and to fail for an f16 unit that flushes denormals.

THE CONTRACT (csrc/pod_split_gemm.h).  Every operand tensor is multiplied by a power of two s taken from an abs-max record R >= max |x|,
s R in [2^top, 2^(top + 1)), and every scaled value is carried by two f16 terms, x s = x0 + x1 + e.  Three partial products (x0 w1, x1 w0,
x0 w0) accumulate in fp32, the two scales come off again in the epilogue, exactly.

THE BOUND of section 3, per output element:   |y - fp64| <= c 2^-24 B + T
  B = |x| * |w| + |b| + |residual|, the magnitude bound every forward test of these kernels uses; c the module's existing bar (8, 32, 8);
  T, the absolute term, DERIVED from the header's promise "values far below the abs-max keep an absolute error of 2^-25 / s":
    a term in f16's denormals is a multiple of 2^-24, so |e| <= 2^-25 in scaled units, 2^-25 / s unscaled, and 1 / s <= 2^-top R.  One more
    bit for the second term's own rounding on top of the first's: 2^-(24 + top) R per activation, 2^-(24 + top) W per weight (W the
    filter's abs-max).  Each meets the other operand's magnitude:
      K13, K14 (top = 14 both):   T = 2^-38 (R sum_c |w| + W sum_c |x|)         (sums over the dot product of the output element; a tap
        on the stem's zero padding is zero in both terms and adds nothing)
      K12: the activations are split AFTER the input transform, V = Bt4 d Bt6^T, under WINO_V_TOP = 9 (the record bounds d, the scale leaves
        room for the transform's gain): |e_V| <= 2^-33 R per transformed value.  It meets U = G4 g G6^T, |U| <= gG max_tap |g| <= gG sum_tap |g|
        (gG: the largest product of absolute row sums of G4 and G6), and the output transform adds up to gA such products per output (gA:
        At2, At4 likewise).  The filter side: |e_U| <= 2^-38 max |U| <= 2^-38 gG W per value, met by |V| <= gB max |d|, summed over the C
        channels -- bounded with the abs-max X of the element's own level (a tile never leaves its level's canvas):
          T = gA gG (2^-33 R sum_{c,tap} |w| + 2^-38 gB W C X)
  Nothing in T is measured.

What the derivation also says: for K12 the absolute term outweighs the fp32 class already for data 2^6 below the record (2^-33 gA gG
against 32 x 2^-24 x 2^-d), so the sharpness precondition "T < a tenth of c 2^-24 B for d <= 12" can hold for K13 and K14 only; for K12
the figure is printed (test_operand_range_cpu.py)."""
import struct

import torch
import torch.nn.functional as F

EPS = 2.0 ** -24
SG_TOP, WINO_U_TOP, WINO_V_TOP = 14, 14, 9          # csrc/pod_split_gemm.h: SG_TOP; csrc/k12_wino_conv_split.hip: WINO_U_TOP, WINO_V_TOP
BAR = {"c1": 8.0, "c3s2": 8.0, "stem": 8.0, "wino": 32.0}      # tests/test_conv1x1_gpu.py, tests/test_stem_gpu.py; tests/test_wino_conv_gpu.py: C_BOUND
K_SHIFTS = (-60, -17, -1, 1, 14, 60)
J_SHIFTS = (-30, 9)
D_SHIFTS = (6, 12, 18, 24, 30)
M_PLANT = 3                                         # binade of the planted maxima of section 2: 8.0 .. 16.0

# The Winograd matrices, restated from csrc/pod_wino.h: G4, G6 at "the filter transform U = G4 g G6t" (lines 156-157); At2, At4 at "OUTPUT
# TRANSFORM" (line 302); Bt4 at wino_rows (line 222); Bt6 from the column transform of csrc/k12_wino_conv_split.hip (columns_level1 / 2).
BT4 = [[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]]
BT6 = [[4, 0, -5, 0, 1, 0], [0, -4, -4, 1, 1, 0], [0, 4, -4, -1, 1, 0], [0, -2, -1, 2, 1, 0], [0, 2, -1, -2, 1, 0], [0, 4, 0, -5, 0, 1]]
G4 = [[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]]
G6 = [[1 / 4, 0, 0], [-1 / 6, -1 / 6, -1 / 6], [-1 / 6, 1 / 6, -1 / 6], [1 / 24, 1 / 12, 1 / 6], [1 / 24, -1 / 12, 1 / 6], [0, 0, 1]]
AT2 = [[1, 1, 1, 0], [0, 1, -1, -1]]
AT4 = [[1, 1, 1, 1, 1, 0], [0, 1, -1, 2, -2, 0], [0, 1, 1, 4, 4, 0], [0, 1, -1, 8, -8, 1]]


def row_sums(m):
    return [sum(abs(v) for v in row) for row in m]


def worst_rows(a, b):
    """(row of a, row of b, product) with the largest product of absolute row sums"""
    ra, rb = row_sums(a), row_sums(b)
    ia, ib = max(range(len(ra)), key=ra.__getitem__), max(range(len(rb)), key=rb.__getitem__)
    return ia, ib, ra[ia] * rb[ib]


GAIN_B = worst_rows(BT4, BT6)[2]        # 2 x 10 = 20: the input transform (the claim at WINO_V_TOP: < 32)
GAIN_G = worst_rows(G4, G6)[2]          # 1.5 x 1 = 1.5
GAIN_A = worst_rows(AT2, AT4)[2]        # 3 x 19 = 57


# ---- the scale functions of pod_split_gemm.h, on the host --------------------------------------------------------------------------------
def f32_bits(v):
    return struct.unpack("<I", struct.pack("<f", v))[0]


def pow2_scale(amax, top):
    """wino_pow2_scale: 2^(top - floor(log2 amax)), the exponent field clamped to 1 .. 254"""
    e = (f32_bits(amax) >> 23) & 0xFF
    return 2.0 ** (min(max(254 + top - e, 1), 254) - 127)


def pow2_inverse(s):
    """wino_pow2_inverse (2^127 -> 0.0: the documented end of its range)"""
    return struct.unpack("<f", struct.pack("<I", (254 << 23) - f32_bits(s)))[0]


def f32_mul(a, b):
    return float(torch.tensor(a, dtype=torch.float32) * torch.tensor(b, dtype=torch.float32))


def to_half(t, flush):
    h = t.half()
    return torch.where(h.abs() < 2.0 ** -14, torch.zeros_like(h), h) if flush else h


def split2(v, s, flush=False):
    """x0 = f16(v s), r = v s - x0 (exact in fp32), x1 = f16(r)"""
    vs = v * s
    x0 = to_half(vs, flush).float()
    return x0, to_half(vs - x0, flush).float()


def gen(seed):
    return torch.Generator().manual_seed(seed)


# ---- a convolution problem -----------------------------------------------------------------------------------------------------------------
class Problem:
    """kind 'c1'   : x (h w, Cin) channels-last, w (Cout, Cin, 1, 1); opt: H, W, stride, splits, waves, up2 (res is the half-resolution map)
            'c3s2' : x (h w, C) channels-last, w (K, C, 3, 3); opt: H, W                               (Conv3x3S2)
            'stem' : x (1, 3, H, W) float or (3, H, W) uint8 with opt mean, std; w (64, 3, 7, 7)
            'wino' : x a list of (copies, C, h, w), one per level; w (K, C, 3, 3); opt: planes, splits, replicas, p
       b, res: None or tensors; opt relu.  Outputs are (pixels, K), channels-last, level-major."""

    def __init__(self, kind, x, w, b=None, res=None, **opt):
        self.kind, self.x, self.w, self.b, self.res, self.opt = kind, x, w, b, res, opt
        self.relu = bool(opt.get("relu", False))

    def but(self, **kw):
        f = dict(x=self.x, w=self.w, b=self.b, res=self.res)
        f.update({k: kw.pop(k) for k in list(kw) if k in f})
        return Problem(self.kind, f["x"], f["w"], f["b"], f["res"], **{**self.opt, **kw})

    def scaled(self, k=0, j=0):
        a, f = 2.0 ** k, 2.0 ** j
        x = [t * a for t in self.x] if self.kind == "wino" else self.x * a
        return self.but(x=x, w=self.w * f, b=None if self.b is None else self.b * a, res=None if self.res is None else self.res * a)

    def geometry(self):
        return {"c1": (self.opt.get("stride", 1), 0), "c3s2": (2, 1), "stem": (2, 3), "wino": (1, 1)}[self.kind]

    def images(self):
        """the NCHW fp32 images the convolution reads"""
        if self.kind == "wino":
            return list(self.x)
        if self.kind == "stem":
            x = self.x
            if x.dtype == torch.uint8:
                x = (x.float() - self.opt["mean"].view(3, 1, 1)) / self.opt["std"].view(3, 1, 1)
            return [x.reshape(1, 3, x.shape[-2], x.shape[-1])]
        return [self.x.view(1, self.opt["H"], self.opt["W"], -1).permute(0, 3, 1, 2)]

    def with_images(self, xs):
        if self.kind == "wino":
            return self.but(x=list(xs))
        if self.kind == "stem":
            return self.but(x=xs[0].contiguous())
        return self.but(x=xs[0].permute(0, 2, 3, 1).reshape(self.x.shape).contiguous())

    def record_max(self):
        return max(float(x.abs().max()) for x in self.images())

    def out_hw(self, x):
        s, p = self.geometry()
        k = self.w.shape[-1]
        return (x.shape[-2] + 2 * p - k) // s + 1, (x.shape[-1] + 2 * p - k) // s + 1

    def res_full(self):
        if self.res is None or not self.opt.get("up2"):
            return self.res
        ho, wo = self.out_hw(self.images()[0])
        hr, wr = (ho + 1) // 2, (wo + 1) // 2
        return self.res.view(hr, wr, -1).repeat_interleave(2, 0).repeat_interleave(2, 1)[:ho, :wo].reshape(ho * wo, -1)

    def conv(self, xs, w):
        s, p = self.geometry()
        return torch.cat([F.conv2d(x, w, stride=s, padding=p).permute(0, 2, 3, 1).reshape(-1, w.shape[0]) for x in xs])

    def finish(self, y):
        """+ bias + residual, ReLU -- in y's precision"""
        if self.b is not None:
            y = y + self.b.to(y.dtype)
        if self.res is not None:
            y = y + self.res_full().to(y.dtype)
        return y.relu() if self.relu else y

    def reference(self):
        """-> (fp64 result, B, sum over the element's window of |x|), each (pixels, K) / (pixels,)"""
        xs, w = [x.double() for x in self.images()], self.w.double()
        bound = self.conv([x.abs() for x in xs], w.abs())
        if self.b is not None:
            bound = bound + self.b.double().abs()
        if self.res is not None:
            bound = bound + self.res_full().double().abs()
        sx = self.conv([x.abs() for x in xs], torch.ones_like(w[:1]))[:, 0]
        return self.finish(self.conv(xs, w)), bound, sx

    def T(self, R, sx):
        """the absolute term (module docstring) under a record R; (pixels, K)"""
        w = self.w.double()
        sw, W = w.abs().sum(dim=(1, 2, 3)), float(w.abs().max())
        if self.kind != "wino":         # (a tap on the zero padding is an exact zero in both terms: the sum runs over the taps inside the image)
            inside = self.conv([torch.ones_like(x, dtype=torch.float64) for x in self.images()], w.abs())
            return 2.0 ** -(24 + SG_TOP) * (R * inside + W * sx[:, None])
        level_max = torch.cat([torch.full((x.shape[0] * x.shape[2] * x.shape[3],), float(x.abs().max()), dtype=torch.float64) for x in self.x])
        return GAIN_A * GAIN_G * (2.0 ** -(24 + WINO_V_TOP) * R * sw[None, :] + 2.0 ** -(24 + WINO_U_TOP) * GAIN_B * W * w.shape[1] * level_max[:, None])


# ---- the contract as plain torch: NOT a port of the kernels ------------------------------------------------------------------------------
def split_product(a, w, sa, sw, flush):
    """(P, n) x (K, n) -> the fp32 accumulators of the three partial products, small ones first"""
    a0, a1 = split2(a, sa, flush)
    w0, w1 = split2(w, sw, flush)

    def dot(u, v):          # every product of two f16 values is exact in fp32; torch.sum adds pairwise in fp32 (a BLAS call need not)
        return (u[:, None, :] * v[None, :, :]).sum(-1)
    return (dot(a1, w0) + dot(a0, w1)) + dot(a0, w0)


def wino_forward(xs, w, R, mode, flush=False):
    """mode 'emu': fp32 transforms, both operands split; 'x0': fp64 throughout with V rounded to its FIRST f16 term, the filter exact"""
    dt = torch.float32 if mode == "emu" else torch.float64
    bt4, bt6, g4, g6, at2, at4 = (torch.tensor(m, dtype=dt) for m in (BT4, BT6, G4, G6, AT2, AT4))
    U = torch.einsum("ai,kcij,pj->kcap", g4, w.to(dt), g6)
    sv, K, C = pow2_scale(R, WINO_V_TOP), w.shape[0], w.shape[1]
    su = pow2_scale(float(U.abs().max()), WINO_U_TOP)
    inv = f32_mul(pow2_inverse(sv), pow2_inverse(su))
    outs = []
    for x in xs:
        n, _, h, wd = x.shape
        th, tw = (h + 1) // 2, (wd + 3) // 4
        d = F.pad(x.to(dt), (1, 4 * tw + 1 - wd, 1, 2 * th + 1 - h)).unfold(2, 4, 2).unfold(3, 6, 4)          # (n, c, th, tw, 4, 6)
        V = torch.einsum("ai,nctuij,pj->nctuap", bt4, d, bt6).permute(0, 2, 3, 4, 5, 1).reshape(-1, 24, C)     # (tiles, position, c)
        if mode == "emu":
            M = torch.stack([split_product(V[:, q], U.reshape(K, C, 24)[:, :, q], sv, su, flush) for q in range(24)], dim=1)   # (tiles, 24, K)
        else:
            M = torch.einsum("tqc,kcq->tqk", (V * sv).half().double() / sv, U.reshape(K, C, 24))
        Y = torch.einsum("ya,ntuapk,xp->nktyux", at2, M.reshape(n, th, tw, 4, 6, K), at4)
        if mode == "emu":
            Y = Y * inv
        outs.append(Y.reshape(n, K, 2 * th, 4 * tw)[:, :, :h, :wd])
    return torch.cat([y.permute(0, 2, 3, 1).reshape(-1, K) for y in outs])


def emulate(prob, record=None, flush=False):
    R = prob.record_max() if record is None else float(record)
    if prob.kind == "wino":
        return prob.finish(wino_forward(prob.images(), prob.w, R, "emu", flush))
    s, p = prob.geometry()
    a = F.unfold(prob.images()[0], prob.w.shape[-2:], padding=p, stride=s)[0].t().contiguous()
    wm = prob.w.reshape(prob.w.shape[0], -1)
    sa, sw = pow2_scale(R, SG_TOP), pow2_scale(float(wm.abs().max()), SG_TOP)
    return prob.finish(split_product(a, wm, sa, sw, flush) * f32_mul(pow2_inverse(sa), pow2_inverse(sw)))


def first_term_only(prob, R):
    """fp64 evaluation with every activation rounded to f16 after scaling: what a kernel that dropped its second terms would compute"""
    if prob.kind == "wino":
        return prob.finish(wino_forward(prob.images(), prob.w, R, "x0"))
    s = pow2_scale(R, SG_TOP)
    return prob.finish(prob.conv([(x.double() * s).half().double() / s for x in prob.images()], prob.w.double()))


# ---- the cases -------------------------------------------------------------------------------------------------------------------------------
C1_FORMS = [(48, 1, 1), (32, 1, 1), (128, 1, 2), (128, 1, 4), (64, 2, 1)]          # (Cin, n_splits, waves): tests/amax_records/test_conv1x1_gpu.py, C1_FORMS
C1_FORM_IDS = ["direct-3-ksteps", "lds-1-wave", "lds-2-waves", "lds-4-waves", "2-splits+reduce"]
C1_MAPS = [(5, 13, 1), (9, 9, 2)]
STEM_FRAMES = [(17, 33), (7, 250)]


def c1_problem(cin, splits, waves, h, w, stride, cout=64, residual="none", relu=False, seed=0):
    g = gen(1000 * cin + 10 * h + cout + seed)
    ho, wo = (h - 1) // stride + 1, (w - 1) // stride + 1
    rows = {"none": 0, "full": ho * wo, "up2": ((ho + 1) // 2) * ((wo + 1) // 2)}[residual]
    return Problem("c1", torch.randn(h * w, cin, generator=g) * 1.5, torch.randn(cout, cin, 1, 1, generator=g) * (2.0 / cin) ** 0.5, torch.randn(cout, generator=g),
                   torch.randn(rows, cout, generator=g) * 2.0 if rows else None, H=h, W=w, stride=stride, splits=splits, waves=waves, up2=residual == "up2", relu=relu)


def c1_problems(cin, splits, waves):
    """every map and Cout, with and without a full-resolution residual and ReLU; one residual_up2 case"""
    out = [c1_problem(cin, splits, waves, h, w, s, cout, res, relu) for h, w, s in C1_MAPS for cout in (64, 128) for res, relu in (("none", False), ("full", True))]
    return out + [c1_problem(cin, splits, waves, 5, 13, 1, 64, "up2", True)]


def c1_edge_problems(cin, splits, waves):
    """the two maps, one with a residual and ReLU: sections 2 to 4"""
    return [c1_problem(cin, splits, waves, 5, 13, 1, 64, "full", True), c1_problem(cin, splits, waves, 9, 9, 2, 128)]


def c3s2_problem(seed=5):
    g = gen(seed)
    return Problem("c3s2", torch.randn(81, 32, generator=g) * 1.5, torch.randn(64, 32, 3, 3, generator=g) * (2.0 / 288) ** 0.5, torch.randn(64, generator=g), H=9, W=9, relu=True)


def stem_problem(h, w, relu=True, seed=0):
    g = gen(h * 1000 + w + seed)
    return Problem("stem", torch.randn(1, 3, h, w, generator=g) * 1.5, torch.randn(64, 3, 7, 7, generator=g) * (2.0 / 147) ** 0.5, torch.randn(64, generator=g), relu=relu)


def stem_u8_problem(h=17, w=33, seed=3):
    g = gen(seed)
    return Problem("stem", torch.randint(0, 256, (3, h, w), dtype=torch.uint8, generator=g), torch.randn(64, 3, 7, 7, generator=g) * (2.0 / 147) ** 0.5,
                   torch.randn(64, generator=g) * 0.01, relu=False, mean=torch.tensor([103.53, 116.28, 123.675]), std=torch.tensor([1.0, 57.375, 58.395]))


def stem_u8_record(prob):
    """conv1x1.normalised_input_bound for a uint8 frame: (255 + max |mean|) / min |std|"""
    return (255.0 + float(prob.opt["mean"].abs().max())) * (1.0 / float(prob.opt["std"].abs().min()))


def check_u8_frame(run, prob, label):
    """The one uint8 case: the frame is normalised on load under the analytic record -- channel 0 (std 1) up to 152, the others below 2.3:
    bright and dim data under one loose record, as a real stem launch has them.  The scaling properties do not apply (integers in)."""
    want, B, sx = prob.reference()
    return measure(label, run(prob), want, B, prob.T(stem_u8_record(prob), sx), BAR["stem"])


WINO_LEVELS = [(9, 13), (5, 7)]


def wino_problem(name, seed=0):
    """'cl': two levels, two copies, C = 32, K = 64, channels-last; 'planes': K = 36 as planes; 'c16': C = 16; 'splits': n_splits = 2 at
    (6, 11, 128, 64); 'replicas': one image per level stored 3 times under dropout masks, p = 0.25"""
    levels, copies, C, K, opt = {"cl": (WINO_LEVELS, 2, 32, 64, {}), "planes": (WINO_LEVELS, 2, 32, 36, {"planes": True}), "c16": (WINO_LEVELS, 2, 16, 64, {}),
                                 "splits": ([(6, 11)], 1, 128, 64, {"splits": 2}), "replicas": (WINO_LEVELS, 1, 32, 64, {"replicas": 3, "p": 0.25})}[name]
    g = gen(len(name) * 100 + C + seed)
    xs = [torch.randn(copies, C, h, w, generator=g) * 1.5 for h, w in levels]
    return Problem("wino", xs, torch.randn(K, C, 3, 3, generator=g) * (2.0 / (9 * C)) ** 0.5, torch.randn(K, generator=g), relu=True, **opt)


WINO_NAMES = ["cl", "planes", "c16", "splits", "replicas"]


# ---- the properties --------------------------------------------------------------------------------------------------------------------------
FIGURES = []            # (label, measured c, share of elements where T dominated, part of the bound used): what the tests printed, for profiles/operand_range.md


def measure(label, y, want, B, T, c, rows=None, enforce=True):
    """measured c = max over elements of (|err| - T)+ / (2^-24 B); share of the elements where T > c 2^-24 B; how much of the whole bound
    the worst element uses"""
    assert bool(torch.isfinite(y).all()), label
    err = (y.double() - want).abs()
    if rows is not None:
        err, B, T = err[rows], B[rows], (T[rows] if torch.is_tensor(T) else T)
    T = T if torch.is_tensor(T) else torch.full_like(B, float(T))
    excess = (err - T).clamp(min=0.0)
    need = torch.where(B > 0, excess / (EPS * B).clamp(min=1e-300), torch.where(excess > 0, torch.full_like(B, float("inf")), torch.zeros_like(B)))
    c_meas, share = float(need.max()), float((T > c * EPS * B).double().mean())
    full = c * EPS * B + T
    used = float(torch.where(full > 0, err / full.clamp(min=1e-300), (err > 0).double() * float("inf")).max())
    FIGURES.append((label, c_meas, share, used))
    print("operand_range %-58s c = %7.3f (bar %g)   T dominates on %5.1f %%   largest |err| / (c 2^-24 B + T) = %.3f" % (label, c_meas, c, 100.0 * share, used))
    if enforce:
        assert c_meas <= c, (label, c_meas)
    return c_meas


def normal_in_fp32(*ts):
    """no nonzero value outside fp32's normal range"""
    for t in ts:
        a = t.double().abs()
        a = a[a > 0]
        if a.numel() and not (float(a.min()) >= 2.0 ** -126 and float(a.max()) < 2.0 ** 127):
            return False
    return True


def shift_precondition(prob):
    """section 1's precondition: the fp64 reference of the shifted problem, its inputs and its bound stay normal fp32 values"""
    want, bound, _ = prob.reference()
    return normal_in_fp32(want, bound, prob.w, *prob.images()) and (prob.b is None or normal_in_fp32(prob.b))


def check_activation_shifts(run, prob):
    """1a. activations, bias and residual x 2^k under a fresh exact record: the result x 2^k, bit for bit"""
    base = run(prob)
    assert bool(torch.isfinite(base).all()) and shift_precondition(prob)
    for k in K_SHIFTS:
        q = prob.scaled(k=k)
        assert shift_precondition(q), k
        assert torch.equal(run(q), base * 2.0 ** k), (prob.kind, prob.opt, k)


def check_weight_shifts(run, prob):
    """1b. weights x 2^j, bias-free: the result x 2^j, bit for bit"""
    prob = prob.but(b=None, res=None)
    base = run(prob)
    assert bool(torch.isfinite(base).all())
    for j in J_SHIFTS:
        q = prob.scaled(j=j)
        assert shift_precondition(q), j
        assert torch.equal(run(q), base * 2.0 ** j), (prob.kind, prob.opt, j)


def planted_values(m=M_PLANT):
    lo = 2.0 ** m
    top = float(torch.nextafter(torch.tensor(2.0 ** (m + 1)), torch.tensor(0.0)))
    return [s * v for v in (lo, lo * (1.0 + 2.0 ** -23), top) for s in (1.0, -1.0)]


def plant_sites(prob):
    """(image, channel, y, x) of the planted maximum: first and last pixel and channel, a pixel of the ragged tail, (K12) a tile's corners"""
    xs = prob.images()
    first, last = xs[0], xs[-1]
    sites = [(0, 0, 0, 0, 0), (len(xs) - 1, last.shape[0] - 1, last.shape[1] - 1, last.shape[2] - 1, last.shape[3] - 1),
             (0, 0, 1, first.shape[2] - 1, first.shape[3] // 2 + 1)]
    if prob.kind == "wino":        # level 0, image 0 stands at the canvas origin: tiles are 2 x 4 from (0, 0)
        sites += [(0, 0, 3, 2, 4), (0, 0, 5, 1, 3)]
    return sites


def planted(prob, site, value, m=M_PLANT, seed=0):
    """the problem's activations replaced by uniform values below 2^m in magnitude, `value` at `site`"""
    g = gen(seed)
    xs = [(torch.rand(x.shape, generator=g) * 2.0 - 1.0) * 2.0 ** m for x in prob.images()]
    i, n, c, y, x = site
    xs[i][n, c, y, x] = value
    q = prob.with_images(xs)
    assert q.record_max() == abs(value) and int(sum((t.abs() == abs(value)).sum() for t in xs)) == 1
    return q


def check_binade_edges(run, prob, label):
    """2. the single largest element at 2^m, a last place above it and a last place below 2^(m+1), both signs, at every site: finite, the
    module's bar against fp64; and 2^m against its upper neighbour: the same result up to that bar"""
    c, worst = BAR[prob.kind], 0.0
    for site in plant_sites(prob):
        got = {}
        for v in planted_values():
            q = planted(prob, site, v)
            want, bound, _ = q.reference()
            y = run(q)
            assert bool(torch.isfinite(y).all()), (site, v)
            need = float(((y.double() - want).abs() / (EPS * bound)).max())
            worst = max(worst, need)
            assert need <= c, (label, site, v, need)
            got[v] = (y.double(), want, bound)
        for sgn in (1.0, -1.0):
            (ya, wa, ba), (yb, wb, bb) = got[sgn * 2.0 ** M_PLANT], got[sgn * 2.0 ** M_PLANT * (1.0 + 2.0 ** -23)]
            assert bool(((ya - yb).abs() <= c * EPS * (ba + bb) + (wa - wb).abs()).all()), (label, site, sgn)
    FIGURES.append((label + " binade edges", worst, 0.0, worst / c))
    print("operand_range %-58s c = %7.3f (bar %g)" % (label + " binade edges", worst, c))


def banded(shape, g, R):
    """magnitudes uniform in [R / 2, R), random signs: the record's scale is then as tight as the derivation of T takes it"""
    return (torch.rand(shape, generator=g) * 0.5 + 0.5) * R * torch.where(torch.rand(shape, generator=g) < 0.5, -1.0, 1.0)


def mixed(prob, d, R=8.0, seed=0):
    """3. bright and dim data under ONE record R = 2^3 (planted at the first element): K12: the last level x 2^-d; K13, K14: the lower half
    of the pixels x 2^-d.  No bias, no residual, no ReLU (they would swamp B).  -> (problem, rows of the outputs no bright value reaches)"""
    g = gen(seed + d)
    xs = [banded(x.shape, g, R) for x in prob.images()]
    xs[0].view(-1)[0] = R
    bright = [x.clone() for x in xs]
    if prob.kind == "wino":
        xs[-1] *= 2.0 ** -d
        bright[-1].zero_()
    else:
        h = xs[0].shape[2]
        xs[0][:, :, h // 2:] *= 2.0 ** -d
        bright[0][:, :, h // 2:] = 0.0
    q = prob.with_images(xs).but(b=None, res=None, relu=False)
    dim = q.with_images(bright).reference()[2] == 0
    assert q.record_max() == R and 0 < int(dim.sum()) < dim.numel()
    return q, dim


def homogeneous(prob, R=8.0, seed=0):
    g = gen(seed + 77)
    xs = [banded(x.shape, g, R) for x in prob.images()]
    xs[0].view(-1)[0] = R
    return prob.with_images(xs).but(b=None, res=None, relu=False)


def sharpness(prob, d, B, T, rows):
    """the two CPU preconditions that keep the bound sharp; -> the shares they are stated on"""
    c = BAR[prob.kind]
    small = float((T[rows] < 0.1 * c * EPS * B[rows]).double().mean())
    large = float((T[rows] > EPS * B[rows]).double().mean())
    if d <= 12 and prob.kind != "wino":         # (K12: module docstring)
        assert small >= 0.99, (prob.kind, d, small)
    if d >= 24:
        assert large >= 0.5, (prob.kind, d, large)
    return small, large


def check_mixed(run, prob, label, enforce=True, ds=D_SHIFTS, second_terms=True):
    """3. one record over bright and dim data, and homogeneous data under a record 2^d too high.  -> {(variant, d): measured c}"""
    c, out = BAR[prob.kind], {}
    for d in ds:
        h = homogeneous(prob)
        Rl = h.record_max() * 2.0 ** d
        want, B, sx = h.reference()
        T = h.T(Rl, sx)
        sharpness(h, d, B, T, slice(None))
        out["loose", d] = measure("%s record 2^%d too high" % (label, d), run(h, record=Rl), want, B, T, c, None, enforce)
        if prob.kind == "wino" and len(prob.x) < 2:              # (the form cut over its input channels serves one image: no second level)
            continue
        q, dim = mixed(prob, d)
        R = q.record_max()
        want, B, sx = q.reference()
        T = q.T(R, sx)
        sharpness(q, d, B, T, dim)
        y = run(q)
        out["mixed", d] = measure("%s bright+dim d=%d, dim elements" % (label, d), y, want, B, T, c, dim, enforce)
        measure("%s bright+dim d=%d, bright elements" % (label, d), y, want, B, T, c, ~dim, enforce)
        if second_terms and (d == 24 or (d == 18 and prob.kind == "wino")):     # (K12 scales 5 binades lower: its second terms are denormals from d = 12 on)
            alone = first_term_only(q, R)
            near = ((y.double() - want).abs() < (y.double() - alone).abs())[dim]
            assert bool((want != alone)[dim].any()) and float(near.double().mean()) > 0.5, (label, "the second terms of the dim values were dropped")
    return out


def check_ends(run, prob, label):
    """4. zero input under a zero record: bias (+ residual, ReLU) exactly; abs-max 2^-120: finite, within 2^-100 of that; abs-max 2^100 with
    the weights x 2^-20: finite, the module's bar"""
    zero = prob.with_images([torch.zeros_like(x) for x in prob.images()])
    K = prob.w.shape[0]
    pixels = run(zero).shape[0]
    alone = zero.finish(torch.zeros(pixels, K))
    assert torch.equal(run(zero), alone), label
    g = gen(11)

    def spread(top, first):
        xs = [(torch.rand(x.shape, generator=g) * 2.0 - 1.0) * top for x in prob.images()]
        xs[0][0, 0, 0, 0] = first
        return xs
    tiny = prob.with_images(spread(2.0 ** -120, 2.0 ** -120))
    assert tiny.record_max() == 2.0 ** -120
    y = run(tiny)
    assert bool(torch.isfinite(y).all()) and float((y.double() - alone.double()).abs().max()) <= 2.0 ** -100, label
    huge = prob.with_images(spread(2.0 ** 100, -2.0 ** 100)).but(w=prob.w * 2.0 ** -20, res=None)
    assert huge.record_max() == 2.0 ** 100
    want, B, _ = huge.reference()
    measure(label + " abs-max 2^100, weights x 2^-20", run(huge), want, B, 0.0, BAR[prob.kind])


def worst_gain_problem(prob, m=M_PLANT, seed=0):
    """K12: the 4 x 6 patch of tile (1, 1) of level 0, image 0 -- rows 1 .. 4, columns 3 .. 8 -- filled in every channel with
    +- nextafter(2^(m+1), 0) in the sign pattern of the worst rows of Bt4 and Bt6 (zeros of a row count as +): that position's transformed
    value is gain x max.  -> (problem, rows of the tile's outputs)"""
    ia, ib, gain = worst_rows(BT4, BT6)
    top = float(torch.nextafter(torch.tensor(2.0 ** (m + 1)), torch.tensor(0.0)))
    g = gen(seed)
    xs = [(torch.rand(x.shape, generator=g) * 2.0 - 1.0) * 2.0 ** m for x in prob.images()]
    sa = torch.tensor([-1.0 if v < 0 else 1.0 for v in BT4[ia]])
    sb = torch.tensor([-1.0 if v < 0 else 1.0 for v in BT6[ib]])
    xs[0][0, :, 1:5, 3:9] = top * sa[:, None] * sb[None, :]
    q = prob.with_images(xs)
    h, w = xs[0].shape[2:]
    rows = torch.tensor([y * w + x for y in (2, 3) for x in (4, 5, 6, 7)])
    d = xs[0][0, 0, 1:5, 3:9].double()
    v = torch.tensor(BT4[ia], dtype=torch.float64) @ d @ torch.tensor(BT6[ib], dtype=torch.float64)
    assert abs(float(v)) == gain * top and q.record_max() == top
    return q, rows


# ---- the kernels, through the wrappers the other tests use (GPU modules only) ---------------------------------------------------------------
def kernel(prob, record=None):
    """run(problem, record): exact record (amax.of) unless `record` is given -- then a hand-filled one holding it in every slot"""
    from pod_compare_amd import amax
    from pod_compare_amd.conv1x1 import Conv1x1, Conv3x3S2, Stem7x7
    from pod_compare_amd.wino import WinoConv, block_table, level_pixel_offsets

    def dev(t):
        return None if t is None else t.cuda().contiguous()

    def carry(t):
        return t if record is None else amax.attach(t, torch.full((amax.RECORD,), float(record), device="cuda"))
    o, w, b = prob.opt, dev(prob.w), dev(prob.b)
    if prob.kind == "c1":
        y = Conv1x1(w, b, o["stride"])(carry(dev(prob.x)), o["H"], o["W"], relu=prob.relu, residual=dev(prob.res), residual_up2=bool(o.get("up2")),
                                        n_splits=o["splits"], waves=o["waves"])
    elif prob.kind == "c3s2":
        y = Conv3x3S2(w, b)(carry(dev(prob.x)), o["H"], o["W"], relu=prob.relu)[0]
    elif prob.kind == "stem":
        x = dev(prob.x)
        y = Stem7x7(w, b)(x if x.dtype == torch.uint8 else carry(x), relu=prob.relu, mean=dev(o.get("mean")), std=dev(o.get("std")))[0]
    else:
        levels, copies, C, K = [tuple(x.shape[2:]) for x in prob.x], prob.x[0].shape[0], prob.w.shape[1], prob.w.shape[0]
        conv = WinoConv(w, b, split=True)
        assert conv.split
        src = carry(torch.cat([x.permute(0, 2, 3, 1).reshape(-1, C) for x in prob.x]).contiguous().cuda())
        if o.get("splits"):
            assert len(levels) == 1 and copies == 1
            y = conv.channels_last_of_one_image(src, block_table(levels, 1, "cuda"), relu=prob.relu, n_splits=o["splits"])
        elif o.get("replicas"):
            r = o["replicas"]
            y = torch.full((level_pixel_offsets(levels, r)[-1], K), float("nan"), device="cuda")
            conv.replicas(src, y, block_table(levels, 1, "cuda", out_copies=r), r, relu=prob.relu, dropout_p=o["p"], seed=77, offset=9 << 34)
        elif o.get("planes"):
            offs = level_pixel_offsets(levels, copies)
            out = torch.full((offs[-1] * K,), float("nan"), device="cuda")
            conv(src, out, block_table(levels, copies, "cuda"), relu=prob.relu, planes=True)
            y = torch.cat([out[offs[i] * K:offs[i + 1] * K].view(copies, K, h, wd).permute(0, 2, 3, 1).reshape(-1, K) for i, (h, wd) in enumerate(levels)])
        else:
            y = conv(src, torch.full((src.shape[0], K), float("nan"), device="cuda"), block_table(levels, copies, "cuda"), relu=prob.relu)
    return y.cpu()
