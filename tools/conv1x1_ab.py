"""GPU box: sha-256 of what the split-GEMM family (k13_conv1x1_split.hip, k14_stem_conv.hip) writes on seeded inputs -- the output and the
abs-max record the launch publishes for it: run it with two builds of the library (POD_MI355X_LIB=...) to compare them bit for bit across
processes.  Covers every kernel form: the LDS kernel with 1 / 2 / 4 wavefronts (forced and chosen), the direct-fragment kernel (an odd
number of k-steps per split: the 3x3 / stride 2 convolution of p7), grid.y splits + reduce, stride 2, ragged pixel counts, full- and
half-resolution residuals, ReLU, Cin = 16 / 48, the stem on fp32 and on uint8 frames, the max-pool."""
import hashlib
import sys
import torch
sys.path.insert(0, ".")
from pod_compare_amd import amax  # noqa: E402
from pod_compare_amd.conv1x1 import Conv1x1, Conv3x3S2, Stem7x7, maxpool3x3s2_cl  # noqa: E402


def digest(y):
    h = hashlib.sha256(y.cpu().numpy().tobytes())
    h.update(amax.of(y).cpu().numpy().tobytes())
    return h.hexdigest()[:24]


def gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


# (Cin, Cout, h, w, stride, residual: None / "full" / "up2", relu, n_splits (None: splits_for), waves (0: the library's choice))
SHAPES = ((256, 1024, 48, 84, 1, "full", False, 1, 0), (64, 256, 192, 336, 1, "full", False, 1, 0), (1024, 256, 48, 84, 1, None, False, 4, 0),
          (512, 1024, 96, 168, 2, None, False, 1, 0), (2048, 256, 24, 42, 1, "full", False, 16, 0), (96, 128, 37, 53, 2, "full", False, 1, 0),
          (64, 64, 5, 7, 1, None, False, 2, 0),
          (512, 256, 47, 83, 1, "up2", True, 1, 0),                                               # FPN's top-down sum, odd map
          (1024, 256, 24, 42, 1, None, True, 1, 1), (1024, 256, 24, 42, 1, None, True, 1, 2), (1024, 256, 24, 42, 1, None, True, 1, 4),
          (16, 64, 33, 17, 1, None, True, 1, 0), (48, 128, 33, 17, 1, "full", False, 1, 0))        # one k-step; three (the direct-fragment kernel)
for cin, cout, h, w, s, res, relu, splits, waves in SHAPES:
    g = gen(cin * 31 + cout)
    wt = torch.randn(cout, cin, 1, 1, device="cuda", generator=g) * 0.05
    b = torch.randn(cout, device="cuda", generator=g)
    x = torch.randn(h * w, cin, device="cuda", generator=g)
    conv = Conv1x1(wt, b, s)
    ho, wo = conv.out_hw(h, w)
    r = None
    if res == "full":
        r = torch.randn(ho * wo, cout, device="cuda", generator=g)
    elif res == "up2":
        r = torch.randn(((ho + 1) // 2) * ((wo + 1) // 2), cout, device="cuda", generator=g)
    y = conv(x, h, w, relu=relu, residual=r, n_splits=splits, waves=waves, residual_up2=res == "up2")
    print("%4d -> %4d %3dx%3d s%d res %-4s relu %d splits %2d waves %d: %s" % (cin, cout, ho, wo, s, res, relu, splits, waves, digest(y)))

# p7: 9 k-steps per split -- the direct-fragment kernel, behind pod_im2col3x3s2_cl with relu_input
g = gen(7)
conv = Conv3x3S2(torch.randn(256, 256, 3, 3, device="cuda", generator=g) * 0.02, torch.randn(256, device="cuda", generator=g))
x = torch.randn(12 * 21, 256, device="cuda", generator=g)
y, ho, wo = conv(x, 12, 21, relu_input=True)
print("Conv3x3S2 256 -> 256 %dx%d relu_input, %d splits: %s" % (ho, wo, conv.gemm.splits_for(ho * wo), digest(y)))

g = gen(14)
stem = Stem7x7(torch.randn(64, 3, 7, 7, device="cuda", generator=g) * 0.1, torch.randn(64, device="cuda", generator=g))
y, ho, wo = stem(torch.randn(1, 3, 96, 168, device="cuda", generator=g))
print("Stem7x7 fp32 96x168 -> %dx%d: %s" % (ho, wo, digest(y)))
frame = torch.randint(0, 256, (3, 75, 101), device="cuda", generator=g, dtype=torch.uint8)
mean, std = torch.tensor([103.53, 116.28, 123.675], device="cuda"), torch.tensor([57.375, 57.12, 58.395], device="cuda")
y, ho, wo = stem(frame, mean=mean, std=std, padded_hw=(96, 128))
print("Stem7x7 uint8 75x101 in 96x128 -> %dx%d: %s" % (ho, wo, digest(y)))
p, hp, wp = maxpool3x3s2_cl(y, ho, wo)
print("maxpool3x3s2_cl %dx%d -> %dx%d: %s" % (ho, wo, hp, wp, digest(p)))
