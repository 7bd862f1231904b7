"""GPU box: checksums of the 3x3 Winograd convolution's output -- whichever kernel WinoConv selects: pod_wino_conv3x3_split, or with
POD_WINO_SPLIT=0 pod_wino_conv3x3 -- on the bench launch, two ragged launches, an NCHW-planes launch and (split kernel) a replicas
launch, i.e. every variant of the store pass, to compare two builds of the library bit for bit across processes:
    POD_MI355X_LIB=<lib A> python tools/k12_ab.py ; POD_MI355X_LIB=<lib B> python tools/k12_ab.py"""
import hashlib
import sys

import torch

sys.path.insert(0, ".")
from pod_compare_amd.wino import WinoConv, block_table, level_pixel_offsets  # noqa: E402

dev = torch.device("cuda")


def digest(what, dst):
    torch.cuda.synchronize()
    print(what, hashlib.sha256(dst.cpu().numpy().tobytes()).hexdigest()[:16], float(dst.abs().max()))


def make(levels, copies, C, K):
    torch.manual_seed(C)
    conv = WinoConv(torch.randn(K, C, 3, 3, device=dev) * 0.03, torch.randn(K, device=dev))
    return conv, torch.randn(copies * sum(h * w for h, w in levels), C, device=dev).relu()


for levels, copies, C, K in (([(96, 168), (48, 84), (24, 42), (12, 21), (6, 11)], 3, 256, 256), ([(23, 40), (7, 9), (1, 1)], 2, 48, 64), ([(17, 33)], 1, 16, 128)):
    conv, src = make(levels, copies, C, K)
    tab = block_table(levels, copies, dev)
    dst = torch.empty(tab.pod_pixels, K, device=dev)
    conv(src, dst, tab, relu=True, dropout_p=0.1, seed=1)
    digest("split=%d channels-last C=%d K=%d copies=%d" % (conv.split, C, K, copies), dst)

levels, copies, C, K = [(23, 40), (12, 21), (7, 9)], 3, 64, 63                 # a predictor: K real channels as NCHW planes, no dropout
conv, src = make(levels, copies, C, K)
dst = torch.full((level_pixel_offsets(levels, copies)[-1] * K,), float("nan"), device=dev)
conv(src, dst, block_table(levels, copies, dev), planes=True)
digest("split=%d planes C=%d K=%d copies=%d" % (conv.split, C, K, copies), dst)

levels, replicas, C, K = [(20, 28), (12, 21), (5, 7)], 5, 32, 64              # one image per level stored 5 times, a mask each
conv, src = make(levels, 1, C, K)
if conv.split:
    dst = torch.full((level_pixel_offsets(levels, replicas)[-1], K), float("nan"), device=dev)
    conv.replicas(src, dst, block_table(levels, 1, dev, out_copies=replicas), replicas, relu=True, dropout_p=0.25, seed=77, offset=9 << 34)
    digest("split=1 replicas C=%d K=%d replicas=%d" % (C, K, replicas), dst)
