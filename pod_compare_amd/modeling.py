"""ResNet-50-FPN + probabilistic RetinaNet head on PyTorch-ROCm (row a1 of SURVEY 8a).

The reference model (probabilistic_modeling/probabilistic_retinanet.py) subclasses detectron2's
RetinaNet, which is not installed; this is a from-scratch statement of the same architecture in
plain torch.  On the GPU its convolutions run on the hand-written HIP kernels (pod_stem7x7_split, pod_conv1x1_split, pod_wino_conv3x3[_split]:
the switches below); MIOpen and the NCHW paths remain for CPU tensors and as the tests' references:

  backbone  detectron2 `build_retinanet_resnet_fpn_backbone`: ResNet-50 (FrozenBN, stride in the
            1x1 conv of each bottleneck), FPN on res3..res5 (256 ch) + LastLevelP6P7 from res5
            (Base-RetinaNet.yaml:3-10).
  head      ProbabilisticRetinaNetHead, PR:370-537: two 4 x (conv3x3 256->256, ReLU, Dropout p)
            subnets; cls_score 256->A*K (bias -log(99), PR:454-455), bbox_pred 256->A*4,
            cls_var 256->A*K (bias -10, PR:458-470), bbox_cov 256->A*D (std 1e-4, PR:473-484).

MI355X-first differences from the reference's forward (PR:95-108, PR:486-537), numerically neutral:
  * MC-dropout runs are batched along the batch dimension instead of replicating python lists of
    feature maps N times (PR:104-106); outputs stay NCHW `(N, A*C, H, W)` -- exactly the layout
    kernel K1 streams -- so `permute_to_N_HWA_K` (PR:343-349) never runs;
  * the first conv+ReLU of each subnet sees the same input in every run (dropout only follows it),
    so it is evaluated once and broadcast;
  * in MC mode the mean and variance branches still use independent dropout draws (SURVEY Q2:
    the reference evaluates each subnet twice, PR:518-523); without dropout the two evaluations are
    identical and the trunk is shared (SURVEY f-4);
  * dropout is enabled by a flag instead of `model.train()` (PI:53-56).
"""
import math
import os
from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple

import torch
import torch.nn.functional as F
from torch import nn

from . import amax, conv1x1, hip, sparse, wino          # (modules, called through: bench.py and the tests replace wino.grouped_launch, wino.block_table, ... on them)
from . import anchors as _anchors
from . import losses as _losses
from .conv_forms import c1_of, s2_of, stem_of, wino_of   # (wino_of: tests and tools reach it as modeling.wino_of)
from .synthetic import HeadOutputs

PIXEL_MEAN_BGR = (103.530, 116.280, 123.675)   # detectron2 defaults used by the BDD configs
PIXEL_STD = (1.0, 1.0, 1.0)


class FrozenBatchNorm2d(nn.Module):
    """BatchNorm with fixed statistics and affine terms (detectron2 FrozenBatchNorm2d)."""

    def __init__(self, num_features: int, eps: float = 1e-5):
        super().__init__()
        self.eps = eps
        self.register_buffer("weight", torch.ones(num_features))
        self.register_buffer("bias", torch.zeros(num_features))
        self.register_buffer("running_mean", torch.zeros(num_features))
        self.register_buffer("running_var", torch.ones(num_features) - eps)

    def forward(self, x):
        scale = self.weight * (self.running_var + self.eps).rsqrt()
        shift = self.bias - self.running_mean * scale
        return x * scale.reshape(1, -1, 1, 1) + shift.reshape(1, -1, 1, 1)


def fold_frozen_bn(module: nn.Module) -> int:
    """Folds every `Sequential(Conv2d(bias=False), FrozenBatchNorm2d)` pair into one biased conv (w * scale, shift):
    the same affine map without ~100 tiny element-wise launches per image in the batch-1 backbone.  Returns the number
    of pairs folded.  Inference only (the statistics are frozen by definition)."""
    n = 0
    for child in module.children():
        if isinstance(child, nn.Sequential) and len(child) == 2 and isinstance(child[0], nn.Conv2d) and \
                isinstance(child[1], FrozenBatchNorm2d) and child[0].bias is None:
            conv, bn = child[0], child[1]
            scale = bn.weight * (bn.running_var + bn.eps).rsqrt()
            shift = bn.bias - bn.running_mean * scale
            with torch.no_grad():
                conv.weight.mul_(scale.reshape(-1, 1, 1, 1))
                conv.bias = nn.Parameter(shift.clone(), requires_grad=False)
            child[1] = nn.Identity()
            n += 1
        else:
            n += fold_frozen_bn(child)
    if n:                                                       # (a model serving HIP graphs: they were captured against the unfolded filters)
        bump_param_generation()
    return n


# Anything that replaces or moves parameter STORAGE without bumping a tensor's version counter -- nn.Module._apply on the model or on ANY of
# its submodules (model.head.to(...), model.bottom_up.float()), load_state_dict, fold_frozen_bn on a part of the model -- moves this
# process-wide counter on; every model's graph fingerprint contains it, so graphs captured against the old storage are dropped (ADVICE r5:
# a counter on the root module alone missed the submodule cases).
_PARAM_GENERATION = [0]


def bump_param_generation() -> None:
    _PARAM_GENERATION[0] += 1


class _TracksStorage(nn.Module):
    """nn.Module whose `_apply` (to / cuda / float / ...) is seen by the graph fingerprints."""

    def _apply(self, fn, *a, **kw):
        out = super()._apply(fn, *a, **kw)
        bump_param_generation()
        return out


def _plain_conv(m) -> Optional[nn.Conv2d]:
    """The biased conv behind `m` if its element-wise tail can be fused: a Conv2d, or a folded (conv, Identity) pair."""
    if isinstance(m, nn.Sequential) and len(m) == 2 and isinstance(m[0], nn.Conv2d) and isinstance(m[1], nn.Identity):
        m = m[0]
    return m if isinstance(m, nn.Conv2d) else None


FUSE_CONV_TAIL = True     # GPU only: conv without bias + ONE pod_bias_act pass (bias, residual, ReLU, dropout)


def conv_bias_act(m, x: torch.Tensor, relu: bool = False, residual: Optional[torch.Tensor] = None, residual_module=None,
                  residual_input: Optional[torch.Tensor] = None, dropout_p: float = 0.0, seed: int = 0, offset: int = 0,
                  out_nchw: bool = False, residual_raw: Optional[torch.Tensor] = None) -> torch.Tensor:
    """act(m(x) [+ residual]) with the element-wise tail in one HIP pass.

    torch's conv on ROCm is MIOpen's kernel plus a separate bias `add_`; followed by clamp (and the bottleneck's add, and
    dropout) that is 2-4 read+write passes over the activation.  Here the conv runs without its bias and pod_bias_act does
    `dropout(relu((y + b[c]) + (r + rb[c])))` in place.  `residual_module(residual_input)` (a shortcut conv) is evaluated without
    its bias too and folded into the same pass.  CPU tensors / unfolded BN / non-fp32 take the plain torch ops."""
    conv = _plain_conv(m)
    rconv = _plain_conv(residual_module) if residual_module is not None else None
    fuse = (FUSE_CONV_TAIL and conv is not None and x.is_cuda and x.dtype == torch.float32 and
            (residual_module is None or rconv is not None))
    if not fuse:
        y = m(x)
        if residual_module is not None:
            residual = residual_module(residual_input)
        if residual is not None:
            y = y + residual
        if relu:
            y = F.relu_(y)
        return F.dropout(y, dropout_p, training=True) if dropout_p > 0.0 else y
    lib = hip.load()
    nhwc = x.dim() == 4 and x.shape[1] > 1 and x.is_contiguous(memory_format=torch.channels_last) and not x.is_contiguous()
    y = F.conv2d(x, _weight_for(conv, nhwc), None, conv.stride, conv.padding, conv.dilation, conv.groups)
    res_bias = None
    if rconv is not None:
        residual = residual_raw if residual_raw is not None else shortcut_raw(rconv, residual_input)
        res_bias = rconv.bias
    C, HW = y.shape[1], y.shape[2] * y.shape[3]
    if nhwc and residual is None and y.is_contiguous(memory_format=torch.channels_last):
        if out_nchw and C % 4 == 0 and HW % 4 == 0:
            # leave the channels-last trunk on the element-wise pass that exists anyway: NHWC in, NCHW planes out
            out = torch.empty(y.shape, dtype=y.dtype, device=y.device)
            hip.check(lib.pod_bias_act_to_nchw(y.data_ptr(), out.data_ptr(), hip.ptr(conv.bias), y.shape[0], C, HW, 1 if relu else 0,
                                               float(dropout_p), seed, offset, hip.current_stream()), "pod_bias_act_to_nchw")
            return out
        HW = 1                                  # NHWC: channel = flat index mod C (include/pod_mi355x.h)
    else:
        if not y.is_contiguous():
            y = y.contiguous()
        if residual is not None:
            assert residual.shape == y.shape
            residual = residual.contiguous()
    hip.check(lib.pod_bias_act(y.data_ptr(), hip.ptr(conv.bias), hip.ptr(residual), hip.ptr(res_bias), y.numel(), C, HW,
                               1 if relu else 0, float(dropout_p), seed, offset, hip.current_stream()), "pod_bias_act")
    return y


def shortcut_raw(rconv: nn.Conv2d, x: torch.Tensor) -> torch.Tensor:
    """A shortcut conv without its bias (the bias rides on the pass that adds the residual)."""
    return F.conv2d(x, rconv.weight, None, rconv.stride, rconv.padding, rconv.dilation, rconv.groups)


def _weight_for(conv: nn.Conv2d, channels_last: bool) -> torch.Tensor:
    """conv.weight, or a cached channels-last copy of it (refreshed when the parameter is modified or moved)."""
    w = conv.weight
    if not channels_last:
        return w
    key = (w.data_ptr(), w._version)
    cached = getattr(conv, "_pod_w_nhwc", None)
    if cached is None or cached[0] != key:
        cached = (key, w.detach().contiguous(memory_format=torch.channels_last))
        if w.is_cuda:
            torch.cuda.current_stream(w.device).synchronize()   # made once, then read from any stream
        conv._pod_w_nhwc = cached
    return cached[1]


WINO_HEAD = True              # GPU only: the head subnets' 3x3 convs on pod_wino_conv3x3 (all levels, all runs per launch)
WINO_BACKBONE = os.environ.get("POD_WINO_BACKBONE", "1") != "0"   # GPU only: the bottlenecks' and the FPN's 3x3 / stride-1 convs on pod_wino_conv3x3 too (batch 1: few
                              # workgroups per launch, but a third of MIOpen's CU-time per FLOP -- the other streams' images fill the idle CUs)
NHWC_TRUNK_MIN_CELLS = 8192   # head trunks of maps at least this large run channels-last (p3 of a 768x1344 input: 16128)


def wino_eligible(conv: Optional[nn.Conv2d], x: torch.Tensor) -> bool:
    """pod_wino_conv3x3 can stand in for `conv` on x: 3x3 / stride 1 / pad 1, fp32 on the GPU, one image, channel counts it tiles."""
    return (WINO_BACKBONE and FUSE_CONV_TAIL and wino.WinoConv.eligible(conv) and x.is_cuda and x.dtype == torch.float32 and x.dim() == 4
            and x.shape[0] == 1
            and conv.in_channels % 8 == 0                       # either kernel may serve an NCHW map: the fp32-MFMA kernel's channel step
            and conv.out_channels in (64, 128, 256, 512)        # the backbone's and the FPN's own widths, none padded
            and x.shape[2] < 4096 and x.shape[3] < 4096
            and x.shape[2] * x.shape[3] * max(conv.in_channels, conv.out_channels) * 4 <= wino.MAX_CANVAS_BYTES)      # 32-bit offsets inside a canvas


def wino_conv_nchw(conv: nn.Conv2d, x: torch.Tensor, relu: bool, pre_bias: Optional[torch.Tensor] = None, pre_relu: bool = False) -> torch.Tensor:
    """act(conv(pre_act(x + pre_bias))) for an NCHW x (1, C, H, W): the element-wise tail of the PRODUCER of x (bias + ReLU of the conv
    before) rides on the pass that lays x out channels-last (pod_bias_act_to_nhwc), the 3x3 conv runs on pod_wino_conv3x3 with its own
    bias + ReLU in the store, and the result comes back as NCHW planes."""
    _, C, H, W = x.shape
    a = torch.empty((H * W, C), dtype=x.dtype, device=x.device)
    hip.check(hip.load().pod_bias_act_to_nhwc(x.contiguous().data_ptr(), a.data_ptr(), hip.ptr(pre_bias), 1, C, H * W, 1 if pre_relu else 0,
                                              hip.current_stream()), "pod_bias_act_to_nhwc")
    out = torch.empty((1, conv.out_channels, H, W), dtype=x.dtype, device=x.device)
    wino_of(conv).planes_of_one_image(a, out.view(-1), wino.block_table([(H, W)], 1, x.device), relu=relu)     # (small maps: split over C)
    return out


# ---- channels-last backbone (round 4) ---------------------------------------------------------------------------------------
# With the 3x3 convolutions on pod_wino_conv3x3[_split] (channels-last in and out) the 1x1 convolutions were what kept the backbone in
# NCHW: MIOpen GEMM + one element-wise pass each for bias / residual / ReLU, plus a layout pass in front of every 3x3.  On
# pod_conv1x1_split (csrc/k13_conv1x1_split.hip: channels-last GEMM, bias + residual + ReLU in the store, same exact-split products as
# the 3x3 kernel) a bottleneck is three launches on (pixels, C) buffers and the whole trunk stays channels-last from the max-pool on.
GROUPED_HEAD = os.environ.get("POD_GROUPED_HEAD", "1") != "0"         # layer l of the cls and the bbox subnet, and the four predictors, in one launch each
CL_BACKBONE = os.environ.get("POD_CL_BACKBONE", "1") != "0"
HIP_P6P7 = os.environ.get("POD_HIP_P6P7", "1") != "0"         # FPN's p6 / p7 (3x3 / stride 2) as pod_im2col3x3s2_cl + pod_conv1x1_split instead of MIOpen
HIP_STEM = os.environ.get("POD_HIP_STEM", "1") != "0"         # the 7x7 stem + max-pool of the channels-last trunk on pod_stem7x7_split / pod_maxpool3x3s2_cl


def kernel_selection() -> tuple:
    """Every switch that selects the kernels of a forward (part of the HIP-graph key: a graph captured under one selection must not answer for another)."""
    return (WINO_HEAD, WINO_BACKBONE, GROUPED_HEAD, CL_BACKBONE, HIP_STEM, HIP_P6P7, FUSE_CONV_TAIL, NHWC_TRUNK_MIN_CELLS, bool(wino.SPLIT_BF16))


def _c1_ok(conv: Optional[nn.Conv2d]) -> bool:
    return conv is not None and conv.bias is not None and conv1x1.Conv1x1.eligible(conv)


def _w3_ok(conv: Optional[nn.Conv2d]) -> bool:
    return (wino.WinoConv.eligible(conv) and conv.bias is not None
            and conv.in_channels % 16 == 0                      # the split kernel: the one the channels-last trunk chains with pod_conv1x1_split
            and conv.out_channels in (64, 128, 256, 512))       # channels-last output has no padded channels (K == Kpad)


def wino_cl(conv: nn.Conv2d, x: torch.Tensor, h: int, w: int, relu: bool, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """act(conv3x3(x) + bias) of one channels-last image (h * w, C) -> (h * w, K)."""
    return wino_of(conv).channels_last_of_one_image(x, wino.block_table([(h, w)], 1, x.device, channels=max(conv.in_channels, conv.out_channels)), relu=relu, out=out)


def levels_channels_last(features: List[torch.Tensor]) -> torch.Tensor:
    """The FPN levels as ONE channels-last buffer, level after level (what the head's grouped launches read): the buffer FPN.forward_cl wrote
    them into when they still are its consecutive slices (no copy), else their concatenation."""
    buf = getattr(features[0], "_pod_cl_levels", None)
    if buf is not None and buf.shape[0] == sum(int(f.shape[2]) * int(f.shape[3]) for f in features) and buf._version == features[0]._pod_cl_version:
        at, ok = buf.data_ptr(), True
        for f in features:
            ok = ok and f.shape[0] == 1 and f.shape[1] == buf.shape[1] and f.data_ptr() == at and f.stride(1) == 1
            at += int(f.shape[2]) * int(f.shape[3]) * int(buf.shape[1]) * 4
        if ok:
            return buf
    return torch.cat([f.permute(0, 2, 3, 1).reshape(-1, f.shape[1]) for f in features])


def cl_as_nchw(x: torch.Tensor, h: int, w: int) -> torch.Tensor:
    """(h * w, C) channels-last buffer as a (1, C, h, w) tensor (channels_last strides: a view)."""
    return x.view(1, h, w, x.shape[1]).permute(0, 3, 1, 2)


def nchw_as_cl(x: torch.Tensor) -> torch.Tensor:
    """(1, C, h, w) tensor of either memory format as an (h * w, C) channels-last buffer (a view when it already is channels-last)."""
    return x.permute(0, 2, 3, 1).reshape(-1, x.shape[1]).contiguous()


def _conv_bn(cin, cout, k, stride=1, padding=0):
    conv = nn.Conv2d(cin, cout, k, stride=stride, padding=padding, bias=False)
    nn.init.kaiming_normal_(conv.weight, mode="fan_out", nonlinearity="relu")   # c2_msra_fill
    return nn.Sequential(conv, FrozenBatchNorm2d(cout))


class Bottleneck(_TracksStorage):
    def __init__(self, cin, cout, mid, stride):
        super().__init__()
        self.shortcut = _conv_bn(cin, cout, 1, stride) if cin != cout else None
        self.conv1 = _conv_bn(cin, mid, 1, stride)          # STRIDE_IN_1X1 = True (MSRA R-50)
        self.conv2 = _conv_bn(mid, mid, 3, 1, 1)
        self.conv3 = _conv_bn(mid, cout, 1)

    def forward(self, x):
        c1, c2 = _plain_conv(self.conv1), _plain_conv(self.conv2)

        def main():
            if c1 is not None and c1.bias is not None and c2 is not None and c2.bias is not None and wino_eligible(c2, x):
                y = F.conv2d(x, c1.weight, None, c1.stride, c1.padding)                   # conv1 without its bias (MIOpen, NCHW)
                return wino_conv_nchw(c2, y, relu=True, pre_bias=c1.bias, pre_relu=True)  # its bias + ReLU, then conv2 + bias + ReLU
            return conv_bias_act(self.conv2, conv_bias_act(self.conv1, x, relu=True), relu=True)

        if self.shortcut is None:
            return conv_bias_act(self.conv3, main(), relu=True, residual=x)
        rconv = _plain_conv(self.shortcut)
        if rconv is None or rconv.bias is None or not (FUSE_CONV_TAIL and x.is_cuda and x.dtype == torch.float32):
            return conv_bias_act(self.conv3, main(), relu=True, residual_module=self.shortcut, residual_input=x)
        out = main()
        raw = shortcut_raw(rconv, x)
        return conv_bias_act(self.conv3, out, relu=True, residual_module=self.shortcut, residual_input=x, residual_raw=raw)


    def cl_eligible(self) -> bool:
        convs = (_plain_conv(self.conv1), _plain_conv(self.conv2), _plain_conv(self.conv3))
        sc = None if self.shortcut is None else _plain_conv(self.shortcut)
        return _c1_ok(convs[0]) and _w3_ok(convs[1]) and _c1_ok(convs[2]) and (self.shortcut is None or _c1_ok(sc))

    def forward_cl(self, x: torch.Tensor, h: int, w: int, keep: Optional[dict] = None):
        """The block on a channels-last buffer x (h * w, Cin): conv1 (1x1, stride) -> conv2 (3x3) -> conv3 (1x1) + shortcut + ReLU, three
        (four) launches, every bias / ReLU / residual in the producing kernel's store.  Returns (y, h_out, w_out).  keep: a dict that receives
        what a backward pass needs of this forward (resnet_train.py): the input x, conv1's and conv2's outputs a and b, the output y."""
        c1, c2, c3 = c1_of(_plain_conv(self.conv1)), _plain_conv(self.conv2), c1_of(_plain_conv(self.conv3))
        h1, w1 = c1.out_hw(h, w)
        a = c1(x, h, w, relu=True)
        b = wino_cl(c2, a, h1, w1, relu=True)
        r = x if self.shortcut is None else c1_of(_plain_conv(self.shortcut))(x, h, w, relu=False)
        y = c3(b, h1, w1, relu=True, residual=r)
        if keep is not None:
            keep.update(x=x, a=a, b=b, y=y, hw_in=(h, w), hw=(h1, w1))
        return y, h1, w1


class ResNet50(_TracksStorage):
    """res2..res5 of ResNet-50; returns res3, res4, res5 (strides 8, 16, 32)."""

    def __init__(self):
        super().__init__()
        self.stem = _conv_bn(3, 64, 7, 2, 3)
        cfg = ((3, 64, 256, 1), (4, 128, 512, 2), (6, 256, 1024, 2), (3, 512, 2048, 2))
        stages, cin = [], 64
        for blocks, mid, cout, stride in cfg:
            layers = []
            for b in range(blocks):
                layers.append(Bottleneck(cin, cout, mid, stride if b == 0 else 1))
                cin = cout
            stages.append(nn.Sequential(*layers))
        self.res2, self.res3, self.res4, self.res5 = stages

    def forward(self, x):
        x = conv_bias_act(self.stem, x, relu=True)
        x = F.max_pool2d(x, kernel_size=3, stride=2, padding=1)
        x = self.res2(x)
        c3 = self.res3(x)
        c4 = self.res4(c3)
        c5 = self.res5(c4)
        return c3, c4, c5

    def cl_eligible(self) -> bool:
        return all(b.cl_eligible() for stage in (self.res2, self.res3, self.res4, self.res5) for b in stage)

    def hip_stem_ok(self) -> bool:
        stem = _plain_conv(self.stem)
        return HIP_STEM and stem is not None and stem.bias is not None and conv1x1.Stem7x7.eligible(stem)

    def forward_cl(self, x, frame=None, stop_after_res2: bool = False, res2=None):
        """Channels-last from the stem on: returns [(c3, h, w), (c4, h, w), (c5, h, w)] with c* (h * w, C) buffers.  frame = (image (3, h, w)
        uint8 / fp32 on the device, pixel mean, pixel std, padded (h, w)) instead of x: the stem kernel normalises and pads on load.
        The two halves a trainer of res3 - res5 runs apart (resnet_train.py): stop_after_res2 returns res2's (t, h, w) -- the part
        detectron2 freezes; res2 = that triple runs res3 - res5 on it instead of a frame."""
        if res2 is not None:
            t, h, w = res2
            outs = []
            for stage in (self.res3, self.res4, self.res5):
                for block in stage:
                    t, h, w = block.forward_cl(t, h, w)
                outs.append((t, h, w))
            return outs
        stem = _plain_conv(self.stem)
        if frame is not None:
            img, mean, std, padded = frame
            t, h, w = stem_of(stem)(img, relu=True, mean=mean, std=std, padded_hw=padded)
            t, h, w = conv1x1.maxpool3x3s2_cl(t, h, w)
        elif self.hip_stem_ok() and x.shape[0] == 1 and x.is_contiguous():
            t, h, w = stem_of(stem)(x, relu=True)                        # 7x7 / stride 2 on pod_stem7x7_split: channels-last out
            t, h, w = conv1x1.maxpool3x3s2_cl(t, h, w)
        else:
            x = conv_bias_act(self.stem, x, relu=True)                   # MIOpen, NCHW
            x = F.max_pool2d(x, kernel_size=3, stride=2, padding=1)
            h, w = int(x.shape[2]), int(x.shape[3])
            t = nchw_as_cl(x)
        outs = []
        for stage in (self.res2, self.res3, self.res4, self.res5):
            for block in stage:
                t, h, w = block.forward_cl(t, h, w)
            outs.append((t, h, w))
            if stop_after_res2:
                return outs[0]
        return outs[1:]


class FPN(_TracksStorage):
    """detectron2 FPN (sum fusion, no norm) on res3..res5 + LastLevelP6P7(in_feature='res5')."""

    def __init__(self, in_channels=(512, 1024, 2048), out_channels=256):
        super().__init__()
        self.lateral = nn.ModuleList(nn.Conv2d(c, out_channels, 1) for c in in_channels)
        self.output = nn.ModuleList(nn.Conv2d(out_channels, out_channels, 3, padding=1) for _ in in_channels)
        self.p6 = nn.Conv2d(in_channels[-1], out_channels, 3, stride=2, padding=1)
        self.p7 = nn.Conv2d(out_channels, out_channels, 3, stride=2, padding=1)
        for m in list(self.lateral) + list(self.output) + [self.p6, self.p7]:
            nn.init.kaiming_uniform_(m.weight, a=1)      # c2_xavier_fill
            nn.init.constant_(m.bias, 0)

    def forward(self, feats):
        c3, c4, c5 = feats
        l5 = self.lateral[2](c5)
        l4 = self.lateral[1](c4) + F.interpolate(l5, size=c4.shape[-2:], mode="nearest")
        l3 = self.lateral[0](c3) + F.interpolate(l4, size=c3.shape[-2:], mode="nearest")
        out = lambda m, l: wino_conv_nchw(m, l, relu=False) if wino_eligible(m, l) else m(l)
        p3, p4, p5 = out(self.output[0], l3), out(self.output[1], l4), out(self.output[2], l5)
        p6 = self.p6(c5)
        return [p3, p4, p5, p6, self.p7(F.relu(p6))]

    def cl_eligible(self) -> bool:
        return all(_c1_ok(m) for m in self.lateral) and all(_w3_ok(m) for m in self.output)

    def forward_cl(self, feats, keep: Optional[dict] = None):
        """feats: [(c3, h, w), (c4, h, w), (c5, h, w)] channels-last buffers.  Lateral 1x1 convs on pod_conv1x1_split, top-down sums on
        channels-last views, output 3x3 convs on pod_wino_conv3x3[_split]; p6 / p7 (stride-2 3x3) as a patch matrix on pod_conv1x1_split (round 5; POD_HIP_P6P7=0: MIOpen on channels_last views).
        Returns (1, 256, h, w) tensors with channels_last strides: the head lays them out channels-last anyway.  keep: a dict that receives
        what a backward pass needs of this forward (fpn_train.py): the summed laterals l3, l4, l5 and whether the one-buffer path ran."""
        (c3, h3, w3), (c4, h4, w4), (c5, h5, w5) = feats
        l5 = c1_of(self.lateral[2])(c5, h5, w5)
        def lateral(conv, c, h, w, top, ht, wt):               # lateral + nearest-upsampled top-down map in one store
            if (ht, wt) == ((h + 1) // 2, (w + 1) // 2):      # a factor of two (every ResNet stage): read at (y >> 1, x >> 1), never materialised
                return c1_of(conv)(c, h, w, residual=top, residual_up2=True)
            return c1_of(conv)(c, h, w, residual=nchw_as_cl(F.interpolate(cl_as_nchw(top, ht, wt), size=(h, w), mode="nearest")))
        l4 = lateral(self.lateral[1], c4, h4, w4, l5, h5, w5)
        l3 = lateral(self.lateral[0], c3, h3, w3, l4, h4, w4)
        if keep is not None:
            keep.update(l3=l3, l4=l4, l5=l5, hip_p6p7=False)
        S2 = conv1x1.Conv3x3S2
        one_buffer = HIP_P6P7 and S2.eligible(self.p6) and S2.eligible(self.p7) and self.output[0].out_channels == self.p6.out_channels == self.p7.out_channels
        hw, parts = [(h3, w3), (h4, w4), (h5, w5)], [None] * 3
        if one_buffer:
            # the five levels go straight into ONE buffer, level after level -- the layout the head's grouped launches read (no concatenation
            # in front of the head) -- and max their abs-max into one record (the head's `in_amax`)
            hw.append(S2.out_hw(h5, w5))
            hw.append(S2.out_hw(*hw[3]))
            buf = torch.empty((sum(h * w for h, w in hw), self.p6.out_channels), dtype=torch.float32, device=c5.device)
            rec, parts, at = amax.word(buf.device), [], 0
            for h, w in hw:
                parts.append(buf[at:at + h * w])
                parts[-1]._pod_amax_shared = rec             # (amax.produced: the launch that writes this slice max'es into the shared record)
                at += h * w
        p345 = [wino_cl(conv, l, h, w, relu=False, out=out) for conv, l, (h, w), out in zip(self.output, (l3, l4, l5), hw, parts)]
        if not one_buffer:
            p6 = self.p6(cl_as_nchw(c5, h5, w5))
            return [cl_as_nchw(t, h, w) for t, (h, w) in zip(p345, hw)] + [p6, self.p7(F.relu(p6))]
        s2_of(self.p6)(c5, h5, w5, out=parts[3])
        s2_of(self.p7)(parts[3], *hw[3], relu_input=True, out=parts[4])
        amax.attach(buf, rec)
        outs = [cl_as_nchw(t, h, w) for t, (h, w) in zip(parts, hw)]
        outs[0]._pod_cl_levels, outs[0]._pod_cl_version = buf, buf._version
        if keep is not None:
            keep["hip_p6p7"] = True
        return outs


@dataclass(eq=False)
class HeadPlan:
    """What one evaluation of the head carries from `_plan` to its launches and on to the model: every field, who sets it, its default.
    Inference form: `ProbabilisticRetinaNetHead._plan` (images = 0).  Training form: head_train.py builds HeadPlan(x0, levels, dropout =
    False, grouped = True, images = B, channels) and leaves the run fields at their defaults."""
    n: int = 1                      # _plan: MC runs
    m: int = 1                      # _plan: the runs whose cls / cls_var / reg_var are needed, n - skip
    skip: int = 0                   # _plan: 1 when the last run's unused evaluations are left out
    dropout: bool = False           # _plan: MC dropout is active (mc_dropout and p > 0)
    cls_copies: int = 1             # _plan: evaluations of the cls trunk
    box_copies: int = 1             # _plan: evaluations of the bbox trunk
    wino: bool = False              # _plan: every conv of the head takes pod_wino_conv3x3[_split]; the four below are set only then
    grouped: bool = False           # _plan (`_grouped_ok`) / head_train: one grid per layer of both subnets, one for the predictors
    levels: Optional[list] = None   # _plan / head_train: (h, w) per FPN level
    x0: Optional[torch.Tensor] = None    # _plan / head_train: the features as (pixels of all levels, C) channels-last, level after level
    images: int = 0                 # head_train: B images per level, every layer's output kept; 0 = the inference form
    channels: int = 512             # head_train: the channel count that bounds the block tables' canvases
    saved: Optional[list] = None    # _trunks, when `images` is set: saved[subnet][layer] = (input, output)
    logits: Optional[list] = None        # forward_cls: cls_score's planes per level
    logit_vars: Optional[list] = None    # forward_cls: cls_var's, or None
    padded: Optional[tuple] = None       # ProbabilisticRetinaNet._cls_eager: the padded frame's (h, w)
    image_hw: Optional[tuple] = None     # ProbabilisticRetinaNet._cls_eager: the frame's (h, w)
    shapes: Optional[list] = None        # ProbabilisticRetinaNet._cls_eager: (h, w) per FPN level


class ProbabilisticRetinaNetHead(_TracksStorage):
    """PR:365-537."""

    def __init__(self, in_channels=256, num_anchors=9, num_classes=7, num_convs=4, prior_prob=0.01,
                 dropout_rate=0.0, compute_cls_var=False, compute_bbox_cov=False, bbox_cov_dims=4):
        super().__init__()
        self.num_anchors, self.num_classes = num_anchors, num_classes
        self.dropout_rate = float(dropout_rate)
        self.fused_relu_dropout = True      # GPU only; falls back to torch ops on CPU tensors
        self.dropout_seed = 0x0D50ED
        self._drop_calls = 0                # distinct Philox counter block per call
        # parity mode (the head's analogue of the hot path's eps replay): a callable (subnet 0 = cls / 1 = bbox, layer, level,
        # copy) -> bool keep-mask (C, H, W) that replaces the Philox dropout masks, so that a head evaluation can be held to
        # the reference's `nn.Dropout` on recorded masks (tests/test_head_reference*.py); None in production
        self.dropout_replay = None
        # device word folded into the Philox key of every dropout mask of the Winograd head path (include/pod_mi355x.h: `epoch`): a
        # forward replayed from a HIP graph bumps it (the launch arguments seed / offset are constants of a captured launch)
        self.register_buffer("_epoch", torch.zeros(1, dtype=torch.int64), persistent=False)
        self._sparse_pool = {}
        self.compute_cls_var, self.compute_bbox_cov, self.bbox_cov_dims = compute_cls_var, compute_bbox_cov, bbox_cov_dims
        self.cls_subnet = nn.ModuleList(nn.Conv2d(in_channels, in_channels, 3, padding=1) for _ in range(num_convs))
        self.bbox_subnet = nn.ModuleList(nn.Conv2d(in_channels, in_channels, 3, padding=1) for _ in range(num_convs))
        self.cls_score = nn.Conv2d(in_channels, num_anchors * num_classes, 3, padding=1)
        self.bbox_pred = nn.Conv2d(in_channels, num_anchors * 4, 3, padding=1)
        for m in list(self.cls_subnet) + list(self.bbox_subnet) + [self.cls_score, self.bbox_pred]:
            nn.init.normal_(m.weight, mean=0, std=0.01)
            nn.init.constant_(m.bias, 0)
        nn.init.constant_(self.cls_score.bias, -math.log((1 - prior_prob) / prior_prob))      # PR:454-455
        self.cls_var = self.bbox_cov = None
        if compute_cls_var:                                                                    # PR:458-470
            self.cls_var = nn.Conv2d(in_channels, num_anchors * num_classes, 3, padding=1)
            nn.init.normal_(self.cls_var.weight, mean=0, std=0.01)
            nn.init.constant_(self.cls_var.bias, -10.0)
        if compute_bbox_cov:                                                                   # PR:473-484
            self.bbox_cov = nn.Conv2d(in_channels, num_anchors * bbox_cov_dims, 3, padding=1)
            nn.init.normal_(self.bbox_cov.weight, mean=0, std=0.0001)
            nn.init.constant_(self.bbox_cov.bias, 0)

    def _replayed(self, x: torch.Tensor, sid: int, layer: int, level: int) -> torch.Tensor:
        """x (copies, C, H, W), any memory format, times the replayed keep-masks / (1 - p) (torch's dropout arithmetic)."""
        keep = torch.stack([self.dropout_replay(sid, layer, level, c) for c in range(x.shape[0])]).to(x.device)
        return x * (keep.to(x.dtype) / (1.0 - self.dropout_rate))

    def _trunk(self, convs, feature, copies: int, dropout: bool, level: int = 0):
        """`copies` independent evaluations of a subnet, batched on dim 0.  The first conv+ReLU is
        identical across copies (dropout only follows it) and is computed once.

        On the GPU the trunk of a large map runs channels-last: MIOpen's fp32 implicit-GEMM kernel for these shapes is an
        NHWC kernel and otherwise transposes its input and output on every call (2 x 120 us per conv on p3, 19 copies)."""
        fused = self.fused_relu_dropout and feature.is_cuda and feature.dtype == torch.float32 and FUSE_CONV_TAIL
        nhwc = fused and dropout and feature.shape[-2] * feature.shape[-1] >= NHWC_TRUNK_MIN_CELLS
        if nhwc:
            feature = feature.contiguous(memory_format=torch.channels_last)
        x = conv_bias_act(convs[0], feature, relu=True)
        if not dropout:
            for conv in convs[1:]:
                x = conv_bias_act(conv, x, relu=True)
            return x                                  # batch 1; shared by every copy
        sid = 0 if convs is self.cls_subnet else 1
        if self.dropout_replay is not None:
            x = self._replayed(x.expand(copies, -1, -1, -1), sid, 0, level)
            for j, conv in enumerate(convs[1:], 1):
                x = self._replayed(conv_bias_act(conv, x, relu=True) if fused else F.relu(conv(x)), sid, j, level)
            return x.contiguous()
        if fused and x.numel() % 4 == 0:
            src = x if (x.is_contiguous() or x.is_contiguous(memory_format=torch.channels_last)) else x.contiguous()
            x = torch.empty((copies,) + tuple(src.shape[1:]), dtype=src.dtype, device=src.device,
                            memory_format=torch.channels_last if (nhwc and not src.is_contiguous()) else torch.contiguous_format)
            self._drop_calls += 1
            hip.check(hip.load().pod_expand_dropout(src.data_ptr(), x.data_ptr(), src.numel(), copies, float(self.dropout_rate),
                                                    self.dropout_seed, self._drop_calls << 34, None, hip.current_stream()), "pod_expand_dropout")
        else:
            x = F.dropout(x.expand(copies, -1, -1, -1), self.dropout_rate, training=True)
        for conv in convs[1:]:
            if fused:
                self._drop_calls += 1                 # distinct Philox counter block per call
                x = conv_bias_act(conv, x, relu=True, dropout_p=self.dropout_rate, seed=self.dropout_seed,
                                  offset=self._drop_calls << 34, out_nchw=conv is convs[-1])
            else:
                x = self._relu_dropout(conv(x))
        return x

    def _wino(self, conv: nn.Conv2d):
        return wino_of(conv)

    def _grouped_ok(self, *copies) -> bool:
        """The subnets' launches in one grid (pod_wino_conv3x3_split_grouped): the split kernel, the replicas in the store pass."""
        return (GROUPED_HEAD and all(1 <= c <= 127 for c in copies)
                and all(self._wino(c).split for c in list(self.cls_subnet) + list(self.bbox_subnet)))

    def _trunk_plan(self, subnets, st: HeadPlan, bufs=None) -> dict:
        """The bookkeeping of the trunks' launches, subnets: [(0 = cls / 1 = bbox, copies)]; touches the device for buffers and
        `block_table`s only.  st: the HeadPlan, x0 = the features as (pixels of all levels, C) channels-last, level after level, in two forms.
        Inference: ONE image per level.  With st.dropout (MC dropout) a subnet is evaluated `copies` times -- its first activation,
        identical for every copy, is computed once and stored `copies` times under the copies' masks (`firsts` tables, "replicas") -- and
        a subnet's layers ping-pong between two buffers (bufs: `new(key, shape)`, the sparse tower's re-used ones); without, one evaluation
        and no mask arguments.  Training (st.images = B, head_train.py): B images per level, evaluated once by every subnet, every layer
        writes a buffer of its own (the backward reads them), and masks are keyed at p = 0 too.  st.channels bounds the tables' canvases.
        Masked, subnet i's layer l draws the Philox offset base + i L + l + 1, ONE for the whole buffer: an element's mask is keyed by its
        index in it.  -> layers: per layer the `sets` of wino.grouped_launch ("conv" still the nn.Conv2d, `_launch` looks its WinoConv up);
        kw: their common arguments; copies: images per level in each subnet's buffers; replay: recorded masks stand in for Philox's."""
        x0, levels, B = st.x0, st.levels, st.images
        L, C, dev, ch = len(self.cls_subnet), x0.shape[1], x0.device, st.channels
        replicas, masked = st.dropout and not B, bool(st.dropout or B)
        copies = [B or (c if replicas else 1) for _, c in subnets]
        new = bufs or (lambda key, shape: torch.empty(shape, dtype=x0.dtype, device=dev))
        dsts = [[new("t%d_%d" % (i, j), (wino.level_pixel_offsets(levels, c)[-1], C)) for j in range(L if B else 2)] for i, c in enumerate(copies)]
        tables = [wino.block_table(levels, c, dev, channels=ch) for c in copies]
        firsts = [wino.block_table(levels, 1, dev, out_copies=c, channels=ch) for c in copies] if replicas else tables
        replay = masked and self.dropout_rate > 0.0 and self.dropout_replay is not None
        kw = {"relu": True}
        if masked:
            kw.update(dropout_p=0.0 if replay else float(self.dropout_rate), seed=self.dropout_seed, epoch=self._epoch)
            base = self._drop_calls
            self._drop_calls += len(subnets) * L
        layers = [[{"conv": (self.cls_subnet, self.bbox_subnet)[sid][l], "src": d[(l - 1) % len(d)] if l else x0, "dst": d[l % len(d)],
                    "table": tables[i] if l else firsts[i], "offset": (base + i * L + l + 1) << 34 if masked else 0,
                    **({"replicas": copies[i]} if replicas and l == 0 else {})}
                   for i, ((sid, _), d) in enumerate(zip(subnets, dsts))] for l in range(L)]
        return {"layers": layers, "kw": kw, "copies": copies, "replay": replay}

    def _launch(self, sets, st: HeadPlan, live=None, **kw) -> None:
        """Launches `sets` (a layer of the trunks, or the predictors): ONE grid (pod_wino_conv3x3_split, n_sets > 1) when the head's launches
        are grouped and the convs share a padded width -- the kernel runs one workgroup per CU, so a launch costs whole rounds of 256
        workgroups: two launches of 1.5 rounds cost 4, one of 3.0 costs 3 -- and one one-set launch each otherwise: the same buffers, tables,
        Philox offsets and therefore the same bits.  live: a callable (table) -> its live records (the sparse tower), or None."""
        sets = [dict(s, conv=self._wino(s["conv"])) for s in sets]
        if st.grouped and len({s["conv"].Kpad for s in sets}) == 1 and all(s["conv"].split for s in sets):
            return wino.grouped_launch(sets, live=live, **kw)
        for s in sets:
            conv, r = s["conv"], s.get("replicas", 0)
            if conv.split and r <= 127:                        # (the copies stored by the conv's own store pass)
                wino.grouped_launch([s], live=live, **kw)
            elif not r:                                        # the fp32-MFMA kernel
                conv(s["src"], s["dst"], s["table"], offset=s.get("offset", 0), planes=s.get("planes", False),
                     **({} if live is None else {"live": live(s["table"])}), **kw)
            else:                                              # ... its copies stored by a pass of their own per level (the same masks)
                levels, x0 = st.levels, s["src"]
                y = conv(x0, torch.empty_like(x0), wino.block_table(levels, 1, x0.device), relu=True)
                off1, offr = wino.level_pixel_offsets(levels, 1), wino.level_pixel_offsets(levels, r)
                for lv, (h, w) in enumerate(levels):
                    hip.check(hip.load().pod_expand_dropout(y[off1[lv]:].data_ptr(), s["dst"][offr[lv]:].data_ptr(), h * w * conv.C, r,
                                                            kw["dropout_p"], kw["seed"], s["offset"] + offr[lv] * conv.C // 8,
                                                            kw["epoch"].data_ptr(), hip.current_stream()), "pod_expand_dropout")

    def _trunks(self, subnets, st: HeadPlan, live=None, bufs=None):
        """Subnet evaluations on ALL levels: `_trunk_plan`'s launches, one per conv layer (fp32 Winograd on the matrix cores, bias + ReLU +
        dropout in its store) instead of one MIOpen call + one element-wise pass per level and layer.  Returns per subnet (buffer, images
        per level): the last activation as (pixels of all levels x images, C) channels-last, level after level; in the training form
        st.saved[i][l] = (input, output) of layer l besides.
        live (sparse bbox tower, pod_compare_amd/sparse.py): a LiveBlocks -- layer j is launched over the blocks of reach L - j only; bufs:
        the tower's buffers (only live blocks are written; what dead blocks hold is never read)."""
        assert live is None or st.grouped, "the sparse tower needs the split kernel's grouped launches"
        plan = self._trunk_plan(subnets, st, bufs)
        levels, L = st.levels, len(plan["layers"])
        for l, sets in enumerate(plan["layers"]):
            self._launch(sets, st, live=None if live is None else (lambda t: live(t, sparse.reach_of_subnet_layer(l, L), sparse.DENSE_INPUT if l == 0 else -1)),
                         **plan["kw"])
            if plan["replay"]:      # parity mode: the recorded masks on the channels-last images of the layer's output (the in-place
                for s, (sid, _), c in zip(sets, subnets, plan["copies"]):         # copy bumps its version: the launch's abs-max record lapses)
                    offs = wino.level_pixel_offsets(levels, c)
                    for lv, (h, w) in enumerate(levels):
                        v = s["dst"][offs[lv]:offs[lv + 1]].view(c, h, w, -1)
                        v.copy_(self._replayed(v.permute(0, 3, 1, 2), sid, l, lv).permute(0, 2, 3, 1))
        if st.images:
            st.saved = [[(sets[i]["src"], sets[i]["dst"]) for sets in plan["layers"]] for i in range(len(subnets))]
        return [(plan["layers"][-1][i]["dst"], c) for i, c in enumerate(plan["copies"])]

    def _jobs(self, side: int, trunk, st: HeadPlan):
        """The predictor jobs (`_predict`) of one side -- 0: cls_score (+ cls_var), 1: bbox_pred (+ bbox_cov) -- on its trunk (buffer, images
        per level).  With dropout the mean branch reads the trunk's first images and the variance branch the m after them (an independent
        dropout draw, Q2): cls [0, m) and [m, 2m), bbox [0, n) and [n, n + m).  Without, both read the one evaluation."""
        buf, copies = trunk
        mean, var = (self.cls_score, self.cls_var) if side == 0 else (self.bbox_pred, self.bbox_cov)
        if not st.dropout:
            return [(conv, buf, 1, 0, 1, 1) for conv in (mean, var) if conv is not None]
        n, m = st.n, st.m
        first = m if side == 0 else n
        return [(mean, buf, copies, 0, first, n)] + ([(var, buf, copies, first, m, n)] if var is not None else [])

    def _predict(self, jobs, st: HeadPlan, live=None, bufs=None, flat: bool = False):
        """The predictor convs (cls_score / bbox_pred / cls_var / bbox_cov, PR:430-484), one `_launch`.  jobs: (conv, trunk buffer, images in
        it per level, first image, image count, output images) -- inference: `_jobs`'; training: all B images of a trunk, (conv, buf, B, 0,
        B, B).  Returns per job and level an (out_copies, K, H, W) NCHW tensor -- the planes K1 streams -- whose images past `count` are zero
        (never uninitialised memory: a consumer without the quirk merge would read them); flat: per job the one buffer those are views of.
        live / bufs: the sparse tower (`_trunks`)."""
        levels = st.levels
        sets, outs = [], []
        for ji, (conv, buf, buf_copies, first, count, out_copies) in enumerate(jobs):
            K = conv.out_channels
            offs = wino.level_pixel_offsets(levels, out_copies)
            if bufs is not None:
                out = bufs("p%d" % ji, (offs[-1] * K,))
            else:
                out = (torch.zeros if out_copies > count else torch.empty)(offs[-1] * K, dtype=buf.dtype, device=buf.device)
            sets.append({"conv": conv, "src": buf, "dst": out, "planes": True,
                         "table": wino.block_table(levels, count, buf.device, in_copies=buf_copies, in_first=first, out_copies=out_copies,
                                                   channels=st.channels)})
            outs.append(out if flat else [out[offs[i] * K:offs[i + 1] * K].view(out_copies, K, h, w) for i, (h, w) in enumerate(levels)])
        self._launch(sets, st, live=None if live is None else (lambda table: live(table, sparse.REACH_PREDICTOR)))
        return outs

    @staticmethod
    def _expanded(res, st: HeadPlan):
        """Eval mode: the one evaluation of each predictor as the n runs' images (every run would give the same)."""
        if st.dropout or st.n == 1:
            return res
        return [[t.expand(st.n, -1, -1, -1).contiguous() for t in ts] for ts in res]

    def takes_wino_path(self) -> bool:
        """Every conv of the head runs on pod_wino_conv3x3[_split] (GPU, fp32, one image): then all its dropout masks take the `_epoch` word."""
        predictors = [c for c in (self.cls_score, self.bbox_pred, self.cls_var, self.bbox_cov) if c is not None]
        return (WINO_HEAD and self.fused_relu_dropout and FUSE_CONV_TAIL
                and self.cls_subnet[0].in_channels % 8 == 0                       # either kernel: the fp32-MFMA kernel's channel step
                and self.cls_subnet[0].out_channels in (64, 128, 256, 512)        # a trunk layer's channels-last output is the next one's input: no padded channels
                and max(c.out_channels for c in predictors) <= 512)               # the predictors store their real K planes: only the padded width is bound

    def _relu_dropout(self, x: torch.Tensor) -> torch.Tensor:
        """ReLU + Dropout(p) after a subnet conv (PR:403-424).  On the GPU one fused in-place HIP pass
        (pod_relu_dropout) instead of torch's clamp + fused_dropout kernels."""
        if not (self.fused_relu_dropout and x.is_cuda and x.is_contiguous() and x.dtype == torch.float32):
            return F.dropout(F.relu(x), self.dropout_rate, training=True)
        lib = hip.load()
        self._drop_calls += 1
        hip.check(lib.pod_relu_dropout(x.data_ptr(), x.numel(), float(self.dropout_rate), self.dropout_seed,
                                       self._drop_calls << 34, hip.current_stream()), "pod_relu_dropout")
        return x

    def sparse_buffers(self, key):
        """Re-used activation buffers of the sparse bbox tower, per (stream, geometry): new(name, shape)."""
        pool = self._sparse_pool.setdefault(key, {})

        def new(name, shape):
            t = pool.get(name)
            if t is None or tuple(t.shape) != tuple(shape):
                # zeroed once (a reader of the DENSE tensors finds finite numbers outside the live blocks).  The tower itself never reads
                # what an earlier image left here: a sparse launch reads the cells the layer below did not compute for this image as 0.0
                # (the need bits of sparse.LiveBlocks), and every launch gets a fresh abs-max record -- results depend on the image alone
                t = pool[name] = torch.zeros(shape, dtype=torch.float32, device=self.cls_score.weight.device)
            return t
        return new

    def _plan(self, features: List[torch.Tensor], num_runs: int, mc_dropout: bool, skip_unused_last_run: bool) -> HeadPlan:
        """The run bookkeeping of a head evaluation: n runs, of which m = n - skip need cls / cls_var / reg_var, the copies each trunk
        evaluates, and whether every conv takes pod_wino_conv3x3 (`wino`; then `grouped` (`_grouped_ok`), `levels` and `x0`, the features
        as one channels-last buffer, level after level)."""
        dropout = mc_dropout and self.dropout_rate > 0.0
        n = num_runs
        skip = 1 if (skip_unused_last_run and dropout and n > 1) else 0
        m = n - skip                                               # runs whose cls / cls_var / reg_var are needed
        st = HeadPlan(n=n, m=m, skip=skip, dropout=dropout, cls_copies=m * (2 if self.compute_cls_var else 1),
                      box_copies=n + (m if self.compute_bbox_cov else 0))
        f = features[0]
        st.wino = (self.takes_wino_path() and f.is_cuda and f.dtype == torch.float32 and f.shape[0] == 1
                   and f.shape[1] == self.cls_subnet[0].in_channels)
        if st.wino:
            st.grouped, st.levels = self._grouped_ok(st.cls_copies, st.box_copies), [(int(f.shape[2]), int(f.shape[3])) for f in features]
            st.x0 = levels_channels_last(features)
        return st

    def forward_cls(self, features: List[torch.Tensor], num_runs: int = 1, mc_dropout: bool = False, skip_unused_last_run: bool = False) -> HeadPlan:
        """First half of the sparse evaluation (ProbabilisticRetinaNet.cls_part): the cls subnet + cls_score (+ cls_var) of all levels and
        runs.  Returns the plan `forward_bbox` continues from, `logits` and `logit_vars` set."""
        st = self._plan(features, num_runs, mc_dropout, skip_unused_last_run)
        if not (st.wino and st.grouped):
            raise RuntimeError("the sparse bbox tower needs the split kernels on the GPU (POD_WINO_SPLIT=1, one fp32 image, grouped head)")
        (tc,) = self._trunks([(0, st.cls_copies)], st)
        res = self._expanded(self._predict(self._jobs(0, tc, st), st), st)
        st.logits, st.logit_vars = res[0], (res[1] if self.compute_cls_var else None)
        return st

    def forward_bbox(self, st: HeadPlan, live):
        """Second half: bbox_subnet + bbox_pred (+ bbox_cov) over the blocks `live` (sparse.LiveBlocks) lists; None = all of them."""
        bufs = None if live is None else self.sparse_buffers((torch.cuda.current_stream(st.x0.device).cuda_stream, tuple(st.levels), st.n,
                                                              st.dropout, st.skip))
        (tb,) = self._trunks([(1, st.box_copies)], st, live=live, bufs=bufs)
        res = self._expanded(self._predict(self._jobs(1, tb, st), st, live=live, bufs=bufs), st)
        return res[0], (res[1] if self.compute_bbox_cov else None)

    def forward_train(self, features: List[torch.Tensor], anchors=None, image_size=None) -> HeadOutputs:
        """The training forward (PR:403-537 with dropout after every trunk conv, one evaluation per image): features per level
        (B, C, H, W), B images of one padded size -> HeadOutputs whose leading dimension is the image and whose tensors carry a grad_fn
        (pod_compare_amd/head_train.py: the HIP backward of the head's convolutions).  GPU only."""
        from .head_train import forward_train      # local, the one cycle: head_train imports modeling (HeadPlan) at its top
        return forward_train(self, features, anchors, image_size)

    def forward(self, features: List[torch.Tensor], num_runs: int = 1, mc_dropout: bool = False, skip_unused_last_run: bool = False):
        """features: per-level (1, 256, H, W).  Returns per-level lists of (num_runs, A*C, H, W).

        skip_unused_last_run: the reference's merge (PI:216-222) never reads run N-1 of box_cls,
        box_cls_var and box_reg_var (only box_delta's last run is used, by the epistemic covariance PI:325-331).
        With the flag set those three evaluations of the last run are not computed (their slab in the returned
        tensors is zero): 3 of the 4N subnet evaluations, 7.5 % of the head at N = 10.  Only valid
        together with `merge_quirk=True` in the hot path."""
        st = self._plan(features, num_runs, mc_dropout, skip_unused_last_run)
        if st.wino:
            # every conv of the head on pod_wino_conv3x3: one launch per layer over all levels and all runs, both trunks, then the predictors
            tc, tb = self._trunks([(0, st.cls_copies), (1, st.box_copies)], st)
            cj, bj = self._jobs(0, tc, st), self._jobs(1, tb, st)
            res = self._expanded(self._predict(cj[:1] + bj[:1] + cj[1:] + bj[1:], st), st)       # cls_score, bbox_pred (, cls_var) (, bbox_cov)
            return res[0], res[1], (res[2] if self.compute_cls_var else None), (res[-1] if self.compute_bbox_cov else None)
        n, m, dropout = st.n, st.m, st.dropout

        def padded(t):                                            # (m, C, H, W) -> (n, C, H, W) NCHW planes (what K1 streams),
            if m == n:                                            # last slab untouched; a channels-last trunk output is
                return t.contiguous()                             # transposed by the same copy
            out = torch.empty((n,) + tuple(t.shape[1:]), dtype=t.dtype, device=t.device)
            out[:m].copy_(t)
            out[m:].zero_()                                       # never hand out uninitialised memory (a consumer without
            return out                                            # the quirk merge would read it); 1/n of one small tensor

        logits, deltas, logit_vars, delta_covs = [], [], [], []
        for level, f in enumerate(features):
            tc = self._trunk(self.cls_subnet, f, st.cls_copies, dropout, level)
            tb = self._trunk(self.bbox_subnet, f, st.box_copies, dropout, level)
            if dropout:
                # (a channels-last trunk hands its last activation over as NCHW planes: the A*K / A*4-channel predictor convs
                #  are faster as NCHW Winograd calls than as NHWC implicit GEMMs)
                logits.append(padded(conv_bias_act(self.cls_score, tc[:m])))
                deltas.append(conv_bias_act(self.bbox_pred, tb[:n]).contiguous())
                if self.compute_cls_var:
                    logit_vars.append(padded(conv_bias_act(self.cls_var, tc[m:])))     # independent dropout draw (Q2)
                if self.compute_bbox_cov:
                    delta_covs.append(padded(conv_bias_act(self.bbox_cov, tb[n:])))
            else:
                ex = (lambda t: t.expand(n, -1, -1, -1).contiguous()) if n > 1 else (lambda t: t)
                logits.append(ex(self.cls_score(tc)))
                deltas.append(ex(self.bbox_pred(tb)))
                if self.compute_cls_var:
                    logit_vars.append(ex(self.cls_var(tc)))
                if self.compute_bbox_cov:
                    delta_covs.append(ex(self.bbox_cov(tb)))
        return logits, deltas, (logit_vars if self.compute_cls_var else None), (delta_covs if self.compute_bbox_cov else None)


class ProbabilisticRetinaNet(_TracksStorage):
    """PR:20-166, and `losses` (PR:168-333 with the labelling of PR:129-130) evaluated on the head outputs of a forward by the K21 kernels
    (pod_compare_amd/losses.py).  The head's convolutions have a backward pass (head.forward_train, pod_compare_amd/head_train.py), and
    so have the FPN's (pod_compare_amd/fpn_train.py); the ResNet's have none: it stays frozen."""

    def __init__(self, num_classes=7, dropout_rate=0.0, cls_var_loss="none", cls_var_num_samples=3,
                 bbox_cov_loss="none", bbox_cov_type="diagonal", test_score_thresh=0.05, test_topk_candidates=1000,
                 test_nms_thresh=0.5, max_detections_per_image=100, min_size_test=800, max_size_test=1333, bbox_cov_num_samples=1000):
        super().__init__()
        self.num_classes = num_classes
        self.bbox_cov_loss, self.bbox_cov_num_samples = bbox_cov_loss, bbox_cov_num_samples      # PR:33-35
        self.compute_cls_var = cls_var_loss != "none"                  # PR:29-30
        self.cls_var_num_samples = cls_var_num_samples
        self.compute_bbox_cov = bbox_cov_loss != "none"                # PR:33-34
        self.bbox_cov_dims = 4 if bbox_cov_type == "diagonal" else 10  # PR:37-44
        self.dropout_rate = dropout_rate
        self.use_dropout = dropout_rate != 0.0
        self.test_score_thresh, self.test_topk_candidates = test_score_thresh, test_topk_candidates
        self.test_nms_thresh, self.max_detections_per_image = test_nms_thresh, max_detections_per_image
        self.min_size_test, self.max_size_test = min_size_test, max_size_test
        self.input_format = "BGR"
        self.in_features = ["p3", "p4", "p5", "p6", "p7"]
        self.num_anchors = len(_anchors.ANCHOR_SIZES[0]) * len(_anchors.ASPECT_RATIOS)
        self.bottom_up = ResNet50()
        self.fpn = FPN()
        self.head = ProbabilisticRetinaNetHead(256, self.num_anchors, num_classes, 4, 0.01, dropout_rate,
                                               self.compute_cls_var, self.compute_bbox_cov, self.bbox_cov_dims)
        self.register_buffer("pixel_mean", torch.tensor(PIXEL_MEAN_BGR).view(3, 1, 1), persistent=False)
        self.register_buffer("pixel_std", torch.tensor(PIXEL_STD).view(3, 1, 1), persistent=False)
        self._anchor_cache: Dict[Tuple[int, int], List[torch.Tensor]] = {}
        self.use_graphs = False
        self.max_graphs = 16                                   # (stream, frame shape, flags) entries kept (four frame shapes on each of apply_net's four streams); each owns its activations
        self.graph_after_seen = 0                              # forwards of a (stream, shape, flags) run eagerly before it is captured
        self._graphs: Dict[tuple, tuple] = {}
        self._graph_seen: Dict[tuple, int] = {}
        self._graph_serial = 0
        self._fingerprint_tensors = None
        self._graphs_fingerprint = None
        self.register_load_state_dict_post_hook(lambda module, incompatible: bump_param_generation())

    @property
    def device(self):
        return self.pixel_mean.device

    def preprocess_image(self, image: torch.Tensor) -> torch.Tensor:
        """(3,H,W) BGR uint8/float -> normalised, zero-padded (1,3,H',W') with H',W' % 32 == 0 (PR:96)."""
        x = (image.to(self.device, torch.float32) - self.pixel_mean) / self.pixel_std
        h, w = x.shape[-2:]
        ph, pw = _anchors.padded_size(h, w)
        return F.pad(x, (0, pw - w, 0, ph - h)).unsqueeze(0)

    def anchors_for(self, padded_hw: Tuple[int, int]) -> List[torch.Tensor]:
        if padded_hw not in self._anchor_cache:
            shapes = _anchors.level_shapes(*padded_hw)
            self._anchor_cache[padded_hw] = _anchors.grid_anchors(shapes, device=self.device)
            if self.device.type == "cuda":
                torch.cuda.current_stream(self.device).synchronize()   # made once, then read from any stream
        return self._anchor_cache[padded_hw]

    def losses(self, outputs: HeadOutputs, gt_boxes, gt_classes, eps=None, normalizer=None) -> Dict[str, torch.Tensor]:
        """PR:129-130 + PR:168-333 on `outputs` (a forward's HeadOutputs; the leading dimension of its tensors is the image): gt_boxes /
        gt_classes are per-image lists of (G_i, 4) XYXY boxes in network-input pixels and (G_i,) contiguous class ids.  Returns
        {"loss_cls", "loss_box_reg"} as device scalars.  The state the reference keeps on the model (loss_normalizer, current_step) lives in
        `self.loss_state` (losses.ProbabilisticLosses); eps / normalizer as in its __call__."""
        if getattr(self, "loss_state", None) is None:
            self.loss_state = _losses.ProbabilisticLosses(num_classes=self.num_classes, cls_var_num_samples=self.cls_var_num_samples,
                                                          bbox_cov_loss=self.bbox_cov_loss, bbox_cov_num_samples=self.bbox_cov_num_samples)
        labels, matched, _ = _losses.label_anchors(outputs.anchors, gt_boxes, gt_classes, self.num_classes)
        boxes, _, _ = _losses.concat_ground_truth(gt_boxes, gt_classes, labels.device)
        return self.loss_state(outputs, labels, matched, boxes, eps=eps, normalizer=normalizer)

    # ---- HIP graphs --------------------------------------------------------------------------------------------------------
    # One image's forward is ~200 launches (MIOpen calls, pod_* kernels, torch element-wise ops) issued from Python: 2.3 - 2.5 ms of
    # host time, which is the whole step of the single-run configurations (BASELINE configs[1], [3]: 2.5 ms of GPU time).  With
    # `enable_graphs()` the forward of a given (stream, frame shape, flags) is captured once into a HIP graph and replayed: one
    # host call per image.  MC-dropout forwards too, when the head runs on the Winograd kernels: their masks' Philox key folds in a
    # device word (`head._epoch`) that the captured forward itself bumps first thing, so every replay draws fresh masks although
    # seed / offset are constants of the captured launches.  Not captured: a dropout forward on the MIOpen head path, anything off
    # the GPU, the parity mode (`dropout_replay`).  The returned tensors belong to the graph: they are valid until the next forward
    # of the same (stream, shape, flags) -- on the same stream, so a consumer enqueued there before that is safe.
    def enable_graphs(self, on: bool = True) -> "ProbabilisticRetinaNet":
        self.use_graphs = bool(on)
        if not on:
            self._drop_graphs()
        return self

    def _drop_graphs(self):
        if self._graphs:
            torch.cuda.synchronize(self.device)          # (a consumer of a graph's tensors may still be queued)
            self._graphs.clear()

    # A captured graph holds raw pointers to the pre-transformed filters (WinoConv.U, Conv1x1.Ws, Stem7x7.Ws) and folded biases of the
    # moment of capture: a graph must never answer for parameters that changed since.  Two things change them: a move / re-allocation
    # (.to(), .cuda(), load_state_dict(assign=True), fold_frozen_bn: all go through _apply / the load hook / module surgery -> the
    # generation counter) and an in-place write (load_state_dict, copy_: bumps the tensors' `_version`).  Both are in the fingerprint;
    # when it moves, every graph is dropped and the next forward re-captures against re-transformed filters.
    def _param_fingerprint(self):
        gen = _PARAM_GENERATION[0]
        ts = self._fingerprint_tensors
        if ts is None or ts[0] != gen:
            ts = self._fingerprint_tensors = (gen, [t for t in list(self.parameters()) + list(self.buffers()) if t is not self.head._epoch])
        return gen, len(ts[1]), sum(t._version for t in ts[1])

    def _cls_eager(self, image: torch.Tensor, n: int, dropout: bool, skip: bool) -> HeadPlan:
        feats, padded = self._trunk_eager(image)
        st = self.head.forward_cls(feats, n, mc_dropout=dropout, skip_unused_last_run=skip)
        st.padded, st.image_hw, st.shapes = padded, tuple(image.shape[-2:]), [tuple(f.shape[-2:]) for f in feats]
        return st

    def _run_args(self, num_mc_dropout_runs: int, mc_dropout: Optional[bool]) -> Tuple[int, bool]:
        """(n runs, dropout active) of a forward's arguments: dropout defaults to "several runs are requested", and needs a model that has it."""
        n = num_mc_dropout_runs if num_mc_dropout_runs > 1 else 1
        if mc_dropout is None:
            mc_dropout = n > 1
        return n, bool(mc_dropout) and self.use_dropout

    def _graphable(self, image: torch.Tensor, dropout: bool) -> bool:
        """This forward may be captured and replayed (see "HIP graphs" above for what may not)."""
        return (self.use_graphs and image.is_cuda and self.device.type == "cuda" and self.head.dropout_replay is None
                and (not dropout or self.head.takes_wino_path()))

    @torch.no_grad()
    def cls_part(self, image: torch.Tensor, num_mc_dropout_runs: int = -1, skip_unused_last_run: bool = False, mc_dropout: Optional[bool] = None) -> HeadPlan:
        """First part of a forward with the sparse bbox tower: trunk + the cls side of the head (captured into a HIP graph like a whole forward
        when graphs are enabled).  Returns the plan `bbox_part` continues from; `partial_outputs` of it is the HeadOutputs with cls / cls_var set."""
        n, dropout = self._run_args(num_mc_dropout_runs, mc_dropout)
        if self._graphable(image, dropout):
            return self._forward_graphed(image, n, dropout, skip_unused_last_run, part="cls")
        return self._cls_eager(image, n, dropout, skip_unused_last_run)

    def partial_outputs(self, st: HeadPlan, delta=None, reg_var=None) -> HeadOutputs:
        return HeadOutputs(st.logits, delta, st.logit_vars, reg_var, self.anchors_for(st.padded), st.shapes, self.num_anchors,
                           self.num_classes, st.image_hw, last_run_valid=not bool(st.skip))

    @torch.no_grad()
    def bbox_part(self, st: HeadPlan, live) -> HeadOutputs:
        """Second part: the bbox side over the blocks `live` (sparse.LiveBlocks, made from the candidates the caller selected) lists."""
        delta, reg_var = self.head.forward_bbox(st, live)
        return self.partial_outputs(st, delta, reg_var)

    def _forward_graphed(self, image: torch.Tensor, n: int, dropout: bool, skip: bool, part: str = "all"):
        stream = torch.cuda.current_stream(image.device)
        run = self._forward_eager if part == "all" else self._cls_eager
        fp = self._param_fingerprint()
        if fp != self._graphs_fingerprint:
            self._drop_graphs()
            self._fingerprint_tensors = None                   # (module surgery -- fold_frozen_bn -- also changes WHICH tensors there are)
            self._graphs_fingerprint = self._param_fingerprint()
        # (the kernel selection is part of the key: a graph captured with one convolution kernel must not answer for the other)
        key = (stream.cuda_stream, tuple(image.shape), image.dtype, n, dropout, skip, kernel_selection(), part)
        ent = self._graphs.get(key)
        if ent is None:
            # graphs are for (stream, shape) pairs that come back: the first GRAPH_AFTER_SEEN forwards of a key run eagerly (a data set of
            # many frame sizes would otherwise pay two eager forwards + a capture per image -- slower than no graphs at all)
            seen = self._graph_seen.get(key, 0) + 1
            if len(self._graph_seen) > 4096:
                self._graph_seen.clear()
            self._graph_seen[key] = seen
            if seen <= self.graph_after_seen:
                return run(image, n, dropout, skip)
            static_in = image.clone()
            shared_epoch = self.head._epoch
            # every graph owns its epoch word: replays of two graphs on two streams must not read-modify-write one word (the masks
            # would depend on GPU timing).  It starts at (serial of the graph) << 32, so no two graphs ever draw the same masks and
            # the masks of the i-th replay of the j-th captured graph are a function of (seed, j, i) alone.
            self._graph_serial += 1
            epoch = torch.full_like(shared_epoch, self._graph_serial << 32)
            self.head._epoch = epoch
            try:
                for _ in range(2):                       # eager: MIOpen's solver search, filter transforms, block tables, anchors
                    run(static_in, n, dropout, skip)
                stream.synchronize()
                side = torch.cuda.Stream(device=image.device)          # (capture is not allowed on the legacy default stream)
                side.wait_stream(stream)
                graph = torch.cuda.CUDAGraph()
                # thread_local: only this thread's calls are policed during the capture (an RCCL watchdog thread polling its events
                # must not abort it)
                # (the warm-up forwards attached an abs-max record to a float frame: it is the FIRST frame's, and a capture that found it
                #  would record no pod_absmax -- every replay would scale the stem's split by that frame's range.  ADVICE r5)
                amax.forget(static_in)
                amax.reset()                               # the operand abs-max words of the captured launches come from pools zeroed INSIDE the
                with torch.cuda.graph(graph, stream=side, capture_error_mode="thread_local"):      # capture: every replay starts from zeroed words
                    if dropout:
                        epoch.add_(1)                      # (captured: every replay starts by moving on to the next set of masks)
                    out = run(static_in, n, dropout, skip)
                stream.wait_stream(side)
            finally:
                amax.reset()                               # (eager launches never max into a graph's words)
                self.head._epoch = shared_epoch
            while len(self._graphs) >= self.max_graphs:          # frames of many different sizes: keep the most recent shapes only
                old_key = next(iter(self._graphs))
                torch.cuda.ExternalStream(old_key[0], device=image.device).synchronize()   # (a consumer of the evicted graph's tensors may
                self._graphs.pop(old_key)                                                  #  still be queued -- on ITS stream, nowhere else)
            ent = (graph, static_in, out, epoch)
        else:
            self._graphs.pop(key)
        self._graphs[key] = ent                                # most recently used last
        graph, static_in, out, _ = ent
        static_in.copy_(image, non_blocking=True)
        graph.replay()
        return out

    def graph_epoch(self, stream=None, **match) -> Optional[torch.Tensor]:
        """The epoch word of the most recently used graph on `stream` (default: the current one); tests and diagnostics."""
        st = (stream or torch.cuda.current_stream(self.device)).cuda_stream
        for key in reversed(list(self._graphs)):
            if key[0] == st and key[4]:
                return self._graphs[key][3]
        return None

    @torch.no_grad()
    def forward(self, image: torch.Tensor, num_mc_dropout_runs: int = -1, skip_unused_last_run: bool = False,
                mc_dropout: Optional[bool] = None, sparse_bbox=None) -> HeadOutputs:
        """Raw anchor-wise output (`return_anchorwise_output=True`, PR:352-361) in NCHW plane layout.
        num_mc_dropout_runs > 1 batches that many dropout-perturbed head evaluations (PR:103-108).
        mc_dropout: dropout active in the head subnets -- the reference's `model.train()` (PI:53-56), which it sets
        whenever MC_DROPOUT.ENABLE is true, also for a single run; default: active iff several runs are requested.
        sparse_bbox: None, or a callable (partial HeadOutputs: cls / cls_var set, delta = reg_var = None) -> sparse.LiveBlocks.  The cls side
        of the head is then evaluated FIRST, the callable selects the image's candidates from it (K1f + K2 of the hot path, PI:283-308) and
        the bbox side -- bbox_subnet, bbox_pred, bbox_cov: PR:518-537 evaluates them densely although PI:310-331 reads them at the candidates
        only -- runs over the blocks that can reach a candidate.  Its outputs are defined at the candidates' cells and stale elsewhere; same
        Philox offsets, so the same dropout masks as the dense evaluation.  The trunk + cls half is replayed as a HIP graph (`cls_part`), the
        bbox half is enqueued eagerly (its live lists are made per image)."""
        n, dropout = self._run_args(num_mc_dropout_runs, mc_dropout)
        if sparse_bbox is not None:
            st = self.cls_part(image, num_mc_dropout_runs, skip_unused_last_run, mc_dropout)
            return self.bbox_part(st, sparse_bbox(self.partial_outputs(st)))
        if self._graphable(image, dropout):
            return self._forward_graphed(image, n, dropout, skip_unused_last_run)
        return self._forward_eager(image, n, dropout, skip_unused_last_run)

    def _cl_backbone(self, x: torch.Tensor) -> bool:
        """The trunk runs channels-last on pod_conv1x1_split + pod_wino_conv3x3_split: GPU, fp32, FrozenBN folded, the split kernels
        selected (POD_WINO_SPLIT=0 -- the fp32-MFMA reference leg -- keeps the 1x1 convolutions on MIOpen as in round 3)."""
        if not (CL_BACKBONE and FUSE_CONV_TAIL and WINO_BACKBONE and wino.SPLIT_BF16 and x.is_cuda and x.dtype == torch.float32):
            return False
        if not getattr(self, "_cl_ok", False):
            self._cl_ok = self.bottom_up.cl_eligible() and self.fpn.cl_eligible()       # (cached once true: folding is one-way)
        return self._cl_ok

    def _backbone_cl(self, image: torch.Tensor, padded: Optional[Tuple[int, int]] = None):
        """Frame -> ([(c3, h, w), (c4, h, w), (c5, h, w)] channels-last, padded (h, w)) when the channels-last HIP backbone takes it, else None.
        padded: the size the frame is run against (a training batch's common ImageList size, a multiple of 32 that holds the frame: the
        stem reads everything outside the frame as zero after normalisation); None: the frame's own anchors.padded_size.  Only the HIP
        stem pads on load: with `padded` anything else is an error."""
        if padded is not None:
            padded = _check_padded(image, padded)
        if (image.is_cuda and image.device == self.device and image.dim() == 3 and image.shape[0] == 3 and image.is_contiguous()
                and image.dtype in (torch.uint8, torch.float32) and self._cl_backbone(self.pixel_mean) and self.bottom_up.hip_stem_ok()):
            # the frame as the loader hands it over: pod_stem7x7_split normalises ((x - mean) / std, PR:96) and pads on load
            if padded is None:
                padded = _anchors.padded_size(int(image.shape[1]), int(image.shape[2]))
            return self.bottom_up.forward_cl(None, frame=(image, self.pixel_mean.reshape(3), self.pixel_std.reshape(3), padded)), padded
        if padded is not None:
            raise hip.PodError("a frame is run against a common padded size only by the channels-last HIP backbone (a (3, h, w) uint8 / fp32 frame "
                               "on the model's GPU, FrozenBN folded, the split kernels and the HIP stem selected)")
        x = self.preprocess_image(image)
        if self._cl_backbone(x):
            return self.bottom_up.forward_cl(x), tuple(x.shape[-2:])      # channels-last trunk on pod_conv1x1_split + pod_wino_conv3x3[_split]
        return None

    def _trunk_eager(self, image: torch.Tensor, padded: Optional[Tuple[int, int]] = None):
        """Frame -> (the five FPN maps, padded (h, w)): everything ahead of the head.  padded: as _backbone_cl's."""
        cl = self._backbone_cl(image, padded)
        if cl is not None:
            return self.fpn.forward_cl(cl[0]), cl[1]
        x = self.preprocess_image(image)                                 # the NCHW path (CPU tensors, the tests' reference; normalised a second time here)
        return self.fpn(self.bottom_up(x)), tuple(x.shape[-2:])

    def _head_eager(self, feats, padded, image_hw, n: int, mc_dropout: bool, skip_unused_last_run: bool) -> HeadOutputs:
        shapes = [tuple(f.shape[-2:]) for f in feats]
        skipped = skip_unused_last_run and n > 1 and bool(mc_dropout) and self.use_dropout
        cls, delta, cls_var, reg_var = self.head(feats, n, mc_dropout=bool(mc_dropout) and self.use_dropout, skip_unused_last_run=skip_unused_last_run)
        return HeadOutputs(cls, delta, cls_var, reg_var, self.anchors_for(padded), shapes, self.num_anchors,
                           self.num_classes, tuple(image_hw), last_run_valid=not skipped)

    def _forward_eager(self, image: torch.Tensor, n: int, mc_dropout: bool, skip_unused_last_run: bool) -> HeadOutputs:
        feats, padded = self._trunk_eager(image)
        return self._head_eager(feats, padded, image.shape[-2:], n, mc_dropout, skip_unused_last_run)


def _check_padded(image: torch.Tensor, padded) -> Tuple[int, int]:
    """A common padded size for `image` (3, h, w): two multiples of the FPN's divisibility that hold the frame."""
    ph, pw = int(padded[0]), int(padded[1])
    d = _anchors.SIZE_DIVISIBILITY
    if len(padded) != 2 or ph % d or pw % d or ph < int(image.shape[-2]) or pw < int(image.shape[-1]):
        raise ValueError("padded = {} does not hold a frame of {} x {} in multiples of {}".format(tuple(padded), int(image.shape[-2]), int(image.shape[-1]), d))
    return ph, pw


def resize_test_image(image: torch.Tensor, min_size: int = 800, max_size: int = 1333) -> torch.Tensor:
    """detectron2 ResizeShortestEdge test transform (apply_net.py:83), bilinear, on the device."""
    h, w = image.shape[-2:]
    nh, nw = _anchors.resize_shortest_edge(h, w, min_size, max_size)
    if (nh, nw) == (h, w):
        return image
    return F.interpolate(image.unsqueeze(0).float(), size=(nh, nw), mode="bilinear", align_corners=False).squeeze(0)
