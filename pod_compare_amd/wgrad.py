"""Host side of K22 (csrc/k22_conv3x3_wgrad.hip): the weight / bias gradients of a 3x3 / stride-1 / pad-1 convolution and the
ReLU + dropout gate of the head's backward pass (probabilistic_retinanet.py:403-484 under train_net.py's loop) -- and of K23
(csrc/k23_fpn_backward.hip): the weight gradient without taps and the two gathers of the FPN's backward pass -- and of K24
(csrc/k24_resnet_backward.hip): the 1x1 weight gradient at the backbone's widths and strides and the scatter that undoes a stride-2 pixel
selection.  GPU only: there is no CPU path."""
import ctypes
from typing import Optional, Sequence, Tuple

import torch

from . import amax, hip


def _level_array(levels: Sequence[Tuple[int, int]]):
    arr = (ctypes.c_int32 * (2 * len(levels)))()
    for i, (h, w) in enumerate(levels):
        arr[2 * i], arr[2 * i + 1] = int(h), int(w)
    return arr


def conv3x3_wgrad(x: torch.Tensor, dy: torch.Tensor, levels: Sequence[Tuple[int, int]], copies: int, K: int):
    """x (pixels, C), dy (pixels, Kpad): channels-last, `copies` images per level, level-major (wino.level_pixel_offsets).  Returns
    (dW (K, C, 3, 3), db (K,)) in fp32.  The operands' abs-max records are their producers' (pod_compare_amd.amax), else computed now."""
    for name, t in (("x", x), ("dy", dy)):
        if not (t.is_cuda and t.dtype == torch.float32 and t.dim() == 2 and t.is_contiguous()):
            raise hip.PodError("pod_conv3x3_wgrad: {} must be a contiguous fp32 (pixels, channels) tensor on the GPU, got {} {} on {}".format(
                name, t.dtype, tuple(t.shape), t.device))
    pixels, C, Kpad = int(copies) * sum(h * w for h, w in levels), int(x.shape[1]), int(dy.shape[1])
    if int(x.shape[0]) != pixels or int(dy.shape[0]) != pixels:
        raise hip.PodError("pod_conv3x3_wgrad: the geometry holds {} pixels, x has {} and dy {}".format(pixels, x.shape[0], dy.shape[0]))
    lib, lv = hip.load(), _level_array(levels)
    n = int(lib.pod_conv3x3_wgrad_partials(lv, len(levels), int(copies), C, int(K), Kpad))
    if n <= 0:
        raise hip.PodError("pod_conv3x3_wgrad: C % 16 == 0, K <= Kpad, Kpad % 64 == 0 and Kpad <= 512 required, got C={} K={} Kpad={}".format(C, K, Kpad))
    partials = torch.empty(n, dtype=torch.float32, device=x.device)
    dW = torch.empty((int(K), C, 3, 3), dtype=torch.float32, device=x.device)
    db = torch.empty((int(K),), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        hip.check(lib.pod_conv3x3_wgrad(x.data_ptr(), dy.data_ptr(), lv, len(levels), int(copies), C, int(K), Kpad, amax.of(x).data_ptr(),
                                        amax.of(dy).data_ptr(), dW.data_ptr(), db.data_ptr(), partials.data_ptr(), hip.current_stream()),
                  "pod_conv3x3_wgrad")
    return dW, db


def relu_dropout_backward(out: torch.Tensor, d_out: torch.Tensor, p: float, d_z: Optional[torch.Tensor] = None) -> torch.Tensor:
    """d_z = d_out (out > 0) / (1 - p): the gate of a trunk layer's conv + bias + ReLU + dropout, read off the layer's stored output.
    d_z: None = in place on d_out.  The abs-max record of d_z is published by the same pass."""
    d_z = d_out if d_z is None else d_z
    for t in (out, d_out, d_z):
        if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.numel() == out.numel()):
            raise hip.PodError("pod_relu_dropout_backward: contiguous fp32 GPU tensors of one size required")
    with torch.cuda.device(out.device):
        hip.check(hip.load().pod_relu_dropout_backward(out.data_ptr(), d_out.data_ptr(), d_z.data_ptr(), out.numel(), float(p),
                                                       amax.produced(d_z).data_ptr(), hip.current_stream()), "pod_relu_dropout_backward")
    return d_z


def _cl(name: str, what: str, t: torch.Tensor) -> None:
    if not (t.is_cuda and t.dtype == torch.float32 and t.dim() == 2 and t.is_contiguous()):
        raise hip.PodError("{}: {} must be a contiguous fp32 (pixels, channels) tensor on the GPU, got {} {} on {}".format(
            name, what, t.dtype, tuple(t.shape), t.device))


def conv1x1_wgrad(x: torch.Tensor, dy: torch.Tensor, bias: bool = True):
    """x (pixels, C), dy (pixels, K), channels-last: (dW (K, C), db (K,) or None) in fp32, dW[k][c] = sum_p dy[p][k] x[p][c].  The weight
    gradient of a 1x1 convolution and, on the patch matrix of pod_im2col3x3s2_cl, of a 3x3 / stride-2 one laid out (K, ty, tx, Cin).  The
    operands' abs-max records are their producers' (pod_compare_amd.amax), else computed now."""
    _cl("pod_conv1x1_wgrad", "x", x)
    _cl("pod_conv1x1_wgrad", "dy", dy)
    pixels, C, K = int(x.shape[0]), int(x.shape[1]), int(dy.shape[1])
    if int(dy.shape[0]) != pixels or dy.device != x.device:
        raise hip.PodError("pod_conv1x1_wgrad: x has {} pixels on {}, dy {} on {}".format(pixels, x.device, dy.shape[0], dy.device))
    lib = hip.load()
    n = int(lib.pod_conv1x1_wgrad_partials(pixels, C, K))
    if n <= 0:
        raise hip.PodError("pod_conv1x1_wgrad: pixels >= 1, C % 16 == 0, C <= 18432, K % 64 == 0 and K <= 512 required, got pixels={} C={} K={}".format(
            pixels, C, K))
    partials = torch.empty(n, dtype=torch.float32, device=x.device)
    dW = torch.empty((K, C), dtype=torch.float32, device=x.device)
    db = torch.empty((K,), dtype=torch.float32, device=x.device) if bias else None
    with torch.cuda.device(x.device):
        hip.check(lib.pod_conv1x1_wgrad(x.data_ptr(), dy.data_ptr(), pixels, C, K, amax.of(x).data_ptr(), amax.of(dy).data_ptr(), dW.data_ptr(),
                                        hip.ptr(db), partials.data_ptr(), hip.current_stream()), "pod_conv1x1_wgrad")
    return dW, db


def _record_of(out: torch.Tensor, record: Optional[torch.Tensor]) -> torch.Tensor:
    """The record a gather max'es into: the caller's (one record over the images of a batch: the caller attaches it) or a fresh one."""
    return amax.produced(out) if record is None else record


def col2im3x3s2_cl(dcols: torch.Tensor, h: int, w: int, gate: Optional[torch.Tensor] = None, add: Optional[torch.Tensor] = None,
                   out: Optional[torch.Tensor] = None, record: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The input gradient of pod_im2col3x3s2_cl for one (h, w) image: dcols (ho * wo, 9 C) -> dx (h * w, C) = (gate > 0) * gathered sum + add."""
    _cl("pod_col2im3x3s2_cl", "dcols", dcols)
    ho, wo = (int(h) - 1) // 2 + 1, (int(w) - 1) // 2 + 1
    if h < 1 or w < 1 or int(dcols.shape[1]) % 36 or int(dcols.shape[0]) != ho * wo:
        raise hip.PodError("pod_col2im3x3s2_cl: a {} x {} map has ({}, 9 C) patch rows with C % 4 == 0, got {}".format(h, w, ho * wo, tuple(dcols.shape)))
    C = int(dcols.shape[1]) // 9
    dx = torch.empty((h * w, C), dtype=torch.float32, device=dcols.device) if out is None else out
    for what, t in (("gate", gate), ("add", add), ("dx", dx)):
        if t is not None:
            _cl("pod_col2im3x3s2_cl", what, t)
            if tuple(t.shape) != (h * w, C) or t.device != dcols.device:
                raise hip.PodError("pod_col2im3x3s2_cl: {} must be ({}, {}) on {}, got {} on {}".format(what, h * w, C, dcols.device, tuple(t.shape), t.device))
    with torch.cuda.device(dcols.device):
        hip.check(hip.load().pod_col2im3x3s2_cl(dcols.data_ptr(), hip.ptr(gate), hip.ptr(add), dx.data_ptr(), int(h), int(w), C,
                                                _record_of(dx, record).data_ptr(), hip.current_stream()), "pod_col2im3x3s2_cl")
    return dx


def upsample2_sum_cl(d_child: torch.Tensor, h: int, w: int, add: torch.Tensor, out: Optional[torch.Tensor] = None,
                     record: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The backward of FPN's nearest top-down sum at factor two: d_child (h * w, C) -> d_top (((h + 1) // 2) * ((w + 1) // 2), C) = add + the
    sum of each pixel's children.  out: None = in place on `add`."""
    _cl("pod_upsample2_sum_cl", "d_child", d_child)
    _cl("pod_upsample2_sum_cl", "add", add)
    d_top = add if out is None else out
    _cl("pod_upsample2_sum_cl", "d_top", d_top)
    ht, wt, C = (int(h) + 1) // 2, (int(w) + 1) // 2, int(d_child.shape[1])
    if h < 1 or w < 1 or C % 4 or int(d_child.shape[0]) != h * w or tuple(add.shape) != (ht * wt, C) or tuple(d_top.shape) != (ht * wt, C) \
            or add.device != d_child.device or d_top.device != d_child.device:
        raise hip.PodError("pod_upsample2_sum_cl: a {} x {} child of C % 4 == 0 channels sums into ({}, C), got child {} add {} out {}".format(
            h, w, ht * wt, tuple(d_child.shape), tuple(add.shape), tuple(d_top.shape)))
    with torch.cuda.device(d_child.device):
        hip.check(hip.load().pod_upsample2_sum_cl(d_child.data_ptr(), int(h), int(w), add.data_ptr(), d_top.data_ptr(), C,
                                                  _record_of(d_top, record).data_ptr(), hip.current_stream()), "pod_upsample2_sum_cl")
    return d_top


def conv1x1_wgrad_strided(x: torch.Tensor, dy: torch.Tensor, images: int, h: int, w: int, stride: int = 1, bias: bool = False):
    """x (images * h * w, C), dy (images * ho * wo, K), channels-last, ho = (h - 1) // stride + 1: (dW (K, C), db (K,) or None) in fp32,
    dW[k][c] = sum over (b, oy, ox) of dy[(b, oy, ox)][k] x[b h w + stride oy w + stride ox][c] -- the weight gradient of a 1x1 convolution of
    stride 1 or 2 with up to 2048 output channels (the bottlenecks' conv1 / conv3 / shortcut).  The rows the stride selects are gathered in
    the kernel.  The operands' abs-max records are their producers' (pod_compare_amd.amax), else computed now."""
    _cl("pod_conv1x1_wgrad_strided", "x", x)
    _cl("pod_conv1x1_wgrad_strided", "dy", dy)
    images, h, w, stride = int(images), int(h), int(w), int(stride)
    C, K = int(x.shape[1]), int(dy.shape[1])
    lib = hip.load()
    n = int(lib.pod_conv1x1_wgrad_strided_partials(images, h, w, stride, C, K))
    if n <= 0:
        raise hip.PodError("pod_conv1x1_wgrad_strided: images >= 1, stride 1 or 2, C % 16 == 0, C <= 18432, K % 64 == 0 and K <= 2048 required, got "
                           "images={} {} x {} stride={} C={} K={}".format(images, h, w, stride, C, K))
    ho, wo = (h - 1) // stride + 1, (w - 1) // stride + 1
    if int(x.shape[0]) != images * h * w or int(dy.shape[0]) != images * ho * wo or dy.device != x.device:
        raise hip.PodError("pod_conv1x1_wgrad_strided: {} images of {} x {} at stride {} pair {} rows of x with {} of dy, got {} on {} and {} on {}".format(
            images, h, w, stride, images * h * w, images * ho * wo, x.shape[0], x.device, dy.shape[0], dy.device))
    partials = torch.empty(n, dtype=torch.float32, device=x.device)
    dW = torch.empty((K, C), dtype=torch.float32, device=x.device)
    db = torch.empty((K,), dtype=torch.float32, device=x.device) if bias else None
    with torch.cuda.device(x.device):
        hip.check(lib.pod_conv1x1_wgrad_strided(x.data_ptr(), dy.data_ptr(), images, h, w, stride, C, K, amax.of(x).data_ptr(), amax.of(dy).data_ptr(),
                                                dW.data_ptr(), hip.ptr(db), partials.data_ptr(), hip.current_stream()), "pod_conv1x1_wgrad_strided")
    return dW, db


def subsample2_scatter_cl(d_small: torch.Tensor, h: int, w: int, gate: Optional[torch.Tensor] = None, add: Optional[torch.Tensor] = None,
                          out: Optional[torch.Tensor] = None, record: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The input gradient of a stride-2 pixel selection for one (h, w) image: d_small (ho * wo, C) -> dx (h * w, C) = (gate > 0) * (d_small on
    the pixels with even coordinates, zero elsewhere, + add).  out may be `add`."""
    _cl("pod_subsample2_scatter_cl", "d_small", d_small)
    h, w = int(h), int(w)
    ho, wo, C = (h - 1) // 2 + 1, (w - 1) // 2 + 1, int(d_small.shape[1])
    if h < 1 or w < 1 or C % 4 or int(d_small.shape[0]) != ho * wo:
        raise hip.PodError("pod_subsample2_scatter_cl: a {} x {} map has ({}, C) selected rows with C % 4 == 0, got {}".format(h, w, ho * wo, tuple(d_small.shape)))
    dx = torch.empty((h * w, C), dtype=torch.float32, device=d_small.device) if out is None else out
    for what, t in (("gate", gate), ("add", add), ("dx", dx)):
        if t is not None:
            _cl("pod_subsample2_scatter_cl", what, t)
            if tuple(t.shape) != (h * w, C) or t.device != d_small.device:
                raise hip.PodError("pod_subsample2_scatter_cl: {} must be ({}, {}) on {}, got {} on {}".format(what, h * w, C, d_small.device, tuple(t.shape), t.device))
    with torch.cuda.device(d_small.device):
        hip.check(hip.load().pod_subsample2_scatter_cl(d_small.data_ptr(), hip.ptr(gate), hip.ptr(add), dx.data_ptr(), h, w, C,
                                                       _record_of(dx, record).data_ptr(), hip.current_stream()), "pod_subsample2_scatter_cl")
    return dx
