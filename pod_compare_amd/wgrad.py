"""Host side of K22 (csrc/k22_conv3x3_wgrad.hip): the weight / bias gradients of a 3x3 / stride-1 / pad-1 convolution and the
ReLU + dropout gate of the head's backward pass (probabilistic_retinanet.py:403-484 under train_net.py's loop) -- and of K23
(csrc/k23_fpn_backward.hip): the weight gradient without taps and the two gathers of the FPN's backward pass -- and of K24
(csrc/k24_resnet_backward.hip): the 1x1 weight gradient at the backbone's widths and strides and the scatter that undoes a stride-2 pixel
selection -- and of K30 (csrc/k30_stem_backward.hip): the stem's 7x7 weight gradient and the max-pool's backward.  GPU only: there is no CPU path."""
import ctypes
from typing import Optional, Sequence, Tuple

import torch

from . import amax, conv1x1, hip

_STEM_BOUNDS: dict = {}     # conv1x1.normalised_input_bound's constants per (mean, std), for callers without a Stem7x7 of their own


def _level_array(levels: Sequence[Tuple[int, int]]):
    arr = (ctypes.c_int32 * (2 * len(levels)))()
    for i, (h, w) in enumerate(levels):
        arr[2 * i], arr[2 * i + 1] = int(h), int(w)
    return arr


def conv3x3_wgrad(x: torch.Tensor, dy: torch.Tensor, levels: Sequence[Tuple[int, int]], copies: int, K: int):
    """x (pixels, C), dy (pixels, Kpad): channels-last, `copies` images per level, level-major (wino.level_pixel_offsets).  Returns
    (dW (K, C, 3, 3), db (K,)) in fp32.  The operands' abs-max records are their producers' (pod_compare_amd.amax), else computed now."""
    _cl("pod_conv3x3_wgrad", "x", x)
    _cl("pod_conv3x3_wgrad", "dy", dy)
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


def _c1w(name: str, x: torch.Tensor, dy: torch.Tensor, geometry: tuple, bias: bool, refusal: str):
    """The allocation and call behind conv1x1_wgrad and conv1x1_wgrad_strided: entry `name` takes `geometry` between dy and C; what
    `name`_partials(*geometry, C, K) answers with 0, the entry refuses: PodError(refusal)."""
    C, K, lib = int(x.shape[1]), int(dy.shape[1]), hip.load()
    n = int(getattr(lib, name + "_partials")(*geometry, C, K))
    if n <= 0:
        raise hip.PodError(refusal)
    partials = torch.empty(n, dtype=torch.float32, device=x.device)
    dW = torch.empty((K, C), dtype=torch.float32, device=x.device)
    db = torch.empty((K,), dtype=torch.float32, device=x.device) if bias else None
    with torch.cuda.device(x.device):
        hip.check(getattr(lib, name)(x.data_ptr(), dy.data_ptr(), *geometry, C, K, amax.of(x).data_ptr(), amax.of(dy).data_ptr(), dW.data_ptr(), hip.ptr(db),
                                     partials.data_ptr(), hip.current_stream()), name)
    return dW, db


def conv1x1_wgrad(x: torch.Tensor, dy: torch.Tensor, bias: bool = True):
    """x (pixels, C), dy (pixels, K), channels-last: (dW (K, C), db (K,) or None) in fp32, dW[k][c] = sum_p dy[p][k] x[p][c].  The weight
    gradient of a 1x1 convolution and, on the patch matrix of pod_im2col3x3s2_cl, of a 3x3 / stride-2 one laid out (K, ty, tx, Cin).  The
    operands' abs-max records are their producers' (pod_compare_amd.amax), else computed now."""
    _cl("pod_conv1x1_wgrad", "x", x)
    _cl("pod_conv1x1_wgrad", "dy", dy)
    pixels = int(x.shape[0])
    if int(dy.shape[0]) != pixels or dy.device != x.device:
        raise hip.PodError("pod_conv1x1_wgrad: x has {} pixels on {}, dy {} on {}".format(pixels, x.device, dy.shape[0], dy.device))
    return _c1w("pod_conv1x1_wgrad", x, dy, (pixels,), bias,
                "pod_conv1x1_wgrad: pixels >= 1, C % 16 == 0, C <= 18432, K % 64 == 0 and K <= 512 required, got pixels={} C={} K={}".format(
                    pixels, x.shape[1], dy.shape[1]))


def _map_gather(name: str, src: torch.Tensor, h: int, w: int, C: int, rule: str, gate, add, out, record, call=None) -> torch.Tensor:
    """The call behind col2im3x3s2_cl, subsample2_scatter_cl and maxpool3x3s2_backward_cl: entry `name` gathers the ho * wo rows of src, which
    hold C channels each (0: they cannot; `rule` names what they should be), into dx (h * w, C).  record: the caller's (one over a batch's
    images, which the caller attaches: over_images), None = dx's own.  call(lib, dx, record): an entry with arguments of its own."""
    h, w = int(h), int(w)
    rows = ((h - 1) // 2 + 1) * ((w - 1) // 2 + 1)
    if h < 1 or w < 1 or C < 1 or C % 4 or int(src.shape[0]) != rows:
        raise hip.PodError("{}: a {} x {} map has {} with C % 4 == 0, got {}".format(name, h, w, rule.format(rows), tuple(src.shape)))
    dx = torch.empty((h * w, C), dtype=torch.float32, device=src.device) if out is None else out
    for what, t in (("gate", gate), ("add", add), ("dx", dx)):
        if t is not None:
            _cl(name, what, t)
            if tuple(t.shape) != (h * w, C) or t.device != src.device:
                raise hip.PodError("{}: {} must be ({}, {}) on {}, got {} on {}".format(name, what, h * w, C, src.device, tuple(t.shape), t.device))
    with torch.cuda.device(src.device):
        rec = amax.produced(dx) if record is None else record
        if call is not None:
            hip.check(call(hip.load(), dx, rec), name)
        else:
            hip.check(getattr(hip.load(), name)(src.data_ptr(), hip.ptr(gate), hip.ptr(add), dx.data_ptr(), h, w, C, rec.data_ptr(), hip.current_stream()), name)
    return dx


def over_images(B: int, out: torch.Tensor, op) -> torch.Tensor:
    """A per-image gather on the B images of a batch under ONE abs-max record, attached to `out`: op(b, rows, record) for every image b;
    rows(t): image b's rows of a tensor that stacks the B images."""
    rec = amax.word(out.device)
    for b in range(B):
        op(b, lambda t: t[b * (int(t.shape[0]) // B):(b + 1) * (int(t.shape[0]) // B)], rec)
    return amax.attach(out, rec)


def require_maps(who: str, maps, channels: Optional[int] = None, device=None) -> None:
    """maps: per image the (t, h, w) a training pass starts from (channels, device: None = the first map's)."""
    t0, h0, w0 = maps[0]
    for t, h, w in maps:
        if not (torch.is_tensor(t) and torch.is_tensor(t0) and t.is_cuda and t.device == (t0.device if device is None else device) and t.dtype == torch.float32
                and t.is_contiguous() and t.dim() == 2 and tuple(t.shape) == (int(h) * int(w), int(t0.shape[1]) if channels is None else channels)
                and (int(h), int(w)) == (int(h0), int(w0))):
            raise hip.PodError("{} runs on contiguous fp32 channels-last (h * w, C) maps of one size on one GPU: there is no CPU path".format(who))


def col2im3x3s2_cl(dcols: torch.Tensor, h: int, w: int, gate: Optional[torch.Tensor] = None, add: Optional[torch.Tensor] = None,
                   out: Optional[torch.Tensor] = None, record: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The input gradient of pod_im2col3x3s2_cl for one (h, w) image: dcols (ho * wo, 9 C) -> dx (h * w, C) = (gate > 0) * gathered sum + add."""
    _cl("pod_col2im3x3s2_cl", "dcols", dcols)
    C9 = int(dcols.shape[1])
    return _map_gather("pod_col2im3x3s2_cl", dcols, h, w, 0 if C9 % 36 else C9 // 9, "({}, 9 C) patch rows", gate, add, out, record)


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
                                                  (amax.produced(d_top) if record is None else record).data_ptr(), hip.current_stream()), "pod_upsample2_sum_cl")
    return d_top


def conv1x1_wgrad_strided(x: torch.Tensor, dy: torch.Tensor, images: int, h: int, w: int, stride: int = 1, bias: bool = False):
    """x (images * h * w, C), dy (images * ho * wo, K), channels-last, ho = (h - 1) // stride + 1: (dW (K, C), db (K,) or None) in fp32,
    dW[k][c] = sum over (b, oy, ox) of dy[(b, oy, ox)][k] x[b h w + stride oy w + stride ox][c] -- the weight gradient of a 1x1 convolution of
    stride 1 or 2 with up to 2048 output channels (the bottlenecks' conv1 / conv3 / shortcut).  The rows the stride selects are gathered in
    the kernel.  The operands' abs-max records are their producers' (pod_compare_amd.amax), else computed now."""
    _cl("pod_conv1x1_wgrad_strided", "x", x)
    _cl("pod_conv1x1_wgrad_strided", "dy", dy)
    images, h, w, stride = int(images), int(h), int(w), int(stride)
    if stride in (1, 2):                                # (any other the entry refuses, below)
        ho, wo = (h - 1) // stride + 1, (w - 1) // stride + 1
        if int(x.shape[0]) != images * h * w or int(dy.shape[0]) != images * ho * wo or dy.device != x.device:
            raise hip.PodError("pod_conv1x1_wgrad_strided: {} images of {} x {} at stride {} pair {} rows of x with {} of dy, got {} on {} and {} on {}".format(
                images, h, w, stride, images * h * w, images * ho * wo, x.shape[0], x.device, dy.shape[0], dy.device))
    return _c1w("pod_conv1x1_wgrad_strided", x, dy, (images, h, w, stride), bias,
                "pod_conv1x1_wgrad_strided: images >= 1, stride 1 or 2, C % 16 == 0, C <= 18432, K % 64 == 0 and K <= 2048 required, got "
                "images={} {} x {} stride={} C={} K={}".format(images, h, w, stride, x.shape[1], dy.shape[1]))


def subsample2_scatter_cl(d_small: torch.Tensor, h: int, w: int, gate: Optional[torch.Tensor] = None, add: Optional[torch.Tensor] = None,
                          out: Optional[torch.Tensor] = None, record: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The input gradient of a stride-2 pixel selection for one (h, w) image: d_small (ho * wo, C) -> dx (h * w, C) = (gate > 0) * (d_small on
    the pixels with even coordinates, zero elsewhere, + add).  out may be `add`."""
    _cl("pod_subsample2_scatter_cl", "d_small", d_small)
    return _map_gather("pod_subsample2_scatter_cl", d_small, h, w, int(d_small.shape[1]), "({}, C) selected rows", gate, add, out, record)


def stem7x7_wgrad(x: torch.Tensor, ds: torch.Tensor, padded_hw: Optional[tuple] = None, mean: Optional[torch.Tensor] = None,
                  std: Optional[torch.Tensor] = None, bound: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The gradient of the stem's folded 7x7 / stride-2 / pad-3 filter (K30, pod_stem7x7_wgrad).  x (images, 3, hi, wi) or (3, hi, wi),
    contiguous uint8 or fp32 on the GPU: the frames as conv1x1.Stem7x7 takes them, normalised on load with mean / std (3 floats each; None:
    already normalised) and zero outside (hi, wi) up to padded_hw; ds (images * ho * wo, 64) channels-last, ho = (h - 1) // 2 + 1 of the
    padded extent.  Returns dW (64, 3, 7, 7) fp32.  bound: the record that bounds the normalised input (Stem7x7._input_bound: the forward's
    in_amax; None: formed here by the same rule); ds's record is its producer's, else computed now."""
    name = "pod_stem7x7_wgrad"
    if not (torch.is_tensor(x) and x.is_cuda and x.dtype in (torch.uint8, torch.float32) and x.is_contiguous() and x.dim() in (3, 4) and int(x.shape[-3]) == 3):
        raise hip.PodError("{}: the frames must be a contiguous uint8 / fp32 (images, 3, h, w) tensor on the GPU, got {} {} on {}".format(
            name, getattr(x, "dtype", None), tuple(getattr(x, "shape", ())), getattr(x, "device", None)))
    _cl(name, "ds", ds)
    images, hi, wi = (1 if x.dim() == 3 else int(x.shape[0])), int(x.shape[-2]), int(x.shape[-1])
    h, w = (hi, wi) if padded_hw is None else (int(padded_hw[0]), int(padded_hw[1]))
    if (mean is None) != (std is None) or any(t is not None and not (t.is_cuda and t.dtype == torch.float32 and t.numel() == 3 and t.is_contiguous()) for t in (mean, std)):
        raise hip.PodError("{}: mean and std come together, 3 contiguous fp32 values each on the GPU".format(name))
    if mean is None and x.dtype != torch.float32:
        raise hip.PodError("{}: a uint8 frame is normalised on load: mean and std required".format(name))
    if bound is None:
        bound = conv1x1.normalised_input_bound(x, mean, std, _STEM_BOUNDS)
    lib = hip.load()
    n = int(lib.pod_stem7x7_wgrad_partials(images, hi, wi, h, w))
    if n <= 0:
        raise hip.PodError("{}: images >= 1 and 1 <= frame extent <= padded extent <= 16384 required (what pod_stem7x7_split accepts), got images={} "
                           "frame {} x {} padded {} x {}".format(name, images, hi, wi, h, w))
    rows = images * ((h - 1) // 2 + 1) * ((w - 1) // 2 + 1)
    if tuple(ds.shape) != (rows, 64) or ds.device != x.device:
        raise hip.PodError("{}: {} frames padded to {} x {} pair with a ({}, 64) ds on {}, got {} on {}".format(name, images, h, w, rows, x.device, tuple(ds.shape), ds.device))
    partials = torch.empty(n, dtype=torch.float32, device=x.device)
    dW = torch.empty((64, 3, 7, 7), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        hip.check(lib.pod_stem7x7_wgrad(x.data_ptr(), 1 if x.dtype == torch.uint8 else 0, images, hi, wi, hip.ptr(mean), hip.ptr(std), ds.data_ptr(), h, w,
                                        bound.data_ptr(), amax.of(ds).data_ptr(), dW.data_ptr(), partials.data_ptr(), hip.current_stream()), name)
    return dW


def maxpool3x3s2_backward_cl(s: torch.Tensor, dp: torch.Tensor, h: int, w: int, out: Optional[torch.Tensor] = None,
                             record: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The backward of conv1x1.maxpool3x3s2_cl and of the ReLU in front of it for one (h, w) image (K30): s (h * w, C), the stem's stored
    post-ReLU output; dp (hq * wq, C), hq = (h - 1) // 2 + 1 -> ds (h * w, C) = (s > 0) * the sum of dp over the windows whose arg-max the
    pixel is (torch's: the first maximum in row-major order wins)."""
    _cl("pod_maxpool3x3s2_backward_cl", "s", s)
    _cl("pod_maxpool3x3s2_backward_cl", "dp", dp)
    if dp.device != s.device or int(dp.shape[1]) != int(s.shape[1]):
        raise hip.PodError("pod_maxpool3x3s2_backward_cl: s {} on {} against dp {} on {}".format(tuple(s.shape), s.device, tuple(dp.shape), dp.device))
    return _map_gather("pod_maxpool3x3s2_backward_cl", dp, h, w, int(dp.shape[1]), "({}, C) pooled rows", s, None, out, record, call=lambda lib, dx, rec: lib.pod_maxpool3x3s2_backward_cl(
        s.data_ptr(), dp.data_ptr(), dx.data_ptr(), int(h), int(w), int(dp.shape[1]), rec.data_ptr(), hip.current_stream()))
