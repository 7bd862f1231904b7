"""Host side of K22 (csrc/k22_conv3x3_wgrad.hip): the weight / bias gradients of a 3x3 / stride-1 / pad-1 convolution and the
ReLU + dropout gate of the head's backward pass (probabilistic_retinanet.py:403-484 under train_net.py's loop).  GPU only: there is no
CPU path."""
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
