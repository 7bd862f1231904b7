"""The loader's resize on the device (csrc/k20_resize_u8.hip, C ABI pod_resize_*): what apply_net.CocoImages does to a decoded frame --
detectron2's ResizeShortestEdge with PIL's bilinear filter on the uint8 HWC array, RGB -> BGR, HWC -> CHW (AN:83-84) -- in one launch,
to the byte.  The coefficient tables of a geometry are computed once on the host (Pillow's fp64 arithmetic) and kept on the device."""
import ctypes
from collections import OrderedDict
from typing import Optional, Tuple

import numpy as np
import torch

from . import anchors, hip

MAX_TABLES = 16        # geometries kept per process, as the model keeps 16 graphs: a data set has few frame sizes
_tables: "OrderedDict[tuple, tuple]" = OrderedDict()


def axis_tables(in_size: int, out_size: int) -> Tuple[np.ndarray, np.ndarray]:
    """Host tables of one axis: bounds (out, 2) int32 = (first source index, taps used), coeffs (out, ksize) int32 in 22-bit fixed point."""
    lib = hip.load()
    k = lib.pod_resize_taps(in_size, out_size)
    if k < 0:
        hip.check(k, "pod_resize_taps")
    bounds = np.zeros((out_size, 2), dtype=np.int32)
    coeffs = np.zeros((out_size, k), dtype=np.int32)
    hip.check(lib.pod_resize_coeffs(in_size, out_size, bounds.ctypes.data_as(ctypes.c_void_p), coeffs.ctypes.data_as(ctypes.c_void_p)),
              "pod_resize_coeffs")
    return bounds, coeffs


def _device_tables(h: int, w: int, nh: int, nw: int, device: torch.device):
    """((xbounds, xcoeffs, xk), (ybounds, ycoeffs, yk)) on `device`; an axis that keeps its size has (None, None, 0): its pass is skipped."""
    key = (h, w, nh, nw, device.type, device.index if device.index is not None else torch.cuda.current_device())
    ent = _tables.get(key)
    if ent is not None:
        _tables.move_to_end(key)
        return ent
    if len(_tables) >= MAX_TABLES:
        torch.cuda.synchronize(device)          # a launch that reads the oldest tables may still be queued on some stream
        _tables.popitem(last=False)
    ent = []
    for a, b in ((w, nw), (h, nh)):
        if a == b:
            ent.append((None, None, 0))
            continue
        bounds, coeffs = axis_tables(a, b)
        ent.append((torch.from_numpy(bounds).to(device), torch.from_numpy(coeffs).to(device), coeffs.shape[1]))
    torch.cuda.current_stream(device).synchronize()      # uploaded on this stream, read from any
    _tables[key] = ent = tuple(ent)
    return ent


def resize_frame_u8(frame_hwc_u8: torch.Tensor, min_size: int, max_size: int, bgr: bool = True, stream: Optional[int] = None) -> torch.Tensor:
    """frame (h, w, 3) uint8 RGB on the device (rows may be padded: stride(0) >= 3 w) -> (3, nh, nw) uint8, (nh, nw) =
    anchors.resize_shortest_edge(h, w, min_size, max_size), channels flipped to BGR unless bgr=False.  Equal to the host path's
    `Image.resize((nw, nh), Image.BILINEAR)` + flip + transpose bit for bit; a frame that keeps its size is still flipped and transposed
    on the device.  stream: a HIP stream handle (default: torch's current stream)."""
    f = frame_hwc_u8
    if not (f.is_cuda and f.dtype == torch.uint8 and f.dim() == 3 and f.shape[2] == 3):
        raise ValueError("resize_frame_u8 needs a (h, w, 3) uint8 tensor on the device, got {} {} on {}".format(tuple(f.shape), f.dtype, f.device))
    h, w = int(f.shape[0]), int(f.shape[1])
    if f.stride(2) != 1 or f.stride(1) != 3 or (h > 1 and f.stride(0) < 3 * w):
        f = f.contiguous()
    nh, nw = anchors.resize_shortest_edge(h, w, min_size, max_size)
    (xb, xc, xk), (yb, yc, yk) = _device_tables(h, w, nh, nw, f.device)
    out = torch.empty((3, nh, nw), dtype=torch.uint8, device=f.device)
    p = lambda t: None if t is None else t.data_ptr()
    rc = hip.load().pod_resize_frame_u8(f.data_ptr(), h, w, f.stride(0) if h > 1 else 3 * w, p(xb), p(xc), xk, p(yb), p(yc), yk, out.data_ptr(),
                                        nh, nw, 1 if bgr else 0, hip.current_stream() if stream is None else stream)
    hip.check(rc, "pod_resize_frame_u8")
    return out
