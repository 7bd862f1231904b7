"""Synthetic corruptions of the decoded frame on the device (csrc/k35_corrupt_u8.hip, C ABI pod_corrupt_*): the controlled data-set shift
of the study, after Hendrycks and Dietterich's ImageNet-C -- eight kinds at five severities, applied to the uint8 (h, w, 3) RGB frame at
its own size, before the loader's resize (K20).  Nothing in the reference does this: it measures shift with other data sets.

The table below is this project's (constants after ImageNet-C's); no package that implements the corruptions is a dependency, and parity
with one is not claimed.  A corrupted frame is a pure function of (frame bytes, name, severity, key).  The filters' tables are
built here in fp64, rounded to fp32 and kept on the device."""
import ctypes
import math
from typing import Dict, Optional, Tuple

import numpy as np
import torch

from . import hip

NAMES = ("gaussian_noise", "speckle_noise", "impulse_noise", "gaussian_blur", "defocus_blur", "brightness", "contrast", "saturate")
SEVERITY = {      # name -> the parameter of severity 1..5
    "gaussian_noise": (0.08, 0.12, 0.18, 0.26, 0.38),                                   # sigma
    "speckle_noise": (0.15, 0.2, 0.35, 0.45, 0.6),                                      # c
    "impulse_noise": (0.03, 0.06, 0.09, 0.17, 0.27),                                    # amount
    "gaussian_blur": (1, 2, 3, 4, 6),                                                   # sigma
    "defocus_blur": ((3, 0.1), (4, 0.5), (6, 0.5), (8, 0.5), (10, 0.5)),                # (radius, alias sigma)
    "brightness": (0.1, 0.2, 0.3, 0.4, 0.5),                                            # c
    "contrast": (0.4, 0.3, 0.2, 0.1, 0.05),                                             # c
    "saturate": ((0.3, 0), (0.1, 0), (2, 0), (5, 0.1), (20, 0.2)),                      # (c0, c1)
}
KINDS = {n: k for k, n in enumerate(NAMES)}            # include/pod_mi355x.h: POD_CORRUPT_*
STREAM_CORRUPT = 0x636f7200                            # the counter's 4th word ("cor"), DESIGN 19
GAUSS_MAX_RADIUS, DEFOCUS_MAX_RADIUS = 24, 12
_tables: Dict[tuple, Optional[torch.Tensor]] = {}      # (name, severity, device) -> the filter's fp32 taps on the device (40 entries at most)


def parameters(name: str, severity: int):
    """The table's entry: a number, or a pair for defocus_blur and saturate."""
    if name not in SEVERITY:
        raise ValueError("unknown corruption %r: one of %s" % (name, ", ".join(NAMES)))
    if isinstance(severity, bool) or not isinstance(severity, int) or not 1 <= severity <= 5:
        raise ValueError("severity %r of %s: one of 1, 2, 3, 4, 5" % (severity, name))
    return SEVERITY[name][severity - 1]


def gaussian_taps(sigma: float) -> np.ndarray:
    """exp(-k^2 / (2 sigma^2)), k = -r .. r, r = min(int(4 sigma + 0.5), 24), normalised to sum 1 (fp64): scipy's truncate=4.0 kernel."""
    r = min(int(4.0 * float(sigma) + 0.5), GAUSS_MAX_RADIUS)
    k = np.arange(-r, r + 1, dtype=np.float64)
    t = np.exp(-(k * k) / (2.0 * float(sigma) * float(sigma)))
    return t / t.sum()


def _reflect101(i: int, n: int) -> int:
    if n == 1:
        return 0
    p = 2 * (n - 1)
    i %= p
    return i if i < n else p - i


def defocus_stencil(radius: int, alias: float) -> np.ndarray:
    """The disk of `radius` on the grid [-L, L]^2 (L = 8 for radius <= 8, else radius), normalised, blurred by a k x k Gaussian of sigma
    `alias` (k = 3 for radius <= 8, else 5; reflect-101 borders inside the grid) and normalised to sum 1 again (fp64)."""
    radius = int(radius)
    L = 8 if radius <= 8 else radius
    k = 3 if radius <= 8 else 5
    c = np.arange(-L, L + 1, dtype=np.float64)
    disk = ((c[None, :] ** 2 + c[:, None] ** 2) <= float(radius) ** 2).astype(np.float64)
    disk /= disk.sum()
    g = np.exp(-((np.arange(k, dtype=np.float64) - (k - 1) / 2.0) ** 2) / (2.0 * float(alias) * float(alias)))
    g /= g.sum()
    n = 2 * L + 1
    idx = np.array([[_reflect101(i + j - (k - 1) // 2, n) for j in range(k)] for i in range(n)])       # (n, k): the source of tap j at i
    out, c = disk, (k - 1) // 2
    for axis in (0, 1):       # the two neighbours at one distance are added first: the pass is exactly symmetric under a flip
        acc = g[c] * np.take(out, idx[:, c], axis=axis)
        for j in range(1, c + 1):
            acc = acc + g[c + j] * (np.take(out, idx[:, c - j], axis=axis) + np.take(out, idx[:, c + j], axis=axis))
        out = acc
    out = 0.5 * (out + out.T)      # ... and under the transpose, whichever axis went first
    return out / out.sum()


def corruption_key(seed: int, index: int) -> int:
    """The noises' Philox key: (seed & 0xFFFFFFFF) | (index & 0xFFFFFFFF) << 32, index = the image's position in the json's `images`."""
    return (int(seed) & 0xFFFFFFFF) | ((int(index) & 0xFFFFFFFF) << 32)


def impulse_threshold(amount: float) -> int:
    """An element flips iff its 32-bit word is below min(floor(amount 2^32), 2^32 - 1) (fp64)."""
    return min(int(math.floor(float(amount) * 4294967296.0)), 4294967295)


def filter_table(name: str, severity: int) -> Tuple[int, Optional[np.ndarray]]:
    """(radius, the fp32 taps the device reads) of a filter kind; (0, None) for the other kinds."""
    p = parameters(name, severity)
    if name == "gaussian_blur":
        t = gaussian_taps(p)
        return (len(t) - 1) // 2, t.astype(np.float32)
    if name == "defocus_blur":
        s = defocus_stencil(*p)
        return (s.shape[0] - 1) // 2, np.ascontiguousarray(s, dtype=np.float32)
    return 0, None


def _device_table(name: str, severity: int, device: torch.device):
    key = (name, severity, device.type, device.index if device.index is not None else torch.cuda.current_device())
    if key not in _tables:
        radius, taps = filter_table(name, severity)
        t = None
        if taps is not None:
            t = torch.from_numpy(taps).to(device)
            torch.cuda.current_stream(device).synchronize()      # uploaded on this stream, read from any
        _tables[key] = (radius, t)
    return _tables[key]


def record(name: str, severity: int, key: int, device: torch.device) -> "hip.PodCorruption":
    """The C ABI's record of (name, severity, key); a filter's taps are the cached device table, which lives as long as the process."""
    p = parameters(name, severity)
    radius, taps = _device_table(name, severity, device)
    pair = p if isinstance(p, tuple) else (p, 0.0)
    return hip.PodCorruption(kind=KINDS[name], radius=radius, p0=float(pair[0]), p1=float(pair[1]), taps=None if taps is None else taps.data_ptr(),
                             impulse_threshold=impulse_threshold(p) if name == "impulse_noise" else 0, reserved=0, key=int(key) & 0xFFFFFFFFFFFFFFFF)


def corrupt_frame_u8(frame_hwc_u8: torch.Tensor, name: str, severity: int, key: int, stream: Optional[int] = None) -> torch.Tensor:
    """frame (h, w, 3) uint8 RGB on the device (rows may be padded) -> the corrupted frame, (h, w, 3) uint8 contiguous, on the device.
    key: corruption_key(seed, index) -- only the noises read it.  stream: a HIP stream handle (default: torch's current stream)."""
    parameters(name, severity)
    f = frame_hwc_u8
    if not (f.is_cuda and f.dtype == torch.uint8 and f.dim() == 3 and f.shape[2] == 3):
        raise ValueError("corrupt_frame_u8 needs a (h, w, 3) uint8 tensor on the device, got {} {} on {}".format(tuple(f.shape), f.dtype, f.device))
    h, w = int(f.shape[0]), int(f.shape[1])
    if f.stride(2) != 1 or f.stride(1) != 3 or (h > 1 and f.stride(0) < 3 * w):
        f = f.contiguous()
    lib = hip.load()
    with torch.cuda.device(f.device):
        rec = record(name, severity, key, f.device)
        need = int(lib.pod_corrupt_scratch_bytes(rec.kind, h, w))
        scratch = torch.empty(((need + 7) // 8,), dtype=torch.int64, device=f.device) if need else None
        out = torch.empty((h, w, 3), dtype=torch.uint8, device=f.device)
        rc = lib.pod_corrupt_frame_u8(f.data_ptr(), h, w, f.stride(0) if h > 1 else 3 * w, out.data_ptr(), 3 * w, ctypes.byref(rec),
                                      None if scratch is None else scratch.data_ptr(), need, hip.current_stream() if stream is None else stream)
    hip.check(rc, "pod_corrupt_frame_u8")
    return out
