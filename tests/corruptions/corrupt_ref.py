"""Host reference of the corruptions (K35), fp64, independent of pod_compare_amd/corruptions.py and the HIP code: numpy expressions of
DESIGN 11a, scipy for the two filters, Philox and box_muller16 from tests/rng/rng_ref.py with the corruption stream's counter map written
out here (rng_ref's own table of streams is not edited: this file restates the new row of DESIGN 19).

`corrupt` is the referee.  `corrupt_fp32` restates the four kinds whose device arithmetic is fp32 -- the two noises and the two blurs -- in
numpy fp32: test_corruptions_cpu.py shows with it that fp32 against fp64 stays inside the GPU tests' cap with room to spare."""
import functools

import numpy as np
from scipy import ndimage

from tests.rng import rng_ref

NAMES = ("gaussian_noise", "speckle_noise", "impulse_noise", "gaussian_blur", "defocus_blur", "brightness", "contrast", "saturate")
TABLE = {
    "gaussian_noise": (0.08, 0.12, 0.18, 0.26, 0.38),
    "speckle_noise": (0.15, 0.2, 0.35, 0.45, 0.6),
    "impulse_noise": (0.03, 0.06, 0.09, 0.17, 0.27),
    "gaussian_blur": (1, 2, 3, 4, 6),
    "defocus_blur": ((3, 0.1), (4, 0.5), (6, 0.5), (8, 0.5), (10, 0.5)),
    "brightness": (0.1, 0.2, 0.3, 0.4, 0.5),
    "contrast": (0.4, 0.3, 0.2, 0.1, 0.05),
    "saturate": ((0.3, 0), (0.1, 0), (2, 0), (5, 0.1), (20, 0.2)),
}
EXACT = ("brightness", "contrast", "saturate", "impulse_noise")
CAPPED = ("gaussian_noise", "speckle_noise", "gaussian_blur", "defocus_blur")
STREAM_CORRUPT = 0x636f7200
SEED = 7

# the GPU tests' frames: smaller than every stencil; odd sizes; rows 13 bytes apart on the device; several tiles on both axes
FRAMES = ((3, 5), (37, 53), (48, 80), (130, 70))
SEVERITIES = (1, 3, 5)
CAP_BYTE, CAP_SHARE = 1, 1e-3          # capped kinds: no byte differs by more than 1; at most 1 byte in 1 000 differs over the four frames


def frame(hw, seed=0):
    return np.random.default_rng(1000 * hw[0] + hw[1] + seed).integers(0, 256, size=(hw[0], hw[1], 3), dtype=np.uint8)


def key_of(seed, index):
    return (int(seed) & 0xFFFFFFFF) | ((int(index) & 0xFFFFFFFF) << 32)


def quantise(v):
    return np.floor(np.minimum(np.maximum(v, 0.0), 1.0) * 255.0 + 0.5).astype(np.uint8)


# ---- the counter map: (c0, c1, c2, c3) = (x, y, call, STREAM_CORRUPT), x, y the pixel of the decoded frame ----------------------------
def counter(h, w, call):
    c = np.zeros((h, w, 4), dtype=np.uint32)
    c[..., 0] = np.arange(w, dtype=np.uint32)[None, :]
    c[..., 1] = np.arange(h, dtype=np.uint32)[:, None]
    c[..., 2] = call
    c[..., 3] = STREAM_CORRUPT
    return c


def words(h, w, call, key):
    return rng_ref.philox4x32_10(counter(h, w, call), rng_ref.key_words(key))


def normals(h, w, key):
    """(h, w, 3) fp64: the normal of channel ch is component ch of call 0 -- normal ch & 1 of output word ch >> 1."""
    out = words(h, w, 0, key)
    a0, a1 = rng_ref.box_muller16(out[..., 0])
    b0, _ = rng_ref.box_muller16(out[..., 1])
    return np.stack([a0, a1, b0], axis=-1)


def impulse_threshold(amount):
    return min(int(np.floor(np.float64(amount) * np.float64(4294967296.0))), 4294967295)


# ---- the filters' tables, built here on their own ------------------------------------------------------------------------------------
def gaussian_kernel(sigma):
    """scipy's own kernel: a unit impulse through gaussian_filter1d."""
    r = int(4.0 * sigma + 0.5)
    e = np.zeros(2 * r + 1)
    e[r] = 1.0
    return ndimage.gaussian_filter1d(e, sigma, mode="constant", truncate=4.0)


def stencil(radius, alias):
    L = 8 if radius <= 8 else radius
    k = 3 if radius <= 8 else 5
    y, x = np.mgrid[-L:L + 1, -L:L + 1]
    disk = (x * x + y * y <= radius * radius).astype(np.float64)
    disk /= disk.sum()
    g = np.exp(-(np.arange(k) - (k - 1) / 2.0) ** 2 / (2.0 * alias ** 2))
    g /= g.sum()
    out = ndimage.correlate1d(ndimage.correlate1d(disk, g, axis=0, mode="mirror"), g, axis=1, mode="mirror")
    return out / out.sum()


# ---- fp64 -----------------------------------------------------------------------------------------------------------------------------
def _hsv(x, name, c0, c1):
    r, g, b = (x[..., i].astype(np.float64) / 255.0 for i in range(3))
    V = np.maximum(np.maximum(r, g), b)
    m = np.minimum(np.minimum(r, g), b)
    d = V - m
    with np.errstate(divide="ignore", invalid="ignore"):
        S = np.where(V > 0, d / V, 0.0)
        hr = (g - b) / d
        hr = np.where(hr < 0, hr + 6.0, hr)
        hg = 2.0 + (b - r) / d
        hb = 4.0 + (r - g) / d
    h6 = np.where(d == 0, 0.0, np.where(V == r, hr, np.where(V == g, hg, hb)))
    if name == "brightness":
        V = np.minimum(V + c0, 1.0)
    else:
        S = np.minimum(np.maximum(S * c0 + c1, 0.0), 1.0)
    fl = np.floor(h6)
    f = h6 - fl
    i = fl.astype(np.int64) % 6
    p, q, t = V * (1.0 - S), V * (1.0 - f * S), V * (1.0 - (1.0 - f) * S)
    R = np.choose(i, [V, q, p, p, t, V])
    G = np.choose(i, [t, V, V, q, p, p])
    B = np.choose(i, [p, p, t, V, V, q])
    return quantise(np.stack([R, G, B], axis=-1))


def corrupt(x, name, severity, key=0):
    """x (h, w, 3) uint8 -> (h, w, 3) uint8, fp64 throughout."""
    p = TABLE[name][severity - 1]
    h, w = x.shape[:2]
    xf = x.astype(np.float64) / 255.0
    if name == "gaussian_noise":
        return quantise(xf + p * normals(h, w, key))
    if name == "speckle_noise":
        return quantise(xf + xf * p * normals(h, w, key))
    if name == "impulse_noise":
        out = words(h, w, 1, key).astype(np.uint64)
        flip = out[..., :3] < np.uint64(impulse_threshold(p))
        high = ((out[..., 3:4] >> np.arange(3, dtype=np.uint64)) & np.uint64(1)) == 1
        return np.where(flip, np.where(high, 255, 0), x).astype(np.uint8)
    if name == "gaussian_blur":
        return quantise(ndimage.gaussian_filter(xf, sigma=(p, p, 0), mode="nearest", truncate=4.0))
    if name == "defocus_blur":
        s = stencil(*p)
        return quantise(np.stack([ndimage.correlate(xf[..., c], s, mode="mirror") for c in range(3)], axis=-1))
    if name == "contrast":
        mean = x.reshape(-1, 3).astype(np.int64).sum(axis=0).astype(np.float64) / (255.0 * (h * w))
        return quantise((xf - mean) * p + mean)
    if name in ("brightness", "saturate"):
        c0, c1 = p if isinstance(p, tuple) else (p, 0.0)
        return _hsv(x, name, float(c0), float(c1))
    raise KeyError(name)


# ---- fp32 restatement of the capped kinds -----------------------------------------------------------------------------------------------
def _quantise32(v):
    f = np.float32
    return np.floor(np.minimum(np.maximum(v, f(0)), f(1)) * f(255) + f(0.5)).astype(np.uint8)


def _taps_along(a, taps, axis, mode):
    """sum_k taps[k] a[i + k - r] along `axis` in fp32, taps ascending; a padded by `mode` (numpy's 'edge' / 'reflect' = reflect-101)."""
    r = (len(taps) - 1) // 2
    pad = [(0, 0)] * a.ndim
    pad[axis] = (r, r)
    ap = np.pad(a, pad, mode=mode)
    n = a.shape[axis]
    acc = np.zeros(a.shape, dtype=np.float32)
    for k in range(len(taps)):
        acc = acc + np.float32(taps[k]) * np.take(ap, np.arange(k, k + n), axis=axis)
    return acc


def corrupt_fp32(x, name, severity, key=0):
    f = np.float32
    p = TABLE[name][severity - 1]
    h, w = x.shape[:2]
    xf = x.astype(np.float32) / f(255)
    if name == "gaussian_noise":
        return _quantise32(xf + f(p) * normals(h, w, key).astype(np.float32))
    if name == "speckle_noise":
        return _quantise32(xf + (xf * f(p)) * normals(h, w, key).astype(np.float32))
    xb = x.astype(np.float32)
    if name == "gaussian_blur":
        t = gaussian_kernel(p).astype(np.float32)
        return _quantise32(_taps_along(_taps_along(xb, t, 1, "edge"), t, 0, "edge") / f(255))
    if name == "defocus_blur":
        s = stencil(*p).astype(np.float32)
        r = (s.shape[0] - 1) // 2
        ap = np.pad(xb, ((r, r), (r, r), (0, 0)), mode="reflect")
        acc = np.zeros(xb.shape, dtype=np.float32)
        for i in range(s.shape[0]):
            for j in range(s.shape[1]):
                acc = acc + s[i, j] * ap[i:i + h, j:j + w]
        return _quantise32(acc / f(255))
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def reference(name, severity, index):
    """The referee's bytes of FRAMES[index] (key: SEED, index), computed once and shared; read-only."""
    out = corrupt(frame(FRAMES[index]), name, severity, key_of(SEED, index))
    out.setflags(write=False)
    return out


def within_cap(pairs):
    """pairs: (got, want) uint8 arrays of one (name, severity) -> (largest byte difference, differing bytes, bytes, allowed differing bytes)."""
    worst = differing = total = 0
    for got, want in pairs:
        d = np.abs(got.astype(np.int16) - want.astype(np.int16))
        worst, differing, total = max(worst, int(d.max())), differing + int((d != 0).sum()), total + d.size
    return worst, differing, total, int(total * CAP_SHARE)
