"""numpy restatement of K19 (csrc/k19_vis_render.hip) for the tests: the layout (draw order, corner ellipses, colours, label anchors) in
the kernel's fp64 / fp32 steps, and the render (sampling, primitive coverage, compositing) in fp32, primitive by primitive over its
bounding box.  The kernel must equal the layout exactly and the render within one level on a few pixels."""
import math

import numpy as np

INST_WORDS = 32
R2 = 6.180074306244173
LABEL_BOX, LABEL_GLYPH = 3, 4
f32 = np.float32


def pymod1(x):
    return x % 1.0


def text_colour(c):
    import colorsys
    h, l, s = colorsys.rgb_to_hls(*c)
    nl = min(max(l + 0.7 * l, 0.0), 1.0)
    out = list(colorsys.hls_to_rgb(h, nl, s))
    out = [max(v, 0.2) for v in out]
    am = int(np.argmax(out))
    out[am] = max(0.8, out[am])
    return out


def cov_ellipse(a, b, c):
    """(drawn, width, height, rotation + 180, cos, sin) as the kernel computes them (fp64, lower triangle b)."""
    a, b, c = float(a), float(b), float(c)
    half_tr, d = 0.5 * (a + c), 0.5 * (a - c)
    rad = math.sqrt(d * d + b * b) if not (math.isnan(d) or math.isnan(b)) else float("nan")
    lmax = half_tr + rad
    lmin = half_tr - rad
    det = a * c - b * b
    if lmax != 0.0 and abs(lmin) < 0.5 * abs(lmax):
        lmin = det / lmax
    vx, vy = lmin - c, b
    ux, uy = b, lmin - a
    if ux * ux + uy * uy > vx * vx + vy * vy:
        vx, vy = ux, uy
    if vx == 0.0 and vy == 0.0:
        vx, vy = 1.0, 0.0
    with np.errstate(invalid="ignore"):
        width = 2.0 * float(np.sqrt(np.float64(lmin * R2)))
        height = 2.0 * float(np.sqrt(np.float64(lmax * R2)))
    rotation = math.atan2(vy, vx) * (180.0 / math.pi) if not (math.isnan(vx) or math.isnan(vy)) else float("nan")
    if math.isnan(width) or math.isnan(height) or math.isnan(rotation):
        return 0, 0, 0, 0, f32(0), f32(0)
    w = int(width) if width < 2147483647.0 else 2147483647
    h = int(height) if height < 2147483647.0 else 2147483647
    rot = int(rotation) + 180
    t = rot * (math.pi / 180.0)
    return 1, w, h, rot, f32(math.cos(t)), f32(math.sin(t))


def entropy_colour(probs_row):
    s = f32(np.max(np.asarray(probs_row, dtype=f32)))
    t = f32(f32(1.0) - s)
    sm = f32(s + t)
    ps, pt = f32(s / sm), f32(t / sm)
    ent = lambda p: f32(-float(p) * math.log(float(p))) if p > 0 else (f32(0) if p == 0 else f32(-np.inf))
    e = f32(float(f32(ent(ps) + ent(pt))) / math.log(2.0))
    x = f32(e * f32(256.0))
    x = f32(255.0) if x == 256.0 else x
    x = min(max(x, f32(-1.0)), f32(256.0))
    idx = 0 if x < 0 else min(int(x), 255)
    return (1.0, 1.0 if idx == 255 else idx * (1.0 / 255.0), 0.0), idx


def palette_colour(i):
    import colorsys
    hh = pymod1(i * 0.6180339887498949) * 6.0
    sec = int(hh)
    f, v = hh - sec, 1.0
    p, q, t = v * 0.25, v * (1.0 - 0.75 * f), v * (1.0 - 0.75 * (1.0 - f))
    return [(v, t, p), (q, v, p), (p, v, t), (p, q, v), (t, p, v), (v, p, q)][sec % 6]


def default_font_size(H, W, scale):
    return max(np.sqrt(H * W) // 90, 10 // scale)


def layout(boxes, cov=None, probs=None, colour=None, alpha=1.0, frame_hw=(720, 1280), scale=1.0, n=None, colours=None, pairing="rank"):
    """-> (n, 32) float32 records in draw order (int words as int32 bits).  colours: (n, >= 3) per-instance colours (fp32);
    pairing "rank": the box drawn k-th gets covariance k (PV:70-86), "own": its own covariance."""
    boxes = np.asarray(boxes, dtype=f32).reshape(-1, 4)
    n = boxes.shape[0] if n is None else n
    boxes = boxes[:n]
    area = (boxes[:, 2] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 1])
    key = np.where(np.isnan(area), np.inf, -area.astype(np.float64))
    order = sorted(range(n), key=lambda i: (key[i], i))
    H, W = frame_hw
    sq = math.sqrt(H * W)
    dfs = max(sq // 90, 10 // scale)
    out = np.zeros((n, INST_WORDS), dtype=f32)
    oi = out.view(np.int32)
    for rank, i in enumerate(order):
        x0, y0, x1, y1 = boxes[i]
        oi[rank, 0] = i
        out[rank, 1:5] = boxes[i]
        if probs is not None:
            col = entropy_colour(probs[i])[0]
        elif colours is not None:
            col = tuple(float(f32(c)) for c in np.asarray(colours[i])[:3])
        elif colour is not None:
            col = tuple(float(f32(c)) for c in colour[:3])          # PodVisList.colour is fp32
        else:
            col = palette_colour(i)
        out[rank, 5:8] = col
        out[rank, 8] = alpha
        if cov is not None:
            cv = np.asarray(cov[rank if pairing == "rank" else i], dtype=f32).reshape(4, 4)
            for e in range(2):
                r0 = 2 * e
                ok, w, h, rot, cs, sn = cov_ellipse(cv[r0, r0], cv[r0 + 1, r0], cv[r0 + 1, r0 + 1])
                oi[rank, 9 + 4 * e:13 + 4 * e] = (ok, w, h, rot)
                out[rank, 17 + 2 * e] = cs
                out[rank, 18 + 2 * e] = sn
        tx, ty = x0, y0
        ia = f32((y1 - y0) * (x1 - x0))
        if float(ia) < 1000.0 * scale or float(f32(y1 - y0)) < 40.0 * scale:
            if float(y1) >= H - 5.0:
                tx, ty = x1, y0
            else:
                tx, ty = x0, y1
        hr = float(f32(y1 - y0)) / sq
        fs = min(max((hr - 0.02) / 0.08 + 1.0, 1.2), 2.0) * 0.5 * dfs
        out[rank, 21], out[rank, 22], out[rank, 23] = tx, ty, fs
        out[rank, 24:27] = text_colour(col)
        out[rank, 27] = area[i]
    return out


def _prims(records, scale, stroke):
    """The instance primitives of one list in draw order: (kind, params (8,), rgb*255 (3,), alpha, bbox (4,))."""
    s, hw = f32(scale), f32(f32(0.5) * f32(stroke))
    pad = f32(hw + f32(1.0))
    ri = records.view(np.int32)
    out = []
    for r, q in zip(records, ri):
        rgb = (r[5:8] * f32(255.0)).astype(f32)
        X0, Y0, X1, Y1 = (r[1:5] * s).astype(f32)
        out.append((1, (X0, Y0, X1, Y1, hw), rgb, r[8], (min(X0, X1) - pad, min(Y0, Y1) - pad, max(X0, X1) + pad, max(Y0, Y1) + pad)))
        for e in range(2):
            if q[9 + 4 * e] == 0:
                continue
            cx, cy = (f32(r[1] * s), f32(r[2] * s)) if e == 0 else (f32(r[3] * s), f32(r[4] * s))
            a = max(f32(f32(f32(q[10 + 4 * e]) * f32(0.5)) * s), f32(0.5))
            b = max(f32(f32(f32(q[11 + 4 * e]) * f32(0.5)) * s), f32(0.5))
            cs, sn = r[17 + 2 * e], r[18 + 2 * e]
            ex = np.sqrt(f32(f32(a * cs) * f32(a * cs) + f32(b * sn) * f32(b * sn)))
            ey = np.sqrt(f32(f32(a * sn) * f32(a * sn) + f32(b * cs) * f32(b * cs)))
            out.append((2, (cx, cy, a, b, cs, sn, hw), rgb, r[8], (f32(f32(cx - ex) - pad), f32(f32(cy - ey) - pad), f32(f32(cx + ex) + pad), f32(f32(cy + ey) + pad))))
    return out


def _coverage(kind, p, bbox, px, py, cx, cy, atlas):
    inb = (px >= bbox[0]) & (px <= bbox[2]) & (py >= bbox[1]) & (py <= bbox[3])
    if kind == 1:
        X0, Y0, X1, Y1, hw = p
        X0, X1, Y0, Y1 = min(X0, X1), max(X0, X1), min(Y0, Y1), max(Y0, Y1)
        ox = np.maximum(np.maximum(X0 - px, px - X1), f32(0))
        oy = np.maximum(np.maximum(Y0 - py, py - Y1), f32(0))
        outside = (ox > 0) | (oy > 0)
        d = np.where(outside, np.sqrt(ox * ox + oy * oy), np.minimum(np.minimum(px - X0, X1 - px), np.minimum(py - Y0, Y1 - py)))
        c = np.clip(f32(hw + f32(0.5)) - d, f32(0), f32(1))
    elif kind == 2:
        cxe, cye, a, b, cs, sn, hw = p
        dx, dy = px - cxe, py - cye
        u = cs * dx + sn * dy
        v = cs * dy - sn * dx
        ua, vb = u / a, v / b
        g = ua * ua + vb * vb - f32(1.0)
        gu, gv = f32(2.0) * (ua / a), f32(2.0) * (vb / b)
        nrm = np.sqrt(gu * gu + gv * gv)
        with np.errstate(divide="ignore", invalid="ignore"):
            d = np.abs(g) / nrm
            c = np.where(nrm > 0, np.clip(f32(hw + f32(0.5)) - d, f32(0), f32(1)), f32(0))
    elif kind == LABEL_BOX:
        X0, Y0, X1, Y1 = p[1:5]
        d = np.minimum(np.minimum(px - X0, X1 - px), np.minimum(py - Y0, Y1 - py))
        c = np.clip(d + f32(0.5), f32(0), f32(1))
    else:
        X0, Y0, X1, Y1 = (int(v) for v in p[1:5])
        off, gw = int(p[9]), int(p[10])
        gx, gy = cx - X0, cy - Y0
        ok = (gx >= 0) & (gy >= 0) & (gx < X1 - X0) & (gy < Y1 - Y0) & (gx < gw)
        idx = np.where(ok, off + gy * gw + gx, 0)
        c = np.where(ok, atlas[idx].astype(f32) * f32(1.0 / 255.0), f32(0))
    return np.where(inb, c, f32(0)).astype(f32)


def sample(src, frame_hw, scale, out_hw, bgr=False):
    """The canvas before any primitive: nearest sampling of the (frame_h, frame_w) frame, or of src resampled bilinearly to it."""
    src = np.asarray(src)
    if bgr:
        src = src[:, :, ::-1]
    fh, fw = frame_hw
    sh, sw = src.shape[:2]
    oh, ow = out_hw
    px = (np.arange(ow, dtype=f32) + f32(0.5))
    py = (np.arange(oh, dtype=f32) + f32(0.5))
    fx = np.minimum(np.floor(px / f32(scale)).astype(np.int64), fw - 1)
    fy = np.minimum(np.floor(py / f32(scale)).astype(np.int64), fh - 1)
    if (sh, sw) == (fh, fw):
        return src[fy][:, fx].astype(f32)
    rx, ry = f32(f32(sw) / f32(fw)), f32(f32(sh) / f32(fh))
    sx = np.maximum((fx.astype(f32) + f32(0.5)) * rx - f32(0.5), f32(0))
    sy = np.maximum((fy.astype(f32) + f32(0.5)) * ry - f32(0.5), f32(0))
    x0 = np.minimum(sx.astype(np.int64), sw - 1)
    y0 = np.minimum(sy.astype(np.int64), sh - 1)
    x1, y1 = np.minimum(x0 + 1, sw - 1), np.minimum(y0 + 1, sh - 1)
    wx = (sx - x0.astype(f32))[None, :, None]
    wy = (sy - y0.astype(f32))[:, None, None]
    s = src.astype(f32)
    top = s[y0][:, x0] * (f32(1) - wx) + s[y0][:, x1] * wx
    bot = s[y1][:, x0] * (f32(1) - wx) + s[y1][:, x1] * wx
    v = top * (f32(1) - wy) + bot * wy
    return np.clip(np.rint(v), 0, 255).astype(f32)


def render(src, frame_hw, scale, stroke, lists, labels=None, atlas=None, bgr=False):
    """lists: layout() records of up to two lists; labels: (m, 12) host label primitives in the kernel's word order."""
    fh, fw = frame_hw
    oh, ow = int(math.floor(fh * scale + 0.01)), int(math.floor(fw * scale + 0.01))
    dst = sample(src, frame_hw, scale, (oh, ow), bgr)
    prims = [p for rec in lists for p in _prims(rec, scale, stroke)]
    for q in (labels if labels is not None else []):
        q = np.asarray(q, dtype=f32)
        grow = f32(0.5) if int(q[0]) == LABEL_BOX else f32(0)
        prims.append((int(q[0]), q, (q[5:8] * f32(255.0)).astype(f32), q[8],
                      (f32(q[1] - grow), f32(q[2] - grow), f32(q[3] + grow), f32(q[4] + grow))))
    for kind, p, rgb, alpha, bbox in prims:
        x0 = max(int(math.floor(float(bbox[0]) - 0.5)), 0)
        x1 = min(int(math.ceil(float(bbox[2]))) + 1, ow)
        y0 = max(int(math.floor(float(bbox[1]) - 0.5)), 0)
        y1 = min(int(math.ceil(float(bbox[3]))) + 1, oh)
        if x0 >= x1 or y0 >= y1:
            continue
        cx = np.arange(x0, x1)[None, :]
        cy = np.arange(y0, y1)[:, None]
        px, py = cx.astype(f32) + f32(0.5), cy.astype(f32) + f32(0.5)
        cov = _coverage(kind, p, bbox, px, py, cx, cy, atlas)
        w = (f32(alpha) * cov).astype(f32)[:, :, None]
        region = dst[y0:y1, x0:x1]
        upd = region + (rgb[None, None, :] - region) * w
        dst[y0:y1, x0:x1] = np.where(cov[:, :, None] > 0, upd, region)
    return np.clip(np.rint(dst), 0, 255).astype(np.uint8)
