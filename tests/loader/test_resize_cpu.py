"""K20's host side (pod_resize_taps / pod_resize_coeffs, csrc/k20_resize_u8.hip) against Pillow, without a GPU: the tables applied in
numpy -- horizontal pass into a uint8 intermediate, then the vertical pass -- give Image.resize(BILINEAR)'s bytes; argument validation
of the three entries; apply_net.CocoImages(device_resize=True)."""
import ctypes
import json

import numpy as np
import pytest
import torch
from PIL import Image

from pod_compare_amd import apply_net, hip

# (h, w) -> (nh, nw): both axes up / down, reductions of more than two taps, one axis only, tiny
GEOMETRIES = (((72, 128), (75, 120)), ((37, 61), (53, 87)), ((108, 192), (75, 133)), ((64, 97), (19, 29)), ((40, 40), (40, 67)),
              ((33, 50), (71, 50)), ((5, 7), (11, 3)), ((90, 160), (29, 160)))


def frame(rng, h, w):
    """Random bytes; a third of the rows only 0 / 255, where the fixed-point sums reach the saturating ends."""
    f = rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)
    hard = rng.permutation(h)[: (h + 2) // 3]
    f[hard] = rng.integers(0, 2, size=(len(hard), w, 3), dtype=np.uint8) * 255
    return f


def tables(in_size, out_size):
    lib = hip.load()
    k = lib.pod_resize_taps(in_size, out_size)
    assert k >= 3
    bounds = np.full((out_size, 2), -7, dtype=np.int32)
    coeffs = np.full((out_size, k), -7, dtype=np.int32)
    assert lib.pod_resize_coeffs(in_size, out_size, bounds.ctypes.data_as(ctypes.c_void_p), coeffs.ctypes.data_as(ctypes.c_void_p)) == 0
    return bounds, coeffs


def one_pass(src, bounds, coeffs):
    """Axis 0 of src (n, ...) uint8 resampled with the tables: clip8((2^21 + sum pixel * coeff) >> 22) in int32."""
    out = np.empty((len(bounds),) + src.shape[1:], dtype=np.uint8)
    for i, (lo, n) in enumerate(bounds):
        acc = np.full(src.shape[1:], 1 << 21, dtype=np.int32)
        for t in range(n):
            acc = acc + src[lo + t].astype(np.int32) * np.int32(coeffs[i, t])
        out[i] = np.clip(acc >> 22, 0, 255).astype(np.uint8)
    return out


def resize_np(f, nh, nw, always=False):
    h, w = f.shape[:2]
    if nw != w or always:
        f = one_pass(f.transpose(1, 0, 2), *tables(w, nw)).transpose(1, 0, 2)
    if nh != h or always:
        f = one_pass(f, *tables(h, nh))
    return f


@pytest.mark.parametrize("hw,new", GEOMETRIES, ids=["%dx%d-%dx%d" % (a + b) for a, b in GEOMETRIES])
def test_tables_reproduce_pillow(hw, new):
    rng = np.random.default_rng(hw[0] * 1000 + new[1])
    f = frame(rng, *hw)
    want = np.asarray(Image.fromarray(f).resize((new[1], new[0]), Image.BILINEAR))
    assert np.array_equal(resize_np(f, *new), want)


def test_table_layout_and_identity():
    lib = hip.load()
    assert lib.pod_resize_taps(128, 120) == 5 and lib.pod_resize_taps(61, 87) == 3 and lib.pod_resize_taps(50, 50) == 3
    assert lib.pod_resize_taps(97, 29) == 2 * 4 + 1
    for a, b in ((128, 120), (61, 87), (97, 29), (7, 3), (5, 11)):
        bounds, coeffs = tables(a, b)
        lo, n = bounds[:, 0], bounds[:, 1]
        assert lo.min() >= 0 and n.min() >= 1 and (lo + n).max() <= a and n.max() <= coeffs.shape[1]
        assert lo[0] == 0 and (lo + n)[-1] == a                                     # clamped at both edges
        for i in range(b):
            assert not coeffs[i, n[i]:].any()                                       # zero beyond the count
        assert np.abs(coeffs.sum(1) - (1 << 22)).max() <= coeffs.shape[1]           # normalised, up to the rounding of each tap
        assert coeffs.min() >= 0
    # an axis of equal size: the identity, so a table gives the bytes that skipping the pass gives
    bounds, coeffs = tables(50, 50)
    assert np.array_equal(bounds[:, 0], np.arange(50)) and np.array_equal(coeffs[:, 0], np.full(50, 1 << 22)) and not coeffs[:, 1:].any()
    f = frame(np.random.default_rng(4), 33, 50)
    assert np.array_equal(resize_np(f, 33, 50, always=True), f)


def test_bad_arguments_are_rejected_without_a_gpu():
    lib = hip.load()
    big = hip.POD_RESIZE_MAX_SIDE + 1
    for a, b in ((0, 5), (5, 0), (-3, 5), (5, -1), (big, 5), (5, big)):
        assert lib.pod_resize_taps(a, b) == -1
    bounds, coeffs = np.zeros((8, 2), np.int32), np.zeros((8, 3), np.int32)
    pb, pc = bounds.ctypes.data_as(ctypes.c_void_p), coeffs.ctypes.data_as(ctypes.c_void_p)
    assert lib.pod_resize_coeffs(5, 8, None, pc) == -1 and lib.pod_resize_coeffs(5, 8, pb, None) == -1
    assert lib.pod_resize_coeffs(0, 8, pb, pc) == -1 and lib.pod_resize_coeffs(5, 0, pb, pc) == -1
    assert lib.pod_resize_coeffs(5, 8, pb, pc) == 0
    # pod_resize_frame_u8 validates before any launch; the pointers below are never followed
    S, D, T = 0x1000, 0x2000, 0x3000
    ok = dict(src=S, in_h=5, in_w=8, stride=24, xb=T, xc=T, xk=3, yb=T, yc=T, yk=3, dst=D, out_h=7, out_w=9, flip=1)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.pod_resize_frame_u8(a["src"], a["in_h"], a["in_w"], a["stride"], a["xb"], a["xc"], a["xk"], a["yb"], a["yc"], a["yk"],
                                       a["dst"], a["out_h"], a["out_w"], a["flip"], None)

    for bad in (dict(src=None), dict(dst=None), dict(in_h=0), dict(in_w=0), dict(out_h=0), dict(out_w=-2), dict(in_h=big), dict(out_w=big),
                dict(stride=23),                            # rows shorter than their pixels
                dict(xb=None), dict(xc=None), dict(yb=None), dict(yc=None),          # half a table
                dict(xb=None, xc=None, xk=0),               # no table, but the width changes
                dict(yb=None, yc=None, yk=0),
                dict(xb=None, xc=None, xk=3, out_w=8),      # no table, a tap count
                dict(xk=5), dict(yk=2), dict(xk=0)):        # not the geometry's tap count
        assert call(**bad) == -1, bad


def test_coco_images_device_resize_hands_out_the_decoded_frame(tmp_path):
    rng = np.random.default_rng(3)
    rgb = rng.integers(0, 256, size=(72, 128, 3), dtype=np.uint8)
    Image.fromarray(rgb).save(tmp_path / "a.png")
    Image.fromarray(rgb[:40, :50, 0]).save(tmp_path / "grey.png")                    # mode L: convert("RGB") makes it three channels
    spec = {"images": [{"id": 901, "file_name": "a.png", "height": 72, "width": 128}, {"id": 17, "file_name": "grey.png", "height": 40, "width": 50}]}
    (tmp_path / "set.json").write_text(json.dumps(spec))
    ds = apply_net.CocoImages(str(tmp_path / "set.json"), str(tmp_path), min_size=80, max_size=120, device_resize=True)
    host = apply_net.CocoImages(str(tmp_path / "set.json"), str(tmp_path), min_size=80, max_size=120)
    for i, name in enumerate(("a.png", "grey.png")):
        d, e = ds[i], host[i]
        with Image.open(tmp_path / name) as im:
            want = np.asarray(im.convert("RGB"))
        assert "image" not in d and d["frame"].dtype == torch.uint8 and d["frame"].is_contiguous()
        assert np.array_equal(d["frame"].numpy(), want)
        assert "frame" not in e and {k: v for k, v in d.items() if k != "frame"} == {k: v for k, v in e.items() if k != "image"}
    # the default call: what tests/test_host_cpu.py pins
    a = host[0]
    want = np.asarray(Image.fromarray(rgb).resize((120, 68), Image.BILINEAR))[:, :, ::-1].transpose(2, 0, 1)
    assert tuple(a["image"].shape) == (3, 68, 120) and np.array_equal(a["image"].numpy(), want)
    assert (a["height"], a["width"], a["image_id"], a["file_name"]) == (72, 128, 901, "a.png")
    # the prefetching loader passes either entry on (no GPU here: nothing to pin)
    got = list(apply_net.Prefetched(ds, [1, 0], workers=2, pin=False))
    assert [i for i, _ in got] == [1, 0] and torch.equal(got[1][1]["frame"], ds[0]["frame"])


def test_flag_is_off_by_default_and_documented():
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    r = subprocess.run([sys.executable, "-m", "pod_compare_amd.apply_net", "--help"], cwd=root, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0
    text = " ".join(r.stdout.split())
    assert "--resize-on-gpu" in text and "identical to the host path" in text
    assert '"--resize-on-gpu", action="store_true"' in open(apply_net.__file__).read()
