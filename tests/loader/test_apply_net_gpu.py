"""K20 (csrc/k20_resize_u8.hip) on the GPU: the loader's resize -- PIL's uint8 bilinear filter, RGB -> BGR, HWC -> CHW -- against Pillow
itself, to the byte; resize.resize_frame_u8 against apply_net.CocoImages; the same detections through either route; apply_net
--resize-on-gpu against the host path.

The module shares its name with tests/test_apply_net_gpu.py (its last test is two apply_net runs) so that the GPU run order in
tests/conftest.py (GPU_ORDER, keyed by module name) gives it a place."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from PIL import Image

from pod_compare_amd import apply_net, hip, inference_utils, resize
from tests.loader.test_resize_cpu import GEOMETRIES, frame, tables

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
DEV = "cuda"

# + both passes skipped (flip and transpose only), + one BDD frame at the test transform's size
KERNEL_GEOMETRIES = GEOMETRIES + (((50, 64), (50, 64)), ((720, 1280), (750, 1333)))


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _launch(src, new, flip, with_identity_tables=False):
    """pod_resize_frame_u8 on src (h, w, 3) uint8 device tensor whose rows may be padded."""
    h, w = src.shape[:2]
    nh, nw = new
    tabs = []
    for a, b in ((w, nw), (h, nh)):
        if a == b and not with_identity_tables:
            tabs.append((None, None, 0))
        else:
            bounds, coeffs = tables(a, b)
            tabs.append((_dev(bounds), _dev(coeffs), coeffs.shape[1]))
    (xb, xc, xk), (yb, yc, yk) = tabs
    buf = torch.full((3 * nh * nw + 256,), 77, dtype=torch.uint8, device=DEV)             # 128 guard bytes on either side of the output
    out = buf[128:128 + 3 * nh * nw].view(3, nh, nw)
    p = lambda t: None if t is None else t.data_ptr()
    assert src.stride(2) == 1 and src.stride(1) == 3
    rc = hip.load().pod_resize_frame_u8(src.data_ptr(), h, w, src.stride(0), p(xb), p(xc), xk, p(yb), p(yc), yk, out.data_ptr(), nh, nw,
                                        int(flip), hip.current_stream())
    assert rc == 0
    torch.cuda.synchronize()
    assert bool((buf[:128] == 77).all()) and bool((buf[-128:] == 77).all())
    return out


def _pillow(f, new, flip):
    h, w = f.shape[:2]
    im = Image.fromarray(f)
    if new != (h, w):
        im = im.resize((new[1], new[0]), Image.BILINEAR)
    a = np.asarray(im)
    if flip:
        a = a[:, :, ::-1]
    return torch.from_numpy(np.ascontiguousarray(a.transpose(2, 0, 1)))


@pytest.mark.parametrize("hw,new", KERNEL_GEOMETRIES, ids=["%dx%d-%dx%d" % (a + b) for a, b in KERNEL_GEOMETRIES])
def test_kernel_equals_pillow(hw, new):
    rng = np.random.default_rng(hw[0] * 1000 + new[1] + 1)
    f = frame(rng, *hw)
    h, w = hw
    padded = torch.full((h, 3 * w + 13), 201, dtype=torch.uint8, device=DEV)              # rows 13 bytes apart from one another
    padded[:, :3 * w] = _dev(f).reshape(h, 3 * w)
    strided = padded[:, :3 * w].unflatten(1, (w, 3))
    assert strided.stride() == (3 * w + 13, 3, 1)
    for flip in (True, False):
        want = _pillow(f, new, flip)
        assert torch.equal(_launch(_dev(f), new, flip).cpu(), want), flip
        assert torch.equal(_launch(strided, new, flip).cpu(), want), flip
    if new[0] == h or new[1] == w:                                                        # a table for an axis of equal size: the same bytes
        assert torch.equal(_launch(_dev(f), new, True, with_identity_tables=True).cpu(), _pillow(f, new, True))


def _write_set(tmp_path, sizes, seed=3, ext="jpg"):
    rng = np.random.default_rng(seed)
    images = []
    for k, (h, w) in enumerate(sizes):
        name = "f%d.%s" % (k, ext)
        Image.fromarray(rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)).save(tmp_path / name, quality=95)
        images.append({"id": 900 + k, "file_name": name, "height": h, "width": w})
    (tmp_path / "set.json").write_text(json.dumps({"images": images}))
    return images


def test_resize_frame_u8_equals_the_host_loader(tmp_path):
    """Same file, either route: CocoImages' "image" (host) and CocoImages(device_resize=True)'s "frame" through resize_frame_u8."""
    sizes = [(72, 128), (40, 50), (128, 72), (80, 100)]
    _write_set(tmp_path, sizes, ext="png")
    for lo, hi in ((80, 120), (800, 1333)):          # (80, 120): up, capped by the long side, down and -- (80, 100) -- unchanged
        host = apply_net.CocoImages(str(tmp_path / "set.json"), str(tmp_path), lo, hi)
        dev = apply_net.CocoImages(str(tmp_path / "set.json"), str(tmp_path), lo, hi, device_resize=True)
        for i in range(len(sizes)):
            got = resize.resize_frame_u8(dev[i]["frame"].to(DEV), lo, hi)
            assert got.dtype == torch.uint8 and got.is_contiguous() and torch.equal(got.cpu(), host[i]["image"]), (lo, hi, i)
            rgb = resize.resize_frame_u8(dev[i]["frame"].to(DEV), lo, hi, bgr=False)
            assert torch.equal(rgb.cpu(), host[i]["image"].flip(0))
    # on another stream, and with more geometries than the table cache keeps
    s = torch.cuda.Stream()
    f = torch.from_numpy(frame(np.random.default_rng(9), 60, 90))
    with torch.cuda.stream(s):
        for k in range(resize.MAX_TABLES + 3):
            lo = 40 + k
            got = resize.resize_frame_u8(f.to(DEV), lo, 200)
            nh, nw = got.shape[1:]
            assert torch.equal(got.cpu(), torch.from_numpy(np.ascontiguousarray(
                np.asarray(Image.fromarray(f.numpy()).resize((nw, nh), Image.BILINEAR))[:, :, ::-1].transpose(2, 0, 1))))
    assert len(resize._tables) <= resize.MAX_TABLES
    with pytest.raises(ValueError):
        resize.resize_frame_u8(f.to(DEV).permute(2, 0, 1), 40, 200)


def test_same_detections_through_either_route(tmp_path):
    """Three frames through the predictor as apply_net drives it (device records, no host sync): the host-resized "image" and
    "frame" -> resize_frame_u8 give equal records and counts.  The model's class bias is shifted so that detections exist."""
    from pod_compare_amd import config
    from pod_compare_amd.probabilistic_inference import build_predictor
    from tests.test_sparse_tower_gpu import build
    cfgs = os.path.join(ROOT, "pod_compare_amd", "configs")
    cfg = config.setup_config(os.path.join(cfgs, "BDD-Detection", "retinanet", "retinanet_R_50_FPN_1x_reg_cls_var.yaml"),
                              os.path.join(cfgs, "Inference", "bayes_od.yaml"))
    cfg.MODEL.DEVICE = DEV
    m = build()
    with torch.no_grad():
        m.head.cls_score.weight.mul_(40.0)
        m.head.cls_score.bias.fill_(-2.5)
    _write_set(tmp_path, [(180, 320), (200, 300), (180, 320)], seed=5)
    lo, hi = cfg.INPUT.MIN_SIZE_TEST, cfg.INPUT.MAX_SIZE_TEST
    host = apply_net.CocoImages(str(tmp_path / "set.json"), str(tmp_path), lo, hi)
    dev = apply_net.CocoImages(str(tmp_path / "set.json"), str(tmp_path), lo, hi, device_resize=True)
    p = build_predictor(cfg, model=m)
    p.return_device = True
    p.sparse_bbox_tower = True
    counts = []
    with torch.no_grad():
        for i in range(3):
            a, b = host[i], dev[i]
            image = resize.resize_frame_u8(b["frame"].to(DEV), lo, hi)
            assert torch.equal(image.cpu(), a["image"])
            outs = []
            for im in (a["image"].to(DEV), image):
                det = p([{"image": im, "height": a["height"], "width": a["width"], "image_id": i}])
                outs.append((det.records.clone(), det.n_det.clone()))
            (r0, n0), (r1, n1) = outs
            n = int(n0)
            assert torch.equal(n0, n1) and torch.equal(r0[:n], r1[:n]), i      # (rows behind the count are never written: torch.empty)
            counts.append(n)
    assert max(counts) > 0, counts


def test_apply_net_resize_on_gpu_writes_the_same_results(tmp_path):
    images = _write_set(tmp_path, [(180, 320), (200, 300), (180, 320), (200, 300)])
    env = dict(os.environ, PYTHONPATH=ROOT)
    outs = {}
    for name, extra in (("host", []), ("gpu", ["--resize-on-gpu"])):
        out, side = str(tmp_path / (name + ".json")), str(tmp_path / (name + ".podr"))
        cmd = [sys.executable, "-m", "pod_compare_amd.apply_net", "--coco-json", str(tmp_path / "set.json"), "--image-root", str(tmp_path),
               "--random-init", "--output", out, "--binary-output", side] + extra
        r = subprocess.run(cmd, cwd=ROOT, env=env, timeout=900, capture_output=True, text=True)
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
        assert ("resized on the GPU" in r.stdout) == bool(extra)
        outs[name] = (open(out, "rb").read(), open(side, "rb").read(), side)
    assert outs["host"][0] == outs["gpu"][0] and outs["host"][1] == outs["gpu"][1]
    ids, counts, _, _ = inference_utils.read_binary_results(outs["gpu"][2])
    assert [int(v) for v in ids] == [im["id"] for im in images]
