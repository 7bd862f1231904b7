"""K19, the visualisation kernels (csrc/k19_vis_render.hip), on the GPU: the layout against its numpy restatement (tests/vis_render_np.py)
exactly, the render within one level on a few pixels, an independent check of the drawn geometry, the degenerate and batched cases, and
the two front ends -- apply_net --vis-dir (PI:113-146) and python -m pod_compare_amd.visualize_predictions (VP:20-142).

The module shares its name with tests/test_apply_net_gpu.py (the --vis-dir half is an apply_net run) so that the GPU run order in
tests/conftest.py (GPU_ORDER, keyed by module name) gives it a place."""
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

from pod_compare_amd import inference_utils, visualization as vis
from tests import vis_render_np as vr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
DEV = "cuda"


def _instances(rng, n, H, W, edge=True, degenerate=True, bottom=True):
    """n boxes (overlapping, some crossing the frame's edges, some at the bottom edge), corner covariances (some degenerate / NaN /
    indefinite), class probabilities."""
    cx, cy = rng.uniform(-0.05 * W, 1.05 * W, n), rng.uniform(-0.05 * H, 1.05 * H, n)
    w, h = 10.0 ** rng.uniform(0.3, 2.6, n), 10.0 ** rng.uniform(0.3, 2.4, n)
    boxes = np.stack([cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2], 1)
    if not edge:
        boxes = np.clip(boxes, 0, [W, H, W, H])
    if bottom and n > 2:
        boxes[1] = [W * 0.3, H - 20, W * 0.3 + 25, H - 2]      # small, at the bottom edge: label beside it
        boxes[2] = boxes[0]                                    # an exact tie of areas
    cov = np.zeros((n, 4, 4))
    for k in range(n):
        a = rng.normal(size=(4, 4)) * 10.0 ** rng.uniform(-1, 1.5)
        cov[k] = a @ a.T
    if degenerate and n > 6:
        cov[3] = 0.0                                           # zero: both ellipses are points (clamped to 0.5 px)
        cov[4, 0, 0], cov[4, 1, 1], cov[4, 0, 1], cov[4, 1, 0] = 100.0, 1e-6, 0.0, 0.0      # a segment
        cov[5, 2:, 2:] = [[4.0, 5.0], [5.0, 4.0]]              # indefinite: skipped
        cov[6, 0, 0] = np.nan                                  # NaN: skipped
    probs = rng.dirichlet(np.ones(7) * 0.3, n)
    return boxes.astype(np.float32), cov.astype(np.float32), probs.astype(np.float32)


def _frame(rng, H, W):
    return rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8)


def _t(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _lists_for(rng, n, H, W, labels):
    b, c, p = _instances(rng, n, H, W)
    gt = b[: max(n // 3, 1)] + rng.uniform(-3, 3, (max(n // 3, 1), 4)).astype(np.float32)
    lst = []
    if n:
        lst.append(vis.InstanceList(_t(gt), colour=vis.LIGHTGREEN, labels=["car"] * len(gt) if labels else None, alpha=1.0))
        lst.append(vis.InstanceList(_t(b), cov=_t(c), probs=_t(p), labels=[str(np.float32(v)) for v in p.max(1)] if labels else None, alpha=1.0))
    np_lists = [(gt, None, None, vis.LIGHTGREEN, 1.0), (b, c, p, None, 1.0)] if n else []
    return lst, np_lists


def _np_render(frame, scale, np_lists, labels=None, atlas=None, out_hw=None):
    H, W = out_hw or frame.shape[:2]
    recs = [vr.layout(b, c, p, col, a, (H, W), scale) for b, c, p, col, a in np_lists]      # (the default pairing: the reference's)
    return vr.render(frame, (H, W), scale, vis.stroke_pixels(H, W, scale), recs, labels, atlas)


def _close(got, want):
    diff = np.abs(got.astype(np.int32) - want.astype(np.int32))
    assert diff.max() <= 1, (int(diff.max()), np.argwhere(diff > 1)[:5])
    frac = float((diff > 0).any(-1).mean())
    assert frac <= 1e-3, frac


def _layout_of(L, H, W, scale):
    layouts, _ = vis._layout([vis.Frame(torch.zeros((H, W, 3), dtype=torch.uint8, device=DEV), lists=[L])], scale, torch.cuda.current_stream().cuda_stream)
    out, n_out = layouts.views[0][0]
    return out.cpu().numpy(), int(n_out.item())


def test_layout_equals_numpy_restatement():
    rng = np.random.default_rng(190)
    for n, H, W, scale, mode in ((1, 720, 1280, 1.5, "entropy"), (100, 720, 1280, 1.5, "entropy"), (228, 720, 1280, 1.0, "fixed"),
                                 (37, 375, 1242, 1.5, "palette"), (256, 64, 96, 1.0, "entropy"), (60, 720, 1280, 1.5, "array")):
        b, c, p = _instances(rng, n, H, W)
        cols = rng.uniform(0, 1, (n, 4)).astype(np.float32)
        kw = dict(probs=_t(p)) if mode == "entropy" else dict(colour=(0.2, 0.4, 0.6)) if mode == "fixed" else \
            dict(colours=_t(cols)) if mode == "array" else {}
        for pairing, np_pairing in (("reference", "rank"), ("box", "own")):
            got, m = _layout_of(vis.InstanceList(_t(b), cov=_t(c), alpha=0.5, cov_pairing=pairing, **kw), H, W, scale)
            assert m == n
            want = vr.layout(b, c, p if mode == "entropy" else None, (0.2, 0.4, 0.6) if mode == "fixed" else None, 0.5, (H, W), scale,
                             colours=cols if mode == "array" else None, pairing=np_pairing)
            assert np.array_equal(got.view(np.int32), want.view(np.int32)), (mode, pairing, np.argwhere(got.view(np.int32) != want.view(np.int32))[:8])


def test_layout_reads_the_device_count():
    rng = np.random.default_rng(191)
    b, c, p = _instances(rng, 50, 720, 1280)
    for count in (0, 7, 50, 90):
        L = vis.InstanceList(_t(b), cov=_t(c), count=torch.tensor(count, dtype=torch.int32, device=DEV), max_n=20, alpha=0.5)
        got, m = _layout_of(L, 720, 1280, 1.0)
        n = min(count, 20)
        assert m == n
        want = vr.layout(b[:n], c[:n], None, None, 0.5, (720, 1280), 1.0)
        assert np.array_equal(got[:n].view(np.int32), want.view(np.int32))


def test_render_matches_numpy_restatement():
    rng = np.random.default_rng(192)
    cases = [(n, s, lab) for s in (1.5, 1.0) for n in (0, 1, 100, 228) for lab in (False, True)] + [(100, 1.5, True)] * 4
    assert len(cases) >= 20
    for k in range(0, len(cases), 4):
        batch = cases[k:k + 4]
        frames, np_frames = [], []
        for n, s, lab in batch:
            fr = _frame(rng, 720, 1280)
            lst, np_lists = _lists_for(rng, n, 720, 1280, lab)
            frames.append(vis.Frame(_t(fr), lists=lst))
            np_frames.append((fr, np_lists))
        scales = {s for _, s, _ in batch}
        for s in scales:
            sel = [i for i, c in enumerate(batch) if c[1] == s]
            fsel = [frames[i] for i in sel]
            layouts, _ = vis._layout(fsel, s, torch.cuda.current_stream().cuda_stream)
            labels, atlas = vis._labels(fsel, layouts, s, DEV)
            got = [c.cpu().numpy() for c in vis.render_frames(fsel, s)]
            host_atlas = atlas.cpu().numpy() if atlas is not None else None
            for j, i in enumerate(sel):
                fr, np_lists = np_frames[i]
                want = _np_render(fr, s, np_lists, labels[j] or None, host_atlas)
                assert got[j].shape == want.shape == (int(720 * s), int(1280 * s), 3)
                _close(got[j], want)


def test_ellipse_geometry_independent_of_the_restatement():
    """One ellipse of known centre, width, height and rotation, white on black: the lit ring's centroid is the corner, its principal axis
    (the height's direction: width lies along the smaller eigenvalue's eigenvector) the rotation + 90 degrees."""
    H, W, s = 360, 480, 1.0
    phi = np.deg2rad(30.4)
    v0, v1 = np.array([np.cos(phi), np.sin(phi)]), np.array([-np.sin(phi), np.cos(phi)])
    lam0, lam1 = (30.0 / 2) ** 2 / vr.R2, (90.0 / 2) ** 2 / vr.R2             # width ~30 px, height ~90 px
    block = lam0 * np.outer(v0, v0) + lam1 * np.outer(v1, v1)
    cov = np.full((1, 4, 4), np.nan, np.float32)
    cov[0, :2, :2] = block
    corner = (200.0, 170.0)
    boxes = np.array([[corner[0], corner[1], corner[0], corner[1]]], np.float32)   # a point box: an isotropic blob at the corner
    L = vis.InstanceList(_t(boxes), cov=_t(cov), colour=(1.0, 1.0, 1.0), alpha=1.0)
    img = vis.render_frames([vis.Frame(torch.zeros((H, W, 3), dtype=torch.uint8, device=DEV), lists=[L])], s)[0].cpu().numpy()
    m = img[:, :, 0].astype(np.float64)
    ys, xs = np.nonzero(m)
    wts = m[ys, xs]
    cx, cy = (wts * (xs + 0.5)).sum() / wts.sum(), (wts * (ys + 0.5)).sum() / wts.sum()
    assert abs(cx - corner[0] * s) <= 0.5 and abs(cy - corner[1] * s) <= 0.5, (cx, cy)
    dx, dy = xs + 0.5 - cx, ys + 0.5 - cy
    cxx, cyy, cxy = (wts * dx * dx).sum(), (wts * dy * dy).sum(), (wts * dx * dy).sum()
    ang = np.degrees(0.5 * np.arctan2(2 * cxy, cxx - cyy))
    want = 30.0 + 90.0
    d = (ang - want) % 180
    assert min(d, 180 - d) <= 1.0, ang
    # the extent along each axis: the ring's radius ~ the semi-axes (width 30 -> 15, height 90 -> 45)
    u, v = dx * np.cos(phi) + dy * np.sin(phi), -dx * np.sin(phi) + dy * np.cos(phi)
    assert 13 <= np.abs(u).max() <= 19 and 43 <= np.abs(v).max() <= 49, (np.abs(u).max(), np.abs(v).max())


def test_box_geometry_independent_of_the_restatement():
    H, W, s = 300, 400, 1.5
    box = np.array([[50.3, 40.7, 250.2, 180.9]], np.float32)
    L = vis.InstanceList(_t(box), colour=(1.0, 1.0, 1.0), alpha=1.0)
    img = vis.render_frames([vis.Frame(torch.zeros((H, W, 3), dtype=torch.uint8, device=DEV), lists=[L])], s)[0].cpu().numpy()
    ys, xs = np.nonzero(img[:, :, 0])
    assert len(xs) > 0
    px, py = xs + 0.5, ys + 0.5
    X0, Y0, X1, Y1 = box[0] * s
    ox = np.maximum(np.maximum(X0 - px, px - X1), 0)
    oy = np.maximum(np.maximum(Y0 - py, py - Y1), 0)
    d = np.where((ox > 0) | (oy > 0), np.hypot(ox, oy), np.minimum(np.minimum(px - X0, X1 - px), np.minimum(py - Y0, Y1 - py)))
    assert d.max() <= vis.stroke_pixels(H, W, s), d.max()
    # every side is drawn
    for xv, yv in (((X0 + X1) / 2, Y0), ((X0 + X1) / 2, Y1), (X0, (Y0 + Y1) / 2), (X1, (Y0 + Y1) / 2)):
        assert img[int(yv), int(xv), 0] > 128


def test_no_instances_batches_and_repeats():
    rng = np.random.default_rng(193)
    fr = _frame(rng, 720, 1280)
    for s in (1.5, 1.0):
        img = vis.render_frames([vis.Frame(_t(fr))], s)[0].cpu().numpy()
        oh, ow = vis.canvas_size(720, 1280, s)
        fx = np.minimum(np.floor((np.arange(ow, dtype=np.float32) + np.float32(0.5)) / np.float32(s)).astype(int), 1279)
        fy = np.minimum(np.floor((np.arange(oh, dtype=np.float32) + np.float32(0.5)) / np.float32(s)).astype(int), 719)
        assert np.array_equal(img, fr[fy][:, fx])
    frames = []
    for k in range(11):                                    # > POD_VIS_LAUNCH_FRAMES: two launches, sizes differ
        H, W = (720, 1280) if k % 2 else (375, 600)
        f = _frame(rng, H, W)
        lst, _ = _lists_for(rng, 30 * (k % 3), H, W, labels=k % 4 == 0)
        frames.append(vis.Frame(_t(f), lists=lst))
    together = [c.cpu().numpy() for c in vis.render_frames(frames, 1.5)]
    again = [c.cpu().numpy() for c in vis.render_frames(frames, 1.5)]
    alone = [vis.render_frames([f], 1.5)[0].cpu().numpy() for f in frames]
    for a, b, c in zip(together, again, alone):
        assert np.array_equal(a, b) and np.array_equal(a, c)


def test_bgr_chw_frame_resampled_to_the_output_size():
    """visualize_inference's path: a (3, h, w) BGR network-input frame resampled bilinearly to (height, width), RGB out."""
    rng = np.random.default_rng(194)
    src = _frame(rng, 400, 711)
    b, c, _ = _instances(rng, 20, 720, 1280)
    chw_bgr = np.ascontiguousarray(src[:, :, ::-1].transpose(2, 0, 1))
    got = vis.render_inference(_t(chw_bgr), 720, 1280, _t(b), _t(c), None, 20).cpu().numpy()
    rec = vr.layout(b, c, None, None, 0.5, (720, 1280), 1.0)
    want = vr.render(src, (720, 1280), 1.0, vis.stroke_pixels(720, 1280, 1.0), [rec])
    _close(got, want)


def _coco_set(tmp_path, n=4, seed=3):
    from PIL import Image
    rng = np.random.default_rng(seed)
    images, anns = [], []
    for k in range(n):
        h, w = (180, 320) if k % 2 == 0 else (200, 300)
        Image.fromarray(rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)).save(tmp_path / ("f%d.jpg" % k), quality=95)
        images.append({"id": 900 + k, "file_name": "f%d.jpg" % k, "height": h, "width": w})
        for j in range(2):
            x, y = float(rng.uniform(10, w - 70)), float(rng.uniform(h / 2 + 10, h - 55))       # the lower half
            anns.append({"id": len(anns) + 1, "image_id": 900 + k, "category_id": int(rng.choice([1, 4])), "bbox": [x, y, 60.0, 50.0],
                         "area": 3000.0, "iscrowd": 0})
    (tmp_path / "set.json").write_text(json.dumps({"images": images, "annotations": anns}))
    return images, anns


def test_apply_net_vis_dir_changes_no_detection(tmp_path):
    images, _ = _coco_set(tmp_path)
    env = dict(os.environ, PYTHONPATH=ROOT)
    outs = {}
    for name, extra in (("plain", []), ("vis", ["--vis-dir", str(tmp_path / "vis"), "--vis-max-boxes", "20"])):
        out, side = str(tmp_path / (name + ".json")), str(tmp_path / (name + ".podr"))
        cmd = [sys.executable, "-m", "pod_compare_amd.apply_net", "--coco-json", str(tmp_path / "set.json"), "--image-root", str(tmp_path),
               "--random-init", "--output", out, "--binary-output", side] + extra
        r = subprocess.run(cmd, cwd=ROOT, env=env, timeout=900, capture_output=True, text=True)
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
        outs[name] = (open(out, "rb").read(), open(side, "rb").read(), side)
    assert outs["plain"][0] == outs["vis"][0] and outs["plain"][1] == outs["vis"][1]
    _, counts, _, _ = inference_utils.read_binary_results(outs["vis"][2])
    assert int(counts.sum()) > 0, "no detections: the frames would not show anything was drawn"
    from PIL import Image
    from pod_compare_amd.apply_net import CocoImages
    ids, counts, rec, k = inference_utils.read_binary_results(outs["vis"][2])
    frames = CocoImages(str(tmp_path / "set.json"), str(tmp_path))
    checked = 0
    for j, im in enumerate(images):
        p = tmp_path / "vis" / (os.path.splitext(im["file_name"])[0] + ".png")
        with Image.open(p) as f:
            assert f.size == (im["width"], im["height"]) and f.mode == "RGB"
            png = np.asarray(f).astype(np.int32)
        # the bare frame: the network input resampled to the output size, nothing drawn
        image = frames[j]["image"].to(DEV)
        none = torch.zeros((), dtype=torch.int32, device=DEV)
        bare = vis.render_inference(image, im["height"], im["width"], torch.zeros((1, 4), device=DEV), None, none, 20).cpu().numpy().astype(np.int32)
        n = min(int(counts[j]), 20)
        if n == 0:
            assert np.array_equal(png, bare)
            continue
        # every recorded box (output pixels) shows on its edges: the drawn pixels differ from the bare frame there
        hit = tot = 0
        for x, y, w, h in rec[j, :n, :4].tolist():
            xs = np.clip(np.linspace(x, x + w, 9), 0, im["width"] - 1).astype(int)
            ys = np.clip(np.linspace(y, y + h, 9), 0, im["height"] - 1).astype(int)
            for px, py in [(v, ys[0]) for v in xs] + [(v, ys[-1]) for v in xs] + [(xs[0], v) for v in ys] + [(xs[-1], v) for v in ys]:
                tot += 1
                hit += int(np.abs(png[py, px] - bare[py, px]).max() > 0)
        assert hit >= 0.9 * tot, (im["file_name"], hit, tot)
        checked += 1
    assert checked > 0


def test_visualize_predictions_end_to_end(tmp_path):
    from PIL import Image
    from pod_compare_amd import visualize_predictions as vp
    images, anns = _coco_set(tmp_path, n=3, seed=4)
    results = []
    for im in images:
        for j in range(3):                                     # side by side in the upper half, apart from the ground truth
            p = [0.05] * 7
            p[j] = 0.9 - 0.15 * j
            cov = np.diag([4.0, 9.0, 16.0, 25.0]) + 1.0
            results.append({"image_id": im["id"], "category_id": j + 1, "bbox": [20.0 + 90.0 * j, 20.0, 70.0, 55.0], "score": p[j],
                            "cls_prob": p, "bbox_covar": cov.tolist()})
    (tmp_path / "res.json").write_text(json.dumps(results))
    out_dir = tmp_path / "out"
    written = vp.main(["--results", str(tmp_path / "res.json"), "--gt", str(tmp_path / "set.json"), "--image-root", str(tmp_path),
                       "--output-dir", str(out_dir)])
    assert sorted(os.path.basename(w) for w in written) == ["f0.png", "f1.png", "f2.png"]
    green = np.array([144, 238, 144])
    for im in images:
        arr = np.asarray(Image.open(out_dir / (os.path.splitext(im["file_name"])[0] + ".png")).convert("RGB")).astype(int)
        assert arr.shape == (int(im["height"] * 1.5), int(im["width"] * 1.5), 3)
        # a ground-truth box's left edge (not crossed by a label or a prediction there): light green
        g = next(a for a in anns if a["image_id"] == im["id"])
        x, y, w, h = g["bbox"]
        hits = sum(int(np.abs(arr[int((y + h * f) * 1.5), int(x * 1.5)] - green).max() <= 2) for f in (0.5, 0.6, 0.7, 0.8))
        assert hits >= 2, arr[int((y + h * 0.6) * 1.5), int(x * 1.5) - 2:int(x * 1.5) + 3]
        # a prediction's ellipse at its top-left corner carries the entropy colour: cm.autumn of entropy(s, 1 - s) (VP:99-107)
        ok, wd, ht, rot, _, _ = vr.cov_ellipse(5.0, 1.0, 10.0)        # the xyxy block [[5, 1], [1, 10]] of every prediction
        assert ok
        t = np.deg2rad(rot)
        a, b = wd / 2 * 1.5, ht / 2 * 1.5
        for r in (r for r in results if r["image_id"] == im["id"]):
            want = np.round(np.float32(vr.entropy_colour([np.float32(max(r["cls_prob"]))])[0]) * 255).astype(int)
            x0, y0 = r["bbox"][0] * 1.5, r["bbox"][1] * 1.5
            hits = 0
            for u in np.deg2rad(np.arange(0, 360, 45)):
                px = x0 + np.cos(t) * a * np.cos(u) - np.sin(t) * b * np.sin(u)
                py = y0 + np.sin(t) * a * np.cos(u) + np.cos(t) * b * np.sin(u)
                hits += int(np.abs(arr[int(py), int(px)] - want).max() <= 2)
            assert hits >= 3, (r["cls_prob"], want, hits)


def test_probabilistic_visualizer_call_shape():
    """PV's own call shape (VP:123-136): ground truth with 'lightgreen' and class names, predictions with their covariances, per-instance
    cm.autumn colours and score labels -- equals the CLI's form of the same frame, where the kernel computes the entropy colours; and
    without labels it equals the numpy restatement."""
    cm = pytest.importorskip("matplotlib.cm")
    stats = pytest.importorskip("scipy.stats")
    rng = np.random.default_rng(195)
    H, W = 360, 640
    fr = _frame(rng, H, W)
    b, c, p = _instances(rng, 30, H, W)
    gt = b[:8] + 2.0
    s = p.max(1)
    colours = cm.autumn(stats.entropy(np.stack((s, 1 - s)), base=2))
    v = vis.ProbabilisticVisualizer(fr, None, scale=1.5)
    v.overlay_covariance_instances(boxes=gt, assigned_colors=["lightgreen" for _ in gt], labels=["car"] * len(gt), alpha=1.0)
    v.overlay_covariance_instances(boxes=b, covariance_matrices=c, assigned_colors=colours, alpha=1.0, labels=s)
    got = v.get_image()
    cli = vis.render_frames([vis.Frame(_t(fr), lists=[
        vis.InstanceList(_t(gt), colour=vis.LIGHTGREEN, labels=["car"] * len(gt), alpha=1.0),
        vis.InstanceList(_t(b), cov=_t(c), probs=_t(p), labels=[str(np.float32(x)) for x in s], alpha=1.0)])], 1.5)[0].cpu().numpy()
    _close(got, cli)
    v = vis.ProbabilisticVisualizer(fr, None, scale=1.0)
    cols = rng.uniform(0, 1, (30, 3))
    v.overlay_covariance_instances(boxes=b, covariance_matrices=c, assigned_colors=[tuple(x) for x in cols])
    rec = vr.layout(b, c, colours=cols.astype(np.float32), alpha=0.5, frame_hw=(H, W), scale=1.0)
    _close(v.get_image(), vr.render(fr, (H, W), 1.0, vis.stroke_pixels(H, W, 1.0), [rec]))


def test_predictor_visualize_inference():
    """predictor.visualize_inference (PI:113-146): the first 20 results over the BGR network-input frame resized to the output size."""
    from pod_compare_amd.config import setup_config
    from pod_compare_amd.probabilistic_inference import RetinaNetProbabilisticPredictor, model_test_attributes
    cfgs = os.path.join(ROOT, "pod_compare_amd", "configs")
    cfg = setup_config(os.path.join(cfgs, "BDD-Detection/retinanet/retinanet_R_50_FPN_1x_reg_cls_var.yaml"), os.path.join(cfgs, "Inference/bayes_od.yaml"))
    pred = RetinaNetProbabilisticPredictor(cfg, model=model_test_attributes(cfg))
    rng = np.random.default_rng(196)
    src = _frame(rng, 450, 800)
    b, c, _ = _instances(rng, 35, 720, 1280)
    results = types.SimpleNamespace(pred_boxes=types.SimpleNamespace(tensor=_t(b)), pred_boxes_covariance=_t(c))
    inputs = [{"image": torch.from_numpy(np.ascontiguousarray(src[:, :, ::-1].transpose(2, 0, 1))), "height": 720, "width": 1280}]
    got = pred.visualize_inference(inputs, results)
    assert got.shape == (720, 1280, 3) and got.dtype == np.uint8
    rec = vr.layout(b[:20], c[:20], None, None, 0.5, (720, 1280), 1.0)
    _close(got, vr.render(src, (720, 1280), 1.0, vis.stroke_pixels(720, 1280, 1.0), [rec]))
