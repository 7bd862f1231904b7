"""K19's host-side restatement (tests/vis_render_np.py, which the GPU tests hold the kernel to) against the reference itself: the corner
ellipses of ProbabilisticVisualizer.cov_ellipse / draw_ellipse (PV:148-193, PV:322-354), the entropy colours of VP:99-107, the draw
order of PV:64-75 and detectron2's label rules (PV:87-122); the visualize_predictions CLI's plumbing; the ABI mirrors."""
import importlib.util
import math
import os
import subprocess
import sys
import types

import numpy as np
import pytest

from oracle.refimport import REFERENCE_SRC
from pod_compare_amd import hip, visualization
from tests import vis_render_np as vr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_PV = os.path.join(REFERENCE_SRC, "core", "visualization_tools", "probabilistic_visualizer.py")


class _RecordingVisualizer:
    """Stand-in for detectron2's Visualizer under PV: records what PV draws, in order -- boxes (draw_box), ellipse patches (the
    matplotlib Ellipse PV adds to output.ax) and texts (draw_text) -- with detectron2's default font size and colour brightening."""

    def __init__(self, img_rgb, metadata=None, scale=1.0, instance_mode=None):
        h, w = np.asarray(img_rgb).shape[:2]
        self.calls = []
        self.output = types.SimpleNamespace(scale=scale, height=h, width=w, ax=types.SimpleNamespace(add_patch=self._patch))
        self._default_font_size = max(np.sqrt(h * w) // 90, 10 // scale)

    def _patch(self, p):
        self.calls.append(("ellipse", tuple(float(v) for v in p.center), int(np.asarray(p.width).reshape(-1)[0]),
                           int(np.asarray(p.height).reshape(-1)[0]), int(np.asarray(p.angle).reshape(-1)[0])))

    def _convert_boxes(self, boxes):
        return np.asarray(boxes)

    def draw_box(self, box_coord, alpha=0.5, edge_color="g", line_style="-"):
        self.calls.append(("box", tuple(float(v) for v in box_coord), tuple(edge_color)[:3]))

    def draw_text(self, text, position, *, font_size=None, color="g", horizontal_alignment="center", rotation=0):
        self.calls.append(("text", text, tuple(float(v) for v in position), float(font_size)))

    def _change_color_brightness(self, color, brightness_factor):
        import colorsys
        h, l, s = colorsys.rgb_to_hls(*tuple(color)[:3])
        return colorsys.hls_to_rgb(h, min(max(l + brightness_factor * l, 0.0), 1.0), s)


def _reference_visualizer():
    """probabilistic_visualizer.py imported by path, over test-local stand-ins for the two detectron2 modules it imports."""
    if not os.path.exists(REF_PV):
        pytest.skip("reference not available")
    pytest.importorskip("scipy")
    pytest.importorskip("matplotlib")
    import matplotlib.patches  # noqa: F401  (detectron2's visualizer imports matplotlib.figure, which loads it; PV uses mpl.patches)
    saved = {k: sys.modules.get(k) for k in ("detectron2", "detectron2.utils", "detectron2.utils.visualizer", "detectron2.utils.colormap")}
    d2, utils = types.ModuleType("detectron2"), types.ModuleType("detectron2.utils")
    vis, cmap = types.ModuleType("detectron2.utils.visualizer"), types.ModuleType("detectron2.utils.colormap")
    vis.Visualizer, vis.ColorMode, vis._SMALL_OBJECT_AREA_THRESH = _RecordingVisualizer, types.SimpleNamespace(IMAGE=0), 1000
    cmap.random_color = lambda rgb=True, maximum=1: (0.0, 0.0, 0.0)
    d2.utils, utils.visualizer, utils.colormap = utils, vis, cmap
    sys.modules.update({"detectron2": d2, "detectron2.utils": utils, "detectron2.utils.visualizer": vis, "detectron2.utils.colormap": cmap})
    try:
        spec = importlib.util.spec_from_file_location("_ref_probabilistic_visualizer", REF_PV)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
    return mod.ProbabilisticVisualizer


def _covariances(n=2400, seed=19):
    rng = np.random.default_rng(seed)
    var = 10.0 ** rng.uniform(-2, 5, size=(n, 2))
    rho = rng.uniform(-0.999, 0.999, size=n)
    rho[: n // 10] = np.sign(rho[: n // 10]) * 0.999
    out = np.zeros((n, 2, 2))
    out[:, 0, 0], out[:, 1, 1] = var[:, 0], var[:, 1]
    out[:, 0, 1] = out[:, 1, 0] = rho * np.sqrt(var[:, 0] * var[:, 1])
    extra = [np.zeros((2, 2)), np.diag([0.0, 4.0]), np.diag([9.0, 0.0]), np.diag([5.0, 5.0])]
    for k in range(40):                                  # slightly indefinite: |correlation| a little above one
        a, c = 10.0 ** rng.uniform(-1, 4, size=2)
        b = (1.0 + 10.0 ** rng.uniform(-4, -2)) * math.sqrt(a * c) * (1 if k % 2 else -1)
        extra.append(np.array([[a, b], [b, c]]))
    return np.concatenate([out, np.stack(extra)]).astype(np.float32)


def test_corner_ellipses_match_the_reference():
    PV = _reference_visualizer()
    covs = _covariances()
    assert covs.shape[0] >= 2000
    skipped = 0
    for m in covs:
        width, height, rotation = PV.cov_ellipse(m.astype(np.float64))
        width, height = np.array(width), np.array(height)
        width[width < 0] = 0
        height[height < 0] = 0
        ref_skip = bool(np.isnan(width) or np.isnan(height) or np.isnan(rotation))
        ok, w, h, rot, _, _ = vr.cov_ellipse(m[0, 0], m[1, 0], m[1, 1])
        assert (not ok) == ref_skip, (m, width, height, rotation)
        if ref_skip:
            skipped += 1
            continue
        assert (w, h) == (int(width.astype(np.int32)[0]), int(height.astype(np.int32)[0])), (m, w, h, width, height)
        ref_rot = int(np.asarray(rotation).astype(np.int32)) + 180
        diff = (rot - ref_rot) % 180
        assert min(diff, 180 - diff) <= 1, (m, rot, ref_rot)
    assert skipped >= 30                              # the indefinite ones are skipped by both


def test_chi_square_radius():
    scipy_stats = pytest.importorskip("scipy.stats")
    q = 2 * scipy_stats.norm.cdf(2) - 1
    assert vr.R2 == pytest.approx(float(scipy_stats.chi2.ppf(q, 2)), rel=1e-15)
    assert vr.R2 == pytest.approx(-2.0 * math.log(1.0 - q), rel=1e-15)


def test_entropy_colours_match_matplotlib_autumn():
    stats = pytest.importorskip("scipy.stats")
    cm = pytest.importorskip("matplotlib.cm")
    rng = np.random.default_rng(5)
    s = np.concatenate([rng.uniform(0, 1, 4000), [0.0, 1.0, 0.5, 0.25, 0.75, 1e-7, 1 - 1e-7]]).astype(np.float32)
    ref = cm.autumn(stats.entropy(np.stack((s, 1 - s)), base=2))
    for k, v in enumerate(s):
        col, _ = vr.entropy_colour([v])
        assert np.array_equal(np.float32(col), np.float32(ref[k][:3])), (v, col, ref[k])


def test_draw_order_is_area_descending_with_ties_by_index():
    boxes = np.array([[0, 0, 10, 10], [0, 0, 20, 5], [5, 5, 25, 25], [0, 0, 5, 20], [1, 1, 2, 2], [0, 0, 20, 20]], np.float32)
    rec = vr.layout(boxes, frame_hw=(100, 100))
    assert rec.view(np.int32)[:, 0].tolist() == [2, 5, 0, 1, 3, 4]
    areas = np.prod(boxes[:, 2:] - boxes[:, :2], axis=1)
    assert rec[:, 27].tolist() == sorted(areas.tolist(), reverse=True)


def test_label_rules_restated_with_colorsys():
    import colorsys
    rng = np.random.default_rng(7)
    for H, W, scale in ((720, 1280, 1.5), (720, 1280, 1.0), (375, 1242, 1.5), (64, 64, 1.0)):
        dfs = max(np.sqrt(H * W) // 90, 10 // scale)
        assert vr.default_font_size(H, W, scale) == dfs == visualization.default_font_size(H, W, scale)
        x0, y0 = rng.uniform(0, W - 60, 50), rng.uniform(0, H - 60, 50)
        w, h = rng.uniform(1, 200, 50), rng.uniform(1, 200, 50)
        boxes = np.stack([x0, y0, x0 + w, np.minimum(y0 + h, H)], 1).astype(np.float32)
        boxes[0, 3] = H - 2                                   # a small box at the bottom edge: label at (x1, y0)
        boxes[0, 1] = H - 12
        colour = (0.25, 0.5, 0.75)
        rec = vr.layout(boxes, colour=colour, frame_hw=(H, W), scale=scale)
        for r in rec:
            i = int(r[:1].view(np.int32)[0])
            bx0, by0, bx1, by1 = boxes[i]
            pos = (bx0, by0)
            if (by1 - by0) * (bx1 - bx0) < 1000 * scale or by1 - by0 < 40 * scale:
                pos = (bx1, by0) if by1 >= H - 5 else (bx0, by1)
            assert (r[21], r[22]) == (np.float32(pos[0]), np.float32(pos[1]))
            fs = np.clip(((by1 - by0) / np.sqrt(H * W) - 0.02) / 0.08 + 1, 1.2, 2) * 0.5 * dfs
            assert r[23] == np.float32(fs)
            hh, ll, ss = colorsys.rgb_to_hls(*colour)
            lt = list(colorsys.hls_to_rgb(hh, min(max(ll + 0.7 * ll, 0.0), 1.0), ss))
            lt = np.maximum(lt, 0.2)
            lt[np.argmax(lt)] = max(0.8, np.max(lt))
            assert np.array_equal(r[24:27], np.float32(lt))
        first = rec[rec.view(np.int32)[:, 0] == 0][0]
        assert (first[21], first[22]) == (boxes[0, 2], boxes[0, 1])


def test_canvas_and_stroke():
    assert visualization.canvas_size(720, 1280, 1.5) == (1080, 1920)
    assert visualization.canvas_size(720, 1280, 1.0) == (720, 1280)
    assert visualization.stroke_pixels(720, 1280, 1.5) == pytest.approx(max(10 / 4, 1) * 1.5 * 100 / 72, rel=1e-6)


def test_abi_mirrors(tmp_path):
    """ABI 18: the two K19 entry points, and the ctypes mirrors of PodVisList / PodVisFrame against the C header (compiled with gcc)."""
    import ctypes
    import shutil
    assert hip.POD_ABI_VERSION == 18
    assert "pod_vis_layout" in hip.EXPORTS and "pod_vis_render" in hip.EXPORTS
    header = open(os.path.join(ROOT, "include", "pod_mi355x.h")).read()
    assert "#define POD_ABI_VERSION 18" in header
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    src = tmp_path / "vis_layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "pod_mi355x.h"\n'
                   'int main(void){printf("%zu %zu %zu %zu %zu %zu %zu\\n", sizeof(PodVisList), offsetof(PodVisList, colour), offsetof(PodVisList, alpha),'
                   ' sizeof(PodVisFrame), offsetof(PodVisFrame, dst), offsetof(PodVisFrame, inst), offsetof(PodVisFrame, n_labels));'
                   ' printf("%zu %zu\\n", offsetof(PodVisList, colours), offsetof(PodVisList, cov_pairing)); return 0;}\n')
    exe = tmp_path / "vis_layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    want = [ctypes.sizeof(hip.PodVisList), hip.PodVisList.colour.offset, hip.PodVisList.alpha.offset, ctypes.sizeof(hip.PodVisFrame),
            hip.PodVisFrame.dst.offset, hip.PodVisFrame.inst.offset, hip.PodVisFrame.n_labels.offset, hip.PodVisList.colours.offset,
            hip.PodVisList.cov_pairing.offset]
    assert got == want


def test_cli_defaults_and_file_names():
    from pod_compare_amd import visualize_predictions as vp
    a = vp.parse_args(["--results", "r.json", "--gt", "g.json", "--image-root", "imgs", "--output-dir", "out"])
    assert a.min_allowed_score == 0.5 and a.scale == 1.5 and a.max_images == 0
    assert a.train_dataset == "bdd_train" and a.test_dataset == "bdd_val"
    assert vp.output_name("out", "a/b/frame_0001.jpg") == os.path.join("out", "frame_0001.png")


def test_apply_net_flags_default_off_and_eval_only_untouched():
    from pod_compare_amd import apply_net
    src = open(apply_net.__file__).read()
    assert '"--vis-dir", default=""' in src and '"--vis-max-boxes", type=int, default=20' in src
    r = subprocess.run([sys.executable, "-m", "pod_compare_amd.apply_net", "--help"], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "--vis-dir" in r.stdout and "--eval-only" in r.stdout


def _expected_calls(rec, labels):
    """What PV draws, as the restatement's records say: per drawn instance its box, its two ellipses (when drawn), its text."""
    ri = rec.view(np.int32)
    calls = []
    for r, q in zip(rec, ri):
        calls.append(("box", tuple(float(v) for v in r[1:5]), tuple(float(v) for v in r[5:8])))
        for e, (cx, cy) in enumerate(((r[1], r[2]), (r[3], r[4]))):
            if q[9 + 4 * e]:
                calls.append(("ellipse", (float(cx), float(cy)), int(q[10 + 4 * e]), int(q[11 + 4 * e]), int(q[12 + 4 * e])))
        calls.append(("text", labels[int(q[0])], (float(r[21]), float(r[22])), float(r[23])))
    return calls


def _same_calls(got, want):
    assert [c[0] for c in got] == [c[0] for c in want]
    for g, w in zip(got, want):
        if g[0] == "box":
            assert g[1] == w[1] and np.array_equal(np.float32(g[2]), np.float32(w[2])), (g, w)
        elif g[0] == "ellipse":
            assert g[1:4] == w[1:4], (g, w)
            d = (g[4] - w[4]) % 180
            assert min(d, 180 - d) <= 1, (g, w)
        else:
            assert g[1:3] == w[1:3] and np.float32(g[3]) == np.float32(w[3]), (g, w)


def test_overlay_order_and_ellipse_pairing_match_the_reference():
    """PV.overlay_covariance_instances itself, over a recording Visualizer: boxes / colours / labels are drawn in area order and the k-th
    drawn box gets covariance_matrices[k] (PV:70-86 does not reorder the covariances) -- the restatement's "rank" pairing, which the
    layout kernel is held to on the GPU; the "own" pairing (each box its own covariance) is a different picture."""
    PV = _reference_visualizer()
    rng = np.random.default_rng(23)
    H, W = 720, 1280
    for n in (1, 2, 7, 40):
        x0, y0 = rng.uniform(0, W - 300, n), rng.uniform(0, H - 200, n)
        boxes = np.stack([x0, y0, x0 + rng.uniform(5, 300, n), y0 + rng.uniform(5, 200, n)], 1).astype(np.float32)
        a = rng.normal(size=(n, 4, 4)) * 10.0 ** rng.uniform(-1, 1.5, (n, 1, 1))
        cov = (a @ a.transpose(0, 2, 1)).astype(np.float32)
        if n > 2:
            cov[1, 0, 0] = np.nan
        colours = rng.uniform(0, 1, (n, 3)).astype(np.float32)
        labels = ["l%d" % k for k in range(n)]
        for scale in (1.5, 1.0):
            v = PV(np.zeros((H, W, 3), np.uint8), None, scale=scale)
            v.overlay_covariance_instances(boxes=boxes, covariance_matrices=cov, labels=labels,
                                           assigned_colors=[tuple(float(x) for x in c) for c in colours], alpha=1.0)
            rec = vr.layout(boxes, cov, colours=colours, frame_hw=(H, W), scale=scale, pairing="rank")
            _same_calls(v.calls, _expected_calls(rec, labels))
            if n >= 7:
                own = vr.layout(boxes, cov, colours=colours, frame_hw=(H, W), scale=scale, pairing="own")
                assert not np.array_equal(own.view(np.int32)[:, 9:17], rec.view(np.int32)[:, 9:17])


def test_image_writer_is_bounded_and_reports_failures(tmp_path):
    import threading
    import time
    writer = visualization.ImageWriter(workers=2)
    assert writer.depth == 4
    gate, seen = threading.Event(), []
    real = visualization.ImageWriter._write

    def slow(path, image, event):
        gate.wait(5)
        return real(path, image, event)

    writer._write = slow
    img = np.zeros((8, 8, 3), np.uint8)
    for k in range(4):
        writer.submit(str(tmp_path / ("a%d.png" % k)), img)
        seen.append(len(writer.pending))
    t = threading.Thread(target=lambda: writer.submit(str(tmp_path / "a4.png"), img))
    t.start()
    time.sleep(0.2)
    assert t.is_alive()                      # the fifth waits for the oldest
    gate.set()
    t.join(5)
    assert not t.is_alive() and max(seen) <= 4
    writer.close()
    assert sorted(os.listdir(tmp_path)) == ["a%d.png" % k for k in range(5)]
    bad = visualization.ImageWriter(workers=1)
    bad.submit(str(tmp_path / "missing" / "x.png"), img)
    with pytest.raises(OSError):
        bad.close()


def test_cli_pairing_option_and_dataset_pair():
    from pod_compare_amd import visualize_predictions as vp
    a = vp.parse_args(["--results", "r", "--gt", "g", "--image-root", "i", "--output-dir", "o"])
    assert a.ellipse_pairing == "reference"
    a = vp.parse_args(["--results", "r", "--gt", "g", "--image-root", "i", "--output-dir", "o", "--ellipse-pairing", "box"])
    assert a.ellipse_pairing == "box"
    assert visualization.COV_PAIRINGS == {"reference": hip.POD_VIS_COV_BY_RANK, "box": hip.POD_VIS_COV_OWN}
