"""Annotated frames on the GPU: the reference's ProbabilisticVisualizer (core/visualization_tools/probabilistic_visualizer.py, PV) over
detectron2's Visualizer, restated on K19 (csrc/k19_vis_render.hip).

`pod_vis_layout` orders each instance list (descending area, ties by index), computes the corner ellipses, colours and label anchors;
`pod_vis_render` draws a batch of frames in one launch.  The host only lays out label strings (glyph quads from a PIL glyph atlas) and
encodes files.  `render_frames` is what visualize_predictions.py and apply_net --vis-dir share; `ProbabilisticVisualizer` keeps the
reference's call shape (overlay_covariance_instances, then get_image).
"""
import math
import os
from collections import deque
from concurrent.futures import ThreadPoolExecutor
from dataclasses import dataclass, field
from functools import lru_cache
from typing import List, Optional, Sequence

import numpy as np
import torch

from . import hip

DPI = 100.0                      # matplotlib's default figure dpi: a point is DPI / 72 pixels
SMALL_OBJECT_AREA_THRESH = 1000  # detectron2.utils.visualizer._SMALL_OBJECT_AREA_THRESH
LABEL_PAD_POINTS = 0.7           # draw_text's bbox pad: points (matplotlib Text.set_bbox without a boxstyle)
LABEL_BOX_ALPHA = 0.8
LIGHTGREEN = (144 / 255.0, 238 / 255.0, 144 / 255.0)   # matplotlib's 'lightgreen' (#90EE90), VP:124-128
COV_PAIRINGS = {"reference": hip.POD_VIS_COV_BY_RANK, "box": hip.POD_VIS_COV_OWN}


def default_font_size(height: int, width: int, scale: float) -> float:
    """detectron2 Visualizer.__init__: max(sqrt(H W) // 90, 10 // scale)."""
    return float(max(np.sqrt(height * width) // 90, 10 // scale))


def stroke_pixels(height: int, width: int, scale: float) -> float:
    """draw_box / draw_ellipse: linewidth max(default_font_size / 4, 1) times the scale, in points at DPI -> canvas pixels."""
    return float(np.float32(max(default_font_size(height, width, scale) / 4, 1) * scale * DPI / 72.0))


def canvas_size(height: int, width: int, scale: float):
    """VisImage: a figure of (W s + 0.01) x (H s + 0.01) pixels, rasterised to its floor."""
    return int(math.floor(height * scale + 0.01)), int(math.floor(width * scale + 0.01))


def font_file() -> Optional[str]:
    """matplotlib's bundled DejaVu Sans (what detectron2's family="sans-serif" resolves to), if matplotlib imports."""
    try:
        import matplotlib
        p = os.path.join(matplotlib.get_data_path(), "fonts", "ttf", "DejaVuSans.ttf")
        return p if os.path.exists(p) else None
    except Exception:
        return None


class GlyphAtlas:
    """ASCII 32..126 of one pixel size: coverage bitmaps (uint8) concatenated, with per-glyph offset, size, bearing and advance."""

    def __init__(self, pixel_size: int):
        from PIL import ImageFont
        path = font_file()
        self.font = ImageFont.truetype(path, pixel_size) if path else ImageFont.load_default(pixel_size)
        ascent, descent = self.font.getmetrics()
        self.ascent, self.height = ascent, ascent + descent
        chunks, self.glyphs, off = [], {}, 0
        for code in range(32, 127):
            ch = chr(code)
            left, top, right, bottom = self.font.getbbox(ch)
            w, h = max(right - left, 0), max(bottom - top, 0)
            bmp = np.zeros((h, w), dtype=np.uint8)
            if w and h:
                mask = self.font.getmask(ch)
                mw, mh = mask.size
                m = np.asarray(mask, dtype=np.uint8).reshape(mh, mw)
                bmp[:min(h, mh), :min(w, mw)] = m[:h, :w]
            self.glyphs[ch] = (off, w, h, left, top, float(self.font.getlength(ch)))
            chunks.append(bmp.reshape(-1))
            off += w * h
        self.data = np.concatenate(chunks) if chunks else np.zeros(0, np.uint8)


@lru_cache(maxsize=None)
def glyph_atlas(pixel_size: int) -> GlyphAtlas:
    return GlyphAtlas(pixel_size)


def label_primitives(text: str, x: float, y: float, font_points: float, scale: float, rgb, atlas_base: int, atlas: GlyphAtlas) -> List[list]:
    """draw_text (va top, ha left) at frame point (x, y): the black background box (alpha 0.8, padded by 0.7 pt), then one quad per glyph."""
    X, Y = float(x) * scale, float(y) * scale
    pen, quads = X, []
    for ch in text:
        g = atlas.glyphs.get(ch, atlas.glyphs["?"])
        off, w, h, left, top, adv = g
        if w and h:
            gx, gy = int(round(pen + left)), int(round(Y + top))
            quads.append([float(hip.POD_VIS_LABEL_GLYPH), gx, gy, gx + w, gy + h, rgb[0], rgb[1], rgb[2], 1.0, float(atlas_base + off), float(w), 0.0])
        pen += adv
    pad = LABEL_PAD_POINTS * DPI / 72.0
    box = [float(hip.POD_VIS_LABEL_BOX), X - pad, Y - pad, pen + pad, Y + atlas.height + pad, 0.0, 0.0, 0.0, LABEL_BOX_ALPHA, 0.0, 0.0, 0.0]
    return [box] + quads


@dataclass
class InstanceList:
    """One overlay_covariance_instances call.  boxes: device (n, 4) XYXY in frame pixels; cov: device
    (n, 4, 4) corner covariances or None; probs: device (n, K) class probabilities -> entropy colours (VP:99-107), else `colour` (one
    colour for all), `colours` (device (n, 3 or 4), one per instance) or, when those are None too, the fixed palette.  count: device int32
    scalar, n = min(count, max_n).  labels: one string per input row (host), or None.  cov_pairing: "reference" = PV:70-86's pairing (the
    box drawn k-th gets covariance k: the reference sorts boxes but not covariance_matrices), "box" = every box its own covariance."""
    boxes: torch.Tensor
    cov: Optional[torch.Tensor] = None
    probs: Optional[torch.Tensor] = None
    colour: Optional[Sequence[float]] = None
    labels: Optional[Sequence[str]] = None
    alpha: float = 1.0
    count: Optional[torch.Tensor] = None
    max_n: Optional[int] = None
    colours: Optional[torch.Tensor] = None
    cov_pairing: str = "reference"


@dataclass
class Frame:
    """A device uint8 frame: `image` (H, W, 3) when layout == "HWC", (3, H, W) for "CHW"; bgr: channel 0 is blue.  out_hw: the
    visualiser's image size when it differs from the frame's (bilinear resampling first, PI:135)."""
    image: torch.Tensor
    layout: str = "HWC"
    bgr: bool = False
    out_hw: Optional[tuple] = None
    lists: List[InstanceList] = field(default_factory=list)

    def hw(self):
        return tuple(self.image.shape[:2]) if self.layout == "HWC" else tuple(self.image.shape[1:])


def _colour_array(colours: torch.Tensor, n: int) -> torch.Tensor:
    c = colours.to(torch.float32)
    if c.dim() != 2 or c.shape[0] < n or c.shape[1] < 3:
        raise hip.PodError("colours: (n, 3 or 4) per instance, got {}".format(tuple(c.shape)))
    return c.contiguous()


class Layouts:
    """pod_vis_layout's outputs of a batch: every list's records and count word are views of ONE device buffer, so that one copy reads
    them all back.  views[frame][list] = (records (rows, POD_VIS_INST_WORDS) fp32, count (1,) int32)."""

    def __init__(self, frames: Sequence[Frame], dev):
        rows = [[max(_list_length(L), 1) for L in f.lists] for f in frames]
        total = sum(sum(r) for r in rows) * hip.POD_VIS_INST_WORDS
        n_lists = sum(len(r) for r in rows)
        self.buf = torch.zeros(total + n_lists, dtype=torch.float32, device=dev)
        counts = self.buf[total:].view(torch.int32)
        self.views, off, k = [], 0, 0
        for r in rows:
            row = []
            for m in r:
                row.append((self.buf[off:off + m * hip.POD_VIS_INST_WORDS].view(m, hip.POD_VIS_INST_WORDS), counts[k:k + 1]))
                off += m * hip.POD_VIS_INST_WORDS
                k += 1
            self.views.append(row)

    def host(self):
        """[frame][list] -> (records, count) on the host, from one device->host copy."""
        h = self.buf.cpu().numpy()
        total = h.size - sum(len(r) for r in self.views)
        counts = h[total:].view(np.int32)
        out, off, k = [], 0, 0
        for r in self.views:
            row = []
            for rec, _ in r:
                m = rec.shape[0]
                row.append((h[off:off + m * hip.POD_VIS_INST_WORDS].reshape(m, hip.POD_VIS_INST_WORDS), int(counts[k])))
                off += m * hip.POD_VIS_INST_WORDS
                k += 1
            out.append(row)
        return out


def _list_length(L: InstanceList) -> int:
    return int(L.boxes.shape[0]) if L.max_n is None else min(int(L.max_n), int(L.boxes.shape[0]))


def _layout(frames: Sequence[Frame], scale: float, stream: int):
    """pod_vis_layout of every list of `frames` -> (Layouts, tensors that must outlive the launch)."""
    lib = hip.load()
    lists, keep = [], []
    layouts = Layouts(frames, frames[0].image.device)
    for fi, f in enumerate(frames):
        fh, fw = f.out_hw or f.hw()
        for li, L in enumerate(f.lists):
            n = _list_length(L)
            if n > hip.POD_VIS_MAX_INSTANCES:
                raise hip.PodError("{} instances in one list: K19 draws at most {}".format(n, hip.POD_VIS_MAX_INSTANCES))
            out, n_out = layouts.views[fi][li]
            boxes = L.boxes if L.boxes.is_contiguous() else L.boxes.contiguous()
            cov = None if L.cov is None else L.cov.reshape(L.cov.shape[0], 16).contiguous()
            if cov is not None and cov.shape[0] < n:
                raise hip.PodError("fewer covariances than boxes")
            probs = None if L.probs is None else L.probs.contiguous()
            colours = None if L.colours is None or probs is not None else _colour_array(L.colours, n)
            keep += [boxes, cov, probs, colours]
            s = hip.PodVisList()
            s.boxes, s.cov, s.probs, s.colours = hip.ptr(boxes), hip.ptr(cov), hip.ptr(probs), hip.ptr(colours)
            s.count = hip.ptr(L.count) if L.count is not None else None
            s.out, s.n_out = out.data_ptr(), n_out.data_ptr()
            s.max_n, s.box_stride = n, int(boxes.stride(0)) if boxes.dim() == 2 and boxes.shape[0] > 0 else 4
            s.cov_stride, s.prob_stride = 16, int(probs.shape[1]) if probs is not None else 0
            s.n_probs = s.prob_stride
            s.colour_stride = int(colours.stride(0)) if colours is not None else 0
            if L.cov_pairing not in COV_PAIRINGS:
                raise ValueError("cov_pairing: one of {}".format(sorted(COV_PAIRINGS)))
            s.cov_pairing = COV_PAIRINGS[L.cov_pairing]
            if probs is not None:
                s.colour_mode = hip.POD_VIS_COLOUR_ENTROPY
            elif colours is not None:
                s.colour_mode = hip.POD_VIS_COLOUR_ARRAY
            elif L.colour is not None:
                s.colour_mode = hip.POD_VIS_COLOUR_FIXED
                for k in range(3):
                    s.colour[k] = float(L.colour[k])
                s.colour[3] = 1.0
            else:
                s.colour_mode = hip.POD_VIS_COLOUR_PALETTE
            s.frame_h, s.frame_w, s.scale, s.alpha = int(fh), int(fw), float(scale), float(L.alpha)
            lists.append(s)
    if lists:
        arr = (hip.PodVisList * len(lists))(*lists)
        hip.check(lib.pod_vis_layout(arr, len(lists), stream), "pod_vis_layout")
    return layouts, keep


def _labels(frames: Sequence[Frame], layouts: Layouts, scale: float, dev):
    """Host layout of the label strings over the layout kernel's anchors / font sizes / text colours: one device->host copy of the batch's
    layouts (a synchronisation), only when some list has labels."""
    per_frame = [[] for _ in frames]
    if not any(L.labels is not None for f in frames for L in f.lists):
        return per_frame, None
    host = layouts.host()
    atlases, base, chunks = {}, 0, []
    for fi, f in enumerate(frames):
        for li, L in enumerate(f.lists):
            if L.labels is None:
                continue
            rec, n = host[fi][li]
            for r in rec[:n]:
                idx = int(r[:1].view(np.int32)[0])
                px = max(1, int(round(float(r[23]) * scale * DPI / 72.0)))
                if px not in atlases:
                    atlases[px] = (base, glyph_atlas(px))
                    chunks.append(atlases[px][1].data)
                    base += atlases[px][1].data.size
                b, at = atlases[px]
                per_frame[fi] += label_primitives(str(L.labels[idx]), float(r[21]), float(r[22]), float(r[23]), scale,
                                                  (float(r[24]), float(r[25]), float(r[26])), b, at)
    atlas = torch.from_numpy(np.concatenate(chunks) if chunks else np.zeros(1, np.uint8)).to(dev)
    return per_frame, atlas


def render_frames(frames: Sequence[Frame], scale: float = 1.0) -> List[torch.Tensor]:
    """Annotated canvases (device uint8 (h, w, 3) RGB, h x w = canvas_size of the visualiser's image) of `frames`, each with up to two
    instance lists drawn in order (VP:123-136: ground truth, then predictions), at `scale` -- one layout and one render launch per
    POD_VIS_LAUNCH_FRAMES frames, on the current stream.  A batch with labels costs one device->host copy of its layouts (a synchronisation:
    the strings are laid out on the host); without labels nothing waits."""
    if not frames:
        return []
    if any(len(f.lists) > 2 for f in frames):
        raise hip.PodError("K19 draws at most two instance lists per frame")
    lib = hip.load()
    dev = frames[0].image.device
    layouts, keep = _layout(frames, scale, hip.current_stream())
    labels, atlas = _labels(frames, layouts, scale, dev)
    canvases, descs = [], []
    for fi, f in enumerate(frames):
        sh, sw = f.hw()
        fh, fw = f.out_hw or (sh, sw)
        oh, ow = canvas_size(fh, fw, scale)
        img = f.image
        if img.dtype != torch.uint8:
            raise hip.PodError("frames are uint8")
        canvas = torch.empty((oh, ow, 3), dtype=torch.uint8, device=dev)
        d = hip.PodVisFrame()
        d.src = img.data_ptr()
        if f.layout == "HWC":
            d.sy, d.sx, d.sc = img.stride(0), img.stride(1), img.stride(2)
        else:
            d.sy, d.sx, d.sc = img.stride(1), img.stride(2), img.stride(0)
        d.src_h, d.src_w, d.bgr, d.bilinear = sh, sw, int(f.bgr), int((fh, fw) != (sh, sw))
        d.frame_h, d.frame_w, d.out_h, d.out_w = fh, fw, oh, ow
        d.dst, d.scale, d.stroke = canvas.data_ptr(), float(scale), stroke_pixels(fh, fw, scale)
        for k, (out, n_out) in enumerate(layouts.views[fi]):
            d.inst[k], d.n_inst[k] = out.data_ptr(), n_out.data_ptr()
        if labels[fi]:
            lab = torch.tensor(labels[fi], dtype=torch.float32).to(dev)
            keep.append(lab)
            d.labels, d.atlas, d.n_labels = lab.data_ptr(), atlas.data_ptr(), len(labels[fi])
        descs.append(d)
        canvases.append(canvas)
    arr = (hip.PodVisFrame * len(descs))(*descs)
    hip.check(lib.pod_vis_render(arr, len(descs), hip.current_stream()), "pod_vis_render")
    # (every buffer above was allocated on this stream: the caching allocator hands it out again only behind the launches)
    del keep
    return canvases


def _colours_of(assigned_colors):
    """assigned_colors (matplotlib colour specs or RGB(A) rows, e.g. VP's `cm.autumn(...)`, or one colour string) -> (one colour, or
    None; an (n, 3) array of per-instance colours, or None).  None -> (None, None): the fixed palette."""
    if assigned_colors is None:
        return None, None
    cols = [assigned_colors] if isinstance(assigned_colors, str) else list(assigned_colors)
    if not cols:
        return None, None
    from matplotlib import colors as mplc
    rgb = [tuple(mplc.to_rgb(c)) for c in cols]
    if all(c == rgb[0] for c in rgb):
        return rgb[0], None
    return None, np.asarray(rgb, dtype=np.float32)


class ProbabilisticVisualizer:
    """PV:9-125 over K19: `overlay_covariance_instances(...)` (at most twice per image, as VP:123-136 calls it) then `get_image()`.
    img_rgb: (H, W, 3) uint8 RGB, numpy or a tensor (kept on its device).  assigned_colors: as the reference takes them (one colour per
    instance, e.g. VP's cm.autumn rows); None gives the fixed palette (the reference's random_color); cls_probs= has the kernel compute
    VP:99-107's entropy colours itself.  cov_pairing: see InstanceList (default: the reference's)."""

    def __init__(self, img_rgb, metadata=None, scale: float = 1.0, device="cuda", cov_pairing: str = "reference"):
        img = img_rgb if isinstance(img_rgb, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(img_rgb).clip(0, 255).astype(np.uint8)))
        self.img = img.to(device) if not img.is_cuda else img
        self.metadata, self.scale, self.lists, self.cov_pairing = metadata, float(scale), [], cov_pairing
        self.output = self

    def overlay_covariance_instances(self, *, boxes=None, covariance_matrices=None, labels=None, assigned_colors=None, alpha=0.5,
                                     cls_probs=None):
        if boxes is None:
            return self
        dev = self.img.device
        t = lambda x: None if x is None else torch.as_tensor(np.asarray(x) if not isinstance(x, torch.Tensor) else x, dtype=torch.float32).to(dev)
        b = t(boxes).reshape(-1, 4)
        if labels is not None:
            assert len(labels) == b.shape[0]
            labels = [str(x) for x in labels]
        if b.shape[0] == 0:
            return self
        if len(self.lists) == 2:
            raise ValueError("at most two overlays per image")
        colour, colours = _colours_of(assigned_colors) if cls_probs is None else (None, None)
        self.lists.append(InstanceList(b, t(covariance_matrices), t(cls_probs), colour, labels, float(alpha), colours=t(colours),
                                       cov_pairing=self.cov_pairing))
        return self

    def get_image(self) -> np.ndarray:
        canvas = render_frames([Frame(self.img, lists=self.lists)], self.scale)[0]
        return canvas.cpu().numpy()


class ImageWriter:
    """Encodes canvases to PNG (or JPEG, by extension) with PIL on `workers` host threads -- the pattern of apply_net.Prefetched, with its
    bound: at most `depth` images (default 2 x workers) wait to be encoded; submit() blocks on the oldest one beyond that, so the host memory
    held by pending images does not grow with the data set.  submit() takes a host uint8 array, or a pinned host tensor with the CUDA event
    after which it is valid (the copy's event).  A failed write raises at the submit() or close() that collects it."""

    def __init__(self, workers: int = 4, depth: int = 0):
        workers = max(1, int(workers))
        self.pool = ThreadPoolExecutor(max_workers=workers, thread_name_prefix="pod-vis-writer")
        self.depth = int(depth) if depth > 0 else 2 * workers
        self.pending = deque()

    @staticmethod
    def _write(path, image, event):
        from PIL import Image
        if event is not None:
            event.synchronize()
        arr = image.numpy() if isinstance(image, torch.Tensor) else np.asarray(image)
        Image.fromarray(arr).save(path)
        return path

    def submit(self, path: str, image, event=None):
        while len(self.pending) >= self.depth:
            self.pending.popleft().result()          # in submission order: every future's result is collected exactly once
        self.pending.append(self.pool.submit(self._write, path, image, event))

    def close(self):
        try:
            while self.pending:
                self.pending.popleft().result()
        finally:
            for f in self.pending:
                f.cancel()
            self.pool.shutdown()


def render_inference(image: torch.Tensor, height: int, width: int, boxes: torch.Tensor, cov: Optional[torch.Tensor], count=None,
                     max_boxes: int = 20, bgr: bool = True, cov_pairing: str = "reference") -> torch.Tensor:
    """ProbabilisticPredictor.visualize_inference (PI:113-146) on the device: the first `max_boxes` detections in the results' order (PI:140-141)
    with their ellipses, palette colours and alpha 0.5, over the (3, h, w) uint8 frame resampled to the output (height, width) (PI:135),
    scale 1.  count: the device detection count (no host sync).  The canvas is RGB whatever the frame's channel order."""
    lst = InstanceList(boxes, cov=cov, count=count, max_n=max_boxes, alpha=0.5, cov_pairing=cov_pairing)
    return render_frames([Frame(image, layout="CHW", bgr=bgr, out_hw=(int(height), int(width)), lists=[lst])], 1.0)[0]


class InferenceFrameWriter:
    """apply_net --vis-dir: per image, the render enqueued on the image's stream behind its detections, the canvas copied to pinned memory
    on that stream, and the PNG encoded on host threads once the copy's event has completed.  The GPU loop runs ahead of the encoding by at
    most ImageWriter's depth (2 x workers images); beyond that it waits for the oldest file."""

    def __init__(self, out_dir: str, max_boxes: int = 20, bgr: bool = True, workers: int = 4, cov_pairing: str = "reference"):
        os.makedirs(out_dir, exist_ok=True)
        self.out_dir, self.max_boxes, self.bgr, self.cov_pairing = out_dir, int(max_boxes), bool(bgr), cov_pairing
        self.writer = ImageWriter(workers)
        self.count = 0

    def add(self, name: str, image: torch.Tensor, height: int, width: int, det) -> None:
        canvas = render_inference(image, height, width, det.boxes, det.cov, det.n_det, self.max_boxes, self.bgr, self.cov_pairing)
        host = torch.empty(canvas.shape, dtype=torch.uint8, pin_memory=True)
        host.copy_(canvas, non_blocking=True)
        done = torch.cuda.Event()
        done.record()
        self.writer.submit(os.path.join(self.out_dir, name), host, done)
        self.count += 1

    def close(self) -> None:
        self.writer.close()
