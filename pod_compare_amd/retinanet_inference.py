"""Host side of K32 (csrc/k32_retinanet_inference.hip): detectron2's `RetinaNet.inference` + `detector_postprocess` for one image --
what the reference model runs in eval mode (probabilistic_retinanet.py:156-166), the routine `Trainer.test` evaluates.

`RetinaNetInference` is the counterpart of `hotpath.HotPath`: it owns the workspace of one level geometry and enqueues the chain on the
current HIP stream -- one C call (`infer_image`), or stage by stage (`score`, `topk`, `decode`, `nms`, `postprocess`; the tests hold each
on its own).  Nothing here computes on the CPU or synchronises; counts stay in device words, so the one-call form is hipGraph-capturable.
The ordering contract -- descending logit, ties to the lower flat index f = (cell * A + a) * K + k -- is stated in include/pod_mi355x.h
and DESIGN.md.
"""
from dataclasses import dataclass
from typing import List, Sequence, Tuple

import torch

from . import hip


@dataclass
class InferenceParams:
    """MODEL.RETINANET.{NUM_CLASSES, SCORE_THRESH_TEST, TOPK_CANDIDATES_TEST, NMS_THRESH_TEST, BBOX_REG_WEIGHTS} and
    TEST.DETECTIONS_PER_IMAGE, with detectron2's defaults."""
    num_classes: int = 7
    num_anchors: int = 9
    topk_candidates: int = 1000
    score_thresh: float = 0.05
    nms_thresh: float = 0.5
    max_detections: int = 100
    box_weights: Tuple[float, float, float, float] = (1.0, 1.0, 1.0, 1.0)


@dataclass
class ImageDetections:
    """infer_image's result: device tensors.  boxes (max_detections, 4) XYXY in output pixels, scores, classes (int32) and the device
    count n; rows >= n are not written.  `trimmed()` reads n back (the one synchronisation) and returns exact-size tensors."""
    boxes: torch.Tensor
    scores: torch.Tensor
    classes: torch.Tensor
    n: torch.Tensor

    def trimmed(self):
        m = int(self.n.item())
        return self.boxes[:m], self.scores[:m], self.classes[:m].long(), m


class RetinaNetInference:
    """Workspace + launcher for one (level geometry, inference parameters)."""

    def __init__(self, shapes: Sequence[Tuple[int, int]], anchors: Sequence[torch.Tensor], params: InferenceParams, device="cuda"):
        self.lib = hip.load()
        self.p = params
        self.device = torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.shapes = [tuple(int(v) for v in s) for s in shapes]
        self.L = len(self.shapes)
        A, K = params.num_anchors, params.num_classes
        self.level_R = [h * w * A for h, w in self.shapes]
        self.anchor_base = [0]
        for r in self.level_R[:-1]:
            self.anchor_base.append(self.anchor_base[-1] + r)
        self.R = sum(self.level_R)
        self.n_cap = self.L * params.topk_candidates
        self.cfg = self._make_cfg()
        self._levels_t = hip.PodLevel * max(self.L, 1)
        layout = hip.PodRetinaNetLayout()
        total = int(self.lib.pod_retinanet_infer_workspace(self.cfg, self._geometry_levels(), layout)) if 1 <= self.L <= hip.POD_MAX_LEVELS else -1
        if total < 0:
            raise hip.PodError("unsupported geometry for K32: levels={} (max {}), classes={} (max {}), topk={} (max {}, {} over the levels), "
                               "max_detections={} (max {})".format(self.L, hip.POD_MAX_LEVELS, K, hip.POD_MAX_CLASSES - 1, params.topk_candidates,
                                                                   hip.POD_MAX_TOPK, hip.POD_MAX_CANDIDATES, params.max_detections, hip.POD_MAX_DETECTIONS))
        self.anchors = torch.cat([a.to(self.device, torch.float32) for a in anchors]).contiguous()
        assert self.anchors.shape == (self.R, 4), (self.anchors.shape, self.R)
        self.layout = layout
        self.workspace = torch.zeros(total, dtype=torch.uint8, device=self.device)      # zeroed once: counters, tickets, K4's generation word
        n = self.n_cap

        def view(name, dtype, count):
            off = getattr(layout, name)
            return self.workspace[off:off + count * torch.empty((), dtype=dtype).element_size()].view(dtype)

        self.cand_keys = view("cand_keys", torch.int64, self.R * K)
        self.counters = view("cand_count", torch.int32, 2 * hip.POD_MAX_LEVELS)
        self.cand_count = self.counters[: self.L]
        self.sel_keys, self.sel_count = view("sel_keys", torch.int64, n), view("sel_count", torch.int32, self.L)
        self.cat_keys, self.cat_level = view("cat_keys", torch.int64, n), view("cat_level", torch.int32, n)
        self.n_total = view("n_total", torch.int32, 1)
        self.cand_flat, self.cand_level = view("cand_flat", torch.int32, n), view("cand_level", torch.int32, n)
        self.boxes = view("boxes", torch.float32, 4 * n).view(n, 4)
        self.scores, self.classes = view("scores", torch.float32, n), view("classes", torch.int32, n)
        self.keep, self.n_keep = view("keep", torch.int32, hip.POD_MAX_DETECTIONS), view("n_keep", torch.int32, 1)
        self.nms_scratch = self.workspace[layout.nms_scratch:layout.total]
        self._dirty = False

    def _make_cfg(self) -> hip.PodConfig:
        p, c = self.p, hip.PodConfig()
        c.n_levels, c.n_runs, c.num_anchors, c.num_classes = self.L, 1, p.num_anchors, p.num_classes
        c.topk, c.max_detections = p.topk_candidates, p.max_detections
        c.score_thresh, c.nms_thresh = p.score_thresh, p.nms_thresh
        for i in range(4):
            c.box_weights[i] = p.box_weights[i]
        return c

    def _geometry_levels(self):
        lv = self._levels_t()
        for l, (h, w) in enumerate(self.shapes):
            lv[l].H, lv[l].W, lv[l].anchor_base = h, w, self.anchor_base[l]
        return lv

    def set_anchors(self, anchors: Sequence[torch.Tensor]) -> None:
        new = torch.cat([a.to(self.anchors.device, torch.float32) for a in anchors])
        assert new.shape == self.anchors.shape, (new.shape, self.anchors.shape)
        self.anchors.copy_(new)

    def _plane(self, name: str, l: int, t: torch.Tensor, c: int) -> int:
        h, w = self.shapes[l]
        want = (self.p.num_anchors * c, h, w)
        shape = tuple(t.shape[1:]) if t.dim() == 4 and t.shape[0] == 1 else tuple(t.shape)
        if not (t.dtype == torch.float32 and shape == want and t.is_contiguous() and t.device == self.device):
            raise hip.PodError("{}[{}]: expected contiguous fp32 {} (or one run of it) on {}, got {} {} on {}".format(
                name, l, want, self.device, t.dtype, tuple(t.shape), t.device))
        return t.data_ptr()

    def levels(self, cls: Sequence[torch.Tensor], delta: Sequence[torch.Tensor]):
        """The PodLevel array of one image's eval-mode head output: cls[l] (A*K, H, W), delta[l] (A*4, H, W) (a leading run dimension of 1
        is accepted, as the model's forward returns it)."""
        if len(cls) != self.L or len(delta) != self.L:
            raise hip.PodError("{} levels of cls and {} of delta for a workspace of {}".format(len(cls), len(delta), self.L))
        arr = self._geometry_levels()
        for l in range(self.L):
            arr[l].cls = self._plane("cls", l, cls[l], self.p.num_classes)
            arr[l].delta = self._plane("delta", l, delta[l], 4)
        self._keep_inputs = (list(cls), list(delta), arr)
        return arr

    def _clean(self) -> None:
        """The counters are zero between images (the decode kernel consumes them); after an enqueue that raised half way they are reset."""
        if self._dirty:
            hip.check(self.lib.pod_reset_counters(hip.ptr(self.counters), int(self.counters.numel()), hip.current_stream()), "pod_reset_counters")
            self._dirty = False

    # ---- the stages, one entry point each ---------------------------------------------------------------------------------------
    def score(self, lv) -> None:
        self._clean()
        self._dirty = True
        hip.check(self.lib.pod_retinanet_score(self.cfg, lv, hip.ptr(self.cand_keys), hip.ptr(self.cand_count), hip.current_stream()),
                  "pod_retinanet_score")

    def topk(self, lv) -> None:
        P = hip.ptr
        hip.check(self.lib.pod_retinanet_topk(self.cfg, lv, P(self.cand_keys), P(self.cand_count), P(self.sel_keys), P(self.sel_count),
                                              P(self.cat_keys), P(self.cat_level), P(self.n_total), hip.current_stream()), "pod_retinanet_topk")

    def decode(self, lv) -> None:
        P = hip.ptr
        hip.check(self.lib.pod_retinanet_decode(self.cfg, lv, P(self.anchors), P(self.cat_keys), P(self.cat_level), P(self.n_total),
                                                P(self.cand_count), P(self.cand_flat), P(self.cand_level), P(self.boxes), P(self.scores),
                                                P(self.classes), hip.current_stream()), "pod_retinanet_decode")
        self._dirty = False

    def nms(self) -> None:
        P = hip.ptr
        hip.check(self.lib.pod_nms_cluster(self.cfg, P(self.n_total), self.n_cap, P(self.boxes), P(self.scores), P(self.classes),
                                           P(self.keep), P(self.n_keep), P(self.nms_scratch), hip.current_stream()), "pod_nms_cluster")

    def new_detections(self) -> ImageDetections:
        md, dev = self.p.max_detections, self.device
        return ImageDetections(torch.empty((md, 4), dtype=torch.float32, device=dev), torch.empty(md, dtype=torch.float32, device=dev),
                               torch.empty(md, dtype=torch.int32, device=dev), torch.empty(1, dtype=torch.int32, device=dev))

    def postprocess(self, image_size, out_size, out: ImageDetections = None) -> ImageDetections:
        P = hip.ptr
        out = out if out is not None else self.new_detections()
        sx, sy = out_size[1] / image_size[1], out_size[0] / image_size[0]
        hip.check(self.lib.pod_retinanet_postprocess(self.cfg, P(self.keep), P(self.n_keep), P(self.boxes), P(self.scores), P(self.classes),
                                                     sx, sy, float(out_size[0]), float(out_size[1]), P(out.boxes), P(out.scores),
                                                     P(out.classes), P(out.n), hip.current_stream()), "pod_retinanet_postprocess")
        return out

    # ---- one image, one call ----------------------------------------------------------------------------------------------------
    def infer_levels(self, lv, image_size, out_size, out: ImageDetections = None) -> ImageDetections:
        """pod_retinanet_infer_image on a PodLevel array `levels()` made (kept alive by the caller across a graph capture)."""
        P = hip.ptr
        out = out if out is not None else self.new_detections()
        self._clean()
        self._dirty = True
        hip.check(self.lib.pod_retinanet_infer_image(self.cfg, lv, P(self.anchors), P(self.workspace), int(image_size[0]), int(image_size[1]),
                                                     int(out_size[0]), int(out_size[1]), P(out.boxes), P(out.scores), P(out.classes), P(out.n),
                                                     hip.current_stream()), "pod_retinanet_infer_image")
        self._dirty = False
        return out

    def infer_image(self, levels, image_size, out_size) -> ImageDetections:
        """levels: (cls, delta), the per-level lists of the eval-mode head output.  image_size: the network input (h, w) the boxes are
        decoded in; out_size: the frame's original (height, width).  Returns device tensors boxes (n, 4), scores (n), classes (n) and n
        as ImageDetections (fixed capacity; `.trimmed()` for exact sizes)."""
        cls, delta = levels
        return self.infer_levels(self.levels(cls, delta), image_size, out_size)

    def selected(self) -> List[torch.Tensor]:
        """Per level, the selected flat indices in rank order (a read-back: tests and diagnostics)."""
        n = int(self.n_total.item())
        flat, level = self.cand_flat[:n].cpu(), self.cand_level[:n].cpu()
        return [flat[level == l].long() for l in range(self.L)]
