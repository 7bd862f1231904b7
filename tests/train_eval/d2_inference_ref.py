"""The referee of K32: detectron2's `RetinaNet.inference_single_image` + `detector_postprocess` restated in plain torch on the CPU,
from detectron2's documented behaviour (the v0.1 line the reference was written against; detectron2 itself is not a dependency).

Per level: the (A*K, H, W) logits in `permute_to_N_HWA_K(...).flatten()` order -- flat index f = (cell * A + a) * K + k --, ranked by a
STABLE descending sort of the logits (ties: lower f first), the first min(topk, H*W*A*K) kept, then those whose fp32 sigmoid exceeds the
threshold; anchor = f // K, class = f % K; Box2BoxTransform.apply_deltas; over the level concatenation batched_nms and the first
max_detections survivors; then scale to the output size, clip, drop empty boxes.

`literal_level` is the form detectron2 writes (sort on the sigmoid scores themselves); on tie-free inputs the two agree, which is what
tests/train_eval/test_train_eval_cpu.py asserts.  box decoding and NMS are the project's standing restatements (oracle/pod_oracle.py).
"""
from typing import List, Sequence, Tuple

import torch

from oracle.pod_oracle import class_aware_nms, decode_boxes


def flat_logits(cls: torch.Tensor, K: int) -> torch.Tensor:
    """(A*K, H, W) or (1, A*K, H, W) planes -> the (H*W*A*K,) vector of permute_to_N_HWA_K(...).flatten()."""
    cls = cls.reshape(cls.shape[-3:]).float().cpu()
    AK, H, W = cls.shape
    return cls.reshape(AK // K, K, H, W).permute(2, 3, 0, 1).reshape(-1)


def flat_deltas(delta: torch.Tensor) -> torch.Tensor:
    """(A*4, H, W) planes -> (H*W*A, 4)."""
    delta = delta.reshape(delta.shape[-3:]).float().cpu()
    A4, H, W = delta.shape
    return delta.reshape(A4 // 4, 4, H, W).permute(2, 3, 0, 1).reshape(-1, 4)


def rank_level(logits: torch.Tensor, topk: int, score_thresh: float) -> Tuple[torch.Tensor, torch.Tensor]:
    """The selected flat indices of one level in rank order, and their fp32 scores."""
    order = torch.sort(logits, descending=True, stable=True)[1][: min(int(topk), logits.numel())]
    scores = torch.sigmoid(logits)[order]          # over the whole level, as flatten().sigmoid_() evaluates it
    keep = scores > score_thresh
    return order[keep], scores[keep]


def literal_level(logits: torch.Tensor, topk: int, score_thresh: float) -> Tuple[torch.Tensor, torch.Tensor]:
    """detectron2's own lines: flatten().sigmoid_(), sort on the scores, [:num_topk], > threshold."""
    prob = logits.clone().sigmoid_()
    num_topk = min(int(topk), prob.numel())
    predicted_prob, topk_idxs = prob.sort(descending=True)
    predicted_prob, topk_idxs = predicted_prob[:num_topk], topk_idxs[:num_topk]
    keep = predicted_prob > score_thresh
    return topk_idxs[keep], predicted_prob[keep]


class Reference:
    """Everything the tests compare with, computed once per input."""

    def __init__(self, cls: Sequence[torch.Tensor], delta: Sequence[torch.Tensor], anchors: Sequence[torch.Tensor], K: int, topk: int = 1000,
                 score_thresh: float = 0.05, nms_thresh: float = 0.5, max_detections: int = 100, weights=(1.0, 1.0, 1.0, 1.0),
                 image_size=None, out_size=None):
        self.flat: List[torch.Tensor] = []          # per level: selected flat indices in rank order
        boxes, scores, classes = [], [], []
        for c, d, a in zip(cls, delta, anchors):
            f, s = rank_level(flat_logits(c, K), topk, score_thresh)
            self.flat.append(f)
            anchor_idx, cl = f // K, f % K
            boxes.append(decode_boxes(flat_deltas(d)[anchor_idx], a.float().cpu()[anchor_idx], weights))
            scores.append(s)
            classes.append(cl)
        self.boxes, self.scores, self.classes = torch.cat(boxes), torch.cat(scores), torch.cat(classes)      # the level concatenation
        self.keep = class_aware_nms(self.boxes, self.scores, self.classes, nms_thresh)[: int(max_detections)]
        self.det_boxes = self.det_scores = self.det_classes = None
        if image_size is not None:
            self.postprocess(image_size, out_size if out_size is not None else image_size)

    def postprocess(self, image_size, out_size) -> None:
        """detector_postprocess: Boxes.scale by (out_w / w, out_h / h), Boxes.clip to the output size, Boxes.nonempty()."""
        b = self.boxes[self.keep].clone()
        sx, sy = out_size[1] / image_size[1], out_size[0] / image_size[0]
        b[:, 0::2] *= sx
        b[:, 1::2] *= sy
        b[:, 0].clamp_(min=0, max=out_size[1])
        b[:, 2].clamp_(min=0, max=out_size[1])
        b[:, 1].clamp_(min=0, max=out_size[0])
        b[:, 3].clamp_(min=0, max=out_size[0])
        ok = ((b[:, 2] - b[:, 0]) > 0) & ((b[:, 3] - b[:, 1]) > 0)
        self.nonempty = ok
        self.det_boxes, self.det_scores, self.det_classes = b[ok], self.scores[self.keep][ok], self.classes[self.keep][ok]

    @property
    def n(self) -> int:
        return int(self.det_boxes.shape[0])
