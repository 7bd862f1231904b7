"""Host side of the COCO bbox evaluation kernels (csrc/k17_coco_eval.hip, C ABI pod_coco_eval_images / pod_coco_accumulate).

Packs `COCO.loadRes`-style annotation dicts into the kernels' arrays -- one row per (image, category) pair with ground truth or
detections, sorted by (category, image position in sorted imgIds), each pair's boxes contiguous in file order -- runs the two
entry points on one stream and returns pycocotools' (precision, recall, scores).  No CPU fallback: a missing library raises.
"""
import ctypes

import numpy as np
import torch

from . import hip


def _params(iou_thrs, rec_thrs, max_dets, area_rngs, n_cat) -> hip.PodCocoParams:
    p = hip.PodCocoParams()
    p.n_iou, p.n_rec, p.n_area, p.n_maxdet, p.n_cat = len(iou_thrs), len(rec_thrs), len(area_rngs), len(max_dets), n_cat
    if (p.n_iou > hip.POD_COCO_MAX_IOU or p.n_rec > hip.POD_COCO_MAX_REC or p.n_area > hip.POD_COCO_MAX_AREA
            or p.n_maxdet > hip.POD_COCO_MAX_MAXDET or p.n_iou * p.n_area > 64 or max(max_dets) > hip.POD_COCO_MAX_KEEP):
        raise hip.PodError("COCO parameters beyond the kernels' limits (include/pod_mi355x.h, POD_COCO_MAX_*)")
    for i, v in enumerate(iou_thrs):
        p.iou_thrs[i] = float(v)
    for i, v in enumerate(rec_thrs):
        p.rec_thrs[i] = float(v)
    for i, (lo, hi) in enumerate(area_rngs):
        p.area_rng[2 * i], p.area_rng[2 * i + 1] = float(lo), float(hi)
    for i, v in enumerate(max_dets):
        p.max_dets[i] = int(v)
    return p


def _group(anns, cat_index, img_pos, n_img):
    """Annotations of the evaluated categories / images, stably ordered by pair key k * n_img + image position."""
    sel = [a for a in anns if a["category_id"] in cat_index and a["image_id"] in img_pos]
    key = np.array([cat_index[a["category_id"]] * n_img + img_pos[a["image_id"]] for a in sel], dtype=np.int64)
    order = np.argsort(key, kind="stable")
    return [sel[i] for i in order], key[order]


def evaluate_accumulate(gts, dts, img_ids, cat_ids, iou_thrs, rec_thrs, max_dets, area_rngs, device="cuda"):
    """COCOeval.evaluate + accumulate on the GPU.  Same signature (plus `device`) as the `impl=` seam of
    compute_average_precision.coco_average_precision.  Returns numpy (precision[T,R,K,A,M], recall[T,K,A,M], scores[T,R,K,A,M])."""
    lib = hip.load()
    K, A, T, R, M = len(cat_ids), len(area_rngs), len(iou_thrs), len(rec_thrs), len(max_dets)
    prm = _params(iou_thrs, rec_thrs, max_dets, area_rngs, K)
    cat_index = {c: k for k, c in enumerate(cat_ids)}
    img_pos = {i: p for p, i in enumerate(img_ids)}
    n_img = max(len(img_ids), 1)
    g, gkey = _group(gts, cat_index, img_pos, n_img)
    d, dkey = _group(dts, cat_index, img_pos, n_img)
    dt_score = np.array([x["score"] for x in d], dtype=np.float64)
    if not np.isfinite(dt_score).all():
        raise ValueError("detection scores must be finite")
    pair_keys = np.union1d(gkey, dkey).astype(np.int64)
    P = pair_keys.size
    gt_off = np.searchsorted(gkey, pair_keys, "left")
    gt_n = np.searchsorted(gkey, pair_keys, "right") - gt_off
    dt_off = np.searchsorted(dkey, pair_keys, "left")
    dt_n = np.searchsorted(dkey, pair_keys, "right") - dt_off
    keep = np.minimum(dt_n, max_dets[-1])
    out_off = np.concatenate([[0], np.cumsum(keep)])[:-1] if P else np.zeros(0, np.int64)
    n_kept = int(keep.sum())
    big = np.nonzero(gt_n > hip.POD_COCO_LDS_GT)[0]
    scratch_n = np.zeros(P, dtype=np.int64)
    for i in big:
        scratch_n[i] = lib.pod_coco_eval_scratch_bytes(int(keep[i]), int(gt_n[i]))
    scratch_off = np.concatenate([[0], np.cumsum(scratch_n)])[:-1] if P else np.zeros(0, np.int64)
    pairs = np.stack([pair_keys // n_img, pair_keys % n_img, gt_off, gt_n, dt_off, dt_n, out_off, scratch_off], 1).astype(np.int64) \
        if P else np.zeros((0, 8), np.int64)
    cat_of_pair = pair_keys // n_img
    cat_off = np.zeros(K + 1, dtype=np.int64)
    np.add.at(cat_off, cat_of_pair + 1, keep)
    cat_off = np.cumsum(cat_off)
    max_seg = int(np.diff(cat_off).max()) if K else 0

    dev = torch.device(device)

    def to_dev(a, dtype):
        return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(dev)

    t_pairs = to_dev(pairs.reshape(-1), torch.int64)
    t_dt_boxes = to_dev(np.array([x["bbox"] for x in d], dtype=np.float64).reshape(-1), torch.float64)
    t_dt_score = to_dev(dt_score, torch.float64)
    t_gt_boxes = to_dev(np.array([x["bbox"] for x in g], dtype=np.float64).reshape(-1), torch.float64)
    t_gt_area = to_dev(np.array([x["area"] for x in g], dtype=np.float64), torch.float64)
    t_gt_crowd = to_dev(np.array([int(x["iscrowd"]) for x in g], dtype=np.int32), torch.int32)
    t_gt_id = to_dev(np.array([int(x["id"]) for x in g], dtype=np.int64), torch.int64)
    t_cat_off = to_dev(cat_off, torch.int64)
    scratch = torch.zeros(max(int(scratch_n.sum()), 1), dtype=torch.uint8, device=dev)
    kept_score = torch.empty(max(n_kept, 1), dtype=torch.float64, device=dev)
    kept_match = torch.empty(max(n_kept, 1), dtype=torch.int64, device=dev)
    kept_ignore = torch.empty(max(n_kept, 1), dtype=torch.int64, device=dev)
    kept_rank = torch.empty(max(n_kept, 1), dtype=torch.int32, device=dev)
    npig = torch.empty(K * A, dtype=torch.int32, device=dev)
    ws = torch.empty(max(int(lib.pod_coco_accumulate_workspace_bytes(n_kept)), 1), dtype=torch.uint8, device=dev)
    precision = torch.empty((T, R, K, A, M), dtype=torch.float64, device=dev)
    recall = torch.empty((T, K, A, M), dtype=torch.float64, device=dev)
    scores = torch.empty((T, R, K, A, M), dtype=torch.float64, device=dev)
    stream = hip.current_stream()
    hip.check(lib.pod_coco_eval_images(ctypes.byref(prm), hip.ptr(t_pairs), P, hip.ptr(t_dt_boxes), hip.ptr(t_dt_score),
                                       hip.ptr(t_gt_boxes), hip.ptr(t_gt_area), hip.ptr(t_gt_crowd), hip.ptr(t_gt_id), hip.ptr(scratch),
                                       hip.ptr(kept_score), hip.ptr(kept_match), hip.ptr(kept_ignore), hip.ptr(kept_rank), hip.ptr(npig),
                                       stream), "pod_coco_eval_images")
    hip.check(lib.pod_coco_accumulate(ctypes.byref(prm), hip.ptr(t_cat_off), max_seg, n_kept, hip.ptr(kept_score), hip.ptr(kept_match),
                                      hip.ptr(kept_ignore), hip.ptr(kept_rank), hip.ptr(npig), hip.ptr(ws), hip.ptr(precision),
                                      hip.ptr(recall), hip.ptr(scores), stream), "pod_coco_accumulate")
    return precision.cpu().numpy(), recall.cpu().numpy(), scores.cpu().numpy()
