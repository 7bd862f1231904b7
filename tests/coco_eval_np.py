"""A numpy restatement of COCO bbox evaluation (pycocotools `COCOeval.evaluate` / `accumulate` / `summarize` with the default
`Params`, iouType 'bbox') and of the reference's optimal-F1 score threshold (compute_average_precision.py:50-59, "AP").

Written from the published algorithm, loop for loop, so that the HIP path (pod_compare_amd/csrc/k17_coco_eval.hip)
can be compared with it bit for bit.  pycocotools itself is not a dependency of this project, so this file is anchored by the
hand-worked cases in tests/test_average_precision_cpu.py, not by a run of pycocotools.

`evaluate_accumulate` has the signature of the `impl=` seam of `pod_compare_amd.compute_average_precision.coco_average_precision`.
"""
import numpy as np


def _iou(dt, gt, crowd):
    """maskUtils.iou for xywh boxes (fp64): rows = detections, columns = ground truth."""
    out = np.zeros((len(dt), len(gt)))
    for g, G in enumerate(gt):
        ga = G[2] * G[3]
        for d, D in enumerate(dt):
            da = D[2] * D[3]
            w = min(D[2] + D[0], G[2] + G[0]) - max(D[0], G[0])
            if w <= 0:
                continue
            h = min(D[3] + D[1], G[3] + G[1]) - max(D[1], G[1])
            if h <= 0:
                continue
            i = w * h
            u = da if crowd[g] else da + ga - i
            out[d, g] = i / u
    return out


def _evaluate_img(gt, dt, a_rng, max_det, iou_thrs):
    if len(gt) == 0 and len(dt) == 0:
        return None
    for g in gt:
        g["_ignore"] = 1 if (g["iscrowd"] or g["area"] < a_rng[0] or g["area"] > a_rng[1]) else 0
    gtind = np.argsort([g["_ignore"] for g in gt], kind="mergesort")
    gt = [gt[i] for i in gtind]
    dtind = np.argsort([-d["score"] for d in dt], kind="mergesort")
    dt = [dt[i] for i in dtind[0:max_det]]
    iscrowd = [int(o["iscrowd"]) for o in gt]
    ious = _iou([d["bbox"] for d in dt], [g["bbox"] for g in gt], iscrowd)
    T, G, D = len(iou_thrs), len(gt), len(dt)
    gtm, dtm = np.zeros((T, G)), np.zeros((T, D))
    gt_ig = np.array([g["_ignore"] for g in gt])
    dt_ig = np.zeros((T, D))
    if G and D:
        for tind, t in enumerate(iou_thrs):
            for dind, d in enumerate(dt):
                iou = min([t, 1 - 1e-10])
                m = -1
                for gind in range(G):
                    if gtm[tind, gind] > 0 and not iscrowd[gind]:
                        continue
                    if m > -1 and gt_ig[m] == 0 and gt_ig[gind] == 1:
                        break
                    if ious[dind, gind] < iou:
                        continue
                    iou = ious[dind, gind]
                    m = gind
                if m == -1:
                    continue
                dt_ig[tind, dind] = gt_ig[m]
                dtm[tind, dind] = gt[m]["id"]
                gtm[tind, m] = d["id"]
    a = np.array([d["area"] < a_rng[0] or d["area"] > a_rng[1] for d in dt]).reshape((1, len(dt)))
    dt_ig = np.logical_or(dt_ig, np.logical_and(dtm == 0, np.repeat(a, T, 0)))
    return {"dtMatches": dtm, "dtScores": [d["score"] for d in dt], "gtIgnore": gt_ig, "dtIgnore": dt_ig}


def evaluate_accumulate(gts, dts, img_ids, cat_ids, iou_thrs, rec_thrs, max_dets, area_rngs):
    """gts / dts: annotation dicts as `COCO.loadRes` leaves them (image_id, category_id, bbox, area, iscrowd, id; dts also score).
    Returns (precision[T,R,K,A,M], recall[T,K,A,M], scores[T,R,K,A,M])."""
    by_pair_gt, by_pair_dt = {}, {}
    for g in gts:
        by_pair_gt.setdefault((g["image_id"], g["category_id"]), []).append(dict(g))
    for d in dts:
        by_pair_dt.setdefault((d["image_id"], d["category_id"]), []).append(dict(d))
    T, R, K, A, M = len(iou_thrs), len(rec_thrs), len(cat_ids), len(area_rngs), len(max_dets)
    eval_imgs = [_evaluate_img(by_pair_gt.get((i, c), []), by_pair_dt.get((i, c), []), a_rng, max_dets[-1], iou_thrs)
                 for c in cat_ids for a_rng in area_rngs for i in img_ids]
    precision, recall, scores = -np.ones((T, R, K, A, M)), -np.ones((T, K, A, M)), -np.ones((T, R, K, A, M))
    I0, A0 = len(img_ids), A
    for k in range(K):
        for a in range(A):
            for m, max_det in enumerate(max_dets):
                E = [eval_imgs[k * A0 * I0 + a * I0 + i] for i in range(I0)]
                E = [e for e in E if e is not None]
                if len(E) == 0:
                    continue
                dt_scores = np.concatenate([np.asarray(e["dtScores"][0:max_det], dtype=np.float64) for e in E])
                inds = np.argsort(-dt_scores, kind="mergesort")
                dt_scores_sorted = dt_scores[inds]
                dtm = np.concatenate([e["dtMatches"][:, 0:max_det] for e in E], axis=1)[:, inds]
                dt_ig = np.concatenate([e["dtIgnore"][:, 0:max_det] for e in E], axis=1)[:, inds]
                gt_ig = np.concatenate([e["gtIgnore"] for e in E])
                npig = np.count_nonzero(gt_ig == 0)
                if npig == 0:
                    continue
                tps = np.logical_and(dtm, np.logical_not(dt_ig))
                fps = np.logical_and(np.logical_not(dtm), np.logical_not(dt_ig))
                tp_sum = np.cumsum(tps, axis=1).astype(dtype=np.float64)
                fp_sum = np.cumsum(fps, axis=1).astype(dtype=np.float64)
                for t, (tp, fp) in enumerate(zip(tp_sum, fp_sum)):
                    tp, fp = np.array(tp), np.array(fp)
                    nd = len(tp)
                    rc = tp / npig
                    pr = tp / (fp + tp + np.spacing(1))
                    q, ss = np.zeros((R,)), np.zeros((R,))
                    recall[t, k, a, m] = rc[-1] if nd else 0
                    pr, q = pr.tolist(), q.tolist()
                    for i in range(nd - 1, 0, -1):
                        if pr[i] > pr[i - 1]:
                            pr[i - 1] = pr[i]
                    inds_r = np.searchsorted(rc, rec_thrs, side="left")
                    try:
                        for ri, pi in enumerate(inds_r):
                            q[ri] = pr[pi]
                            ss[ri] = dt_scores_sorted[pi]
                    except IndexError:
                        pass
                    precision[t, :, k, a, m] = np.array(q)
                    scores[t, :, k, a, m] = np.array(ss)
    return precision, recall, scores


def summarize(precision, recall, iou_thrs, max_dets=(1, 10, 100)):
    """COCOeval.summarize's 12 stats (area labels all / small / medium / large)."""
    def one(ap, iou_thr=None, area=0, max_det=100):
        m = list(max_dets).index(max_det)
        s = precision if ap else recall
        if iou_thr is not None:
            s = s[np.where(iou_thr == np.asarray(iou_thrs))[0]]
        s = s[:, :, :, area, m] if ap else s[:, :, area, m]
        return -1 if len(s[s > -1]) == 0 else np.mean(s[s > -1])
    stats = np.zeros((12,))
    stats[0] = one(1)
    stats[1] = one(1, iou_thr=.5)
    stats[2] = one(1, iou_thr=.75)
    stats[3], stats[4], stats[5] = one(1, area=1), one(1, area=2), one(1, area=3)
    stats[6], stats[7], stats[8] = one(0, max_det=max_dets[0]), one(0, max_det=max_dets[1]), one(0, max_det=max_dets[2])
    stats[9], stats[10], stats[11] = one(0, area=1), one(0, area=2), one(0, area=3)
    return stats


def optimal_score_threshold(precision, scores, rec_thrs):
    """AP:50-59, quirks included (NaN F1 at p = r = 0 wins argmax; -1 precision entries enter the mean over IoU thresholds;
    zero thresholds are dropped before the mean)."""
    with np.errstate(invalid="ignore", divide="ignore"):
        precisions = precision.mean(0)[:, :, 0, 2]
        recalls = np.expand_dims(rec_thrs, 1)
        f1 = 2 * (precisions * recalls) / (precisions + recalls)
        best = f1.argmax(0)
        sc = scores.mean(0)[:, :, 0, 2]
        thr = np.array([sc[b, i] for i, b in enumerate(best)])
        thr = thr[thr != 0]
        return thr.mean()


def synthetic_set(n_images, seed, n_classes=7, big_image=True):
    """Seeded COCO-style ground truth and results.  Non-contiguous image ids in shuffled order; ground-truth ids from 0 (as the BDD
    converter numbers them); `area` fields that differ from the box areas; crowd boxes; scores on a 0.01 grid (ties within and
    across images); every 97th image with 150 detections; with big_image, one image with 80 boxes of one class (its IoU matrix
    takes the global scratch path)."""
    rng = np.random.default_rng(seed)
    img_ids = [int(i) for i in rng.permutation(n_images * 3)[:n_images]]
    anns, dets, next_id = [], [], 0

    def box():
        w, h = np.exp(rng.uniform(np.log(4), np.log(300), 2))
        return [float(rng.uniform(0, 1000)), float(rng.uniform(0, 600)), float(w), float(h)]

    for n, img in enumerate(img_ids):
        many = big_image and n == 0
        n_gt = 80 if many else int(rng.poisson(6))
        for _ in range(n_gt):
            b = box()
            cat = 1 if many else int(rng.integers(1, n_classes + 1))
            anns.append({"id": next_id, "image_id": img, "category_id": cat, "bbox": b, "area": b[2] * b[3] * float(rng.uniform(.8, 1.1)),
                         "iscrowd": int(rng.random() < .03)})
            next_id += 1
            if rng.random() < .8:
                j = [b[0] + rng.normal(0, .08 * b[2]), b[1] + rng.normal(0, .08 * b[3]), b[2] * rng.uniform(.8, 1.25), b[3] * rng.uniform(.8, 1.25)]
                dets.append({"image_id": img, "category_id": cat if rng.random() < .9 else int(rng.integers(1, n_classes + 1)),
                             "bbox": [float(v) for v in j], "score": round(float(rng.random()), 2)})
        n_fp = 150 if n % 97 == 5 else 120 if many else int(rng.poisson(3))
        for _ in range(n_fp):
            dets.append({"image_id": img, "category_id": 1 if many else int(rng.integers(1, n_classes + 1)), "bbox": box(),
                         "score": round(float(rng.random()), 2)})
    order = rng.permutation(len(dets))
    return {"images": [{"id": i} for i in img_ids], "annotations": anns}, [dets[i] for i in order]
