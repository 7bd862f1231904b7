"""Post-hoc recalibration on the GPU (csrc/k36_recalibrate.hip, C ABI pod_recal_*; include/pod_mi355x.h has the definitions).

The calibration pass (K18) measures how badly calibrated a detector is; this fits the two-parameter-family map users apply next, on a
held-out fold of the validation set, and applies it to a result file, so that every evaluator reports the numbers again:

  * one global temperature: every class probability p becomes sigmoid(beta logit p), beta the minimiser of the binary cross-entropy of
    exactly what the marginal calibration error is measured on (CE:117-131: the flattened probability rows of true positives and
    duplicates against the one-hot converted ground-truth class, the false positives' rows against zeros) -- Newton's method on the
    host, the three sums of every step on the device;
  * per-coordinate standard-deviation scales s of the xyxy box covariance, Sigma -> D Sigma D with D = diag(s), global or per class, fitted on
    the standardised residuals z of the matched detections: `moment` is the maximum-likelihood scale sqrt(mean z^2); `ece` minimises the
    reference's own regression calibration objective (CE:206-261) over a grid of 1025 scales 2^((j - 512) / 128).

No CPU fallback: a missing library raises.  The fp64 host restatement the kernels are tested against lives with the tests
(tests/recalibration/recal_ref.py).
"""
import json
import math
import statistics
from dataclasses import asdict, dataclass, field
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import hip
from .inference_utils import RECORD_HEAD, record_width

FORMAT = 1
GRID_POINTS, GRID_ONE, GRID_PER_OCTAVE = 1025, 512, 128
N_QUANTILES = 14
NEWTON_MAX_ITER = 50
NEWTON_TOL = 2.0 ** -40


def grid_scales() -> List[float]:
    """The 1025 scales 2^((j - 512) / 128): 1/16 .. 16, j = 512 exactly 1."""
    return [2.0 ** ((j - GRID_ONE) / GRID_PER_OCTAVE) for j in range(GRID_POINTS)]


def quantiles() -> List[float]:
    """Phi^-1(i / 15), i = 1 .. 14: the 14 cumulative bin edges of CE:253-256 as standard-normal quantiles."""
    nd = statistics.NormalDist()
    return [nd.inv_cdf(i / (N_QUANTILES + 1.0)) for i in range(1, N_QUANTILES + 1)]


@dataclass
class Recalibration:
    """A fitted map: settings only.  scales: [1][4] (global) or [classes][4] (per class), xyxy standard-deviation factors."""
    beta: float = 1.0
    scales: List[List[float]] = field(default_factory=lambda: [[1.0, 1.0, 1.0, 1.0]])
    per_class: bool = False
    cls_method: str = "none"
    reg_method: str = "none"
    n_scores: int = 0
    n_matched: int = 0
    invalid: List[int] = field(default_factory=lambda: [0, 0, 0, 0])
    cls_objective_before: Optional[float] = None          # L / n_scores at beta = 1 and at the fitted beta
    cls_objective_after: Optional[float] = None
    reg_objective_before: Optional[List[float]] = None    # the ECE objective per segment (reg_method "ece")
    reg_objective_after: Optional[List[float]] = None
    newton_iterations: int = 0
    fold: Optional[List[int]] = None                      # [k, n]: fitted on the images of rank = k (mod n)
    min_allowed_score: Optional[float] = None

    def save(self, path: str) -> None:
        with open(path, "w") as f:
            json.dump(dict({"format": FORMAT}, **asdict(self)), f, indent=2)

    @staticmethod
    def load(path: str) -> "Recalibration":
        with open(path, "r") as f:
            d = json.load(f)
        if d.get("format") != FORMAT:
            raise ValueError("{}: unknown recalibration format {!r} (this version reads format {})".format(path, d.get("format"), FORMAT))
        d.pop("format")
        return Recalibration(**d)

    def is_identity(self) -> bool:
        return self.beta == 1.0 and all(s == 1.0 for row in self.scales for s in row)


def parse_fold(text: str):
    """"k/n" -> (k, n), 0 <= k < n."""
    try:
        k, n = (int(v) for v in text.split("/"))
    except ValueError:
        raise ValueError("--fold takes k/n, got {!r}".format(text))
    if n < 1 or not 0 <= k < n:
        raise ValueError("--fold k/n needs 0 <= k < n, got {!r}".format(text))
    return k, n


def fold_image_ids(image_ids: Sequence, k: int, n: int, complement: bool = False) -> set:
    """The images whose rank among the sorted distinct ids is = k (mod n); complement: the others."""
    ranked = sorted(set(image_ids))
    return {i for r, i in enumerate(ranked) if (r % n == k) != complement}


def _dev(device):
    dev = torch.device(device)
    return torch.device("cuda", torch.cuda.current_device()) if dev.type == "cuda" and dev.index is None else dev


def _workspace(lib, n: int, n_seg: int, dev) -> torch.Tensor:
    return torch.empty(max(int(lib.pod_recal_workspace_bytes(int(n), int(n_seg))), 8), dtype=torch.uint8, device=dev)


class ClsSums:
    """pod_recal_cls_sums on fixed scores and labels: the logits are computed by the first call and reused by the later ones."""

    def __init__(self, scores: torch.Tensor, labels: torch.Tensor):
        self.lib = hip.load()
        self.p = scores.reshape(-1).to(torch.float32).contiguous()
        self.y = labels.reshape(-1).to(self.p.device, torch.uint8).contiguous()
        self.n = int(self.p.numel())
        if self.y.numel() != self.n:
            raise ValueError("scores and labels: equally many")
        dev = self.p.device
        self.x = torch.empty(max(self.n, 1), dtype=torch.float64, device=dev)
        self.ws = _workspace(self.lib, self.n, 0, dev)
        self.out = torch.empty(3, dtype=torch.float64, device=dev)
        self.ready = False

    def __call__(self, beta: float):
        """-> (L, g, h) at beta, Python floats."""
        P = hip.ptr
        with torch.cuda.device(self.p.device):
            hip.check(self.lib.pod_recal_cls_sums(P(self.p), P(self.y), self.n, float(beta), P(self.x), int(self.ready), P(self.ws), P(self.out),
                                                  hip.current_stream()), "pod_recal_cls_sums")
        self.ready = True
        return tuple(self.out.cpu().tolist())


def fit_temperature(scores: torch.Tensor, labels: torch.Tensor):
    """Newton from beta = 1 on the convex L(beta): beta -= g / h until |step| <= 2^-40 |beta|, at most 50 iterations.
    -> (beta, iterations, L at 1, L at beta).  h == 0 or a value that is not finite raises."""
    sums = ClsSums(scores, labels)
    if sums.n == 0:
        return 1.0, 0, 0.0, 0.0
    beta, first = 1.0, None
    for it in range(1, NEWTON_MAX_ITER + 1):
        L, g, h = sums(beta)
        first = L if first is None else first
        if not (math.isfinite(L) and math.isfinite(g) and math.isfinite(h)) or h == 0.0:
            raise ValueError("temperature fit: L, g, h = {}, {}, {} at beta = {} (scores outside [0, 1], or every logit zero)".format(L, g, h, beta))
        step = g / h
        beta -= step
        if not math.isfinite(beta):
            raise ValueError("temperature fit: beta is not finite after {} iterations".format(it))
        if abs(step) <= NEWTON_TOL * abs(beta):
            return beta, it, first, sums(beta)[0]
    raise ValueError("temperature fit: no convergence in {} iterations (beta = {})".format(NEWTON_MAX_ITER, beta))


def reg_z(means: torch.Tensor, covs: torch.Tensor, gt: torch.Tensor, det_class: Optional[torch.Tensor] = None, n_class: int = 0):
    """pod_recal_reg_z: -> (z (n, 4) fp64, seg (n, 4) int32, invalid (4,) int64), device tensors.  n_class = 0: global segments."""
    lib = hip.load()
    dev = means.device
    f = lambda t, *s: t.to(dev, torch.float32).reshape(*s).contiguous()
    means, covs, gt = f(means, -1, 4), f(covs, -1, 4, 4), f(gt, -1, 4)
    n = int(means.shape[0])
    if covs.shape[0] != n or gt.shape[0] != n:
        raise ValueError("means, covariances and ground truths: equally many rows")
    cls = det_class.to(dev, torch.int32).reshape(-1).contiguous() if n_class else None
    if cls is not None and cls.numel() != n:
        raise ValueError("one class per row")
    z = torch.zeros((n, 4), dtype=torch.float64, device=dev)
    seg = torch.full((n, 4), -1, dtype=torch.int32, device=dev)
    invalid = torch.zeros(4, dtype=torch.int64, device=dev)
    ws = _workspace(lib, 4 * n, 0, dev)
    P = hip.ptr
    with torch.cuda.device(dev):
        hip.check(lib.pod_recal_reg_z(P(means), P(covs), P(gt), P(cls), n, int(n_class), P(ws), P(z), P(seg), P(invalid), hip.current_stream()),
                  "pod_recal_reg_z")
    return z, seg, invalid


def moment(z: torch.Tensor, seg: torch.Tensor, n_seg: int):
    """pod_recal_moment: -> (zg (n,) fp64 grouped, seg_off (n_seg + 1,) int64, count (n_seg,) int64, sum (n_seg,) fp64), device tensors."""
    lib = hip.load()
    dev = z.device
    z, seg = z.reshape(-1).to(torch.float64).contiguous(), seg.reshape(-1).to(dev, torch.int32).contiguous()
    n = int(z.numel())
    zg = torch.zeros(max(n, 1), dtype=torch.float64, device=dev)
    seg_off = torch.zeros(n_seg + 1, dtype=torch.int64, device=dev)
    count = torch.zeros(n_seg, dtype=torch.int64, device=dev)
    total = torch.zeros(n_seg, dtype=torch.float64, device=dev)
    ws = _workspace(lib, n, n_seg, dev)
    P = hip.ptr
    with torch.cuda.device(dev):
        hip.check(lib.pod_recal_moment(P(z), P(seg), n, int(n_seg), P(ws), P(zg), P(seg_off), P(count), P(total), hip.current_stream()),
                  "pod_recal_moment")
    return zg[:n], seg_off, count, total


def ece_grid(zg: torch.Tensor, seg_off: torch.Tensor, count: torch.Tensor, scales: Optional[Sequence[float]] = None, j_one: int = GRID_ONE,
             q: Optional[Sequence[float]] = None):
    """pod_recal_ece_grid on pod_recal_moment's grouping: -> (obj (n_seg, n_grid) fp64, best_j (n_seg,) int32, best_obj, one_obj (n_seg,) fp64)."""
    lib = hip.load()
    dev = zg.device
    scales = grid_scales() if scales is None else list(scales)
    q = quantiles() if q is None else list(q)
    n, n_seg = int(zg.numel()), int(count.numel())
    max_seg = int(count.max()) if n_seg else 0
    t_scales = torch.tensor(scales, dtype=torch.float64, device=dev)
    t_q = torch.tensor(q, dtype=torch.float64, device=dev)
    obj = torch.zeros((n_seg, len(scales)), dtype=torch.float64, device=dev)
    best_j = torch.zeros(n_seg, dtype=torch.int32, device=dev)
    best_obj = torch.zeros(n_seg, dtype=torch.float64, device=dev)
    one_obj = torch.zeros(n_seg, dtype=torch.float64, device=dev)
    ws = _workspace(lib, n, n_seg, dev)
    zg = zg.contiguous() if n else torch.zeros(1, dtype=torch.float64, device=dev)
    P = hip.ptr
    with torch.cuda.device(dev):
        hip.check(lib.pod_recal_ece_grid(P(zg), P(seg_off.contiguous()), n, n_seg, max_seg, P(t_scales), len(scales), int(j_one), P(t_q), len(q),
                                         P(ws), P(obj), P(best_j), P(best_obj), P(one_obj), hip.current_stream()), "pod_recal_ece_grid")
    return obj, best_j, best_obj, one_obj


def fit_recalibration(matched: dict, cat_mapping_dict: Dict[int, int], cls: str = "temperature", reg: str = "moment", per_class_reg: bool = False,
                      device="cuda", fold=None, min_allowed_score: Optional[float] = None) -> Recalibration:
    """Fits on the dict `match_predictions_to_groundtruth` returns, with calibration_pass's class conversion and POD_MAX_CLASSES check.
    cls: "temperature" | "none"; reg: "moment" | "ece" | "none"; per_class_reg: one row of scales per contiguous class (a class without a
    matched detection keeps 1).  fold / min_allowed_score are recorded, not used."""
    if cls == "per_class":
        raise ValueError("cls=\"per_class\" is not supported: a temperature per class can change a detection's arg-max class, and with it the "
                         "average precision; one global temperature keeps every ranking")
    if cls not in ("temperature", "none") or reg not in ("moment", "ece", "none"):
        raise ValueError("cls: temperature | none, reg: moment | ece | none; got {!r}, {!r}".format(cls, reg))
    dev = _dev(device)
    tp, dup, fp = matched["true_positives"], matched["duplicates"], matched["false_positives"]
    f32 = lambda t, *shape: t.to(dev, torch.float32).reshape(*shape)
    k1 = int(tp["predicted_cls_probs"].shape[1])
    values = [int(c) for c in cat_mapping_dict.values()]
    if any(c < 0 or c >= hip.POD_MAX_CLASSES for c in values) or k1 < 2:
        raise ValueError("contiguous class ids must lie in [0, {}) and the scores need a background column".format(hip.POD_MAX_CLASSES))
    n_tp, n_dup, n_fp = (int(p["predicted_cls_probs"].shape[0]) for p in (tp, dup, fp))
    n_m = n_tp + n_dup
    gt_ids = torch.cat((tp["gt_cat_idxs"].reshape(-1), dup["gt_cat_idxs"].reshape(-1))).to(dev)
    ids = [int(c) for c in torch.unique(gt_ids.long()).tolist()]
    lut = torch.zeros(max(ids + [0]) + 1, dtype=torch.int64, device=dev)
    for c in ids:
        lut[c] = int(cat_mapping_dict[c])                                                            # KeyError as the calibration pass
    conv = lut[gt_ids.long()] if n_m else torch.zeros(0, dtype=torch.int64, device=dev)
    out = Recalibration(per_class=bool(per_class_reg), cls_method=cls, reg_method=reg, n_matched=n_m,
                        fold=list(fold) if fold is not None else None, min_allowed_score=min_allowed_score)
    with torch.cuda.device(dev):
        if cls == "temperature":
            probs = torch.cat([f32(p["predicted_cls_probs"], -1, k1) for p in (tp, dup, fp)]).contiguous()
            onehot = torch.cat((torch.nn.functional.one_hot(conv, k1).reshape(-1), torch.zeros(n_fp * k1, dtype=torch.int64, device=dev)))
            out.n_scores = int(probs.numel())
            beta, its, before, after = fit_temperature(probs.reshape(-1), onehot)
            out.beta, out.newton_iterations = beta, its
            if out.n_scores:
                out.cls_objective_before, out.cls_objective_after = before / out.n_scores, after / out.n_scores
        n_class = max(values) + 1 if values else 1
        rows = n_class if per_class_reg else 1
        out.scales = [[1.0] * 4 for _ in range(rows)]
        if reg != "none" and n_m:
            means = torch.cat([f32(p["predicted_box_means"], -1, 4) for p in (tp, dup)])
            covs = torch.cat([f32(p["predicted_box_covariances"], -1, 4, 4) for p in (tp, dup)])
            gt = torch.cat([f32(p["gt_box_means"], -1, 4) for p in (tp, dup)])
            z, seg, invalid = reg_z(means, covs, gt, conv.to(torch.int32) if per_class_reg else None, n_class if per_class_reg else 0)
            out.invalid = [int(v) for v in invalid.cpu().tolist()]
            zg, seg_off, count, total = moment(z, seg, 4 * rows)
            cnt, tot = count.cpu().tolist(), total.cpu().tolist()
            if reg == "moment":
                flat = [math.sqrt(t / c) if c else 1.0 for c, t in zip(cnt, tot)]
            else:
                grid = grid_scales()
                _, best_j, best_obj, one_obj = ece_grid(zg, seg_off, count, grid)
                flat = [grid[j] if c else 1.0 for c, j in zip(cnt, best_j.cpu().tolist())]
                out.reg_objective_before, out.reg_objective_after = one_obj.cpu().tolist(), best_obj.cpu().tolist()
            if any(not math.isfinite(s) or s <= 0.0 for s in flat):
                raise ValueError("variance-scale fit: a scale is not positive and finite: {}".format(flat))
            out.scales = [flat[4 * r:4 * r + 4] for r in range(rows)]
    return out


def apply_to_records(records: torch.Tensor, counts: torch.Tensor, num_classes: int, recal: Recalibration) -> torch.Tensor:
    """pod_recal_apply on a record table (n_images, max_det, 6 + K + 16) with counts (n_images,): a new table, the input untouched."""
    return apply_table(records, counts, num_classes, float(recal.beta), recal.scales)


def apply_table(records: torch.Tensor, counts: torch.Tensor, num_classes: int, beta: float, scales) -> torch.Tensor:
    lib = hip.load()
    if records.dim() != 3 or records.shape[2] != record_width(num_classes) or counts.numel() != records.shape[0]:
        raise ValueError("records must be (n_images, max_det, {}) with one count per image".format(record_width(num_classes)))
    dev = records.device
    rec = records.to(torch.float32).contiguous()
    cnt = counts.to(dev, torch.int32).reshape(-1).contiguous()
    sc = torch.as_tensor(scales, dtype=torch.float64).reshape(-1, 4).to(dev).contiguous()
    out = torch.empty_like(rec)
    if rec.numel() == 0:
        return out
    P = hip.ptr
    with torch.cuda.device(dev):
        hip.check(lib.pod_recal_apply(P(rec), P(cnt), int(rec.shape[0]), int(rec.shape[1]), int(num_classes), float(beta), P(sc), int(sc.shape[0]),
                                      P(out), hip.current_stream()), "pod_recal_apply")
    return out


def pack_results(predicted: List[dict], class_of_category: Optional[Dict[int, int]] = None):
    """Result dicts (`instances_to_json`) -> (records (n_images, max_det, 6 + K + 16) fp32, counts int32, K, place): K7's layout on the host;
    place[i] = (image row, slot) of predicted[i].  The record's class: class_of_category[category_id] where given, else the arg-max of cls_prob."""
    rows: Dict = {}
    place = []
    for inst in predicted:
        slot = rows.setdefault(inst["image_id"], [])
        place.append((inst["image_id"], len(slot)))
        slot.append(inst)
    images = list(rows)
    index = {image_id: r for r, image_id in enumerate(images)}
    K = len(predicted[0]["cls_prob"]) if predicted else 1
    max_det = max([len(v) for v in rows.values()] + [1])
    rec = np.zeros((len(images), max_det, record_width(K)), dtype=np.float32)
    for image_id, insts in rows.items():
        r = index[image_id]
        for s, inst in enumerate(insts):
            if len(inst["cls_prob"]) != K:
                raise ValueError("every detection needs the same number of class probabilities")
            cls = class_of_category[inst["category_id"]] if class_of_category is not None else int(np.argmax(inst["cls_prob"]))
            rec[r, s, 0:4] = inst["bbox"]
            rec[r, s, 4] = inst["score"]
            rec[r, s, 5] = cls
            rec[r, s, RECORD_HEAD:RECORD_HEAD + K] = inst["cls_prob"]
            rec[r, s, RECORD_HEAD + K:] = np.asarray(inst["bbox_covar"], dtype=np.float64).reshape(16)
    counts = np.array([len(rows[i]) for i in images], dtype=np.int32)
    return torch.from_numpy(rec), torch.from_numpy(counts), K, [(index[i], s) for i, s in place]


def apply_to_results(predicted: List[dict], recal: Recalibration, class_of_category: Optional[Dict[int, int]] = None, device="cuda") -> List[dict]:
    """The result dicts with score, cls_prob and bbox_covar recalibrated on the GPU: packed into a record table, pod_recal_apply, unpacked.
    category_id, image_id, bbox, the order and the keys are untouched."""
    if not predicted:
        return []
    rec, counts, K, place = pack_results(predicted, class_of_category)
    dev = _dev(device)
    out = apply_to_records(rec.to(dev), counts.to(dev), K, recal).cpu()
    res = []
    for inst, (r, s) in zip(predicted, place):
        row = out[r, s].tolist()
        cov = row[RECORD_HEAD + K:]
        new = dict(inst)
        new["score"] = row[4]
        new["cls_prob"] = row[RECORD_HEAD:RECORD_HEAD + K]
        new["bbox_covar"] = [cov[0:4], cov[4:8], cov[8:12], cov[12:16]]
        res.append(new)
    return res


def format_table(recal: Recalibration) -> str:
    lines = ["beta {:.6f} ({}; {} Newton iterations; {} scores)".format(recal.beta, recal.cls_method, recal.newton_iterations, recal.n_scores)]
    if recal.cls_objective_before is not None:
        lines.append("cross-entropy per score: {:.6f} -> {:.6f}".format(recal.cls_objective_before, recal.cls_objective_after))
    lines.append("scales ({}{}; {} matched detections; invalid per coordinate {})".format(recal.reg_method, ", per class" if recal.per_class else "",
                                                                                         recal.n_matched, recal.invalid))
    for r, row in enumerate(recal.scales):
        text = "  " + ("class {:2d}".format(r) if recal.per_class else "all     ") + "  x1 {:.4f}  y1 {:.4f}  x2 {:.4f}  y2 {:.4f}".format(*row)
        if recal.reg_objective_before is not None:
            b, a = recal.reg_objective_before[4 * r:4 * r + 4], recal.reg_objective_after[4 * r:4 * r + 4]
            text += "   ECE objective " + "  ".join("{:.5f}->{:.5f}".format(x, y) for x, y in zip(b, a))
        lines.append(text)
    if recal.fold is not None:
        lines.append("fitted on fold {}/{}".format(*recal.fold))
    return "\n".join(lines)
