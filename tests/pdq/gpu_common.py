"""What the GPU tests of tests/pdq/ share: the direct calls of pod_pdq_pairs / pod_pdq_assign with sentinels behind every output, and the
referee's numbers of the fixtures, computed once.  Imports without a GPU."""
import functools

import numpy as np
import torch

from tests.pdq import fixtures as fx
from tests.pdq import pdq_ref as pr

DEV = "cuda:0"
SENTINEL = -12345.0
ISENTINEL = -12345


def tables(images):
    """The four host tables of a list of images (CPU tensors) and the totals."""
    cum = lambda xs: torch.tensor([0] + list(xs), dtype=torch.int64).cumsum(0)
    nd, ng = [len(im["means"]) for im in images], [len(im["gt_boxes"]) for im in images]
    frames = torch.tensor([list(im["frame"]) for im in images], dtype=torch.int32).reshape(len(images), 2).contiguous()
    return frames, cum(nd).to(torch.int32).contiguous(), cum(ng).to(torch.int32).contiguous(), cum([d * g for d, g in zip(nd, ng)]).contiguous()


def workspace(lib, n_images):
    return torch.empty(max(int(lib.pod_pdq_workspace_bytes(n_images)), 8), dtype=torch.uint8, device=DEV)


def pairs(images, p_min=pr.P_MIN):
    """pod_pdq_pairs on a list of fixture images -> per image a dict of (G, D) numpy arrays (the five planes, sum_fg, sum_bg) and
    "invalid" (D,).  Every output is one element too long and filled with a sentinel that must come back untouched; every element the
    kernel owns must have been written."""
    from pod_compare_amd import hip
    lib = hip.load()
    frames, det_off, gt_off, pair_off = tables(images)
    n_det, n_gt, n_pairs = int(det_off[-1]), int(gt_off[-1]), int(pair_off[-1])
    cat = lambda key, shape, dt: torch.from_numpy(np.concatenate([np.asarray(im[key]).reshape(shape) for im in images]).astype(dt)).to(DEV).contiguous()
    means, covs, probs = cat("means", (-1, 4), np.float32), cat("covs", (-1, 16), np.float32), cat("probs", (-1, fx.K), np.float32)
    gtb, gtc = cat("gt_boxes", (-1, 4), np.float32), cat("gt_classes", (-1,), np.int32)
    quality = torch.full((5 * n_pairs + 1,), SENTINEL, dtype=torch.float64, device=DEV)
    sums = torch.full((2 * n_pairs + 1,), SENTINEL, dtype=torch.float64, device=DEV)
    invalid = torch.full((n_det + 1,), ISENTINEL, dtype=torch.int32, device=DEV)
    ws = workspace(lib, len(images))
    hip.check(lib.pod_pdq_pairs(frames.data_ptr(), det_off.data_ptr(), gt_off.data_ptr(), pair_off.data_ptr(), len(images), hip.ptr(means),
                                hip.ptr(covs), hip.ptr(probs), fx.K, hip.ptr(gtb), hip.ptr(gtc), float(p_min), hip.ptr(ws), hip.ptr(quality),
                                hip.ptr(sums), hip.ptr(invalid), hip.current_stream()), "pod_pdq_pairs")
    quality, sums, invalid = quality.cpu().numpy(), sums.cpu().numpy(), invalid.cpu().numpy()
    assert quality[-1] == SENTINEL and sums[-1] == SENTINEL and invalid[-1] == ISENTINEL          # nothing written past the end
    assert not (quality[:-1] == SENTINEL).any() and not (sums[:-1] == SENTINEL).any()               # and every pair written
    if n_det:
        assert not (invalid[:-1] == ISENTINEL).any()
    out = []
    for m, im in enumerate(images):
        G, D = len(im["gt_boxes"]), len(im["means"])
        a, b = int(pair_off[m]), int(pair_off[m + 1])
        r = {name: quality[k * n_pairs + a:k * n_pairs + b].reshape(G, D).copy() for k, name in enumerate(pr.PLANES)}
        r["sum_fg"], r["sum_bg"] = sums[a:b].reshape(G, D).copy(), sums[n_pairs + a:n_pairs + b].reshape(G, D).copy()
        r["invalid"] = invalid[int(det_off[m]):int(det_off[m + 1])].astype(bool)
        out.append(r)
    return out


def assign(matrices, other_planes=None):
    """pod_pdq_assign on a list of (G, D) fp64 matrices (plane 0; planes 1 .. 4 are `other_planes[k]`, else multiples of it) ->
    per image (match (G,), counts (3,), sums (5,)), all numpy.  Sentinels as in `pairs`."""
    from pod_compare_amd import hip
    lib = hip.load()
    cum = lambda xs: torch.tensor([0] + list(xs), dtype=torch.int64).cumsum(0)
    nd, ng = [q.shape[1] for q in matrices], [q.shape[0] for q in matrices]
    det_off, gt_off = cum(nd).to(torch.int32).contiguous(), cum(ng).to(torch.int32).contiguous()
    pair_off = cum([q.size for q in matrices]).contiguous()
    n_gt, n_pairs, n = int(gt_off[-1]), int(pair_off[-1]), len(matrices)
    plane0 = np.concatenate([np.asarray(q, dtype=np.float64).reshape(-1) for q in matrices]) if matrices else np.zeros(0)
    planes = [plane0] + [plane0 * (k + 2) for k in range(4)] if other_planes is None else [plane0] + list(other_planes)
    quality = torch.from_numpy(np.concatenate(planes + [np.zeros(1)])).to(DEV).contiguous()
    match = torch.full((n_gt + 1,), ISENTINEL, dtype=torch.int32, device=DEV)
    counts = torch.full((3 * n + 1,), ISENTINEL, dtype=torch.int32, device=DEV)
    sums = torch.full((5 * n + 1,), SENTINEL, dtype=torch.float64, device=DEV)
    ws = workspace(lib, n)
    hip.check(lib.pod_pdq_assign(det_off.data_ptr(), gt_off.data_ptr(), pair_off.data_ptr(), n, hip.ptr(quality), hip.ptr(ws), hip.ptr(match),
                                 hip.ptr(counts), hip.ptr(sums), hip.current_stream()), "pod_pdq_assign")
    match, counts, sums = match.cpu().numpy(), counts.cpu().numpy(), sums.cpu().numpy()
    assert match[-1] == ISENTINEL and counts[-1] == ISENTINEL and sums[-1] == SENTINEL
    assert not (match[:-1] == ISENTINEL).any() and not (counts[:-1] == ISENTINEL).any() and not (sums[:-1] == SENTINEL).any()
    return [(match[int(gt_off[m]):int(gt_off[m + 1])].astype(np.int64), counts[3 * m:3 * m + 3].astype(np.int64), sums[5 * m:5 * m + 5].copy())
            for m in range(n)]


@functools.lru_cache(maxsize=None)
def referee():
    """The referee's numbers of fixtures.all_images(), computed once and shared (callers must not modify them)."""
    return [pr.image_ref(im["frame"], im["means"], im["covs"], im["probs"], im["gt_boxes"], im["gt_classes"]) for im in fx.all_images()]
