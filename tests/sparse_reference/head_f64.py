"""A plain restatement of the reference head (PR:403-537) with torch.nn.functional.conv2d on the CPU, the number format a parameter.
It knows nothing of pod_compare_amd.modeling: parameters and features come from the seeded generators of oracle/model_fixture.py (any
level list), dropout masks from a callable with HeadFixture.replay's signature, and the output is the reference's (N, H*W*A, C) layout.
In float64 it is the referee the sparse bbox tower is held to at geometries the fixtures do not have; tests/sparse_reference/
test_head_f64_cpu.py pins it to the fixtures first (measured: profiles/sparse_reference.md)."""
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch
import torch.nn.functional as F

from oracle import model_fixture as mf

FIELDS = ("box_cls", "box_delta", "box_cls_var", "box_reg_var")
NUM_CONVS, NUM_ANCHORS, NUM_CLASSES = mf.NUM_CONVS, 9, mf.NUM_CLASSES


def reference_keys(variant: dict) -> Dict[str, Tuple[int, ...]]:
    """Reference state-dict key -> shape divided by the channel count, for a variant of oracle.model_fixture.VARIANTS: the j-th conv of a
    subnet is entry 3 j of nn.Sequential(conv, ReLU, Dropout, ...) with dropout, 2 j without (PR:403-427)."""
    step = 3 if variant["dropout_rate"] > 0.0 else 2
    out = {}
    for subnet in ("cls_subnet", "bbox_subnet"):
        for j in range(NUM_CONVS):
            out["%s.%d" % (subnet, step * j)] = None
    out["cls_score"], out["bbox_pred"] = NUM_ANCHORS * NUM_CLASSES, NUM_ANCHORS * 4
    if variant["cls_var"]:
        out["cls_var"] = NUM_ANCHORS * NUM_CLASSES
    if variant["bbox_cov"]:
        out["bbox_cov"] = NUM_ANCHORS * variant["cov_dims"]
    return out


def seeded_parameters(variant: dict, seed: int, channels: int, dtype=torch.float64) -> Dict[str, torch.Tensor]:
    """The variant's parameters under the reference's key names (float32 values, held in `dtype`)."""
    params = {}
    for name, planes in reference_keys(variant).items():
        k = channels if planes is None else planes
        params[name + ".weight"] = mf.seeded_parameter(name + ".weight", (k, channels, 3, 3), seed).to(dtype)
        params[name + ".bias"] = mf.seeded_parameter(name + ".bias", (k,), seed).to(dtype)
    return params


def permute_to_N_HWA_K(t: torch.Tensor, k: int) -> torch.Tensor:
    """(N, A*K, H, W) -> (N, H*W*A, K), PR:343-349."""
    n, _, h, w = t.shape
    return t.view(n, -1, k, h, w).permute(0, 3, 4, 1, 2).reshape(n, -1, k)


class SeededMasks:
    """Keep-masks (Bernoulli(1 - p)) from numpy's MT19937, addressed like oracle.model_fixture.MaskReader: (subnet 0 = cls / 1 = bbox,
    evaluation 0 = mean / 1 = variance branch, run, level, layer): a stream per address, so the order of the calls does not matter."""

    def __init__(self, seed: int, p: float):
        self.seed, self.p, self._made = int(seed), float(p), {}

    def get(self, subnet: int, evaluation: int, run: int, level: int, layer: int, shape) -> torch.Tensor:
        key = (subnet, evaluation, run, level, layer) + tuple(shape)
        if key not in self._made:
            rs = np.random.RandomState((self.seed * 1000003 + (((subnet * 2 + evaluation) * 64 + run) * 16 + level) * 16 + layer) & 0xFFFFFFFF)
            self._made[key] = torch.from_numpy(rs.random_sample(tuple(shape)) >= self.p)
        return self._made[key]


def replay_of(masks, levels: Sequence[Tuple[int, int]], channels: int, n: int, m: Optional[int] = None) -> Callable:
    """(subnet, layer, level, copy) -> (C, H, W) keep-mask, HeadFixture.replay's signature and copy order: cls copies [0, m) are the mean
    branch of runs 0 .. m-1 and [m, 2m) the variance branch; bbox copies [0, n) the mean and [n, n + m) the variance branch."""
    m = n if m is None else m

    def fn(sid, layer, level, copy):
        first = m if sid == 0 else n
        ev, run = (0, copy) if copy < first else (1, copy - first)
        return masks.get(sid, ev, run, level, layer, (1, channels) + tuple(levels[level]))[0]
    return fn


def head_f64(params: Dict[str, torch.Tensor], features: List[torch.Tensor], variant: dict, replay: Optional[Callable] = None, runs: int = 1,
             dtype=torch.float64, sides=(0, 1)) -> Dict[str, Optional[List[torch.Tensor]]]:
    """PR:486-537 on one image.  replay None: eval mode (nn.Dropout is the identity), one evaluation.  replay given (with all `runs` runs'
    masks: m = n): the MC branch of PR:103-108, `features * runs` -- every subnet evaluation draws masks of its own, the mean and the
    variance predictor of a side each evaluate the subnet (PR:518-523).  sides: 0 = cls, 1 = bbox.  -> field -> per level (N, H*W*A, C)."""
    p = float(variant["dropout_rate"])
    step = 3 if p > 0.0 else 2
    P = {k: v.to(dtype) for k, v in params.items()}
    n = runs if replay is not None else 1

    def conv(name, x):
        return F.conv2d(x, P[name + ".weight"], P[name + ".bias"], padding=1)

    def subnet(name, sid, x, level, copy):
        for j in range(NUM_CONVS):                               # conv -> ReLU -> Dropout (PR:403-427)
            x = F.relu(conv("%s.%d" % (name, step * j), x))
            if replay is not None:
                x = x * (replay(sid, j, level, copy)[None].to(dtype) / (1.0 - p))
        return x

    out = {f: None for f in FIELDS}
    jobs = [("box_cls", "cls_score", "cls_subnet", 0, 0, NUM_CLASSES), ("box_delta", "bbox_pred", "bbox_subnet", 1, 0, 4)]
    if variant["cls_var"]:
        jobs.append(("box_cls_var", "cls_var", "cls_subnet", 0, 1, NUM_CLASSES))
    if variant["bbox_cov"]:
        jobs.append(("box_reg_var", "bbox_cov", "bbox_subnet", 1, 1, variant["cov_dims"]))
    with torch.no_grad():
        for field, pred, sub, sid, ev, k in jobs:
            if sid not in sides:
                continue
            out[field] = []
            for level, f in enumerate(features):
                x = f.to(dtype)
                # the replay callable counts copies: the variance branch's follow the n mean-branch copies of its side (m = n here)
                rows = [conv(pred, subnet(sub, sid, x, level, ev * n + run)) for run in range(n)]
                out[field].append(permute_to_N_HWA_K(torch.cat(rows), k))
    return out
