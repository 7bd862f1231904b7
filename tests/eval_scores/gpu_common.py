"""What the GPU tests of tests/eval_scores/ share: the direct call of pod_reg_scores with sentinels behind every output, and the kernel's
draws restated on the host (rng_ref's words through the kernels' own box_muller16).  Imports without a GPU."""
import numpy as np
import torch

from tests.eval_instrument import instrument_ref as ir
from tests.eval_scores import scores_ref as sr

DEV = "cuda:0"


def reg_scores(means, covs, gt, M=16, seed=0, energy=True, crps=True, eps_in=None, want_eps=False):
    """pod_reg_scores on CPU tensors -> dict(energy, crps, eps) of CPU tensors (the keys asked for).  Every output is allocated one row
    (eps: one sample) too long and filled with a sentinel: the element past the end must come back untouched."""
    from pod_compare_amd import hip
    lib = hip.load()
    d = [t.to(DEV).contiguous() for t in (means, covs, gt)]
    n = int(means.shape[0])
    sent = float(ir.SENTINEL)
    out = {k: torch.full((n + 1,), sent, device=DEV) for k, on in (("energy", energy), ("crps", crps)) if on}
    eps_out = torch.full(((M + 1) * n * 4 + 4,), sent, device=DEV) if want_eps else None
    eps_dev = None if eps_in is None else eps_in.to(DEV).contiguous()
    assert eps_dev is None or tuple(eps_dev.shape) == (M + 1, n, 4)
    hip.check(lib.pod_reg_scores(hip.ptr(d[0]), hip.ptr(d[1]), hip.ptr(d[2]), n, M, seed, hip.ptr(eps_dev), hip.ptr(eps_out),
                                 hip.ptr(out.get("energy")), hip.ptr(out.get("crps")), hip.current_stream()), "pod_reg_scores")
    res = {}
    for k, v in out.items():
        v = v.cpu()
        assert float(v[n]) == sent, k          # nothing written past row n - 1
        res[k] = v[:n]
    if want_eps:
        e = eps_out.cpu()
        assert bool((e[-4:] == sent).all())
        res["eps"] = e[:-4].view(M + 1, n, 4)
        assert bool((res["eps"] != sent).all())          # and every normal of every row written
    return res


def gpu_box_muller(words):
    """numpy uint32, any shape -> fp32 (..., 2) on the CPU: the kernels' box_muller16 of every word (pod_debug_box_muller16)."""
    from pod_compare_amd import hip
    src = torch.from_numpy(np.ascontiguousarray(words.reshape(-1), dtype=np.uint32).view(np.int32)).to(DEV)
    out = torch.empty((src.numel(), 2), dtype=torch.float32, device=DEV)
    hip.check(hip.load().pod_debug_box_muller16(src.data_ptr(), out.data_ptr(), src.numel(), hip.current_stream()), "pod_debug_box_muller16")
    return out.cpu().view(*words.shape, 2)


def expected_normals(key, rows, M):
    """(M + 1, n, 4) fp32: the normals rows `rows` must draw under `key` -- host words, the kernels' own box_muller16, host layout."""
    word, which = sr.eval_score_normals(key, rows, M)
    z = gpu_box_muller(word)
    return torch.gather(z, -1, torch.from_numpy(which.astype(np.int64))[..., None])[..., 0]


def rel_err(got, ref):
    return float(((got.double() - ref).abs() / ref.abs().clamp(min=1.0)).max())
