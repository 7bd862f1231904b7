"""Times pod_reg_scores (K33: energy score + CRPS per detection) at n = 100 000 and n = 1 000 rows, M = 1000 draws, beside a plain-torch
statement of the same estimator on the same GPU -- torch.randn normals materialised as (M + 1, n, 4), fp64 after them, torch.linalg.cholesky
for the factor.  Seeded Wishart covariances (tests' `wishart` family's recipe).  Every figure is the median over WINDOWS windows of CALLS
calls enqueued back to back between two device events, after a warm-up window; the windows' minimum and maximum are kept beside it.  A
window holds at least CALLS calls and as many more as make it WINDOW_S long by the warm-up's rate; at n = 1 000 a call is shorter than a
launch, so that figure is the rate of back-to-back launches.

    python tools/eval_scores_bench.py [--out profiles/eval_scores.json]
"""
import argparse
import json
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pod_compare_amd import hip      # noqa: E402

WINDOWS, CALLS, WINDOW_S, M = 5, 20, 0.2, 1000
SIZES = (100_000, 1_000)


def rows(n, dev):
    g = torch.Generator().manual_seed(33)
    l = torch.randn(n, 4, 4, generator=g)
    covs = l @ l.transpose(1, 2) + 0.5 * torch.eye(4)
    means = 300.0 + 50.0 * torch.randn(n, 4, generator=g)
    gt = means + 2.0 * torch.randn(n, 4, generator=g)
    return means.to(dev), (0.5 * (covs + covs.transpose(1, 2))).to(dev), gt.to(dev)


def torch_scores(means, covs, gt, m):
    """The same two rules in eager torch: fp32 normals, fp64 after them."""
    n = means.shape[0]
    sig = (covs + 1e-2 * torch.eye(4, dtype=torch.float32, device=covs.device)).double()
    L = torch.linalg.cholesky(sig)
    d = means.double() - gt.double()
    eps = torch.randn(m + 1, n, 4, device=means.device)
    u1 = d.unsqueeze(0) + torch.einsum("nij,snj->sni", L, eps[:-1].double())
    u2 = torch.einsum("nij,snj->sni", L, (eps[:-1] - eps[1:]).double())
    energy = u1.norm(dim=-1).mean(0) - 0.5 * u2.norm(dim=-1).mean(0)
    sd = torch.sqrt(torch.diagonal(sig, dim1=-2, dim2=-1))
    z = -d / sd
    crps = (sd * (z * torch.special.erf(z / math.sqrt(2.0)) + 2.0 * torch.exp(-0.5 * z * z) / math.sqrt(2.0 * math.pi) - 1.0 / math.sqrt(math.pi))).mean(-1)
    return energy.float(), crps.float()


def timed(call):
    sync = lambda: torch.cuda.current_stream().synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    call()
    sync()
    e0.record()
    for _ in range(CALLS):
        call()
    e1.record()
    sync()
    calls = min(5000, max(CALLS, int(WINDOW_S * 1e3 / max(e0.elapsed_time(e1) / CALLS, 1e-4))))
    out = []
    for _ in range(WINDOWS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            call()
        e1.record()
        sync()
        out.append(e0.elapsed_time(e1) / calls)
    return {"median_ms": statistics.median(out), "min_ms": min(out), "max_ms": max(out), "calls_per_window": calls}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default="")
    ap.add_argument("--device", default="cuda:0")
    args = ap.parse_args(argv)
    dev = torch.device(args.device)
    torch.cuda.set_device(dev)
    lib, stream = hip.load(), hip.current_stream()
    result = {"num_samples": M, "windows": WINDOWS, "window_seconds": WINDOW_S, "device": torch.cuda.get_device_name(dev)}
    for n in SIZES:
        means, covs, gt = rows(n, dev)
        energy, crps = torch.empty(n, device=dev), torch.empty(n, device=dev)

        def kernel(e=energy, c=crps, m=M):
            hip.check(lib.pod_reg_scores(hip.ptr(means), hip.ptr(covs), hip.ptr(gt), n, m, 7, None, None, hip.ptr(e) if e is not None else None,
                                         hip.ptr(c) if c is not None else None, stream), "pod_reg_scores")

        r = {"pod_reg_scores, energy + crps": timed(kernel), "pod_reg_scores, energy": timed(lambda: kernel(c=None)),
             "pod_reg_scores, crps": timed(lambda: kernel(e=None)), "eager torch, energy + crps": timed(lambda: torch_scores(means, covs, gt, M))}
        kernel()
        te, tc = torch_scores(means, covs, gt, M)
        # two independent sets of draws: the means over the rows agree to their sampling error; the CRPS has no draws
        r["mean_energy"] = {"pod_reg_scores": float(energy.double().mean()), "eager torch": float(te.double().mean())}
        r["max_abs_crps_difference"] = float((crps - tc).abs().max())
        r["samples_per_second"] = n * M / (r["pod_reg_scores, energy + crps"]["median_ms"] * 1e-3)
        result["n = %d" % n] = r
    print(json.dumps(result, indent=1))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
    return result


if __name__ == "__main__":
    main()
