"""What recalibration (K36, pod_recal_*) costs against its fp64 host restatement.

Seeded detections as the tests' fixture draws them (box residuals over- and under-confident, class probabilities over-confident by a
factor 2 in logit space), --detections of them with --classes probability columns, three quarters matched:

  fit   the temperature's Newton loop (pod_recal_cls_sums per step, the logits computed once), the residuals and the moment fit
        (pod_recal_reg_z, pod_recal_moment), the grid fit (pod_recal_ece_grid: two segmented sorts and 4 x 1025 x 14 searches);
  apply pod_recal_apply on a record table of 100 slots per image.

Wall time per call with the device drained before and after each timed window (the fit steps read their results back, as a user's fit
does); a window is 10 temperature fits, 100 moment or grid fits or 500 applies back to back, so that it lasts a good fraction of a second;
one warm-up, then --repeats windows: median, minimum, maximum.  The host column is tests/recalibration/recal_ref.py on the same arrays, numpy on this
machine's CPU, once.

    python tools/recalibration_bench.py [--detections 1000000] [--out recalibration_bench.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
from pod_compare_amd import recalibration as rc      # noqa: E402
from tests.recalibration import recal_ref as ref     # noqa: E402


def timed(fn, repeats, inner):
    """Seconds per call: `inner` calls back to back in every timed window (a window of a fraction of a millisecond would measure the
    clock and the scheduler), the device drained before and after."""
    fn()
    out = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(inner):
            fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t) / inner)
    return {"median_s": statistics.median(out), "min_s": min(out), "max_s": max(out), "calls_per_window": inner}


def once(fn):
    t = time.perf_counter()
    res = fn()
    return time.perf_counter() - t, res


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--detections", type=int, default=1000000)
    ap.add_argument("--classes", type=int, default=7)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--skip-host", action="store_true")
    ap.add_argument("--out", default="")
    ap.add_argument("--device", default="cuda:0")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("recalibration_bench.py measures on the GPU: none found")
    dev = torch.device(args.device)
    torch.cuda.set_device(dev)
    n, K = args.detections, args.classes
    n_m = 3 * n // 4
    fx = ref.fixture(n_m, n - n_m, K)
    rng = np.random.default_rng(1)
    p, y = fx["p"].reshape(-1), fx["labels"].reshape(-1)
    gt = rng.uniform(0.0, 1000.0, size=(n_m, 4)).astype(np.float32)
    means = (gt.astype(np.float64) - fx["resid"]).astype(np.float32)
    covs = np.zeros((n_m, 4, 4), dtype=np.float32)
    covs[:, np.arange(4), np.arange(4)] = (fx["sigma"] ** 2).astype(np.float32)
    n_img = -(-n // 100)
    rec = rng.uniform(0.0, 50.0, size=(n_img, 100, 6 + K + 16)).astype(np.float32)
    rec[:, :, 6:6 + K] = np.resize(fx["p"], (n_img * 100, K)).reshape(n_img, 100, K)
    rec[:, :, 4] = rec[:, :, 6:6 + K].max(2)
    counts = np.full(n_img, 100, dtype=np.int32)
    counts[-1] = n - 100 * (n_img - 1)
    t = lambda a: torch.from_numpy(a).to(dev)
    tp, ty, tm, tc, tg, trec, tcnt = t(p), t(y), t(means), t(covs), t(gt), t(rec), t(counts)
    recal = rc.Recalibration(beta=0.5, scales=[[2.0, 0.67, 2.0, 0.67]])
    state = {}

    def gpu_moment():
        z, seg, _ = rc.reg_z(tm, tc, tg)
        state["grouped"] = rc.moment(z, seg, 4)
        return state["grouped"][3].cpu()

    res = {"device": torch.cuda.get_device_name(dev), "detections": n, "classes": K, "scores": int(p.size), "matched": n_m, "repeats": args.repeats, "gpu": {}, "host": {}}
    res["gpu"]["temperature"] = timed(lambda: state.__setitem__("beta", rc.fit_temperature(tp, ty)), args.repeats, 10)
    res["gpu"]["residuals_moment"] = timed(gpu_moment, args.repeats, 100)
    res["gpu"]["ece_grid"] = timed(lambda: rc.ece_grid(*state["grouped"][:3])[1].cpu(), args.repeats, 100)
    res["gpu"]["apply"] = timed(lambda: rc.apply_to_records(trec, tcnt, K, recal), args.repeats, 500)
    res["gpu"]["beta"], res["gpu"]["newton_iterations"] = state["beta"][0], state["beta"][1]
    if not args.skip_host:
        res["host"]["temperature_s"], (beta, its) = once(lambda: ref.fit_temperature(p, y))
        res["host"]["beta"], res["host"]["newton_iterations"] = beta, its

        def host_moment():
            z, seg, _ = ref.reg_z(means, covs, gt)
            zg, off = ref.group(z, seg, 4)
            return zg, off, ref.moment(zg, off)
        res["host"]["residuals_moment_s"], (zg, off, _) = once(host_moment)
        res["host"]["ece_grid_s"], _ = once(lambda: ref.ece_fit(zg, off))
        res["host"]["apply_s"], _ = once(lambda: ref.apply_records(rec, counts, K, recal.beta, recal.scales))
    for k, v in res["gpu"].items():
        if isinstance(v, dict):
            host = res["host"].get(k + "_s")
            print("%-18s GPU %8.2f ms (%.2f - %.2f)%s" % (k, 1e3 * v["median_s"], 1e3 * v["min_s"], 1e3 * v["max_s"],
                                                         "" if host is None else "   host restatement %9.1f ms   x%.0f" % (1e3 * host, host / v["median_s"])), flush=True)
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    return res


if __name__ == "__main__":
    main()
