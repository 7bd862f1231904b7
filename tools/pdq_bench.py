"""Times PDQ's two kernels (K34: pod_pdq_pairs, pod_pdq_assign) at 1, 100 and 1 000 images of 1280x720 with 20 ground truths and 30
detections each, beside the same formulas in eager torch fp64 on the same GPU: per detection its region of interest as the kernel takes it,
P and Q on that (rows, columns) grid with the kernel's quadrature as one (pixels, nodes) tensor, the two sums per ground truth by masks.
The eager statement is a Python loop over detections; it is timed at 1 and 100 images only (EAGER_MAX_IMAGES) and compared with the
kernel's planes there.  Seeded boxes: ground truths 40 .. 300 px wide, 40 .. 200 px high; 20 detections are ground truths jittered by
N(0, 3^2) and 10 lie anywhere; full covariances L L^T with diag(L) in [1, 4].  Every figure is the median of REPEATS calls between two device
events after one warm-up call; the minimum and maximum are kept beside it.

    python tools/pdq_bench.py [--out profiles/pdq.json] [--sizes 1 100 1000]
"""
import argparse
import json
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pod_compare_amd import evaluation_utils as ev      # noqa: E402

REPEATS, EAGER_MAX_IMAGES = 5, 100
W, H, G, D, K = 1280, 720, 20, 30, 7
SMALL, RHO_MAX = 1e-14, 0.99
GL_X = [0.076526521133497338, 0.2277858511416451, 0.37370608871541955, 0.51086700195082713, 0.63605368072651502,
        0.7463319064601508, 0.83911697182221878, 0.91223442825132584, 0.96397192727791381, 0.99312859918509488]
GL_W = [0.15275338713072578, 0.14917298647260366, 0.14209610931838187, 0.13168863844917653, 0.11819453196151825,
        0.10193011981724026, 0.083276741576704671, 0.062672048334109443, 0.040601429800386217, 0.017614007139153273]


def data_set(n, dev):
    g = torch.Generator().manual_seed(34)
    r = lambda *s: torch.rand(*s, generator=g)
    wh = torch.stack([40.0 + 260.0 * r(n, G), 40.0 + 160.0 * r(n, G)], -1)
    xy = torch.stack([r(n, G) * (W - wh[..., 0]), r(n, G) * (H - wh[..., 1])], -1)
    gt = torch.cat([xy, xy + wh], -1)
    near = gt + 3.0 * torch.randn(n, G, 4, generator=g)
    far_xy = torch.stack([r(n, D - G) * (W - 200.0), r(n, D - G) * (H - 150.0)], -1)
    far = torch.cat([far_xy, far_xy + torch.stack([50.0 + 150.0 * r(n, D - G), 40.0 + 110.0 * r(n, D - G)], -1)], -1)
    means = torch.cat([near, far], 1)
    L = torch.tril(0.7 * torch.randn(n, D, 4, 4, generator=g), -1) + torch.diag_embed(1.0 + 3.0 * r(n, D, 4))
    covs = L @ L.transpose(-1, -2)
    probs = torch.softmax(torch.randn(n, D, K, generator=g), -1)
    classes = torch.randint(0, K, (n, G), generator=g)
    f = lambda t, *s: t.reshape(*s).float().contiguous().to(dev)
    return f(means, -1, 4), f(covs, -1, 4, 4), f(probs, -1, K), f(gt, -1, 4), classes.reshape(-1).to(torch.int32).to(dev)


def timed(call, repeats=REPEATS):
    sync = lambda: torch.cuda.current_stream().synchronize()
    call()
    sync()
    out = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        sync()
        out.append(e0.elapsed_time(e1))
    return {"median_ms": statistics.median(out), "min_ms": min(out), "max_ms": max(out), "calls": repeats}


def phi(x):
    return 0.5 * torch.special.erfc(-x / math.sqrt(2.0))


def eager_pairs(means, covs, probs, gt, classes, n_images, p_min=ev.PDQ_P_MIN):
    """The five planes, (5, n_images * G * D) fp64, by the kernel's formulas in eager torch (every image has G ground truths, D detections)."""
    dev = means.device
    f64 = lambda v: torch.tensor(v, dtype=torch.float64, device=dev)
    gx, gw = torch.cat([-f64(GL_X).flip(0), f64(GL_X)]), torch.cat([f64(GL_W).flip(0), f64(GL_W)])
    z = math.sqrt(2.0) * float(torch.special.erfinv(torch.tensor(2.0 * p_min - 1.0, dtype=torch.float64)))
    out = torch.zeros((5, n_images * G * D), dtype=torch.float64, device=dev)
    var = (torch.diagonal(covs, dim1=-2, dim2=-1) + 1e-2).double()
    sd_all, mu_all = var.sqrt().cpu(), means.double().cpu()
    rho_all = torch.stack([covs[:, 1, 0].double().cpu() / (sd_all[:, 0] * sd_all[:, 1]), covs[:, 3, 2].double().cpu() / (sd_all[:, 2] * sd_all[:, 3])], -1).clamp(-RHO_MAX, RHO_MAX)
    gtd = gt.double()
    ga, gb = torch.ceil(gtd[:, 0] - 0.5).clamp(0, W), torch.ceil(gtd[:, 2] - 0.5).clamp(0, W)
    gc, gd = torch.ceil(gtd[:, 1] - 0.5).clamp(0, H), torch.ceil(gtd[:, 3] - 0.5).clamp(0, H)
    n_i = (gb - ga).clamp(min=0) * (gd - gc).clamp(min=0)

    def integral(h, k, rho):
        top = math.asin(rho)
        if top == 0.0:
            return torch.zeros_like(h * k)
        panels = min(4, math.ceil(abs(top) / (math.asin(RHO_MAX) / 4)))
        half = 0.5 * top / panels
        t = torch.cat([half * (2 * p + 1) + half * gx for p in range(panels)])
        wt = (gw * half / (2.0 * math.pi)).repeat(panels)
        a, b = (h * h + k * k).unsqueeze(-1), (2.0 * h * k).unsqueeze(-1)
        return (wt * torch.exp(-(a - b * torch.sin(t)) / (2.0 * torch.cos(t) ** 2))).sum(-1)

    for d in range(means.shape[0]):
        m, j = divmod(d, D)
        mu, sd, rho = mu_all[d].tolist(), sd_all[d].tolist(), rho_all[d].tolist()
        u0 = int(min(max(math.floor(mu[0] + z * sd[0] - 0.5) - 1, 0), W))
        u1 = int(min(max(math.ceil(mu[2] - z * sd[2] - 0.5) + 2, 0), W))
        v0 = int(min(max(math.floor(mu[1] + z * sd[1] - 0.5) - 1, 0), H))
        v1 = int(min(max(math.ceil(mu[3] - z * sd[3] - 0.5) + 2, 0), H))
        if u1 <= u0 or v1 <= v0:
            continue
        us, vs = torch.arange(u0, u1, device=dev), torch.arange(v0, v1, device=dev)
        cx, cy = (us.double() + 0.5)[None, :], (vs.double() + 0.5)[:, None]
        h1, k1, h2, k2 = (cx - mu[0]) / sd[0], (cy - mu[1]) / sd[1], (mu[2] - cx) / sd[2], (mu[3] - cy) / sd[3]
        i1, i2 = integral(h1, k1, rho[0]), integral(h2, k2, rho[1])
        A, B = phi(h1) * phi(k1) + i1, phi(h2) * phi(k2) + i2
        Ac = phi(-h1) + phi(-k1) - (phi(-h1) * phi(-k1) + i1)
        Bc = phi(-h2) + phi(-k2) - (phi(-h2) * phi(-k2) + i2)
        P = A * B
        T = P >= p_min
        lp = torch.where(T, torch.log(P.clamp(min=SMALL)), torch.zeros_like(P))
        lq = torch.where(T, torch.log((Ac + A * Bc).clamp(min=SMALL)), torch.zeros_like(P))
        rows = slice(m * G, (m + 1) * G)
        inside = ((us[None, None, :] >= ga[rows, None, None]) & (us[None, None, :] < gb[rows, None, None])
                  & (vs[None, :, None] >= gc[rows, None, None]) & (vs[None, :, None] < gd[rows, None, None]))          # (G, rows, columns)
        cnt = (inside & T).sum((1, 2)).double()
        s_fg = (lp * inside).sum((1, 2)) + math.log(SMALL) * (n_i[rows] - cnt)
        s_bg = (lq * ~inside).sum((1, 2))
        ok = (n_i[rows] > 0) & (cnt > 0)
        n = n_i[rows].clamp(min=1)
        q_label = probs[d, classes[rows].long()].double()
        q_sp = torch.exp((s_fg + s_bg) / n)
        vals = torch.stack([torch.sqrt(q_sp * q_label), q_sp, q_label, torch.exp(s_fg / n), torch.exp(s_bg / n)])
        at = m * G * D + torch.arange(G, device=dev) * D + j
        out[:, at] = torch.where(ok, vals, torch.zeros_like(vals))
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default="")
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--sizes", type=int, nargs="+", default=[1, 100, 1000])
    args = ap.parse_args(argv)
    dev = torch.device(args.device)
    torch.cuda.set_device(dev)
    result = {"frame": [W, H], "ground_truths": G, "detections": D, "repeats": REPEATS, "device": torch.cuda.get_device_name(dev)}
    for n in args.sizes:
        means, covs, probs, gt, classes = data_set(n, dev)
        tables = ev.PdqTables([(W, H)] * n, [D] * n, [G] * n, dev)
        quality, _ = ev.pdq_pair_quality(tables, means, covs, probs, gt, classes)
        r = {"pod_pdq_pairs": timed(lambda: ev.pdq_pair_quality(tables, means, covs, probs, gt, classes)),
             "pod_pdq_assign": timed(lambda: ev.pdq_assign(tables, quality))}
        _, counts, sums = ev.pdq_assign(tables, quality)
        tp, fp, fn = (int(v) for v in counts.sum(0).tolist())
        r["TP_FP_FN"] = [tp, fp, fn]
        r["PDQ"] = float(sums[:, 0].sum()) / max(tp + fp + fn, 1)
        if n <= EAGER_MAX_IMAGES:
            r["eager torch fp64, pairs"] = timed(lambda: eager_pairs(means, covs, probs, gt, classes, n), repeats=1 if n > 1 else 3)
            r["max_abs_plane_difference"] = float((eager_pairs(means, covs, probs, gt, classes, n) - quality).abs().max())
        result["images = %d" % n] = r
        print("images = %d: %s" % (n, json.dumps(r)), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
    return result


if __name__ == "__main__":
    main()
