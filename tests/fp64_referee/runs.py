"""Fixture plumbing of the fp64 referee tests: one fp32 oracle run per predictor fixture (with its decisions), the referee
chained over it at float32 and float64, and the measured-reference figures of profiles/fp64_referee.md.

`python -m tests.fp64_referee.runs` prints the CPU section of that file."""
import functools

import torch

from oracle import pod_oracle as po
from pod_compare_amd import synthetic
from tests.helpers import Golden, fixture_id, fixture_paths
from tests.fp64_referee import f64_ref as fr

ALL = fixture_paths()
FULL_OVER_BAR = ("full_worst_cfg3_bayes_od_mc10_s1006", "full_cfg5_ensembles_pre_nms_s1005")


def fixture_kwargs(g: Golden, ho=None):
    """(reference-layout inputs, modes) of a fixture."""
    s = g.spec
    ho = g.head_outputs() if ho is None else ho
    runs = [synthetic.to_reference_layout(ho, r) for r in range(s["runs"])]
    modes = dict(box_merge_mode=s.get("box_merge", "bayesian_inference"), cls_merge_mode=s.get("cls_merge", "max_score"))
    return runs, modes


def staged(mode, runs, p: po.PathParams, img, out, eps_fn, modes=None, post_nms=False):
    """The fp32 oracle run on reference-layout `runs` (one dict per run) with `eps_fn`'s normals, and the LevelInputs the referee reads."""
    modes = modes or {}
    if post_nms:
        run = fr.oracle_run_post_nms(p, img, out, runs, eps_fn)
        levels = [fr.level_inputs(o, None, p.merge_quirk) for o in runs]
    elif len(runs) > 1:
        run = fr.oracle_run(mode, p, img, out, run_outputs=runs, eps_fn=eps_fn, **modes)
        levels = [fr.level_inputs(None, runs, p.merge_quirk)]
    else:
        run = fr.oracle_run(mode, p, img, out, outputs=runs[0], eps_fn=eps_fn, **modes)
        levels = [fr.level_inputs(runs[0], None, p.merge_quirk)]
    return run, levels


def oracle_and_levels(g: Golden, p: po.PathParams, eps_fn, ho=None):
    """The same for a fixture."""
    runs, modes = fixture_kwargs(g, ho)
    run, levels = staged(g.spec.get("mode"), runs, p, tuple(g.meta["image"]), tuple(g.meta["out"]), eps_fn, modes, bool(g.spec.get("post_nms")))
    return run, levels, modes


def chain(g: Golden, run, levels, modes, p, dtype):
    return fr.referee_chain(run, g.spec.get("mode", "standard_nms"), dtype, p.box_weights, levels, image_size=tuple(g.meta["image"]),
                            out_size=tuple(g.meta["out"]), **modes)


@functools.lru_cache(maxsize=None)
def golden_run(path):
    """(Golden, params, oracle run, levels, modes, fp64 chain) of a fixture on its own recorded normals; computed once per session."""
    g = Golden(path)
    p = po.PathParams(topk_candidates=g.meta["topk"])
    run, levels, modes = oracle_and_levels(g, p, g.eps_source())
    return g, p, run, levels, modes, chain(g, run, levels, modes, p, torch.float64)


def cat_cand(run, c64):
    """Candidate boxes / covariances of a run, members concatenated: (oracle boxes, referee boxes, oracle cov | None, referee cov | None)."""
    b32, b64 = torch.cat([a.boxes for a in run.aw]), torch.cat([c.boxes for c in c64.cand])
    if run.aw[0].cov is None:
        return b32, b64, None, None
    return b32, b64, torch.cat([a.cov for a in run.aw]), torch.cat([c.cov for c in c64.cand])


def measure(path):
    """The fp32 oracle against the fp64 referee on one fixture: per quantity the figures of the CPU table."""
    g, p, run, levels, modes, c64 = golden_run(path)
    b32, b64, k32, k64 = cat_cand(run, c64)
    out = {"n": int(b32.shape[0]), "m": len(run.det)}
    for name, x, ref in (("candidate boxes", b32, b64), ("final boxes", run.det.pred_boxes, c64.det.boxes)):
        worst, rms, _ = fr.stats(fr.box_error(x, ref))
        out[name] = dict(worst=worst, rms=rms, elem=fr.bar_fractions(x, ref)[0])
    for name, x, ref in (("candidate cov", k32, k64), ("final cov", run.det.pred_boxes_covariance, c64.det.cov)):
        if x is None:
            continue
        worst, rms, _ = fr.stats(fr.cov_error(x, ref))
        elem, mat = fr.bar_fractions(x, ref)
        out[name] = dict(worst=worst, rms=rms, elem=elem, mat=mat)
    return out


def cpu_table():
    lines = ["| fixture | n | m | quantity | worst fraction of the element-wise 1e-4 bar | of the per-matrix bar | worst normalised error | rms |",
             "|---|---|---|---|---|---|---|---|"]
    for path in ALL:
        r = measure(path)
        for q in ("candidate boxes", "candidate cov", "final boxes", "final cov"):
            if q in r:
                v = r[q]
                lines.append("| `%s` | %d | %d | %s | %.3g | %s | %.2e | %.2e |" % (
                    fixture_id(path), r["n"], r["m"], q, v["elem"], ("%.3g" % v["mat"]) if "mat" in v else "-", v["worst"], v["rms"]))
    return "\n".join(lines)


def gpu_section(json_path):
    """From the parity_errors_fp64.json a GPU session leaves (tests/helpers.py: write_parity_report): the worst ratio per quantity
    and where it occurred, then every row."""
    import json
    rows = json.load(open(json_path))
    short = lambda r: r["test"].split("::", 1)[-1]
    out = ["| quantity | rows | worst e_hip / e_ref (max) | in | worst e_hip / e_ref (rms) | in |", "|---|---|---|---|---|---|"]
    for q in sorted({r["quantity"] for r in rows}):
        # ratios only where one side's worst error is above the rule's floor (4 ulps): below it both sides are exact to a few ulps
        sel = [r for r in rows if r["quantity"] == q and max(r["ref_max"], r["hip_max"]) > fr.FLOOR]
        if not sel:
            continue
        a, b = max(sel, key=lambda r: r["ratio_max"]), max(sel, key=lambda r: r["ratio_rms"])
        out.append("| %s | %d | %.2f | `%s` | %.2f | `%s` |" % (q, len(sel), a["ratio_max"], short(a), b["ratio_rms"], short(b)))
    out += ["", "| test | quantity | entries | e_hip max | e_ref max | ratio | e_hip rms | e_ref rms | ratio |", "|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        out.append("| `%s` | %s | %d | %.2e | %.2e | %.2f | %.2e | %.2e | %.2f |" % (
            short(r), r["quantity"], r["n"], r["hip_max"], r["ref_max"], r["ratio_max"], r["hip_rms"], r["ref_rms"], r["ratio_rms"]))
    return "\n".join(out)


if __name__ == "__main__":
    import sys
    print(gpu_section(sys.argv[2]) if sys.argv[1:2] == ["gpu"] else cpu_table())
