"""Offline evaluation step 3, the calibration errors, with the calibration pass on the GPU (csrc/k18_calibration.hip) against the host
function `calibration_errors`; the test-set category maps of PM / CE (EU:370-397); apply_net's --eval / --eval-only chain (AN:104-106).

The module shares its name with tests/test_probabilistic_metrics.py (step 2 of the same chain) so that the GPU run order in
tests/conftest.py (GPU_ORDER, keyed by module name) gives it a place."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from pod_compare_amd import apply_net
from pod_compare_amd import calibration_gpu as cg
from pod_compare_amd import compute_average_precision as cap
from pod_compare_amd import compute_calibration_errors as ce
from pod_compare_amd import compute_probabilistic_metrics as pm
from tests.helpers import GOLDEN

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def load_partitions():
    z = np.load(os.path.join(GOLDEN, "calib_errors.npz"))
    matched = {}
    for key in z.files:
        if "." in key:
            part, name = key.split(".", 1)
            matched.setdefault(part, {})[name] = torch.from_numpy(z[key])
    return z, matched


def test_fixture_parity():
    z, matched = load_partitions()
    k = int(z["num_classes"])
    torch.manual_seed(0)
    res = ce.calibration_errors_gpu(matched, {i: i for i in range(k)}, marginal_fn=lambda p, l: 0.12345)
    got = [res["reg_expected_calibration_error"], res["reg_maximum_calibration_error"], res["cls_minimum_uncertainty_error"],
           res["reg_minimum_uncertainty_error"]]
    assert np.allclose(got, z["values"], rtol=1e-6, atol=0.0), (got, z["values"])
    probs, labels = res["cls_marginal_inputs"]
    assert np.array_equal(probs, z["cal_probs"]) and np.array_equal(labels, z["cal_labels"])
    assert ["%.4f" % v for v in [res["cls_marginal_calibration_error"]] + got] == [str(s) for s in z["row"]]
    assert list(res) == list(ce.calibration_errors(matched, {i: i for i in range(k)}, marginal_fn=lambda p, l: 0.12345))


def seeded_partitions(n=200_000, seed=5):
    """~n detections over 7 classes (+ background column): class 5 has no true positive, class 6 no detection at all.  A quarter of the
    class scores are quantised to 1/64 (ties of the classification entropy); covariances are random SPD matrices of moderate condition
    (an fp32 Cholesky of an ill-conditioned matrix differs from LAPACK's by its conditioning, not by a few ulp)."""
    g = torch.Generator().manual_seed(seed)
    n_tp, n_dup = n // 2, n // 8
    n_fp = n - n_tp - n_dup

    def probs(m):
        p = torch.rand((m, 8), generator=g) ** 3
        p[:, 6] = 0.0
        p = p / p.sum(1, keepdim=True)
        q = torch.rand(m, generator=g) < 0.25
        p[q] = torch.round(p[q] * 64) / 64
        return p.float()

    def cov(m):
        L = torch.tril(torch.randn((m, 4, 4), generator=g)) * 0.2             # well conditioned, as a detector's box covariances are
        L[:, range(4), range(4)] = torch.rand((m, 4), generator=g) * 3 + 0.5
        return (L @ L.transpose(1, 2)).float()

    def part(m, classes):
        mu = torch.rand((m, 4), generator=g) * 500
        c = cov(m)
        sd = torch.sqrt(torch.diagonal(c, dim1=1, dim2=2))
        gtb = (mu + sd * torch.randn((m, 4), generator=g) * 1.3).float()
        cls = torch.as_tensor(classes)[torch.randint(len(classes), (m,), generator=g)]
        return {"predicted_box_means": mu.float(), "predicted_box_covariances": c, "predicted_cls_probs": probs(m), "gt_box_means": gtb,
                "gt_cat_idxs": (cls + 1).reshape(-1, 1)}

    tp = part(n_tp, [0, 1, 2, 3, 4])
    dup = part(n_dup, [0, 1, 2, 3, 4, 5])
    fp = part(n_fp, [0])
    del fp["gt_box_means"], fp["gt_cat_idxs"]
    return {"true_positives": tp, "duplicates": dup, "false_positives": fp}


def ulps(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return np.abs(a.astype(np.float64) - b.astype(np.float64)) / np.spacing(np.maximum(np.abs(a), np.abs(b)))


def same(a, b):
    if isinstance(a, str) or isinstance(b, str):
        return a == b
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))


def test_gpu_pass_against_the_host_on_a_seeded_set():
    matched = seeded_partitions()
    cmap = {i + 1: i for i in range(7)}
    torch.manual_seed(11)
    res, det = cg.calibration_pass(matched, cmap, marginal_fn=lambda p, l: 0.0)
    torch.manual_seed(11)
    res2, det2 = cg.calibration_pass(matched, cmap, marginal_fn=lambda p, l: 0.0)
    for k in ("reg_expected_calibration_error", "reg_maximum_calibration_error", "cls_minimum_uncertainty_error", "reg_minimum_uncertainty_error"):
        assert same(res[k], res2[k]), k                                                   # two runs bit-identical
    for k in det:
        assert same(det[k], det2[k]), k

    # the keys: within 4 ulp of torch's
    tp, dup, fp = matched["true_positives"], matched["duplicates"], matched["false_positives"]
    cls_g, reg_g, cls_of = cg.keys_gpu(matched, cmap)
    probs = torch.cat([p["predicted_cls_probs"] for p in (tp, dup, fp)])
    covs = torch.cat([p["predicted_box_covariances"] for p in (tp, dup, fp)])
    cls_h = -torch.log(probs[:, :-1].max(1).values)
    reg_h = torch.distributions.multivariate_normal.MultivariateNormal(torch.zeros(covs.shape[0:2]), covs + 1e-4 * torch.eye(4)).entropy()
    assert ulps(cls_g, cls_h).max() <= 4 and ulps(reg_g, reg_h).max() <= 4

    # minimum-uncertainty errors: bit-equal to the host formula on the GPU's own keys, the same draws; NaN where the host has NaN
    n_tp, n_m = tp["predicted_cls_probs"].shape[0], tp["predicted_cls_probs"].shape[0] + dup["predicted_cls_probs"].shape[0]
    is_tp_row = (torch.arange(cls_of.numel()) < n_tp).double()
    torch.manual_seed(11)
    for j, c in enumerate(cmap.values()):
        rows = cls_of == c
        want_cls = ce._min_uncertainty_error(cls_g[rows], is_tp_row[rows]).double()
        want_reg = ce._min_uncertainty_error(reg_g[rows], is_tp_row[rows]).double()
        assert same(det["cls_min_u"][j], want_cls.numpy()) and same(det["reg_min_u"][j], want_reg.numpy()), (c, det["cls_min_u"][j], want_cls)
    assert np.isnan(det["cls_min_u"][5]) and np.isnan(det["cls_min_u"][6]) and np.isfinite(det["cls_min_u"][:5]).all()

    # regression counts: equal to the host's up to the host cdf values within 2 ulp of the edge
    torch.manual_seed(11)
    host = ce.calibration_errors(matched, {i + 1: i for i in range(6)}, marginal_fn=lambda p, l: 0.0)    # (the host fails on class 6: empty)
    means = torch.cat((tp["predicted_box_means"], dup["predicted_box_means"]))
    var = torch.diagonal(torch.cat((tp["predicted_box_covariances"], dup["predicted_box_covariances"])), dim1=1, dim2=2)
    gt = torch.cat((tp["gt_box_means"], dup["gt_box_means"]))
    gcls = torch.cat((tp["gt_cat_idxs"], dup["gt_cat_idxs"])).reshape(-1) - 1
    edges = cg._edges()
    all_equal = True
    for j, c in enumerate(cmap.values()):
        sel = gcls == c
        equal_c = True
        for d in range(4):
            cdf = torch.distributions.Normal(means[sel, d], scale=torch.sqrt(var[sel, d])).cdf(gt[sel, d])
            assert det["totals"][j, d] == cdf.shape[0]
            for i, e in enumerate(edges):
                h = int((cdf < e).sum())
                near = int((ulps(cdf.numpy(), np.full(cdf.shape, float(e), np.float32)) <= 2).sum())
                assert abs(int(det["counts"][j, d, i]) - h) <= near, (c, d, i, det["counts"][j, d, i], h, near)
                equal_c &= int(det["counts"][j, d, i]) == h
        if equal_c:                                                                       # equal counts: the host's own per-class errors
            errs_host = []
            for d in range(4):
                cdf = torch.distributions.Normal(means[sel, d], scale=torch.sqrt(var[sel, d])).cdf(gt[sel, d])
                errs_host.append(torch.stack([((cdf < e).float().sum() / cdf.shape[0] - e) ** 2 for e in edges]))
            assert same(det["reg_ece"][j], torch.stack([x.mean() for x in errs_host]).numpy())
            assert same(det["reg_mce"][j], torch.stack([x.max() for x in errs_host]).numpy())
        all_equal &= equal_c
    if all_equal:
        assert res["reg_expected_calibration_error"] == host["reg_expected_calibration_error"]
        assert res["reg_maximum_calibration_error"] == host["reg_maximum_calibration_error"]
    assert np.array_equal(res["cls_marginal_inputs"][0], host["cls_marginal_inputs"][0])
    assert np.array_equal(res["cls_marginal_inputs"][1], host["cls_marginal_inputs"][1])


@pytest.mark.parametrize("kind", ["continuous", "discrete", "fixture"])
def test_marginal_error_on_the_gpu(kind):
    rng = np.random.default_rng(3)
    if kind == "continuous":
        p = rng.uniform(0.0, 1.0, 1_000_003).astype(np.float32) ** 2
        y = (rng.uniform(size=p.size) < np.clip(p * 1.3, 0, 1)).astype(np.int64)
    elif kind == "discrete":
        p = (np.round(rng.uniform(0.0, 1.0, 300_000) * 40) / 40).astype(np.float32)
        y = (rng.uniform(size=p.size) < 0.8 * p).astype(np.int64)
    else:
        z, _ = load_partitions()
        p, y = z["cal_probs"], z["cal_labels"]
    want = ce.marginal_calibration_error(p, y)
    got = cg.marginal_calibration_error_gpu(torch.from_numpy(p).cuda(), torch.from_numpy(y).cuda())
    assert want > 0 and abs(got - want) <= 1e-12 * abs(want), (got, want)
    assert got == cg.marginal_calibration_error_gpu(torch.from_numpy(p).cuda(), torch.from_numpy(y).cuda())
    if kind == "discrete":
        assert np.unique(p).size < p.size / 4


def eval_fixture(tmp_path, cats=None, to=None):
    z = np.load(os.path.join(GOLDEN, "eval_metrics.npz"))
    predicted, gt = json.loads(str(z["predicted_json"])), json.loads(str(z["gt_json"]))
    if cats is not None:
        predicted = [dict(d, category_id=to[d["category_id"]]) for d in predicted if d["category_id"] in cats]
        gt = [dict(a, category_id=to[a["category_id"]]) for a in gt if a["category_id"] in cats]
    ids = sorted({a["image_id"] for a in gt} | {d["image_id"] for d in predicted})
    return predicted, {"images": [{"id": i} for i in ids], "annotations": gt}


def write(tmp_path, name, obj):
    p = tmp_path / name
    p.parent.mkdir(parents=True, exist_ok=True)
    p.write_text(json.dumps(obj))
    return str(p)


def test_kitti_mapping(tmp_path):
    """The same detections and ground truth (cars and persons), written with BDD ids and with KITTI ids: PM / CE with --test-dataset kitti_val
    on the KITTI files equal PM / CE on the BDD files (CE over classes 0 and 3); read through the BDD map, the KITTI files score differently."""
    pb, gb = eval_fixture(tmp_path, {1, 4}, {1: 1, 4: 4})
    pk, gk = eval_fixture(tmp_path, {1, 4}, {1: 1, 4: 2})
    files = {k: write(tmp_path, k + ".json", v) for k, v in (("pb", pb), ("gb", gb), ("pk", pk), ("gk", gk))}
    pm_b = pm.main(["--results", files["pb"], "--gt", files["gb"]])
    pm_k = pm.main(["--results", files["pk"], "--gt", files["gk"], "--test-dataset", "kitti_val"])
    assert pm_b["counts"] == pm_k["counts"] and json.dumps(pm_b["average"]) == json.dumps(pm_k["average"])
    pm_wrong = pm.main(["--results", files["pk"], "--gt", files["gk"]])
    assert json.dumps(pm_wrong["average"]) != json.dumps(pm_b["average"])
    torch.manual_seed(4)
    ce_k = ce.main(["--results", files["pk"], "--gt", files["gk"], "--test-dataset", "kitti_val"])
    torch.manual_seed(4)
    ce_b = ce.calibration_errors_of_results(pb, gb["annotations"], {1: 0, 4: 3}, 0.0)
    for k in ce_b:
        if k == "cls_marginal_inputs":
            assert all(np.array_equal(a, b) for a, b in zip(ce_b[k], ce_k[k]))
        else:
            assert same(ce_b[k], ce_k[k]), k


def test_chain_equivalence(tmp_path):
    """apply_net --eval-only = AP --output mAP_res.txt, then PM --map-results, then CE --map-results, with the same seed."""
    predicted, gt = eval_fixture(tmp_path)
    gt_file = write(tmp_path, "gt.json", gt)
    ra, rb = write(tmp_path, "a/r.json", predicted), write(tmp_path, "b/r.json", predicted)
    chain = apply_net.main(["--eval-only", "--coco-json", gt_file, "--output", ra, "--random-seed", "0"])
    mres = str(tmp_path / "b" / "mAP_res.txt")
    ap = cap.main(["--results", rb, "--gt", gt_file, "--output", mres])
    p = pm.main(["--results", rb, "--gt", gt_file, "--map-results", mres])
    torch.manual_seed(0)
    c = ce.main(["--results", rb, "--gt", gt_file, "--map-results", mres])
    assert np.array_equal(chain["ap"]["stats"], ap["stats"])
    assert chain["ap"]["optimal_score_threshold"] == ap["optimal_score_threshold"]
    assert chain["min_allowed_score"] == cap.read_min_allowed_score(mres)
    assert json.dumps(chain["pm"]) == json.dumps(p)
    for k in c:
        if k == "cls_marginal_inputs":
            assert all(np.array_equal(a, b) for a, b in zip(chain["ce"][k], c[k]))
        else:
            assert same(chain["ce"][k], c[k]), k
    assert open(str(tmp_path / "a" / "mAP_res.txt"), "rb").read() == open(mres, "rb").read()


def test_apply_net_eval_end_to_end(tmp_path):
    from PIL import Image
    rng = np.random.default_rng(2)
    images, anns = [], []
    for k, (h, w) in enumerate(((180, 320), (200, 300), (180, 320))):
        Image.fromarray(rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)).save(tmp_path / ("f%d.png" % k))
        images.append({"id": 500 + k, "file_name": "f%d.png" % k, "height": h, "width": w})
        for j in range(2):
            x, y = float(rng.uniform(0, w / 2)), float(rng.uniform(0, h / 2))
            anns.append({"id": len(anns) + 1, "image_id": 500 + k, "category_id": int(rng.choice([1, 4])), "bbox": [x, y, 40.0, 30.0],
                         "area": 1200.0, "iscrowd": 0})
    (tmp_path / "set.json").write_text(json.dumps({"images": images, "annotations": anns}))
    out = str(tmp_path / "r.json")
    cmd = [sys.executable, "-m", "pod_compare_amd.apply_net", "--coco-json", str(tmp_path / "set.json"), "--image-root", str(tmp_path),
           "--random-init", "--output", out, "--eval"]
    r = subprocess.run(cmd, cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT), timeout=900, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert os.path.exists(str(tmp_path / "mAP_res.txt"))
    thr = cap.read_min_allowed_score(str(tmp_path / "mAP_res.txt"))
    dets = json.load(open(out))
    n_above = sum(1 for d in dets if d["score"] >= thr)
    count = lambda name: int(re.search(r"\| *" + name + r": *\| *(\d+) *\|", r.stdout).group(1))
    tp, fp, fn = count("True Positives"), count("False Positives"), count("False Negatives")
    assert tp + fp <= n_above and tp + fn <= len(anns)
    if n_above == 0:
        assert fn == len(anns) and tp == fp == 0
    assert "Cls Marginal Calibration Error" in r.stdout and "Average Precision" in r.stdout
