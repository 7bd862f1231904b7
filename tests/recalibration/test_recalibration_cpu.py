"""Recalibration without a GPU: the host restatement's own properties on the seeded fixture, the settings file, the fold selection, the
header / binding agreement of K36's symbols with their argument checks, and the parsers."""
import ctypes
import json
import math
import os

import numpy as np
import pytest

from pod_compare_amd import apply_net, hip
from pod_compare_amd import recalibrate as cli
from pod_compare_amd import recalibration as rc
from tests.recalibration import recal_fixture as fxt
from tests.recalibration import recal_ref as ref
from tests.test_abi_cpu import declared_symbols

SIZES = ((257, 64), (300, 100))
NEW_SYMBOLS = ("pod_recal_workspace_bytes", "pod_recal_cls_sums", "pod_recal_reg_z", "pod_recal_moment", "pod_recal_ece_grid", "pod_recal_apply")


@pytest.fixture(scope="module", params=SIZES, ids=lambda s: "%d_%d" % s)
def fitted(request):
    fx = ref.fixture(*request.param)
    p, y = fx["p"].reshape(-1), fx["labels"].reshape(-1)
    beta, its = ref.fit_temperature(p, y)
    z = fx["resid"] / fx["sigma"]
    return fx, p, y, beta, its, z


def test_newton_reaches_a_fixed_point(fitted):
    fx, p, y, beta, its, _ = fitted
    # the labels are drawn at half the logit: beta estimates 0.5 with a standard error of about 1 / sqrt(sum s (1 - s) x^2) < 0.02
    assert 0.44 <= beta <= 0.56 and its <= 8
    L, g, h = (np.asarray(t) for t in ref.cls_terms(p, y, beta))
    assert abs(math.fsum(g)) <= 2.0 ** -40 * abs(beta) * math.fsum(h) + 64 * 2.0 ** -53 * math.fsum(np.abs(g))
    assert ref.cls_sums(p, y, beta)[0] < ref.cls_sums(p, y, 1.0)[0]
    # the stated order is a sum: it agrees with the exactly rounded one to a few ulp of the terms' magnitude
    assert abs(ref.chunk_sum(L) - math.fsum(L)) <= 2.0 ** -40 * math.fsum(np.abs(L))


def test_chunk_sum_is_the_stated_order():
    rng = np.random.default_rng(1)
    v = rng.standard_normal(2 * 256 + 1) * 10.0 ** rng.integers(-8, 8, size=513)
    partials = []
    for c in range(3):
        a = 0.0
        for t in v[256 * c:256 * (c + 1)].tolist():
            a += t
        partials.append(a)
    assert ref.chunk_sum(v) == (0.0 + partials[0] + partials[1]) + partials[2]
    assert ref.chunk_sum([]) == 0.0 and ref.chunk_sum([3.5]) == 3.5


def test_moment_is_the_root_mean_square(fitted):
    _, _, _, _, _, z = fitted
    zg, seg_off = ref.group(z, np.tile(np.arange(4, dtype=np.int32), (z.shape[0], 1)), 4)
    counts, sums = ref.moment(zg, seg_off)
    scales = ref.moment_scales(counts, sums)
    assert counts.tolist() == [z.shape[0]] * 4
    for d in range(4):
        assert np.array_equal(zg[seg_off[d]:seg_off[d + 1]], z[:, d])            # grouped by coordinate, row order kept
        assert math.isclose(scales[d], math.sqrt(np.mean(z[:, d] ** 2)), rel_tol=1e-13)
    # true scales 2 and 1 / 1.5; the standard error of a root mean square of m normals is s / sqrt(2 m) <= 0.09 and 0.03: four of them
    assert all(abs(scales[d] - 2.0) <= 0.36 for d in (0, 2)) and all(abs(scales[d] - 1 / 1.5) <= 0.12 for d in (1, 3))


def test_grid_fit_is_never_worse_than_the_moment_fit(fitted):
    _, _, _, _, _, z = fitted
    grid = np.array(ref.grid_scales())
    assert grid[ref.GRID_ONE] == 1.0 and grid[0] == 1 / 16 and grid[-1] == 16.0 and len(grid) == 1025
    for d in range(4):
        obj = ref.ece_objectives(z[:, d])
        j = ref.argmin_tie(obj)
        s_moment = math.sqrt(np.mean(z[:, d] ** 2))
        at_moment = ref.ece_objectives(z[:, d], [s_moment])[0]
        assert obj[j] <= obj[ref.GRID_ONE] and obj[j] <= at_moment * (1 + 1e-12) + 1e-4       # the grid is 0.54 % fine: one count can move
        assert obj[ref.GRID_ONE] / obj[j] >= 3.0       # a factor 2 or 1.5 in the spread against the counting noise of m >= 257 values


def test_argmin_tie_rule():
    assert ref.argmin_tie([3.0, 1.0, 2.0, 1.0, 3.0], j_one=2) == 1            # a symmetric tie: the smaller j
    assert ref.argmin_tie([1.0, 5.0, 2.0, 1.0, 3.0], j_one=2) == 3            # the smaller |j - j_one| before the smaller j
    assert ref.argmin_tie([1.0, 1.0, 1.0, 1.0, 1.0], j_one=2) == 2
    # a symmetric grid around scale 1 gives bit-equal objectives at j and 2 j_one - j: the tie the kernel test replays
    z = ref.fixture(257, 64)["resid"][:, 0] / ref.fixture(257, 64)["sigma"][:, 0]
    obj = ref.ece_objectives(z, [2.5, 2.0, 1.0, 2.0, 2.5])
    assert obj[1] == obj[3] < obj[2] and ref.argmin_tie(obj, 2) == 1


def test_apply_identity_and_order():
    fx = ref.fixture(300, 100)
    rng = np.random.default_rng(5)
    rec = rng.uniform(0.0, 1.0, size=(3, 9, 29)).astype(np.float32)
    rec[:, :, 6:13] = fx["p"][:27].reshape(3, 9, 7)
    counts = np.array([9, 0, 4], dtype=np.int32)
    same = ref.apply_records(rec, counts, 7, 1.0, [[1.0] * 4])
    live = np.arange(9)[None, :] < counts[:, None]
    assert np.array_equal(same[live].view(np.uint32), rec[live].view(np.uint32)) and not same[~live].any()
    out = ref.apply_records(rec, counts, 7, 0.5, [[2.0, 0.5, 2.0, 0.5]])
    assert np.array_equal(out[live][:, :4], rec[live][:, :4]) and np.array_equal(out[live][:, 5], rec[live][:, 5])
    # C = T Sigma T^T with Sigma -> D Sigma D: the xyxy variances scale by s^2
    tinv = np.array([[1.0, 0, 0, 0], [0, 1.0, 0, 0], [1.0, 0, 1.0, 0], [0, 1.0, 0, 1.0]])
    sig0 = tinv @ rec[0, 0, 13:].astype(np.float64).reshape(4, 4) @ tinv.T
    sig1 = tinv @ out[0, 0, 13:].astype(np.float64).reshape(4, 4) @ tinv.T
    d = np.diag([2.0, 0.5, 2.0, 0.5])
    assert np.allclose(sig1, d @ sig0 @ d, rtol=1e-6, atol=1e-6)


def test_settings_file_round_trip(tmp_path):
    r = rc.Recalibration(beta=0.4971, scales=[[1.9, 0.66, 2.01, 0.7]], cls_method="temperature", reg_method="ece", n_scores=2247, n_matched=257,
                         invalid=[0, 1, 0, 2], cls_objective_before=0.41, cls_objective_after=0.33, reg_objective_before=[0.01] * 4,
                         reg_objective_after=[0.001] * 4, newton_iterations=7, fold=[0, 2], min_allowed_score=0.25)
    path = str(tmp_path / "recal.json")
    r.save(path)
    assert rc.Recalibration.load(path) == r
    d = json.load(open(path))
    assert d["format"] == 1 and d["beta"] == 0.4971 and d["fold"] == [0, 2]
    d["format"] = 2
    json.dump(d, open(path, "w"))
    with pytest.raises(ValueError, match="format"):
        rc.Recalibration.load(path)
    assert rc.Recalibration().is_identity() and not r.is_identity()


def test_fold_and_complement_partition_the_images():
    ids = [907, 3, 3, 41, 12, 500, 77, 8]
    for n in (1, 2, 3):
        folds = [rc.fold_image_ids(ids, k, n) for k in range(n)]
        assert set().union(*folds) == set(ids) and sum(len(f) for f in folds) == len(set(ids))
        for k in range(n):
            assert rc.fold_image_ids(ids, k, n, complement=True) == set(ids) - folds[k]
    assert rc.fold_image_ids(ids, 0, 2) == {3, 12, 77, 907} and rc.fold_image_ids(ids, 0, 1) == set(ids)      # ranks 0, 2, 4, 6 of 3 8 12 41 77 500 907
    assert rc.parse_fold("1/3") == (1, 3)
    for bad in ("3/3", "-1/2", "a/b", "1", "0/0"):
        with pytest.raises(ValueError):
            rc.parse_fold(bad)


def test_header_and_binding_carry_the_new_symbols():
    assert hip.POD_ABI_VERSION == 18
    declared = declared_symbols()
    for name in NEW_SYMBOLS:
        assert name in declared and name in hip.EXPORTS
    assert "pod_recal_workspace_bytes" in hip._SIZE_QUERIES
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))), "include", "pod_mi355x.h")).read()
    for token, value in (("POD_RECAL_CHUNK", hip.POD_RECAL_CHUNK), ("POD_RECAL_MAX_SEGMENTS", hip.POD_RECAL_MAX_SEGMENTS),
                         ("POD_RECAL_MAX_GRID", hip.POD_RECAL_MAX_GRID), ("POD_RECAL_MAX_QUANTILES", hip.POD_RECAL_MAX_QUANTILES)):
        assert "#define %s" % token in text and str(value) in text.split("#define %s" % token)[1].split("\n")[0]
    assert "k36_recalibrate.hip" in __import__("pod_compare_amd.build", fromlist=["SOURCES"]).SOURCES


def test_entry_points_refuse_bad_sizes_without_a_gpu():
    lib = hip.load()
    buf = ctypes.create_string_buffer(256)
    X = (ctypes.addressof(buf) + 63) & ~63                 # an aligned non-null pointer: never dereferenced on these paths
    assert lib.pod_recal_workspace_bytes(-1, 0) == 0 and lib.pod_recal_workspace_bytes(1 << 31, 0) == 0
    assert lib.pod_recal_workspace_bytes(8, hip.POD_RECAL_MAX_SEGMENTS + 1) == 0
    assert lib.pod_recal_workspace_bytes(1028, 4) >= 2 * 8 * 1028 + 2 * 4 * 1028 + 8 * (3 * 5 + 4)
    sums = lambda **kw: lib.pod_recal_cls_sums(*[kw.get(k, v) for k, v in (("p", X), ("y", X), ("n", 8), ("beta", 1.0), ("x", X), ("ready", 0), ("ws", X), ("out", X), ("st", None))])
    for kw in ({"n": -1}, {"n": 1 << 31}, {"out": None}, {"y": None}, {"ws": None}, {"p": None}, {"beta": float("nan")}, {"x": None, "ready": 1}, {"x": X + 4}):
        assert sums(**kw) == -1, kw
    regz = lambda **kw: lib.pod_recal_reg_z(*[kw.get(k, v) for k, v in (("m", X), ("c", X), ("g", X), ("cls", X), ("n", 8), ("k", 0), ("ws", X), ("z", X), ("seg", X), ("inv", X), ("st", None))])
    for kw in ({"n": -1}, {"n": (1 << 29)}, {"k": -1}, {"k": hip.POD_MAX_CLASSES + 1}, {"inv": None}, {"m": None}, {"c": None}, {"g": None}, {"z": None}, {"seg": None},
               {"ws": None}, {"k": 3, "cls": None}, {"z": X + 4}):
        assert regz(**kw) == -1, kw
    mom = lambda **kw: lib.pod_recal_moment(*[kw.get(k, v) for k, v in (("z", X), ("seg", X), ("n", 8), ("ns", 4), ("ws", X), ("zg", X), ("off", X), ("cnt", X), ("sum", X), ("st", None))])
    for kw in ({"n": -1}, {"n": 1 << 31}, {"ns": 0}, {"ns": hip.POD_RECAL_MAX_SEGMENTS + 1}, {"z": None}, {"seg": None}, {"ws": None}, {"zg": None}, {"off": None},
               {"cnt": None}, {"sum": None}, {"zg": X + 4}):
        assert mom(**kw) == -1, kw
    ece = lambda **kw: lib.pod_recal_ece_grid(*[kw.get(k, v) for k, v in (("zg", X), ("off", X), ("n", 8), ("ns", 4), ("mx", 8), ("sc", X), ("ng", 5), ("j1", 2), ("q", X), ("nq", 14),
                                                                            ("ws", X), ("obj", X), ("bj", X), ("bo", X), ("oo", X), ("st", None))])
    for kw in ({"n": -1}, {"ns": 0}, {"mx": -1}, {"mx": 9}, {"ng": 0}, {"ng": hip.POD_RECAL_MAX_GRID + 1}, {"j1": -1}, {"j1": 5}, {"nq": 0}, {"nq": hip.POD_RECAL_MAX_QUANTILES + 1},
               {"zg": None}, {"off": None}, {"sc": None}, {"q": None}, {"ws": None}, {"obj": None}, {"bj": None}, {"bo": None}, {"oo": None}, {"obj": X + 4}):
        assert ece(**kw) == -1, kw
    app = lambda **kw: lib.pod_recal_apply(*[kw.get(k, v) for k, v in (("rec", X), ("cnt", X), ("ni", 2), ("md", 4), ("K", 7), ("beta", 0.5), ("sc", X), ("rows", 1), ("out", X + 128), ("st", None))])
    for kw in ({"ni": -1}, {"md": 0}, {"K": 0}, {"K": hip.POD_MAX_CLASSES + 1}, {"beta": 0.0}, {"beta": -1.0}, {"beta": float("nan")}, {"beta": float("inf")}, {"rows": 0},
               {"rows": hip.POD_MAX_CLASSES + 1}, {"sc": None}, {"rec": None}, {"cnt": None}, {"out": None}, {"out": X}, {"ni": 1 << 30, "md": 4}, {"sc": X + 4}):
        assert app(**kw) == -1, kw
    assert app(ni=0) == 0                                   # an empty table: accepted, nothing launched


def test_per_class_temperature_is_refused_with_the_reason():
    with pytest.raises(ValueError, match="arg-max"):
        rc.fit_recalibration({}, {1: 0}, cls="per_class")
    with pytest.raises(ValueError):
        rc.fit_recalibration({}, {1: 0}, reg="isotonic")


def test_apply_net_refuses_a_file_count_that_does_not_match_the_configs(tmp_path):
    here = os.path.dirname(os.path.abspath(apply_net.__file__))
    a, b = (os.path.join(here, "configs", "Inference", n) for n in ("standard_nms.yaml", "bayes_od.yaml"))
    gt = tmp_path / "gt.json"
    gt.write_text(json.dumps({"images": [], "annotations": []}))
    common = ["--eval-only", "--coco-json", str(gt)]
    with pytest.raises(SystemExit, match="--recalibration takes one file per --inference-config.*1 file.*2 config"):
        apply_net.main(common + ["--inference-config", a, b, "--recalibration", "r.json"])
    with pytest.raises(SystemExit, match="--recalibration takes one file per --inference-config.*3 file.*2 config"):
        apply_net.main(common + ["--inference-config", a, b, "--recalibration", "r.json", "s.json", "t.json"])
    with pytest.raises(SystemExit, match="--recalibration takes one file per --inference-config.*2 file.*1 config"):
        apply_net.main(common + ["--inference-config", a, "--recalibration", "r.json", "s.json"])
    with pytest.raises(SystemExit, match="needs --eval"):
        apply_net.main(["--coco-json", str(gt), "--recalibration", "r.json"])


def test_command_line_parsers():
    ap = cli.build_parser()
    f = ap.parse_args(["fit", "--results", "r", "--gt", "g", "--output", "o"])
    assert (f.fold, f.cls, f.reg, f.per_class_reg, f.binary_results, f.iou_min, f.iou_correct) == ("0/2", "temperature", "moment", False, False, 0.1, 0.7)
    a = ap.parse_args(["apply", "--results", "r", "--recalibration", "c", "--output", "o"])
    assert a.complement is None and not a.binary_output and a.gt_output == ""
    assert ap.parse_args(["apply", "--results", "r", "--recalibration", "c", "--output", "o", "--complement"]).complement is True


def test_result_dicts_keep_keys_order_and_ids_through_the_host_apply():
    predicted, gt, links = fxt.detection_set(60, 20, n_images=8)
    out = fxt.host_apply(predicted, 0.5, [[2.0, 0.5, 2.0, 0.5]])
    assert len(out) == len(predicted)
    for a, b in zip(predicted, out):
        assert list(a) == list(b) and a["image_id"] == b["image_id"] and a["category_id"] == b["category_id"] and a["bbox"] == b["bbox"]
        assert int(np.argmax(a["cls_prob"])) == int(np.argmax(b["cls_prob"])) and b["score"] != a["score"]
    rec, counts, k, place = rc.pack_results(predicted)
    assert k == 7 and int(counts.sum()) == len(predicted) and rec.shape == (8, int(counts.max()), 29) and len(set(place)) == len(place)
    assert sum(1 for l in links if l >= 0) == 60 and len(gt["annotations"]) == 60


def test_the_restatement_alone_improves_the_held_out_calibration():
    """The host-only chain the end-to-end bar rests on (profiles/recalibration.md records these figures): fit on fold 0/2, apply to the
    complement, measure with the package's host calibration_errors."""
    ece, mce, beta, scales = fxt.host_ratios("moment")
    print("reg ECE %.6f -> %.6f, cls MCE %.6f -> %.6f, beta %.4f, scales %s" % (ece + mce + (beta, scales)))
    assert ece[1] < ece[0] / 2 and mce[1] < mce[0] and 0.4 < beta < 0.7
