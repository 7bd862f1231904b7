"""The comparison pass without a GPU: the grouping of configs into families and sub-families as a pure function, the refusals of
build_comparison and apply_net, the table's formatting from canned evaluator dictionaries, and the new symbol and structure of the C ABI."""
import ctypes
import os
import subprocess
import sys

import pytest

from pod_compare_amd import apply_net, build, comparison, config, hip
from pod_compare_amd.probabilistic_inference import build_comparison

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
CONFIGS = os.path.join(ROOT, "pod_compare_amd", "configs")
MODEL = os.path.join(CONFIGS, "BDD-Detection", "retinanet", "retinanet_R_50_FPN_1x_reg_cls_var_dropout.yaml")
# the eight inference YAMLs the reference ships, and BayesOD's other box merge as a ninth config
YAMLS = ("standard_nms", "anchor_statistics", "bayes_od", "bayes_od_mc_dropout", "mc_dropout_ensembles_pre_nms", "mc_dropout_ensembles_post_nms",
         "ensembles_pre_nms", "ensembles_post_nms")


def inference(name):
    return os.path.join(CONFIGS, "Inference", name + ".yaml")


def nine():
    cfgs = [config.setup_config(MODEL, inference(n)) for n in YAMLS]
    cfgs.append(config.setup_config(MODEL, inference("bayes_od"), opts=["PROBABILISTIC_INFERENCE.BAYES_OD.BOX_MERGE_MODE", "covariance_intersection"]))
    return cfgs


def test_family_grouping_of_the_nine_configs():
    """Written by hand from the YAMLs.  Single-run: standard_nms (which reads no affinity threshold: its 0.7 default does not split it off),
    anchor_statistics and both BayesOD merges -- one evaluation without dropout, one front.  MC dropout, 10 runs, last run's unread outputs
    skipped: BayesOD and the pre-NMS merge, one front.  MC dropout, all 10 runs: the post-NMS merge, alone -- its evaluation draws other
    masks.  Ensembles: the two merges share the members' forwards, not the candidate list."""
    F, S = comparison.Family, comparison.SubFamily
    seeds = (0, 1000, 2000, 3000, 4000)
    assert comparison.group_families(nine()) == [
        F(("model", False, 1, False), (0, 1, 2, 8), (S("merged", 0.9, (0, 1, 2, 8)),)),
        F(("model", True, 10, True), (3, 4), (S("merged", 0.9, (3, 4)),)),
        F(("model", True, 10, False), (5,), (S("post_nms", 0.9, (5,)),)),
        F(("ensembles", seeds), (6, 7), (S("merged", None, (6,)), S("post_nms", 0.9, (7,))))]


def test_grouping_follows_config_order_and_the_values_that_matter():
    pi = lambda **kw: config.setup_config(MODEL, opts=[x for k, v in kw.items() for x in ("PROBABILISTIC_INFERENCE." + k, v)])
    cfgs = [pi(INFERENCE_MODE="bayes_od", **{"MC_DROPOUT.ENABLE": "true", "MC_DROPOUT.NUM_RUNS": "5"}),
            pi(INFERENCE_MODE="standard_nms", **{"MC_DROPOUT.NUM_RUNS": "5"}),                                      # NUM_RUNS without ENABLE: one run
            pi(INFERENCE_MODE="anchor_statistics", AFFINITY_THRESHOLD="0.5"),
            pi(INFERENCE_MODE="bayes_od", AFFINITY_THRESHOLD="0.8"),                                                   # another affinity: its own front
            pi(INFERENCE_MODE="standard_nms", **{"MC_DROPOUT.ENABLE": "true", "MC_DROPOUT.NUM_RUNS": "1"}),           # one run WITH dropout
            pi(INFERENCE_MODE="mc_dropout_ensembles", **{"MC_DROPOUT.ENABLE": "true", "MC_DROPOUT.NUM_RUNS": "7"})]   # other run count
    got = comparison.group_families(cfgs)
    assert [f.key for f in got] == [("model", True, 5, True), ("model", False, 1, False), ("model", True, 1, False), ("model", True, 7, True)]
    assert [f.members for f in got] == [(0,), (1, 2, 3), (4,), (5,)]
    assert got[1].subfamilies == (comparison.SubFamily("merged", 0.5, (1, 2)), comparison.SubFamily("merged", 0.8, (3,)))


def test_a_front_is_served_by_a_workspace_with_the_threshold_its_tails_read():
    """standard_nms carries the default AFFINITY_THRESHOLD 0.7 and reads none; the anchor-statistics and BayesOD tails that share its front
    read 0.9: the sub-family's PodConfig comes from one of them, whatever the config order."""
    cfgs = [config.setup_config(MODEL, inference(n)) for n in ("standard_nms", "anchor_statistics", "bayes_od")]
    cmp = build_comparison(cfgs, model=object())
    (fam,) = cmp.families
    (sub,) = fam.subfamilies
    assert sub.affinity == 0.9 and cmp._leader(sub) is cmp.predictors[1]
    assert cmp._tails(sub) == [("standard_nms", "bayesian_inference", "bayesian_inference"), ("anchor_statistics", "bayesian_inference", "bayesian_inference"),
                               ("bayes_od", "bayesian_inference", "max_score")]
    alone = build_comparison(cfgs[:1], model=object())
    assert alone._leader(alone.families[0].subfamilies[0]) is alone.predictors[0]


def test_the_graph_cache_holds_every_family_as_long_as_its_own_run_would():
    """A model keeps `max_graphs` captured forwards, sized for one evaluation call per (stream, frame shape).  Every family of the model
    is a call with a graph key of its own, so a comparison scales the cache by its families of that model -- once, however many
    comparisons are built on the model."""
    from pod_compare_amd import modeling
    import torch
    torch.manual_seed(0)
    m = modeling.ProbabilisticRetinaNet(dropout_rate=0.1, cls_var_loss="loss_attenuation", bbox_cov_loss="negative_log_likelihood").eval()
    per_call = m.max_graphs
    cfgs = nine()
    assert len([f for f in comparison.group_families(cfgs) if f.key[0] == "model"]) == 3
    members = [object()] * 5
    build_comparison(cfgs, model=m, model_list=members)
    assert m.max_graphs == 3 * per_call
    build_comparison(cfgs[:5], model=m, model_list=members)
    assert m.max_graphs == 2 * per_call
    build_comparison(cfgs[:1], model=m)
    assert m.max_graphs == per_call
    m.max_graphs = 4                                          # a caller's own setting is the new per-call size
    build_comparison(cfgs[:5], model=m, model_list=members)
    assert m.max_graphs == 8


def test_configs_may_differ_in_the_inference_section_only():
    a, b = config.setup_config(MODEL, inference("bayes_od")), config.setup_config(MODEL, inference("standard_nms"))
    comparison.check_same_outside_inference([a, b])
    b.MODEL.RETINANET.SCORE_THRESH_TEST = 0.3
    with pytest.raises(ValueError, match=r"MODEL\.RETINANET\.SCORE_THRESH_TEST"):
        comparison.check_same_outside_inference([a, b])
    with pytest.raises(ValueError, match=r"MODEL\.RETINANET\.SCORE_THRESH_TEST"):     # before any model is built
        build_comparison([a, b])
    c = config.setup_config(MODEL, inference("standard_nms"), random_seed=4)
    with pytest.raises(ValueError, match="SEED"):
        comparison.check_same_outside_inference([a, c])
    d = config.setup_config(MODEL, inference("ensembles_pre_nms"))
    e = config.setup_config(MODEL, inference("ensembles_post_nms"), opts=["PROBABILISTIC_INFERENCE.ENSEMBLES.RANDOM_SEED_NUMS", "[0, 1]"])
    with pytest.raises(ValueError, match="RANDOM_SEED_NUMS"):
        build_comparison([d, e])
    with pytest.raises(ValueError, match="at least one"):
        build_comparison([])


def test_apply_net_refuses_one_run_arguments_by_name(tmp_path):
    two = ["--inference-config", inference("standard_nms"), inference("bayes_od")]
    for flags, word in ((["--output", str(tmp_path / "r.json")], "--output"), (["--vis-dir", str(tmp_path)], "--vis-dir"),
                        (["--ensemble-per-gpu"], "--ensemble-per-gpu"), (["--binary-output", str(tmp_path / "r.podr")], "--binary-output")):
        with pytest.raises(SystemExit) as e:
            apply_net.main(two + flags)
        assert word in str(e.value), flags
    with pytest.raises(SystemExit) as e:
        apply_net.main(["--inference-config", inference("bayes_od"), str(tmp_path / "bayes_od.yaml")])
    assert "bayes_od" in str(e.value)
    with pytest.raises(SystemExit) as e:
        apply_net.main(two + ["--eval"])
    assert "ground truth" in str(e.value)


def test_help_states_the_dense_rule():
    r = subprocess.run([sys.executable, "-m", "pod_compare_amd.apply_net", "--help"], cwd=ROOT, capture_output=True, text=True, timeout=120)
    text = " ".join(r.stdout.split())
    assert r.returncode == 0 and "--dense-bbox" in text and "not the candidate list" in text


def canned(k):
    reg = lambda v: {"ignorance_score_mean": v, "mean_squared_error": 1.0}
    return {"ap": {"stats": [0.1 * k + 0.01234, 0.5, 0.25] + [0.0] * 9, "optimal_score_threshold": 0.3},
            "pm": {"average": {"true_positives_cls_analysis": {"ignorance_score_mean": 0.5 + k}, "true_positives_reg_analysis": reg(12.25),
                               "false_positives_cls_analysis": {"ignorance_score_mean": None if k else 2.0},
                               "false_positives_reg_analysis": {"total_entropy_mean": 9.87654}}, "counts": {}},
            "ce": {"cls_marginal_calibration_error": 0.0123, "reg_expected_calibration_error": 0.04, "reg_maximum_calibration_error": 0.2,
                   "cls_minimum_uncertainty_error": 0.11111, "reg_minimum_uncertainty_error": 0.3}}


def test_comparison_table_from_canned_evaluator_dictionaries():
    table = apply_net.format_comparison_table(["standard_nms", "bayes_od_mc_dropout"], [canned(0), canned(1)])
    lines = table.split("\n")
    assert len(lines) == 6 and len({len(l) for l in lines}) == 1 and lines[0] == lines[2] == lines[5] and set(lines[0]) == {"+", "-"}
    cells = [[c.strip() for c in l.strip("|").split("|")] for l in (lines[1], lines[3], lines[4])]
    assert cells[0] == ["Inference Config", "AP", "AP50", "AP75", "TP Cls NLL", "TP Reg NLL", "FP Cls NLL", "FP Reg Entropy", "Cls MCE", "Reg ECE",
                        "Reg MaxCE", "Cls MUE", "Reg MUE"]
    assert cells[1] == ["standard_nms", "0.012", "0.500", "0.250", "0.5000", "12.2500", "2.0000", "9.8765", "0.0123", "0.0400", "0.2000", "0.1111", "0.3000"]
    assert cells[2] == ["bayes_od_mc_dropout", "0.112", "0.500", "0.250", "1.5000", "12.2500", "-", "9.8765", "0.0123", "0.0400", "0.2000", "0.1111", "0.3000"]


def test_eval_only_builds_the_table_from_the_result_files_without_a_model(tmp_path, monkeypatch):
    from pod_compare_amd import probabilistic_inference
    import json
    monkeypatch.setattr(probabilistic_inference, "build_comparison", lambda *a, **k: pytest.fail("--eval-only built a model"))
    monkeypatch.setattr(probabilistic_inference, "build_model", lambda *a, **k: pytest.fail("--eval-only built a model"))
    calls = []
    monkeypatch.setattr(apply_net, "evaluate_results", lambda *a, **k: calls.append((a, k)) or canned(len(calls) - 1))
    monkeypatch.chdir(tmp_path)
    gt = tmp_path / "gt.json"
    gt.write_text(json.dumps({"images": [], "annotations": []}))
    for n in ("standard_nms", "bayes_od"):
        os.makedirs(tmp_path / "output" / "inference" / "kitti_val" / n)
    res = apply_net.main(["--eval-only", "--coco-json", str(gt), "--test-dataset", "kitti_val", "--inference-config", inference("standard_nms"),
                          inference("bayes_od"), "--min-allowed-score", "0.25"])
    assert res == [canned(0), canned(1)]
    assert [a[:4] for a, _ in calls] == [(os.path.join("./output", "inference", "kitti_val", n, "coco_instances_results.json"), str(gt), "bdd_train",
                                          "kitti_val") for n in ("standard_nms", "bayes_od")]
    assert all(k["binary"] is False and k["min_allowed_score"] == 0.25 for _, k in calls)
    table = (tmp_path / "output" / "inference" / "kitti_val" / "standard_nms" / "comparison.txt").read_text()
    assert table == apply_net.format_comparison_table(["standard_nms", "bayes_od"], [canned(0), canned(1)]) + "\n"


# ---- the C ABI: tests/test_abi_cpu.py's pattern for the new symbol, structure and constants -------------------------------------------
@pytest.fixture(scope="module")
def lib_path():
    return build.build_library()


def test_new_symbol_is_declared_bound_and_exported(lib_path):
    header = open(os.path.join(ROOT, "include", "pod_mi355x.h")).read()
    assert "int pod_run_image_modes(" in header and "pod_run_image_modes" in hip.EXPORTS
    lib = ctypes.CDLL(lib_path)
    assert hasattr(lib, "pod_run_image_modes")
    assert lib.pod_abi_version() == hip.POD_ABI_VERSION == 18          # additions only: the number stands


def test_mode_tail_layout_and_constants_match_c(lib_path, tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "pod_mi355x.h"\n'
                   'int main(void){printf("%zu %zu %zu %zu %d %d %d %d %d %d\\n", sizeof(PodModeTail), offsetof(PodModeTail, cls_merge_mode),'
                   ' offsetof(PodModeTail, out), offsetof(PodModeTail, out.n_det), POD_MAX_MODE_TAILS, POD_PART_SELECT, POD_PART_FINISH,'
                   ' POD_PART_CANDIDATES, POD_PART_FRONT, POD_PART_TAIL); return 0;}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got == [ctypes.sizeof(hip.PodModeTail), hip.PodModeTail.cls_merge_mode.offset, hip.PodModeTail.out.offset,
                   hip.PodModeTail.out.offset + hip.PodDetections.n_det.offset, hip.POD_MAX_MODE_TAILS, hip.POD_PART_SELECT, hip.POD_PART_FINISH,
                   hip.POD_PART_CANDIDATES, hip.POD_PART_FRONT, hip.POD_PART_TAIL]


def test_modes_entry_rejects_invalid_arguments_without_a_gpu(lib_path):
    """Every refusal comes before the first launch, so it is safe without a GPU: the null pointers, the tail count, an unknown mode, a
    BayesOD tail without covariances or with a merge mode out of range, a tail without outputs -- and pod_run_image_part's new part values
    take what the old ones took."""
    lib = hip.load()
    buf = ctypes.create_string_buffer(64)
    X = ctypes.addressof(buf)                        # any non-null pointer: never dereferenced on these paths
    lv = (hip.PodLevel * hip.POD_MAX_LEVELS)()

    def cfg_with(**kw):
        c = hip.PodConfig()
        c.n_levels, c.n_runs, c.num_anchors, c.num_classes, c.cov_dims, c.prop_samples, c.topk = 5, 1, 9, 7, 0, 1000, 1000
        for k, v in kw.items():
            setattr(c, k, v)
        return c

    ws = hip.PodWorkspace()
    for name, _ in hip.PodWorkspace._fields_[:-2]:
        setattr(ws, name, X)
    ws.n_capacity = 5000

    def tails(n, **kw):
        arr = (hip.PodModeTail * max(n, 1))()
        for t in arr:
            t.out = hip.PodDetections(X, X, X, X, X, X, X)
        for k, v in kw.items():
            setattr(arr[max(n, 1) - 1], k, v)
        return arr

    call = lambda c, t, n, ws_=ws, lv_=lv: lib.pod_run_image_modes(c, lv_, ws_, t, n, 10, 10, 10, 10, None)
    ok = cfg_with()
    assert call(ok, tails(1), 0) == -1 and call(ok, tails(1), -3) == -1
    assert call(ok, tails(hip.POD_MAX_MODE_TAILS + 1), hip.POD_MAX_MODE_TAILS + 1) == -1
    assert call(ok, None, 1) == -1 and call(None, tails(1), 1) == -1 and call(ok, tails(1), 1, ws_=None) == -1 and call(ok, tails(1), 1, lv_=None) == -1
    assert call(ok, tails(3, mode=7), 3) == -1 and call(ok, tails(2, mode=-1), 2) == -1
    assert call(ok, tails(2, mode=hip.POD_MODE_BAYES_OD), 2) == -1                                   # no reg_var head, one run: no covariances
    for kw in ({"box_merge_mode": 2}, {"cls_merge_mode": -1}):
        assert call(cfg_with(cov_dims=4), tails(2, mode=hip.POD_MODE_BAYES_OD, **kw), 2) == -1, kw
    no_out = tails(2)
    no_out[1].out = hip.PodDetections(X, X, X, X, X, X, None)
    assert call(ok, no_out, 2) == -1
    assert lib.pod_run_image_modes(ok, lv, ws, tails(1), 1, 0, 10, 10, 10, None) == -1                # what pod_run_image refuses
    d = hip.PodDetections(X, X, X, X, X, X, X)
    part = lambda parts, out=d, mode=0: lib.pod_run_image_part(ok, lv, ws, mode, 0, 0, 10, 10, 10, 10, out, parts, None)
    for parts in (0, 6, 7, 9, 12, 16, -1):
        assert part(parts) == -1, parts
    assert part(hip.POD_PART_TAIL, out=None) == -1 and part(hip.POD_PART_FINISH, out=None) == -1
    assert part(hip.POD_PART_TAIL, mode=hip.POD_MODE_BAYES_OD) == -1 and part(hip.POD_PART_CANDIDATES, mode=5) == -1
