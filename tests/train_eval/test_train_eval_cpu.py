"""CPU side of the evaluation-while-training feature: the referee against detectron2's literal lines, the new config keys, the K32
boundary (header, binding, library, argument checks before any launch), train_head's new flags, verify_results, and the shape of the
results json and the AP dictionary (fed from a hand-made evaluate + accumulate output: no GPU)."""
import ctypes
import json
import math
import os
import re

import numpy as np
import pytest
import torch

from pod_compare_amd import build, hip, train_eval, train_head
from pod_compare_amd.config import get_cfg, setup_config
from tests.train_eval import d2_inference_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
HEADER = os.path.join(ROOT, "include", "pod_mi355x.h")
BASE = os.path.join(os.path.dirname(train_head.__file__), "configs/BDD-Detection/retinanet/retinanet_R_50_FPN_1x.yaml")
K32 = ("pod_retinanet_infer_workspace", "pod_retinanet_score", "pod_retinanet_topk", "pod_retinanet_decode", "pod_retinanet_postprocess",
       "pod_retinanet_infer_image")


@pytest.mark.parametrize("K, topk", [(1, 50), (7, 200), (7, 100000), (15, 333)])
def test_referee_equals_the_literal_form_on_tie_free_inputs(K, topk):
    """flatten().sigmoid_(), sort on the scores, // K, % K -- against the stable sort on the logits.  The scores are a permutation of an
    evenly spaced grid (neighbours 2e-4 apart): no two are equal, so detectron2's unstable sort has one answer."""
    A, H, W = 3, 5, 7
    n = A * K * H * W
    g = torch.Generator().manual_seed(K + topk)
    scores = torch.linspace(0.0451, 0.0451 + 2e-4 * (n - 1), n, dtype=torch.float64)[torch.randperm(n, generator=g)]
    planes = torch.log(scores / (1 - scores)).float().reshape(A * K, H, W)
    flat = ref.flat_logits(planes, K)
    assert torch.equal(flat.reshape(H, W, A, K)[2, 3, 1], planes.reshape(A, K, H, W)[1, :, 2, 3])          # f = ((h W + w) A + a) K + k
    assert len(torch.unique(torch.sigmoid(flat))) == n
    (f, s), (lf, ls) = ref.rank_level(flat, topk, 0.05), ref.literal_level(flat, topk, 0.05)
    assert torch.equal(f, lf) and torch.equal(s, ls) and 0 < len(f) <= min(topk, n)
    assert torch.equal(f // K, lf // K) and torch.equal(f % K, lf % K) and bool((s[:-1] > s[1:]).all()) and float(s.min()) > 0.05
    if topk >= n:
        assert len(f) == int((torch.sigmoid(flat) > 0.05).sum())
    # the stable sort is what decides between equal logits: the lower flat index first
    tied = flat.clone()
    tied[[11, 4, 30]] = 9.0
    assert ref.rank_level(tied, 2, 0.05)[0].tolist() == [4, 11]


def test_config_carries_the_new_keys_with_detectron2s_defaults(tmp_path):
    cfg = get_cfg()
    assert cfg.TEST.EVAL_PERIOD == 0 and cfg.TEST.EXPECTED_RESULTS == [] and cfg.TEST.DETECTIONS_PER_IMAGE == 100
    y = tmp_path / "m.yaml"
    y.write_text("_BASE_: %s\nTEST:\n  EVAL_PERIOD: 500\n  EXPECTED_RESULTS: [['bbox', 'AP', 38.5, 0.2]]\n" % BASE)
    cfg = setup_config(str(y))
    assert cfg.TEST.EVAL_PERIOD == 500 and cfg.TEST.EXPECTED_RESULTS == [["bbox", "AP", 38.5, 0.2]] and cfg.TEST.DETECTIONS_PER_IMAGE == 100
    p = train_eval.inference_params(cfg, 9)
    assert (p.num_classes, p.topk_candidates, p.score_thresh, p.nms_thresh, p.max_detections, p.box_weights) == (7, 1000, 0.05, 0.5, 100, (1.0, 1.0, 1.0, 1.0))


def test_header_binding_and_library_name_the_new_symbols():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"#define\s+POD_ABI_VERSION\s+18\b", text) and hip.POD_ABI_VERSION == 18
    lib = ctypes.CDLL(build.build_library())
    for name in K32:
        assert re.search(r"\b%s\s*\(" % name, text) and name in hip.EXPORTS and hasattr(lib, name), name
    assert lib.pod_abi_version() == 18 and "k32_retinanet_inference.hip" in build.SOURCES
    assert "PodRetinaNetLayout" in text and ctypes.sizeof(hip.PodRetinaNetLayout) == 16 * 8


def _geometry(L=3, K=7, topk=1000, max_det=100, n_runs=1):
    c = hip.PodConfig()
    c.n_levels, c.n_runs, c.num_anchors, c.num_classes, c.topk, c.max_detections = L, n_runs, 9, K, topk, max_det
    lv = (hip.PodLevel * max(L, 1))()
    base = 0
    for l in range(L):
        lv[l].H, lv[l].W, lv[l].anchor_base = 12 >> l, 16 >> l, base
        base += lv[l].H * lv[l].W * 9
    return c, lv, base


def test_k32_entry_points_check_their_arguments_before_any_launch():
    """Argument validation happens on the host: safe without a GPU.  The limits are the library's existing ones."""
    lib = hip.load()
    c, lv, R = _geometry()
    lo = hip.PodRetinaNetLayout()
    total = lib.pod_retinanet_infer_workspace(c, lv, lo)
    n = 3 * 1000
    assert total == lo.total > 0 and lo.cand_keys == 0 and lo.cand_count >= 8 * R * 7 and lo.sel_keys - lo.cand_count >= 4 * 2 * hip.POD_MAX_LEVELS
    offs = [getattr(lo, f) for f, _ in hip.PodRetinaNetLayout._fields_]
    assert offs == sorted(offs) and all(o % 256 == 0 for o in offs)
    assert lo.scores - lo.boxes >= 16 * n and lo.total - lo.nms_scratch >= lib.pod_nms_scratch_bytes(n)
    assert lib.pod_retinanet_infer_workspace(c, lv, None) == total
    for bad in (dict(K=16), dict(K=0), dict(topk=hip.POD_MAX_TOPK + 1), dict(topk=0), dict(max_det=hip.POD_MAX_DETECTIONS + 1), dict(n_runs=2),
                dict(L=0), dict(L=hip.POD_MAX_LEVELS + 1), dict(L=5, topk=2048)):
        cb, lb, _ = _geometry(**bad)
        assert lib.pod_retinanet_infer_workspace(cb, lb, None) == -1, bad
    lv[1].anchor_base += 1                                   # the levels' lists must tile the key buffer
    assert lib.pod_retinanet_infer_workspace(c, lv, None) == -1
    lv[1].anchor_base -= 1
    lv[0].H = 1 << 14
    lv[0].W = 1 << 14                                        # A * K * H * W past 2^31
    assert lib.pod_retinanet_infer_workspace(c, lv, None) == -1
    c, lv, R = _geometry()
    p = ctypes.c_void_p(256)                                 # a non-null, aligned pointer that is never dereferenced: every call below returns first
    assert lib.pod_retinanet_score(c, lv, None, p, None) == -1 and lib.pod_retinanet_score(c, lv, p, p, None) == -1      # levels[].cls is null
    assert lib.pod_retinanet_topk(c, lv, None, p, p, p, p, p, p, None) == -1
    assert lib.pod_retinanet_decode(c, lv, p, p, p, p, p, p, p, p, p, p, None) == -1                                      # levels[].delta is null
    assert lib.pod_retinanet_postprocess(c, p, p, p, p, p, 1.0, 1.0, 8.0, 8.0, p, p, None, p, None) == -1
    assert lib.pod_retinanet_postprocess(c, p, p, ctypes.c_void_p(260), p, p, 1.0, 1.0, 8.0, 8.0, p, p, p, p, None) == -1      # boxes: 16-byte aligned
    assert lib.pod_retinanet_infer_image(c, lv, p, None, 8, 8, 8, 8, p, p, p, p, None) == -1
    assert lib.pod_retinanet_infer_image(c, lv, p, p, 0, 8, 8, 8, p, p, p, p, None) == -1
    assert lib.pod_retinanet_infer_image(c, lv, p, p, 8, 8, 8, 8, p, p, p, p, None) == -1                                 # levels[].cls is null


def _args(tmp_path, yaml_body="", *flags):
    y = tmp_path / "m.yaml"
    y.write_text("_BASE_: %s\n%s" % (BASE, yaml_body))
    return ["--config-file", str(y), "--coco-json", str(tmp_path / "none.json"), "--image-root", str(tmp_path), "--random-init", "--output-dir",
            str(tmp_path / "out"), "--device", "cuda:0"] + list(flags)


def test_eval_period_without_a_validation_set_is_refused_before_a_model_is_built(tmp_path, monkeypatch):
    from pod_compare_amd import probabilistic_inference
    monkeypatch.setattr(train_head, "build_model", lambda *a, **k: pytest.fail("a model was built"))
    monkeypatch.setattr(probabilistic_inference, "build_model", lambda *a, **k: pytest.fail("a model was built"))
    with pytest.raises(SystemExit) as e:
        train_head.main(_args(tmp_path, "TEST:\n  EVAL_PERIOD: 2\n"))
    assert "TEST.EVAL_PERIOD = 2" in str(e.value) and "--val-coco-json" in str(e.value)
    with pytest.raises(SystemExit) as e:
        train_head.main(_args(tmp_path, "TEST:\n  EVAL_PERIOD: -1\n", "--val-coco-json", "v.json", "--val-image-root", "."))
    assert "TEST.EVAL_PERIOD = -1" in str(e.value)
    with pytest.raises(SystemExit) as e:
        train_head.main(_args(tmp_path, "", "--eval-only"))
    assert "--eval-only needs --val-coco-json" in str(e.value)
    with pytest.raises(SystemExit) as e:
        train_head.main(_args(tmp_path, "", "--val-coco-json", "v.json"))
    assert "--val-image-root" in str(e.value)


def test_eval_only_argument_handling(tmp_path, monkeypatch):
    """--eval-only goes to _eval_only with the flags parsed and builds no trainer; without the new flags the parser's defaults are inert."""
    a = train_head.arg_parser().parse_args(_args(tmp_path))
    assert (a.val_coco_json, a.val_image_root, a.eval_only) == ("", "", False)
    assert train_head.evaluation_period(get_cfg(), a) == 0
    seen = {}

    def fake(args, cfg, rank, world, group, say):
        seen.update(args=args, cfg=cfg, rank=rank, world=world)
        return {"eval_results": {"bbox": {"AP": 1.0}}}

    monkeypatch.setattr(train_head, "_eval_only", fake)
    monkeypatch.setattr(train_head, "HeadTrainer", lambda *a, **k: pytest.fail("an optimiser was built"))
    out = train_head.main(_args(tmp_path, "TEST:\n  EVAL_PERIOD: 7\n", "--eval-only", "--resume", "--val-coco-json", "v.json", "--val-image-root", "frames",
                                "--weights", "w.pth"))
    assert out == {"eval_results": {"bbox": {"AP": 1.0}}} and (seen["rank"], seen["world"]) == (0, 1)
    assert seen["args"].eval_only and seen["args"].resume and seen["args"].val_coco_json == "v.json" and seen["args"].val_image_root == "frames"
    assert seen["cfg"].MODEL.WEIGHTS == "w.pth" and seen["cfg"].TEST.EVAL_PERIOD == 7 and seen["cfg"].OUTPUT_DIR == str(tmp_path / "out")


def test_verify_results_semantics():
    cfg = get_cfg()
    results = {"bbox": {"AP": 38.6, "AP50": 59.0, "APs": float("nan")}}
    said = []
    assert train_eval.verify_results(cfg, results, said.append) is True and said == []                  # nothing expected
    cfg.TEST.EXPECTED_RESULTS = [["bbox", "AP", 38.5, 0.2], ["bbox", "AP50", 59.0, 0.0]]
    assert train_eval.verify_results(cfg, results, said.append) is True and said == ["Results verification passed."]
    for bad in ([["bbox", "AP", 38.5, 0.05]],              # |actual - expected| > tolerance
                [["bbox", "AP75", 40.0, 100.0]],           # the metric is missing
                [["segm", "AP", 38.5, 100.0]],             # the task is missing
                [["bbox", "APs", 1.0, 100.0]]):            # not finite
        cfg.TEST.EXPECTED_RESULTS = bad
        said.clear()
        with pytest.raises(SystemExit) as e:
            train_eval.verify_results(cfg, results, said.append)
        assert e.value.code == 1 and said[0] == "Result verification failed!", bad
    cfg.TEST.EXPECTED_RESULTS = [["bbox", "AP", 38.4, 0.2]]          # exactly at the tolerance (in doubles: 38.6 - 38.4 > 0.2 fails, as detectron2's would)
    assert (abs(38.6 - 38.4) > 0.2) is True
    with pytest.raises(SystemExit):
        train_eval.verify_results(cfg, results, said.append)


def test_results_json_and_ap_dictionary_have_coco_evaluators_shape(tmp_path):
    reverse = {v: k for k, v in train_head.evaluation_category_map("bdd_train", "bdd_val").items()}
    boxes = torch.tensor([[10.0, 20.0, 50.5, 80.25], [0.0, 0.0, 4.0, 3.0]])
    recs = train_eval.instances_to_records(71, boxes, torch.tensor([0.75, 0.5]), torch.tensor([0, 3]), reverse)
    assert recs == [{"image_id": 71, "category_id": 1, "bbox": [10.0, 20.0, 40.5, 60.25], "score": 0.75},
                    {"image_id": 71, "category_id": 4, "bbox": [0.0, 0.0, 4.0, 3.0], "score": 0.5}]
    assert json.loads(json.dumps(recs)) == recs and train_eval.instances_to_records(71, boxes[:0], boxes[:0, 0], torch.zeros(0, dtype=torch.long), reverse) == []
    # a BDD model on KITTI: classes KITTI does not annotate have no id there
    kitti = {v: k for k, v in train_head.evaluation_category_map("bdd_train", "kitti_val").items()}
    assert [r["category_id"] for r in train_eval.instances_to_records(1, boxes, torch.tensor([0.9, 0.8]), torch.tensor([3, 1]), kitti)] == [2]
    assert train_eval.results_path("/o") == "/o/inference/coco_instances_results.json"

    gt = {"images": [{"id": 71, "file_name": "a.png", "height": 96, "width": 128}],
          "annotations": [{"id": 1, "image_id": 71, "category_id": 1, "bbox": [10, 20, 40, 60], "area": 2400, "iscrowd": 0}],
          "categories": [{"id": k + 1, "name": n} for k, n in enumerate(["car", "bus", "truck", "person", "rider", "bike", "motor"])]}
    (tmp_path / "gt.json").write_text(json.dumps(gt))
    calls = []

    def stub(gts, dts, img_ids, cat_ids, iou_thrs, rec_thrs, max_dets, area_rngs):
        """A hand-made evaluate + accumulate output: category 0 at precision 0.5 everywhere, category 3 at 0.25 for the small area only."""
        calls.append((len(gts), len(dts), list(img_ids), list(cat_ids)))
        T, R, K, A, M = len(iou_thrs), len(rec_thrs), len(cat_ids), len(area_rngs), len(max_dets)
        precision, recall = -np.ones((T, R, K, A, M)), -np.ones((T, K, A, M))
        precision[:, :, 0, :, :] = 0.5
        precision[:, :, 3, 1, :] = 0.25
        precision[:, :, 3, 0, :] = 0.25
        recall[:, 0] = 1.0
        return precision, recall, np.zeros((T, R, K, A, M))

    res = train_eval.score_results(recs, str(tmp_path / "gt.json"), "bdd_train", "bdd_val", impl=stub)
    assert calls == [(1, 2, [71], [1, 2, 3, 4, 5, 6, 7])]
    assert list(res) == ["AP", "AP50", "AP75", "APs", "APm", "APl", "AP-car", "AP-bus", "AP-truck", "AP-person", "AP-rider", "AP-bike", "AP-motor"]
    assert res["AP"] == res["AP50"] == res["AP75"] == pytest.approx(37.5) and res["APs"] == pytest.approx(37.5) and res["APm"] == res["APl"] == 50.0
    assert res["AP-car"] == 50.0 and res["AP-person"] == 25.0 and res["AP-bus"] == -1.0 and all(math.isfinite(v) for v in res.values())
    # no predictions: every metric is -1, nothing is scored
    assert train_eval.score_results([], str(tmp_path / "gt.json"), "bdd_train", "bdd_val", impl=stub)["AP"] == -1.0 and len(calls) == 1
    lines = train_eval.copypaste_lines({"bbox": res})
    assert lines == ["copypaste: Task: bbox", "copypaste: AP,AP50,AP75,APs,APm,APl", "copypaste: 37.5000,37.5000,37.5000,37.5000,50.0000,50.0000"]
    assert train_eval.ap_line(4, {"bbox": res}) == "iter 4  bbox AP 37.5000  AP50 37.5000  AP75 37.5000" and train_eval.ap_line(4, {}).startswith("iter 4  bbox AP -1.0000")
