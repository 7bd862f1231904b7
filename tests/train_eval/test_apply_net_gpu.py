"""Evaluation while training, end to end: train_eval.evaluate_model on a model object against the CPU referee applied to that model's
eval-mode head outputs, and train_head with --val-coco-json as a command -- a run with TEST.EVAL_PERIOD = 2 ends bit-equal to the run
without evaluation, --eval-only on its checkpoint prints the AP of its last evaluation, and two data-parallel ranks write the results
file of one, byte for byte.  Six synthetic 96 x 128 validation frames, four training frames, a random-init model.

The module shares its name with tests/test_apply_net_gpu.py so that the GPU run order in tests/conftest.py (GPU_ORDER, keyed by module
name) gives it a place."""
import contextlib
import json
import math
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist

from pod_compare_amd import train_eval, train_head
from pod_compare_amd.config import setup_config
from pod_compare_amd.probabilistic_inference import build_model
from tests.data_parallel import dp
from tests.helpers import assert_close
from tests.optimizer_step.test_apply_net_gpu import assert_same_run, final
from tests.train_eval.d2_inference_ref import Reference

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BASE = os.path.join(os.path.dirname(train_head.__file__), "configs/BDD-Detection/retinanet/retinanet_R_50_FPN_1x.yaml")
NAMES = ["car", "bus", "truck", "person", "rider", "bike", "motor"]
# the prior leaves a random-init model's scores at 0.01: a threshold below it, so that the command-line runs have detections to write
YAML_BODY = "_BASE_: %s\nINPUT:\n  MIN_SIZE_TEST: 96\n  MAX_SIZE_TEST: 128\nMODEL:\n  RETINANET:\n    SCORE_THRESH_TEST: 0.005\n"


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    from PIL import Image
    root = tmp_path_factory.mktemp("frames")
    rng = np.random.default_rng(11)
    cats = [{"id": k + 1, "name": n} for k, n in enumerate(NAMES)]
    for split, n, first in (("train", 4, 40), ("val", 6, 70)):
        images, anns = [], []
        for k in range(n):
            h, w = (96, 128) if (split == "train" or k % 2 == 0) else (120, 160)          # the odd validation frames are resized to 96 x 128
            name = "%s%d.png" % (split, k)
            Image.fromarray(rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)).save(root / name)
            images.append({"id": first + k, "file_name": name, "height": h, "width": w})
            anns.append({"id": 2 * k + 1, "image_id": first + k, "category_id": 1 + k % 3, "bbox": [6 + 4 * k, 8, 40, 36], "area": 1440, "iscrowd": 0})
            anns.append({"id": 2 * k + 2, "image_id": first + k, "category_id": 4, "bbox": [50, 20 + k, 44, 50], "area": 2200, "iscrowd": 0})
        (root / (split + ".json")).write_text(json.dumps({"images": images, "annotations": anns, "categories": cats}))
    (root / "plain.yaml").write_text(YAML_BODY % BASE)
    (root / "eval.yaml").write_text(YAML_BODY % BASE + "TEST:\n  EVAL_PERIOD: 2\n")
    return root


def command(data, out_dir, yaml, *flags, max_iter=4):
    return train_head.main(["--config-file", str(data / yaml), "--coco-json", str(data / "train.json"), "--image-root", str(data), "--random-init",
                            "--output-dir", str(out_dir), "--max-iter", str(max_iter), "--log-period", "1", "--loader-workers", "0", "--device", DEV] + list(flags))


def val_flags(data):
    return ("--val-coco-json", str(data / "val.json"), "--val-image-root", str(data))


def test_evaluate_model_writes_the_referees_detections(data, tmp_path, capsys):
    cfg = setup_config(str(data / "plain.yaml"))
    cfg.MODEL.DEVICE, cfg.MODEL.RETINANET.SCORE_THRESH_TEST, cfg.OUTPUT_DIR = DEV, 0.05, str(tmp_path)
    torch.manual_seed(5)
    model = build_model(cfg, load_weights=False)
    frame = torch.randint(0, 256, (3, 96, 128), generator=torch.Generator().manual_seed(1), dtype=torch.uint8).to(DEV)
    with torch.no_grad():           # tests/test_predictor_gpu.py's idea: spread the logits and shift cls_score.bias so that detections exist
        head = model.head           # (the box side stays at its initialisation: boxes near their anchors, inside the frame)
        spread = float(torch.cat([t.reshape(-1) for t in model(frame).cls]).std())
        assert math.isfinite(spread) and spread > 0.0, spread
        head.cls_score.weight.mul_(1.5 / spread)
        head.cls_score.bias.fill_(-2.5)
        logits = torch.cat([t.reshape(-1) for t in model(frame).cls])
        assert bool(torch.isfinite(logits).all()) and 0.001 < float((torch.sigmoid(logits) > 0.05).float().mean()) < 0.999
    model.train()                                     # the mode is the caller's, and restored
    seen = []

    def on_image(i, d, out, det):
        seen.append((i, d["image_id"], (d["height"], d["width"]), [t.cpu().clone() for t in out.cls], [t.cpu().clone() for t in out.delta],
                     [a.cpu().clone() for a in out.anchors], tuple(out.image_size), [t.cpu().clone() for t in det]))

    res = train_eval.evaluate_model(model, cfg, str(data / "val.json"), str(data), str(tmp_path), workers=2, on_image=on_image)
    assert model.training
    said = capsys.readouterr().out
    assert "copypaste: Task: bbox\ncopypaste: AP,AP50,AP75,APs,APm,APl\ncopypaste: " in said
    assert sum(int(s[7][1].numel()) for s in seen) > 6, "no detections"
    assert sorted(res) == ["bbox"] and list(res["bbox"])[:6] == list(train_eval.METRICS) and list(res["bbox"])[6:] == ["AP-" + n for n in NAMES]
    assert all(v == -1.0 or 0.0 <= v <= 100.0 for v in res["bbox"].values())
    records = json.load(open(train_eval.results_path(str(tmp_path))))
    assert [s[0] for s in seen] == list(range(6)) and len(records) > 6
    r = cfg.MODEL.RETINANET
    at = 0
    for i, image_id, out_size, cls, delta, anchors, image_size, det in seen:
        assert image_size == (96, 128)
        ref = Reference(cls, delta, anchors, 7, topk=r.TOPK_CANDIDATES_TEST, score_thresh=0.05, nms_thresh=r.NMS_THRESH_TEST,
                        max_detections=cfg.TEST.DETECTIONS_PER_IMAGE, image_size=image_size, out_size=out_size)
        assert ref.n > 0, i
        mine = records[at:at + ref.n]
        at += ref.n
        assert [m["image_id"] for m in mine] == [image_id] * ref.n and [m["category_id"] - 1 for m in mine] == ref.det_classes.tolist(), i
        xywh = ref.det_boxes.clone()
        xywh[:, 2:] -= xywh[:, :2]
        assert_close(torch.tensor([m["bbox"] for m in mine]), xywh, "evaluate_model: bbox XYWH")
        assert_close(torch.tensor([m["score"] for m in mine]), ref.det_scores, "evaluate_model: score")
        assert torch.equal(det[2], ref.det_classes)
    assert at == len(records)


@pytest.fixture(scope="module")
def evaluated(data, tmp_path_factory):
    """The 4-iteration run with TEST.EVAL_PERIOD = 2 every other command is compared with: what it returned, said and wrote."""
    import io
    out = tmp_path_factory.mktemp("evaluated")
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        res = command(data, out, "eval.yaml", "--train-backbone", "--fused-step", *val_flags(data))
    return res, buf.getvalue(), out


def test_a_run_with_evaluation_ends_bit_equal_to_the_run_without(data, evaluated, tmp_path):
    res, said, out = evaluated
    plain = command(data, tmp_path / "plain", "plain.yaml", "--train-backbone", "--fused-step")
    assert res["iterations"] == plain["iterations"] == 4 and res["last_line"] == plain["last_line"] and "eval_results" not in plain
    assert_same_run(final(out), final(tmp_path / "plain"), "TEST.EVAL_PERIOD = 2 with a validation set against no evaluation")
    assert not (tmp_path / "plain" / "inference").exists()
    # evaluated after iterations 2 and 4; the AP line stands behind the loss line of its iteration
    assert [it for it, _ in res["evaluations"]] == [2, 4] and res["eval_results"] is res["evaluations"][-1][1]
    lines = [l for l in said.splitlines() if l.startswith("iter ")]
    assert [l.split()[1] + " " + l.split()[2] for l in lines] == ["1 loss_cls", "2 loss_cls", "2 bbox", "3 loss_cls", "4 loss_cls", "4 bbox"], lines
    assert said.count("copypaste: Task: bbox") == 2
    records = json.load(open(train_eval.results_path(str(out))))
    assert len(records) > 0 and {r["image_id"] for r in records} <= set(range(70, 76)) and set(records[0]) == {"image_id", "category_id", "bbox", "score"}


def test_eval_only_prints_the_ap_of_the_runs_last_evaluation(data, evaluated, tmp_path, capsys):
    res, said, out = evaluated
    want = json.load(open(train_eval.results_path(str(out))))
    capsys.readouterr()
    only = command(data, tmp_path / "only", "plain.yaml", "--eval-only", "--weights", str(out / "model_final.pth"), *val_flags(data))
    text = capsys.readouterr().out
    assert only["eval_results"] == res["eval_results"] and "trainer" not in only
    last = [l for l in said.splitlines() if l.startswith("copypaste: ")][-1]
    assert last in text.splitlines() and not (tmp_path / "only" / "model_final.pth").exists()
    assert json.load(open(train_eval.results_path(str(tmp_path / "only")))) == want
    # --resume: OUTPUT_DIR/last_checkpoint instead of MODEL.WEIGHTS
    again = command(data, out, "plain.yaml", "--eval-only", "--resume", *val_flags(data))
    assert again["eval_results"] == res["eval_results"]


def eval_worker(rank, world, port, tmp, data, weights):
    from pathlib import Path
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=dp.TIMEOUT)
    tmp, data = Path(tmp), Path(data)
    try:
        with open(str(tmp / ("stdout_%d.txt" % rank)), "w") as f, contextlib.redirect_stdout(f):
            res = command(data, tmp / "dp", "plain.yaml", "--eval-only", "--weights", weights, "--data-parallel", "--backend", "gloo", "--share-gpu",
                          *val_flags(data))
        with open(str(tmp / ("res_%d.json" % rank)), "w") as f:
            json.dump(res["eval_results"], f)
    finally:
        dist.destroy_process_group()


def _spawned_eval_worker(i, *args):
    eval_worker(i + 1, *args)


def test_two_ranks_write_the_results_file_of_one(data, evaluated, tmp_path):
    res, said, out = evaluated
    port = 39500 + os.getpid() % 2000
    dp.with_one_spawned_rank(eval_worker, _spawned_eval_worker, (2, port, str(tmp_path), str(data), str(out / "model_final.pth")))
    one = open(train_eval.results_path(str(out)), "rb").read()
    two = open(train_eval.results_path(str(tmp_path / "dp")), "rb").read()
    assert len(one) > 2 and one == two
    assert json.load(open(str(tmp_path / "res_0.json"))) == res["eval_results"] and json.load(open(str(tmp_path / "res_1.json"))) == {}
    assert (tmp_path / "stdout_1.txt").read_text() == ""
