"""The full box covariance as the commands select it: train_head under `BBOX_COV_LOSS: {COVARIANCE_TYPE: full}` of a user's YAML trains a
90-channel bbox_cov predictor under each of the three objectives (K28), repeatably and resumably to the bit; --bbox-cov-type full on the
diagonal YAML is the full YAML; compute_losses evaluates either loss on the checkpoint; build_predictor loads it and runs a frame; a
diagonal checkpoint is refused by a full head.  Two 64 x 96 frames, two boxes.  SOLVER.STEPS and BASE_LR as in
tests/score_losses/test_apply_net_gpu.py, for its reasons: the annealing step is STEPS[1] (at 80000 the covariance loss would weigh
nothing in three steps), and at 2.5e-9 every weight of a random initialisation stays finite, which the runs assert."""
import json
import os

import numpy as np
import pytest
import torch

from pod_compare_amd import checkpoint, compute_losses, config, train_head
from pod_compare_amd.probabilistic_inference import build_predictor

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CONFIGS = os.path.join(os.path.dirname(train_head.__file__), "configs")
BASE = os.path.join(CONFIGS, "BDD-Detection/retinanet/retinanet_R_50_FPN_1x_reg_cls_var.yaml")
FLAGS = ("--random-init", "--fused-step")
NAMES = ("negative_log_likelihood", "second_moment_matching", "energy_loss")
SOLVER = 'SOLVER: {STEPS: [1, 2], BASE_LR: 2.5e-9}\n'


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    from PIL import Image
    root = tmp_path_factory.mktemp("frames")
    rng = np.random.default_rng(3)
    images = []
    for k in range(2):
        Image.fromarray(rng.integers(0, 256, size=(64, 96, 3), dtype=np.uint8)).save(root / ("f%d.png" % k))
        images.append({"id": 40 + k, "file_name": "f%d.png" % k, "height": 64, "width": 96})
    anns = [{"id": 1, "image_id": 40, "category_id": 1, "bbox": [10, 8, 34, 32], "iscrowd": 0},
            {"id": 2, "image_id": 40, "category_id": 4, "bbox": [50, 20, 40, 40], "iscrowd": 0}]
    (root / "gt.json").write_text(json.dumps({"images": images, "annotations": anns}))
    for name in NAMES:
        (root / (name + ".yaml")).write_text('_BASE_: "%s"\nMODEL:\n  PROBABILISTIC_MODELING:\n    BBOX_COV_LOSS: {NAME: "%s", COVARIANCE_TYPE: "full", '
                                             'NUM_SAMPLES: 64}\n' % (BASE, name) + SOLVER)
    (root / "diagonal.yaml").write_text('_BASE_: "%s"\nMODEL:\n  PROBABILISTIC_MODELING:\n    BBOX_COV_LOSS: {NAME: "energy_loss", NUM_SAMPLES: 64}\n' % BASE
                                        + SOLVER)
    return root


def run(data, yaml, out_dir, max_iter, *flags):
    return train_head.main(["--config-file", str(data / yaml), "--coco-json", str(data / "gt.json"), "--image-root", str(data),
                            "--output-dir", str(out_dir), "--max-iter", str(max_iter), "--log-period", "1", "--min-size-test", "64",
                            "--max-size-test", "96", "--loader-workers", "0", "--device", DEV] + list(FLAGS) + list(flags))


def final(out_dir):
    return torch.load(str(out_dir / "model_final.pth"), map_location="cpu", weights_only=True)


def cov_weight(ckpt):
    (key,) = [k for k in ckpt["model"] if k.endswith("bbox_cov.weight")]
    return ckpt["model"][key]


def assert_same_run(a, b, what):
    """Two checkpoints: weights, momentum and loss state, to the bit."""
    assert sorted(a["model"]) == sorted(b["model"]) and a["iteration"] == b["iteration"], what
    for k in a["model"]:
        assert torch.equal(a["model"][k], b["model"][k]), (what, "model", k)
    ta, tb = a[train_head.TRAINER_KEY], b[train_head.TRAINER_KEY]
    assert sorted(ta["momentum"]) == sorted(tb["momentum"]), what
    for k in ta["momentum"]:
        assert torch.equal(ta["momentum"][k], tb["momentum"][k]), (what, "momentum", k)
    la, lb = ta["loss_state"], tb["loss_state"]
    assert sorted(la) == sorted(lb) == ["current_step", "draws", "loss_normalizer"], what          # no key was added
    assert (la["current_step"], la["draws"]) == (lb["current_step"], lb["draws"]) and torch.equal(la["loss_normalizer"], lb["loss_normalizer"]), what


def box_reg(line):
    return float(line.split("loss_box_reg ")[1].split()[0])


@pytest.fixture(scope="module")
def trained(data, tmp_path_factory):
    """Three iterations under the energy score with the full covariance: (the run's result, its directory)."""
    out = tmp_path_factory.mktemp("full_energy")
    res = run(data, "energy_loss.yaml", out, 3)
    state = res["model"].loss_state
    assert state.bbox_cov_loss == "energy_loss" and state.bbox_cov_num_samples == 64 and state.draws == 3 and state.annealing_step == 2
    assert res["model"].head.bbox_cov.out_channels == 90
    return res, out


@pytest.mark.parametrize("name", NAMES)
def test_three_iterations_under_each_objective(data, trained, tmp_path, name):
    res, out = trained if name == "energy_loss" else (run(data, name + ".yaml", tmp_path / name, 3), tmp_path / name)
    assert res["iterations"] == 3 and res["last_line"].startswith("iter 3  loss_cls ") and np.isfinite(box_reg(res["last_line"]))
    assert res["model"].loss_state.bbox_cov_loss == name
    ckpt = final(out)
    assert all(bool(torch.isfinite(v).all()) for v in ckpt["model"].values() if v.is_floating_point())
    assert tuple(cov_weight(ckpt).shape) == (90, 256, 3, 3)
    print(name, res["last_line"])


def test_two_runs_are_bit_equal(data, trained, tmp_path):
    a, a_dir = trained
    a2 = run(data, "energy_loss.yaml", tmp_path / "a2", 3)
    assert_same_run(final(a_dir), final(tmp_path / "a2"), "two uninterrupted runs")
    assert a["last_line"] == a2["last_line"]


def test_stopped_and_resumed_equals_uninterrupted(data, trained, tmp_path, capsys):
    a, a_dir = trained
    assert run(data, "energy_loss.yaml", tmp_path / "b", 2)["iterations"] == 2
    capsys.readouterr()
    b = run(data, "energy_loss.yaml", tmp_path / "b", 3, "--resume")
    lines = [l for l in capsys.readouterr().out.splitlines() if l.startswith("iter ")]
    assert b["iterations"] == 3 and len(lines) == 1                       # one step was taken
    assert b["last_line"] == a["last_line"], (b["last_line"], a["last_line"])
    assert_same_run(final(tmp_path / "b"), final(a_dir), "stopped at 2 and resumed against uninterrupted")


def test_the_type_flag_on_the_diagonal_yaml_equals_the_full_yaml(data, trained, tmp_path):
    a, a_dir = trained
    f = run(data, "diagonal.yaml", tmp_path / "flag", 3, "--bbox-cov-type", "full")
    assert f["model"].head.bbox_cov.out_channels == 90
    assert_same_run(final(tmp_path / "flag"), final(a_dir), "--bbox-cov-type full against COVARIANCE_TYPE: full")
    assert f["last_line"] == a["last_line"]


def test_compute_losses_evaluates_nll_and_energy_on_the_checkpoint(data, trained):
    _, a_dir = trained
    common = ["--config-file", str(data / "energy_loss.yaml"), "--coco-json", str(data / "gt.json"), "--image-root", str(data), "--weights",
              str(a_dir / "model_final.pth"), "--iteration", "2", "--min-size-test", "64", "--max-size-test", "96", "--loader-workers", "0",
              "--device", DEV]
    es = compute_losses.main(common + ["--bbox-cov-loss", "energy_loss", "--bbox-cov-samples", "64"])
    nll = compute_losses.main(common + ["--bbox-cov-loss", "negative_log_likelihood"])
    assert es["annealing_weight"] == 1.0 and nll["annealing_weight"] == 1.0 and es["images"] == nll["images"] == 2
    assert es["bbox_cov_loss"] == "energy_loss" and nll["bbox_cov_loss"] == "negative_log_likelihood"
    assert es["bbox_cov_type"] == nll["bbox_cov_type"] == "full"
    print("validation energy score", es["loss_box_reg"], "NLL", nll["loss_box_reg"])
    assert np.isfinite(es["loss_box_reg"]) and np.isfinite(nll["loss_box_reg"]) and es["loss_box_reg"] != nll["loss_box_reg"]
    assert es["loss_cls"] > 0 and es["positives_per_image"] == nll["positives_per_image"] > 0


def test_the_predictor_loads_the_checkpoint_and_runs_a_frame(data, trained):
    _, a_dir = trained
    cfg = config.setup_config(str(data / "energy_loss.yaml"), os.path.join(CONFIGS, "Inference/standard_nms.yaml"))
    cfg.MODEL.WEIGHTS, cfg.OUTPUT_DIR, cfg.MODEL.DEVICE = str(a_dir / "model_final.pth"), "", DEV
    cfg.MODEL.RETINANET.SCORE_THRESH_TEST = 0.0          # (a model three steps from a random initialisation: keep whatever it scores)
    pred = build_predictor(cfg)
    assert pred.model.loaded_from.endswith("model_final.pth") and pred.model.head.bbox_cov.out_channels == 90
    frame = torch.randint(0, 256, (3, 64, 96), generator=torch.Generator().manual_seed(7), dtype=torch.uint8).to(DEV)
    res = pred([{"image": frame, "height": 64, "width": 96, "image_id": 3}])
    m = len(res)
    assert res.pred_boxes.tensor.shape == (m, 4) and res.pred_boxes_covariance.shape == (m, 4, 4) and res.pred_cls_probs.shape == (m, 7)
    assert bool(torch.isfinite(res.pred_boxes.tensor).all()) and bool(torch.isfinite(res.pred_boxes_covariance).all())
    assert bool(torch.isfinite(res.scores).all())
    print("standard_nms on the trained full-covariance checkpoint:", m, "detections")


def test_a_diagonal_checkpoint_into_a_full_head_raises(data, tmp_path):
    d = run(data, "diagonal.yaml", tmp_path / "diag", 1)
    assert d["model"].head.bbox_cov.out_channels == 36 and tuple(cov_weight(final(tmp_path / "diag")).shape) == (36, 256, 3, 3)
    evaluate = lambda yaml, *flags: compute_losses.main(
        ["--config-file", str(data / yaml), "--coco-json", str(data / "gt.json"), "--image-root", str(data), "--weights",
         str(tmp_path / "diag" / "model_final.pth"), "--min-size-test", "64", "--max-size-test", "96", "--loader-workers", "0", "--device", DEV]
        + list(flags))
    for yaml, flags in (("energy_loss.yaml", ()), ("diagonal.yaml", ("--bbox-cov-type", "full"))):          # both shapes are named
        with pytest.raises(checkpoint.CheckpointError, match=r"\(36, 256, 3, 3\).*\(90, 256, 3, 3\)"):
            evaluate(yaml, *flags)
    back = evaluate("energy_loss.yaml", "--bbox-cov-type", "diagonal")                                          # and the flag the other way loads it
    assert back["bbox_cov_type"] == "diagonal" and np.isfinite(back["loss_box_reg"])
