"""The box-covariance loss as the commands select it: train_head under `BBOX_COV_LOSS: {NAME: energy_loss, NUM_SAMPLES: 64}` of a user's
YAML is repeatable and resumable to the bit (the energy score's draws are keyed by the loss state's seed word, which a checkpoint carries),
--bbox-cov-loss overrides the name, and compute_losses evaluates either loss on one checkpoint.  Two 64 x 96 frames, two boxes.
SOLVER.STEPS is [1, 2]: the annealing step is STEPS[1], and at the packaged 80000 the covariance loss's weight in a three-step run would
be below 1e-6 and show nothing.  SOLVER.BASE_LR is 2.5e-9: from a random initialisation the classification loss of the variance head
(loss_attenuation, exp of a random log-variance) starts near 1e5, and at the packaged 0.0025 it is inf after the first step and the
weights NaN after the second -- under the NLL as under the energy loss, to the same bits of loss_cls -- which would leave nothing to
compare; at 2.5e-9 every weight stays finite, which `trained` asserts."""
import json
import os

import numpy as np
import pytest
import torch

from pod_compare_amd import compute_losses, train_head

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BASE = os.path.join(os.path.dirname(train_head.__file__), "configs/BDD-Detection/retinanet/retinanet_R_50_FPN_1x_reg_cls_var.yaml")
FLAGS = ("--random-init", "--fused-step")


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
    (root / "energy.yaml").write_text('_BASE_: "%s"\nMODEL:\n  PROBABILISTIC_MODELING:\n    BBOX_COV_LOSS: {NAME: "energy_loss", NUM_SAMPLES: 64}\n'
                                      'SOLVER: {STEPS: [1, 2], BASE_LR: 2.5e-9}\n' % BASE)
    return root


def run(data, out_dir, max_iter, *flags):
    return train_head.main(["--config-file", str(data / "energy.yaml"), "--coco-json", str(data / "gt.json"), "--image-root", str(data),
                            "--output-dir", str(out_dir), "--max-iter", str(max_iter), "--log-period", "1", "--min-size-test", "64",
                            "--max-size-test", "96", "--loader-workers", "0", "--device", DEV] + list(FLAGS) + list(flags))


def final(out_dir):
    return torch.load(str(out_dir / "model_final.pth"), map_location="cpu", weights_only=True)


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


@pytest.fixture(scope="module")
def trained(data, tmp_path_factory):
    """Three iterations under the energy loss: (the run's result, its directory)."""
    out = tmp_path_factory.mktemp("energy_a")
    res = run(data, out, 3)
    state = res["model"].loss_state
    assert state.bbox_cov_loss == "energy_loss" and state.bbox_cov_num_samples == 64 and state.draws == 3 and state.annealing_step == 2
    assert all(bool(torch.isfinite(v).all()) for v in final(out)["model"].values() if v.is_floating_point())
    return res, out


def box_reg(line):
    return float(line.split("loss_box_reg ")[1].split()[0])


def test_two_runs_under_the_energy_loss_are_bit_equal(data, trained, tmp_path):
    a, a_dir = trained
    a2 = run(data, tmp_path / "a2", 3)
    assert_same_run(final(a_dir), final(tmp_path / "a2"), "two uninterrupted runs")
    assert a["last_line"] == a2["last_line"] and a["last_line"].startswith("iter 3  loss_cls ") and np.isfinite(box_reg(a["last_line"]))


def test_stopped_and_resumed_equals_uninterrupted(data, trained, tmp_path, capsys):
    a, a_dir = trained
    assert run(data, tmp_path / "b", 2)["iterations"] == 2
    capsys.readouterr()
    b = run(data, tmp_path / "b", 3, "--resume")
    lines = [l for l in capsys.readouterr().out.splitlines() if l.startswith("iter ")]
    assert b["iterations"] == 3 and len(lines) == 1                       # one step was taken
    assert b["last_line"] == a["last_line"], (b["last_line"], a["last_line"])
    assert_same_run(final(tmp_path / "b"), final(a_dir), "stopped at 2 and resumed against uninterrupted")


def test_the_flag_overrides_the_yaml(data, trained, tmp_path):
    a, a_dir = trained
    n = run(data, tmp_path / "nll", 3, "--bbox-cov-loss", "negative_log_likelihood")
    assert n["model"].loss_state.bbox_cov_loss == "negative_log_likelihood"
    A, N = final(a_dir), final(tmp_path / "nll")
    assert sorted(A["model"]) == sorted(N["model"]) and any(not torch.equal(A["model"][k], N["model"][k]) for k in A["model"])
    print("energy:", a["last_line"], "| NLL:", n["last_line"])
    assert box_reg(n["last_line"]) != box_reg(a["last_line"])


def test_compute_losses_evaluates_either_loss_on_one_checkpoint(data, trained):
    _, a_dir = trained
    common = ["--config-file", str(data / "energy.yaml"), "--coco-json", str(data / "gt.json"), "--image-root", str(data), "--weights",
              str(a_dir / "model_final.pth"), "--iteration", "2", "--min-size-test", "64", "--max-size-test", "96", "--loader-workers", "0",
              "--device", DEV]
    es = compute_losses.main(common + ["--bbox-cov-loss", "energy_loss", "--bbox-cov-samples", "64"])
    nll = compute_losses.main(common + ["--bbox-cov-loss", "negative_log_likelihood"])
    assert es["annealing_weight"] == 1.0 and nll["annealing_weight"] == 1.0 and es["images"] == nll["images"] == 2
    assert es["bbox_cov_loss"] == "energy_loss" and nll["bbox_cov_loss"] == "negative_log_likelihood"
    print("validation energy score", es["loss_box_reg"], "NLL", nll["loss_box_reg"])
    assert np.isfinite(es["loss_box_reg"]) and np.isfinite(nll["loss_box_reg"]) and es["loss_box_reg"] != nll["loss_box_reg"]
    assert es["loss_cls"] > 0 and es["positives_per_image"] == nll["positives_per_image"] > 0
