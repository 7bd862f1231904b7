"""train_head --resume as a command: a run stopped after two iterations and resumed for the third ends where an uninterrupted run of three
ends -- weights, momentum, loss state, sampler state and the loss line, to the bit -- with the fused step and with torch's optimiser.
Two 64 x 96 frames against SOLVER.IMS_PER_BATCH = 4: every step spans a pass boundary of the data set."""
import json
import os

import numpy as np
import pytest
import torch

from pod_compare_amd import train_head
from pod_compare_amd.head_train import head_convs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
YAML = os.path.join(os.path.dirname(train_head.__file__), "configs/BDD-Detection/retinanet/retinanet_R_50_FPN_1x.yaml")


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
    return root


def run(data, out_dir, max_iter, *flags):
    return train_head.main(["--config-file", YAML, "--coco-json", str(data / "gt.json"), "--image-root", str(data), "--random-init", "--output-dir", str(out_dir),
                            "--max-iter", str(max_iter), "--log-period", "1", "--min-size-test", "64", "--max-size-test", "96", "--loader-workers", "0",
                            "--device", DEV] + list(flags))


def final(out_dir):
    return torch.load(str(out_dir / "model_final.pth"), map_location="cpu", weights_only=True)


def assert_same_run(a, b, what):
    """Two checkpoints: model tensors and the whole trainer state, to the bit."""
    assert sorted(a["model"]) == sorted(b["model"]) and a["iteration"] == b["iteration"], what
    for k in a["model"]:
        assert torch.equal(a["model"][k], b["model"][k]), (what, "model", k)
    ta, tb = a[train_head.TRAINER_KEY], b[train_head.TRAINER_KEY]
    assert sorted(ta["momentum"]) == sorted(tb["momentum"]), what
    for k in ta["momentum"]:
        assert torch.equal(ta["momentum"][k], tb["momentum"][k]), (what, "momentum", k)
    assert ta["iteration"] == tb["iteration"] and ta["trained"] == tb["trained"] and ta["momentum_mu"] == tb["momentum_mu"], what
    la, lb = ta["loss_state"], tb["loss_state"]
    assert (la["current_step"], la["draws"]) == (lb["current_step"], lb["draws"]) and torch.equal(la["loss_normalizer"], lb["loss_normalizer"]), what
    sa, sb = ta["sampler"], tb["sampler"]
    assert sa["next_index"] == sb["next_index"] and sa["pending"] == sb["pending"] and torch.equal(sa["flip_generator"], sb["flip_generator"]), what


def stopped_and_resumed_equals_uninterrupted(data, tmp_path, capsys, flags, below_the_head):
    a = run(data, tmp_path / "a", 3, *flags)
    a2 = run(data, tmp_path / "a2", 3, *flags)
    A, A2 = final(tmp_path / "a"), final(tmp_path / "a2")
    assert_same_run(A, A2, "two uninterrupted runs")                     # first: a later failure then names resume, not the training step
    assert a["last_line"] == a2["last_line"] and a["last_line"].startswith("iter 3  loss_cls ")
    st = A[train_head.TRAINER_KEY]
    assert st["iteration"] == 3 and st["loss_state"]["current_step"] == 3 and st["loss_state"]["draws"] == 3 and len(st["momentum"]) == 2 * len(head_convs(a["model"].head)) + below_the_head
    assert all(bool(v.any()) for k, v in st["momentum"].items() if k.endswith(".weight"))
    assert st["sampler"]["pending"] == [] and st["sampler"]["next_index"] == 0          # 3 steps x 4 frames = 6 whole passes over 2 frames
    b = run(data, tmp_path / "b", 2, *flags)
    assert b["iterations"] == 2
    B2 = final(tmp_path / "b")
    assert B2[train_head.TRAINER_KEY]["iteration"] == 2
    capsys.readouterr()
    b = run(data, tmp_path / "b", 3, "--resume", *flags)
    lines = [l for l in capsys.readouterr().out.splitlines() if l.startswith("iter ")]
    assert b["iterations"] == 3 and len(lines) == 1                       # one step was taken
    assert b["last_line"] == a["last_line"], (b["last_line"], a["last_line"])
    assert_same_run(final(tmp_path / "b"), A, "stopped at 2 and resumed against uninterrupted")
    return tmp_path / "b"


def test_resume_with_the_fused_step_random_flip_and_the_backbone_training(data, tmp_path, capsys):
    flags = ("--train-backbone", "--fused-step", "--random-flip")
    b_dir = stopped_and_resumed_equals_uninterrupted(data, tmp_path, capsys, flags, below_the_head=2 * 8 + 42)
    # without --resume a run in that directory starts at iteration 0, as it always has
    again = run(data, b_dir, 1, *flags)
    assert again["iterations"] == 1 and again["last_line"].startswith("iter 1  loss_cls ")
    assert final(b_dir)[train_head.TRAINER_KEY]["iteration"] == 1


def test_resume_with_torchs_optimiser_restores_its_momentum(data, tmp_path, capsys):
    b_dir = stopped_and_resumed_equals_uninterrupted(data, tmp_path, capsys, (), below_the_head=0)
    # a checkpoint of a head-only run does not resume a --train-backbone one
    with pytest.raises(SystemExit) as e:
        run(data, b_dir, 4, "--resume", "--train-backbone")
    assert str(b_dir / "model_final.pth") in str(e.value) and "trained head" in str(e.value) and "head + fpn + backbone" in str(e.value)


def test_resume_restores_the_frames_that_waited_in_the_shape_buckets(tmp_path, capsys):
    """Two 64 x 96 frames and one 96 x 64: the wide frames complete a batch every second pass, the tall one waits.  The run stopped after
    two iterations holds three tall frames in its bucket, each with its flip; the resumed run's first step is the batch they complete."""
    from PIL import Image
    root = tmp_path / "frames"
    root.mkdir()
    rng = np.random.default_rng(5)
    images, anns = [], []
    for k, (h, w) in enumerate([(64, 96), (64, 96), (96, 64)]):
        Image.fromarray(rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)).save(root / ("g%d.png" % k))
        images.append({"id": 70 + k, "file_name": "g%d.png" % k, "height": h, "width": w})
        anns.append({"id": k + 1, "image_id": 70 + k, "category_id": 1 + k, "bbox": [8 + k, 10, 30, 36], "iscrowd": 0})
    (root / "gt.json").write_text(json.dumps({"images": images, "annotations": anns}))
    flags = ("--fused-step", "--random-flip")
    a = run(root, tmp_path / "a", 3, *flags)
    assert run(root, tmp_path / "b", 2, *flags)["iterations"] == 2
    waiting = final(tmp_path / "b")[train_head.TRAINER_KEY]["sampler"]
    assert waiting["next_index"] == 2 and [i for i, _ in waiting["pending"]] == [2, 2, 2]
    assert len({f for _, f in waiting["pending"]}) == 2                    # (seed 0: the three were not all drawn alike)
    capsys.readouterr()
    b = run(root, tmp_path / "b", 3, "--resume", *flags)
    assert len([l for l in capsys.readouterr().out.splitlines() if l.startswith("iter ")]) == 1
    assert b["iterations"] == 3 and b["last_line"] == a["last_line"]
    assert_same_run(final(tmp_path / "b"), final(tmp_path / "a"), "three waiting frames restored")
    assert final(tmp_path / "a")[train_head.TRAINER_KEY]["sampler"]["pending"] == []
