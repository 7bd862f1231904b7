"""train_head --train-loader as a command: six PNG frames of two aspects and three sizes, one of them without annotations; mixed-size
batches of two at freeze point 2 under the fused step.  Two runs end bit-equal; --batch-on-gpu (K31 in the loop) ends bit-equal to the host
loader; a run stopped at 2 and resumed to 3 equals the uninterrupted one, with and without loader threads; --data-parallel at world 1
equals the plain run; without the flag the sampler state keeps exactly its three keys.

The module shares its name with tests/test_apply_net_gpu.py so that the GPU run order in tests/conftest.py (GPU_ORDER, keyed by module
name) gives it a place."""
import json
import math
import os

import numpy as np
import pytest
import torch

from pod_compare_amd import train_head

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BASE = os.path.join(os.path.dirname(train_head.__file__), "configs/BDD-Detection/retinanet/retinanet_R_50_FPN_1x.yaml")
FLAGS = ("--train-backbone", "--fused-step", "--train-loader")
SIZES = [(64, 96), (64, 96), (64, 96), (96, 64), (96, 64), (48, 80)]          # the last has no annotation


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    from PIL import Image
    root = tmp_path_factory.mktemp("frames")
    rng = np.random.default_rng(7)
    images, anns = [], []
    for k, (h, w) in enumerate(SIZES):
        Image.fromarray(rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)).save(root / ("f%d.png" % k))
        images.append({"id": 40 + k, "file_name": "f%d.png" % k, "height": h, "width": w})
        if k < 5:
            anns.append({"id": 2 * k + 1, "image_id": 40 + k, "category_id": 1 + k % 3, "bbox": [6 + k, 8, 30, 28], "iscrowd": 0})
            anns.append({"id": 2 * k + 2, "image_id": 40 + k, "category_id": 4, "bbox": [30, 20 + k, 26, 30], "iscrowd": 0})
    (root / "gt.json").write_text(json.dumps({"images": images, "annotations": anns}))
    (root / "model.yaml").write_text("_BASE_: %s\nSOLVER:\n  IMS_PER_BATCH: 2\nINPUT:\n  MIN_SIZE_TRAIN: [48, 64]\n  MIN_SIZE_TRAIN_SAMPLING: choice\n"
                                     "  MAX_SIZE_TRAIN: 96\n" % BASE)
    return root


def run(data, out_dir, max_iter, *flags, workers=0, yaml=None):
    return train_head.main(["--config-file", str(data / "model.yaml") if yaml is None else yaml, "--coco-json", str(data / "gt.json"), "--image-root", str(data),
                            "--random-init", "--output-dir", str(out_dir), "--max-iter", str(max_iter), "--log-period", "1", "--loader-workers", str(workers),
                            "--device", DEV] + list(flags))


def final(out_dir):
    return torch.load(str(out_dir / "model_final.pth"), map_location="cpu", weights_only=True)


def assert_same_run(a, b, what):
    """tests/optimizer_step/test_apply_net_gpu.py's comparison with the plan's sampler keys: model tensors and the whole trainer state, to the bit."""
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
    assert sorted(sa) == sorted(sb) == sorted(["kind", "pass_generator", "draw_generator", "position", "passes", "emitted", "frames", "waiting"]), what
    assert all(sa[k] == sb[k] for k in ("kind", "position", "passes", "emitted", "frames", "waiting")), (what, sa, sb)
    assert torch.equal(sa["pass_generator"], sb["pass_generator"]) and torch.equal(sa["draw_generator"], sb["draw_generator"]), what


@pytest.fixture(scope="module")
def whole(data, tmp_path_factory):
    """The uninterrupted run of three iterations every other run is compared with."""
    out = tmp_path_factory.mktemp("whole")
    return run(data, out, 3, *FLAGS), final(out)


def test_three_iterations_on_mixed_batches(data, whole, tmp_path, capsys):
    a, A = whole
    assert a["iterations"] == 3 and a["last_line"].startswith("iter 3  loss_cls ")
    for word in a["last_line"].split()[3:6:2]:
        assert math.isfinite(float(word))
    # the plan: five frames, never the one without annotations; batches of one aspect group; the drawn sizes vary inside a batch
    assert a["plan"].indices == [0, 1, 2, 3, 4] and len(a["trained"]) == 3
    entries = [e for b in a["trained"] for e in b]
    assert all(e.index != 5 for e in entries) and all(len(b) == 2 for b in a["trained"])
    assert all(len({SIZES[e.index][1] > SIZES[e.index][0] for e in b}) == 1 for b in a["trained"])
    assert {e.short_edge for e in entries} <= {48, 64} and all(max(e.size) <= 96 for e in entries)
    st = A[train_head.TRAINER_KEY]
    assert st["sampler"]["kind"] == "train_loader" and st["sampler"]["emitted"] == 3 and st["sampler"]["frames"] == 5 and st["iteration"] == 3
    capsys.readouterr()
    a2 = run(data, tmp_path / "a2", 3, *FLAGS)
    said = capsys.readouterr().out
    assert "Removed 1 images with no usable annotations. 5 images left." in said and len([l for l in said.splitlines() if l.startswith("iter ")]) == 3
    assert a2["last_line"] == a["last_line"] and a2["trained"] == a["trained"]
    assert_same_run(final(tmp_path / "a2"), A, "the same command twice")


def test_batch_on_gpu_ends_where_the_host_loader_ends(data, whole, tmp_path):
    a, A = whole
    g = run(data, tmp_path / "g", 3, "--batch-on-gpu", *FLAGS)
    assert g["last_line"] == a["last_line"] and g["trained"] == a["trained"]
    assert_same_run(final(tmp_path / "g"), A, "K31 in the loop against the host loader")


@pytest.mark.parametrize("workers", [0, 2])
def test_stopped_and_resumed_equals_uninterrupted(data, whole, tmp_path, capsys, workers):
    a, A = whole
    assert run(data, tmp_path / "b", 2, *FLAGS, workers=workers)["iterations"] == 2
    assert final(tmp_path / "b")[train_head.TRAINER_KEY]["sampler"]["emitted"] == 2
    capsys.readouterr()
    b = run(data, tmp_path / "b", 3, "--resume", *FLAGS, workers=workers)
    assert len([l for l in capsys.readouterr().out.splitlines() if l.startswith("iter ")]) == 1           # one step was taken
    assert b["iterations"] == 3 and b["last_line"] == a["last_line"] and b["trained"] == a["trained"][2:]
    assert_same_run(final(tmp_path / "b"), A, "stopped at 2 and resumed against uninterrupted, %d loader threads" % workers)


def test_data_parallel_at_world_one_equals_the_plain_run(data, whole, tmp_path, monkeypatch):
    a, A = whole
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    d = run(data, tmp_path / "d", 3, "--data-parallel", *FLAGS)
    assert d["last_line"] == a["last_line"] and d["trained"] == a["trained"]
    assert_same_run(final(tmp_path / "d"), A, "--data-parallel at world 1 against the plain fused step")


def test_without_the_flag_the_sampler_state_keeps_its_three_keys(data, whole, tmp_path):
    r = run(data, tmp_path / "p", 3, "--train-backbone", "--fused-step", "--min-size-test", "64", "--max-size-test", "96", yaml=BASE)
    assert r["iterations"] == 3 and "plan" not in r
    st = final(tmp_path / "p")[train_head.TRAINER_KEY]
    assert sorted(st["sampler"]) == ["flip_generator", "next_index", "pending"]
    # and the two kinds of data order do not resume one another
    with pytest.raises(SystemExit) as e:
        run(data, tmp_path / "p", 4, "--resume", *FLAGS)
    assert str(tmp_path / "p" / "model_final.pth") in str(e.value) and "`frame_sampler`" in str(e.value) and "`train_loader`" in str(e.value)
