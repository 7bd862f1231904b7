"""train_head --data-parallel as a command.  Two ranks on one GPU over gloo (rank 0 is the test process, rank 1 the one process that is
started; both find the process group initialised, as main allows): only rank 0 prints and writes, the checkpoint loads strictly, a run
stopped after two iterations and resumed for the third ends where the uninterrupted run of three ends -- weights, momentum, sampler, EVERY
rank's loss state and the loss line, to the bit -- and a resume at another world size is refused.  On one rank the flag changes no bit of
what --fused-step writes.  Three 64 x 96 frames against SOLVER.IMS_PER_BATCH = 4: every step spans a pass boundary of the data set, and the
two halves of a batch differ."""
import contextlib
import json
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist

from pod_compare_amd import checkpoint, config, train_head
from pod_compare_amd.probabilistic_inference import build_model
from tests.data_parallel import dp
from tests.optimizer_step.test_apply_net_gpu import YAML, assert_same_run, final, run

pytestmark = pytest.mark.gpu
FLAGS = ("--train-backbone", "--random-flip", "--data-parallel", "--backend", "gloo", "--share-gpu")


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    from PIL import Image
    root = tmp_path_factory.mktemp("frames")
    rng = np.random.default_rng(7)
    images, anns = [], []
    for k in range(3):
        Image.fromarray(rng.integers(0, 256, size=(64, 96, 3), dtype=np.uint8)).save(root / ("f%d.png" % k))
        images.append({"id": 40 + k, "file_name": "f%d.png" % k, "height": 64, "width": 96})
        anns.append({"id": k + 1, "image_id": 40 + k, "category_id": 1 + k, "bbox": [8 + 20 * k, 10, 34, 32 + 4 * k], "iscrowd": 0})
    (root / "gt.json").write_text(json.dumps({"images": images, "annotations": anns}))
    return root


def command_worker(rank, world, port, tmp, data):
    """The three runs of the resume test on one rank, under one process group: a (3 iterations), b (2), b resumed to 3.  What the rank
    printed and what main returned go to <tmp>/cmd_<rank>.json."""
    from pathlib import Path
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=dp.TIMEOUT)
    tmp, data, out = Path(tmp), Path(data), []
    try:
        for name, max_iter, extra in (("a", 3, ()), ("b", 2, ()), ("b", 3, ("--resume",))):
            with open(str(tmp / ("stdout_%d.txt" % rank)), "a") as f, contextlib.redirect_stdout(f):
                res = run(data, tmp / name, max_iter, *(FLAGS + extra))
            assert res["trainer"].bucket.host_staged and res["trainer"].world == 2
            out.append({"iterations": res["iterations"], "last_line": res["last_line"], "checkpoints": res["checkpoints"]})
        with open(str(tmp / ("cmd_%d.json" % rank)), "w") as f:
            json.dump(out, f)
    finally:
        dist.destroy_process_group()


def _spawned_command_worker(i, *args):
    command_worker(i + 1, *args)


def test_two_ranks_write_one_checkpoint_and_resume_to_the_bits_of_the_uninterrupted_run(data, tmp_path):
    port = 37500 + os.getpid() % 2000
    dp.with_one_spawned_rank(command_worker, _spawned_command_worker, (2, port, str(tmp_path), str(data)))
    r0, r1 = (json.load(open(str(tmp_path / ("cmd_%d.json" % r)))) for r in range(2))
    # only rank 0 writes files and prints; every rank knows the loss line (the rank means came with the gradients)
    assert all(x["checkpoints"] and x["checkpoints"][-1].endswith("model_final.pth") for x in r0) and all(x["checkpoints"] == [] for x in r1)
    assert (tmp_path / "stdout_1.txt").read_text() == ""
    lines = [l for l in (tmp_path / "stdout_0.txt").read_text().splitlines() if l.startswith("iter ")]
    assert len(lines) == 3 + 2 + 1 and lines[2] == lines[5] == r0[0]["last_line"] and lines[:2] == lines[3:5]
    assert [x["last_line"] for x in r0] == [x["last_line"] for x in r1] and r0[0]["last_line"].startswith("iter 3  loss_cls ")
    assert [x["iterations"] for x in r0] == [3, 2, 3] == [x["iterations"] for x in r1]
    assert sorted(os.listdir(str(tmp_path / "a"))) == ["last_checkpoint", "model_final.pth"]
    # stopped at 2 and resumed to 3 against uninterrupted: the whole file, and every rank's loss state
    A, B = final(tmp_path / "a"), final(tmp_path / "b")
    assert_same_run(B, A, "two ranks: stopped at 2 and resumed against uninterrupted")
    ta, tb = A[train_head.TRAINER_KEY], B[train_head.TRAINER_KEY]
    assert ta["world"] == tb["world"] == 2 and len(ta["ranks"]) == len(tb["ranks"]) == 2 and ta["iteration"] == 3
    for ra, rb_ in zip(ta["ranks"], tb["ranks"]):
        assert (ra["current_step"], ra["draws"]) == (rb_["current_step"], rb_["draws"]) == (3, 3) and torch.equal(ra["loss_normalizer"], rb_["loss_normalizer"])
    assert torch.equal(ta["ranks"][0]["loss_normalizer"], ta["loss_state"]["loss_normalizer"])       # `loss_state` is the writing rank's
    assert all(bool(v.any()) for k, v in ta["momentum"].items() if k.endswith(".weight"))
    # the checkpoint is a model like any other
    cfg = config.setup_config(YAML)
    cfg.MODEL.DEVICE = "cpu"
    torch.manual_seed(123)
    fresh = build_model(cfg, load_weights=False, fold=False)
    assert checkpoint.load_model_weights(fresh, str(tmp_path / "a"), "", strict=True) == str(tmp_path / "a" / "model_final.pth")
    # a resume at world 1 of the two-rank file is refused, before a model is built
    with pytest.raises(SystemExit) as e:
        run(data, tmp_path / "b", 4, "--resume", "--train-backbone", "--random-flip", "--fused-step")
    assert str(tmp_path / "b" / "model_final.pth") in str(e.value) and "2 ranks" in str(e.value) and "has 1" in str(e.value)


def test_on_one_rank_the_flag_writes_the_bits_of_the_fused_step(data, tmp_path):
    a = run(data, tmp_path / "fused", 2, "--train-backbone", "--random-flip", "--fused-step")
    b = run(data, tmp_path / "dp", 2, "--train-backbone", "--random-flip", "--data-parallel")
    assert b["trainer"].bucket is not None and b["trainer"].world == 1 and not b["trainer"].bucket.host_staged and a["trainer"].bucket is None
    A, B = final(tmp_path / "fused"), final(tmp_path / "dp")
    assert_same_run(A, B, "--data-parallel on one rank against --fused-step")
    assert sorted(A[train_head.TRAINER_KEY]) == sorted(B[train_head.TRAINER_KEY]) and "world" not in B[train_head.TRAINER_KEY]
    assert a["last_line"] == b["last_line"] and a["last_line"].startswith("iter 2  loss_cls ")
