"""CPU side of data-parallel training: the declarations of the gradient bucket (K26), its layout, every refusal of pod_grad_pack that comes
before a launch, a rank's share of a batch, the per-rank loss states' way through a checkpoint file, the world-size check of --resume, and
all_reduce_flat on CPU tensors over gloo.  No GPU."""
import ctypes
import datetime
import inspect
import os

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from pod_compare_amd import data_parallel, hip, losses, modeling, train_head

NEW = ("pod_grad_bucket_layout", "pod_grad_pack")
C = hip.POD_SGD_CHUNK


def test_header_binding_and_library_carry_the_gradient_bucket():
    """Additions only: the symbols are declared, bound and exported; the ABI number stays 18 and K25's descriptor is the table."""
    from pod_compare_amd import build
    from tests.test_abi_cpu import HEADER, declared_symbols
    assert declared_symbols() == sorted(hip.EXPORTS)
    for name in NEW:
        assert name in hip.EXPORTS and name in declared_symbols()
    assert "pod_grad_bucket_layout" in hip._SIZE_QUERIES and "pod_grad_pack" not in hip._SIZE_QUERIES
    assert hip.POD_ABI_VERSION == 18 and "#define POD_ABI_VERSION 18\n" in open(HEADER).read()
    assert "k26_grad_bucket.hip" in build.SOURCES
    lib = ctypes.CDLL(build.build_library())
    assert lib.pod_abi_version() == hip.POD_ABI_VERSION and all(hasattr(lib, n) for n in NEW)
    bound = hip.load()
    assert bound.pod_grad_bucket_layout.restype is ctypes.c_int64 and len(bound.pod_grad_bucket_layout.argtypes) == 3
    assert len(bound.pod_grad_pack.argtypes) == 10 and bound.pod_grad_pack.argtypes[8] is ctypes.c_float
    assert [n for n, _ in hip.PodSgdTensor._fields_] == ["w", "grad", "momentum", "folded", "scale", "n", "per_channel"]
    assert len(bound.pod_sgd_step.argtypes) == 9                                # K25's entry point is as it was


def _table(*rows):
    t = (hip.PodSgdTensor * max(1, len(rows)))()
    for d, r in zip(t, rows):
        for k, v in r.items():
            setattr(d, k, v)
    return t


def _row(i, n, **kw):
    """Tensor i of a table on host addresses that are never dereferenced: 1 MiB apart, far below the bucket's."""
    base = 0x1000000 * (i + 1)
    return dict(dict(w=base, grad=base + 0x400000, momentum=base + 0x800000, n=n), **kw)


def test_layout_puts_every_tensor_on_sixteen_bytes():
    lib = hip.load()
    sizes = (0, 1, 3, 4, 5, 63, 4096, 4097)
    t = _table(*[_row(i, n) for i, n in enumerate(sizes)])
    off = (ctypes.c_int64 * (len(sizes) + 1))(*([-7] * (len(sizes) + 1)))
    total = lib.pod_grad_bucket_layout(t, len(sizes), off)
    want, run = [], 0
    for n in sizes:
        want.append(run)
        run += -(-n // 4) * 4
    assert list(off)[:len(sizes)] == want == [0, 0, 4, 8, 12, 20, 84, 4180] and off[len(sizes)] == -7
    assert total == run == 4180 + 4100 and total % 4 == 0 and all(o % 4 == 0 for o in want)
    assert lib.pod_grad_bucket_layout(t, len(sizes), None) == total            # offsets are optional
    # the n alone: other addresses, scales and folded filters give the same layout
    other = _table(*[_row(i + 20, n, **(dict(scale=0x500000, folded=0x600000, per_channel=1) if n else {})) for i, n in enumerate(sizes)])
    off2 = (ctypes.c_int64 * len(sizes))()
    assert lib.pod_grad_bucket_layout(other, len(sizes), off2) == total and list(off2) == want
    assert lib.pod_grad_bucket_layout(None, 0, None) == 0
    # -1 for what pod_sgd_chunk_map refuses
    for bad in (dict(w=None), dict(momentum=None), dict(n=-4), dict(grad=0x1400004), dict(w=0x1000008)):
        rows = [dict(_row(0, 63), **bad), _row(1, 5)]
        assert lib.pod_sgd_chunk_map(_table(*rows), 2, None, 0) == -1 and lib.pod_grad_bucket_layout(_table(*rows), 2, off) == -1, bad
    assert lib.pod_grad_bucket_layout(None, 2, None) == -1 and lib.pod_grad_bucket_layout(t, -1, None) == -1


ROWS = [_row(0, 27 * 64), _row(1, 63), _row(2, C + 1)]
TOTAL = 27 * 64 + 64 + C + 4
CHUNKS = 1 + 1 + 2
BUCKET = 0x40000000


def _pack(rows=ROWS, n_tensors=None, table_dev=0x90000, chunk_map=0xA0000, n_chunks=CHUNKS, offsets_dev=0xB0000, bucket=BUCKET, bucket_floats=TOTAL,
          scale=0.5, null_table=False):
    """pod_grad_pack on host addresses that are never dereferenced: whatever it returns comes from the argument checks."""
    t = _table(*rows)
    return hip.load().pod_grad_pack(None if null_table else t, table_dev, len(rows) if n_tensors is None else n_tensors, chunk_map, n_chunks, offsets_dev,
                                    bucket, bucket_floats, scale, None)


def test_the_valid_pack_passes_every_check_that_comes_before_the_device_is_touched():
    """The refusals below each differ from THIS call in one argument; with a device pointer missing it is refused last of all, and with
    nothing to do it returns POD_OK without touching anything."""
    lib = hip.load()
    assert lib.pod_grad_bucket_layout(_table(*ROWS), 3, None) == TOTAL and lib.pod_sgd_chunk_map(_table(*ROWS), 3, None, 0) == CHUNKS
    for kw in (dict(table_dev=None), dict(chunk_map=None), dict(offsets_dev=None), dict(bucket=None)):
        assert _pack(**kw) == -1, kw
    empty = [_row(0, 0), _row(1, 0, grad=None)]                                # every n == 0: a gradient may be missing where there is none
    assert _pack(rows=empty, n_chunks=0, bucket_floats=0, table_dev=None, chunk_map=None, offsets_dev=None, bucket=None) == 0
    assert _pack(rows=[], n_tensors=0, null_table=True, n_chunks=0, bucket_floats=0, table_dev=None, chunk_map=None, offsets_dev=None, bucket=None) == 0


@pytest.mark.parametrize("name,rows,kw", [
    ("null table", None, dict(null_table=True)),
    ("n_tensors < 0", None, dict(n_tensors=-1)),
    ("a gradient is missing", [dict(ROWS[0], grad=None)] + ROWS[1:], {}),
    ("the last gradient is missing", ROWS[:2] + [dict(ROWS[2], grad=None)], {}),
    ("null w", [dict(ROWS[0], w=None)] + ROWS[1:], {}),
    ("grad misaligned", [dict(ROWS[0], grad=ROWS[0]["grad"] + 4)] + ROWS[1:], {}),
    ("w misaligned", ROWS[:1] + [dict(ROWS[1], w=ROWS[1]["w"] + 8)] + ROWS[2:], {}),
    ("bucket misaligned", None, dict(bucket=BUCKET + 4)),
    ("bucket null", None, dict(bucket=None)),
    ("bucket begins inside a gradient", None, dict(bucket=ROWS[1]["grad"] + 16)),
    ("bucket ends inside a gradient", None, dict(bucket=ROWS[0]["grad"] - 4 * TOTAL + 16)),
    ("bucket holds a gradient", None, dict(bucket=ROWS[2]["grad"] - 4 * 64)),
    ("bucket one float short", None, dict(bucket_floats=TOTAL - 1)),
    ("bucket with the tail counted", None, dict(bucket_floats=TOTAL + 4)),
    ("the unpadded sum", None, dict(bucket_floats=27 * 64 + 63 + C + 1)),
    ("another table's chunk count", None, dict(n_chunks=CHUNKS + 1)),
    ("no chunks", None, dict(n_chunks=0)),
    ("scale 0", None, dict(scale=0.0)),
    ("scale < 0", None, dict(scale=-0.5)),
    ("scale nan", None, dict(scale=float("nan"))),
    ("scale inf", None, dict(scale=float("inf"))),
])
def test_pack_refusals_before_any_launch(name, rows, kw):
    """Nothing is enqueued: the addresses are not device memory, so a call that got as far as the copy would not return -1 (POD_E_INVALID)
    but -2, or fault."""
    assert _pack(**dict(dict(rows=ROWS if rows is None else rows), **kw)) == -1, name


def test_a_ranks_share_of_a_batch_and_the_refusal_of_a_batch_that_does_not_split():
    assert [data_parallel.rank_slice(16, r, 4) for r in range(4)] == [(0, 4), (4, 8), (8, 12), (12, 16)]
    assert data_parallel.rank_slice(4, 1, 2) == (2, 4) and data_parallel.rank_slice(3, 0, 1) == (0, 3)
    with pytest.raises(SystemExit) as e:
        data_parallel.rank_slice(16, 0, 3)
    assert "16" in str(e.value) and "3" in str(e.value) and "IMS_PER_BATCH" in str(e.value)
    with pytest.raises(ValueError):
        data_parallel.rank_slice(4, 2, 2)
    # the sampler files frames by key alone and hands back the batch in arrival order: rank r's frames are a slice of it
    sampler = train_head.FrameSampler(4)
    got = [sampler.add_keyed((3, 64, 96) if i != 2 else (3, 96, 64), 10 + i, bool(i % 2)) for i in range(5)]
    assert got[:4] == [None] * 4 and got[4] == [(10, False), (11, True), (13, True), (14, False)]
    assert got[4][slice(*data_parallel.rank_slice(4, 1, 2))] == [(13, True), (14, False)]
    assert sampler.state()["pending"] == [[12, 0]]


def test_the_command_refuses_a_batch_that_does_not_split_before_anything_is_built(tmp_path, monkeypatch):
    (tmp_path / "gt.json").write_text('{"images": [], "annotations": []}')
    monkeypatch.setenv("WORLD_SIZE", "3")
    monkeypatch.setenv("RANK", "1")
    monkeypatch.setattr(dist, "init_process_group", lambda *a, **k: None)       # (the refusal needs no process group)
    monkeypatch.setattr(dist, "destroy_process_group", lambda *a, **k: None)
    with pytest.raises(SystemExit) as e:                                        # the config's SOLVER.IMS_PER_BATCH is 4
        train_head.main(["--coco-json", str(tmp_path / "gt.json"), "--image-root", str(tmp_path), "--output-dir", str(tmp_path / "o"), "--data-parallel",
                         "--backend", "gloo", "--share-gpu"])
    assert "IMS_PER_BATCH = 4" in str(e.value) and "world size 3" in str(e.value)


def _tiny_trainer(**kw):
    torch.manual_seed(5)
    model = modeling.ProbabilisticRetinaNet(num_classes=7).eval()
    model.loss_state = losses.ProbabilisticLosses(num_classes=7, cls_var_num_samples=3, annealing_step=80000, seed=11)
    return train_head.HeadTrainer(model, **kw), model


def _rank_states():
    return [{"current_step": 9, "draws": 9 + r, "loss_normalizer": torch.tensor(50.25 + r, dtype=torch.float64)} for r in range(2)]


def test_per_rank_loss_states_round_trip_through_a_checkpoint_file(tmp_path):
    trainer, model = _tiny_trainer()
    model.loss_state.current_step, model.loss_state.draws, model.loss_state.loss_normalizer = 9, 9, 50.25
    one = train_head.trainer_state(trainer)
    assert "world" not in one and "ranks" not in one                            # a one-rank run writes the keys it always wrote
    assert train_head.trainer_state(trainer, ranks=[train_head.loss_state_of(trainer)]).keys() == one.keys()
    state = train_head.trainer_state(trainer, ranks=_rank_states())
    assert set(state) - set(one) == {"world", "ranks"} and state["world"] == 2
    path = str(tmp_path / "model_final.pth")
    torch.save({"model": {}, "iteration": 9, train_head.TRAINER_KEY: state}, path)
    back = train_head.read_trainer_state(path)                                  # weights_only=True
    assert back["world"] == 2 and len(back["ranks"]) == 2
    for got, want in zip(back["ranks"], _rank_states()):
        assert (got["current_step"], got["draws"]) == (want["current_step"], want["draws"])
        assert got["loss_normalizer"].dtype == torch.float64 and torch.equal(got["loss_normalizer"], want["loss_normalizer"])
    assert back["loss_state"]["draws"] == 9 and float(back["loss_state"]["loss_normalizer"]) == 50.25
    # rank 1 of a world of two takes its own entry
    other, omodel = _tiny_trainer()
    other.rank, other.world = 1, 2
    train_head.restore_trainer(other, back, path)
    assert omodel.loss_state.draws == 10 and omodel.loss_state.loss_normalizer == 51.25 and omodel.loss_state.current_step == 9


def test_resume_with_another_world_size_is_refused_and_names_the_file(tmp_path):
    trainer, _ = _tiny_trainer()
    two, one = train_head.trainer_state(trainer, ranks=_rank_states()), train_head.trainer_state(trainer)
    with pytest.raises(SystemExit) as e:                                        # a two-rank file at world 1
        train_head.restore_trainer(trainer, two, "two_ranks.pth")
    assert "two_ranks.pth" in str(e.value) and "2 ranks" in str(e.value) and "has 1" in str(e.value) and trainer.iteration == 0
    with pytest.raises(SystemExit) as e:                                        # a file without the fields resumes only at world 1
        train_head.check_world(one, 2, "one_rank.pth")
    assert "one_rank.pth" in str(e.value) and "1 rank," in str(e.value) and "has 2" in str(e.value)
    train_head.check_world(one, 1, "one_rank.pth")
    train_head.check_world(two, 2, "two_ranks.pth")
    with pytest.raises(SystemExit):                                             # `world` without as many entries
        train_head.check_world(dict(two, ranks=two["ranks"][:1]), 2, "short.pth")
    # the command refuses before a model is built or a GPU touched
    out = tmp_path / "out"
    out.mkdir()
    (tmp_path / "gt.json").write_text('{"images": [], "annotations": []}')
    torch.save({"model": {}, "iteration": 2, train_head.TRAINER_KEY: two}, str(out / "model_final.pth"))
    (out / "last_checkpoint").write_text("model_final.pth")
    with pytest.raises(SystemExit) as e:
        train_head.main(["--coco-json", str(tmp_path / "gt.json"), "--image-root", str(tmp_path), "--output-dir", str(out), "--resume"])
    assert str(out / "model_final.pth") in str(e.value) and "2 ranks" in str(e.value) and "has 1" in str(e.value)


def test_the_command_and_the_trainer_offer_data_parallelism_off_by_default(capsys):
    with pytest.raises(SystemExit) as e:
        train_head.main(["--help"])
    assert e.value.code == 0
    text = " ".join(capsys.readouterr().out.split())
    assert "--data-parallel" in text and "--backend" in text and "--share-gpu" in text
    assert inspect.signature(train_head.HeadTrainer.__init__).parameters["data_parallel"].default is None
    assert inspect.signature(train_head.save_checkpoint).parameters["ranks"].default is None
    trainer, _ = _tiny_trainer()
    assert trainer.bucket is None and (trainer.rank, trainer.world) == (0, 1)
    for name in ("forward_backward", "reduce_gradients", "optimizer_step"):
        assert callable(getattr(trainer, name))
    with pytest.raises(ValueError):                                             # the averaged gradients are stepped by K25
        _tiny_trainer(data_parallel=(0, 2, None))
    with pytest.raises(ValueError):
        trainer.reduce_gradients()


def _reduce_worker(rank, world, port, tmp):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(minutes=5))
    try:
        t = torch.arange(11, dtype=torch.float32) * (rank + 1) + 0.25
        assert not data_parallel.host_staged(t)
        assert data_parallel.all_reduce_flat(t) is t
        torch.save(t, os.path.join(tmp, "sum_%d.pt" % rank))
        dist.barrier()
    finally:
        dist.destroy_process_group()


def _spawned_reduce_worker(i, *args):
    _reduce_worker(i + 1, *args)


def test_all_reduce_flat_sums_cpu_tensors_over_gloo_at_world_two(tmp_path):
    port = 38500 + os.getpid() % 2000
    saved = {k: os.environ.get(k) for k in ("MASTER_ADDR", "MASTER_PORT")}
    ctx = mp.spawn(_spawned_reduce_worker, args=(2, port, str(tmp_path)), nprocs=1, join=False)
    try:
        _reduce_worker(0, 2, port, str(tmp_path))
        while not ctx.join():
            pass
    finally:
        if dist.is_initialized():
            dist.destroy_process_group()
        for p in ctx.processes:
            if p.is_alive():
                p.terminate()
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    want = torch.arange(11, dtype=torch.float32) * 3 + 0.5
    for r in range(2):
        assert torch.equal(torch.load(str(tmp_path / ("sum_%d.pt" % r)), weights_only=True), want), r
    assert not data_parallel.host_staged(torch.zeros(4))                        # no process group: nothing is staged
