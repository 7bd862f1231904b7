"""CPU side of the fused optimiser step (K25) and of resumable training: the declarations of pod_sgd_step, its descriptor's layout, its chunk
map, every refusal that comes before a launch, the flip of the boxes, the trainer state's way through a checkpoint file, and the command's
new flags.  No GPU."""
import ctypes
import inspect
import os
import subprocess

import pytest
import torch

from pod_compare_amd import checkpoint, hip, losses, modeling, train_head

NEW = ("pod_sgd_chunk_map", "pod_sgd_step")
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def test_header_binding_and_library_carry_the_sgd_step():
    """Additions only: the symbols are declared, bound and exported; the ABI number stays 18."""
    from pod_compare_amd import build
    from tests.test_abi_cpu import HEADER, declared_symbols
    for name in NEW:
        assert name in hip.EXPORTS and name in declared_symbols()
    assert "pod_sgd_chunk_map" in hip._SIZE_QUERIES
    header = open(HEADER).read()
    assert hip.POD_ABI_VERSION == 18 and "#define POD_ABI_VERSION 18\n" in header
    assert "#define POD_SGD_CHUNK %d\n" % hip.POD_SGD_CHUNK in header and hip.POD_SGD_CHUNK % 4 == 0
    assert "k25_sgd_step.hip" in build.SOURCES
    lib = ctypes.CDLL(build.build_library())
    assert lib.pod_abi_version() == hip.POD_ABI_VERSION and all(hasattr(lib, n) for n in NEW)
    bound = hip.load()
    assert bound.pod_sgd_chunk_map.restype is ctypes.c_int64 and len(bound.pod_sgd_chunk_map.argtypes) == 4
    assert len(bound.pod_sgd_step.argtypes) == 9 and bound.pod_sgd_step.argtypes[5:8] == [ctypes.c_float] * 3


def test_descriptor_layout_matches_c(tmp_path):
    """sizeof / offsetof of hip.PodSgdTensor against the header, compiled with gcc."""
    fields = [n for n, _ in hip.PodSgdTensor._fields_]
    assert fields == ["w", "grad", "momentum", "folded", "scale", "n", "per_channel"]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "pod_mi355x.h"\nint main(void){printf("%zu", sizeof(PodSgdTensor));\n'
                   + "".join('printf(" %%zu", offsetof(PodSgdTensor, %s));\n' % f for f in fields) + "return 0;}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got == [ctypes.sizeof(hip.PodSgdTensor)] + [getattr(hip.PodSgdTensor, f).offset for f in fields]
    assert ctypes.sizeof(hip.PodSgdTensor) % 8 == 0


def _table(*rows):
    t = (hip.PodSgdTensor * max(1, len(rows)))()
    for d, r in zip(t, rows):
        for k, v in r.items():
            setattr(d, k, v)
    return t


GOOD = dict(w=0x10000, grad=0x20000, momentum=0x30000, folded=0x40000, scale=0x50000, n=27 * 64, per_channel=27)
PLAIN = dict(w=0x60000, grad=0x70000, momentum=0x80000, n=63)
VALID_CHUNKS = -(-GOOD["n"] // hip.POD_SGD_CHUNK) + 1                       # of the table [GOOD, PLAIN]


def _step(rows, n_tensors=None, table_dev=0x90000, chunk_map=0xA0000, n_chunks=None, lr=0.01, mu=0.9, wd=1e-4, null_table=False):
    """pod_sgd_step on host addresses that are never dereferenced: whatever it returns comes from the argument checks."""
    lib = hip.load()
    t = _table(*rows)
    n = len(rows) if n_tensors is None else n_tensors
    if n_chunks is None:
        n_chunks = sum(-(-r.get("n", 0) // hip.POD_SGD_CHUNK) for r in rows)
    return lib.pod_sgd_step(None if null_table else t, table_dev, n, chunk_map, n_chunks, lr, mu, wd, None)


def test_chunk_map_lists_every_chunk_of_every_tensor_once_in_table_order():
    lib = hip.load()
    C = hip.POD_SGD_CHUNK
    sizes = [0, 1, 63, C - 1, C, C + 1, 3 * C + 3, 0, 36]
    rows = [dict(PLAIN, n=n) for n in sizes]
    t = _table(*rows)
    want = [(i, c) for i, n in enumerate(sizes) for c in range(-(-n // C))]
    assert lib.pod_sgd_chunk_map(t, len(rows), None, 0) == len(want) == 11
    buf = (ctypes.c_int32 * (2 * len(want) + 2))(*([-7] * (2 * len(want) + 2)))
    assert lib.pod_sgd_chunk_map(t, len(rows), buf, len(want) - 1) == len(want) and set(buf) == {-7}      # too small a map is left alone
    assert lib.pod_sgd_chunk_map(t, len(rows), buf, len(want)) == len(want)
    assert [(buf[2 * k], buf[2 * k + 1]) for k in range(len(want))] == want and buf[2 * len(want)] == buf[2 * len(want) + 1] == -7
    assert lib.pod_sgd_chunk_map(None, 0, None, 0) == 0 and lib.pod_sgd_chunk_map(None, 2, None, 0) == -1
    assert lib.pod_sgd_chunk_map(_table(dict(PLAIN, w=None)), 1, None, 0) == -1


def test_the_valid_table_passes_every_check_that_comes_before_the_device_is_touched():
    """The refusals below each differ from THIS call in one argument.  With the device table missing it is refused last of all, after every
    check of the descriptors and rates; with nothing to do it returns POD_OK without touching anything."""
    assert _step([GOOD, PLAIN], table_dev=None) == -1 and _step([GOOD, PLAIN], chunk_map=None) == -1
    assert _step([dict(GOOD, n=0), dict(PLAIN, n=0)], table_dev=None, chunk_map=None) == 0                # every n == 0
    assert _step([], n_tensors=0, null_table=True, table_dev=None, chunk_map=None) == 0                     # n_tensors == 0
    assert _step([dict(GOOD, n=0, grad=None), dict(PLAIN, n=0, scale=None)]) == 0
    assert hip.load().pod_sgd_chunk_map(_table(GOOD, PLAIN), 2, None, 0) == VALID_CHUNKS                     # the descriptors themselves are valid


@pytest.mark.parametrize("name,row,kw", [
    ("null table", None, dict(null_table=True)),
    ("n_tensors < 0", None, dict(n_tensors=-1)),
    ("null w", dict(GOOD, w=None), {}),
    ("null momentum", dict(GOOD, momentum=None), {}),
    ("n < 0", dict(PLAIN, n=-4), {}),
    ("w misaligned", dict(GOOD, w=0x10008), {}),
    ("grad misaligned", dict(GOOD, grad=0x20004), {}),
    ("momentum misaligned", dict(GOOD, momentum=0x30002), {}),
    ("folded misaligned", dict(GOOD, folded=0x40008), {}),
    ("scale misaligned", dict(GOOD, scale=0x50004), {}),
    ("scale without per_channel", dict(GOOD, per_channel=0), {}),
    ("negative per_channel", dict(GOOD, per_channel=-27), {}),
    ("n % per_channel", dict(GOOD, per_channel=25), {}),
    ("folded without scale", dict(GOOD, scale=None), {}),
    ("folded == w", dict(GOOD, folded=GOOD["w"]), {}),
    ("lr nan", None, dict(lr=float("nan"))),
    ("lr inf", None, dict(lr=float("inf"))),
    ("momentum nan", None, dict(mu=float("nan"))),
    ("weight decay inf", None, dict(wd=float("inf"))),
    ("momentum 1", None, dict(mu=1.0)),
    ("momentum < 0", None, dict(mu=-0.1)),
    ("weight decay < 0", None, dict(wd=-1e-4)),
    ("another table's chunk count", None, dict(n_chunks=VALID_CHUNKS + 1)),
])
def test_refusals_before_any_launch(name, row, kw):
    """Each call is the valid one of the test above with ONE argument changed; the chunk count is the valid table's, so a refusal is the
    changed argument's.  Nothing is enqueued: the addresses are not device memory."""
    rows = [GOOD if row is None else row, PLAIN]
    assert _step(rows, **dict(dict(n_chunks=VALID_CHUNKS), **kw)) == -1, name
    if row is not None:
        assert hip.load().pod_sgd_chunk_map(_table(*rows), 2, None, 0) == -1, name


def test_hflip_boxes_is_detectron2s_hflip_transform():
    g = torch.Generator().manual_seed(3)
    W = 96
    x1 = torch.randint(0, W - 1, (50,), generator=g).float()
    x2 = (x1 + 1 + torch.randint(0, W, (50,), generator=g).float()).clamp(max=W)
    y = torch.randint(0, 64, (50, 2), generator=g).float()
    boxes = torch.stack([x1, y[:, 0], x2, y[:, 1]], dim=1)
    kept = boxes.clone()
    flipped = train_head.hflip_boxes(boxes, W)
    assert torch.equal(boxes, kept)                                        # not in place
    assert torch.equal(flipped[:, 0], W - x2) and torch.equal(flipped[:, 2], W - x1) and torch.equal(flipped[:, [1, 3]], boxes[:, [1, 3]])
    assert bool((flipped[:, 0] < flipped[:, 2]).all()) and bool((flipped[:, 0] >= 0).all()) and bool((flipped[:, 2] <= W).all())
    assert torch.equal(train_head.hflip_boxes(flipped, W), boxes)          # integer-valued boxes: twice is the identity, to the bit
    assert torch.equal(train_head.hflip_boxes(torch.tensor([[10.0, 5.0, 30.0, 9.0]]), 96.0), torch.tensor([[66.0, 5.0, 86.0, 9.0]]))
    assert tuple(train_head.hflip_boxes(torch.zeros((0, 4)), W).shape) == (0, 4)


def _tiny_trainer(**kw):
    torch.manual_seed(5)
    model = modeling.ProbabilisticRetinaNet(num_classes=7).eval()
    model.loss_state = losses.ProbabilisticLosses(num_classes=7, cls_var_num_samples=3, annealing_step=80000, seed=11)
    return train_head.HeadTrainer(model, **kw), model


def test_trainer_state_round_trips_through_a_checkpoint_file(tmp_path):
    """torch.save -> the restricted unpickler (weights_only=True, what read_checkpoint_file uses): every field comes back as it went in, the
    model tensors still load, and a trainer restored from it continues at that iteration with those buffers."""
    trainer, model = _tiny_trainer(train_fpn=True)
    names = trainer.param_names()
    assert len(names) == len(set(names)) == len(trainer.params) and "head.cls_score.bias" in names and "backbone.fpn_lateral3.weight" in names
    g = torch.Generator().manual_seed(1)
    for p in trainer.params[::2]:                                          # torch's path: a buffer exists once a step has been taken
        trainer.opt.state[p]["momentum_buffer"] = torch.randn(p.shape, generator=g)
    trainer.iteration, model.loss_state.current_step, model.loss_state.draws = 567, 567, 567
    model.loss_state.loss_normalizer = torch.tensor(87.5675678905675, dtype=torch.float64)
    sampler = train_head.FrameSampler(4, random_flip=True, seed=9)
    drawn = [sampler.draw_flip() for _ in range(5)]
    assert True in drawn and False in drawn
    for k, shape in enumerate([(3, 64, 96), (3, 96, 64), (3, 64, 96)]):
        assert sampler.add(7 + k, drawn[k], torch.zeros(shape, dtype=torch.uint8), torch.zeros((0, 4)), torch.zeros(0, dtype=torch.int64)) is None
    sampler.next_index = 10
    state = train_head.trainer_state(trainer, sampler, random_seed=9)
    path = str(tmp_path / "model_0000566.pth")
    torch.save({"model": {"head.cls_score.bias": torch.ones(63)}, "iteration": 567, train_head.TRAINER_KEY: state}, path)
    assert set(checkpoint.read_checkpoint_file(path)) == {"head.cls_score.bias"}                 # the loaders see the model alone
    back = train_head.read_trainer_state(path)
    assert back["iteration"] == 567 and back["trained"] == ["head", "fpn"] and back["random_seed"] == 9 and back["momentum_mu"] == 0.9
    assert back["loss_state"]["current_step"] == 567 and back["loss_state"]["draws"] == 567
    assert back["loss_state"]["loss_normalizer"].dtype == torch.float64 and float(back["loss_state"]["loss_normalizer"]) == 87.5675678905675
    assert back["sampler"]["next_index"] == 10 and back["sampler"]["pending"] == [[7, int(drawn[0])], [8, int(drawn[1])], [9, int(drawn[2])]]
    assert torch.equal(back["sampler"]["flip_generator"], sampler.generator.get_state())
    assert sorted(back["momentum"]) == sorted(names)
    for name, p in zip(names, trainer.params):
        buf = trainer.opt.state.get(p, {}).get("momentum_buffer")
        assert torch.equal(back["momentum"][name], torch.zeros_like(p) if buf is None else buf), name
    other, omodel = _tiny_trainer(train_fpn=True)
    train_head.restore_trainer(other, back, path)
    assert other.iteration == 567 and omodel.loss_state.current_step == 567 and omodel.loss_state.draws == 567
    assert omodel.loss_state.loss_normalizer == 87.5675678905675
    assert other.lr == train_head.warmup_multistep_lr(567, **other.schedule) != trainer.schedule["base_lr"]
    for p, q in zip(other.params, trainer.params):
        want = trainer.opt.state.get(q, {}).get("momentum_buffer")
        assert torch.equal(other.opt.state[p]["momentum_buffer"], torch.zeros_like(q) if want is None else want)
    fresh = train_head.FrameSampler(4, random_flip=True, seed=0)
    assert fresh.load_state(back["sampler"]) == back["sampler"]["pending"] and fresh.next_index == 10
    assert [fresh.draw_flip() for _ in range(8)] == [sampler.draw_flip() for _ in range(8)]     # the draws continue where they stopped


def test_resume_refuses_what_does_not_fit_and_names_the_file(tmp_path):
    trainer, _ = _tiny_trainer(train_fpn=True)
    state = train_head.trainer_state(trainer)
    bare = str(tmp_path / "bare.pth")
    torch.save({"model": {}, "iteration": 3}, bare)
    with pytest.raises(SystemExit) as e:
        train_head.read_trainer_state(bare)
    assert bare in str(e.value) and "pod_trainer" in str(e.value)
    head_only, _ = _tiny_trainer()
    with pytest.raises(SystemExit) as e:                                   # another set of trained parts
        train_head.restore_trainer(head_only, state, "some.pth")
    assert "some.pth" in str(e.value) and "head + fpn" in str(e.value) and head_only.iteration == 0
    short = dict(state, momentum={k: v for k, v in state["momentum"].items() if k != "head.cls_score.bias"})
    with pytest.raises(SystemExit) as e:                                   # a name missing
        train_head.restore_trainer(trainer, short, "some.pth")
    assert "some.pth" in str(e.value) and "head.cls_score.bias" in str(e.value)
    bent = dict(state, momentum=dict(state["momentum"], **{"head.cls_score.bias": torch.zeros(64)}))
    with pytest.raises(SystemExit) as e:                                   # a shape that differs
        train_head.restore_trainer(trainer, bent, "some.pth")
    assert "some.pth" in str(e.value) and "(64,)" in str(e.value) and trainer.iteration == 0


def test_resume_on_a_checkpoint_without_trainer_state_is_refused_by_the_command(tmp_path):
    """The refusal comes before any model is built or GPU touched."""
    (tmp_path / "gt.json").write_text('{"images": [], "annotations": []}')
    out = tmp_path / "out"
    out.mkdir()
    torch.save({"model": {}, "iteration": 2}, str(out / "model_final.pth"))
    (out / "last_checkpoint").write_text("model_final.pth")
    with pytest.raises(SystemExit) as e:
        train_head.main(["--coco-json", str(tmp_path / "gt.json"), "--image-root", str(tmp_path), "--output-dir", str(out), "--resume"])
    assert str(out / "model_final.pth") in str(e.value) and "pod_trainer" in str(e.value)


def test_the_command_and_the_trainer_offer_the_new_switches_off_by_default(capsys):
    with pytest.raises(SystemExit) as e:
        train_head.main(["--help"])
    assert e.value.code == 0
    text = " ".join(capsys.readouterr().out.split())
    assert "--fused-step" in text and "--random-flip" in text and "--resume" in text
    params = inspect.signature(train_head.HeadTrainer.__init__).parameters
    assert params["fused_step"].default is False
    sig = inspect.signature(train_head.save_checkpoint).parameters
    assert sig["trainer"].default is None and sig["masters"].default is None
    trainer, _ = _tiny_trainer()
    assert trainer.fused is None and isinstance(trainer.opt, torch.optim.SGD)
    assert trainer.lr == train_head.warmup_multistep_lr(0, **trainer.schedule)
    assert not train_head.FrameSampler(4).draw_flip()                      # without --random-flip nothing is drawn
