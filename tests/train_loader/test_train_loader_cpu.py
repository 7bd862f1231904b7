"""The data plan of `train_head --train-loader` (pod_compare_amd/train_loader.py) without a GPU: order, size and flip draws, aspect-ratio
grouping, the filter, the ranks' slices, resume through a checkpoint round trip, the refusals -- and pod_train_batch_u8's (K31) argument
validation, which runs on the host before anything is enqueued."""
import ctypes
import json
import os

import pytest
import torch

from pod_compare_amd import build, config, data_parallel, hip, train_head, train_loader as tl
from pod_compare_amd.train_batch import fill_frame

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
WIDE, TALL = (720, 1280), (1280, 720)


def plan(sizes, indices=None, **kw):
    kw.setdefault("flip", False)
    return tl.TrainPlan(sizes, list(range(len(sizes))) if indices is None else indices, tl.PlanSettings(**kw))


def indices_of(p, batches):
    return [e.index for _ in range(batches) for e in p.next_batch()]


def test_order_is_training_samplers():
    g = torch.Generator().manual_seed(5)
    want = [int(i) for _ in range(3) for i in torch.randperm(7, generator=g)]
    assert indices_of(plan([WIDE] * 7, batch=1, seed=5), 21) == want
    assert len(set(want[:7])) == 7 and want[:7] != want[7:14]                      # a fresh permutation every pass
    # batches of 3 cut the concatenated stream without a boundary at the pass's end
    assert indices_of(plan([WIDE] * 7, batch=3, seed=5), 7) == want
    assert indices_of(plan([WIDE] * 7, batch=1, seed=5, shuffle=False), 21) == list(range(7)) * 3
    # the plan samples from the indices it is given
    assert sorted(set(indices_of(plan([WIDE] * 7, indices=[1, 4, 6], batch=1, seed=5), 12))) == [1, 4, 6]


def test_choice_draws_are_uniform_over_the_entries():
    p = plan([WIDE] * 4, batch=1, min_sizes=(640, 672, 704), seed=1)
    draws = [p.next_batch()[0].short_edge for _ in range(3000)]
    assert set(draws) == {640, 672, 704}
    for s in (640, 672, 704):                          # expectation 1000, standard deviation sqrt(3000 / 3 * 2 / 3) = 25.8
        assert 800 <= draws.count(s) <= 1200, (s, draws.count(s))
    again = plan([WIDE] * 4, batch=1, min_sizes=(640, 672, 704), seed=1)
    assert [again.next_batch()[0].short_edge for _ in range(300)] == draws[:300]
    other = plan([WIDE] * 4, batch=1, min_sizes=(640, 672, 704), seed=2)
    assert [other.next_batch()[0].short_edge for _ in range(300)] != draws[:300]


def test_range_draws_cover_min_to_max_inclusive():
    p = plan([WIDE] * 4, batch=1, min_sizes=(640, 800), sampling="range", seed=3)
    draws = [p.next_batch()[0].short_edge for _ in range(30000)]
    assert min(draws) == 640 and max(draws) == 800 and all(isinstance(d, int) for d in draws)
    assert len(set(draws)) == 161


def test_sizes_follow_resize_shortest_edge_and_the_cap():
    e = plan([WIDE], batch=1, min_sizes=(800,), max_size=1333).next_batch()[0]
    assert (e.short_edge, e.size) == (800, (750, 1333))
    assert plan([WIDE], batch=1, min_sizes=(720,), max_size=1333).next_batch()[0].size == (720, 1280)
    assert plan([TALL], batch=1, min_sizes=(640,), max_size=1333).next_batch()[0].size == (1138, 640)


def test_flip_draws_and_no_draw_without_a_choice():
    p = plan([WIDE] * 4, batch=1, flip=True, seed=9)
    flips = [p.next_batch()[0].flipped for _ in range(2000)]
    assert 900 <= sum(flips) <= 1100                   # p = 0.5: standard deviation 22
    # one entry and no flip: the draw generator is never touched
    q = plan([WIDE] * 4, batch=1, min_sizes=(720,), seed=9)
    before = q.draw_generator.get_state().clone()
    for _ in range(20):
        q.next_batch()
    assert torch.equal(q.draw_generator.get_state(), before)
    # size first, then flip: the first frame's draws are the generator's first two
    g = torch.Generator().manual_seed(9)
    size = (640, 672, 704)[int(torch.randint(0, 3, (), generator=g))]
    flipped = bool(torch.rand((), generator=g) < 0.5)
    e = plan([WIDE] * 4, batch=1, min_sizes=(640, 672, 704), flip=True, seed=9).next_batch()[0]
    assert (e.short_edge, e.flipped) == (size, flipped)


def test_aspect_ratio_grouping():
    sizes = [WIDE, WIDE, TALL, WIDE, TALL, TALL]       # wide, wide, tall, wide, tall, tall in file order
    p = plan(sizes, batch=2, shuffle=False)
    got = [[e.index for e in p.next_batch()] for _ in range(6)]
    # AspectRatioGroupedDataset: 0, 1 fill the wide bucket; 2 waits; 3 waits; 4 completes the tall one (2, 4); 5 waits; second pass: 0 completes
    # the wide one (3, 0); 1 waits; 2 completes the tall one (5, 2); 3 completes the wide one (1, 3); 4 waits, 5 completes (4, 5); 0, 1
    assert got == [[0, 1], [2, 4], [3, 0], [5, 2], [1, 3], [4, 5]]
    q = plan(sizes, batch=2, shuffle=False, grouping=False)
    assert [[e.index for e in q.next_batch()] for _ in range(4)] == [[0, 1], [2, 3], [4, 5], [0, 1]]
    # a square frame is not wide
    assert [e.index for e in plan([(64, 64), WIDE, TALL], batch=2, shuffle=False).next_batch()] == [0, 2]


def test_filter_drops_frames_without_usable_annotations():
    images = [{"id": 10 + i, "file_name": "%d.png" % i, "height": 8, "width": 8} for i in range(5)]
    anns = [{"image_id": 10, "category_id": 1, "iscrowd": 0}, {"image_id": 12, "category_id": 1, "iscrowd": 1},
            {"image_id": 13, "category_id": 99}, {"image_id": 14, "category_id": 99}, {"image_id": 14, "category_id": 2}]
    cat_map = {1: 0, 2: 1}
    kept = tl.planned_indices(images, anns, cat_map, True)
    assert kept == [0, 4]                              # 1: none, 2: only crowd, 3: only an unmapped category
    p = plan(tl.frame_sizes(images), indices=kept, batch=1, seed=2)
    assert set(indices_of(p, 40)) == {0, 4}
    assert tl.planned_indices(images, anns, cat_map, False) == [0, 1, 2, 3, 4]
    assert set(indices_of(plan(tl.frame_sizes(images), indices=[0, 1, 2, 3, 4], batch=1, seed=2), 40)) == {0, 1, 2, 3, 4}
    with pytest.raises(SystemExit, match="no frame to train on"):
        plan(tl.frame_sizes(images), indices=[])


@pytest.mark.parametrize("world", [1, 2, 4])
def test_rank_slices_partition_every_batch_in_order(world):
    p = plan([WIDE, TALL] * 5, batch=4, min_sizes=(640, 672), flip=True, seed=4)
    for _ in range(12):
        batch = p.next_batch()
        parts = [batch[slice(*data_parallel.rank_slice(4, r, world))] for r in range(world)]
        assert [e for part in parts for e in part] == batch and all(len(part) == 4 // world for part in parts)


@pytest.mark.parametrize("k,where", [(0, "start"), (3, "inside"), (2, "waiting"), (4, "boundary"), (9, "boundary"), (6, "waiting")])
def test_resume_continues_the_plan(k, where, tmp_path):
    # 9 frames of two aspects, batches of 2: a pass is no whole number of batches, so entries wait across checkpoints and passes
    sizes = [WIDE, TALL, WIDE, WIDE, TALL, WIDE, TALL, TALL, WIDE]
    kw = dict(batch=2, min_sizes=(640, 672, 704), flip=True, seed=11)
    whole = plan(sizes, **kw)
    want = [whole.next_batch() for _ in range(k + 50)]
    first = plan(sizes, **kw)
    assert [first.next_batch() for _ in range(k)] == want[:k]
    torch.save({"pod_trainer": {"sampler": first.state()}}, tmp_path / "s.pth")
    state = torch.load(tmp_path / "s.pth", weights_only=True)["pod_trainer"]["sampler"]
    assert {"start": state["position"] == 0, "inside": 0 < state["position"] < 9 and not state["waiting"], "waiting": len(state["waiting"]) == 1,
            "boundary": state["position"] == 9}[where], state
    assert state["kind"] == "train_loader" and set(state) == {"kind", "pass_generator", "draw_generator", "position", "passes", "emitted", "frames", "waiting"}
    second = plan(sizes, **kw)
    second.load_state(state)
    assert [second.next_batch() for _ in range(50)] == want[k:]
    # reading ahead does not move the plan
    third = plan(sizes, **kw)
    third.load_state(state)
    ahead = third.until_pass_end()
    assert ahead == want[k:k + len(ahead)] and len(ahead) >= 1 and third.state()["position"] == state["position"]
    assert [third.next_batch() for _ in range(5)] == want[k:k + 5]


def test_states_that_do_not_fit_are_refused():
    p = plan([WIDE] * 4, batch=2)
    s = p.state()
    with pytest.raises(ValueError):
        plan([WIDE] * 5, batch=2).load_state(s)
    with pytest.raises(ValueError):
        p.load_state(dict(s, kind="other"))
    with pytest.raises(ValueError):
        p.load_state(dict(s, waiting=[[0, 0, 800], [1, 0, 800]]))                   # a complete batch was never left waiting


def cfg_with(**inp):
    cfg = config.get_cfg()
    cfg.INPUT.merge_from_dict(inp)
    return cfg


def test_settings_and_their_refusals():
    cfg = config.get_cfg()
    assert tuple(cfg.INPUT.MIN_SIZE_TRAIN) == (800,) and cfg.INPUT.MAX_SIZE_TRAIN == 1333 and cfg.INPUT.MIN_SIZE_TRAIN_SAMPLING == "choice"
    assert cfg.INPUT.RANDOM_FLIP == "horizontal" and cfg.DATALOADER.ASPECT_RATIO_GROUPING is True and cfg.DATALOADER.FILTER_EMPTY_ANNOTATIONS is True
    bdd = config.setup_config(os.path.join(ROOT, "pod_compare_amd/configs/BDD-Detection/retinanet/retinanet_R_50_FPN_1x.yaml"))
    assert list(bdd.INPUT.MIN_SIZE_TRAIN) == [720]
    s = tl.plan_settings(bdd, seed=3)
    assert (s.batch, s.min_sizes, s.sampling, s.max_size, s.flip, s.grouping, s.filter_empty, s.shuffle, s.seed) == \
        (4, (720,), "choice", 1333, True, True, True, True, 3)
    assert tl.plan_settings(cfg_with(RANDOM_FLIP="none")).flip is False and tl.plan_settings(cfg_with(RANDOM_FLIP="none"), random_flip=True).flip is True
    for bad, key in ((dict(RANDOM_FLIP="vertical"), "INPUT.RANDOM_FLIP"), (dict(MIN_SIZE_TRAIN_SAMPLING="range", MIN_SIZE_TRAIN=[640, 672, 704]), "INPUT.MIN_SIZE_TRAIN"),
                     (dict(MIN_SIZE_TRAIN_SAMPLING="sometimes"), "INPUT.MIN_SIZE_TRAIN_SAMPLING"), (dict(MIN_SIZE_TRAIN=[]), "INPUT.MIN_SIZE_TRAIN")):
        with pytest.raises(SystemExit, match=key):
            tl.plan_settings(cfg_with(**bad))


def main_exit(tmp_path, yaml_text, images, *flags, checkpoint=None) -> str:
    """train_head.main on a machine without a GPU: the SystemExit's text, or what it failed on later (past the checks)."""
    (tmp_path / "m.yaml").write_text(yaml_text)
    (tmp_path / "gt.json").write_text(json.dumps({"images": images, "annotations": [{"image_id": 1, "category_id": 1, "bbox": [1, 1, 4, 4], "iscrowd": 0}]}))
    out = tmp_path / "out"
    if checkpoint is not None:
        out.mkdir(exist_ok=True)
        torch.save({"model": {}, "pod_trainer": checkpoint}, out / "model_final.pth")
        (out / "last_checkpoint").write_text("model_final.pth")
    built = []
    real = train_head.build_model
    train_head.build_model = lambda *a, **k: built.append(1) or real(*a, **k)
    try:
        train_head.main(["--config-file", str(tmp_path / "m.yaml"), "--coco-json", str(tmp_path / "gt.json"), "--image-root", str(tmp_path), "--device", "cpu",
                         "--random-init", "--max-iter", "0", "--output-dir", str(out)] + list(flags))
    except SystemExit as e:
        assert not built, "refused only after a model was built"
        return str(e)
    except Exception as e:
        return "%s: %s" % (type(e).__name__, e)
    finally:
        train_head.build_model = real
    return ""


GOOD = [{"id": 1, "file_name": "a.png", "height": 64, "width": 96}]


def test_the_command_refuses_before_a_model_is_built(tmp_path):
    said = main_exit(tmp_path, "INPUT:\n  RANDOM_FLIP: vertical\n", GOOD, "--train-loader")
    assert "INPUT.RANDOM_FLIP" in said and "vertical" in said
    said = main_exit(tmp_path, "INPUT:\n  MIN_SIZE_TRAIN_SAMPLING: range\n  MIN_SIZE_TRAIN: [640, 672, 704]\n", GOOD, "--train-loader")
    assert "INPUT.MIN_SIZE_TRAIN" in said and "range" in said
    said = main_exit(tmp_path, "INPUT:\n  MIN_SIZE_TRAIN_SAMPLING: weekly\n", GOOD, "--train-loader")
    assert "INPUT.MIN_SIZE_TRAIN_SAMPLING" in said and "weekly" in said
    said = main_exit(tmp_path, "SEED: 0\n", [{"id": 1, "file_name": "a.png", "width": 96}], "--train-loader")
    assert "`height` / `width`" in said and "a.png" in said
    assert "belong to --train-loader" in main_exit(tmp_path, "SEED: 0\n", GOOD, "--batch-on-gpu")
    # without the flag none of the keys is read: the same configs get past these checks
    assert "INPUT." not in main_exit(tmp_path, "INPUT:\n  RANDOM_FLIP: vertical\n", GOOD)


def test_resume_across_kinds_is_refused(tmp_path):
    old = {"trained": ["head"], "sampler": train_head.FrameSampler(1).state()}
    new = {"trained": ["head"], "sampler": plan([WIDE], batch=1).state()}
    said = main_exit(tmp_path, "SEED: 0\n", GOOD, "--train-loader", "--resume", checkpoint=old)
    assert "model_final.pth" in said and "`frame_sampler`" in said and "`train_loader`" in said
    said = main_exit(tmp_path, "SEED: 0\n", GOOD, "--resume", checkpoint=new)
    assert "model_final.pth" in said and "`frame_sampler`" in said and "`train_loader`" in said
    assert set(train_head.FrameSampler(1).state()) == {"next_index", "pending", "flip_generator"}       # without the flag: exactly its three keys


def test_abi_and_build_list():
    header = open(os.path.join(ROOT, "include", "pod_mi355x.h")).read()
    assert hip.POD_ABI_VERSION == 18 and "#define POD_ABI_VERSION 18\n" in header and "#define POD_TRAIN_BATCH_MAX_FRAMES 64\n" in header
    assert "k31_train_batch.hip" in build.SOURCES and any(h.endswith("pod_resize_u8.h") for h in build.HEADERS)
    lib = hip.load()
    assert lib.pod_abi_version() == hip.POD_ABI_VERSION and hasattr(lib, "pod_train_batch_u8") and hasattr(lib, "pod_train_batch_tiles")
    assert ctypes.sizeof(hip.PodTrainFrame) == 104 and hip.PodTrainFrame.first_tile.offset == 96 and hip.PodTrainFrame.dst.offset == 72


def test_struct_layout_matches_c(tmp_path):
    import subprocess
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "pod_mi355x.h"\n'
                   'int main(void){printf("%zu %zu %zu %zu %zu %zu %zu\\n", sizeof(PodTrainFrame), offsetof(PodTrainFrame, row_stride), offsetof(PodTrainFrame, xk),'
                   ' offsetof(PodTrainFrame, ybounds), offsetof(PodTrainFrame, dst), offsetof(PodTrainFrame, hflip), offsetof(PodTrainFrame, first_tile)); return 0;}\n')
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "layout")])
    got = [int(x) for x in subprocess.check_output([str(tmp_path / "layout")]).split()]
    T = hip.PodTrainFrame
    assert got == [ctypes.sizeof(T), T.row_stride.offset, T.xk.offset, T.ybounds.offset, T.dst.offset, T.hflip.offset, T.first_tile.offset]


def test_train_batch_refusals_without_a_gpu():
    """Every case pod_train_batch_u8 refuses returns POD_E_INVALID before anything is enqueued: the pointers below are never followed."""
    lib = hip.load()
    T, DEV = 0x100000, 0x900000                        # tables, the device copy of the launch table
    xk, yk = lib.pod_resize_taps(8, 9), lib.pod_resize_taps(5, 7)

    def table(n=2, **kw):
        t = (hip.PodTrainFrame * hip.POD_TRAIN_BATCH_MAX_FRAMES)()
        first = 0
        for i in range(n):
            a = dict(src=0x10000 + 0x1000 * i, in_h=5, in_w=8, stride=24, xt=(T, T, xk), yt=(T, T, yk), dst=0x40000 + 0x1000 * i, out_h=7, out_w=9,
                     first=first)
            a.update({k[:-1]: v for k, v in kw.items() if k.endswith(str(i))})
            first = fill_frame(t[i], a["src"], a["in_h"], a["in_w"], a["stride"], a["xt"], a["yt"], a["dst"], a["out_h"], a["out_w"], True, i == 1, a["first"])
        return t, first

    def call(n=2, tiles=None, frames_dev=DEV, **kw):
        t, total = table(n, **kw)
        return lib.pod_train_batch_u8(t, frames_dev, n, total if tiles is None else tiles, None)

    t, total = table()
    assert total == 4 and lib.pod_train_batch_tiles(t, 2) == 4 and lib.pod_train_batch_tiles(t, 1) == 2
    assert lib.pod_train_batch_tiles(None, 2) == -1 and lib.pod_train_batch_tiles(t, 0) == -1 and lib.pod_train_batch_tiles(t, 65) == -1
    assert lib.pod_train_batch_u8(None, DEV, 2, 4, None) == -1 and call(frames_dev=None) == -1                # NULL tables
    assert lib.pod_train_batch_u8(t, DEV, 0, 4, None) == -1 and lib.pod_train_batch_u8(t, DEV, 65, 4, None) == -1 and lib.pod_train_batch_u8(t, DEV, -1, 4, None) == -1
    big = hip.POD_RESIZE_MAX_SIDE + 1
    for bad in (dict(src1=None), dict(dst0=None), dict(in_h1=0), dict(in_w0=big), dict(out_h1=0), dict(out_w1=big), dict(stride1=23),
                dict(xt0=(None, T, xk)), dict(yt1=(T, None, yk)),                    # half a table
                dict(xt1=(None, None, 0)), dict(yt0=(None, None, 0)),                # no table, but the size changes
                dict(xt0=(T, T, xk + 2)), dict(yt1=(T, T, 2)),                       # not the geometry's tap count
                dict(first1=1), dict(first1=3), dict(first0=1),                      # a first_tile sequence other than the sizes give
                dict(dst1=0x40000), dict(dst1=0x40000 + 3 * 7 * 9 - 1),              # two outputs that overlap
                dict(dst0=0x10000 + 0x1000 + 5 * 24 - 1), dict(src1=0x40000 + 10)):  # an output that overlaps a source (another frame's, its own)
        assert call(**bad) == -1, bad
    assert call(tiles=3) == -1 and call(tiles=5) == -1 and call(tiles=0) == -1          # n_tiles other than the sizes give
