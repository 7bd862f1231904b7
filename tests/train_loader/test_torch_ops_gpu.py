"""K31 (csrc/k31_train_batch.hip) on the GPU against Pillow, to the byte, and mixed-size batches through the training paths: a frame run
against a larger padded size is the forward of the zero-padded normalised frame; the whole ResNet's gradients on a batch of two frame
sizes against the fp64 replica; a batch of one shape gives the bits it gave without a common padded size.

The module shares its name with tests/test_torch_ops_gpu.py so that the GPU run order in tests/conftest.py (GPU_ORDER, keyed by module
name) gives it a place."""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from PIL import Image

import pod_compare_amd.torch_ops  # noqa: F401  (registers torch.ops.pod_mi355x)
from pod_compare_amd import fpn_train, hip, resize, resnet_train, train_batch, train_head
from pod_compare_amd.resnet_train import resnet_forward_train, stem_forward_train, trainable_blocks, trainable_convs, unfolded_pairs
from tests.head_backward import hb
from tests.loader.test_resize_cpu import frame, tables
from tests.resnet_backward import rb
from tests.resnet_backward import test_torch_ops_gpu as resnet_tests
from tests.stem_backward import sb

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# (h, w) -> (nh, nw), hflip, flip_channels, padded source rows: all four combinations of the two flips; an output narrower than a tile;
# one axis only, crossing the 64-column tile edge; no resize; two sources with padded rows
SIX = ((((72, 128), (75, 120)), True, True, False), (((64, 97), (19, 29)), False, True, True), (((5, 7), (11, 3)), True, False, False),
       (((40, 40), (40, 67)), True, True, True), (((50, 64), (50, 64)), False, False, False), (((90, 160), (29, 160)), True, False, False))


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _pillow(f, new, hflip, flipc):
    h, w = f.shape[:2]
    im = Image.fromarray(f)
    if new != (h, w):
        im = im.resize((new[1], new[0]), Image.BILINEAR)
    a = np.asarray(im)
    if hflip:
        a = a[:, ::-1]
    if flipc:
        a = a[:, :, ::-1]
    return torch.from_numpy(np.ascontiguousarray(a.transpose(2, 0, 1)))


def _launch(specs, seed):
    """One pod_train_batch_u8 launch over `specs`; returns (outputs on the CPU, the Pillow referees).  128 guard bytes around every output."""
    rng = np.random.default_rng(seed)
    n = len(specs)
    table = (hip.PodTrainFrame * hip.POD_TRAIN_BATCH_MAX_FRAMES)()
    table_dev = torch.zeros(104 * hip.POD_TRAIN_BATCH_MAX_FRAMES, dtype=torch.uint8, device=DEV)
    keep, bufs, outs, want, first, cache = [], [], [], [], 0, {}
    for i, ((hw, new), hflip, flipc, padded_rows) in enumerate(specs):
        h, w = hw
        f = frame(rng, h, w)
        if padded_rows:
            rows = torch.full((h, 3 * w + 13), 201, dtype=torch.uint8, device=DEV)          # rows 13 bytes apart from one another
            rows[:, :3 * w] = _dev(f).reshape(h, 3 * w)
            src = rows[:, :3 * w].unflatten(1, (w, 3))
        else:
            src = _dev(f)
        tabs = []
        for a, b in ((w, new[1]), (h, new[0])):
            if a == b:
                tabs.append((None, None, 0))
            else:
                if (a, b) not in cache:
                    bounds, coeffs = tables(a, b)
                    cache[(a, b)] = (_dev(bounds), _dev(coeffs), coeffs.shape[1])
                t = cache[(a, b)]
                tabs.append((t[0].data_ptr(), t[1].data_ptr(), t[2]))
        buf = torch.full((3 * new[0] * new[1] + 256,), 77, dtype=torch.uint8, device=DEV)
        out = buf[128:128 + 3 * new[0] * new[1]].view(3, new[0], new[1])
        first = train_batch.fill_frame(table[i], src.data_ptr(), h, w, src.stride(0), tabs[0], tabs[1], out.data_ptr(), new[0], new[1], flipc, hflip, first)
        keep.append(src)
        bufs.append(buf)
        outs.append(out)
        want.append(_pillow(f, new, hflip, flipc))
    assert hip.load().pod_train_batch_tiles(table, n) == first
    torch.cuda.synchronize()
    assert hip.load().pod_train_batch_u8(table, table_dev.data_ptr(), n, first, hip.current_stream()) == 0
    torch.cuda.synchronize()
    for buf in bufs:
        assert bool((buf[:128] == 77).all()) and bool((buf[-128:] == 77).all())
    return [o.cpu() for o in outs], want


def test_six_geometries_in_one_launch_equal_pillow():
    assert {(s[1], s[2]) for s in SIX} == {(True, True), (True, False), (False, True), (False, False)} and sum(s[3] for s in SIX) == 2
    got, want = _launch(SIX, seed=1)
    for i, (g, w) in enumerate(zip(got, want)):
        assert torch.equal(g, w), SIX[i]


def test_one_frame_and_sixty_four_frames():
    for spec in SIX[:3]:
        got, want = _launch([spec], seed=2)
        assert torch.equal(got[0], want[0]), spec
    many = [(((5, 7), (11, 3)), bool(i & 1), bool(i & 2), bool(i % 5 == 0)) for i in range(hip.POD_TRAIN_BATCH_MAX_FRAMES)]
    got, want = _launch(many, seed=3)
    assert len(got) == 64 and all(torch.equal(g, w) for g, w in zip(got, want))


def test_a_bdd_frame_and_the_wrapper_equal_k20_and_a_flip():
    spec = (((720, 1280), (640, 1138)), True, True, False)
    got, want = _launch([spec], seed=4)
    assert torch.equal(got[0], want[0])
    # the wrapper (its own tables, launch table and outputs) and the registered op against K20 followed by .flip(-1), on the device
    rng = np.random.default_rng(5)
    frames = [_dev(frame(rng, 720, 1280)), _dev(frame(rng, 72, 128)), _dev(frame(rng, 128, 72)), _dev(frame(rng, 64, 96))]
    edges, flips = [(640, 1333), (80, 120), (80, 120), (64, 96)], [True, False, True, True]
    k20 = [resize.resize_frame_u8(f, lo, hi) for f, (lo, hi) in zip(frames, edges)]
    k20 = [t.flip(-1) if fl else t for t, fl in zip(k20, flips)]
    sizes = [tuple(t.shape[1:]) for t in k20]
    assert sizes[0] == (640, 1138) and sizes[3] == (64, 96)
    for round_ in range(3):                              # three launches: both pinned tables and the event guarding the first are used
        outs = train_batch.train_batch_u8(frames, sizes, flips)
        assert all(o.is_contiguous() and torch.equal(o, k) for o, k in zip(outs, k20)), round_
    ops = torch.ops.pod_mi355x.train_batch_u8(frames, [v for s in sizes for v in s], flips)
    assert all(torch.equal(o, k) for o, k in zip(ops, k20))
    rgb = train_batch.train_batch_u8(frames[1:2], sizes[1:2], [False], bgr=False)[0]
    assert torch.equal(rgb, k20[1].flip(0))
    with pytest.raises(hip.PodError):
        train_batch.train_batch_u8(frames[:1], sizes[:1], [True], outs=[frames[0].view(-1)[:3 * 640 * 1138].view(3, 640, 1138)])      # an output on its source


def test_the_axis_table_cache_is_bounded():
    f = _dev(frame(np.random.default_rng(6), 60, 90))
    old, train_batch.MAX_AXIS_TABLES = train_batch.MAX_AXIS_TABLES, 6
    torch.cuda.synchronize()
    train_batch._axis_tables.clear()
    try:
        for k in range(9):
            size = (40 + k, 61 + k)
            got = train_batch.train_batch_u8([f, f], [size, (60, 90)], [bool(k & 1), True])
            assert torch.equal(got[0].cpu(), _pillow(f.cpu().numpy(), size, bool(k & 1), True)) and torch.equal(got[1], f.permute(2, 0, 1).flip(0).flip(-1))
            assert len(train_batch._axis_tables) <= 6
    finally:
        train_batch.MAX_AXIS_TABLES = old


# ---- mixed-size batches ------------------------------------------------------------------------------------------------------------------
PADDED = (64, 96)


def mixed_frames():
    g = torch.Generator().manual_seed(16)
    return [torch.randint(0, 256, (3, 64, 96), generator=g, dtype=torch.uint8).to(DEV), torch.randint(0, 256, (3, 37, 70), generator=g, dtype=torch.uint8).to(DEV)]


@pytest.fixture(scope="module")
def models():
    return resnet_tests.make_models()


@pytest.fixture(scope="module")
def reference64(models):
    """The unfolded CPU model in fp64 on each frame, normalised and zero-padded to (64, 96): pool, res2, c3 - c5 and the five FPN maps."""
    model, shadow = models
    ref = copy.deepcopy(shadow).double()
    out = []
    with torch.no_grad():
        for im in mixed_frames():
            xn = sb.normalised_padded(im.cpu().unsqueeze(0), model.pixel_mean.reshape(3).cpu(), model.pixel_std.reshape(3).cpu(), PADDED, torch.float64)
            pool = F.max_pool2d(torch.relu(ref.bottom_up.stem(xn)), 3, 2, 1)
            res2 = ref.bottom_up.res2(pool)
            c = ref.bottom_up(xn)
            out.append({"pool": pool, "res2": res2, "c": list(c), "p": list(ref.fpn(c))})
    return out


def _planes(t, h, w):
    return sb.to_planes(t, h, w).double()


@pytest.mark.parametrize("which", [0, 1], ids=["64x96", "37x70"])
def test_a_frame_against_a_larger_padded_size_is_the_same_forward(models, reference64, which):
    model, _ = models
    im, want = mixed_frames()[which], reference64[which]
    with torch.no_grad():
        feats, pad = model._trunk_eager(im, padded=PADDED)
        t2, h2, w2 = resnet_train.res2_maps(model, im, padded=PADDED)
        tp, hp, wp = resnet_train.pool_maps(model, im, padded=PADDED)
        maps, pad2 = fpn_train.backbone_maps(model, im, padded=PADDED)
    assert tuple(pad) == tuple(pad2) == PADDED and (h2, w2) == (hp, wp) == (16, 24) and [m[1:] for m in maps] == [(8, 12), (4, 6), (2, 3)]
    errs = {"pool": hb.rel_err(_planes(tp, hp, wp), want["pool"]), "res2": hb.rel_err(_planes(t2, h2, w2), want["res2"])}
    for k, ((t, h, w), c) in enumerate(zip(maps, want["c"])):
        errs["c%d" % (k + 3)] = hb.rel_err(_planes(t, h, w), c)
    for k, (f, p) in enumerate(zip(feats, want["p"])):
        assert tuple(f.shape) == tuple(p.shape)
        errs["p%d" % (k + 3)] = hb.rel_err(f, p)
    print("TL_PADDED %s %s" % (tuple(im.shape[1:]), "  ".join("%s %.2e" % kv for kv in errs.items())))
    assert all(e <= hb.BAR for e in errs.values()), errs
    if which == 0:                                       # its own padded size, passed explicitly: the call without `padded=`, to the bit
        with torch.no_grad():
            plain = model._trunk_eager(im)
            assert tuple(plain[1]) == PADDED and all(torch.equal(a, b) for a, b in zip(plain[0], feats))
            assert torch.equal(resnet_train.res2_maps(model, im)[0], t2) and torch.equal(resnet_train.pool_maps(model, im)[0], tp)
            assert all(torch.equal(a[0], b[0]) for a, b in zip(fpn_train.backbone_maps(model, im)[0], maps))
    else:                                                # without a common size the frame pads to its own (64, 96) here too; a size that does not hold it is refused
        for bad in ((32, 96), (64, 64), (64, 100)):
            with pytest.raises(ValueError):
                model._trunk_eager(im, padded=bad)


def test_a_mixed_batchs_resnet_gradients_match_the_fp64_replica():
    """Frames of 64 x 96 and 37 x 70 against the padded size (64, 96), FREEZE_AT 0: all 53 weight gradients of the ResNet -- the stem's,
    which is K30 once per image added in image order, among them -- through hb.Checker against the fp64 replica under the GPU's own gates
    and pool routing (tests/stem_backward/test_torch_ops_gpu.py's construction, split at the ResNet's outputs as there)."""
    model, shadow = resnet_tests.make_models()
    net, ref_net = model.bottom_up, shadow.bottom_up
    for q in model.parameters():
        q.grad = None
    images = mixed_frames()
    B = len(images)
    with pytest.raises(hip.PodError):                    # without a common size a batch holds one shape
        stem_forward_train(model, images)
    g = torch.Generator().manual_seed(62)
    hw, ch = [(8, 12), (4, 6), (2, 3)], (512, 1024, 2048)
    net.train_tap = {}
    try:
        outs = resnet_forward_train(net, stem_forward_train(model, images, padded=PADDED), 0)
        assert [o[1:] for o in outs[0]] == hw and [o[1:] for o in outs[1]] == hw
        with torch.no_grad():                            # the training forward IS the inference forward against that size
            for b in range(B):
                fr = (images[b], model.pixel_mean.reshape(3), model.pixel_std.reshape(3), PADDED)
                for (t, _, _), (r, _, _) in zip(outs[b], net.forward_cl(None, frame=fr)):
                    assert torch.equal(t.detach(), r)
        cot = [torch.randn((B, c, h, w), generator=g) for c, (h, w) in zip(ch, hw)]
        torch.autograd.backward([outs[b][s][0] for b in range(B) for s in range(3)], [resnet_tests._cl_rows(cot[s])[b] for b in range(B) for s in range(3)])
        tap = net.train_tap
    finally:
        del net.train_tap
    got = [c.weight.grad for c in trainable_convs(net, 0)]
    assert len(got) == 53 and all(x is not None and bool(torch.isfinite(x).all()) for x in got)
    kept, (h, w) = tap["stem"]
    s_gpu = torch.cat([sb.to_planes(t, h, w) for t in kept])
    masks = rb.masks_from_tap(tap, B)
    mean, std = model.pixel_mean.reshape(3).cpu(), model.pixel_std.reshape(3).cpu()
    ref = {}
    for dtype in (torch.float32, torch.float64):
        (stem,) = rb.in_dtype([ref_net.stem], dtype)
        blocks = rb.in_dtype(trainable_blocks(ref_net, 0), dtype)
        xn = torch.cat([sb.normalised_padded(im.cpu().unsqueeze(0), mean, std, PADDED, dtype) for im in images])
        ys = rb.replica_forward(blocks, sb.replica_stem((stem[0], stem[1]), xn, s_gpu), masks)
        torch.autograd.backward([ys[i] for i in (6, 12, 15)], [c.to(dtype) for c in cot])
        ref[dtype] = [stem[0].weight.grad] + [c.weight.grad for c, _ in rb.pair_list(blocks)]
    names = ["stem"] + rb.conv_names(trainable_blocks(ref_net, 0))
    chk = hb.Checker()
    for name, a, (_, bn), b32, b64 in zip(names, got, unfolded_pairs(ref_net, 0), ref[torch.float32], ref[torch.float64]):
        chk.add("mixed " + name, rb.unfolded_grad(a, bn), b32, b64)
    chk.finish()


def _boxes():
    gb = [torch.tensor([[10., 8., 44., 40.], [50., 20., 90., 60.]]), torch.tensor([[4., 5., 30., 33.], [36., 10., 66., 30.]])]
    return gb, [torch.tensor([1, 4]), torch.tensor([2, 6])]


@pytest.mark.parametrize("route", ["head", "fpn", "freeze2", "freeze1", "freeze0"])
def test_a_mixed_batch_steps_on_every_route(route):
    """Two boxes per frame: stem -> ResNet -> FPN -> head -> losses -> backward() and one step, finite, on all four routes of
    HeadTrainer.features (the backbone's three freeze points counted apart)."""
    model, shadow = resnet_tests.make_models()
    kw = {"head": {}, "fpn": dict(train_fpn=True)}.get(route) if route in ("head", "fpn") else dict(train_backbone=True, shadow=shadow, freeze_at=int(route[-1]))
    trainer = train_head.HeadTrainer(model, base_lr=0.01, warmup_iters=0, steps=(1000, 2000), **kw)
    images = mixed_frames()
    gb, gc = _boxes()
    if route == "freeze0":
        with pytest.raises(hip.PodError):                # the stem's backward stacks the frames of a batch that names no common size
            trainer.features(images)
    before = [p.detach().clone() for p in trainer.params]
    feats, padded = trainer.features(images, padded=PADDED)
    assert tuple(padded) == PADDED and all(int(f.shape[0]) == 2 for f in feats)
    res = trainer.step(feats, padded, PADDED, gb, gc)
    assert bool(torch.isfinite(res["loss_cls"])) and bool(torch.isfinite(res["loss_box_reg"]))
    moved = [not torch.equal(p.detach(), b) for p, b in zip(trainer.params, before) if p.dim() > 1]          # every filter
    assert all(bool(torch.isfinite(p).all()) for p in trainer.params) and all(moved), moved.count(False)


@pytest.mark.parametrize("freeze_at", [2, 0])
def test_one_shape_gives_the_same_bits_with_and_without_the_common_size(freeze_at):
    from tests.fpn_backward import test_torch_ops_gpu as fpn_tests
    images, gb, gc = fpn_tests.batch()
    ends = []
    for padded in (None, PADDED):
        model, shadow = resnet_tests.make_models()
        trainer = train_head.HeadTrainer(model, base_lr=0.01, warmup_iters=0, steps=(1000, 2000), train_backbone=True, shadow=shadow, freeze_at=freeze_at)
        feats, pad = trainer.features(images) if padded is None else trainer.features(images, padded=padded)
        trainer.step(feats, pad, (64, 96), gb, gc)
        ends.append([p.detach().clone() for p in trainer.params] + [c.weight.detach().clone() for c in trainer.masters.convs])
    assert len(ends[0]) == len(ends[1]) and all(torch.equal(a, b) for a, b in zip(*ends))
