"""MODEL.BACKBONE.FREEZE_AT 1 and 0 end to end (pod_compare_amd/resnet_train.py, train_head.py): res2's three blocks as a chain, the whole
ResNet from the frames down to the stem's filter against an fp64 replica under the GPU's own gates and pool routing, one trainer step per
freeze point with its checkpoint, the fused step against torch's, the momentum state.  The folded filters' gradients are compared as what
the optimiser is handed, s dW'.  Measured figures: profiles/stem_backward.md."""
import copy

import pytest
import torch

from pod_compare_amd import checkpoint, modeling, train_head
from pod_compare_amd.resnet_train import (block_convs, blocks_forward_train, resnet_forward_train, stem_forward_train, trainable_blocks, trainable_convs,
                                          unfolded_pairs)
from tests.fpn_backward import test_torch_ops_gpu as fpn_tests
from tests.head_backward import hb
from tests.optimizer_step.test_torch_ops_gpu import U, f32
from tests.resnet_backward import rb
from tests.resnet_backward import test_torch_ops_gpu as resnet_tests
from tests.stem_backward import sb

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B = 2


def _clear(net):
    for q in net.parameters():
        q.grad = None


# ---- 4. res2 as a chain -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def nets():
    return rb.make_resnet(0, DEV)


def test_res2_as_a_chain_matches_autograd_and_stops_above_an_input_that_needs_no_gradient(nets):
    """res2's three blocks (the first with the stride-1 conv shortcut) on 16 x 24 maps of 64 channels: all 10 weight gradients and dX against
    the unfolded blocks' autograd under the GPU's own gates; then the same chain on an input that requires no gradient."""
    folded, shadow = nets
    blocks, ref_blocks = list(folded.res2), list(shadow.res2)
    h, w = 16, 24
    g = torch.Generator().manual_seed(51)
    planes = torch.relu(torch.randn((B, 64, h, w), generator=g))
    cot = torch.randn((B, 256, h, w), generator=g)
    got = {}
    for needs in (True, False):
        _clear(folded)
        maps, tap = resnet_tests._maps(planes, requires_grad=needs), {}
        outs = blocks_forward_train(blocks, maps, tap=tap)
        assert all(len(o) == 1 and o[0][1:] == (h, w) and o[0][0].grad_fn is not None for o in outs)
        torch.autograd.backward([o[0][0] for o in outs], resnet_tests._cl_rows(cot))
        got[needs] = [c.weight.grad.clone() for blk in blocks for c in block_convs(blk)]
        if needs:
            got_x, masks = torch.cat([m[0].grad for m in maps]), rb.masks_from_tap(tap, B)
        else:
            assert all(m[0].grad is None for m in maps) and (0, "a") in tap["dz"] and len(tap["dz"]) == 9
    assert len(got[True]) == 10 and all(torch.equal(a, b) for a, b in zip(got[True], got[False]))
    ref = {}
    for dtype in (torch.float32, torch.float64):
        rblocks = rb.in_dtype(ref_blocks, dtype)
        x = planes.to(dtype).clone().requires_grad_(True)
        ys = rb.replica_forward(rblocks, x, masks)
        if dtype == torch.float64:
            assert hb.rel_err(torch.cat([o[0][0] for o in outs]), rb.to_cl(ys[-1].detach())) <= hb.BAR
        ys[-1].backward(cot.to(dtype))
        ref[dtype] = [c.weight.grad for c, _ in rb.pair_list(rblocks)] + [rb.to_cl(x.grad)]
    chk = hb.Checker()
    for name, a, (_, bn), b32, b64 in zip(rb.conv_names(ref_blocks), got[True], rb.pair_list(ref_blocks), ref[torch.float32], ref[torch.float64]):
        chk.add("res2 " + name, rb.unfolded_grad(a, bn), b32, b64)
    chk.add("res2 dX", got_x, ref[torch.float32][-1], ref[torch.float64][-1])
    chk.finish()


# ---- 5. the whole ResNet ----------------------------------------------------------------------------------------------------------------
def test_the_whole_resnet_at_freeze_point_0_matches_the_fp64_replica():
    """B = 2 frames of 64 x 96, uint8, normalised on load: all 53 weight gradients (stem 1 + res2 10 + res3 - res5 42) through hb.Checker.
    The replica takes every ReLU gate and the pool's arg-max routing from the GPU's stored activations, so it is the linear map the GPU
    differentiates; the fp32 referee is the same replica in fp32."""
    model, shadow = resnet_tests.make_models()
    net, ref_net = model.bottom_up, shadow.bottom_up
    _clear(model)
    images, _, _ = fpn_tests.batch()
    g = torch.Generator().manual_seed(61)
    hw, ch = [(8, 12), (4, 6), (2, 3)], (512, 1024, 2048)
    net.train_tap = {}
    try:
        outs = resnet_forward_train(net, stem_forward_train(model, images), 0)
        assert [o[1:] for o in outs[0]] == hw and all(t.grad_fn is not None for o in outs for t, _, _ in o)
        with torch.no_grad():                            # the training forward IS the inference forward
            for b in range(B):
                frame = (images[b], model.pixel_mean.reshape(3), model.pixel_std.reshape(3), (64, 96))
                for (t, _, _), (r, _, _) in zip(outs[b], net.forward_cl(None, frame=frame)):
                    assert torch.equal(t.detach(), r)
        cot = [torch.randn((B, c, h, w), generator=g) for c, (h, w) in zip(ch, hw)]
        torch.autograd.backward([outs[b][s][0] for b in range(B) for s in range(3)], [resnet_tests._cl_rows(cot[s])[b] for b in range(B) for s in range(3)])
        tap = net.train_tap
    finally:
        del net.train_tap
    convs = trainable_convs(net, 0)
    got = [c.weight.grad for c in convs]
    assert len(got) == 53 and all(x is not None and bool(torch.isfinite(x).all()) for x in got)
    kept, (h, w) = tap["stem"]
    s_gpu = torch.cat([sb.to_planes(t, h, w) for t in kept])
    masks = rb.masks_from_tap(tap, B)
    assert (h, w) == (32, 48) and len(tap["saved"][0]) == 16
    frames = torch.stack([im.cpu() for im in images])
    ref = {}
    for dtype in (torch.float32, torch.float64):
        (stem,) = rb.in_dtype([ref_net.stem], dtype)
        blocks = rb.in_dtype(trainable_blocks(ref_net, 0), dtype)
        xn = sb.normalised_padded(frames, model.pixel_mean.reshape(3).cpu(), model.pixel_std.reshape(3).cpu(), (64, 96), dtype)
        ys = rb.replica_forward(blocks, sb.replica_stem((stem[0], stem[1]), xn, s_gpu), masks)
        torch.autograd.backward([ys[i] for i in (6, 12, 15)], [c.to(dtype) for c in cot])
        ref[dtype] = [stem[0].weight.grad] + [c.weight.grad for c, _ in rb.pair_list(blocks)]
    pairs = unfolded_pairs(ref_net, 0)
    names = ["stem"] + rb.conv_names(trainable_blocks(ref_net, 0))
    chk = hb.Checker()
    for name, a, (_, bn), b32, b64 in zip(names, got, pairs, ref[torch.float32], ref[torch.float64]):
        chk.add("freeze0 " + name, rb.unfolded_grad(a, bn), b32, b64)
    chk.finish()


# ---- 6. one trainer step per freeze point -----------------------------------------------------------------------------------------------
def _forward_c3_c5(model, image):
    with torch.no_grad():
        frame = (image, model.pixel_mean.reshape(3), model.pixel_std.reshape(3), (64, 96))
        return [t.clone() for t, _, _ in model.bottom_up.forward_cl(None, frame=frame)]


@pytest.mark.parametrize("freeze_at", [2, 1, 0])
def test_one_step_moves_what_the_freeze_point_lets_move(freeze_at, tmp_path):
    model, shadow = resnet_tests.make_models()
    images, gb, gc = fpn_tests.batch()
    trainer = train_head.HeadTrainer(model, base_lr=0.01, warmup_iters=0, steps=(1000, 2000), train_backbone=True, shadow=shadow, freeze_at=freeze_at)
    net = model.bottom_up
    convs = trainable_convs(net, freeze_at)
    n_stem, n_res2 = int(freeze_at == 0), 10 * int(freeze_at < 2)
    assert len(trainer.masters.params) == len(convs) == 42 + n_res2 + n_stem
    assert trainer.trained() == ["head", "fpn", "backbone"] + ["res2"] * int(freeze_at < 2) + ["stem"] * int(freeze_at < 1)
    names = trainer.param_names()
    assert ("backbone.bottom_up.stem.conv1.weight" in names) == (freeze_at == 0)
    assert sum(n.startswith("backbone.bottom_up.res2.") for n in names) == n_res2
    below = {"stem": list(net.stem.parameters()), "res2": list(net.res2.parameters())}
    before = {k: [q.detach().clone() for q in v] for k, v in below.items()}
    masters_before = [p.detach().clone() for p in trainer.masters.params]
    feats, padded = trainer.features(images)
    with torch.no_grad():                                # the training forward IS the inference forward
        for l, f in enumerate(model._trunk_eager(images[0])[0]):
            assert torch.equal(feats[l][0:1].detach(), f)
    res = trainer.step(feats, padded, (64, 96), gb, gc)
    assert bool(torch.isfinite(res["loss_cls"])) and bool(torch.isfinite(res["loss_box_reg"]))
    for i, (p, b) in enumerate(zip(trainer.masters.params, masters_before)):      # every master moves: at 1 res2's ten, at 0 the stem's too
        assert bool(torch.isfinite(p).all()) and not torch.equal(p.detach(), b), i
    for part, frozen in (("stem", freeze_at >= 1), ("res2", freeze_at >= 2)):
        for a, b in zip(below[part], before[part]):
            if frozen:                                   # nothing below the freeze point moves or has a gradient
                assert torch.equal(a.detach(), b) and a.grad is None, part
    assert all(torch.equal(c.bias.detach(), b) for c, b in zip([net.stem[0]], [before["stem"][1]]))      # the folded bias never changes
    # the folded filter is master * s, to the bit: the lowest trained conv (the stem's at 0, res2's shortcut at 1) and one more
    for k in (0, 5):
        c, p, s = trainer.masters.convs[k], trainer.masters.params[k], trainer.masters.scales[k]
        assert torch.equal(c.weight.detach(), p.detach() * s) and c.weight.grad is None
    # the stepped model's forward is the forward of a fresh model that loads the checkpoint
    train_head.save_checkpoint(model, shadow, str(tmp_path), "stepped", 1, train_backbone=True, masters=trainer.masters, trainer=trainer)
    state = torch.load(str(tmp_path / "stepped.pth"), map_location="cpu")
    assert "backbone.bottom_up.stem.conv1.weight" in state["model"] and state[train_head.TRAINER_KEY]["trained"] == trainer.trained()
    assert sorted(state[train_head.TRAINER_KEY]["momentum"]) == sorted(names)
    torch.manual_seed(99)
    fresh = modeling.ProbabilisticRetinaNet(num_classes=7).eval()
    assert checkpoint.load_model_weights(fresh, str(tmp_path), "", strict=True) == str(tmp_path / "stepped.pth")
    fresh = fresh.to(DEV)
    modeling.fold_frozen_bn(fresh)
    for a, b in zip(_forward_c3_c5(model, images[0]), _forward_c3_c5(fresh, images[0])):
        assert torch.equal(a, b)


# ---- 7. the fused step against torch's at freeze point 0 --------------------------------------------------------------------------------
def _trainer(fused: bool, clip: bool):
    model, shadow = resnet_tests.make_models()
    solver = train_head.SolverSettings(clip_type="value", clip_value=0.05) if clip else None
    tr = train_head.HeadTrainer(model, base_lr=0.01, warmup_iters=0, steps=(1000, 2000), train_backbone=True, shadow=shadow, fused_step=fused,
                                freeze_at=0, solver=solver)
    tr.captured = None
    inner = tr.optimizer_step

    def capturing(lr):                                   # the gradients backward() left, as the optimiser's section finds them
        n_plain = len(tr.params) - len(tr.masters.params)
        owners = tr.params[:n_plain] + [c.weight for c in tr.masters.convs]
        tr.captured = [None if o.grad is None else o.grad.detach().clone() for o in owners]
        inner(lr)
    tr.optimizer_step = capturing
    return tr, model


@pytest.mark.parametrize("clip", [False, True], ids=["k25", "k29_clip_value"])
def test_the_fused_step_at_freeze_point_0_steps_as_torchs_within_the_one_step_bound(clip):
    """tests/optimizer_step/test_torch_ops_gpu.py's comparison (test_the_fused_trainer_steps_as_the_torch_one_within_the_one_step_bound) and its
    bound, u = 2^-24: |w' - w^| <= 2 u |w^| + 2 lr 4 u (|a| + wd |w|) with a = s dW' (clipped to +-0.05 under K29's `value`), for both
    optimisers on the longer tensor list; the two backward passes agree to the bit."""
    images, gb, gc = fpn_tests.batch()
    lr32, wd32 = f32(0.01), f32(1e-4)
    grads = {}
    for fused in (False, True):
        tr, model = _trainer(fused, clip)
        n_plain = len(tr.params) - len(tr.masters.params)
        scales = [None] * n_plain + list(tr.masters.scales)
        w0 = [p.detach().cpu().double() for p in tr.params]
        feats, padded = tr.features(images)
        tr.step(feats, padded, (64, 96), gb, gc)
        grads[fused] = tr.captured
        assert len(tr.captured) == len(tr.params) == n_plain + 53
        worst = 0.0
        for i, (p, w, g, s) in enumerate(zip(tr.params, w0, tr.captured, scales)):
            if g is None:
                assert torch.equal(p.detach().cpu().double(), w), (fused, i)
                continue
            a = (g * (1.0 if s is None else s)).cpu().double() if clip else g.cpu().double() * (1.0 if s is None else s.cpu().double())
            if clip:
                a = a.clamp(-f32(0.05), f32(0.05))
            w_hat = w - lr32 * (a + wd32 * w)
            bound = 2 * U * w_hat.abs() + 2 * lr32 * 4 * U * (a.abs() + wd32 * w.abs())
            err = (p.detach().cpu().double() - w_hat).abs()
            worst = max(worst, float((err / bound.clamp(min=1e-300)).max()))
            assert bool((err <= bound).all()), (fused, i, float((err / bound.clamp(min=1e-300)).max()))
        print("SB_TRAINER freeze 0 %s %s: err_w / bound <= %.3f over %d tensors" % ("clip" if clip else "plain", "fused" if fused else "torch", worst, len(w0)))
        for c, p, s in zip(tr.masters.convs, tr.masters.params, tr.masters.scales):
            assert torch.equal(c.weight.detach(), p.detach() * s) and c.weight.grad is None
        assert tr.captured[n_plain] is not None and tuple(tr.captured[n_plain].shape) == (64, 3, 7, 7)      # the stem's
    for i, (a, b) in enumerate(zip(grads[False], grads[True])):       # K21 - K24 and K30 use no float atomics: the two backward passes agree to the bit
        assert (a is None and b is None) or torch.equal(a, b), i


# ---- 8. momentum ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fused", [False, True], ids=["torch", "fused"])
def test_the_momentum_state_round_trips_with_the_stem_and_res2(fused):
    model, shadow = resnet_tests.make_models()
    images, gb, gc = fpn_tests.batch()
    kw = dict(base_lr=0.01, warmup_iters=0, steps=(1000, 2000), train_backbone=True, shadow=shadow, fused_step=fused, freeze_at=0)
    trainer = train_head.HeadTrainer(model, **kw)
    feats, padded = trainer.features(images)
    trainer.step(feats, padded, (64, 96), gb, gc)
    state = trainer.momentum_state()
    assert "backbone.bottom_up.stem.conv1.weight" in state and "backbone.bottom_up.res2.0.shortcut.weight" in state and "backbone.bottom_up.res2.2.conv3.weight" in state
    assert len(state) == len(trainer.params) and bool(state["backbone.bottom_up.stem.conv1.weight"].any())
    model2, shadow2 = resnet_tests.make_models()
    other = train_head.HeadTrainer(model2, **dict(kw, shadow=shadow2))
    if not fused:                                        # torch's optimiser has no buffers before its first step
        f2, p2 = other.features(images)
        other.step(f2, p2, (64, 96), gb, gc)
    other.load_momentum_state(state)
    back = other.momentum_state()
    assert sorted(back) == sorted(state) and all(torch.equal(back[k], state[k]) for k in state)
    at_two = train_head.HeadTrainer(resnet_tests.make_models()[0], **dict(kw, shadow=shadow2, freeze_at=2))
    with pytest.raises(ValueError):                      # a run at another freeze point trains other tensors
        at_two.load_momentum_state(state)
