"""The FPN's backward pass end to end (pod_compare_amd/fpn_train.py) against fp64 CPU autograd through FPN.forward: every parameter
gradient, alone and under the head; the trainer's step with and without train_fpn; gradient accumulation."""
import copy

import pytest
import torch

from pod_compare_amd import hip, losses, modeling, train_head
from pod_compare_amd.fpn_train import fpn_convs, fpn_forward_train
from pod_compare_amd.head_train import head_convs
from tests.head_backward import hb
from tests.head_backward import test_torch_ops_gpu as head_tests

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CIN, K, B = (64, 128, 192), 64, 2
HW = [(10, 14), (5, 7), (3, 4)]                      # odd sizes on both top-down steps; p6 2 x 2, p7 1 x 1
LEVELS = HW + [(2, 2), (1, 1)]
NAMES = ["lateral.%d" % i for i in range(3)] + ["output.%d" % i for i in range(3)] + ["p6", "p7"]


def make_fpn(seed=0):
    torch.manual_seed(seed)
    fpn = modeling.FPN(in_channels=CIN, out_channels=K)
    for conv in fpn_convs(fpn):
        torch.nn.init.normal_(conv.bias, std=0.1)
    return fpn.to(DEV)


def make_inputs(seed=1):
    """Per image the NCHW planes (the reference's form) and the channels-last (h * w, C) maps (ours)."""
    g = torch.Generator().manual_seed(seed)
    planes = [[torch.randn((1, c, h, w), generator=g) for c, (h, w) in zip(CIN, HW)] for _ in range(B)]
    maps = [[(p.permute(0, 2, 3, 1).reshape(h * w, c).contiguous().to(DEV), h, w) for p, c, (h, w) in zip(img, CIN, HW)] for img in planes]
    return planes, maps, g


def fpn_reference(fpn, planes, dtype):
    f = copy.deepcopy(fpn).to("cpu", dtype)
    for q in f.parameters():
        q.grad = None
    return f, f.forward([torch.cat([img[i] for img in planes]).to(dtype) for i in range(3)])


def fpn_grads(f):
    return [q.grad for c in fpn_convs(f) for q in (c.weight, c.bias)]


def test_every_gradient_of_the_fpn_matches_fp64_autograd():
    fpn = make_fpn()
    planes, maps, g = make_inputs()
    outs = fpn_forward_train(fpn, maps)
    assert [tuple(o.shape) for o in outs] == [(B, K, h, w) for h, w in LEVELS] and all(o.grad_fn is not None for o in outs)
    with torch.no_grad():                                # the training forward IS forward_cl of each image
        for b in range(B):
            for o, r in zip(outs, fpn.forward_cl(maps[b])):
                assert torch.equal(o[b:b + 1].detach(), r)
    cot = [torch.randn(o.shape, generator=g) for o in outs]
    torch.autograd.backward(outs, [c.to(DEV) for c in cot])
    got = fpn_grads(fpn)
    assert len(got) == 16 and all(x is not None and bool(torch.isfinite(x).all()) for x in got)
    ref = {}
    for dtype in (torch.float32, torch.float64):
        f, routs = fpn_reference(fpn, planes, dtype)
        if dtype == torch.float64:
            for o, r in zip(outs, routs):
                assert hb.rel_err(o, r.detach()) <= hb.BAR
        torch.autograd.backward(routs, [c.to(dtype) for c in cot])
        ref[dtype] = fpn_grads(f)
    chk = hb.Checker()
    for i, (a, b32, b64) in enumerate(zip(got, ref[torch.float32], ref[torch.float64])):
        assert a.shape == b64.shape
        chk.add("fpn " + NAMES[i // 2] + (".bias" if i % 2 else ".weight"), a, b32, b64)
    chk.finish()


def test_fpn_and_head_chained_match_the_fp64_replica():
    """The head's feature gradient flows into the FPN: FPN and head parameter gradients against FPN.forward + the plain-torch head in fp64."""
    fpn, head = make_fpn(), head_tests.make_head(0.0)
    planes, maps, g = make_inputs(seed=2)
    out = head.forward_train(fpn_forward_train(fpn, maps))
    groups = [out.cls, out.delta, out.cls_var, out.reg_var]
    cot = [[torch.randn(t.shape, generator=g) for t in grp] for grp in groups]
    torch.autograd.backward([t for grp in groups for t in grp], [x.to(DEV) for grp in cot for x in grp])
    got = fpn_grads(fpn) + [q.grad for c in head_convs(head) for q in (c.weight, c.bias)]
    assert all(x is not None and bool(torch.isfinite(x).all()) for x in got)
    ref = {}
    for dtype in (torch.float32, torch.float64):
        f, feats = fpn_reference(fpn, planes, dtype)
        h = copy.deepcopy(head).to("cpu", dtype)
        for q in h.parameters():
            q.grad = None
        routs = head_tests.reference_forward(h, feats, None, 0.0)
        torch.autograd.backward([t for grp in routs for t in grp], [x.to(dtype) for grp in cot for x in grp])
        ref[dtype] = fpn_grads(f) + [q.grad for c in head_convs(h) for q in (c.weight, c.bias)]
    names = ["fpn " + n for n in NAMES] + ["head " + n for n in head_tests.NAMES]
    chk = hb.Checker()
    for i, (a, b32, b64) in enumerate(zip(got, ref[torch.float32], ref[torch.float64])):
        chk.add("chained " + names[i // 2] + (".bias" if i % 2 else ".weight"), a, b32, b64)
    chk.finish()


def test_gradients_accumulate():
    fpn = make_fpn()
    _, maps, _ = make_inputs(seed=3)
    loss = lambda: sum(o.sum() for o in fpn_forward_train(fpn, maps))
    loss().backward()
    first = [x.clone() for x in fpn_grads(fpn)]
    loss().backward()
    for a, b in zip(fpn_grads(fpn), first):
        assert torch.equal(a, b + b)                     # .grad accumulates; launches repeat to the bit


def test_what_the_path_cannot_take_raises():
    fpn = make_fpn()
    _, maps, _ = make_inputs(seed=4)
    with pytest.raises(hip.PodError):                    # CPU maps
        fpn_forward_train(fpn, [[(t.cpu(), h, w) for t, h, w in img] for img in maps])
    with pytest.raises(hip.PodError):                    # a top-down step that is not a factor of two: c5 2 x 4 under c4 5 x 7
        fpn_forward_train(fpn, [[img[0], img[1], (img[2][0][:8].contiguous(), 2, 4)] for img in maps])
    odd = modeling.FPN(in_channels=(64, 128, 200), out_channels=K).to(DEV)       # 200 % 16: no split 1x1 form
    with pytest.raises(hip.PodError):
        fpn_forward_train(odd, [[img[0], img[1], (torch.zeros((12, 200), device=DEV), 3, 4)] for img in maps])
    assert all(q.grad is None for q in fpn.parameters())


# ---- the trainer --------------------------------------------------------------------------------------------------------------------
def make_model(seed=5):
    torch.manual_seed(seed)
    model = modeling.ProbabilisticRetinaNet(num_classes=7).to(DEV).eval()
    modeling.fold_frozen_bn(model)
    model.loss_state = losses.ProbabilisticLosses(num_classes=7, cls_var_num_samples=3, annealing_step=80000)
    return model


def batch(seed=6):
    g = torch.Generator().manual_seed(seed)
    images = [torch.randint(0, 256, (3, 64, 96), generator=g, dtype=torch.uint8).to(DEV) for _ in range(2)]
    gb = [torch.tensor([[10., 8., 44., 40.], [50., 20., 90., 60.]]), torch.zeros((0, 4))]
    gc = [torch.tensor([1, 4]), torch.zeros((0,), dtype=torch.long)]
    return images, gb, gc


def test_a_step_with_train_fpn_moves_every_fpn_parameter_and_the_next_forward_uses_it():
    model = make_model()
    images, gb, gc = batch()
    trainer = train_head.HeadTrainer(model, base_lr=0.01, warmup_iters=0, steps=(1000, 2000), train_fpn=True)
    assert all(q.requires_grad for q in model.fpn.parameters()) and not any(q.requires_grad for q in model.bottom_up.parameters())
    assert len(trainer.params) == 2 * (len(head_convs(model.head)) + 8)
    before = [q.detach().clone() for c in fpn_convs(model.fpn) for q in (c.weight, c.bias)]
    feats, padded = trainer.features(images)
    assert all(f.grad_fn is not None for f in feats) and tuple(padded) == (64, 96)
    old = [f.detach().clone() for f in feats]
    trainer.step(feats, padded, (64, 96), gb, gc)
    after = [q for c in fpn_convs(model.fpn) for q in (c.weight, c.bias)]
    for i, (a, b) in enumerate(zip(after, before)):
        name = NAMES[i // 2] + (".bias" if i % 2 else ".weight")
        assert bool(torch.isfinite(a).all()) and not torch.equal(a.detach(), b), name
    new, _ = trainer.features(images)                    # the derived filters follow the weights' versions
    assert all(not torch.equal(n.detach(), o) for n, o in zip(new, old))


def test_a_step_without_train_fpn_leaves_the_fpn_alone():
    model = make_model()
    images, gb, gc = batch()
    trainer = train_head.HeadTrainer(model, base_lr=0.01, warmup_iters=0, steps=(1000, 2000))
    before = [q.detach().clone() for q in model.fpn.parameters()]
    feats, padded = trainer.features(images)
    assert all(f.grad_fn is None for f in feats)
    trainer.step(feats, padded, (64, 96), gb, gc)
    for a, b in zip(model.fpn.parameters(), before):
        assert torch.equal(a.detach(), b) and a.grad is None and not a.requires_grad
