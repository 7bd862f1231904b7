"""pod_sgd_step (K25) on one table that holds every way it can go wrong, against an fp64 evaluation of its own expression, and
HeadTrainer(fused_step=True) beside the torch optimiser it replaces.

The bounds, u = 2^-24, from counting roundings (at most three on m', two more on w', contracted to fused multiply-adds or not), on the
magnitudes of the TERMS so that cancellation does not tighten them:
    |m' - m^| <= 4 u (|s g| + wd |w| + mu |m|)             |w' - w^| <= 2 u |w^| + 2 lr (that bound)
m^, w^: the expression in fp64 from the fp32 state the kernel started the call from, with lr, mu, wd rounded to fp32 -- a one-step error."""
import copy
import ctypes

import numpy as np
import pytest
import torch

from pod_compare_amd import hip, modeling, train_head
from pod_compare_amd.resnet_train import FoldedMasters, block_convs
from pod_compare_amd.sgd_step import FusedSGD, SgdEntry
from tests.fpn_backward import test_torch_ops_gpu as fpn_tests
from tests.resnet_backward import rb
from tests.resnet_backward import test_torch_ops_gpu as resnet_tests

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24
C = hip.POD_SGD_CHUNK
GAP = 64                                                   # sentinel floats on each side of every buffer
SENTINEL = -12345.671875                                   # (exact in fp32)
MU, WD = 0.9, 1e-4
f32 = lambda x: float(np.float32(x))


class Table:
    """~300 tensors as views into one arena per role (weights, gradients, momentum, folded filters, scales), every view with GAP sentinel
    floats before and behind it and starting on 16 bytes.  Per element the arenas also carry the scale that applies (1 where none does) and
    which tensor the element belongs to, so that the reference is one vectorised fp64 expression over the arena."""

    def __init__(self, seed=0):
        g = torch.Generator().manual_seed(seed)
        plain = [0, 1, 2, 3, 4, 5, 36, 63, 64, 4097, 3 * C + 3]
        scaled = [(1, 5), (9, 7), (27, 64), (64, 3), (1152, 5), (9, 1), (27, 3), (1, 4099)]          # (per_channel, channels)
        self.specs = []                                    # (n, per_channel or 0, folded?)
        for rep in range(12):
            for n in plain:
                self.specs.append((n, 0, False))
            for k, (pc, ch) in enumerate(scaled):
                self.specs.append((pc * ch, pc, (k + rep) % 3 != 0))                                # two in three with a folded filter
            self.specs += [(36 * (rep + 1), 36, True), (0, 9, True), (2 * C, C // 2, True), (C + 4, 4, False), (7 * (rep + 1), 7, rep % 2 == 0),
                           (63 * 9, 9, True)]
        assert 280 <= len(self.specs) <= 320
        self.off, self.soff, total, stotal = [], [], GAP, GAP
        for n, pc, _ in self.specs:
            self.off.append(total)
            total += (n + 3) // 4 * 4 + GAP
            self.soff.append(stotal)
            stotal += ((n // pc if pc else 0) + 3) // 4 * 4 + GAP
        self.total = total
        self.inside = torch.zeros(total, dtype=torch.bool)
        self.owner = torch.full((total,), -1, dtype=torch.int64)
        self.s_elem = torch.ones(total)
        self.is_folded = torch.zeros(total, dtype=torch.bool)
        scale = torch.full((stotal,), SENTINEL)
        for t, ((n, pc, fold), o, so) in enumerate(zip(self.specs, self.off, self.soff)):
            self.inside[o:o + n] = True
            self.owner[o:o + n] = t
            if pc:
                ch = n // pc
                s = torch.randn(ch, generator=g) * torch.tensor([1.0, 1e-3, -1.0, 2.5, -1e-2])[torch.randint(0, 5, (ch,), generator=g)]
                scale[so:so + ch] = s
                self.s_elem[o:o + n] = s.repeat_interleave(pc)
                self.is_folded[o:o + n] = fold
        arena = lambda fill: torch.where(self.inside, fill, torch.full((total,), SENTINEL))
        self.w = arena(torch.randn(total, generator=g)).to(DEV)
        self.m = arena(torch.randn(total, generator=g) * 0.1).to(DEV)
        self.f = torch.full((total,), SENTINEL, device=DEV)
        self.g = torch.full((total,), SENTINEL, device=DEV)
        self.scale_host, self.scale = scale, scale.to(DEV)
        self.gen = g
        n_t = len(self.specs)
        self.table = (hip.PodSgdTensor * n_t)()
        for d, (n, pc, fold), o, so in zip(self.table, self.specs, self.off, self.soff):
            d.w, d.momentum, d.n, d.per_channel = self.w.data_ptr() + 4 * o, self.m.data_ptr() + 4 * o, n, pc
            d.scale = self.scale.data_ptr() + 4 * so if pc else None
            d.folded = self.f.data_ptr() + 4 * o if fold else None
        lib = hip.load()
        self.n_chunks = lib.pod_sgd_chunk_map(self.table, n_t, None, 0)
        assert self.n_chunks > 0
        cmap = torch.zeros((self.n_chunks, 2), dtype=torch.int32)
        assert lib.pod_sgd_chunk_map(self.table, n_t, cmap.data_ptr(), self.n_chunks) == self.n_chunks
        self.cmap, self.table_dev = cmap.to(DEV), torch.zeros(ctypes.sizeof(self.table), dtype=torch.uint8, device=DEV)

    def new_gradients(self, call: int):
        """Fresh gradients, and another set of tensors without one (every 7th, shifted by the call)."""
        self.g = torch.where(self.inside, torch.randn(self.total, generator=self.gen), torch.full((self.total,), SENTINEL)).to(DEV)
        self.has_grad = torch.tensor([(t + call) % 7 != 0 for t in range(len(self.specs))])
        for t, (d, o) in enumerate(zip(self.table, self.off)):
            d.grad = self.g.data_ptr() + 4 * o if bool(self.has_grad[t]) else None
        self.live = self.inside & self.has_grad[self.owner.clamp(min=0)]

    def step(self, lr):
        hip.check(hip.load().pod_sgd_step(self.table, self.table_dev.data_ptr(), len(self.specs), self.cmap.data_ptr(), self.n_chunks, lr, MU, WD,
                                          hip.current_stream()), "pod_sgd_step")
        torch.cuda.synchronize()

    def state(self):
        return [t.clone() for t in (self.w, self.m, self.f)]

    def restore(self, state):
        for t, s in zip((self.w, self.m, self.f), state):
            t.copy_(s)


def test_one_table_with_every_shape_three_steps_against_fp64():
    tab = Table()
    sizes = {n for n, _, _ in tab.specs}
    assert {0, 1, 2, 3, 4, 5, 36, 63, 64, 4097, 3 * C + 3} <= sizes and {pc for _, pc, _ in tab.specs} >= {1, 9, 27, 64, 1152}
    assert bool((tab.s_elem < 0).any()) and bool((tab.s_elem.abs() < 1e-3).any())
    worst_m = worst_w = 0.0
    for call, lr in enumerate((0.05, 0.01, 0.002)):
        tab.new_gradients(call)
        assert 30 <= int((~tab.has_grad).sum()) <= 60
        w0, m0, f0 = (t.cpu() for t in tab.state())
        before = tab.state()
        tab.step(lr)
        w1, m1, f1 = tab.w.cpu(), tab.m.cpu(), tab.f.cpu()
        # the same state again: the same bits
        tab.restore(before)
        tab.step(lr)
        assert torch.equal(tab.w.cpu(), w1) and torch.equal(tab.m.cpu(), m1) and torch.equal(tab.f.cpu(), f1), "call %d: two runs differ" % call
        # sentinels, read-only operands, and tensors without a gradient (weight, momentum AND folded filter) are untouched to the bit
        dead = ~tab.live
        assert torch.equal(w1[dead], w0[dead]) and torch.equal(m1[dead], m0[dead]), "call %d" % call
        wrote_f = tab.live & tab.is_folded
        assert torch.equal(f1[~wrote_f], f0[~wrote_f]), "call %d" % call
        assert torch.equal(tab.scale.cpu(), tab.scale_host) and torch.equal(tab.g.cpu()[~tab.inside], torch.full((int((~tab.inside).sum()),), SENTINEL))
        # every element against fp64
        live = tab.live
        s, g = tab.s_elem[live].double(), tab.g.cpu()[live].double()
        w, m = w0[live].double(), m0[live].double()
        lr32, mu32, wd32 = f32(lr), f32(MU), f32(WD)
        a = s * g
        m_hat = mu32 * m + (a + wd32 * w)
        w_hat = w - lr32 * m_hat
        bound_m = 4 * U * (a.abs() + wd32 * w.abs() + mu32 * m.abs())
        bound_w = 2 * U * w_hat.abs() + 2 * lr32 * bound_m
        err_m, err_w = (m1[live].double() - m_hat).abs(), (w1[live].double() - w_hat).abs()
        ok = bound_m > 0
        worst_m, worst_w = max(worst_m, float((err_m[ok] / bound_m[ok]).max())), max(worst_w, float((err_w[ok] / bound_w[ok]).max()))
        print("SGD_K25 call %d lr %g: %d live elements, err_m / bound <= %.3f, err_w / bound <= %.3f" % (call, lr, int(live.sum()), worst_m, worst_w))
        assert bool((err_m <= bound_m).all()) and bool((err_w <= bound_w).all()), "call %d" % call
        assert bool((m1[live] != m0[live]).any()) and bool((w1[live] != w0[live]).any())
        # the folded filter is the single fp32 product w' s, as torch forms it on the device
        want_f = (tab.w * tab.s_elem.to(DEV)).cpu()
        assert torch.equal(f1[wrote_f], want_f[wrote_f]), "call %d" % call
        assert int(wrote_f.sum()) > 0


def test_the_folded_filter_is_what_refold_and_fold_frozen_bn_make_of_the_stepped_master():
    """A conv-shortcut bottleneck built as test_one_sgd_step_acts_on_the_unfolded_weight builds its block: after one fused step conv.weight
    is, to the bit, what FoldedMasters.refold writes from the same masters and what fold_frozen_bn makes of a twin that holds them."""
    torch.manual_seed(3)
    ref_blk = modeling.Bottleneck(64, 256, 64, 2).eval()
    with torch.no_grad():
        rb.randomise_frozen_bn(ref_blk, torch.Generator().manual_seed(4))
        bn = ref_blk.conv1[1]
        bn.weight[0], bn.running_var[0] = 0.25, 1.0 - bn.eps
    blk = copy.deepcopy(ref_blk).to(DEV)
    modeling.fold_frozen_bn(blk)
    masters = FoldedMasters(block_convs(blk), rb.pair_list([ref_blk]))
    g = torch.Generator().manual_seed(5)
    before = [c.weight.detach().clone() for c in masters.convs]
    for c in masters.convs:
        c.weight.grad = torch.randn(c.weight.shape, generator=g).to(DEV)
    versions = [c.weight._version for c in masters.convs]
    fused = FusedSGD([SgdEntry(p, grad_of=c.weight, scale=s, folded=c.weight) for c, p, s in zip(masters.convs, masters.params, masters.scales)], MU, WD)
    fused.step(0.01)
    by_kernel = [c.weight.detach().clone() for c in masters.convs]
    assert all(not torch.equal(a, b) for a, b in zip(by_kernel, before))
    assert all(c.weight._version > v for c, v in zip(masters.convs, versions)) and all(p._version > 0 for p in masters.params)
    masters.refold()
    assert all(torch.equal(c.weight.detach(), k) for c, k in zip(masters.convs, by_kernel))
    twin = copy.deepcopy(ref_blk)
    masters.copy_to(rb.pair_list([twin]))
    twin = twin.to(DEV)
    modeling.fold_frozen_bn(twin)
    assert all(torch.equal(a.weight.detach(), k) for a, k in zip(block_convs(twin), by_kernel))


def test_a_null_gradient_tensor_keeps_its_momentum_through_fused_sgd():
    """FusedSGD re-sends the table every step: a parameter whose .grad is None this step is skipped, and stepped again once it has one."""
    p, q = (torch.nn.Parameter(torch.randn(n, generator=torch.Generator().manual_seed(n)).to(DEV)) for n in (63, 4097))
    fused = FusedSGD([SgdEntry(p), SgdEntry(q)], MU, WD)
    p.grad, q.grad = torch.ones_like(p), None
    q0 = q.detach().clone()
    fused.step(0.1)
    assert torch.equal(q.detach(), q0) and not bool(fused.buffers[1].any()) and bool(fused.buffers[0].any())
    q.grad, p.grad = torch.ones_like(q), None
    p1, mp = p.detach().clone(), fused.buffers[0].clone()
    fused.step(0.1)
    fused.step(0.1)
    assert torch.equal(p.detach(), p1) and torch.equal(fused.buffers[0], mp) and not torch.equal(q.detach(), q0)


# ---- the trainer ----------------------------------------------------------------------------------------------------------------------
def _trainer(train_backbone: bool, fused: bool):
    model, shadow = resnet_tests.make_models()
    tr = train_head.HeadTrainer(model, base_lr=0.01, warmup_iters=0, steps=(1000, 2000), train_backbone=train_backbone,
                                shadow=shadow if train_backbone else None, fused_step=fused)
    tr.captured = None
    inner = tr.optimizer_step

    def capturing(lr):                                     # the gradients backward() left, as the optimiser's section finds them
        n_plain = len(tr.params) - (len(tr.masters.params) if tr.masters is not None else 0)
        owners = tr.params[:n_plain] + ([c.weight for c in tr.masters.convs] if tr.masters is not None else [])
        tr.captured = [None if o.grad is None else o.grad.detach().clone() for o in owners]
        inner(lr)
    tr.optimizer_step = capturing
    return tr, model


@pytest.mark.parametrize("train_backbone", [True, False], ids=["backbone", "head_only"])
def test_the_fused_trainer_steps_as_the_torch_one_within_the_one_step_bound(train_backbone):
    images, gb, gc = fpn_tests.batch()
    lr32, wd32 = f32(0.01), f32(1e-4)
    grads, fixed, outs = {}, None, {}
    for fused in (False, True):
        tr, model = _trainer(train_backbone, fused)
        assert (tr.fused is not None) == fused and isinstance(tr.opt, torch.optim.SGD) and tr.lr == 0.01
        n_plain = len(tr.params) - (len(tr.masters.params) if tr.masters is not None else 0)
        scales = [None] * n_plain + (list(tr.masters.scales) if tr.masters is not None else [])
        w0 = [p.detach().cpu().double() for p in tr.params]
        feats, padded = tr.features(images)
        if fixed is None:
            fixed = [f.detach().clone() for f in feats]
        tr.step(feats, padded, (64, 96), gb, gc)
        grads[fused] = tr.captured
        assert len(tr.captured) == len(tr.params) == (2 * (len(train_head.head_convs(model.head)) + 8) + 42 if train_backbone else n_plain)
        worst = 0.0
        for i, (p, w, g, s) in enumerate(zip(tr.params, w0, tr.captured, scales)):
            if g is None:                                  # (no gradient: neither optimiser touches the parameter)
                assert torch.equal(p.detach().cpu().double(), w), (fused, i)
                continue
            a = g.cpu().double() * (1.0 if s is None else s.cpu().double())
            w_hat = w - lr32 * (a + wd32 * w)
            bound = 2 * U * w_hat.abs() + 2 * lr32 * 4 * U * (a.abs() + wd32 * w.abs())
            err = (p.detach().cpu().double() - w_hat).abs()
            assert bool((err <= bound).all()), (fused, i, float((err / bound.clamp(min=1e-300)).max()))
            worst = max(worst, float((err / bound.clamp(min=1e-300)).max()))
            assert not torch.equal(p.detach().cpu().double(), w) or not (bool(a.any()) or bool(w.any())), (fused, i)
        print("SGD_TRAINER %s %s: err_w / bound <= %.3f over %d tensors" % ("backbone" if train_backbone else "head", "fused" if fused else "torch", worst, len(w0)))
        if tr.masters is not None:
            for c, p, s in zip(tr.masters.convs, tr.masters.params, tr.masters.scales):
                assert torch.equal(c.weight.detach(), p.detach() * s) and c.weight.grad is None
        if not fused:
            continue
        # the version bump: what is derived from the weights is rebuilt after EVERY fused step
        anchors = model.anchors_for(tuple(padded))
        with torch.no_grad():
            outs[1] = [t.clone() for t in model.head.forward_train(fixed, anchors, (64, 96)).cls]
        feats2, _ = tr.features(images)
        if train_backbone:
            assert all(not torch.equal(a.detach(), b) for a, b in zip(feats2, fixed))
        tr.step(feats2, padded, (64, 96), gb, gc)
        assert tr.iteration == 2 and model.loss_state.current_step == 2
        with torch.no_grad():
            outs[2] = [t.clone() for t in model.head.forward_train(fixed, anchors, (64, 96)).cls]
        assert all(not torch.equal(a, b) for a, b in zip(outs[1], outs[2]))
        assert all(bool(b.any()) for b in tr.fused.buffers)
    assert len(grads[False]) == len(grads[True])
    for i, (a, b) in enumerate(zip(grads[False], grads[True])):       # K21 - K24 use no float atomics: the two backward passes agree to the bit
        assert (a is None and b is None) or torch.equal(a, b), i
    assert sum(a is not None for a in grads[True]) >= len(grads[True]) - 4
