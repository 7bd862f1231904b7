"""pod_grad_pack (K26) alone on a table of every size at which it takes another path, pod_sgd_step from the bucket against pod_sgd_step from
the gradients, two virtual ranks of the small --train-backbone trainer in one process, and a world of one beside the plain fused step.
Everything here is bit-exact: the pack rounds once (scale * g, as torch does), and at scale 1 not at all."""
import ctypes

import pytest
import torch

from pod_compare_amd import hip
from pod_compare_amd.data_parallel import TAIL, GradBucket
from pod_compare_amd.sgd_step import FusedSGD, SgdEntry
from tests.data_parallel import dp

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
C = hip.POD_SGD_CHUNK
SIZES = (1, 3, 4, 5, 63, 4095, 4096, 4097, 2 * C + 3, 0)
GAP = 64                                                   # canary floats in front of and behind the bucket (256 bytes: the bucket stays aligned)
CANARY = -12345.671875                                     # (exact in fp32)


class Raw:
    """The table of SIZES on raw pointers: gradients of their own, a bucket between two canary regions."""

    def __init__(self, seed=0):
        g = torch.Generator().manual_seed(seed)
        lib = hip.load()
        n_t = len(SIZES)
        self.grads = [torch.randn(n, generator=g).to(DEV) for n in SIZES]
        self.keep = [torch.zeros(max(4, n), device=DEV) for n in SIZES] + [torch.zeros(max(4, n), device=DEV) for n in SIZES]      # w, momentum: never read
        self.table = (hip.PodSgdTensor * n_t)()
        for i, (d, n) in enumerate(zip(self.table, SIZES)):
            d.w, d.momentum, d.n = self.keep[i].data_ptr(), self.keep[n_t + i].data_ptr(), n
            d.grad = self.grads[i].data_ptr() if n else None
        offsets = torch.zeros(n_t, dtype=torch.int64)
        self.total = lib.pod_grad_bucket_layout(self.table, n_t, offsets.data_ptr())
        self.offsets = [int(o) for o in offsets]
        assert self.total == sum(-(-n // 4) * 4 for n in SIZES) and all(o % 4 == 0 for o in self.offsets)
        self.n_chunks = lib.pod_sgd_chunk_map(self.table, n_t, None, 0)
        assert self.n_chunks == sum(-(-n // C) for n in SIZES) == 12
        cmap = torch.zeros((self.n_chunks, 2), dtype=torch.int32)
        assert lib.pod_sgd_chunk_map(self.table, n_t, cmap.data_ptr(), self.n_chunks) == self.n_chunks
        self.cmap, self.offsets_dev = cmap.to(DEV), offsets.to(DEV)
        self.table_dev = torch.zeros(ctypes.sizeof(self.table), dtype=torch.uint8, device=DEV)
        self.arena = torch.full((GAP + self.total + GAP,), CANARY, device=DEV)
        self.bucket = self.arena[GAP:GAP + self.total]
        assert self.bucket.data_ptr() % 16 == 0
        self.inside = torch.zeros(self.total, dtype=torch.bool)
        for o, n in zip(self.offsets, SIZES):
            self.inside[o:o + n] = True

    def pack(self, scale):
        hip.check(hip.load().pod_grad_pack(self.table, self.table_dev.data_ptr(), len(SIZES), self.cmap.data_ptr(), self.n_chunks, self.offsets_dev.data_ptr(),
                                           self.bucket.data_ptr(), self.total, scale, hip.current_stream()), "pod_grad_pack")
        torch.cuda.synchronize()


@pytest.mark.parametrize("scale", [1.0, 0.5, 1.0 / 3.0], ids=["1", "half", "third"])
def test_the_pack_writes_scale_times_every_gradient_and_nothing_else(scale):
    raw = Raw()
    assert int((~raw.inside).sum()) == 3 + 1 + 3 + 1 + 1 + 3 + 1      # padding floats: behind n = 1, 3, 5, 63, 4095, 4097, 2C + 3
    raw.bucket.zero_()                                                   # the owner zeroes the bucket once
    kept = [g.clone() for g in raw.grads]
    raw.pack(scale)
    first = raw.arena.cpu()
    got = first[GAP:GAP + raw.total]
    s32 = torch.tensor(scale, dtype=torch.float32)
    for i, (o, n, g) in enumerate(zip(raw.offsets, SIZES, raw.grads)):
        want = (s32.to(DEV) * g).cpu()                                   # one fp32 product per element
        assert torch.equal(got[o:o + n], want), (i, n)
        if scale == 1.0:
            assert torch.equal(got[o:o + n], g.cpu())
        assert torch.equal(g, kept[i])                                   # the gradients are read only
    assert bool((got[raw.inside] != 0).any()) and not bool(got[~raw.inside].any()), "the padding floats are never written"
    assert torch.equal(first[:GAP], torch.full((GAP,), CANARY)) and torch.equal(first[GAP + raw.total:], torch.full((GAP,), CANARY))
    raw.pack(scale)                                                      # a second launch: the same bits
    assert torch.equal(raw.arena.cpu(), first)


def test_the_padding_keeps_what_the_owner_put_there():
    """Never written means never: a bucket that was not zeroed keeps its padding floats to the bit."""
    raw = Raw(seed=1)
    raw.pack(0.5)
    got = raw.bucket.cpu()
    assert torch.equal(got[~raw.inside], torch.full((int((~raw.inside).sum()),), CANARY))


def _entries(seed):
    """Plain tensors of SIZES without the empty one, a scaled one without a folded filter and a folded one whose per_channel = 9 is no
    multiple of 4 -- with gradients."""
    g = torch.Generator().manual_seed(seed)
    entries = []
    for n in [n for n in SIZES if n]:
        p = torch.randn(n, generator=g).to(DEV)
        p.grad = torch.randn(n, generator=g).to(DEV)
        entries.append(SgdEntry(p))
    for shape, fold in (((7, 9), True), ((5, 3, 3, 3), False), ((64, 1153), True)):
        w = torch.randn(shape, generator=g).to(DEV)
        s = (torch.randn(shape[0], generator=g) * 0.5 + 1.0).to(DEV)
        f = (w * s.view(-1, *([1] * (len(shape) - 1)))).contiguous()
        f.grad = torch.randn(shape, generator=g).to(DEV)
        entries.append(SgdEntry(w, grad_of=f, scale=s, folded=f if fold else None))
    return entries


def test_sgd_step_from_the_bucket_at_scale_one_is_sgd_step_from_the_gradients():
    plain_e, bucket_e = _entries(3), _entries(3)
    assert any(e.folded is not None and (e.w.numel() // e.w.shape[0]) % 4 for e in plain_e)
    plain = FusedSGD(plain_e, 0.9, 1e-4)
    bucket = GradBucket(bucket_e, world=1)
    assert bucket.flat.numel() == bucket.floats + TAIL and not bucket.host_staged and bucket.scale == 1.0
    fused = FusedSGD(bucket_e, 0.9, 1e-4, grads_from=bucket)
    for step, lr in enumerate((0.05, 0.01)):
        if step:
            g = torch.Generator().manual_seed(10)
            for a, b in zip(plain_e, bucket_e):
                a.grad_of.grad = torch.randn(a.w.shape, generator=g).to(DEV)
                b.grad_of.grad = a.grad_of.grad.clone()
        bucket.pack()
        for i, e in enumerate(bucket_e):
            assert torch.equal(bucket.slice(i), e.grad_of.grad) and bucket.slice_ptr(i) % 16 == 0, i
        versions = [e.w._version for e in bucket_e]
        plain.step(lr)
        fused.step(lr)
        for i, (a, b) in enumerate(zip(plain_e, bucket_e)):
            assert torch.equal(a.w, b.w) and torch.equal(plain.buffers[i], fused.buffers[i]), (step, i)
            assert (a.folded is None) == (b.folded is None) and (a.folded is None or torch.equal(a.folded, b.folded)), (step, i)
            assert b.w._version > versions[i]
        assert all(bool(m.any()) for m in fused.buffers)
    bucket_e[2].grad_of.grad = None                          # under data parallelism a missing gradient is an error, not K25's skip
    with pytest.raises(hip.PodError):
        bucket.pack()
    with pytest.raises(hip.PodError):                        # a bucket laid out for other tensors
        FusedSGD(bucket_e[:-1], 0.9, 1e-4, grads_from=bucket)


def test_two_virtual_ranks_average_their_gradients_and_stay_bit_equal():
    trainers = [dp.make_trainer(r, 2) for r in range(2)]
    assert all(tr.bucket is not None and tr.bucket.scale == 0.5 and not tr.bucket.host_staged for tr in trainers)
    assert len(trainers[0].fused.entries) == len(trainers[0].params) and trainers[0].bucket.floats >= sum(p.numel() for p in trainers[0].params)
    batch = dp.frames()
    for step in range(2):
        grads = []
        dp.virtual_step(trainers, batch, grads_out=grads)
        g0, g1 = grads
        assert any(not torch.equal(a, b) for a, b in zip(g0, g1))               # the ranks saw different frames
        assert all(bool(torch.isfinite(a).all()) and bool(torch.isfinite(b).all()) for a, b in zip(g0, g1)), step
        for tr in trainers:                                                     # the averaged gradient, from torch, to the bit
            for i, (a, b) in enumerate(zip(g0, g1)):
                assert torch.equal(tr.bucket.slice(i), 0.5 * a + 0.5 * b), (step, i)
        a, b = (dp.state_of(tr) for tr in trainers)
        dp.assert_same_state(a, b, "virtual ranks after step %d" % (step + 1))
        assert a["iteration"] == step + 1
    # each rank kept its own loss state (its normaliser follows its own frames' positives), and the tail holds the ranks' mean losses
    assert trainers[0].model.loss_state is not trainers[1].model.loss_state and all(tr.model.loss_state.draws == 2 for tr in trainers)
    assert bool((a["tail"][:2] > 0).all()) and not bool(a["tail"][2:].any())
    for tr in trainers:                                                        # the masters' filters are the refold of the stepped masters
        for c, p, s in zip(tr.masters.convs, tr.masters.params, tr.masters.scales):
            assert torch.equal(c.weight.detach(), p.detach() * s) and c.weight.grad is None


@pytest.mark.parametrize("train_backbone", [True, False], ids=["backbone", "head_only"])
def test_a_world_of_one_steps_as_the_plain_fused_step(train_backbone):
    images, gb, gc = dp.share(dp.frames(n=2), 0, 1)
    states = []
    for data_parallel in (False, True):
        tr = dp.make_trainer(0, 1, train_backbone=train_backbone, data_parallel=data_parallel)
        assert (tr.bucket is not None) == data_parallel
        for _ in range(2):
            feats, padded = tr.features(images)
            res = tr.step(feats, padded, dp.HW, gb, gc)
            assert bool(torch.isfinite(res["loss_cls"])) and bool(torch.isfinite(res["loss_box_reg"]))
        if data_parallel:                                                       # the tail holds the losses themselves at world 1
            assert torch.equal(tr.mean_losses()["loss_cls"], res["loss_cls"]) and torch.equal(tr.mean_losses()["loss_box_reg"], res["loss_box_reg"])
        st = dp.state_of(tr)
        st["tail"] = None
        states.append(st)
    dp.assert_same_state(states[0], states[1], "world 1 against --fused-step", loss_state=True)
    assert states[1]["iteration"] == 2
