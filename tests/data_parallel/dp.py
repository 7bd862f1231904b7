"""Shared by the data-parallel GPU tests: the small --train-backbone trainer as one rank of a world, the virtual-rank emulation of a
data-parallel step in ONE process (what the real ranks must reproduce to the bit), and the worker the two-rank tests start."""
import datetime
import os

import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from pod_compare_amd import train_head

TIMEOUT = datetime.timedelta(minutes=5)      # a rank that died must not leave the other (the test process) waiting
HW = (64, 96)
LR = 1e-5                                    # small: the seeded random weights take two steps without leaving the finite range


def frames(seed=6, n=4):
    """`n` 64 x 96 frames with their ground truth (one frame without a box), as fpn_backward's batch() makes two."""
    g = torch.Generator().manual_seed(seed)
    images = [torch.randint(0, 256, (3,) + HW, generator=g, dtype=torch.uint8) for _ in range(n)]
    boxes = [torch.tensor([[10., 8., 44., 40.], [50., 20., 90., 60.]]), torch.zeros((0, 4)), torch.tensor([[30., 12., 70., 50.]]),
             torch.tensor([[4., 4., 40., 60.], [60., 30., 92., 62.]])][:n]
    classes = [torch.tensor([1, 4]), torch.zeros((0,), dtype=torch.long), torch.tensor([2]), torch.tensor([0, 5])][:n]
    return images, boxes, classes


def make_trainer(rank, world, group=None, device="cuda:0", train_backbone=True, data_parallel=True):
    from tests.resnet_backward import test_torch_ops_gpu as resnet_tests
    with torch.cuda.device(device):
        model, shadow = resnet_tests.make_models()
        if str(model.head.cls_score.weight.device) != str(torch.device(device)):
            model = model.to(device)
        return train_head.HeadTrainer(model, base_lr=LR, warmup_iters=0, steps=(1000, 2000), train_backbone=train_backbone,
                                      shadow=shadow if train_backbone else None, fused_step=True,
                                      data_parallel=(rank, world, group) if data_parallel else None)


def share(batch, rank, world, device="cuda:0"):
    """Rank `rank`'s frames of a global batch, on the device."""
    from pod_compare_amd.data_parallel import rank_slice
    images, gb, gc = batch
    a, b = rank_slice(len(images), rank, world)
    return [im.to(device) for im in images[a:b]], gb[a:b], gc[a:b]


def state_of(tr):
    """Everything a step writes, on the CPU: trained tensors, momentum, the filters folded from the masters, and the rank's loss state."""
    folded = [c.weight for c in tr.masters.convs] if tr.masters is not None else []
    ls = tr.model.loss_state
    return {"params": [p.detach().cpu().clone() for p in tr.params], "momentum": [m.cpu().clone() for m in tr.fused.buffers],
            "folded": [w.detach().cpu().clone() for w in folded], "tail": tr.bucket.tail.cpu().clone() if tr.bucket is not None else None,
            "loss_normalizer": torch.as_tensor(ls.loss_normalizer).detach().cpu().double().reshape(()), "iteration": tr.iteration}


def assert_same_state(a, b, what, loss_state=False):
    for key in ("params", "momentum", "folded"):
        assert len(a[key]) == len(b[key]) and len(a["params"]) > 0, (what, key)
        for i, (x, y) in enumerate(zip(a[key], b[key])):
            assert torch.equal(x, y), (what, key, i)
    assert a["iteration"] == b["iteration"], what
    assert (a["tail"] is None and b["tail"] is None) or torch.equal(a["tail"], b["tail"]), what
    if loss_state:
        assert torch.equal(a["loss_normalizer"], b["loss_normalizer"]), what


def virtual_step(trainers, batch, grads_out=None):
    """One data-parallel step of len(trainers) ranks in this process: each rank's forward and backward on its share and its pack at
    1 / world; the buckets added in rank order (what a SUM all-reduce of two ranks gives, whichever order: one addition) and the sum copied
    to every rank; each rank's step from it."""
    world = len(trainers)
    for r, tr in enumerate(trainers):
        images, gb, gc = share(batch, r, world)
        feats, padded = tr.features(images)
        res = tr.forward_backward(feats, padded, HW, gb, gc)
        assert bool(torch.isfinite(res["loss_cls"])) and bool(torch.isfinite(res["loss_box_reg"])), r
        if grads_out is not None:
            grads_out.append([e.grad_of.grad.detach().clone() for e in tr.fused.entries])
        tr.bucket.pack()
        tr.bucket.set_tail(res["loss_cls"], res["loss_box_reg"])
    total = trainers[0].bucket.flat.clone()
    for tr in trainers[1:]:
        total += tr.bucket.flat
    for tr in trainers:
        tr.bucket.flat.copy_(total)
        tr.optimizer_step(tr.lr)
        tr.advance()


def emulate(world=2, steps=2, batch=None):
    trainers = [make_trainer(r, world) for r in range(world)]
    for _ in range(steps):
        virtual_step(trainers, frames() if batch is None else batch)
    return [state_of(tr) for tr in trainers]


def rank_worker(rank, world, port, tmp, backend="gloo", own_gpu=False, steps=2):
    """One real rank: `steps` steps of the small --train-backbone trainer on its share of frames(), its state to <tmp>/rank_<r>.pt."""
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    dev_index = rank if own_gpu else 0
    torch.cuda.set_device(dev_index)
    device = "cuda:%d" % dev_index
    if backend == "nccl":
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", dev_index), timeout=TIMEOUT)
    else:
        dist.init_process_group(backend, rank=rank, world_size=world, timeout=TIMEOUT)
    try:
        tr = make_trainer(rank, world, device=device)
        assert tr.bucket.host_staged == (backend != "nccl") and (tr.rank, tr.world) == (rank, world)
        for _ in range(steps):
            images, gb, gc = share(frames(), rank, world, device)
            feats, padded = tr.features(images)
            res = tr.step(feats, padded, HW, gb, gc)
            assert bool(torch.isfinite(res["loss_cls"])) and bool(torch.isfinite(res["loss_box_reg"])), rank
        torch.cuda.synchronize()
        torch.save(state_of(tr), os.path.join(tmp, "rank_%d.pt" % rank))
        dist.barrier()
    finally:
        dist.destroy_process_group()


def _spawned_rank_worker(i, *args):
    rank_worker(i + 1, *args)


def with_one_spawned_rank(worker, spawned, args):
    """Rank 0 = `worker(0, *args)` in this process, rank 1 = `spawned` in the one process that is started; the group is destroyed and the
    child terminated whatever happens."""
    saved = {k: os.environ.get(k) for k in ("MASTER_ADDR", "MASTER_PORT", "HSA_ENABLE_IPC_MODE_LEGACY")}
    ctx = mp.spawn(spawned, args=args, nprocs=1, join=False)
    try:
        out = worker(0, *args)
        while not ctx.join():
            pass
        return out
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


def run_two_ranks(tmp_path, backend="gloo", own_gpu=False, steps=2):
    port = 35500 + os.getpid() % 2000
    with_one_spawned_rank(rank_worker, _spawned_rank_worker, (2, port, str(tmp_path), backend, own_gpu, steps))
    return [torch.load(str(tmp_path / ("rank_%d.pt" % r)), weights_only=True) for r in range(2)]
