"""Data-parallel training as detectron2's launch + DistributedDataParallel give it to train_net.py: one process per GPU, the global batch
split over the processes, gradients averaged -- here by ONE gradient bucket and ONE collective per step.

    * `GradBucket` owns one flat fp32 device buffer that holds every trained tensor's gradient (pod_grad_bucket_layout: each tensor on 16
      bytes) plus a 4-float tail.  `pack()` is ONE launch (K26, csrc/k26_grad_bucket.hip) that writes scale * grad, scale = 1 / world, for
      all tensors through K25's chunk map; its descriptor table is a sgd_step.TensorTable (pinned host memory, twice, guarded by
      events).  `set_tail` puts the two loss scalars, scaled alike, behind the gradients: the rank mean of the log line (detectron2's
      reduce_dict) rides in the same collective and costs no synchronisation of its own.
    * `all_reduce_flat` is the collective: a SUM all-reduce of the flat buffer.  RCCL reduces the device buffer in place; any other backend
      (gloo: several ranks on one GPU, the CPU tests) cannot move device memory, so the buffer is staged through pinned host memory -- the
      rule of ensemble_dist.MemberPipeline.host_staged.
    * FusedSGD(grads_from=bucket) then steps straight from the bucket's slices (sgd_step.py).
The padding floats between tensors are zeroed once and never written: a sum of zeros stays zero.  GPU only for the pack: a table
pod_grad_pack refuses, or a trained tensor without a gradient, raises hip.PodError."""
from typing import List, Optional, Sequence, Tuple

import torch
import torch.distributed as dist

from . import hip
from .sgd_step import TensorTable

TAIL = 4                                               # floats behind the gradients: loss_cls, loss_box_reg, two spare (16 bytes)


def host_staged(t: torch.Tensor, group=None) -> bool:
    """Whether `all_reduce_flat` stages `t` through the host: a device tensor under a backend that is not RCCL."""
    return bool(t.is_cuda) and dist.is_initialized() and dist.get_backend(group) != "nccl"


def all_reduce_flat(t: torch.Tensor, group=None, staging: Optional[torch.Tensor] = None) -> torch.Tensor:
    """SUM all-reduce of a contiguous tensor over `group`, in place.  A CPU tensor, or a device tensor under RCCL, goes to the backend as
    it is; a device tensor under another backend travels through `staging` (pinned host memory of t's shape; allocated if None)."""
    if not t.is_contiguous():
        raise ValueError("all_reduce_flat reduces a contiguous buffer in place")
    if not host_staged(t, group):
        dist.all_reduce(t, op=dist.ReduceOp.SUM, group=group)
        return t
    if staging is None:
        staging = torch.empty(t.shape, dtype=t.dtype).pin_memory()
    staging.copy_(t)                                   # synchronous: the buffer is on the host when the collective starts
    dist.all_reduce(staging, op=dist.ReduceOp.SUM, group=group)
    t.copy_(staging, non_blocking=True)                # ordered on the stream ahead of the step; `staging` is next written after the next pack
    return t


def broadcast_tensors(tensors: Sequence[torch.Tensor], group=None, src: int = 0) -> None:
    """Rank `src`'s values into every rank's `tensors` (fp32, one device), in place, as ONE broadcast of one flat buffer -- staged through
    the host by the rule of all_reduce_flat.  Start-up only; the written tensors' version counters move (copy_)."""
    tensors = [t for t in tensors if t.numel()]
    if not tensors:
        return
    flat = torch.cat([t.detach().reshape(-1) for t in tensors])
    if host_staged(flat, group):
        host = flat.cpu()
        dist.broadcast(host, src=src, group=group)
        flat = host.to(flat.device)
    else:
        dist.broadcast(flat, src=src, group=group)
    off = 0
    with torch.no_grad():
        for t in tensors:
            t.copy_(flat[off:off + t.numel()].view(t.shape))
            off += t.numel()


def gather_objects(obj, world: int, group=None) -> list:
    """Every rank's `obj` (small, picklable: a loss state), in rank order, on every rank."""
    if world == 1:
        return [obj]
    out = [None] * world
    dist.all_gather_object(out, obj, group=group)
    return out


def rank_slice(batch: int, rank: int, world: int) -> Tuple[int, int]:
    """The frames [first, last) of a global batch of `batch` that rank `rank` of `world` takes; SystemExit naming both numbers when the
    batch does not split evenly (detectron2 asserts the same of SOLVER.IMS_PER_BATCH)."""
    batch, rank, world = int(batch), int(rank), int(world)
    if world < 1 or not 0 <= rank < world:
        raise ValueError("rank {} of world {}".format(rank, world))
    if batch % world != 0:
        raise SystemExit("--data-parallel: SOLVER.IMS_PER_BATCH = {} is not a multiple of the world size {}".format(batch, world))
    per = batch // world
    return rank * per, (rank + 1) * per


class GradBucket:
    def __init__(self, entries: Sequence, world: int, group=None):
        """entries: sgd_step.SgdEntry, the trained tensors in the optimiser's order (the gradient of entry e is e.grad_of.grad)."""
        self.entries, self.world, self.group = list(entries), int(world), group
        if self.world < 1:
            raise ValueError("GradBucket: world {}".format(world))
        n = len(self.entries)
        if n == 0:
            raise hip.PodError("GradBucket: nothing is trained")
        dev = self.entries[0].w.device
        if not all(e.w.is_cuda and e.w.device == dev and e.w.dtype == torch.float32 and e.w.is_contiguous() for e in self.entries):
            raise hip.PodError("GradBucket packs the gradients of contiguous fp32 tensors of one GPU: there is no CPU path")
        self.device, self.scale = dev, 1.0 / self.world
        lib = hip.load()
        sizes = (hip.PodSgdTensor * n)()
        for d, e in zip(sizes, self.entries):          # (the layout depends on the n alone; any two aligned addresses make the table valid)
            d.w, d.momentum, d.n = 16, 32, e.w.numel()
        offsets = torch.zeros(n, dtype=torch.int64)
        self.floats = int(lib.pod_grad_bucket_layout(sizes, n, offsets.data_ptr()))
        if self.floats < 0:
            raise hip.PodError("pod_grad_bucket_layout refused the parameter table")
        self.offsets: List[int] = [int(o) for o in offsets]
        self.flat = torch.zeros(self.floats + TAIL, dtype=torch.float32, device=dev)          # zeroed ONCE: the padding is never written
        self.tail = self.flat[self.floats:]
        self._offsets_dev = offsets.to(dev)
        self.host_staged = self.world > 1 and host_staged(self.flat, group)
        self._staging = torch.empty(self.flat.shape, dtype=torch.float32).pin_memory() if self.host_staged else None
        # the pack reads grad and n of its table; w is the weight and `momentum` names the slice the gradient lands in, which makes it a table
        # pod_sgd_chunk_map accepts

        def fill(i, d, e):
            d.w, d.grad, d.momentum, d.n = e.w.data_ptr(), None, self.slice_ptr(i), e.w.numel()
        self.table = TensorTable(self.entries, dev, fill)

    def slice_ptr(self, i: int) -> int:
        """Device address of entry i's gradient inside the bucket (16-byte aligned)."""
        return self.flat.data_ptr() + 4 * self.offsets[i]

    def slice(self, i: int) -> torch.Tensor:
        """Entry i's gradient inside the bucket, as a view of its weight's shape."""
        e = self.entries[i]
        return self.flat[self.offsets[i]:self.offsets[i] + e.w.numel()].view(e.w.shape)

    def pack(self) -> None:
        """ONE launch: every entry's gradient, times 1 / world, into its slice.  The entries' .grad stay (the caller clears them)."""
        table = self.table.begin()
        self.table.refresh_grads(table, "GradBucket", require_all=True)
        with torch.cuda.device(self.device):
            hip.check(hip.load().pod_grad_pack(table, *self.table.launch_args(), *self.pack_args(), self.scale, hip.current_stream()), "pod_grad_pack")
            self.table.end()

    def pack_args(self) -> tuple:
        """What pod_grad_pack takes of the bucket: the tensors' offsets on the device, the buffer, its gradient floats."""
        return self._offsets_dev.data_ptr(), self.flat.data_ptr(), self.floats

    def set_tail(self, loss_cls: torch.Tensor, loss_box_reg: torch.Tensor) -> None:
        """The two loss scalars (device tensors), times 1 / world, into the tail -- from the device, no read-back."""
        torch.mul(torch.stack([loss_cls.detach().reshape(()), loss_box_reg.detach().reshape(())]).to(torch.float32), self.scale, out=self.tail[:2])

    def all_reduce(self) -> None:
        """The step's one collective: gradients and tail summed over the ranks (each already scaled: the sum is the mean)."""
        if self.world > 1:
            all_reduce_flat(self.flat, self.group, self._staging)
