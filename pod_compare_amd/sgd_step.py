"""The optimiser's step as ONE launch (K25, csrc/k25_sgd_step.hip): SGD with momentum and weight decay on every trained tensor, with
FoldedMasters' two side passes inside it -- a folded filter's gradient scaled by FrozenBN's s on the way in, the folded filter rewritten
from the stepped master on the way out.  `FusedSGD` owns the momentum buffers; `TensorTable` owns a launch's tables, for K25 and for K26
(data_parallel.GradBucket) alike:

    * the descriptor table (hip.PodSgdTensor per tensor) lives in PINNED host memory, twice.  Only the gradient pointers change from step
      to step (autograd allocates gradients afresh); a step fills the copy that is not in flight (`begin`, `refresh_grads`), the entry
      enqueues one host-to-device copy of it and the launch, and an event recorded behind them (`end`) guards that copy of the table: it
      is rewritten two steps later, after `event.synchronize()` -- which by then returns at once.  No step waits for the device.
    * the chunk map (pod_sgd_chunk_map) depends on the sizes alone: built once, kept on the device.
    * the kernel writes through raw pointers, so every tensor it may have written gets its version counter bumped
      (torch._C._increment_version, no launch): the derived filters, abs-max records and graph fingerprints key on Tensor._version.
    * grads_from (data-parallel training, data_parallel.GradBucket): the gradients are read from the bucket's slices, where the all-reduce
      left the rank mean; those pointers never change, so the table is filled once and the refresh is the pack's.
GPU only: pod_sgd_step refusing the table raises hip.PodError; there is no fallback to torch's optimiser."""
import ctypes
from typing import List, Optional, Sequence

import torch

from . import hip


class SgdEntry:
    """One tensor of the step: `w` steps on `grad_of.grad` (grad_of: the tensor autograd hands the gradient to -- w itself, or the folded
    conv weight of a master); scale / folded: FrozenBN's s (K, 1, 1, 1) and the folded filter, for a master weight."""

    def __init__(self, w: torch.Tensor, grad_of: Optional[torch.Tensor] = None, scale: Optional[torch.Tensor] = None, folded: Optional[torch.Tensor] = None):
        self.w, self.grad_of, self.scale, self.folded = w, w if grad_of is None else grad_of, scale, folded


def bump_versions(tensors: Sequence[torch.Tensor]) -> None:
    """Marks tensors written behind autograd's back as changed, without a launch (a list: torch iterates what it is given)."""
    torch._C._increment_version(list(tensors))


class TensorTable:
    """The launch table of `entries` for pod_sgd_step / pod_grad_pack: fill(i, descriptor, entry) sets what never changes in both pinned
    copies.  A launch: `table = begin()`, `refresh_grads(table, ...)`, the entry called with (table, *launch_args(), ...), `end()`."""

    def __init__(self, entries: Sequence[SgdEntry], device, fill):
        self.entries, self.device, n = list(entries), device, len(entries)
        nbytes = ctypes.sizeof(hip.PodSgdTensor) * n
        self._pinned = [torch.zeros(nbytes, dtype=torch.uint8).pin_memory() for _ in range(2)]          # (the memory the ctypes arrays view)
        self._tables = [(hip.PodSgdTensor * n).from_address(host.data_ptr()) for host in self._pinned]
        self._events, self._turn = [None, None], 1         # (_turn: the table of the launch in hand; the first launch takes table 0)
        for table in self._tables:
            for i, (d, e) in enumerate(zip(table, self.entries)):
                fill(i, d, e)
        lib = hip.load()
        self.n_chunks = int(lib.pod_sgd_chunk_map(self._tables[0], n, None, 0))
        if self.n_chunks < 0:
            raise hip.PodError("pod_sgd_chunk_map refused the parameter table (a null, misaligned or aliased tensor)")
        chunk_map = torch.zeros((max(1, self.n_chunks), 2), dtype=torch.int32)
        assert lib.pod_sgd_chunk_map(self._tables[0], n, chunk_map.data_ptr(), self.n_chunks) == self.n_chunks
        self._map_dev = chunk_map.to(device)
        self._table_dev = torch.zeros(nbytes, dtype=torch.uint8, device=device)

    def begin(self):
        """The host table this launch fills: the one whose earlier copy to the device has run."""
        self._turn ^= 1
        if self._events[self._turn] is not None:
            self._events[self._turn].synchronize()     # the copy enqueued from this table two launches ago has long run
        return self._tables[self._turn]

    def refresh_grads(self, table, owner: str, require_all: bool) -> None:
        """The entries' current gradients into `table`; require_all: an entry without one raises, otherwise its chunk is skipped."""
        for i, (d, e) in enumerate(zip(table, self.entries)):
            g = e.grad_of.grad
            if g is None and require_all:
                raise hip.PodError("{}: trained tensor {} of shape {} has no gradient this step; under data parallelism every rank "
                                   "reduces every tensor".format(owner, i, tuple(e.w.shape)))
            if g is not None and not (g.is_contiguous() and g.dtype == torch.float32 and g.device == self.device and tuple(g.shape) == tuple(e.w.shape)):
                raise hip.PodError("{}: a gradient that is not a contiguous fp32 tensor of its weight's shape on its GPU".format(owner))
            d.grad = None if g is None else g.data_ptr()

    def launch_args(self) -> tuple:
        """What an entry takes behind the host table."""
        return self._table_dev.data_ptr(), len(self.entries), self._map_dev.data_ptr(), self.n_chunks

    def end(self) -> None:
        """Behind the entry's call, on its stream: guards the table `begin` handed out until its copy has run."""
        if self._events[self._turn] is None:
            self._events[self._turn] = torch.cuda.Event()
        self._events[self._turn].record()


class FusedSGD:
    def __init__(self, entries: Sequence[SgdEntry], momentum: float, weight_decay: float, grads_from=None):
        """grads_from: a data_parallel.GradBucket over the same entries.  The step then reads every gradient from its slice of the bucket
        (the averaged gradient the collective left there): the table's grad pointers are set once, here, and the per-step refresh and the
        checks of .grad are the pack's."""
        self.entries, self.grads_from = list(entries), grads_from
        if grads_from is not None and [e.w.numel() for e in grads_from.entries] != [e.w.numel() for e in self.entries]:
            raise hip.PodError("FusedSGD: the gradient bucket was laid out for other tensors than the ones this optimiser steps")
        self.mu, self.weight_decay = float(momentum), float(weight_decay)
        dev = self.entries[0].w.device if self.entries else torch.device("cpu")
        for e in self.entries:
            ts = [t for t in (e.w, e.grad_of, e.scale, e.folded) if t is not None]
            if not all(t.is_cuda and t.device == dev and t.dtype == torch.float32 and t.is_contiguous() for t in ts):
                raise hip.PodError("FusedSGD steps contiguous fp32 tensors of one GPU: there is no CPU path")
            if tuple(e.grad_of.shape) != tuple(e.w.shape) or (e.folded is not None and tuple(e.folded.shape) != tuple(e.w.shape)):
                raise hip.PodError("FusedSGD: a gradient or folded filter of another shape than its weight")
            if e.scale is not None and (e.w.dim() < 1 or e.scale.numel() != e.w.shape[0]):
                raise hip.PodError("FusedSGD: the scale holds one float per output channel")
        self.device = dev
        self.buffers: List[torch.Tensor] = [torch.zeros_like(e.w, memory_format=torch.contiguous_format) for e in self.entries]
        self._written = [t for e, m in zip(self.entries, self.buffers) for t in (e.w, m, e.folded) if t is not None]

        def fill(i, d, e):
            d.w, d.grad, d.momentum, d.n = e.w.data_ptr(), None if grads_from is None else grads_from.slice_ptr(i), self.buffers[i].data_ptr(), e.w.numel()
            d.folded = None if e.folded is None else e.folded.data_ptr()
            d.scale = None if e.scale is None else e.scale.data_ptr()
            d.per_channel = e.w.numel() // e.w.shape[0] if e.scale is not None and e.w.shape[0] else 0
        self.table = TensorTable(self.entries, dev, fill) if self.entries else None

    def step(self, lr: float) -> None:
        """One launch over every entry whose gradient exists (with a bucket: over every entry, from the bucket); the entries' .grad stay (the
        caller clears them)."""
        if not self.entries:
            return
        table = self.table.begin()
        if self.grads_from is None:
            self.table.refresh_grads(table, "FusedSGD", require_all=False)
        with torch.cuda.device(self.device):
            hip.check(hip.load().pod_sgd_step(table, *self.table.launch_args(), float(lr), self.mu, self.weight_decay, hip.current_stream()), "pod_sgd_step")
            self.table.end()
        bump_versions(self._written)
