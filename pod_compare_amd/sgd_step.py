"""The optimiser's step as ONE launch (K25, csrc/k25_sgd_step.hip): SGD with momentum and weight decay on every trained tensor, with
FoldedMasters' two side passes inside it -- a folded filter's gradient scaled by FrozenBN's s on the way in, the folded filter rewritten
from the stepped master on the way out.  `FusedSGD` owns the momentum buffers and the launch's tables:

    * the descriptor table (hip.PodSgdTensor per tensor) lives in PINNED host memory, twice.  Only the gradient pointers change from step
      to step (autograd allocates gradients afresh); a step fills the copy that is not in flight, pod_sgd_step enqueues one
      host-to-device copy of it and the launch, and an event recorded behind them guards that copy of the table: it is rewritten two
      steps later, after `event.synchronize()` -- which by then returns at once.  No step waits for the device.
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


class FusedSGD:
    def __init__(self, entries: Sequence[SgdEntry], momentum: float, weight_decay: float, grads_from=None):
        """grads_from: a data_parallel.GradBucket over the same entries.  The step then reads every gradient from its slice of the bucket
        (the averaged gradient the collective left there): the table's grad pointers are set once, here, and the per-step refresh and the
        checks of .grad are the pack's."""
        self.entries, self.grads_from = list(entries), grads_from
        if grads_from is not None and [e.w.numel() for e in grads_from.entries] != [e.w.numel() for e in self.entries]:
            raise hip.PodError("FusedSGD: the gradient bucket was laid out for other tensors than the ones this optimiser steps")
        self.mu, self.weight_decay = float(momentum), float(weight_decay)
        n = len(self.entries)
        dev = self.entries[0].w.device if n else torch.device("cpu")
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
        self._tables, self._pinned, self._events, self._turn = [], [], [], 0
        self._n_chunks, self._table_dev, self._map_dev = 0, None, None
        if n == 0:
            return
        lib = hip.load()
        nbytes = ctypes.sizeof(hip.PodSgdTensor) * n
        for _ in range(2):
            host = torch.zeros(nbytes, dtype=torch.uint8).pin_memory()
            table = (hip.PodSgdTensor * n).from_address(host.data_ptr())
            for i, (d, e, m) in enumerate(zip(table, self.entries, self.buffers)):
                d.w, d.grad, d.momentum, d.n = e.w.data_ptr(), None if grads_from is None else grads_from.slice_ptr(i), m.data_ptr(), e.w.numel()
                d.folded = None if e.folded is None else e.folded.data_ptr()
                d.scale = None if e.scale is None else e.scale.data_ptr()
                d.per_channel = e.w.numel() // e.w.shape[0] if e.scale is not None and e.w.shape[0] else 0
            self._pinned.append(host)                  # (keeps the memory the ctypes array views)
            self._tables.append(table)
            self._events.append(None)
        self._n_chunks = int(lib.pod_sgd_chunk_map(self._tables[0], n, None, 0))
        if self._n_chunks < 0:
            raise hip.PodError("pod_sgd_chunk_map refused the parameter table (a null, misaligned or aliased tensor)")
        chunk_map = torch.zeros((max(1, self._n_chunks), 2), dtype=torch.int32)
        assert lib.pod_sgd_chunk_map(self._tables[0], n, chunk_map.data_ptr(), self._n_chunks) == self._n_chunks
        self._map_dev = chunk_map.to(dev)
        self._table_dev = torch.zeros(nbytes, dtype=torch.uint8, device=dev)

    def step(self, lr: float) -> None:
        """One launch over every entry whose gradient exists (with a bucket: over every entry, from the bucket); the entries' .grad stay (the
        caller clears them)."""
        if not self.entries:
            return
        k = self._turn
        self._turn ^= 1
        if self._events[k] is not None:
            self._events[k].synchronize()              # the copy enqueued from this table two steps ago has long run
        for d, e in zip(self._tables[k], self.entries if self.grads_from is None else ()):
            g = e.grad_of.grad
            if g is not None and not (g.is_contiguous() and g.dtype == torch.float32 and g.device == self.device and tuple(g.shape) == tuple(e.w.shape)):
                raise hip.PodError("FusedSGD: a gradient that is not a contiguous fp32 tensor of its weight's shape on its GPU")
            d.grad = None if g is None else g.data_ptr()
        with torch.cuda.device(self.device):
            hip.check(hip.load().pod_sgd_step(self._tables[k], self._table_dev.data_ptr(), len(self.entries), self._map_dev.data_ptr(), self._n_chunks,
                                              float(lr), self.mu, self.weight_decay, hip.current_stream()), "pod_sgd_step")
            if self._events[k] is None:
                self._events[k] = torch.cuda.Event()
            self._events[k].record()
        bump_versions(self._written)
