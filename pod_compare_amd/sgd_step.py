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
    * solver (K29, csrc/k29_sgd_solver.hip): `SolverSettings` holds what SOLVER.* asks of the optimiser beyond K25 -- Nesterov, the bias
      group's learning rate factor and weight decay, gradient clipping, the non-finite guard.  With the default settings FusedSGD calls
      pod_sgd_step exactly as it always did; with any other it owns the group array (uint8 per tensor, host and device), the workspace
      (zeroed once) and one PodSgdSolver record per pinned table, and calls pod_sgd_step_solver.  `status()` is the one read-back.
GPU only: pod_sgd_step refusing the table raises hip.PodError; there is no fallback to torch's optimiser."""
import ctypes
import dataclasses
import math
from typing import List, Optional, Sequence, Union

import torch

from . import hip


CLIP_TYPES = {"off": hip.POD_SGD_CLIP_OFF, "value": hip.POD_SGD_CLIP_VALUE, "norm": hip.POD_SGD_CLIP_NORM, "full_model": hip.POD_SGD_CLIP_FULL_MODEL}
LR_SCHEDULERS = ("WarmupMultiStepLR", "WarmupCosineLR")
WARMUP_METHODS = ("linear", "constant")


@dataclasses.dataclass(frozen=True)
class SolverSettings:
    """What SOLVER.* (and --guard-nonfinite) ask beyond momentum SGD with one group under WarmupMultiStepLR; the defaults are that.
    weight_decay_bias None: the weights' decay.  clip_type "off": CLIP_GRADIENTS.ENABLED False (clip_value is then the default's)."""
    nesterov: bool = False
    bias_lr_factor: float = 1.0
    weight_decay_bias: Optional[float] = None
    clip_type: str = "off"
    clip_value: float = 1.0
    lr_scheduler_name: str = "WarmupMultiStepLR"
    warmup_method: str = "linear"
    guard_nonfinite: bool = False

    def __post_init__(self):
        if self.clip_type not in CLIP_TYPES or self.lr_scheduler_name not in LR_SCHEDULERS or self.warmup_method not in WARMUP_METHODS:
            raise ValueError("SolverSettings: clip_type {!r}, lr_scheduler_name {!r}, warmup_method {!r}".format(
                self.clip_type, self.lr_scheduler_name, self.warmup_method))
        if not (math.isfinite(self.clip_value) and self.clip_value > 0 and math.isfinite(self.bias_lr_factor) and self.bias_lr_factor >= 0):
            raise ValueError("SolverSettings: clip_value {} / bias_lr_factor {}".format(self.clip_value, self.bias_lr_factor))
        if self.weight_decay_bias is not None and not (math.isfinite(self.weight_decay_bias) and self.weight_decay_bias >= 0):
            raise ValueError("SolverSettings: weight_decay_bias {}".format(self.weight_decay_bias))

    @property
    def two_groups(self) -> bool:
        """Whether the biases step differently from the weights at all."""
        return self.bias_lr_factor != 1.0 or self.weight_decay_bias is not None

    @property
    def plain_step(self) -> bool:
        """Whether the optimiser's step is K25's: pod_sgd_step (and torch.optim.SGD with one group, unclipped) as before these settings."""
        return not (self.nesterov or self.two_groups or self.clip_type != "off" or self.guard_nonfinite)

    @property
    def computes_norm(self) -> bool:
        """Whether the fused step takes the reduce pass (and so leaves a gradient norm in the status)."""
        return self.guard_nonfinite or self.clip_type in ("norm", "full_model")


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
    def __init__(self, entries: Sequence[SgdEntry], momentum: float, weight_decay: float, grads_from=None, solver: Optional[SolverSettings] = None,
                 groups: Optional[Sequence[int]] = None):
        """grads_from: a data_parallel.GradBucket over the same entries.  The step then reads every gradient from its slice of the bucket
        (the averaged gradient the collective left there): the table's grad pointers are set once, here, and the per-step refresh and the
        checks of .grad are the pack's.  solver: the SolverSettings (None: the defaults); groups: per entry 0 (a weight) or 1 (a bias, stepped
        at the bias group's rate and decay) -- read only when the settings make two groups."""
        self.entries, self.grads_from = list(entries), grads_from
        self.solver = solver if solver is not None else SolverSettings()
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
        self.n_groups, self._workspace, self._watched = 1, None, None
        if self.entries and not self.solver.plain_step:
            n = len(self.entries)
            self.n_groups = 2 if self.solver.two_groups else 1
            group = [0] * n if (groups is None or self.n_groups == 1) else [int(g) for g in groups]
            if len(group) != n or not all(0 <= g < self.n_groups for g in group):
                raise hip.PodError("FusedSGD: `groups` names one of {} groups per entry".format(self.n_groups))
            self._group_host = (ctypes.c_uint8 * n)(*group)
            self._group_dev = torch.tensor(group, dtype=torch.uint8).to(dev)
            nbytes = int(hip.load().pod_sgd_solver_workspace_bytes(n, self.table.n_chunks))
            self._workspace = torch.zeros(nbytes, dtype=torch.uint8, device=dev)                  # zeroed ONCE; reset() clears the status alone
            wd_bias = self.weight_decay if self.solver.weight_decay_bias is None else float(self.solver.weight_decay_bias)
            self._records = [hip.PodSgdSolver() for _ in range(2)]                                # (read by the entry during the call only)
            for r in self._records:
                r.n_groups, r.nesterov, r.guard = self.n_groups, int(self.solver.nesterov), int(self.solver.guard_nonfinite)
                r.clip_type, r.clip_value, r.momentum = CLIP_TYPES[self.solver.clip_type], float(self.solver.clip_value), self.mu
                r.wd[0], r.wd[1] = self.weight_decay, wd_bias

    def step(self, lr: Union[float, Sequence[float]], iteration: int = 0, watch: Sequence[torch.Tensor] = ()) -> None:
        """One launch over every entry whose gradient exists (with a bucket: over every entry, from the bucket); the entries' .grad stay (the
        caller clears them).  lr: the learning rate, or one per group.  Under other than the default settings (three launches when a norm
        or the guard is asked for): `iteration` is what a bad step leaves in the status, `watch` up to four fp32 device scalars that must
        be finite (the step's losses); the tensors are kept until the next step."""
        if not self.entries:
            return
        lrs = [float(lr)] if isinstance(lr, (int, float)) else [float(x) for x in lr]
        table = self.table.begin()
        if self.grads_from is None:
            self.table.refresh_grads(table, "FusedSGD", require_all=False)
        with torch.cuda.device(self.device):
            if self._workspace is None:
                hip.check(hip.load().pod_sgd_step(table, *self.table.launch_args(), lrs[0], self.mu, self.weight_decay, hip.current_stream()), "pod_sgd_step")
            else:
                if len(lrs) < self.n_groups or len(watch) > 4:
                    raise hip.PodError("FusedSGD.step: {} learning rates for {} groups, {} watched scalars (at most 4)".format(len(lrs), self.n_groups, len(watch)))
                watched = [t.detach() for t in watch]
                if not all(t.is_cuda and t.device == self.device and t.dtype == torch.float32 and t.numel() == 1 for t in watched):
                    raise hip.PodError("FusedSGD.step: a watched value is one fp32 scalar on the optimiser's GPU")
                rec = self._records[self.table._turn]
                rec.iteration = int(iteration)
                for g in range(self.n_groups):
                    rec.lr[g] = lrs[g]
                for q in range(4):
                    rec.watch[q] = watched[q].data_ptr() if q < len(watched) else None
                self._watched = watched
                hip.check(hip.load().pod_sgd_step_solver(table, *self.table.launch_args(), self._group_host, self._group_dev.data_ptr(), ctypes.byref(rec),
                                                         self._workspace.data_ptr(), hip.current_stream()), "pod_sgd_step_solver")
            self.table.end()
        bump_versions(self._written)

    def status(self) -> Optional[dict]:
        """The solver's status record, read back (the one synchronisation): bad_steps, first_bad_iteration, last_norm (of the last step the
        reduce pass ran on), poisoned.  None under the default settings, which keep no status."""
        if self._workspace is None:
            return None
        raw = self._workspace[:ctypes.sizeof(hip.PodSgdSolverStatus)].cpu().numpy().tobytes()
        st = hip.PodSgdSolverStatus.from_buffer_copy(raw)
        return {"bad_steps": int(st.bad_steps), "first_bad_iteration": int(st.first_bad_iteration), "last_norm": float(st.last_norm), "poisoned": bool(st.poisoned)}

    def reset(self) -> None:
        """Clears the status: the steps after it are taken again."""
        if self._workspace is not None:
            with torch.cuda.device(self.device):
                hip.check(hip.load().pod_sgd_solver_reset(self._workspace.data_ptr(), hip.current_stream()), "pod_sgd_solver_reset")
