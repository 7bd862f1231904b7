"""A training batch's network inputs in ONE launch (K31, csrc/k31_train_batch.hip, C ABI pod_train_batch_u8): every decoded frame of a
rank's batch resized at its own drawn size with PIL's bilinear filter, mirrored where its flip was drawn, flipped to BGR and transposed
to CHW -- what `resize.resize_frame_u8` plus `.flip(-1)` give per frame, to the byte, without a launch per frame and per flip.

    * coefficient tables are per AXIS and per (in, out) pair (pod_resize_coeffs on the host, Pillow's fp64 arithmetic), kept on the device
      in an LRU of MAX_AXIS_TABLES: `range` sampling over 640..800 makes up to 161 pairs per axis and source size.  Eviction follows
      resize._device_tables' rule: nothing a queued launch may read is freed without a synchronisation.
    * the launch table (hip.PodTrainFrame per frame) travels as sgd_step.TensorTable's does: pinned host memory twice, the copy not in
      flight is filled, the entry enqueues one host-to-device copy and the launch, an event behind them guards that copy until it has run.
    * every frame gets its own contiguous (3, nh, nw) uint8 tensor: there is no padded batch tensor -- a zero byte is not zero after
      normalisation; the padding to the batch's common size stays in the stem's load.
GPU only: an entry that refuses the table raises hip.PodError; there is no fallback to the per-frame path."""
import ctypes
from collections import OrderedDict
from typing import List, Optional, Sequence, Tuple

import torch

from . import hip, resize

MAX_AXIS_TABLES = 256
_axis_tables: "OrderedDict[tuple, tuple]" = OrderedDict()
_launch_tables = {}


def _axis_table(in_size: int, out_size: int, device: torch.device, keep: list):
    """(bounds, coeffs, k) of one axis on `device`, (None, None, 0) for an axis that keeps its size.  keep: the caller's references, so
    that a table of the batch in hand is not freed by an eviction while the batch is put together."""
    if in_size == out_size:
        return None, None, 0
    key = (in_size, out_size, device.type, device.index if device.index is not None else torch.cuda.current_device())
    ent = _axis_tables.get(key)
    if ent is not None:
        _axis_tables.move_to_end(key)
    else:
        if len(_axis_tables) >= MAX_AXIS_TABLES:
            torch.cuda.synchronize(device)          # a launch that reads the oldest table may still be queued on some stream
            _axis_tables.popitem(last=False)
        bounds, coeffs = resize.axis_tables(in_size, out_size)
        ent = (torch.from_numpy(bounds).to(device), torch.from_numpy(coeffs).to(device), int(coeffs.shape[1]))
        torch.cuda.current_stream(device).synchronize()      # uploaded on this stream, read from any
        _axis_tables[key] = ent
    keep.append(ent)
    return ent


class LaunchTable:
    """pod_train_batch_u8's table of up to POD_TRAIN_BATCH_MAX_FRAMES frames on one device: two pinned host copies and their events
    (sgd_step.TensorTable's scheme), one device copy."""

    def __init__(self, device: torch.device):
        n, size = hip.POD_TRAIN_BATCH_MAX_FRAMES, ctypes.sizeof(hip.PodTrainFrame)
        self.device = device
        self._pinned = [torch.zeros(size * n, dtype=torch.uint8).pin_memory() for _ in range(2)]
        self._tables = [(hip.PodTrainFrame * n).from_address(host.data_ptr()) for host in self._pinned]
        self._events, self._turn = [None, None], 1
        self.table_dev = torch.zeros(size * n, dtype=torch.uint8, device=device)

    def begin(self):
        self._turn ^= 1
        if self._events[self._turn] is not None:
            self._events[self._turn].synchronize()     # the copy enqueued from this table two launches ago has long run
        return self._tables[self._turn]

    def end(self) -> None:
        if self._events[self._turn] is None:
            self._events[self._turn] = torch.cuda.Event()
        self._events[self._turn].record()


def fill_frame(d, src_ptr: int, in_h: int, in_w: int, row_stride: int, xt, yt, dst_ptr: int, out_h: int, out_w: int, bgr: bool, hflip: bool,
               first_tile: int) -> int:
    """Sets one hip.PodTrainFrame; xt / yt: (bounds ptr, coeffs ptr, k) or (None, None, 0).  Returns the next frame's first_tile."""
    d.src, d.in_h, d.in_w, d.row_stride = src_ptr, int(in_h), int(in_w), int(row_stride)
    d.xbounds, d.xcoeffs, d.xk, d.reserved0 = xt[0], xt[1], int(xt[2]), 0
    d.ybounds, d.ycoeffs, d.yk, d.reserved1 = yt[0], yt[1], int(yt[2]), 0
    d.dst, d.out_h, d.out_w, d.flip_channels, d.hflip, d.first_tile = dst_ptr, int(out_h), int(out_w), 1 if bgr else 0, 1 if hflip else 0, int(first_tile)
    return int(first_tile) + ((int(out_w) + 63) // 64) * ((int(out_h) + 3) // 4)


def train_batch_u8(frames: Sequence[torch.Tensor], sizes: Sequence[Tuple[int, int]], hflips: Sequence[bool], bgr: bool = True,
                   outs: Optional[Sequence[torch.Tensor]] = None) -> List[torch.Tensor]:
    """frames: decoded (h, w, 3) uint8 RGB tensors on one GPU (rows may be padded: stride(0) >= 3 w); sizes: the (nh, nw) each is resized
    to; hflips: whether each is mirrored behind the resize.  One launch on the current stream; returns per frame its (3, nh, nw) uint8
    tensor (outs: write into these), equal to resize.resize_frame_u8 at that size followed by .flip(-1) where mirrored, bit for bit."""
    n = len(frames)
    if not (1 <= n <= hip.POD_TRAIN_BATCH_MAX_FRAMES and len(sizes) == n and len(hflips) == n and (outs is None or len(outs) == n)):
        raise hip.PodError("train_batch_u8: 1 .. {} frames, a size and a flip each, got {} / {} / {}".format(
            hip.POD_TRAIN_BATCH_MAX_FRAMES, n, len(sizes), len(hflips)))
    dev = frames[0].device
    fs = []
    for f in frames:
        if not (torch.is_tensor(f) and f.is_cuda and f.device == dev and f.dtype == torch.uint8 and f.dim() == 3 and f.shape[2] == 3):
            raise hip.PodError("train_batch_u8 needs (h, w, 3) uint8 tensors on one GPU, got {} {} on {}".format(
                tuple(getattr(f, "shape", ())), getattr(f, "dtype", None), getattr(f, "device", None)))
        if f.stride(2) != 1 or f.stride(1) != 3 or (f.shape[0] > 1 and f.stride(0) < 3 * f.shape[1]):
            f = f.contiguous()
        fs.append(f)
    result = [torch.empty((3, int(nh), int(nw)), dtype=torch.uint8, device=dev) for nh, nw in sizes] if outs is None else list(outs)
    for o, (nh, nw) in zip(result, sizes):
        if not (o.is_cuda and o.device == dev and o.dtype == torch.uint8 and tuple(o.shape) == (3, int(nh), int(nw)) and o.is_contiguous()):
            raise hip.PodError("train_batch_u8: an output is a contiguous (3, nh, nw) uint8 tensor on the frames' GPU")
    launch = _launch_tables.get(dev)
    if launch is None:
        launch = _launch_tables[dev] = LaunchTable(dev)
    keep, p = [], (lambda t: None if t is None else t.data_ptr())
    table, first = launch.begin(), 0
    for i, (f, o, (nh, nw), flip) in enumerate(zip(fs, result, sizes, hflips)):
        h, w = int(f.shape[0]), int(f.shape[1])
        xb, xc, xk = _axis_table(w, int(nw), dev, keep)
        yb, yc, yk = _axis_table(h, int(nh), dev, keep)
        first = fill_frame(table[i], f.data_ptr(), h, w, f.stride(0) if h > 1 else 3 * w, (p(xb), p(xc), xk), (p(yb), p(yc), yk), o.data_ptr(),
                           nh, nw, bgr, bool(flip), first)
    with torch.cuda.device(dev):
        hip.check(hip.load().pod_train_batch_u8(table, launch.table_dev.data_ptr(), n, first, hip.current_stream()), "pod_train_batch_u8")
        launch.end()
    return result
