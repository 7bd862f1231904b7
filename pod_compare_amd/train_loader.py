"""The data plan of `train_head --train-loader`: detectron2's `build_detection_train_loader(cfg)` (train_net.py's first line of the loop)
as a deterministic, resumable generator of global batches.  It depends on the json, the config and --random-seed alone -- no frame is
read to make it -- so every rank of a data-parallel run computes the same plan and the loader threads can read ahead of it.

    filter     DATALOADER.FILTER_EMPTY_ANNOTATIONS: a frame without an annotation that has iscrowd == 0 and a mapped category is never
               planned (detectron2's filter_images_with_only_crowd_annotations; the unmapped categories are this project's addition).
    order      TrainingSampler(shuffle=True, seed): ONE torch.Generator seeded with the seed -- the PERMUTATION generator -- gives every
               pass its torch.randperm(n); the passes are concatenated without a boundary.  shuffle=False: file order, repeated.
    draws      per frame, in stream order, from a SECOND generator seeded with the seed -- the DRAW generator: first the short edge
               (INPUT.MIN_SIZE_TRAIN under MIN_SIZE_TRAIN_SAMPLING: `choice` torch.randint over the entries, `range` torch.randint over
               min..max inclusive), then the flip (torch.rand < 0.5, INPUT.RANDOM_FLIP `horizontal`): resize, then flip, detectron2's
               order of transforms.  A draw that has one outcome is not made.  detectron2 draws from per-worker numpy streams, which no
               restatement reproduces: the claim is the distribution and the order, not the numbers.
    grouping   DATALOADER.ASPECT_RATIO_GROUPING: two buckets, w > h and the rest (AspectRatioGroupedDataset), from the json's height /
               width; a bucket emits a batch when it holds SOLVER.IMS_PER_BATCH entries.  Off: consecutive entries.
    ranks      rank r of W takes entries [r B / W, (r + 1) B / W) of every global batch (data_parallel.rank_slice).
    state      the permutation generator's state at the START of the current pass, the draw generator's state, the position in the pass,
               the waiting entries with their draws, and `kind` -- tensors, numbers, strings and lists only (torch.load(weights_only))."""
import dataclasses
from typing import Dict, List, Optional, Sequence, Tuple

import torch

from .anchors import padded_size, resize_shortest_edge

KIND = "train_loader"
SAMPLINGS = ("choice", "range")
FLIPS = ("horizontal", "none")


@dataclasses.dataclass(frozen=True)
class PlanSettings:
    batch: int = 1
    min_sizes: Tuple[int, ...] = (800,)
    sampling: str = "choice"
    max_size: int = 1333
    flip: bool = True
    grouping: bool = True
    filter_empty: bool = True
    shuffle: bool = True
    seed: int = 0

    @property
    def draws_size(self) -> bool:
        return (self.sampling == "range" and self.min_sizes[0] != self.min_sizes[1]) or (self.sampling == "choice" and len(self.min_sizes) > 1)


@dataclasses.dataclass(frozen=True)
class Entry:
    """One planned frame: its index in the json's `images`, the drawn flip and short edge, and the size it is resized to."""
    index: int
    flipped: bool
    short_edge: int
    size: Tuple[int, int]


def plan_settings(cfg, random_flip: bool = False, shuffle: bool = True, seed: int = 0) -> PlanSettings:
    """The plan's settings from INPUT.*, DATALOADER.* and SOLVER.IMS_PER_BATCH; SystemExit naming the key for a value this loader does not
    run.  random_flip (--random-flip) forces the flip on."""
    inp, dl = cfg.INPUT, cfg.DATALOADER
    flip = inp.get("RANDOM_FLIP", "horizontal")
    if flip not in FLIPS:
        raise SystemExit("INPUT.RANDOM_FLIP = {!r} is not supported: one of {}".format(flip, ", ".join(FLIPS)))
    sampling = inp.get("MIN_SIZE_TRAIN_SAMPLING", "choice")
    if sampling not in SAMPLINGS:
        raise SystemExit("INPUT.MIN_SIZE_TRAIN_SAMPLING = {!r} is not supported: one of {}".format(sampling, ", ".join(SAMPLINGS)))
    sizes = inp.get("MIN_SIZE_TRAIN", (800,))
    sizes = (sizes,) if isinstance(sizes, int) else tuple(sizes)
    if not sizes or not all(isinstance(s, int) and not isinstance(s, bool) and s >= 1 for s in sizes):
        raise SystemExit("INPUT.MIN_SIZE_TRAIN = {!r} is not supported: positive integers".format(inp.get("MIN_SIZE_TRAIN")))
    if sampling == "range" and (len(sizes) != 2 or sizes[0] > sizes[1]):
        raise SystemExit("INPUT.MIN_SIZE_TRAIN = {!r} is not supported under MIN_SIZE_TRAIN_SAMPLING = 'range': exactly two entries, "
                         "min and max".format(list(sizes)))
    max_size = int(inp.get("MAX_SIZE_TRAIN", 1333))
    if max_size < 1:
        raise SystemExit("INPUT.MAX_SIZE_TRAIN = {!r} is not supported: a positive integer".format(inp.get("MAX_SIZE_TRAIN")))
    return PlanSettings(batch=max(1, int(cfg.SOLVER.IMS_PER_BATCH)), min_sizes=sizes, sampling=sampling, max_size=max_size,
                        flip=bool(random_flip) or flip == "horizontal", grouping=bool(dl.get("ASPECT_RATIO_GROUPING", True)),
                        filter_empty=bool(dl.get("FILTER_EMPTY_ANNOTATIONS", True)), shuffle=bool(shuffle), seed=int(seed))


def frame_sizes(images: Sequence[dict], where: str = "--coco-json") -> List[Tuple[int, int]]:
    """(height, width) of every record of the json's `images`; SystemExit naming the first record without them."""
    out = []
    for i, rec in enumerate(images):
        if "height" not in rec or "width" not in rec:
            raise SystemExit("--train-loader: image {} of {} has no `height` / `width`: the plan (aspect-ratio groups, resized sizes) comes "
                             "from the json alone".format(rec.get("file_name", i), where))
        out.append((int(rec["height"]), int(rec["width"])))
    return out


def planned_indices(images: Sequence[dict], annotations: Sequence[dict], cat_map: Optional[Dict[int, int]], filter_empty: bool = True) -> List[int]:
    """The indices into `images` the plan samples from: with filter_empty those with at least one annotation that has iscrowd == 0 and a
    category in cat_map (None: every category counts)."""
    if not filter_empty:
        return list(range(len(images)))
    usable = {a["image_id"] for a in annotations if not a.get("iscrowd", 0) and (cat_map is None or a["category_id"] in cat_map)}
    return [i for i, rec in enumerate(images) if rec["id"] in usable]


class PlannedFrames:
    """What apply_net.Prefetched reads ahead under the plan: its keys are Entry records, so a size draw is part of an entry's key.
    images: an apply_net.CocoImages; with device_resize the entry is the decoded frame (K31 resizes it), otherwise the host path
    resizes at the entry's drawn size."""

    def __init__(self, images):
        self.images = images

    def __getitem__(self, e: Entry) -> dict:
        return self.images.entry(e.index) if self.images.device_resize else self.images.entry(e.index, size=e.size)


class TrainPlan:
    """The generator of global batches.  sizes: (height, width) per record of the json's `images`; indices: the records sampled from
    (planned_indices).  next_batch() -> the Entry list of the next global batch, in arrival order."""

    def __init__(self, sizes: Sequence[Tuple[int, int]], indices: Sequence[int], settings: PlanSettings):
        self.sizes, self.indices, self.settings = [tuple(s) for s in sizes], [int(i) for i in indices], settings
        if not self.indices:
            raise SystemExit("--train-loader: no frame to train on (of {} frames none has a usable annotation; "
                             "DATALOADER.FILTER_EMPTY_ANNOTATIONS drops the rest)".format(len(self.sizes)))
        self.n = len(self.indices)
        self.perm_generator = torch.Generator().manual_seed(settings.seed)
        self.draw_generator = torch.Generator().manual_seed(settings.seed)
        self.passes = 0                       # complete passes behind the current one
        self.emitted = 0                      # batches handed out
        self.waiting: List[List[Entry]] = [[], []] if settings.grouping else [[]]
        self._arrived: List[Entry] = []       # the waiting entries of all buckets in arrival order
        self._start_pass()

    # -- order
    def _start_pass(self) -> None:
        self._pass_state = self.perm_generator.get_state().clone()
        self.order = torch.randperm(self.n, generator=self.perm_generator).tolist() if self.settings.shuffle else list(range(self.n))
        self.position = 0

    def _next_index(self) -> int:
        if self.position >= self.n:
            self.passes += 1
            self._start_pass()
        i = self.indices[self.order[self.position]]
        self.position += 1
        return i

    # -- draws
    def draw_short_edge(self) -> int:
        s = self.settings
        if not s.draws_size:
            return int(s.min_sizes[0])
        if s.sampling == "range":
            return int(torch.randint(s.min_sizes[0], s.min_sizes[1] + 1, (), generator=self.draw_generator))
        return int(s.min_sizes[int(torch.randint(0, len(s.min_sizes), (), generator=self.draw_generator))])

    def draw_flip(self) -> bool:
        return bool(torch.rand((), generator=self.draw_generator) < 0.5) if self.settings.flip else False

    def entry(self, index: int, flipped: bool, short_edge: int) -> Entry:
        h, w = self.sizes[index]
        return Entry(int(index), bool(flipped), int(short_edge), resize_shortest_edge(h, w, int(short_edge), self.settings.max_size))

    def _bucket_of(self, index: int) -> int:
        h, w = self.sizes[index]
        return (0 if w > h else 1) if self.settings.grouping else 0

    def _file(self, e: Entry) -> Optional[List[Entry]]:
        bucket = self.waiting[self._bucket_of(e.index)]
        bucket.append(e)
        self._arrived.append(e)
        if len(bucket) < self.settings.batch:
            return None
        out = list(bucket)
        bucket.clear()
        for x in out:
            self._arrived.remove(x)
        return out

    def next_batch(self) -> List[Entry]:
        while True:
            index = self._next_index()
            short_edge = self.draw_short_edge()             # resize, then flip: the size is drawn first
            ready = self._file(self.entry(index, self.draw_flip(), short_edge))
            if ready is not None:
                self.emitted += 1
                return ready

    def until_pass_end(self, limit: int = 0) -> List[List[Entry]]:
        """The batches from here to the end of the current pass (the batch that completes across the boundary included; at most `limit`
        when > 0), computed on a copy: this plan does not move.  What the loader threads read ahead of."""
        ahead = TrainPlan(self.sizes, self.indices, self.settings)
        ahead.load_state(self.state())
        out, start = [], ahead.passes
        while ahead.passes == start and not (limit > 0 and len(out) >= limit):
            out.append(ahead.next_batch())
            if ahead.position >= ahead.n:
                break
        return out

    # -- state
    def state(self) -> dict:
        return {"kind": KIND, "pass_generator": self._pass_state.clone(), "draw_generator": self.draw_generator.get_state().clone(),
                "position": int(self.position), "passes": int(self.passes), "emitted": int(self.emitted), "frames": int(self.n),
                "waiting": [[int(e.index), int(e.flipped), int(e.short_edge)] for e in self._arrived]}

    def load_state(self, state: dict) -> None:
        """Continues bit for bit where `state` was taken; ValueError where it does not fit this plan's frames."""
        if state.get("kind") != KIND:
            raise ValueError("not a {} state: kind {!r}".format(KIND, state.get("kind")))
        if int(state["frames"]) != self.n or not 0 <= int(state["position"]) <= self.n:
            raise ValueError("the state plans {} frames at position {}, this plan has {}".format(state["frames"], state["position"], self.n))
        self.perm_generator.set_state(state["pass_generator"])
        self._start_pass()                                  # the pass's permutation again; the generator is where it was behind it
        self.position, self.passes, self.emitted = int(state["position"]), int(state["passes"]), int(state["emitted"])
        self.draw_generator.set_state(state["draw_generator"])
        self.waiting = [[], []] if self.settings.grouping else [[]]
        self._arrived = []
        for index, flipped, short_edge in state["waiting"]:
            if not 0 <= int(index) < len(self.sizes) or self._file(self.entry(int(index), bool(flipped), int(short_edge))) is not None:
                raise ValueError("the waiting frames do not fit this data set and SOLVER.IMS_PER_BATCH")


def batch_padded_size(entries: Sequence[Entry]) -> Tuple[int, int]:
    """detectron2's ImageList.from_tensors at the FPN's divisibility: the common padded size of a batch's frames."""
    return padded_size(max(e.size[0] for e in entries), max(e.size[1] for e in entries))
