"""K32 (pod_retinanet_*: detectron2's RetinaNet.inference + detector_postprocess for one image) against the CPU referee
tests/train_eval/d2_inference_ref.py: every stage entry point on its own, fed with inputs made from the referee's results, and the whole
chain through pod_retinanet_infer_image, eagerly and replayed from a captured graph.

Inputs.  Three or four levels of at most 24 x 32 cells, A = 9, K in {1, 7, 15}.  The logits of a level are a seeded permutation of grids
that are evenly spaced in SIGMOID space, in three bands: a `ranked` band high above the threshold whose neighbours differ by >= 1e-4, a
`crowd` band of further candidates between the threshold and the ranked band, and a band below the threshold.  What the tests observe of
an order is (a) which entries pass the threshold, (b) the order of the entries a level keeps and (c) where the cut at rank topk falls;
`assert_margins` checks on the CPU, before an input is used, that no score lies within 1e-4 of the threshold, that the kept entries of
every level differ from their neighbours by >= 1e-4 and that the first entry not kept lies >= 1e-4 below the last kept -- so the last bits of
an fp32 sigmoid can decide nothing that is compared.  (A level of 48 384 entries cannot hold that many scores 1e-4 apart; the crowd, which
is what takes the level past POD_MAX_TOPK candidates and onto the radix select, ranks behind the cut and its internal order is never
observed.)  The tie case plants a block of exactly equal logits across rank topk: the rule "ties to the lower flat index" decides.

Bars: selected flat indices per level, classes, keep list and n EQUAL to the referee's; boxes and scores within the project's standing
1e-4 * max(1, |ref|), through tests/helpers.py's parity log.

The module shares its name with tests/test_torch_ops_gpu.py so that the GPU run order in tests/conftest.py (keyed by module name) gives it
a place."""
import numpy as np
import pytest
import torch

from pod_compare_amd import anchors as _anchors
from pod_compare_amd import hip
from tests.helpers import assert_close
from tests.train_eval.d2_inference_ref import Reference, flat_logits

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
A = 9
THR = 0.05
IMAGE = (192, 256)            # the network input the anchors are laid out for
OUT = (135, 200)              # a non-unit output scale in both directions


def logit(p):
    p = np.asarray(p, dtype=np.float64)
    return np.log(p / (1.0 - p))


def python_keys(logits_flat: torch.Tensor) -> np.ndarray:
    """K32's key of every flat entry: (order bits of the logit) << 32 | (0xFFFFFFFF - f)."""
    x = (logits_flat.numpy().astype(np.float32) + np.float32(0.0)).view(np.uint32).astype(np.uint64)
    ob = np.where(x & np.uint64(0x80000000), ~x & np.uint64(0xFFFFFFFF), x | np.uint64(0x80000000))
    f = np.arange(x.size, dtype=np.uint64)
    return (ob << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - f)


class Case:
    """One input with its referee results (computed once, shared by the tests of the case, never modified)."""

    def __init__(self, name, K, shapes, ranked, crowd, topk, max_det=100, seed=0, tie=None, big_dw=False, delta_sigma=1.2):
        self.name, self.K, self.shapes, self.topk, self.max_det = name, K, list(shapes), topk, max_det
        rng = np.random.default_rng(seed)
        sizes = [h * w * A * K for h, w in shapes]
        crowd = [min(c, n - r) for c, r, n in zip(crowd, ranked, sizes)]
        assert all(r <= n for r, n in zip(ranked, sizes))
        # the three bands, evenly spaced in sigmoid space, dealt to the levels by one permutation each
        hi = np.linspace(0.30, 0.95, max(sum(ranked), 2))[: sum(ranked)]
        mid = np.linspace(0.06, 0.25, max(sum(crowd), 2))[: sum(crowd)]
        n_low = sum(sizes) - sum(ranked) - sum(crowd)
        low = np.linspace(0.001, 0.04, max(n_low, 2))[:n_low]
        hi, mid, low = rng.permutation(hi), rng.permutation(mid), rng.permutation(low)
        self.cls, self.delta = [], []
        for l, (h, w) in enumerate(shapes):
            r, c, n = ranked[l], crowd[l], sizes[l]
            vals = np.concatenate([hi[:r], mid[:c], low[: n - r - c]])
            hi, mid, low = hi[r:], mid[c:], low[n - r - c:]
            flat = logit(rng.permutation(vals)).astype(np.float32)
            if tie is not None and tie[0] == l:          # (level, first rank, length): equal logits across rank topk
                _, first, length = tie
                order = np.argsort(-flat, kind="stable")
                flat[order[first:first + length]] = flat[order[first]]
            # flat order (cell, a, k) -> (A*K, H, W) planes
            self.cls.append(torch.from_numpy(flat.reshape(h, w, A, K).transpose(2, 3, 0, 1).reshape(A * K, h, w).copy()))
            d = rng.normal(0.0, delta_sigma, size=(A * 4, h, w)).astype(np.float32)
            d.reshape(A, 4, h, w)[:, 2:] *= 0.4
            if big_dw:
                d.reshape(A, 4, h, w)[:, 2:, ::2, ::3] = 6.0          # dw, dh beyond log(1000 / 16) = 4.135
            self.delta.append(torch.from_numpy(d))
        self.anchors = _anchors.grid_anchors(self.shapes, strides=_anchors.FPN_STRIDES[: len(shapes)], sizes=_anchors.ANCHOR_SIZES[: len(shapes)])
        self.assert_margins(allow_tie=tie is not None)
        self.ref = Reference(self.cls, self.delta, self.anchors, K, topk=topk, score_thresh=THR, nms_thresh=0.5, max_detections=max_det,
                             image_size=IMAGE, out_size=OUT)

    def assert_margins(self, allow_tie=False):
        for c in self.cls:
            s = np.sort(torch.sigmoid(flat_logits(c, self.K)).double().numpy())[::-1]
            assert np.abs(s - THR).min() >= 1e-4
            k = min(self.topk, int((s > THR).sum()))
            gaps = s[:k] - s[1:k + 1] if k < s.size else s[: k - 1] - s[1:k]
            if allow_tie:
                gaps = gaps[gaps != 0.0]          # the planted block: exactly equal, decided by the tie rule
            assert gaps.size == 0 or gaps.min() >= 1e-4, gaps.min()

    def path(self):
        from pod_compare_amd.retinanet_inference import InferenceParams, RetinaNetInference
        p = InferenceParams(num_classes=self.K, num_anchors=A, topk_candidates=self.topk, score_thresh=THR, nms_thresh=0.5, max_detections=self.max_det)
        ri = RetinaNetInference(self.shapes, self.anchors, p, device=DEV)
        lv = ri.levels([c.to(DEV) for c in self.cls], [d.to(DEV) for d in self.delta])
        return ri, lv


SHAPES4 = [(24, 32), (12, 16), (6, 8), (2, 3)]
CASES = {
    # level 0: 19 200 candidates (> 16 384: the sliced radix route), level 1: 3 300 (> POD_MAX_TOPK: the one-workgroup radix route), level 2: fewer
    # than topk, level 3: H*W*A = 54 < topk; 2 340 candidates reach the NMS, far more than 100 survive it; dw / dh beyond the clamp
    "k7": dict(K=7, shapes=SHAPES4, ranked=[1200, 1300, 300, 40], crowd=[18000, 2000, 0, 0], topk=1000, big_dw=True),
    "k1": dict(K=1, shapes=SHAPES4, ranked=[1200, 1300, 300, 40], crowd=[4000, 300, 0, 0], topk=1000, seed=1),
    "k15": dict(K=15, shapes=SHAPES4[:3], ranked=[1500, 1200, 200], crowd=[17000, 1600, 0], topk=1000, seed=2, big_dw=True),
    # a level without a candidate between two that have some
    "gap": dict(K=7, shapes=SHAPES4[1:], ranked=[150, 0, 20], crowd=[0, 0, 0], topk=100, seed=3),
    # an image without a candidate
    "none": dict(K=7, shapes=SHAPES4[1:], ranked=[0, 0, 0], crowd=[0, 0, 0], topk=100, seed=4),
    # 30 exactly equal logits across rank topk = 100 of level 0, a level of 2 900 candidates (the radix select meets the block)
    "tie": dict(K=7, shapes=SHAPES4[1:], ranked=[400, 90, 10], crowd=[2500, 0, 0], topk=100, seed=5, tie=(0, 85, 30)),
}
_BUILT = {}


@pytest.fixture(params=list(CASES))
def case(request):
    if request.param not in _BUILT:
        _BUILT[request.param] = Case(request.param, **CASES[request.param])
    return _BUILT[request.param]


def test_inputs_hold_the_cases_they_are_for():
    """On the referee alone: the routes, the multi-class anchors, the clamp, the empty boxes and the NMS overflow are all present."""
    from oracle.pod_oracle import class_aware_nms
    c = _BUILT.setdefault("k7", Case("k7", **CASES["k7"]))
    above = [int((torch.sigmoid(flat_logits(x, c.K)) > THR).sum()) for x in c.cls]
    assert above[0] > 16384 and hip.POD_MAX_TOPK < above[1] <= 16384 and above[2] < c.topk and c.shapes[3][0] * c.shapes[3][1] * A < c.topk
    anchors_of = [f // c.K for f in c.ref.flat]
    assert any(int(torch.unique(a, return_counts=True)[1].max()) >= 2 for a in anchors_of)          # several classes of one anchor
    assert len(class_aware_nms(c.ref.boxes, c.ref.scores, c.ref.classes, 0.5)) > c.max_det == len(c.ref.keep)
    assert not bool(c.ref.nonempty.all()) and c.ref.n > 0                                                # boxes clipped to empty
    sel_dw = torch.cat([x.reshape(A, 4, -1).permute(2, 0, 1).reshape(-1, 4)[a] for x, a in zip(c.delta, anchors_of)])[:, 2:]
    assert bool((sel_dw > 4.2).any())                                                                     # dw / dh beyond the clamp
    t = _BUILT.setdefault("tie", Case("tie", **CASES["tie"]))
    lg = flat_logits(t.cls[0], t.K)
    kept = lg[t.ref.flat[0]]
    assert len(kept) == t.topk and int((lg == kept[-1]).sum()) == 30 and int((kept == kept[-1]).sum()) == 15      # the block straddles the cut
    assert bool((t.ref.flat[0][-15:][1:] > t.ref.flat[0][-15:][:-1]).all())                                 # ties: lower flat index first
    g, n = (_BUILT.setdefault(k, Case(k, **CASES[k])) for k in ("gap", "none"))
    assert len(g.ref.flat[1]) == 0 and len(g.ref.flat[0]) > 0 and len(g.ref.flat[2]) > 0 and sum(len(f) for f in n.ref.flat) == 0


def test_score_appends_exactly_the_candidates(case):
    ri, lv = case.path()
    ri.score(lv)
    counts = ri.cand_count.cpu().tolist()
    K = case.K
    for l, c in enumerate(case.cls):
        lg = flat_logits(c, K)
        want = np.sort(python_keys(lg)[(torch.sigmoid(lg) > THR).numpy()])
        base = ri.anchor_base[l] * K
        got = np.sort(ri.cand_keys[base:base + counts[l]].cpu().numpy().view(np.uint64))
        assert counts[l] == want.size and np.array_equal(got, want), (case.name, l, counts[l], want.size)
    assert ri.counters[ri.L:].cpu().tolist() == [0] * (2 * hip.POD_MAX_LEVELS - ri.L)


def test_topk_selects_and_orders_as_the_referee(case):
    """pod_retinanet_topk on lists written from the CPU (every candidate's key, in flat order)."""
    ri, lv = case.path()
    K = case.K
    counts = []
    for l, c in enumerate(case.cls):
        lg = flat_logits(c, K)
        keys = python_keys(lg)[(torch.sigmoid(lg) > THR).numpy()]
        base = ri.anchor_base[l] * K
        ri.cand_keys[base:base + keys.size] = torch.from_numpy(keys.view(np.int64)).to(DEV)
        counts.append(keys.size)
    ri.cand_count.copy_(torch.tensor(counts, dtype=torch.int32))
    ri.topk(lv)
    sel_count = ri.sel_count.cpu().tolist()
    sel = ri.sel_keys.cpu().numpy().view(np.uint64).reshape(ri.L, case.topk)
    for l in range(ri.L):
        got = (np.uint64(0xFFFFFFFF) - (sel[l, :sel_count[l]] & np.uint64(0xFFFFFFFF))).astype(np.int64)
        assert np.array_equal(got, case.ref.flat[l].numpy()), (case.name, l)
    assert int(ri.n_total.item()) == sum(len(f) for f in case.ref.flat)
    ri.counters.zero_()


def _write_selection(ri, case):
    """The referee's selection as pod_retinanet_topk leaves it: cat_keys / cat_level / n_total."""
    keys, levels = [], []
    for l, (c, f) in enumerate(zip(case.cls, case.ref.flat)):
        keys.append(python_keys(flat_logits(c, case.K))[f.numpy()])
        levels.append(np.full(len(f), l, dtype=np.int32))
    keys, levels = np.concatenate(keys), np.concatenate(levels)
    ri.cat_keys[: keys.size] = torch.from_numpy(keys.view(np.int64)).to(DEV)
    ri.cat_level[: keys.size] = torch.from_numpy(levels).to(DEV)
    ri.n_total.fill_(int(keys.size))
    return int(keys.size)


def test_decode_gathers_and_decodes_as_the_referee(case):
    ri, lv = case.path()
    n = _write_selection(ri, case)
    ri.cand_count.fill_(7)                                # consumed: left zero
    ri.boxes.fill_(-7.0)
    ri.decode(lv)
    ref = case.ref
    assert ri.cand_count.cpu().tolist() == [0] * ri.L
    assert torch.equal(ri.classes[:n].cpu().long(), ref.classes) and torch.equal(ri.cand_flat[:n].cpu().long(), torch.cat(ref.flat))
    assert_close(ri.boxes[:n].cpu(), ref.boxes, "K32 decoded boxes")
    assert_close(ri.scores[:n].cpu(), ref.scores, "K32 scores")
    assert bool((ri.boxes[n:] == -7.0).all())              # nothing written past the candidates


def test_postprocess_scales_clips_and_compacts_as_the_referee(case):
    """pod_retinanet_postprocess on the referee's candidates and keep list."""
    ri, lv = case.path()
    ref = case.ref
    n, nk = len(ref.scores), len(ref.keep)
    ri.boxes[:n] = ref.boxes.to(DEV)
    ri.scores[:n] = ref.scores.to(DEV)
    ri.classes[:n] = ref.classes.to(DEV, torch.int32)
    ri.keep[:nk] = ref.keep.to(DEV, torch.int32)
    ri.n_keep.fill_(nk)
    out = ri.new_detections()
    out.boxes.fill_(-7.0)
    ri.postprocess(IMAGE, OUT, out)
    boxes, scores, classes, m = out.trimmed()
    assert m == ref.n and torch.equal(classes.cpu(), ref.det_classes)
    assert_close(boxes.cpu(), ref.det_boxes, "K32 post-processed boxes")
    assert torch.equal(scores.cpu(), ref.det_scores)
    assert bool((out.boxes[m:] == -7.0).all())


def _assert_image(case, ri, out):
    ref = case.ref
    boxes, scores, classes, m = out.trimmed()
    for l, f in enumerate(ri.selected()):
        assert torch.equal(f, ref.flat[l]), (case.name, "selected flat indices of level", l)
    n = int(ri.n_total.item())
    assert n == len(ref.scores) and torch.equal(ri.classes[:n].cpu().long(), ref.classes)
    nk = int(ri.n_keep.item())
    assert nk == len(ref.keep) and torch.equal(ri.keep[:nk].cpu().long(), ref.keep), (case.name, "keep list")
    assert m == ref.n and torch.equal(classes.cpu(), ref.det_classes)
    assert_close(ri.boxes[:n].cpu(), ref.boxes, "K32 decoded boxes (one call)")
    assert_close(boxes.cpu(), ref.det_boxes, "K32 detections: boxes")
    assert_close(scores.cpu(), ref.det_scores, "K32 detections: scores")
    return boxes, scores, classes


def test_infer_image_equals_the_referee_and_replays_from_a_graph(case):
    ri, lv = case.path()
    out = ri.new_detections()
    out.boxes.fill_(-7.0)
    ri.infer_levels(lv, IMAGE, OUT, out)
    eager = [t.clone() for t in _assert_image(case, ri, out)]
    assert bool((out.boxes[case.ref.n:] == -7.0).all())              # n = 0: nothing written at all
    assert ri.counters.cpu().tolist() == [0] * (2 * hip.POD_MAX_LEVELS)
    # the same image a second time through the same workspace, then twice from a captured graph: the same bits
    ri.infer_levels(lv, IMAGE, OUT, out)
    again = _assert_image(case, ri, out)
    assert all(torch.equal(a, b) for a, b in zip(eager, again))
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    gout = ri.new_detections()
    with torch.cuda.graph(graph, stream=side, capture_error_mode="thread_local"):
        ri.infer_levels(lv, IMAGE, OUT, gout)
    torch.cuda.current_stream().wait_stream(side)
    for _ in range(2):
        gout.boxes.fill_(-7.0)
        gout.n.fill_(-1)
        graph.replay()
        replayed = _assert_image(case, ri, gout)
        assert all(torch.equal(a, b) for a, b in zip(eager, replayed))
    torch.cuda.synchronize()


def test_registered_operator_and_limits():
    import pod_compare_amd.torch_ops  # noqa: F401  (registers the library)
    case = _BUILT.setdefault("gap", Case("gap", **CASES["gap"]))
    boxes, scores, classes = torch.ops.pod_mi355x.retinanet_inference(
        [c.unsqueeze(0).to(DEV) for c in case.cls], [d.unsqueeze(0).to(DEV) for d in case.delta], [a.to(DEV) for a in case.anchors],
        list(IMAGE), list(OUT), case.K, case.topk, THR, 0.5, case.max_det)
    assert torch.equal(classes.cpu(), case.ref.det_classes) and classes.dtype == torch.int64
    assert_close(boxes.cpu(), case.ref.det_boxes, "K32 operator: boxes")
    assert_close(scores.cpu(), case.ref.det_scores, "K32 operator: scores")
    # anything outside the library's limits is refused, not run
    from pod_compare_amd.retinanet_inference import InferenceParams, RetinaNetInference
    for bad in (dict(num_classes=16), dict(topk_candidates=hip.POD_MAX_TOPK + 1), dict(max_detections=hip.POD_MAX_DETECTIONS + 1),
                dict(topk_candidates=2048, levels=5)):
        shapes = (SHAPES4 + [(1, 2)])[: bad.pop("levels", 3)]
        p = InferenceParams(**dict(dict(num_classes=7, num_anchors=A), **bad))
        anchors = [torch.zeros(h * w * A, 4) for h, w in shapes]
        with pytest.raises(hip.PodError):
            RetinaNetInference(shapes, anchors, p, device=DEV)
