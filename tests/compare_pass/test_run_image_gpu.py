"""pod_run_image_modes -- one front, several tails -- against that many pod_run_image calls: the same inputs and Philox key, so every field
of every tail's detections must be bit-identical; a tail must leave the shared candidate arrays and keep list as they were (the tails in
reverse order give the same); a refused call enqueues nothing; the call can be captured into a HIP graph.

The module shares its name with tests/test_run_image_gpu.py so that the GPU run order in tests/conftest.py (GPU_ORDER, keyed by module
name) gives it a place."""

import pytest
import torch

from pod_compare_amd import hip, hotpath, synthetic

pytestmark = pytest.mark.gpu

FIELDS = ("boxes", "cov", "scores", "classes", "probs", "records")
BAYES = [("bayes_od", b, c) for b in ("bayesian_inference", "covariance_intersection") for c in ("max_score", "bayesian_inference")]
TAILS = [("standard_nms",), ("anchor_statistics",)] + BAYES
# (runs, cls_var head, reg_var dims, inputs): no covariance at all (BayesOD is refused there), a reg_var head on inputs whose candidates overlap
# everywhere (clusters of many members), N > 1 runs
FIXTURES = {"no_cov": (1, False, 0, "planted"), "reg_var": (1, True, 4, "worst"), "runs": (3, True, 4, "planted")}
IMAGE, OUT, DRAW = (150, 210), (300, 420), 5


@pytest.fixture(scope="module", params=list(FIXTURES))
def case(request):
    """The fixture's inputs, its workspace, and the reference computed ONCE: a pod_run_image call per tail."""
    runs, cls_var, D, mode = FIXTURES[request.param]
    ho = synthetic.planted_head_outputs((160, 224), runs, seed=11 + runs, num_boxes=5, with_cls_var=cls_var, with_reg_var=D > 0, mode=mode).to("cuda")
    params = hotpath.PathParams(num_classes=ho.num_classes, num_anchors=ho.num_anchors)
    hp = hotpath.HotPath(ho.shapes, ho.anchors, params, n_runs=runs, has_cls_var=cls_var, cov_dims=D, device="cuda")
    tails = TAILS if hp.has_covariance else TAILS[:2]
    want = [hp.run_image(t[0], ho.cls, ho.delta, ho.cls_var, ho.reg_var, IMAGE, OUT, *t[1:], draw_id=DRAW) for t in tails]
    torch.cuda.synchronize()
    assert all(w.count() > 0 for w in want)
    return ho, hp, tails, want


def same(got, want):
    m = want.count()
    assert torch.equal(got.n_det, want.n_det)
    for name in FIELDS:
        assert torch.equal(getattr(got, name)[:m], getattr(want, name)[:m]), name


def counters_are_zero(hp):
    torch.cuda.synchronize()
    return int(hp.counters.abs().sum().item()) == 0


def test_every_tail_equals_its_own_run_image_call(case):
    ho, hp, tails, want = case
    got = hp.run_modes(tails, ho.cls, ho.delta, ho.cls_var, ho.reg_var, image_size=IMAGE, out_size=OUT, draw_id=DRAW)
    assert len(got) == len(tails) and counters_are_zero(hp)
    for g, w in zip(got, want):
        same(g, w)


def test_reversed_tails_give_the_same_detections(case):
    """A tail reads boxes / cov / cand_* / keep and writes m_* and its own outputs only: whatever ran before it, it finds the same arrays."""
    ho, hp, tails, want = case
    got = hp.run_modes(tails[::-1], ho.cls, ho.delta, ho.cls_var, ho.reg_var, image_size=IMAGE, out_size=OUT, draw_id=DRAW)
    for g, w in zip(got[::-1], want):
        same(g, w)


def test_two_part_form_equals_the_one_call(case):
    """select / finish_modes (pod_run_image_part: 1, then 4, then an 8 per tail), the form the sparse bbox tower runs between."""
    ho, hp, tails, want = case
    hp.select(ho.cls, ho.cls_var, draw_id=DRAW)
    got = hp.finish_modes(tails, ho.cls, ho.delta, ho.cls_var, ho.reg_var, IMAGE, OUT)
    assert counters_are_zero(hp)
    for g, w in zip(got, want):
        same(g, w)


def test_refusals_enqueue_nothing(case):
    ho, hp, tails, want = case
    lv = hp._levels(ho.cls, ho.delta, ho.cls_var, ho.reg_var, None)
    outs = [hp.new_detections(OUT) for _ in range(hip.POD_MAX_MODE_TAILS + 1)]
    for o in outs:
        o.n_det.fill_(-7)

    def arr(modes):
        a = (hip.PodModeTail * len(modes))()
        for t, mode, o in zip(a, modes, outs):
            t.mode = mode
            t.out = hip.PodDetections(*[o.ptr(n) for n in ("boxes", "cov", "scores", "classes", "probs", "records", "n_det")])
        return a

    hp.n_total.fill_(-5)                                               # K2 writes it: a front that ran, even to completion, would show
    call = lambda a, n: hp.lib.pod_run_image_modes(hp.cfg, lv, hp.ws, a, n, IMAGE[0], IMAGE[1], OUT[0], OUT[1], hip.current_stream())
    hp._begin_draw(DRAW)
    assert call(arr([0]), 0) == -1
    assert call(arr([0] * (hip.POD_MAX_MODE_TAILS + 1)), hip.POD_MAX_MODE_TAILS + 1) == -1
    assert call(arr([0, 9]), 2) == -1                                  # an unknown mode behind a good one
    if not hp.has_covariance:
        assert call(arr([0, hip.POD_MODE_BAYES_OD]), 2) == -1          # BayesOD without covariances (PI:562-636)
        with pytest.raises(hip.PodError):
            hp.run_modes([("standard_nms",), BAYES[0]], ho.cls, ho.delta, ho.cls_var, ho.reg_var, image_size=IMAGE, out_size=OUT, draw_id=DRAW)
    with pytest.raises(ValueError):
        hp.run_modes(["no_such_mode"], ho.cls, ho.delta, ho.cls_var, ho.reg_var, image_size=IMAGE, out_size=OUT)
    with pytest.raises(hip.PodError):
        hp.run_modes([], ho.cls, ho.delta, ho.cls_var, ho.reg_var, image_size=IMAGE, out_size=OUT)
    assert counters_are_zero(hp) and int(hp.n_total.item()) == -5      # the front never ran: no candidate count stands, no total was written
    assert all(int(o.n_det.item()) == -7 for o in outs)                # and no tail wrote
    # the workspace still serves the next image
    got = hp.run_modes(tails[:1], ho.cls, ho.delta, ho.cls_var, ho.reg_var, image_size=IMAGE, out_size=OUT, draw_id=DRAW)
    same(got[0], want[0])


def test_capture_and_replay_equal_eager(case):
    ho, hp, tails, want = case
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        got = hp.run_modes(tails, ho.cls, ho.delta, ho.cls_var, ho.reg_var, image_size=IMAGE, out_size=OUT, draw_id=DRAW)
    for g in got:
        g.buf.zero_()
    graph.replay()
    torch.cuda.synchronize()
    for g, w in zip(got, want):
        g._n = None
        same(g, w)
    assert counters_are_zero(hp)
