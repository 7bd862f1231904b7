"""pod_pdq_assign on the GPU against its host restatement (pdq_ref.assign_ref): the same matching, and -- additions, subtractions and
comparisons only -- bit-equal sums.  Sides 1, 2, around a wavefront's 64 lanes, 130 and the limit 256, rectangular both ways.

The module shares its name with tests/test_eval_matching.py for its place in the GPU run order (tests/conftest.py: GPU_ORDER)."""
import numpy as np
import pytest

from tests.pdq import gpu_common as gc
from tests.pdq import pdq_ref as pr

pytestmark = pytest.mark.gpu
SIDES = (1, 2, 63, 64, 65, 130, 256)


def _expect(q, planes):
    match = pr.assign_ref(q)
    counts, sums = pr.image_totals(planes, match)
    return match, np.asarray(counts), np.asarray(sums)


def test_random_matrices_match_the_restatement_bit_for_bit():
    rng = np.random.default_rng(34)
    shapes = [(n, n) for n in SIDES] + [(2, 1), (1, 2), (63, 65), (65, 63), (130, 64), (64, 130), (256, 3), (3, 256), (200, 256)]
    qs = [rng.uniform(size=s) * (rng.uniform(size=s) < 0.8) for s in shapes]          # a fifth of the pairs can never be true positives
    got = gc.assign(qs)
    for q, (match, counts, sums) in zip(qs, got):
        planes = {name: q * (k + 1) for k, name in enumerate(pr.PLANES)}              # gpu_common.assign's other planes
        want = _expect(q, planes)
        assert np.array_equal(match, want[0]), q.shape
        assert np.array_equal(counts, want[1]), q.shape
        assert sums.tobytes() == want[2].tobytes(), q.shape
        hits = match[match >= 0]
        assert len(set(hits.tolist())) == len(hits)
    alone = gc.assign([qs[4]])[0]                                                      # an image's result does not depend on the batch
    assert np.array_equal(alone[0], got[4][0]) and alone[2].tobytes() == got[4][2].tobytes()


def test_all_zero_and_all_equal_matrices():
    zero, equal, wide, tall = gc.assign([np.zeros((5, 7)), np.full((66, 66), 0.25), np.full((3, 70), 0.5), np.full((70, 3), 0.5)])
    assert zero[0].tolist() == [-1] * 5 and zero[1].tolist() == [0, 7, 5] and (zero[2] == 0.0).all()
    assert equal[0].tolist() == list(range(66)) and equal[1].tolist() == [66, 0, 0]          # the lowest-index rule: the identity
    assert wide[0].tolist() == [0, 1, 2] and wide[1].tolist() == [3, 67, 0]
    assert np.array_equal(tall[0], pr.assign_ref(np.full((70, 3), 0.5))) and tall[1].tolist() == [3, 0, 67]
    assert sorted(tall[0][tall[0] >= 0].tolist()) == [0, 1, 2]


def test_empty_sides_and_the_fixtures_matrices():
    from tests.pdq import fixtures as fx
    ref = gc.referee()
    qs = [r["pPDQ"] for r in ref]
    got = gc.assign(qs, other_planes=[np.concatenate([r[name].reshape(-1) for r in ref]) for name in pr.PLANES[1:]])
    for m, (r, (match, counts, sums)) in enumerate(zip(ref, got)):
        want = _expect(r["pPDQ"], r)
        assert np.array_equal(match, want[0]) and np.array_equal(counts, want[1]) and sums.tobytes() == want[2].tobytes(), m
    assert got[3][1].tolist() == [0, 2, 0] and got[4][1].tolist() == [0, 0, 2]          # no ground truth: false positives; no detection: false negatives
    assert len(fx.all_images()) == len(got)


def test_a_side_of_257_is_refused():
    from pod_compare_amd import hip
    with pytest.raises(hip.PodError):
        gc.assign([np.zeros((257, 2))])
    with pytest.raises(hip.PodError):
        gc.assign([np.zeros((2, 257))])
    assert gc.assign([np.zeros((256, 2))])[0][1].tolist() == [0, 2, 256]
