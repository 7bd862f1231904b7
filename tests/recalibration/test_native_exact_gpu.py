"""K36 on the GPU against the fp64 host restatement (tests/recalibration/recal_ref.py): residuals, moment sums, grid objectives and the
covariance map bit for bit; the temperature sums through the test's own bound; the torch op."""
import math

import numpy as np
import pytest
import torch

from pod_compare_amd import recalibration as rc
from pod_compare_amd import torch_ops  # noqa: F401  (registers torch.ops.pod_mi355x)
from tests.recalibration import recal_ref as ref

pytestmark = pytest.mark.gpu
K = 7


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def boxes_of(fx, rng):
    """fp32 means, (n, 4, 4) covariances (full, the kernel reads the diagonal) and ground truths of the fixture's matched rows."""
    n = fx["resid"].shape[0]
    gt = rng.uniform(0.0, 1000.0, size=(n, 4)).astype(np.float32)
    means = (gt.astype(np.float64) - fx["resid"]).astype(np.float32)
    covs = rng.uniform(-0.5, 0.5, size=(n, 4, 4)).astype(np.float32)
    covs[:, np.arange(4), np.arange(4)] = (fx["sigma"] ** 2).astype(np.float32)
    return means, covs, gt


def run_reg(means, covs, gt, cls=None, n_class=0):
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    z, seg, invalid = rc.reg_z(t(means), t(covs), t(gt), t(cls) if cls is not None else None, n_class)
    n_seg = 4 * max(n_class, 1)
    zg, seg_off, count, total = rc.moment(z, seg, n_seg)
    return z, seg, invalid, zg, seg_off, count, total


def check_reg(means, covs, gt, cls=None, n_class=0):
    z, seg, invalid, zg, seg_off, count, total = run_reg(means, covs, gt, cls, n_class)
    rz, rseg, rinv = ref.reg_z(means, covs, gt, cls, n_class)
    n_seg = 4 * max(n_class, 1)
    rzg, roff = ref.group(rz, rseg, n_seg)
    rcnt, rsum = ref.moment(rzg, roff)
    assert same_bits(z.cpu().numpy(), rz) and np.array_equal(seg.cpu().numpy(), rseg) and invalid.cpu().tolist() == rinv.tolist()
    assert same_bits(zg.cpu().numpy(), rzg) and seg_off.cpu().tolist() == roff.tolist()
    assert count.cpu().tolist() == rcnt.tolist() and same_bits(total.cpu().numpy(), rsum)
    return (zg, seg_off, count), (rzg, roff, rcnt, rsum), rinv


@pytest.mark.parametrize("n_m", [257, 1])
def test_residuals_and_moment_sums_are_bit_equal(n_m):
    fx = ref.fixture(n_m, 64)
    means, covs, gt = boxes_of(fx, np.random.default_rng(7))
    _, (rzg, roff, rcnt, rsum), rinv = check_reg(means, covs, gt)
    assert rcnt.tolist() == [n_m] * 4 and rinv.tolist() == [0] * 4 and all(s > 0 for s in rsum.tolist())


def test_per_class_segments_with_an_empty_class_and_a_single_row():
    fx = ref.fixture(257, 64)
    rng = np.random.default_rng(8)
    means, covs, gt = boxes_of(fx, rng)
    cls = rng.choice([0, 1, 2], size=257).astype(np.int32)            # class 3 has no matched detection, class 4 exactly one, 5 none
    cls[100] = 4
    _, (rzg, roff, rcnt, rsum), _ = check_reg(means, covs, gt, cls, 6)
    assert rcnt[12:16].tolist() == [0] * 4 and rcnt[16:20].tolist() == [1] * 4 and rcnt[20:].tolist() == [0] * 4 and rcnt.sum() == 4 * 257
    scales = ref.moment_scales(rcnt, rsum)
    assert scales[12:16] == [1.0] * 4 and scales[16] == abs(float(rzg[roff[16]]))


def test_invalid_rows_are_left_out_and_counted():
    fx = ref.fixture(300, 100)
    means, covs, gt = boxes_of(fx, np.random.default_rng(9))
    covs[3, 0, 0] = 0.0
    covs[10, 1, 1] = -2.0
    covs[11, 1, 1] = np.nan
    covs[299, 2, 2] = np.inf
    means[50, 3] = np.inf
    gt[51, 3] = np.nan
    (zg, seg_off, count), (rzg, roff, rcnt, _), rinv = check_reg(means, covs, gt)
    assert rinv.tolist() == [1, 2, 1, 2] and rcnt.tolist() == [299, 298, 299, 298]
    assert np.isfinite(zg.cpu().numpy()).all()
    cls = np.zeros(300, dtype=np.int32)
    cls[7], cls[8] = -1, 2                                           # a class outside [0, n_class): the whole row is left out
    _, (_, _, rcnt2, _), rinv2 = check_reg(means, covs, gt, cls, 2)
    assert rinv2.tolist() == [3, 4, 3, 4] and rcnt2[4:].tolist() == [0] * 4


@pytest.fixture(scope="module")
def grid_case():
    fx = ref.fixture(257, 64)
    rng = np.random.default_rng(10)
    means, covs, gt = boxes_of(fx, rng)
    cls = rng.choice([0, 1, 2], size=257).astype(np.int32)
    cls[100] = 4
    return means, covs, gt, cls


@pytest.mark.parametrize("per_class", [False, True])
def test_grid_objectives_and_arg_min_are_bit_equal(grid_case, per_class):
    means, covs, gt, cls = grid_case
    (zg, seg_off, count), (rzg, roff, rcnt, _), _ = check_reg(means, covs, gt, cls if per_class else None, 6 if per_class else 0)
    obj, best_j, best_obj, one_obj = rc.ece_grid(zg, seg_off, count)
    robj, rbest, rbest_obj, rone = ref.ece_fit(rzg, roff)
    assert same_bits(obj.cpu().numpy(), robj) and best_j.cpu().tolist() == rbest.tolist()
    assert same_bits(best_obj.cpu().numpy(), rbest_obj) and same_bits(one_obj.cpu().numpy(), rone)
    assert (best_obj <= one_obj).all()
    if per_class:                                                     # empty segments: objectives 0, the grid point of scale 1
        assert rbest[12:16].tolist() == [512] * 4 and not robj[12:16].any()


def test_grid_tie_rule_on_a_symmetric_tie(grid_case):
    means, covs, gt, _ = grid_case
    (zg, seg_off, count), (rzg, roff, _, _), _ = check_reg(means, covs, gt)
    for scales, j_one in (([2.5, 2.0, 1.0, 2.0, 2.5], 2), ([2.0, 2.0, 1.0, 9.0, 2.0, 2.0], 2), ([0.7, 1.0, 0.7], 1)):
        obj, best_j, best_obj, one_obj = rc.ece_grid(zg, seg_off, count, scales, j_one)
        robj, rbest, _, rone = ref.ece_fit(rzg, roff, scales, None, j_one)
        assert same_bits(obj.cpu().numpy(), robj) and best_j.cpu().tolist() == rbest.tolist() and same_bits(one_obj.cpu().numpy(), rone)
    obj, best_j, _, _ = rc.ece_grid(zg, seg_off, count, [2.5, 2.0, 1.0, 2.0, 2.5], 2)
    o = obj.cpu().numpy()
    assert o[0, 1] == o[0, 3] < o[0, 2] and best_j.cpu().tolist()[0] == 1 and best_j.cpu().tolist()[1] == 2       # x: tie to the smaller j; y: 1 is best


@pytest.mark.parametrize("n_m,n_fp", [(257, 64), (300, 100), (1500, 700)])
def test_temperature_fit_meets_its_own_stopping_rule(n_m, n_fp):
    fx = ref.fixture(n_m, n_fp)
    p, y = fx["p"].reshape(-1), fx["labels"].reshape(-1)
    tp, ty = torch.from_numpy(p).cuda(), torch.from_numpy(y).cuda()
    beta, its, before, after = rc.fit_temperature(tp, ty)
    _, g_i, h_i = ref.cls_terms(p, y, beta)                         # the HOST's terms at the GPU's beta
    g, h, s_abs = math.fsum(g_i), math.fsum(h_i), math.fsum(np.abs(g_i))
    bound = 2.0 ** -40 * abs(beta) * h + 64 * 2.0 ** -53 * s_abs
    print("n %d: beta %.15g in %d iterations, |g| %.3e, bound %.3e (stop %.3e + sum %.3e)" % (p.size, beta, its, abs(g), bound, 2.0 ** -40 * abs(beta) * h,
                                                                                            64 * 2.0 ** -53 * s_abs))
    assert its <= 50 and abs(g) <= bound
    assert after < before and abs(beta - ref.fit_temperature(p, y)[0]) <= 2.0 ** -38 * beta
    # the three sums against the restatement's (numpy's exp / log are not the device's: a few ulp per term, no bit equality)
    sums = rc.ClsSums(tp, ty)
    for b in (1.0, beta, 3.0):
        got, want = sums(b), ref.cls_sums(p, y, b)
        mags = [math.fsum(np.abs(t)) for t in ref.cls_terms(p, y, b)]
        assert all(abs(a - w) <= 64 * 2.0 ** -53 * m for a, w, m in zip(got, want, mags)), (b, got, want)


def test_sums_of_one_score_and_of_the_clamped_scores():
    for p, y in (([0.3], [1]), ([0.0, 1.0, 1e-12, 1.0 - 2.0 ** -24], [0, 1, 1, 0])):
        p, y = np.array(p, dtype=np.float32), np.array(y, dtype=np.uint8)
        got = rc.ClsSums(torch.from_numpy(p).cuda(), torch.from_numpy(y).cuda())(0.75)
        want = ref.cls_sums(p, y, 0.75)
        assert all(math.isfinite(a) and abs(a - w) <= 1e-13 * max(abs(w), 1.0) for a, w in zip(got, want)), (got, want)


@pytest.fixture(scope="module")
def table():
    """5 images x 70 slots (two workgroups of 256 rows, the second partial), counts from empty to full, garbage behind the counts."""
    fx = ref.fixture(300, 100)
    rng = np.random.default_rng(11)
    rec = rng.uniform(-50.0, 50.0, size=(5, 70, 6 + K + 16)).astype(np.float32)
    p = np.resize(fx["p"], (350, K)).reshape(5, 70, K)
    rec[:, :, 6:6 + K] = p
    rec[:, :, 4] = p.max(2)
    rec[:, :, 5] = p.argmax(2)
    a = rng.uniform(-3.0, 3.0, size=(5, 70, 4, 4))
    rec[:, :, 6 + K:] = (a @ a.transpose(0, 1, 3, 2)).reshape(5, 70, 16).astype(np.float32)
    counts = np.array([70, 0, 33, 1, 69], dtype=np.int32)
    return rec, counts


def ulp_close(a, b):
    return np.all(np.abs(a.astype(np.float64) - b.astype(np.float64)) <= np.spacing(np.abs(b)).astype(np.float64))


@pytest.mark.parametrize("per_class", [False, True])
def test_apply_matches_the_restatement(table, per_class):
    rec, counts = table
    scales = [[1.9, 0.66, 2.05, 0.71]] if not per_class else [[1.0 + 0.1 * c, 0.9 - 0.05 * c, 1.3, 0.7 + 0.02 * c] for c in range(K)]
    if per_class:
        scales[2] = [1.0, 1.0, 1.0, 1.0]                              # a class that keeps its covariance bit for bit
    recal = rc.Recalibration(beta=0.4971, scales=scales, per_class=per_class)
    work = rec.copy()
    if per_class:
        work[0, 3, 5], work[0, 4, 5] = -1.0, 40.0                      # classes without scales: the covariance is copied
    out = rc.apply_to_records(torch.from_numpy(work).cuda(), torch.from_numpy(counts).cuda(), K, recal).cpu().numpy()
    want = ref.apply_records(work, counts, K, recal.beta, scales)
    live = np.arange(70)[None, :] < counts[:, None]
    assert not out[~live].any() and out.shape == rec.shape
    assert same_bits(out[live][:, 6 + K:], want[live][:, 6 + K:])                                          # the covariance: bit-equal
    assert ulp_close(out[live][:, 6:6 + K], want[live][:, 6:6 + K]) and ulp_close(out[live][:, 4], want[live][:, 4])
    assert same_bits(out[live][:, :4], work[live][:, :4]) and same_bits(out[live][:, 5], work[live][:, 5])  # box and class untouched
    if per_class:
        assert same_bits(out[0, 3, 6 + K:], work[0, 3, 6 + K:]) and same_bits(out[0, 4, 6 + K:], work[0, 4, 6 + K:])
        twos = live & (work[:, :, 5] == 2)
        assert twos.any() and same_bits(out[twos][:, 6 + K:], work[twos][:, 6 + K:])
        others = live & (work[:, :, 5] == 1)
        assert not np.array_equal(out[others][:, 6 + K:], work[others][:, 6 + K:])
    old, new = work[live][:, 4], out[live][:, 4]                      # the scores' order survives: no ties made, no pair swapped
    order = np.argsort(old, kind="stable")
    assert np.all(np.diff(old[order]) > 0) and np.all(np.diff(new[order]) > 0)
    assert np.array_equal(out[live][:, 6:6 + K].argmax(1), work[live][:, 6:6 + K].argmax(1))


def test_identity_parameters_reproduce_the_input_bytes(table):
    rec, counts = table
    work = rec.copy()
    work[0, 0, 6], work[0, 1, 6 + K], work[0, 2, 4] = np.nan, -0.0, 1.0
    out = rc.apply_to_records(torch.from_numpy(work).cuda(), torch.from_numpy(counts).cuda(), K, rc.Recalibration()).cpu().numpy()
    live = np.arange(70)[None, :] < counts[:, None]
    assert same_bits(out[live], work[live]) and not bits(out[~live]).any()
    one = rc.apply_to_records(torch.from_numpy(work[3:4, :1]).cuda(), torch.tensor([1], dtype=torch.int32).cuda(), K,
                              rc.Recalibration(beta=0.5, scales=[[2.0, 0.5, 2.0, 0.5]])).cpu().numpy()      # n = 1
    assert same_bits(one[:, :, 6 + K:], ref.apply_records(work[3:4, :1], [1], K, 0.5, [[2.0, 0.5, 2.0, 0.5]])[:, :, 6 + K:])


def test_torch_op_equals_apply_to_records(table):
    rec, counts = table
    recal = rc.Recalibration(beta=0.6, scales=[[1.5, 0.8, 1.4, 0.9]])
    t_rec, t_cnt = torch.from_numpy(rec).cuda(), torch.from_numpy(counts).cuda()
    a = rc.apply_to_records(t_rec, t_cnt, K, recal)
    b = torch.ops.pod_mi355x.recalibrate_records(t_rec, t_cnt, K, recal.beta, torch.tensor(recal.scales, dtype=torch.float64))
    assert torch.equal(a, b) and b.shape == t_rec.shape and b.data_ptr() != t_rec.data_ptr()
    with pytest.raises(RuntimeError):
        torch.ops.pod_mi355x.recalibrate_records(t_rec, t_cnt, K + 1, recal.beta, torch.tensor(recal.scales, dtype=torch.float64))
