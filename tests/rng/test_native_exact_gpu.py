"""The kernels' random draws against the host restatement (tests/rng/rng_ref.py): the generator word for word, box_muller16 against
fp64 on a grid exhaustive in each factor, and every counter -> normal map bit for bit.

The maps are separated from the arithmetic: the expected tensor is host words -> the kernels' own box_muller16 (pod_debug_box_muller16)
-> host layout, so every map comparison is torch.equal.  The one tolerance of this module is box_muller16's distance from fp64, measured on
the MI355X and recorded in profiles/rng_contract.md.

The module shares its name with tests/test_native_exact_gpu.py (the same draws, end to end) so that the GPU run order in
tests/conftest.py (GPU_ORDER, keyed by module name) gives it a place."""
import numpy as np
import pytest
import torch

from pod_compare_amd import hip, losses, synthetic
from tests.rng import rng_ref as rr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# box_muller16 (v_log_f32, v_sqrt_f32, v_cos_f32, v_sin_f32, fp32 products) against the fp64 referee, measured on an MI355X over the grid
# of test_box_muller_against_fp64: max |z_gpu - z_fp64| = 8.287e-7, at word 0x3e000015 (radius field 21, angle field 15872: z = 4.000756,
# 1.7 ulp there; profiles/rng_contract.md).  The function is deterministic and the grid exhaustive in each factor: the bar is twice the
# measured maximum, rounded up to one significant digit -- room for a compiler re-association, not for a different approximation.
BM_MEASURED_MAX = 8.287e-7
BM_ABS_TOL = 2e-6


def u32(a):
    """numpy uint32 -> device tensor of the same bits (torch has no arithmetic on uint32: int32 carries them)."""
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32)).to(DEV)


def gpu_philox(ctr_key):
    n = ctr_key.shape[0]
    src, out = u32(ctr_key), torch.empty((n, 4), dtype=torch.int32, device=DEV)
    hip.check(hip.load().pod_debug_philox4x32(src.data_ptr(), out.data_ptr(), n, hip.current_stream()), "pod_debug_philox4x32")
    return out.cpu().numpy().view(np.uint32)


def gpu_box_muller(words):
    """words: numpy uint32, any shape -> fp32 tensor (..., 2) on the CPU: the kernels' box_muller16 of every word."""
    src = u32(words.reshape(-1))
    out = torch.empty((src.numel(), 2), dtype=torch.float32, device=DEV)
    hip.check(hip.load().pod_debug_box_muller16(src.data_ptr(), out.data_ptr(), src.numel(), hip.current_stream()), "pod_debug_box_muller16")
    return out.cpu().view(*words.shape, 2)


def expected_normals(word_which):
    """rng_ref's (word, which) -> the fp32 normals the GPU must hold, in the same layout."""
    word, which = word_which
    z = gpu_box_muller(word)
    return torch.gather(z, -1, torch.from_numpy(which.astype(np.int64))[..., None])[..., 0]


# ---- the generator -----------------------------------------------------------------------------------------------------------------
def test_philox_words_equal_the_host():
    rng = np.random.default_rng(20240229)
    rows = rng.integers(0, 2 ** 32, size=(2 ** 16, 6), dtype=np.uint64).astype(np.uint32)
    rows[:3] = [list(c) + list(k) for c, k, _ in rr.KAT]
    got = gpu_philox(rows)
    assert got[:3].tolist() == [list(out) for _, _, out in rr.KAT]                                   # Random123's known answers
    assert np.array_equal(got, rr.philox4x32_10(rows[:, :4], rows[:, 4:]))


# ---- box_muller16 ------------------------------------------------------------------------------------------------------------------
ALL = np.arange(65536, dtype=np.uint32)
SPREAD = (1024 * np.arange(64) + 512).astype(np.uint32)              # 64 evenly spaced fields: on the angle side cos^n + sin^n averages as over all 65 536
QUARTERS = np.array([0, 65535, 16383, 16384, 32767, 32768, 49151, 49152], dtype=np.uint32)      # the angle fields nearest 0, 1/4, 1/2, 3/4 turn


@pytest.fixture(scope="module")
def grids():
    """name -> (words, gpu (n, 2) fp64, referee (n, 2) fp64): `radii`: all low halves x (SPREAD + QUARTERS) high halves, the SPREAD block
    first; `angles`: all high halves x (SPREAD, 0, 65535) low halves."""
    out = {}
    for name, words in (("radii", (np.concatenate([SPREAD, QUARTERS])[:, None] << 16 | ALL[None, :]).reshape(-1)),
                        ("angles", (ALL[:, None] << 16 | np.concatenate([SPREAD, [0, 65535]]).astype(np.uint32)[None, :]).reshape(-1))):
        n0, n1 = rr.box_muller16(words)
        out[name] = (words, gpu_box_muller(words).double().numpy(), np.stack([n0, n1], axis=-1))
    return out


def test_box_muller_against_fp64(grids):
    worst = (0.0, None, None)
    for name, (words, got, ref) in grids.items():
        assert np.isfinite(got).all()
        err = np.abs(got - ref)
        i = int(err.max(axis=1).argmax())
        print("RNG_BM grid=%s n=%d max_abs_err=%.3e at word=0x%08x (radius field %d, angle field %d) gpu=(%.7f, %.7f) fp64=(%.9f, %.9f) max|z|=%.6f"
              % (name, len(words), err.max(), words[i], words[i] & 0xFFFF, words[i] >> 16, got[i, 0], got[i, 1], ref[i, 0], ref[i, 1], np.abs(got).max()))
        if err.max() > worst[0]:
            worst = (float(err.max()), name, int(words[i]))
    print("RNG_BM max_abs_err=%.3e grid=%s word=0x%08x measured_before=%.3e bar=%.0e" % (worst[0], worst[1], worst[2], BM_MEASURED_MAX, BM_ABS_TOL))
    assert worst[0] <= BM_ABS_TOL


def test_every_normal_is_inside_the_bound_the_pruning_relies_on(grids):
    """|z| < POD_EPS_MAX (pod_merge_score.h: may_pass) for every radius at the angles where |cos| or |sin| is largest, for every angle at
    the largest radius (field 0), and on the rest of the grid.  The largest value is the lattice's, to the measured error."""
    words, got, _ = grids["radii"]
    q = np.isin(words >> 16, QUARTERS)
    assert q.sum() == 8 * 65536 and np.abs(got[q]).max() < rr.POD_EPS_MAX
    for _, g, _ in grids.values():
        assert np.abs(g).max() < rr.POD_EPS_MAX
    w, g, _ = grids["angles"]
    top = (w & 0xFFFF) == 0
    assert top.sum() == 65536 and np.abs(g[top]).max() < rr.POD_EPS_MAX
    assert abs(max(np.abs(got).max(), np.abs(g).max()) - rr.lattice_moments()["max_abs"]) <= BM_ABS_TOL


def test_grid_moments_equal_the_lattice(grids):
    """All 65 536 radii x 64 evenly spaced angles: E z^2 and E z^4 of the GPU's normals against the lattice's exact values.  The bar is
    what a per-element error of BM_ABS_TOL can move a mean by -- mean((|z| + d)^n - |z|^n) over the grid -- and nothing statistical."""
    lat = rr.lattice_moments()
    words, got, ref = grids["radii"]
    sel = slice(0, 64 * 65536)
    g, r = got[sel], np.abs(ref[sel])
    for n, name in ((2, "m2"), (4, "m4")):
        bar = float(np.mean((r + BM_ABS_TOL) ** n - r ** n)) + 1e-12
        assert abs(float(np.mean(ref[sel] ** n)) - lat[name]) < 1e-11                            # the referee's grid IS the lattice
        print("RNG_BM moment E z^%d gpu=%.9f lattice=%.9f diff=%.3e bar=%.3e" % (n, np.mean(g ** n), lat[name], np.mean(g ** n) - lat[name], bar))
        assert abs(float(np.mean(g ** n)) - lat[name]) <= bar
    assert abs(float(np.mean(g))) <= BM_ABS_TOL + 1e-12
    # all angles x 64 spread radii: the angle factor, against the referee on the same grid
    words, got, ref = grids["angles"]
    sel = slice(None), slice(0, 64)
    g, r = got.reshape(65536, 66, 2)[sel], ref.reshape(65536, 66, 2)[sel]
    for n in (2, 4):
        bar = float(np.mean((np.abs(r) + BM_ABS_TOL) ** n - np.abs(r) ** n)) + 1e-12
        assert abs(float(np.mean(g ** n)) - float(np.mean(r ** n))) <= bar


# ---- the classification map ----------------------------------------------------------------------------------------------------------
PYRAMID = [(8, 12), (4, 6), (2, 3), (1, 2), (1, 1)]          # a 64 x 96 frame, strides 8 .. 128: H W % 4 = 0, 0, 2, 2, 1
RAGGED = [(3, 5), (1, 3), (7, 7)]                            # H W % 4 = 3, 3, 1
DRAW_IDS = (5, 2 ** 31 + 3)
SEED = 0x5EED


def dump_cls(key, shapes, A, K, S):
    lib = hip.load()
    cfg = hip.PodConfig()
    cfg.n_levels, cfg.n_runs, cfg.num_anchors, cfg.num_classes, cfg.cls_samples, cfg.philox_seed = len(shapes), 1, A, K, S, key
    lv = (hip.PodLevel * hip.POD_MAX_LEVELS)()
    for l, (h, w) in enumerate(shapes):
        lv[l].H, lv[l].W = h, w
    out = []
    for l, (h, w) in enumerate(shapes):
        t = torch.full((S, h * w * A, K), float("nan"), device=DEV)
        hip.check(lib.pod_dump_cls_normals(cfg, lv, l, t.data_ptr(), hip.current_stream()), "pod_dump_cls_normals")
        out.append(t.cpu())
    return out


@pytest.mark.parametrize("S", [1, 3, 10, 64])
@pytest.mark.parametrize("K", [1, 7, 16])
def test_cls_normals_equal_the_host_map(K, S):
    """Every level of two ragged pyramids, two draw ids (one past 2^31); S = 10 puts a cell's samples across a call boundary, S = 3 and
    S = 1 put several cells into one call."""
    A = 9
    for shapes in (PYRAMID, RAGGED):
        for draw_id in DRAW_IDS:
            key = rr.hotpath_key(SEED, draw_id)
            for l, (got, (h, w)) in enumerate(zip(dump_cls(key, shapes, A, K, S), shapes)):
                assert torch.equal(got, expected_normals(rr.cls_normals(key, l, h * w, A, K, S))), (shapes, draw_id, l)


def test_hotpath_dumps_use_the_derived_key():
    """HotPath.dump_cls_normals / dump_box_normals (what test_native_exact_gpu.py feeds the oracle): _begin_draw's key, the product's
    geometry (five levels, A = 9, K = 7, S = 10, 1000 box samples)."""
    from tests.test_hip_parity import make_path
    ho = synthetic.planted_head_outputs((192, 256), 2, seed=4, num_boxes=6)
    hp = make_path(ho)
    A, K, S = hp.p.num_anchors, hp.p.num_classes, hp.p.cls_var_num_samples
    gids = torch.tensor([0, 1, hp.anchor_base[1], hp.anchor_base[-1], hp.R - 1], dtype=torch.int32)
    for draw_id in DRAW_IDS:
        key = rr.hotpath_key(hp.p.philox_seed, draw_id)
        for l, (got, (h, w)) in enumerate(zip(hp.dump_cls_normals(draw_id), hp.shapes)):
            assert torch.equal(got.cpu(), expected_normals(rr.cls_normals(key, l, h * w, A, K, S))), (draw_id, l)
        got = hp.dump_box_normals(draw_id, gids).cpu()
        assert torch.equal(got, expected_normals(rr.box_normals(key, gids.numpy(), hp.p.prop_num_samples)))


# ---- the box map ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [2, 3, 1000, 1024])
def test_box_normals_equal_the_host_map(S):
    """Global anchor ids 0, a level's base (the second level of a 768 x 1344 frame starts at 145 152), the last ids of that frame
    (R = 193 374) and one past 2^24 (no float ever carries an id)."""
    gids = np.array([0, 1, 145152, 193371, 193372, 193373, (1 << 24) + 1], dtype=np.int32)
    cfg = hip.PodConfig()
    cfg.prop_samples = S
    for draw_id in DRAW_IDS:
        cfg.philox_seed = key = rr.hotpath_key(SEED, draw_id)
        g = torch.from_numpy(gids).to(DEV)
        t = torch.full((S, len(gids), 4), float("nan"), device=DEV)
        hip.check(hip.load().pod_dump_box_normals(cfg, g.data_ptr(), len(gids), t.data_ptr(), hip.current_stream()), "pod_dump_box_normals")
        assert torch.equal(t.cpu(), expected_normals(rr.box_normals(key, gids, S)))


# ---- K21 / K27 -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fx():
    from tests.training import loss_ref as lr
    f = lr.load_fixture()
    f["shapes"], f["level_anchors"] = lr.fixture_geometry(f)
    return f


@pytest.mark.parametrize("S", [3, 10, 17])
def test_train_loss_draws_equal_the_host_map(fx, S):
    """K21's eps_out on the training fixture (two images, R = 1161, K = 7): rows with a label are the host map's normals -- S = 10 and 17
    take a second and third Philox call per class, the last one partly used --, ignored rows are zero."""
    from tests.training import test_torch_ops_gpu as t21
    ho = t21.head_outputs(fx, True)
    labels, matched, gb = t21.device_labels(fx)
    n_img, R = labels.shape
    assert n_img == 2
    key = rr.loss_key(1234, 2 ** 31 + 1)
    eps_out = torch.full((S, n_img * R, t21.K), float("nan"), device=DEV)
    losses.train_loss_sums(ho.cls, ho.delta, ho.cls_var, ho.reg_var, labels, matched, gb, ho.anchors, t21.A, t21.K, cls_samples=S, eps=None,
                           eps_out=eps_out, seed=key)
    img, r = np.divmod(np.arange(n_img * R), R)
    want = expected_normals(rr.loss_normals(key, r, img, t21.K, S))
    valid = (torch.from_numpy(fx["labels"]) >= 0).reshape(-1)
    assert 0 < int(valid.sum()) < valid.numel()
    want[:, ~valid] = 0.0
    assert torch.equal(eps_out.cpu(), want)


@pytest.mark.parametrize("M", [1, 6, 127, 128, 129, 301])
def test_energy_score_draws_equal_the_host_map(fx, M):
    """K27's eps_reg_out on the same fixture: M + 1 samples per positive anchor, M odd and even; from M = 127 on a lane takes a second trip
    and sample 128 -- the partner of lane 63's sample 127 -- comes from lane 0 of that trip.  Rows that are not positive are zero."""
    from tests.score_losses import score_ref as sr
    from tests.score_losses import test_torch_ops_gpu as t27
    case = sr.fixture_case(fx)
    pos = sr.Referee(case, 0.11).pos.reshape(-1)
    n_img, R = case["labels"].shape
    key = rr.loss_key(77, 3)
    eps_out = torch.full((M + 1, n_img * R, 4), float("nan"), device=DEV)
    t27.run(fx, case, "energy_loss", 0.11, M, eps_out=eps_out, seed=key, want_grads=False)
    img, r = np.divmod(np.arange(n_img * R), R)
    want = expected_normals(rr.reg_score_normals(key, r, img, M))
    assert 0 < int(pos.sum()) < pos.numel()
    want[:, ~pos] = 0.0
    assert torch.equal(eps_out.cpu(), want)
