"""The RNG contract, on the host: the restatement of tests/rng/rng_ref.py against Random123's known answers, the 16-bit Box-Muller
lattice evaluated exhaustively in fp64, injectivity of every counter map over the whole domain the entry points admit, the key
derivations of the Python side, and the refusal of what a counter field cannot hold.  The checkers are themselves checked: each is
handed a restatement broken on purpose and must reject it.  The GPU half (test_native_exact_gpu.py, test_predictor_gpu.py beside this
file) holds the kernels to the same restatement bit for bit."""
import ctypes

import numpy as np
import pytest

from tests.rng import rng_ref as rr

KAT = rr.KAT


def kat_passes(philox):
    return all(tuple(int(x) for x in philox(np.array(c), np.array(k))) == out for c, k, out in KAT)


def test_philox_known_answers():
    assert kat_passes(rr.philox4x32_10)
    c = np.array([k[0] for k in KAT])                       # and vectorised: rows are independent
    k = np.array([k[1] for k in KAT])
    assert rr.philox4x32_10(c, k).tolist() == [list(k[2]) for k in KAT]


@pytest.mark.parametrize("mutant", [dict(rounds=9), dict(m0=rr.M1, m1=rr.M0), dict(rounds=11)], ids=["9-rounds", "M0-M1-swapped", "11-rounds"])
def test_known_answers_reject_a_broken_generator(mutant):
    assert not kat_passes(lambda c, k: rr.philox4x32_10(c, k, **mutant))


def test_constants_are_the_headers():
    from pod_compare_amd import hip
    for name in ("POD_MAX_LEVELS", "POD_MAX_CLASSES", "POD_MAX_RUNS", "POD_MAX_PROP_SAMPLES", "POD_MAX_CLS_SAMPLES", "POD_MAX_REG_SAMPLES"):
        assert getattr(rr, name) == getattr(hip, name), name
    assert len(set(rr.STREAMS.values())) == len(rr.STREAMS)          # a stream word of its own per use: the maps cannot meet each other
    assert [v.to_bytes(4, "big") for v in rr.STREAMS.values()] == [b"cls\0", b"box\0", b"drop", b"los\0", b"reg\0"]


# ---- the lattice -------------------------------------------------------------------------------------------------------------------
def test_box_muller_lattice_moments_exhaustively():
    """65 536 radii x 65 536 angles: every normal the sampler can return.  The bound K1 / K1f prune with, and the sampler's exact
    moments ("RNG contract": what a statistical test should expect instead of 0, 1, 3)."""
    m = rr.lattice_moments()
    assert abs(m["max_abs"] - 4.85459) < 1e-5 and m["max_abs"] < rr.POD_EPS_MAX
    assert abs(m["max_abs"] - np.sqrt(-2.0 * np.log(2.0 ** -17))) < 1e-8          # the smallest u1 at the angle nearest a whole turn
    assert abs(m["m1"]) < 1e-12
    assert abs(m["m2"] - 0.9999947) < 1e-7
    assert abs(m["m4"] - 2.99979) < 1e-5
    rad, cs, sn = rr.lattice()
    n0, n1 = rr.box_muller16(np.array([0, 0xFFFF, 0xFFFF0000, 0xFFFFFFFF, 0x40000000 | 0x1234], dtype=np.uint64))
    f = np.array([0, 0xFFFF, 0, 0xFFFF, 0x1234])
    a = np.array([0, 0, 0xFFFF, 0xFFFF, 0x4000])
    assert np.array_equal(n0, rad[f] * cs[a]) and np.array_equal(n1, rad[f] * sn[a])      # low half: radius; high half: angle


# ---- injectivity -------------------------------------------------------------------------------------------------------------------
A_MAX = rr.POD_MAX_ANCHOR_SHAPES


def cls_parts(HWs, A, K, S, **kw):
    return [rr.cls_addr(l, hw, A, K, S, **kw) for l, hw in enumerate(HWs)]


@pytest.mark.parametrize("A,K,S", [(A_MAX, rr.POD_MAX_CLASSES, rr.POD_MAX_CLS_SAMPLES), (9, 7, 10), (9, 16, 1), (9, 16, 3), (9, 1, 63)])
def test_classification_map_is_injective(A, K, S):
    """All POD_MAX_LEVELS levels, cell counts = 0, 1, 2, 3 mod 4 (a level's last group of four cells is partial), the largest anchor-shape
    and class counts the entry points admit, the largest sample count: no two (level, cell, shape, class, sample) share a normal."""
    HWs = (8, 7, 6, 5, 4, 3, 2, 1)
    assert len(HWs) == rr.POD_MAX_LEVELS and {hw % 4 for hw in HWs} == {0, 1, 2, 3}
    assert rr.count_collisions(*cls_parts(HWs, A, K, S)) == 0


def test_box_map_is_injective():
    gids = np.concatenate([np.arange(0, 40), 193373 + np.arange(-20, 20), [2 ** 31 - 1]])
    for S in (2, 3, 1000, rr.POD_MAX_PROP_SAMPLES):
        assert rr.count_collisions(rr.box_addr(gids, S)) == 0


def test_loss_maps_are_injective():
    r, img = np.meshgrid(np.concatenate([np.arange(40), [193373]]), np.arange(3), indexing="ij")
    assert rr.count_collisions(rr.loss_addr(r.ravel(), img.ravel(), rr.POD_MAX_CLASSES - 1, rr.POD_MAX_CLS_SAMPLES)) == 0      # K21: K <= 15
    r, img = np.meshgrid(np.array([0, 1, 2, 193373]), np.arange(3), indexing="ij")
    for M in (1, 2, 127, rr.POD_MAX_REG_SAMPLES):
        assert rr.count_collisions(rr.reg_score_addr(r.ravel(), img.ravel(), M)) == 0
    # one ProbabilisticLosses call hands K21 and K27 the same key: their stream words keep them apart
    assert rr.count_collisions(rr.loss_addr(r.ravel(), img.ravel(), 7, 10), rr.reg_score_addr(r.ravel(), img.ravel(), 10)) == 0


def field_collisions(*parts):
    """parts: dropout_fields results; a 16-bit field is (call counter, c2, field)."""
    ctr = np.concatenate([p[0].reshape(-1) for p in parts])
    rows = rr.pack_rows([ctr - ctr.min(), np.concatenate([p[1].reshape(-1) for p in parts]), np.concatenate([p[2].reshape(-1) for p in parts])])
    return int(rows.size - np.unique(rows).size)


@pytest.mark.parametrize("n", [1, 3, 4, 5, 7, 8, 8 * 257 + 3, 8 * 257 + 6])
def test_dropout_groups_tail_and_replicas_share_no_field(n):
    """One counter block: the tensor in place (groups + its n % 4 tail) and three replicas of its whole groups, same offset."""
    off = 5 << 34
    parts = [rr.dropout_fields(off, n, "inplace")]
    if n >= 4:
        parts.append(rr.dropout_fields(off, n - n % 4, "replicas", copies=3))
    assert field_collisions(*parts) == 0
    assert parts[0][2].max() <= 7


def test_dropout_blocks_of_consecutive_layers_do_not_overlap():
    """Layer l of the head keys its whole buffer -- every level, every copy -- by the element's index in it, from offset l << 34.  The
    largest buffer the Winograd path can be asked for: a first level whose one image just fits wino.MAX_CANVAS_BYTES, the pyramid of
    halved levels below it, 127 copies (the store pass's limit).  Its last Philox call stays inside the layer's 2^34 calls, the
    per-level offsets included.  (A buffer that crossed into the next block would hold 2^37 floats, 512 GiB: more than the device has.)"""
    from pod_compare_amd import wino
    C, copies = 256, 127
    h = w = int((wino.MAX_CANVAS_BYTES // (4 * C)) ** 0.5)
    assert h * w * C * 4 <= wino.MAX_CANVAS_BYTES < (h + 1) * (w + 1) * C * 4
    levels = [(h, w)]
    while levels[-1] != (1, 1):
        levels.append(((levels[-1][0] + 1) // 2, (levels[-1][1] + 1) // 2))
    offs = wino.level_pixel_offsets(levels, copies)
    for layer in (1, 2):
        base = rr.head_offset(layer)
        starts = [rr.level_offset(base, offs[i], C) for i in range(len(levels))]
        ends = [s + (copies * lh * lw * C + 7) // 8 for s, (lh, lw) in zip(starts, levels)]        # one call per 8 floats
        assert starts[0] == base and all(e <= s for e, s in zip(ends, starts[1:]))               # levels follow each other
        assert ends[-1] <= rr.head_offset(layer + 1)
    assert rr.head_offset(2) - rr.head_offset(1) == 1 << 34


# ---- the checkers catch what they are for ------------------------------------------------------------------------------------------
def test_injectivity_checker_rejects_an_anchor_shape_left_out_of_c1():
    broken = lambda level, a, k: (level << np.uint64(16)) | k
    assert rr.count_collisions(*cls_parts((8, 7), 9, 7, 10, c1=broken)) > 0
    assert rr.count_collisions(*cls_parts((8, 7), 9, 7, 10)) == 0


def test_injectivity_checker_rejects_an_anchor_shape_past_its_field():
    """What pod_cls_counter_fields_ok refuses: shape 256 of class 0 is shape 0 of the next level's class 0."""
    assert rr.count_collisions(*cls_parts((4, 4), rr.POD_MAX_ANCHOR_SHAPES + 1, 2, 1)) > 0


def test_field_checker_rejects_a_tail_drawn_with_c2_0():
    """c2 = 1 matters only BETWEEN tensors keyed from the same offset.  Inside one tensor a tail can never meet a group whatever its c2:
    its calls offset + n4 + t lie past the groups' calls offset .. offset + (n4 - 1) / 2, which is why
    test_dropout_groups_tail_and_replicas_share_no_field would not see this mutant.  They are the calls of groups 2 (n4 + t) of a longer
    tensor from the same offset, and there only c2 keeps them apart: that pair is what the checker is handed."""
    n, off = 8 * 257 + 3, 0
    longer = rr.dropout_fields(off, 4 * n, "inplace")
    assert field_collisions(rr.dropout_fields(off, n, "inplace"), longer) == n - n % 4         # (the whole groups are the same elements)
    assert field_collisions(rr.dropout_fields(off, n, "inplace", tail_c2=0), longer) == n      # ... and now the three tail elements too


def test_field_checker_rejects_replicas_keyed_without_copy():
    broken = lambda copy, n4, g: g + np.uint64(0) * copy
    assert field_collisions(rr.dropout_fields(0, 64, "replicas", copies=3, replica_group=broken)) == 2 * 64
    assert field_collisions(rr.dropout_fields(0, 64, "replicas", copies=3)) == 0


# ---- the mask rule's pieces --------------------------------------------------------------------------------------------------------
def test_dropout_keep_pieces():
    assert [rr.thresh16(p) for p in (0.0, 0.1, 0.2, 0.5)] == [0, 6553, 13107, 32768]          # uint32(fp32(p) * 65536)
    assert rr.dropout_keep(1, 0, 37, 0.0, "inplace").all()
    n, seed, off = 8 * 257 + 3, 0x0D50ED, 3 << 34
    keep = rr.dropout_keep(seed, off, n, 0.2, "inplace")
    assert keep.shape == (n,) and 0.75 < keep.mean() < 0.85
    # the whole groups of a tensor do not depend on its length; the tail does not depend on them
    assert np.array_equal(keep[:n - 3], rr.dropout_keep(seed, off, n - 3, 0.2, "inplace"))
    # an epoch word of 0 is no epoch; another one is another key
    rep = rr.dropout_keep(seed, off, 64, 0.5, "replicas", copies=3)
    assert np.array_equal(rep, rr.dropout_keep(seed, off, 64, 0.5, "replicas", copies=3, epoch=0))
    assert not np.array_equal(rep, rr.dropout_keep(seed, off, 64, 0.5, "replicas", copies=3, epoch=1))
    assert rr.dropout_key(seed, (1 << 40) + 7) == seed ^ ((((1 << 40) + 7) * 0x9E3779B97F4A7C15) % (1 << 64))
    # copy c of the replicas = the groups c n4 .. of one long replica
    assert np.array_equal(rep.reshape(-1), rr.dropout_keep(seed, off, 192, 0.5, "replicas", copies=1).reshape(-1))


# ---- keys --------------------------------------------------------------------------------------------------------------------------
def test_key_derivations_match_the_python_side(monkeypatch):
    """rng_ref's formulas are the product's: HotPath._begin_draw, ProbabilisticLosses.__call__ (read off their effects, no GPU)."""
    import torch
    from pod_compare_amd import hip, hotpath, losses
    hp = hotpath.HotPath.__new__(hotpath.HotPath)
    hp.p, hp.cfg, hp._draws = hotpath.PathParams(philox_seed=0x123456789ABCDEF0), hip.PodConfig(), 41
    for draw_id in (0, 7, 2 ** 31 + 3, None):
        hp._begin_draw(draw_id)
        assert hp.cfg.philox_seed == rr.hotpath_key(0x123456789ABCDEF0, 41 if draw_id is None else draw_id)
    assert hp._draws == 42
    seen = []

    def launch(meta, w, *tensors):                       # stands in for the two launches: records the key they would get
        seen.append(meta["seed"])
        meta["sums"] = None
        return None, None

    monkeypatch.setattr(losses._TrainLoss, "apply", staticmethod(launch))

    class Head:
        cls, delta, cls_var, reg_var, anchors, num_anchors, num_classes = [torch.zeros(1)], [torch.zeros(1)], None, None, None, 9, 7

    crit = losses.ProbabilisticLosses(num_classes=7, seed=0x1_0000_0005)
    crit.draws = 2 ** 32 - 2
    for _ in range(3):
        crit(Head, torch.zeros(1, 1, dtype=torch.int32), torch.zeros(1, 1, dtype=torch.int32), torch.zeros(0, 4), normalizer=1.0)
    assert seen == [rr.loss_key(0x1_0000_0005, d) for d in (2 ** 32 - 2, 2 ** 32 - 1, 2 ** 32)]
    assert seen[0] == 5 | ((2 ** 32 - 2) << 32) and seen[2] == 5                                   # (the counter wraps at 2^32 calls)


def test_ensemble_draw_ids_match_the_python_side(monkeypatch):
    """PostNmsEnsemble.run hands member j the draw id rng_ref.ensemble_draw_id names (a stand-in workspace records it; no GPU)."""
    import torch
    from pod_compare_amd import hip, hotpath

    class Lib:
        def __getattr__(self, name):
            return lambda *a: 0

    class Workspace:                                     # what run() touches of a HotPath; buffers are null pointers here
        lib, has_cls_var, cov_dims, has_covariance = Lib(), False, 0, False

        def __init__(self):
            self.ids = []

        def candidates(self, *a, draw_id=None):
            self.ids.append(draw_id)

        def decode(self, *a):
            pass

        def nms(self):
            pass

        def finalize(self, *a):
            return None

        def __getattr__(self, name):
            return None

    monkeypatch.setattr(hip, "current_stream", lambda: 0)
    ens = hotpath.PostNmsEnsemble.__new__(hotpath.PostNmsEnsemble)
    ens.hp, ens.n_members, ens.cap, ens.total = Workspace(), 5, 500, torch.zeros(1, dtype=torch.int32)
    for name in ("m_boxes", "m_cov", "m_classes", "m_probs", "seeds", "n_seeds", "c_boxes", "c_cov", "c_scores", "c_classes", "c_probs", "keep",
                 "n_keep", "scratch"):
        setattr(ens, name, None)
    members = [(None, None, None, None)] * 5
    for draw_id in (0, 3, 2 ** 31 + 3):
        ens.hp.ids = []
        ens.run(members, image_size=(8, 8), out_size=(8, 8), draw_id=draw_id)
        assert ens.hp.ids == [rr.ensemble_draw_id(draw_id, 5, j) for j in range(5)]
    ens.hp.ids = []
    ens.run(members, image_size=(8, 8), out_size=(8, 8))
    assert ens.hp.ids == [None] * 5                       # no id: the workspace's own counter, one step per member (_begin_draw above)


def test_head_offsets_match_the_python_side(monkeypatch):
    """The head's counter blocks and per-level offsets are rng_ref.head_offset / level_offset: the launch plan of the Winograd path
    (_trunk_plan), the per-level pod_expand_dropout calls that stand in for the store pass's replicas (_launch), and the fused passes
    of the MIOpen path (_trunk, _relu_dropout) -- read off a stand-in library that records its arguments; no GPU."""
    import torch
    from pod_compare_amd import hip, modeling, wino
    calls = []

    class Lib:
        def __getattr__(self, name):
            return lambda *a: calls.append((name, a)) or 0

    monkeypatch.setattr(hip, "load", lambda: Lib())
    monkeypatch.setattr(hip, "current_stream", lambda: 0)
    levels, C = [(12, 20), (6, 10), (3, 5)], 64
    pixels = sum(h * w for h, w in levels)
    head = modeling.ProbabilisticRetinaNetHead(in_channels=C, num_convs=4, dropout_rate=0.1, compute_cls_var=True, compute_bbox_cov=True)
    # ---- the plan: subnet i's layer l draws block base + i L + l + 1
    head._drop_calls = 7
    x0 = torch.zeros(pixels, C)
    st = modeling.HeadPlan(x0=x0, levels=levels, grouped=False, dropout=True)
    plan = head._trunk_plan([(0, 4), (1, 6)], st)
    assert [[s["offset"] for s in sets] for sets in plan["layers"]] == [[rr.head_offset(7 + i * 4 + l + 1) for i in range(2)] for l in range(4)]
    assert head._drop_calls == 15
    # ---- a first layer whose copies are stored level by level: offset + first float of the level's slab / 8
    class Conv:                                          # a convolution outside the split kernel: y = its input, C channels
        split, C = False, 64

        def __call__(self, src, dst, table, **kw):
            return src

    monkeypatch.setattr(head, "_wino", lambda conv: conv)
    first = dict(plan["layers"][0][1], conv=Conv())
    assert first["replicas"] == 6
    head._launch([first], st, **plan["kw"])
    offr = wino.level_pixel_offsets(levels, 6)
    got = [(name, a[2], a[3], a[6]) for name, a in calls]
    assert got == [("pod_expand_dropout", h * w * C, 6, rr.level_offset(first["offset"], offr[i], C)) for i, (h, w) in enumerate(levels)]
    # ---- the fused in-place pass of the MIOpen path: one block per call
    calls.clear()
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    head._relu_dropout(torch.zeros(8))
    head._relu_dropout(torch.zeros(8))
    assert [(name, a[4]) for name, a in calls] == [("pod_relu_dropout", rr.head_offset(16)), ("pod_relu_dropout", rr.head_offset(17))]


def test_keys_of_distinct_draws_are_distinct():
    seed = 0x5EED
    ids = list(range(64)) + [2 ** 31 - 1, 2 ** 31, 2 ** 31 + 3, 2 ** 32 - 1]
    assert len({rr.hotpath_key(seed, d) for d in ids}) == len(ids)
    # the members of an ensemble, this image's and the next's
    for n_members in (1, 5, 64):
        keys = [rr.hotpath_key(seed, rr.ensemble_draw_id(img, n_members, j)) for img in (0, 1, 2, 1000) for j in range(n_members)]
        assert len(set(keys)) == len(keys)
    assert rr.ensemble_draw_id(3, 5, 4) + 1 == rr.ensemble_draw_id(4, 5, 0)
    # the loss's draws counter, and two ranks (seed + rank): no (rank, draw) meets another, in particular not the other rank's next draw
    keys = {(rank, d): rr.loss_key(1234 + rank, d) for rank in range(8) for d in range(64)}
    assert len(set(keys.values())) == len(keys)
    assert rr.loss_key(1234 + 0, 1) != rr.loss_key(1234 + 1, 0)
    # dropout: a rank's key is dropout_seed + rank, a layer's counters its own 2^34 block: rank r's call c + 1 is not rank r + 1's call c
    head_seed = 0x0D50ED
    assert len({(rr.dropout_key(head_seed + rank), rr.head_offset(c)) for rank in range(8) for c in range(64)}) == 8 * 64
    assert len({rr.dropout_key(head_seed, e) for e in (None, 1, 2, (1 << 40) + 7, 1 << 32, (1 << 32) + 1)}) == 6


# ---- what a counter field cannot hold is refused -----------------------------------------------------------------------------------
def refusal_inputs():
    """(lib, X, levels, cfg): five levels of 1 x 1 cells whose every plane pointer is set, and a cfg that passes every other check of
    the entry points below -- so that POD_E_INVALID can only be the answer to the anchor-shape count.  (Were that check missing, a call
    would go on to its launch; nothing here is ever dereferenced on the host.)"""
    from pod_compare_amd import build, hip
    build.build_library()
    lib = hip.load()
    buf = ctypes.create_string_buffer(128)
    X = (ctypes.addressof(buf) + 63) & ~63
    lv = (hip.PodLevel * hip.POD_MAX_LEVELS)()
    for l in range(5):
        lv[l].cls = lv[l].cls_var = lv[l].delta = lv[l].reg_var = X
        lv[l].H = lv[l].W = 1
        lv[l].run_stride_cls = lv[l].run_stride_delta = lv[l].run_stride_reg = 4
        lv[l].anchor_base = l

    def cfg(A, **kw):
        c = hip.PodConfig()
        c.n_levels, c.n_runs, c.num_anchors, c.num_classes, c.cov_dims, c.has_cls_var = 5, 1, A, 7, 4, 1
        c.cls_samples, c.prop_samples, c.topk, c.score_thresh = 10, 1000, 1000, 0.05
        for k, v in kw.items():
            setattr(c, k, v)
        return c
    return lib, X, lv, cfg


def test_entry_points_refuse_an_anchor_shape_count_its_field_cannot_hold():
    """c1 = level << 16 | a << 8 | k: 8 bits for the anchor shape.  Every entry point that may draw classification normals returns
    POD_E_INVALID for num_anchors = 257 before anything is launched, on inputs where no other check can answer (refusal_inputs).
    pod_merge_score_fused has refused more than 255 all along (8 bits of its LDS record); the class and level fields are covered by
    POD_MAX_CLASSES / POD_MAX_LEVELS, far inside 8 and 16 bits.  What is ACCEPTED -- 256 shapes, or any count where nothing is drawn --
    is in test_counter_check_accepts_what_forms_no_aliasing_counter: an accepted call would launch."""
    lib, X, lv, cfg = refusal_inputs()
    bad = cfg(257)
    assert lib.pod_dump_cls_normals(bad, lv, 0, X, None) == -1
    assert lib.pod_dump_cls_normals(cfg(0), lv, 0, X, None) == -1
    assert lib.pod_mc_merge_score(bad, lv, X, X, X, X, X, X, X, None) == -1              # prune mode (maybe_bits given)
    assert lib.pod_mc_merge_score(bad, lv, X, X, X, X, X, X, None, None) == -1           # dense scoring with native draws
    assert lib.pod_score_maybe(bad, lv, X, X, X, X, X, X, None) == -1
    assert lib.pod_merge_score_fused(bad, lv, X, X, X, X, X, None) == -1
    assert lib.pod_gather_candidates(bad, lv, *([X] * 15 + [None])) == -1
    assert lib.pod_gather_decode(bad, lv, *([X] * 17 + [None])) == -1


def test_counter_check_accepts_what_forms_no_aliasing_counter(tmp_path):
    """pod_cls_counter_ok itself (csrc/pod_merge_score.h, compiled for the host): 256 shapes pass; 257 are refused exactly when there is a
    variance head and at least one level draws in-kernel (no eps_cls to replay); pod_merge_score_cfg_ok admits any count, as before."""
    import os
    import subprocess
    from pod_compare_amd import build
    src = tmp_path / "counter_ok.hip"
    src.write_text('''#include "pod_merge_score.h"
#include <stdio.h>
int main() {
    PodConfig c{};
    PodLevel lv[POD_MAX_LEVELS]{};
    c.n_levels = 5; c.n_runs = 1; c.num_classes = 7; c.cls_samples = 10;
    float x;
    for (int A = 256; A <= 257; ++A)
        for (int var = 0; var <= 1; ++var)
            for (int replay = 0; replay <= 5; ++replay) {      // the first `replay` levels replay their normals
                c.num_anchors = A; c.has_cls_var = var;
                for (int l = 0; l < 5; ++l) lv[l].eps_cls = l < replay ? &x : nullptr;
                printf("%d %d %d %d %d\\n", A, var, replay, (int)pod_cls_counter_ok(&c, lv), (int)pod_merge_score_cfg_ok(&c));
            }
    return 0;
}
''')
    exe = tmp_path / "counter_ok"
    subprocess.check_call([build._hipcc(), "--offload-arch=gfx950", "--cuda-host-only", "-std=c++17", "-I", build.CSRC, str(src), "-o", str(exe)])
    rows = [tuple(int(x) for x in line.split()) for line in subprocess.check_output([str(exe)]).decode().splitlines()]
    assert len(rows) == 24
    for A, var, replay, counter_ok, cfg_ok in rows:
        assert cfg_ok == 1
        assert counter_ok == (0 if A == 257 and var == 1 and replay < 5 else 1), (A, var, replay)


def test_debug_entries_reject_invalid_arguments_without_a_gpu():
    lib, X, _, _ = refusal_inputs()
    assert lib.pod_debug_philox4x32(None, X, 1, None) == -1 and lib.pod_debug_philox4x32(X, None, 1, None) == -1
    assert lib.pod_debug_philox4x32(X, X, -1, None) == -1 and lib.pod_debug_philox4x32(X, X, 0, None) == 0
    assert lib.pod_debug_box_muller16(None, X, 1, None) == -1 and lib.pod_debug_box_muller16(X, None, 1, None) == -1
    assert lib.pod_debug_box_muller16(X, X, -1, None) == -1 and lib.pod_debug_box_muller16(X, X, 0, None) == 0
