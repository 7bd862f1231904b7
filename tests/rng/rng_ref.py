"""Host restatement of the project's random draws (numpy, uint64 / fp64; no torch): the referee of tests/rng/.

Everything stochastic the kernels do is a function of a Philox4x32-10 (counter, key) pair.  This module states, independently of the HIP
code and from the prose of csrc/pod_device.h, pod_merge_score.h, pod_candidate.h, k21_train_loss.hip, k27_reg_score_loss.hip and
include/pod_mi355x.h:

  * the generator (`philox4x32_10`) and the word -> two normals step (`box_muller16`, fp64);
  * the counter maps of the four normal streams, each in two forms: `*_addr` returns the raw addressing -- the counter (.., 4) uint32 and
    the component 0..7 of the call, in the layout the GPU writes -- for the injectivity tests; `*_normals` returns the 32-bit word and
    which of its two normals an element takes, for the bit-for-bit GPU comparisons (host words -> the kernels' own box_muller16 -> layout);
  * the dropout mask rule (`dropout_fields`: addressing; `dropout_keep`: the keep mask);
  * the key derivations of the Python side (`hotpath_key`, `ensemble_draw_id`, `loss_key`, `head_offset`, `level_offset`, `dropout_key`).

A component c of a call is normal c & 1 (0: radius * cos, 1: radius * sin) of output word c >> 1.

The keyword hooks (`rounds`, `m0`, `m1`, `c1`, `tail_c2`, `replica_group`) exist for the mutation cases of test_rng_ref_cpu.py alone: the
checkers must reject a restatement that is broken on purpose.
"""
import numpy as np

# include/pod_mi355x.h
POD_MAX_LEVELS, POD_MAX_CLASSES, POD_MAX_RUNS = 8, 16, 64
POD_MAX_PROP_SAMPLES, POD_MAX_CLS_SAMPLES, POD_MAX_REG_SAMPLES = 1024, 64, 4096
POD_MAX_ANCHOR_SHAPES = 256          # pod_merge_score.h: pod_cls_counter_ok (8 bits of c1); pod_merge_score_fused stops at 255
POD_EPS_MAX = 4.9                    # pod_device.h

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
STREAM_CLS, STREAM_BOX, STREAM_DROPOUT = 0x636c7300, 0x626f7800, 0x64726f70
STREAM_LOSS, STREAM_REG_SCORE = 0x6c6f7300, 0x72656700
STREAMS = dict(cls=STREAM_CLS, box=STREAM_BOX, dropout=STREAM_DROPOUT, loss=STREAM_LOSS, reg_score=STREAM_REG_SCORE)
MASK32, MASK64 = 0xFFFFFFFF, 0xFFFFFFFFFFFFFFFF
EPOCH_MIX = 0x9E3779B97F4A7C15

# Random123's known answers for Philox4x32-10: (counter, key, output)
KAT = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
       ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
       ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]


def _u64(x):
    return np.asarray(x, dtype=np.uint64)


def philox4x32_10(counter, key, rounds=10, m0=M0, m1=M1):
    """Random123's Philox4x32-10, vectorised: counter (..., 4), key (..., 2) (broadcast against each other) -> (..., 4) uint32."""
    c, k = _u64(counter), _u64(key)
    lead = np.broadcast_shapes(c.shape[:-1], k.shape[:-1])
    c, k = np.broadcast_to(c, lead + (4,)), np.broadcast_to(k, lead + (2,))
    m = np.uint64(MASK32)
    x, y, z, w = (c[..., i] & m for i in range(4))
    k0, k1 = k[..., 0] & m, k[..., 1] & m
    for _ in range(rounds):
        p0, p1 = np.uint64(m0) * x, np.uint64(m1) * z          # 32 x 32 -> 64 bits: no overflow in uint64
        x, y, z, w = (p1 >> np.uint64(32)) ^ y ^ k0, p1 & m, (p0 >> np.uint64(32)) ^ w ^ k1, p0 & m
        k0, k1 = (k0 + np.uint64(W0)) & m, (k1 + np.uint64(W1)) & m
    return np.stack([x, y, z, w], axis=-1).astype(np.uint32)


def key_words(key):
    """A 64-bit Philox key as the kernels split it: (low word, high word)."""
    key = int(key) & MASK64
    return np.array([key & MASK32, key >> 32], dtype=np.uint64)


def box_muller16(word):
    """The two normals of a 32-bit word, fp64: u = (16-bit field + 0.5) / 65536; radius sqrt(-2 ln u1) from the LOW half, angle
    2 pi u2 from the HIGH half; n0 = radius cos, n1 = radius sin."""
    w = _u64(word)
    u1 = ((w & np.uint64(0xFFFF)).astype(np.float64) + 0.5) / 65536.0
    u2 = ((w >> np.uint64(16)).astype(np.float64) + 0.5) / 65536.0
    rad = np.sqrt(-2.0 * np.log(u1))
    return rad * np.cos(2.0 * np.pi * u2), rad * np.sin(2.0 * np.pi * u2)


def lattice():
    """The sampler's whole range, factorised: (radius[65536], cos[65536], sin[65536]) in fp64, indexed by the 16-bit field."""
    f = (np.arange(65536, dtype=np.float64) + 0.5) / 65536.0
    return np.sqrt(-2.0 * np.log(f)), np.cos(2.0 * np.pi * f), np.sin(2.0 * np.pi * f)


def lattice_moments():
    """Exact moments of a normal drawn uniformly from the 2^32 words (both normals of a word pooled; by the lattice's symmetry either
    alone gives the same): dict(max_abs, m1, m2, m4).  E[z^n] factorises into a radius mean and an angle mean."""
    rad, cs, sn = lattice()
    out = dict(max_abs=float(rad.max() * max(np.abs(cs).max(), np.abs(sn).max())))
    for name, n in (("m1", 1), ("m2", 2), ("m4", 4)):
        out[name] = float(np.mean(rad ** n) * 0.5 * (np.mean(cs ** n) + np.mean(sn ** n)))
    return out


def _finish(ctr_cols, comp, stream):
    lead = comp.shape
    ctr = np.stack([np.broadcast_to(_u64(c), lead) for c in ctr_cols] + [np.full(lead, stream, dtype=np.uint64)], axis=-1)
    return ctr.astype(np.uint32), comp.astype(np.uint8)


def _words(ctr, comp, key):
    """(counter, component) -> (the output word an element's normal comes from, 0 / 1: which normal of the word)."""
    out = philox4x32_10(ctr, key_words(key))
    word = np.take_along_axis(out, (comp >> 1).astype(np.int64)[..., None], axis=-1)[..., 0]
    return word, comp & 1


# ---- classification draws: pod_merge_score.h class_prob_cell (K1 / K1b / K1f / K2b) ----------------------------------------------
def cls_c1(level, a, k):
    return (level << np.uint64(16)) | (a << np.uint64(8)) | k


def cls_addr(level, HW, A, K, S, c1=cls_c1):
    """(S, HW * A, K): normal q = (hw & 3) S + s of the group of four cells hw >> 2 is component q & 7 of the call with counter
    (hw >> 2, level << 16 | a << 8 | k, q >> 3, STREAM_CLS); row r = hw A + a."""
    s = np.arange(S, dtype=np.uint64)[:, None, None]
    r = np.arange(HW * A, dtype=np.uint64)[None, :, None]
    k = np.arange(K, dtype=np.uint64)[None, None, :]
    hw, a = r // np.uint64(A), r % np.uint64(A)
    q = np.broadcast_to((hw & np.uint64(3)) * np.uint64(S) + s, (S, HW * A, K))
    return _finish([hw >> np.uint64(2), c1(np.uint64(level), a, k), q >> np.uint64(3)], q & np.uint64(7), STREAM_CLS)


def cls_normals(key, level, HW, A, K, S):
    return _words(*cls_addr(level, HW, A, K, S), key)


# ---- box-delta draws: pod_candidate.h decode_candidate / generate_samples (K3) ---------------------------------------------------
def box_addr(gids, S):
    """(S, n, 4): sample s of global anchor id gid takes components (s & 1) 4 .. + 3 of the call (gid, s >> 1, 0, STREAM_BOX)."""
    g = _u64(gids).reshape(1, -1, 1)
    s = np.arange(S, dtype=np.uint64)[:, None, None]
    j = np.arange(4, dtype=np.uint64)[None, None, :]
    comp = np.broadcast_to((s & np.uint64(1)) * np.uint64(4) + j, (S, g.shape[1], 4))
    return _finish([g, s >> np.uint64(1), np.uint64(0)], comp, STREAM_BOX)


def box_normals(key, gids, S):
    return _words(*box_addr(gids, S), key)


# ---- K21: classification samples of the training loss ----------------------------------------------------------------------------
def loss_addr(r, img, K, S):
    """(S, n, K) for rows (r[i], img[i]): sample s of class k is component s & 7 of the call (r, img, k | (s >> 3) << 8, STREAM_LOSS);
    r = the anchor's index within the R anchors of an image."""
    r, img = _u64(r).reshape(1, -1, 1), _u64(img).reshape(1, -1, 1)
    s = np.arange(S, dtype=np.uint64)[:, None, None]
    k = np.arange(K, dtype=np.uint64)[None, None, :]
    comp = np.broadcast_to(s & np.uint64(7), (S, r.shape[1], K))
    return _finish([r, img, k | ((s >> np.uint64(3)) << np.uint64(8))], comp, STREAM_LOSS)


def loss_normals(key, r, img, K, S):
    return _words(*loss_addr(r, img, K, S), key)


# ---- K27: box-delta samples of the energy score ------------------------------------------------------------------------------------
def reg_score_addr(r, img, M):
    """(M + 1, n, 4): samples 2c and 2c + 1 of an anchor are the eight components of the call (r, img, c, STREAM_REG_SCORE)."""
    r, img = _u64(r).reshape(1, -1, 1), _u64(img).reshape(1, -1, 1)
    s = np.arange(M + 1, dtype=np.uint64)[:, None, None]
    j = np.arange(4, dtype=np.uint64)[None, None, :]
    comp = np.broadcast_to((s & np.uint64(1)) * np.uint64(4) + j, (M + 1, r.shape[1], 4))
    return _finish([r, img, s >> np.uint64(1)], comp, STREAM_REG_SCORE)


def reg_score_normals(key, r, img, M):
    return _words(*reg_score_addr(r, img, M), key)


# ---- dropout masks: pod_device.h, "the WHOLE rule" -----------------------------------------------------------------------------------
def thresh16(p):
    """keep iff the element's 16-bit field >= uint32(p * 2^16), p taken as the fp32 the entry points receive."""
    return int(float(np.float32(p)) * 65536.0)


def dropout_scale(p):
    """1 / (1 - p) as the kernels form it, in fp32."""
    return np.float32(1.0) / (np.float32(1.0) - np.float32(p))


def dropout_key(seed, epoch=None):
    seed = int(seed) & MASK64
    return seed if epoch is None else seed ^ ((int(epoch) * EPOCH_MIX) & MASK64)


def replica_group(copy, n4, g):
    return copy * n4 + g


def dropout_fields(offset, n, kind, copies=1, tail_c2=1, replica_group=replica_group):
    """Addressing of the mask of a flat tensor of n floats: (call counter uint64, c2, field 0..7), each of shape (n,) for kind "inplace"
    and (copies, n) for kind "replicas" (n % 4 == 0 there).  Float4 group g owns fields 4 (g & 1) .. + 3 of the call offset + (g >> 1)
    (field f = half f & 1 of word f >> 1); c2 = 0 in place, 2 for the replicas, whose group index is copy * n4 + g; tail element t of
    the n % 4 takes field 0 of the call offset + n4 + t with c2 = 1."""
    n4 = n // 4
    e = np.arange(n, dtype=np.uint64)
    g, j = e >> np.uint64(2), e & np.uint64(3)
    if kind == "replicas":
        assert n % 4 == 0
        g = replica_group(np.arange(copies, dtype=np.uint64)[:, None], np.uint64(n4), g[None, :])
        j = np.broadcast_to(j, g.shape)
        c2 = np.full(g.shape, 2, dtype=np.uint64)
    else:
        assert kind == "inplace" and copies == 1
        c2 = np.zeros(n, dtype=np.uint64)
    ctr = (np.uint64(int(offset) & MASK64) + (g >> np.uint64(1))) & np.uint64(MASK64)
    field = np.uint64(4) * (g & np.uint64(1)) + j
    if kind == "inplace" and n % 4:
        t = np.arange(n % 4, dtype=np.uint64)
        ctr[4 * n4:] = np.uint64((int(offset) + n4) & MASK64) + t
        c2[4 * n4:] = tail_c2
        field[4 * n4:] = 0
    return ctr, c2, field


def dropout_keep(seed, offset, n, p, kind, copies=1, epoch=None):
    """bool keep mask: (n,) for "inplace", (copies, n) for "replicas"; p = 0 (thresh16 = 0) keeps everything."""
    ctr, c2, field = dropout_fields(offset, n, kind, copies)
    counter = np.stack([ctr & np.uint64(MASK32), ctr >> np.uint64(32), c2, np.full(ctr.shape, STREAM_DROPOUT, dtype=np.uint64)], axis=-1)
    out = philox4x32_10(counter, key_words(dropout_key(seed, epoch))).astype(np.uint64)
    word = np.take_along_axis(out, (field >> np.uint64(1)).astype(np.int64)[..., None], axis=-1)[..., 0]
    bits = (word >> (np.uint64(16) * (field & np.uint64(1)))) & np.uint64(0xFFFF)
    return bits >= np.uint64(thresh16(p))


# ---- the Python side's keys --------------------------------------------------------------------------------------------------------
def hotpath_key(seed, draw_id):
    """HotPath._begin_draw: low word = the seed's two halves folded together, high word = the draw id (mod 2^32)."""
    seed = int(seed)
    return ((seed ^ (seed >> 32)) & MASK32) | ((int(draw_id) & MASK32) << 32)


def ensemble_draw_id(draw_id, n_members, j):
    return int(draw_id) * int(n_members) + int(j)


def loss_key(seed, draws):
    """ProbabilisticLosses.__call__: (seed & 0xFFFFFFFF) | draws << 32; K21 and K27 of one call share it (their stream words differ)."""
    return (int(seed) & MASK32) | ((int(draws) & MASK32) << 32)


def head_offset(calls):
    """The head's counter block of its `calls`-th masked layer: 2^34 Philox calls = 2^37 floats."""
    return int(calls) << 34


def level_offset(offset, first_pixel, C):
    """The store pass keys an element by its index in the layer's whole buffer; pod_expand_dropout called per level reaches the same
    counters with offset + (first float of the level's slab) / 8."""
    return int(offset) + int(first_pixel) * int(C) // 8


# ---- checkers ----------------------------------------------------------------------------------------------------------------------
def pack_rows(cols):
    """Columns of non-negative integers -> one uint64 per row, exactly (raises if the columns' ranges do not fit 64 bits)."""
    cols = [_u64(c).reshape(-1) for c in cols]
    out, used = np.zeros(cols[0].shape, dtype=np.uint64), 0
    for c in cols:
        c = c - c.min()                                  # (a shift per column keeps equal rows equal and distinct rows distinct)
        bits = int(c.max()).bit_length()
        if used + bits > 64:
            raise OverflowError("rows do not fit 64 bits")
        out = (out << np.uint64(bits)) | c
        used += bits
    return out


def count_collisions(*parts):
    """parts: (counter (..., 4), component (...)) pairs, pooled: how many elements share their (counter, component) with an earlier one."""
    cols = [np.concatenate([np.asarray(c)[..., i].reshape(-1) for c, _ in parts]) for i in range(4)]
    cols.append(np.concatenate([np.asarray(q).reshape(-1) for _, q in parts]))
    rows = pack_rows(cols)
    return int(rows.size - np.unique(rows).size)
