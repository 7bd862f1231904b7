"""CPU-side checks of the drop-in boundary: the C-ABI library builds, loads and exports every
symbol include/pod_mi355x.h declares; the ctypes mirrors have the C layout.  No compute calls."""
import ctypes
import os
import re
import subprocess

import pytest

from pod_compare_amd import build, hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "pod_mi355x.h")


TEST_HEADER = os.path.join(ROOT, "include", "pod_mi355x_test.h")


def declared_symbols(header=HEADER):
    text = open(header).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(?:int|int64_t|size_t)\s+(pod_[a-z0-9_]+)\s*\(", text)))


@pytest.fixture(scope="module")
def lib_path():
    return build.build_library()


def test_header_and_binding_agree():
    assert declared_symbols() == sorted(hip.EXPORTS)
    assert declared_symbols(TEST_HEADER) == sorted(hip.TEST_EXPORTS)          # test support lives in its own header (round 6)
    assert not set(hip.TEST_EXPORTS) & set(declared_symbols())


def test_library_exports_every_declared_symbol(lib_path):
    lib = ctypes.CDLL(lib_path)
    for name in declared_symbols() + declared_symbols(TEST_HEADER):
        assert hasattr(lib, name), name
    assert lib.pod_abi_version() == hip.POD_ABI_VERSION


def test_binding_loads(lib_path):
    lib = hip.load()
    assert lib.pod_nms_scratch_bytes(5000) >= 4 * 16 * (1 + hip.POD_MAX_DETECTIONS)   # flag + per-class survivor lists
    assert lib.pod_nms_scratch_bytes(0) == 0


def test_struct_layout_matches_c(lib_path, tmp_path):
    """sizeof/offsetof of the ctypes mirrors against the C header (compiled with gcc)."""
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "pod_mi355x.h"\n'
                   'int main(void){printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\\n", sizeof(PodLevel), offsetof(PodLevel, run_stride_cls),'
                   ' offsetof(PodLevel, H), sizeof(PodConfig), offsetof(PodConfig, score_thresh), offsetof(PodConfig, box_weights),'
                   ' offsetof(PodConfig, philox_seed), sizeof(PodWorkspace), offsetof(PodWorkspace, cand_run_delta),'
                   ' offsetof(PodWorkspace, m_probs), offsetof(PodWorkspace, n_capacity), sizeof(PodDetections),'
                   ' offsetof(PodDetections, n_det));'
                   'printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu\\n", sizeof(PodConvSet), offsetof(PodConvSet, in_amax), offsetof(PodConvSet, offset),'
                   ' offsetof(PodConvSet, k_planes), sizeof(PodWinoConv), offsetof(PodWinoConv, p), offsetof(PodWinoConv, epoch),'
                   ' offsetof(PodWinoConv, split_stride), offsetof(PodWinoConv, sets)); return 0;}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    want = [ctypes.sizeof(hip.PodLevel), hip.PodLevel.run_stride_cls.offset, hip.PodLevel.H.offset, ctypes.sizeof(hip.PodConfig),
            hip.PodConfig.score_thresh.offset, hip.PodConfig.box_weights.offset, hip.PodConfig.philox_seed.offset,
            ctypes.sizeof(hip.PodWorkspace), hip.PodWorkspace.cand_run_delta.offset, hip.PodWorkspace.m_probs.offset,
            hip.PodWorkspace.n_capacity.offset, ctypes.sizeof(hip.PodDetections), hip.PodDetections.n_det.offset,
            ctypes.sizeof(hip.PodConvSet), hip.PodConvSet.in_amax.offset, hip.PodConvSet.offset.offset, hip.PodConvSet.k_planes.offset,
            ctypes.sizeof(hip.PodWinoConv), hip.PodWinoConv.p.offset, hip.PodWinoConv.epoch.offset, hip.PodWinoConv.split_stride.offset,
            hip.PodWinoConv.sets.offset]
    assert got == want


def test_invalid_arguments_are_rejected_without_a_gpu(lib_path):
    """Argument validation happens on the host before any launch: safe to exercise on CPU."""
    lib = hip.load()
    cfg = hip.PodConfig()
    assert lib.pod_reset_counters(None, 4, None) == -1
    assert lib.pod_level_topk(cfg, None, None, None, None, None, None, None, None, None) == -1
    assert lib.pod_reg_nll(None, None, None, 3, None, None) == -1
    assert lib.pod_run_image(cfg, None, None, 0, 0, 0, 10, 10, 10, 10, None, None) == -1
    assert lib.pod_nms_cluster(cfg, None, 8, None, None, None, None, None, None, None) == -1
    d = hip.PodWinoConv()
    assert lib.pod_wino_conv3x3_split(ctypes.byref(d), None) == -1 and lib.pod_wino_conv3x3_split(None, None) == -1
    assert lib.pod_absmax(None, 4, None, None) == -1
    assert lib.pod_wino_filter_split_bytes(64, 32) == 2 * 24 * 64 * 32 * 2 + 16 and lib.pod_wino_filter_split_bytes(64, 8) == 0


def test_candidate_entry_points_reject_invalid_arguments_without_a_gpu(lib_path):
    """pod_gather_candidates, pod_decode_cov and pod_gather_decode: every null pointer and every out-of-range cfg field an entry
    point checks makes it return POD_E_INVALID before anything is launched; each entry point checks what it always did."""
    lib = hip.load()
    buf = ctypes.create_string_buffer(64)
    X = ctypes.addressof(buf)                        # any non-null pointer: never dereferenced on these paths
    lv = (hip.PodLevel * hip.POD_MAX_LEVELS)()

    def cfg_with(**kw):
        c = hip.PodConfig()
        c.n_levels, c.n_runs, c.num_anchors, c.num_classes, c.cov_dims, c.prop_samples, c.topk = 5, 10, 9, 7, 4, 1000, 1000
        for k, v in kw.items():
            setattr(c, k, v)
        return c

    def gather(c, levels=lv, reg_var=X, **null):     # the 15 pointers after `levels`, by position, and a null stream
        a = [X] * 15 + [None]
        a[12] = reg_var
        for i in null.values():
            a[i] = None
        return lib.pod_gather_candidates(c, levels, *a)

    def decode(c, n_capacity=8, reg_var=X, run_delta=X, idx=X, level=X, eps=None, n_replay=0, n_total=X, delta=X, anchor=X, boxes=X, cov=X):
        return lib.pod_decode_cov(c, lv, n_total, n_capacity, delta, reg_var, anchor, run_delta, idx, level, eps, n_replay, boxes, cov, None)

    def fused(c, levels=lv, reg_var=X, **null):      # the 17 pointers after `levels`, by position, and a null stream
        a = [X] * 17 + [None, None]
        a[12] = reg_var
        for i in null.values():
            a[i] = None
        return lib.pod_gather_decode(c, levels, *a)

    ok = cfg_with()
    # pod_gather_candidates: nulls (probs_dense, cand_reg_var without a head, cand_run_delta and the stream may be null), rows, channels
    assert gather(None) == -1 and gather(ok, levels=None) == -1
    for i in (0, 1, 2, 3, 4, 6, 7, 8, 9, 10, 11, 13):
        assert gather(ok, null=i) == -1, i
    assert gather(ok, reg_var=None) == -1
    assert gather(cfg_with(n_levels=8, topk=4097)) == -1                       # n_levels * topk > 4 * POD_MAX_CANDIDATES
    assert gather(cfg_with(num_classes=16, cov_dims=29)) == -1 and gather(cfg_with(num_classes=29, cov_dims=4)) == -1   # 2K + 4 + D = 65
    # pod_decode_cov: nulls, n_capacity, prop_samples with a reg_var head, n_runs above the maximum, replay without a count
    assert lib.pod_decode_cov(None, lv, X, 8, X, X, X, X, X, X, None, 0, X, X, None) == -1
    assert lib.pod_decode_cov(ok, None, X, 8, X, X, X, X, X, X, None, 0, X, X, None) == -1
    for kw in ({"n_total": None}, {"delta": None}, {"anchor": None}, {"boxes": None}, {"cov": None}, {"n_capacity": 0}, {"reg_var": None},
               {"idx": None}, {"level": None}, {"run_delta": None}, {"eps": X, "n_replay": 0}):
        assert decode(ok, **kw) == -1, kw
    assert decode(cfg_with(prop_samples=1)) == -1 and decode(cfg_with(prop_samples=hip.POD_MAX_PROP_SAMPLES + 1)) == -1
    assert decode(cfg_with(n_runs=hip.POD_MAX_RUNS + 1)) == -1
    # pod_gather_decode: the union, plus the n_levels / n_runs ranges and native draws only
    assert fused(None) == -1 and fused(ok, levels=None) == -1
    for i in (0, 1, 2, 3, 4, 6, 7, 8, 9, 10, 11, 13, 15, 16):
        assert fused(ok, null=i) == -1, i
    assert fused(ok, reg_var=None) == -1
    for kw in ({"n_levels": 0}, {"n_levels": hip.POD_MAX_LEVELS + 1}, {"n_runs": 0}, {"n_runs": hip.POD_MAX_RUNS + 1}, {"n_levels": 8, "topk": 4097},
               {"num_classes": 16, "cov_dims": 29}, {"prop_samples": 1}, {"prop_samples": hip.POD_MAX_PROP_SAMPLES + 1}):
        assert fused(cfg_with(**kw)) == -1, kw
    replay = (hip.PodLevel * hip.POD_MAX_LEVELS)()
    replay[4].eps_cls = X
    assert fused(ok, levels=replay) == -1


def test_cluster_merge_entry_points_reject_invalid_arguments_without_a_gpu(lib_path):
    """pod_bayes_fuse, pod_anchor_stats_merge and pod_ensemble_merge share one validate-and-fill function; each still rejects exactly
    what it rejected before: its null pointers (cov may be null for anchor statistics only), its class-count limit (BayesOD takes one
    class fewer) and its count limit (max_detections, or the ensemble's capacity)."""
    lib = hip.load()
    buf = ctypes.create_string_buffer(64)
    X = ctypes.addressof(buf)                        # any non-null pointer: never dereferenced on these paths
    MC, MD, MN = hip.POD_MAX_CLASSES, hip.POD_MAX_DETECTIONS, hip.POD_MAX_CANDIDATES

    def cfg_with(**kw):
        c = hip.PodConfig()
        c.n_levels, c.topk, c.num_classes, c.max_detections = 5, 1000, 7, 100
        for k, v in kw.items():
            setattr(c, k, v)
        return c

    def bayes(c, box_mode=0, cls_mode=0, null=None):      # 8 input pointers, the modes, 5 outputs, a null stream
        a = [X] * 13
        if null is not None:
            a[null] = None
        return lib.pod_bayes_fuse(c, *a[:8], box_mode, cls_mode, *a[8:], None)

    def anchor(c, null=None):                             # 7 input pointers, 5 outputs
        a = [X] * 12
        if null is not None:
            a[null] = None
        return lib.pod_anchor_stats_merge(c, *a, None)

    def ensemble(c, capacity=300, null=None):             # m_total, then capacity, 4 inputs, seeds, n_seeds, 5 outputs
        a = [X] * 12
        if null is not None:
            a[null] = None
        return lib.pod_ensemble_merge(c, a[0], capacity, *a[1:], None)

    ok = cfg_with()
    assert bayes(None) == -1 and anchor(None) == -1 and ensemble(None) == -1
    for i in range(13):
        assert bayes(ok, null=i) == -1, i
    for i in range(12):
        assert ensemble(ok, null=i) == -1, i
        if i != 4:                                        # cov
            assert anchor(ok, null=i) == -1, i
    for kw in ({"box_mode": -1}, {"box_mode": 2}, {"cls_mode": -1}, {"cls_mode": 2}):
        assert bayes(ok, **kw) == -1, kw
    assert bayes(cfg_with(num_classes=0)) == -1 and bayes(cfg_with(num_classes=MC)) == -1
    for call in (anchor, ensemble):
        assert call(cfg_with(num_classes=0)) == -1 and call(cfg_with(num_classes=MC + 1)) == -1
    for call in (bayes, anchor):
        assert call(cfg_with(max_detections=0)) == -1 and call(cfg_with(max_detections=MD + 1)) == -1
    assert ensemble(ok, capacity=0) == -1 and ensemble(ok, capacity=MN + 1) == -1


def test_model_op_entry_points_reject_invalid_arguments_without_a_gpu(lib_path):
    """The seven entry points of k8_model_ops.hip, pod_reduce_partials and pod_relu_dropout_backward: every null pointer, misalignment,
    range and divisibility condition an entry point checks makes it return POD_E_INVALID, and an empty tensor (n == 0 / N == 0) returns
    POD_OK where the entry point has that exit -- all before anything is launched.  Every rejected call differs from a valid one in
    exactly the argument under test."""
    lib = hip.load()
    buf = ctypes.create_string_buffer(128)
    X = (ctypes.addressof(buf) + 63) & ~63           # 64-byte aligned, never dereferenced on these paths
    M, M2 = X + 4, X + 2                             # misaligned for 16 bytes; for 4 bytes
    Y = X + 64                                       # a second aligned pointer (src != dst)
    nan = float("nan")

    def rejects(fn, base, bad, empty=None):
        """base: a valid argument list; empty: {position: value} that makes it an empty, accepted call; bad: (position, value) pairs."""
        if empty is not None:
            a = list(base)
            for i, v in empty.items():
                a[i] = v
            assert fn(*a) == 0, (fn.__name__, "empty")
        for i, v in bad:
            a = list(base)
            if empty is not None:                    # checks come before the empty exit: the rejected call stays launch-free either way
                for j, w in empty.items():
                    a[j] = w
            a[i] = v
            assert fn(*a) == -1, (fn.__name__, i, v)

    bad_p = [-0.1, 1.0, 1.5, nan]
    # pod_bias_act_to_nhwc(src, dst, bias, N, C, HW, relu, stream)
    rejects(lib.pod_bias_act_to_nhwc, [X, Y, X, 1, 8, 6, 1, None],
            [(0, None), (1, None), (1, X), (3, -1), (4, 0), (4, 3), (4, 6), (5, 0), (0, M), (1, M), (3, 1 << 31)], empty={3: 0})
    assert lib.pod_bias_act_to_nhwc(X, Y, X, 1, 8, 1 << 38, 1, None) == -1                # more workgroups than a grid holds
    # pod_bias_act_to_nchw(src, dst, bias, N, C, HW, relu, p, seed, offset, stream)
    rejects(lib.pod_bias_act_to_nchw, [X, Y, X, 1, 8, 8, 1, 0.3, 1, 0, None],
            [(0, None), (1, None), (1, X), (3, -1), (4, 0), (4, 3), (4, 6), (5, 0), (5, 3), (5, 6), (0, M), (1, M), (2, M), (3, 1 << 31)]
            + [(7, p) for p in bad_p], empty={3: 0})
    assert lib.pod_bias_act_to_nchw(X, Y, X, 1, 8, 1 << 38, 1, 0.3, 1, 0, None) == -1
    # pod_absmax(x, n, amax, stream)
    rejects(lib.pod_absmax, [X, 5, Y, None], [(0, None), (2, None), (1, -1), (0, M), (2, M2)], empty={1: 0})
    # pod_wino_reduce(partials, n_splits, split_stride, bias, planes, HW, Kpad, K, relu, out_amax, stream): no empty exit
    rejects(lib.pod_wino_reduce, [X, 2, 80, X, Y, 10, 8, 6, 1, None, None],
            [(0, None), (4, None), (1, 0), (1, 17), (5, 0), (6, 0), (6, 3), (6, 6), (7, 0), (7, 9), (2, 79), (2, 76), (2, 82), (0, M), (4, M), (3, M)])
    # pod_expand_dropout(src, dst, n, copies, p, seed, offset, epoch, stream)
    rejects(lib.pod_expand_dropout, [X, Y, 8, 2, 0.3, 1, 0, None, None],
            [(0, None), (1, None), (2, -4), (2, 6), (3, 0), (0, M), (1, M)] + [(4, p) for p in bad_p], empty={2: 0})
    # pod_bias_act(x, bias, residual, res_bias, n, C, HW, relu, p, seed, offset, stream)
    rejects(lib.pod_bias_act, [X, X, Y, X, 12, 2, 3, 1, 0.3, 1, 0, None],
            [(0, None), (4, -12), (5, 0), (6, 0), (0, M), (2, M), (2, None)] + [(8, p) for p in bad_p], empty={4: 0})
    assert lib.pod_bias_act(X, X, Y, X, 12, 5, 1, 1, 0.3, 1, 0, None) == -1            # n is not a multiple of C * HW
    assert lib.pod_bias_act(X, X, Y, X, 12, 2, 4, 1, 0.3, 1, 0, None) == -1
    # pod_relu_dropout(x, n, p, seed, offset, stream)
    rejects(lib.pod_relu_dropout, [X, 5, 0.3, 1, 0, None], [(0, None), (1, -1), (0, M)] + [(2, p) for p in bad_p], empty={1: 0})
    # pod_reduce_partials(partials, n_splits, split_stride, bias, residual, y, n, Cout, relu, out_amax, stream)
    rejects(lib.pod_reduce_partials, [X, 2, 16, X, X, Y, 16, 8, 1, None, None],
            [(0, None), (5, None), (1, 0), (1, 17), (7, 0), (7, 3), (7, 6), (0, M), (5, M), (3, M), (4, M)], empty={6: 0})
    for a in ([X, 2, 16, X, X, Y, -8, 8, 1, None, None], [X, 2, 32, X, X, Y, 18, 8, 1, None, None], [X, 2, 16, X, X, Y, 12, 8, 1, None, None],
              [X, 2, 12, X, X, Y, 16, 8, 1, None, None], [X, 2, 18, X, X, Y, 16, 8, 1, None, None]):
        assert lib.pod_reduce_partials(*a) == -1, a                                      # n < 0, n % 4, n % Cout, a short / odd split stride
    # pod_relu_dropout_backward(out, d_out, d_z, n, p, dz_amax, stream)
    rejects(lib.pod_relu_dropout_backward, [X, X, Y, 8, 0.3, None, None],
            [(0, None), (1, None), (2, None), (3, -4), (3, 6), (0, M), (1, M), (2, M)] + [(4, p) for p in bad_p], empty={3: 0})


def test_missing_library_fails_loudly(monkeypatch):
    monkeypatch.setenv("POD_MI355X_LIB", "/nonexistent/libpod_mi355x.so")
    monkeypatch.setattr(hip, "_lib", None)
    with pytest.raises(hip.PodError):
        hip.load()
