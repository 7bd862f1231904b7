// What the merge-and-score kernels share: K1 dense / K1 prune stream / K1b (k1_mc_merge_score.hip) and K1f (k1f_merge_score_fused.hip).
//
// Each of these is stated here ONCE, to be checked against the reference (probabilistic_inference.py) once: the run-merge schedule
// (merge_runs), the prune bound (may_pass), the class probability and the scoring group (class_prob_cell, score_group), the level / role
// search (find_segment) and the host's cfg check and bitmap layout.
#pragma once
#include <math.h>

#include "pod_device.h"

namespace pod {

// ---- the run merge -------------------------------------------------------------------------------------------------------------
// PI:216-222 merge of the N runs, in the reference's association order:
//   quirk: acc = x0; acc += x0; acc += x1 .. x_{N-2}; acc /= N      true mean: acc = x0; acc += x1 .. x_{N-1}; acc /= N
// `acc` owns the values: first() loads run 0, twice() doubles, add<CNT>(run0) loads runs run0 .. run0+CNT-1 -- ALL of them before the
// first add, no branch between the loads, which is what keeps HBM busy -- and adds them run after run, div(N) is the one IEEE divide.
// The runs after the first go in batches of BATCH (4, 2 or 1), then one of 2, then one of 1.
template <int BATCH, class Acc>
__device__ __forceinline__ void merge_runs(Acc& acc, int n_runs, int quirk) {
    static_assert(BATCH == 1 || BATCH == 2 || BATCH == 4, "the tail below covers batches of 4, 2 and 1");
    acc.first();
    if (n_runs == 1) return;
    int r = 1, last = n_runs;          // runs [r, last) are still to be added
    if (quirk) {
        acc.twice();
        last = n_runs - 1;
    }
    while (r + BATCH <= last) {
        acc.template add<BATCH>(r);
        r += BATCH;
    }
    if (BATCH > 2 && r + 2 <= last) {
        acc.template add<2>(r);
        r += 2;
    }
    if (BATCH > 1 && r < last) acc.template add<1>(r);
    acc.div((float)n_runs);
}

// ---- the prune bound -----------------------------------------------------------------------------------------------------------
// Native RNG + variance head.  box_muller16() bounds every draw by |eps| < POD_EPS_MAX, so
//     mean_s sigmoid(logit + eps_s*sigma) <= sigmoid(logit + POD_EPS_MAX*sigma):
// an (anchor, class) with logit + POD_EPS_MAX*sigma <= logit(score_thresh) can never become a candidate.  A streaming pass therefore
// draws nothing: it merges and keeps the anchors that MAY pass (exact superset); only those are sampled (K1b, or K1f's scoring tail).
__device__ __forceinline__ float native_sigma(float logvar) {
    return __builtin_amdgcn_exp2f(0.7213475204444817f * logvar);   // sqrt(exp(v)) = 2^(v / (2 ln 2))
}
__device__ __forceinline__ bool may_pass(float logit, float logvar, bool has_var, float skip_logit) {
    return (has_var ? fmaf(POD_EPS_MAX, native_sigma(logvar), logit) : logit) > skip_logit;
}

// ---- scoring -------------------------------------------------------------------------------------------------------------------
// Class probability of one (anchor, class): PI:289-297.
//   no variance head : sigmoid(logit)
//   variance head    : mean_s sigmoid(logit + eps_s * sqrt(exp(var))), s = 0..S-1, summed in order, / S
//
// eps source.  Replay (parity mode): tensor (S, R_l, K) in the reference layout, every op the reference's.
// Native: Philox draws organised per group of 4 consecutive cells (the 4 anchors one K1 lane owns); normal
// q = j*S + s (j = hw & 3, s = sample) is component q&7 of the call with counter
// (hw>>2, level<<16 | a<<8 | k, q>>3, STREAM_CLS).  K1, K1b / K1f and K2b all come through this one function, so
// they see bit-identical draws and sums and nothing has to be stored.  Transcendentals use the hardware
// approximations in native mode (the draws differ from torch's anyway).
__device__ __forceinline__ float class_prob_cell(float logit, float logvar, bool has_var, int S, const float* replay,
                                                int64_t level_anchors, int K, int A, int level, int hw, int a, int k, uint64_t seed) {
    if (!has_var) return sigmoid_ref(logit);
    float acc = 0.0f;
    if (replay) {
        const float sigma = sqrtf(expf(logvar));
        const float* e = replay + ((int64_t)hw * A + a) * K + k;
        const int64_t stride_s = level_anchors * K;
        for (int s = 0; s < S; ++s) {
            const float x = logit + e[(int64_t)s * stride_s] * sigma;
            acc = acc + sigmoid_ref(x);
        }
        return __fdiv_rn(acc, (float)S);
    }
    const float sigma = native_sigma(logvar);
    const int q0 = (hw & 3) * S, q1 = q0 + S;
    const uint32_t c0 = (uint32_t)(hw >> 2), c1 = ((uint32_t)level << 16) | ((uint32_t)a << 8) | (uint32_t)k;
    for (int call = q0 >> 3; call * 8 < q1; ++call) {
        const u32x4 r = philox4x32_10(u32x4{c0, c1, (uint32_t)call, STREAM_CLS}, (uint32_t)seed, (uint32_t)(seed >> 32));
        float z[8];
        box_muller16(r.x, z[0], z[1]);
        box_muller16(r.y, z[2], z[3]);
        box_muller16(r.z, z[4], z[5]);
        box_muller16(r.w, z[6], z[7]);
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const int q = call * 8 + c;
            if (q >= q0 && q < q1) acc += sigmoid_fast(fmaf(z[c], sigma, logit));
        }
    }
    return acc * __builtin_amdgcn_rcpf((float)S);
}

// The scoring group: KP consecutive lanes are the classes of ONE anchor (level l, cell hw, shape a), lane k = class k with that
// class's merged logit / log-variance (native draws).  Every lane of the wavefront calls it; `valid` = this group has an anchor.
// Evaluates the probability, takes the maximum over the class lanes by butterfly, stores the K probabilities to P.probs_dense when the
// anchor is above the threshold (the gather kernel reuses them: same function, same inputs) and returns true, with the anchor's
// candidate key, on lane k == 0 of such an anchor.  Where the key goes is the caller's.
// P: K1bParams / K1fParams (lv, K, A, cls_samples, seed, score_thresh, probs_dense).
template <int KP, class Params>
__device__ __forceinline__ bool score_group(const Params& P, float logit, float logvar, bool has_var, bool valid, int l, int hw, int a, int k,
                                            uint64_t& key) {
    const int K = P.K, A = P.A;
    float p = 0.0f;
    if (valid && k < K)
        p = class_prob_cell(logit, logvar, has_var, P.cls_samples, nullptr, (int64_t)P.lv[l].H * P.lv[l].W * A, K, A, l, hw, a, k, P.seed);
    float best = p;
#pragma unroll
    for (int o = KP >> 1; o > 0; o >>= 1) best = fmaxf(best, __shfl_xor(best, o, 64));
    const bool pass = valid && best > P.score_thresh;
    if (P.probs_dense && pass && k < K) P.probs_dense[((int64_t)P.lv[l].anchor_base + (int64_t)hw * A + a) * K + k] = p;
    key = make_key(best, hw * A + a);
    return pass && k == 0;
}

// Segment s of n with begin[s] <= x < begin[s + 1] (begin ascending, begin[0] <= x): the level / role that owns block or unit x.
__device__ __forceinline__ int find_segment(const int32_t* begin, int n, int x) {
    int s = 0;
#pragma unroll 1
    while (s + 1 < n && x >= begin[s + 1]) ++s;
    return s;
}

}  // namespace pod

// ---- host ----------------------------------------------------------------------------------------------------------------------
// The skip_logit of may_pass for a score threshold.
static inline float pod_prune_logit(float score_thresh) {
    const double t = (double)score_thresh;
    return (t > 0.0 && t < 1.0) ? (float)(log(t / (1.0 - t)) - 0.02) : -INFINITY;   // margin covers the fast-math error
}

// class_prob_cell's counter word c1 = level << 16 | a << 8 | k: an anchor shape or a class past 8 bits (a level past 16) would run into
// the neighbouring field and share its draws with another (level, shape, class).
static inline bool pod_cls_counter_fields_ok(const PodConfig* cfg) {
    return cfg->num_anchors <= 256 && cfg->num_classes <= 256 && cfg->n_levels <= 65536;
}
// What every entry point that may form that counter asks: a variance head whose samples are drawn in-kernel on at least one level (no
// eps_cls to replay there) needs fields that hold the cfg; a launch that replays every level's normals, or has no variance head, forms no
// counter and takes any anchor-shape count, as it always did.
static inline bool pod_cls_counter_ok(const PodConfig* cfg, const PodLevel* levels) {
    if (!cfg->has_cls_var) return true;
    bool native = false;
    for (int l = 0; l < cfg->n_levels && l < POD_MAX_LEVELS; ++l) native = native || !levels[l].eps_cls;
    return !native || pod_cls_counter_fields_ok(cfg);
}

// The cfg ranges every merge-and-score entry point relies on.
static inline bool pod_merge_score_cfg_ok(const PodConfig* cfg) {
    const int L = cfg->n_levels, K = cfg->num_classes, A = cfg->num_anchors, N = cfg->n_runs;
    if (L < 1 || L > POD_MAX_LEVELS || K < 1 || K > POD_MAX_CLASSES || A < 1 || N < 1 || N > POD_MAX_RUNS) return false;
    return !cfg->has_cls_var || (cfg->cls_samples >= 1 && cfg->cls_samples <= POD_MAX_CLS_SAMPLES);
}

// Layout of the K1 -> K1b bitmap: one word per (plane, 64 cells).  Plane (a, k) of level l owns wpa[l] = ceil(H*W / 64) words, bit
// (a, k, hw) = word word_begin[l] + (a*K + k)*wpa[l] + hw/64, bit hw%64.  Fills wpa[L], word_begin[L + 1]; returns the number of words.
static inline int64_t pod_bitmap_layout(const PodConfig* cfg, const PodLevel* levels, int32_t* wpa, int32_t* word_begin) {
    int64_t words = 0;
    for (int l = 0; l < cfg->n_levels; ++l) {
        wpa[l] = (int32_t)(((int64_t)levels[l].H * levels[l].W + 63) / 64);
        word_begin[l] = (int32_t)words;
        words += (int64_t)cfg->num_anchors * cfg->num_classes * wpa[l];
    }
    word_begin[cfg->n_levels] = (int32_t)words;
    return words;
}
