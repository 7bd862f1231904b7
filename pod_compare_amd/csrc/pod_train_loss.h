// What the kernels of the training objective share (k21_train_loss.hip, k27_reg_score_loss.hip, k28_full_cov_loss.hip): the regression
// target, the smooth-L1 term, the workgroup enumeration over the levels and the configuration check -- one copy, so that the score losses
// of K27 and K28 see the bits K21's regression terms see -- and, for K27 and K28, the launch record, the draws of the energy score, the
// listing of a workgroup's positives, the workgroup's sum and the finish kernel: under one seed an anchor sees the same normals in both.
#pragma once

#include "pod_device.h"

namespace pod {

constexpr int LOSS_BLOCK = 256;

__device__ __forceinline__ void smooth_l1_term(float d, float beta, float& loss, float& dd) {
    const float ad = fabsf(d);
    const float sgn = d > 0.0f ? 1.0f : (d < 0.0f ? -1.0f : 0.0f);
    if (beta < 1e-5f) {
        loss = ad;
        dd = sgn;
    } else if (ad < beta) {
        loss = __fdiv_rn(0.5f * d * d, beta);
        dd = __fdiv_rn(d, beta);
    } else {
        loss = ad - 0.5f * beta;
        dd = sgn;
    }
}

// Box2BoxTransform.get_deltas of anchor s towards box g
__device__ __forceinline__ void box_deltas(const Box& s, const Box& g, const float* wts, float* tgt) {
    const float sw = s.x2 - s.x1, sh = s.y2 - s.y1;
    const float scx = s.x1 + 0.5f * sw, scy = s.y1 + 0.5f * sh;
    const float tw = g.x2 - g.x1, th = g.y2 - g.y1;
    const float tcx = g.x1 + 0.5f * tw, tcy = g.y1 + 0.5f * th;
    tgt[0] = __fdiv_rn(wts[0] * (tcx - scx), sw);
    tgt[1] = __fdiv_rn(wts[1] * (tcy - scy), sh);
    tgt[2] = wts[2] * logf(__fdiv_rn(tw, sw));
    tgt[3] = wts[3] * logf(__fdiv_rn(th, sh));
}

// Host: the workgroups of a launch with one thread per (level, anchor shape, cell), level after level; first_block (n_levels + 1) or NULL.
static int64_t loss_blocks(const PodConfig* cfg, const PodLevel* levels, int32_t* first_block) {
    int64_t n = 0;
    for (int l = 0; l < cfg->n_levels; ++l) {
        if (first_block) first_block[l] = (int32_t)n;
        if (levels[l].H < 1 || levels[l].W < 1) return -1;
        n += ((int64_t)cfg->num_anchors * levels[l].H * levels[l].W + LOSS_BLOCK - 1) / LOSS_BLOCK;
        if (n > 0x7FFFFFFF) return -1;
    }
    if (first_block) first_block[cfg->n_levels] = (int32_t)n;
    return n;
}

static bool loss_cfg_ok(const PodConfig* cfg, const PodLevel* levels) {
    return cfg && levels && cfg->n_levels >= 1 && cfg->n_levels <= POD_MAX_LEVELS && cfg->n_runs >= 1 && cfg->n_runs <= 65535 &&
           cfg->num_anchors >= 1 && cfg->num_classes >= 1 && cfg->num_classes < POD_MAX_CLASSES;
}

// ---- what the covariance objectives on the positive anchors share (K27: diagonal head, K28: full covariance) ------------------------

constexpr uint32_t STREAM_REG_SCORE = 0x72656700u;   // box-delta samples of the energy score ("reg")
constexpr int SCORE_WAVES = LOSS_BLOCK / 64;

struct KScoreParams {
    PodLevel lv[POD_MAX_LEVELS];
    PodLevelGrad gr[POD_MAX_LEVELS];
    int32_t first_block[POD_MAX_LEVELS + 1];
    int32_t n_levels, A, K, R, n_images, n_gt, M, has_grads;
    float beta;
    float wts[4];
    uint64_t seed;
    const int32_t* labels;
    const int32_t* matched_gt;
    const float* gt_boxes;
    const float* anchors;
    const float* eps;
    float* eps_out;
    const float* w;
    double* partials;
};

// the eight normals of sample pair c of one anchor: samples 2c and 2c + 1, four coordinates each (zeros past sample M)
__device__ __forceinline__ f32x8n score_pair(const KScoreParams& P, int r, int img, size_t row, size_t n_rows, int c) {
    f32x8n o;
    if (P.eps) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int s = 2 * c + h;
            float4 v = float4{0.0f, 0.0f, 0.0f, 0.0f};
            if (s <= P.M) v = *reinterpret_cast<const float4*>(P.eps + ((size_t)s * n_rows + row) * 4);
            o.v[4 * h] = v.x; o.v[4 * h + 1] = v.y; o.v[4 * h + 2] = v.z; o.v[4 * h + 3] = v.w;
        }
    } else if (2 * c <= P.M) {
        o = philox_normals8(P.seed, (uint32_t)r, (uint32_t)img, (uint32_t)c, STREAM_REG_SCORE);
    } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) o.v[j] = 0.0f;
    }
    return o;
}

// an anchor that is not positive draws nothing: zeros in its row of every sample of the dense dump
__device__ __forceinline__ void score_zero_draws(const KScoreParams& P, size_t row, size_t n_rows) {
    for (int s = 0; s <= P.M; ++s) *reinterpret_cast<float4*>(P.eps_out + ((size_t)s * n_rows + row) * 4) = float4{0.0f, 0.0f, 0.0f, 0.0f};
}

// The workgroup's positives, in thread order (ballot + prefix, no atomics): s_list[0 .. n) = their thread indices; returns n.
// Every thread of the workgroup calls it; s_list: LOSS_BLOCK ints, s_count: SCORE_WAVES ints of LDS.
__device__ __forceinline__ int score_list_positives(bool pos, int* s_list, int* s_count) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const unsigned long long m = __ballot(pos);
    if (lane == 0) s_count[wv] = __popcll(m);
    __syncthreads();
    int before = 0, n_pos = 0;
    for (int i = 0; i < SCORE_WAVES; ++i) {
        if (i < wv) before += s_count[i];
        n_pos += s_count[i];
    }
    if (pos) s_list[before + __popcll(m & ((1ull << lane) - 1ull))] = threadIdx.x;
    __syncthreads();
    return n_pos;
}

// lanes -> wavefront butterfly -> workgroup (in wavefront order) -> partials[workgroup]; s_part: SCORE_WAVES doubles of LDS
__device__ __forceinline__ void score_block_sum(double acc, double* s_part, double* partials) {
    acc = wave_sum(acc);
    if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = s_part[0];
        for (int i = 1; i < SCORE_WAVES; ++i) s += s_part[i];
        partials[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = s;
    }
}

// K21's k_loss_finish for one quantity: thread-strided sums in index order, then a fixed tree
static __global__ void __launch_bounds__(LOSS_BLOCK) k_score_finish(const double* partials, int64_t n, double* sum) {
    __shared__ double s_sum[LOSS_BLOCK];
    double a = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += LOSS_BLOCK) a += partials[i];
    s_sum[threadIdx.x] = a;
    __syncthreads();
    for (int step = LOSS_BLOCK / 2; step > 0; step >>= 1) {
        if ((int)threadIdx.x < step) s_sum[threadIdx.x] += s_sum[threadIdx.x + step];
        __syncthreads();
    }
    if (threadIdx.x == 0) sum[0] = s_sum[0];
}

// Host: the partials a score launch writes (0: a configuration it refuses)
static int64_t score_partials(const PodConfig* cfg, const PodLevel* levels) {
    if (!loss_cfg_ok(cfg, levels)) return 0;
    const int64_t n = loss_blocks(cfg, levels, nullptr);
    return n < 0 ? 0 : n * cfg->n_runs;
}

// Host: the checks of a score entry and its launch record.  cov_dims: the head the entry needs (4 or 10); kind in [1, n_kinds],
// energy_kind the one that draws.  POD_OK with P filled and n_blocks set, or POD_E_INVALID with nothing enqueued.
static int score_params(const PodConfig* cfg, const PodLevel* levels, const PodLevelGrad* grads, const int32_t* labels, const int32_t* matched_gt,
                        const float* gt_boxes, int32_t n_gt, const float* anchors, int32_t R, int32_t cov_dims, int32_t kind, int32_t n_kinds,
                        int32_t energy_kind, int32_t num_samples, float smooth_l1_beta, const float* eps_reg, float* eps_out, const float* w,
                        double* partials, double* sum, KScoreParams& P, int64_t& n_blocks) {
    // ---- what pod_train_loss refuses
    if (!loss_cfg_ok(cfg, levels) || !labels || !matched_gt || !anchors || !partials || !sum || R < 1 || n_gt < 0) return POD_E_INVALID;
    if (cfg->cov_dims != cov_dims) return POD_E_INVALID;
    if (n_gt > 0 && !gt_boxes) return POD_E_INVALID;
    if (grads && !w) return POD_E_INVALID;
    if (cfg->has_cls_var && (cfg->cls_samples < 1 || cfg->cls_samples > POD_MAX_CLS_SAMPLES)) return POD_E_INVALID;
    if (!(smooth_l1_beta >= 0.0f)) return POD_E_INVALID;
    // ---- and what is a score entry's own
    if (kind < 1 || kind > n_kinds) return POD_E_INVALID;
    const bool energy = kind == energy_kind;
    if (energy && (num_samples < 1 || num_samples > POD_MAX_REG_SAMPLES)) return POD_E_INVALID;
    if (!pod_aligned(16, eps_reg, eps_out)) return POD_E_INVALID;
    n_blocks = loss_blocks(cfg, levels, P.first_block);
    if (n_blocks < 1) return POD_E_INVALID;
    int64_t anchors_seen = 0;
    for (int l = 0; l < cfg->n_levels; ++l) {
        const PodLevel& L = levels[l];
        if (!L.cls || !L.delta || (cfg->has_cls_var && !L.cls_var) || !L.reg_var) return POD_E_INVALID;
        const int64_t n_l = (int64_t)cfg->num_anchors * L.H * L.W;
        if (L.anchor_base < 0 || (int64_t)L.anchor_base + n_l > R) return POD_E_INVALID;      // every label / anchor row the kernel reads exists
        anchors_seen += n_l;
        P.lv[l] = L;
        P.gr[l] = grads ? grads[l] : PodLevelGrad{nullptr, nullptr, nullptr, nullptr};
    }
    if (anchors_seen != R) return POD_E_INVALID;
    P.n_levels = cfg->n_levels; P.A = cfg->num_anchors; P.K = cfg->num_classes; P.R = R; P.n_images = cfg->n_runs; P.n_gt = n_gt;
    P.M = energy ? num_samples : 0; P.has_grads = grads ? 1 : 0; P.beta = smooth_l1_beta;
    for (int i = 0; i < 4; ++i) P.wts[i] = cfg->box_weights[i];
    P.seed = cfg->philox_seed;
    P.labels = labels; P.matched_gt = matched_gt; P.gt_boxes = gt_boxes; P.anchors = anchors;
    P.eps = energy ? eps_reg : nullptr; P.eps_out = energy ? eps_out : nullptr; P.w = w; P.partials = partials;
    return POD_OK;
}

}  // namespace pod
