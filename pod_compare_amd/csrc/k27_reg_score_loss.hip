// K27: the two box-covariance objectives the reference's configuration names beside the NLL -- `second_moment_matching` and `energy_loss`
// (BBOX_COV_LOSS.NAME; the definitions are include/pod_mi355x.h's, the reference names them and defines neither) -- on the positive
// anchors, with their gradients added to the planes pod_train_loss has written.
//
// Serves: ProbabilisticRetinaNet.losses, probabilistic_retinanet.py:285-331, where one of these sums takes the place of the NLL sum.
//   k_reg_score<POD_REG_LOSS_MOMENTS> : one thread per (image, level, anchor shape, cell), K21's enumeration: a positive anchor's four terms,
//                                       its gradients, zeros in the reg_var planes everywhere else.
//   k_reg_score<POD_REG_LOSS_ENERGY>  : the same threads first list the workgroup's positives in LDS in thread order (ballot + prefix, no
//                                       atomics) and write the zeros; the four wavefronts then take the listed positives in turn.  A lane
//                                       owns the sample pairs (2c, 2c + 1), c = lane, lane + 64, ...: one Philox4x32-10 call is the eight
//                                       normals of a pair, sample 2c + 2 comes from the neighbouring lane (lane 63: from lane 0 of the next
//                                       trip, drawn one trip ahead).  Butterfly sums, one lane stores the anchor's gradient.
//   k_score_finish                    : one workgroup adds the partials in index order.
// fp32 terms, fp64 accumulation: lane -> wavefront butterfly -> workgroup -> partials[workgroup].  No floating-point atomics: the same bits
// every run.  A draw depends on (seed, image, anchor, sample, coordinate) alone -- not on the grid, the batch or the other positives.
#include "pod_train_loss.h"

namespace pod {

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

template <int KIND>
__global__ void __launch_bounds__(LOSS_BLOCK) k_reg_score(const KScoreParams P) {
    __shared__ double s_part[SCORE_WAVES];
    __shared__ int s_list[LOSS_BLOCK];
    __shared__ int s_count[SCORE_WAVES];
    const int img = blockIdx.y;
    int l = 0;
    while (l + 1 < P.n_levels && (int)blockIdx.x >= P.first_block[l + 1]) ++l;
    const PodLevel& L = P.lv[l];
    const int HW = L.H * L.W;
    const int t = ((int)blockIdx.x - P.first_block[l]) * LOSS_BLOCK + threadIdx.x;
    const size_t n_rows = (size_t)P.n_images * P.R;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    float w2 = 0.0f;
    if (P.has_grads) w2 = P.w[2];
    double acc = 0.0;
    bool pos = false;
    if (t < P.A * HW) {
        const int a = t / HW, cell = t - a * HW;
        const int r = L.anchor_base + cell * P.A + a;
        const size_t row = (size_t)img * P.R + r;
        const int label = P.labels[row];
        const int mg = (label >= 0 && label < P.K) ? P.matched_gt[row] : -1;
        pos = mg >= 0 && mg < P.n_gt;
        const size_t d_base = (size_t)img * L.run_stride_delta + (size_t)(a * 4) * HW + cell;
        const size_t v_base = (size_t)img * L.run_stride_reg + (size_t)(a * 4) * HW + cell;
        if (KIND == POD_REG_LOSS_MOMENTS) {
            float tgt[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            if (pos) box_deltas(load_box(P.anchors, r), load_box(P.gt_boxes, mg), P.wts, tgt);
            for (int j = 0; j < 4; ++j) {
                float g_v = 0.0f;
                if (pos) {
                    const float lvj = L.reg_var[v_base + (size_t)j * HW];
                    const float d = L.delta[d_base + (size_t)j * HW] - tgt[j];
                    const float v = expf(fminf(fmaxf(lvj, -7.0f), 7.0f));
                    float l1, dd1, l2, dd2;
                    smooth_l1_term(d, P.beta, l1, dd1);
                    smooth_l1_term(v - d * d, P.beta, l2, dd2);
                    acc += (double)l1;
                    acc += (double)l2;
                    g_v = (lvj >= -7.0f && lvj <= 7.0f) ? w2 * (dd2 * v) : 0.0f;
                    if (P.has_grads && P.gr[l].delta) {
                        float* gd = P.gr[l].delta + d_base + (size_t)j * HW;
                        *gd = *gd + w2 * (dd1 - (2.0f * d) * dd2);
                    }
                }
                if (P.has_grads && P.gr[l].reg_var) P.gr[l].reg_var[v_base + (size_t)j * HW] = g_v;
            }
        } else if (!pos) {
            if (P.has_grads && P.gr[l].reg_var)
                for (int j = 0; j < 4; ++j) P.gr[l].reg_var[v_base + (size_t)j * HW] = 0.0f;
            if (P.eps_out)      // an anchor that is not positive draws nothing
                for (int s = 0; s <= P.M; ++s) *reinterpret_cast<float4*>(P.eps_out + ((size_t)s * n_rows + row) * 4) = float4{0.0f, 0.0f, 0.0f, 0.0f};
        }
    }
    if (KIND == POD_REG_LOSS_ENERGY) {
        // ---- the workgroup's positives, in thread order
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
        // ---- a wavefront per listed positive, a lane per sample pair
        const float inv_m = __fdiv_rn(1.0f, (float)P.M);
        const int trips = (P.M / 2 + 1 + 63) / 64;
        for (int p = wv; p < n_pos; p += SCORE_WAVES) {
            const int tl = __builtin_amdgcn_readfirstlane(s_list[p]);
            const int tp = ((int)blockIdx.x - P.first_block[l]) * LOSS_BLOCK + tl;
            const int a = tp / HW, cell = tp - a * HW;
            const int r = L.anchor_base + cell * P.A + a;
            const size_t row = (size_t)img * P.R + r;
            const size_t d_base = (size_t)img * L.run_stride_delta + (size_t)(a * 4) * HW + cell;
            const size_t v_base = (size_t)img * L.run_stride_reg + (size_t)(a * 4) * HW + cell;
            float tgt[4], d[4], sg[4], lvj[4];
            box_deltas(load_box(P.anchors, r), load_box(P.gt_boxes, P.matched_gt[row]), P.wts, tgt);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                lvj[j] = L.reg_var[v_base + (size_t)j * HW];
                d[j] = L.delta[d_base + (size_t)j * HW] - tgt[j];
                sg[j] = expf(0.5f * fminf(fmaxf(lvj[j], -7.0f), 7.0f));
            }
            double a1 = 0.0, a2 = 0.0;                        // sums of sl1(u1), sl1(u2) of this lane's samples
            float gd[4] = {0.0f, 0.0f, 0.0f, 0.0f}, gv1[4] = {0.0f, 0.0f, 0.0f, 0.0f}, gv2[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            f32x8n cur = score_pair(P, r, img, row, n_rows, lane);
            for (int i = 0; i < trips; ++i) {                 // (uniform over the wavefront: the shuffles below see every lane)
                const int c = i * 64 + lane;
                const f32x8n nxt = score_pair(P, r, img, row, n_rows, c + 64);
                float e2[4];                                  // sample 2c + 2: the first half of pair c + 1
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float from_next_lane = __shfl_down(cur.v[j], 1, 64);
                    const float from_next_trip = __shfl(nxt.v[j], 0, 64);
                    e2[j] = lane == 63 ? from_next_trip : from_next_lane;
                }
                if (P.eps_out) {
#pragma unroll
                    for (int h = 0; h < 2; ++h)
                        if (2 * c + h <= P.M)
                            *reinterpret_cast<float4*>(P.eps_out + ((size_t)(2 * c + h) * n_rows + row) * 4) =
                                float4{cur.v[4 * h], cur.v[4 * h + 1], cur.v[4 * h + 2], cur.v[4 * h + 3]};
                }
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    if (2 * c + h < P.M) {
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            const float e = cur.v[4 * h + j];
                            const float de = e - (h == 0 ? cur.v[4 + j] : e2[j]);
                            float l1, dd1, l2, dd2;
                            smooth_l1_term(d[j] + sg[j] * e, P.beta, l1, dd1);
                            smooth_l1_term(sg[j] * de, P.beta, l2, dd2);
                            a1 += (double)l1;
                            a2 += (double)l2;
                            gd[j] += dd1;
                            gv1[j] += dd1 * e;
                            gv2[j] += dd2 * de;
                        }
                    }
                }
                cur = nxt;
            }
            a1 = wave_sum(a1);
            a2 = wave_sum(a2);
            if (lane == 0) acc += (2.0 * a1 - a2) / (double)P.M;
            if (P.has_grads) {                                // (uniform)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float s_d = wave_sum(gd[j]), s_v1 = wave_sum(gv1[j]), s_v2 = wave_sum(gv2[j]);
                    if (lane == 0) {
                        if (P.gr[l].delta) {
                            float* g = P.gr[l].delta + d_base + (size_t)j * HW;
                            *g = *g + w2 * ((2.0f * inv_m) * s_d);
                        }
                        if (P.gr[l].reg_var) {
                            const float dv = (0.5f * sg[j]) * ((2.0f * inv_m) * s_v1 - inv_m * s_v2);
                            P.gr[l].reg_var[v_base + (size_t)j * HW] = (lvj[j] >= -7.0f && lvj[j] <= 7.0f) ? w2 * dv : 0.0f;
                        }
                    }
                }
            }
        }
    }
    acc = wave_sum(acc);
    if (lane == 0) s_part[wv] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = s_part[0];
        for (int i = 1; i < SCORE_WAVES; ++i) s += s_part[i];
        P.partials[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = s;
    }
}

// K21's k_loss_finish for one quantity: thread-strided sums in index order, then a fixed tree
__global__ void __launch_bounds__(LOSS_BLOCK) k_score_finish(const double* partials, int64_t n, double* sum) {
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

}  // namespace pod

extern "C" int64_t pod_reg_score_partials(const PodConfig* cfg, const PodLevel* levels) {
    if (!pod::loss_cfg_ok(cfg, levels)) return 0;
    const int64_t n = pod::loss_blocks(cfg, levels, nullptr);
    return n < 0 ? 0 : n * cfg->n_runs;
}

extern "C" int pod_reg_score_loss(const PodConfig* cfg, const PodLevel* levels, const PodLevelGrad* grads, const int32_t* labels,
                                  const int32_t* matched_gt, const float* gt_boxes, int32_t n_gt, const float* anchors, int32_t R,
                                  int32_t kind, int32_t num_samples, float smooth_l1_beta, const float* eps_reg, float* eps_out,
                                  const float* w, double* partials, double* sum, pod_stream_t stream) {
    // ---- what pod_train_loss refuses
    if (!pod::loss_cfg_ok(cfg, levels) || !labels || !matched_gt || !anchors || !partials || !sum || R < 1 || n_gt < 0) return POD_E_INVALID;
    if (cfg->cov_dims != 4) return POD_E_INVALID;            // both losses need the diagonal covariance head
    if (n_gt > 0 && !gt_boxes) return POD_E_INVALID;
    if (grads && !w) return POD_E_INVALID;
    if (cfg->has_cls_var && (cfg->cls_samples < 1 || cfg->cls_samples > POD_MAX_CLS_SAMPLES)) return POD_E_INVALID;
    if (!(smooth_l1_beta >= 0.0f)) return POD_E_INVALID;
    // ---- and what is this entry's own
    if (kind != POD_REG_LOSS_MOMENTS && kind != POD_REG_LOSS_ENERGY) return POD_E_INVALID;
    const bool energy = kind == POD_REG_LOSS_ENERGY;
    if (energy && (num_samples < 1 || num_samples > POD_MAX_REG_SAMPLES)) return POD_E_INVALID;
    if (!pod_aligned(16, eps_reg, eps_out)) return POD_E_INVALID;
    pod::KScoreParams P;
    const int64_t n_blocks = pod::loss_blocks(cfg, levels, P.first_block);
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
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)n_blocks, (unsigned)cfg->n_runs);
    if (energy)
        hipLaunchKernelGGL(pod::k_reg_score<POD_REG_LOSS_ENERGY>, grid, dim3(pod::LOSS_BLOCK), 0, st, P);
    else
        hipLaunchKernelGGL(pod::k_reg_score<POD_REG_LOSS_MOMENTS>, grid, dim3(pod::LOSS_BLOCK), 0, st, P);
    POD_CHECK_LAUNCH();
    hipLaunchKernelGGL(pod::k_score_finish, dim3(1), dim3(pod::LOSS_BLOCK), 0, st, (const double*)partials, (int64_t)(n_blocks * cfg->n_runs), sum);
    POD_CHECK_LAUNCH();
    return POD_OK;
}
