// K28: the three objectives that train the FULL box covariance (BBOX_COV_LOSS.COVARIANCE_TYPE `full`: ten reg_var channels per anchor, a
// lower-triangular 4 x 4 Cholesky factor) -- the Gaussian's own NLL, moment matching and the energy score -- on the positive anchors, with
// their gradients added to the planes pod_train_loss has written.  The definitions are include/pod_mi355x.h's: the reference lists the
// covariance type and has no loss for it.
//
// Serves: ProbabilisticRetinaNet.losses, probabilistic_retinanet.py:285-331, where one of these sums takes the place of the NLL sum.
//   k_full_cov<POD_FULL_COV_NLL>     : one thread per (image, level, anchor shape, cell), K21's enumeration: a positive anchor's ten loads,
//   k_full_cov<POD_FULL_COV_MOMENTS>   the factor in registers, straight-line terms and derivatives, fourteen stores; zeros in the reg_var
//                                      planes everywhere else.
//   k_full_cov<POD_FULL_COV_ENERGY>  : K27's form: the workgroup's positives listed in LDS in thread order, a wavefront per listed positive,
//                                      a lane per sample pair (2c, 2c + 1) -- K27's draws, from the same call (pod_train_loss.h's score_pair)
//                                      -- fourteen fp32 gradient sums (4 for delta, 10 for L) and two fp64 loss sums a lane, butterfly sums,
//                                      lane 0 stores.
//   k_score_finish                   : one workgroup adds the partials in index order (pod_train_loss.h).
// fp32 terms, fp64 accumulation: lane -> wavefront butterfly -> workgroup -> partials[workgroup].  No floating-point atomics: the same bits
// every run.
#include "pod_train_loss.h"

namespace pod {

// L_jk (k <= j) among an anchor's ten channels: the diagonal in 0 .. 3, then the strict lower triangle in torch.tril_indices(4, 4, -1)
// order (1,0) (2,0) (2,1) (3,0) (3,1) (3,2) -- the order cholesky_from_head reads
__device__ __forceinline__ constexpr int tri(int j, int k) { return j == k ? j : 4 + j * (j - 1) / 2 + k; }

// One positive anchor: d = delta - target, the raw diagonal channels rvd (for the clamp's derivative), c = clamp(rvd, -7, 7) and the factor
// F in tri() order, F_jj = exp(0.5 c_j).
struct FullCovAnchor {
    float d[4], rvd[4], c[4], F[10];
};

__device__ __forceinline__ FullCovAnchor load_full_cov(const KScoreParams& P, const PodLevel& L, size_t d_base, size_t v_base, int HW, int r, int mg) {
    FullCovAnchor x;
    float tgt[4];
    box_deltas(load_box(P.anchors, r), load_box(P.gt_boxes, mg), P.wts, tgt);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        x.d[j] = L.delta[d_base + (size_t)j * HW] - tgt[j];
        x.rvd[j] = L.reg_var[v_base + (size_t)j * HW];
        x.c[j] = fminf(fmaxf(x.rvd[j], -7.0f), 7.0f);
        x.F[j] = expf(0.5f * x.c[j]);
    }
#pragma unroll
    for (int k = 4; k < 10; ++k) x.F[k] = L.reg_var[v_base + (size_t)k * HW];
    return x;
}

// d loss / d F (tri() order) -> d loss / d reg_var: the diagonal through F_jj = exp(0.5 clamp(rv_j)), the rest as it is
__device__ __forceinline__ void chain_to_channels(const FullCovAnchor& x, float* g) {
#pragma unroll
    for (int j = 0; j < 4; ++j) g[j] = (x.rvd[j] >= -7.0f && x.rvd[j] <= 7.0f) ? (0.5f * x.F[j]) * g[j] : 0.0f;
}

// the one owner of a positive anchor's fourteen gradient elements: adds w2 g_delta to the delta planes, writes w2 g to the reg_var planes
__device__ __forceinline__ void store_full_cov(const PodLevelGrad& G, size_t d_base, size_t v_base, int HW, float w2, const float* g_delta,
                                               const float* g) {
    if (G.delta) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float* p = G.delta + d_base + (size_t)j * HW;
            *p = *p + w2 * g_delta[j];
        }
    }
    if (G.reg_var) {
#pragma unroll
        for (int k = 0; k < 10; ++k) G.reg_var[v_base + (size_t)k * HW] = w2 * g[k];
    }
}

// POD_FULL_COV_NLL: y = F^-1 d, loss = 0.5 |y|^2 + 0.5 sum c; q = F^-T y.  g: d / d reg_var, clamp included.
__device__ __forceinline__ double full_cov_nll(const FullCovAnchor& x, float* g_delta, float* g) {
    const float* F = x.F;
    float y[4], q[4];
    y[0] = __fdiv_rn(x.d[0], F[0]);
    y[1] = __fdiv_rn(x.d[1] - F[tri(1, 0)] * y[0], F[1]);
    y[2] = __fdiv_rn((x.d[2] - F[tri(2, 0)] * y[0]) - F[tri(2, 1)] * y[1], F[2]);
    y[3] = __fdiv_rn(((x.d[3] - F[tri(3, 0)] * y[0]) - F[tri(3, 1)] * y[1]) - F[tri(3, 2)] * y[2], F[3]);
    q[3] = __fdiv_rn(y[3], F[3]);
    q[2] = __fdiv_rn(y[2] - F[tri(3, 2)] * q[3], F[2]);
    q[1] = __fdiv_rn((y[1] - F[tri(2, 1)] * q[2]) - F[tri(3, 1)] * q[3], F[1]);
    q[0] = __fdiv_rn(((y[0] - F[tri(1, 0)] * q[1]) - F[tri(2, 0)] * q[2]) - F[tri(3, 0)] * q[3], F[0]);
    double loss = 0.0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        loss += (double)(0.5f * (y[j] * y[j]));
        loss += (double)(0.5f * x.c[j]);
        g_delta[j] = q[j];
        g[j] = (x.rvd[j] >= -7.0f && x.rvd[j] <= 7.0f) ? 0.5f * (1.0f - F[j] * (q[j] * y[j])) : 0.0f;
#pragma unroll
        for (int k = 0; k < j; ++k) g[tri(j, k)] = -(q[j] * y[k]);
    }
    return loss;
}

// POD_FULL_COV_MOMENTS: Sigma = F F^T, E = Sigma - d d^T, loss = sum_j sl1(d_j) + sum_{i >= j} sl1(E_ij).  g: d / d reg_var, clamp included.
__device__ __forceinline__ double full_cov_moments(const FullCovAnchor& x, float beta, float* g_delta, float* g) {
    const float* F = x.F;
    float m[10];                                      // sl1'(E_ij), tri() order
    double loss = 0.0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        float l1, dd1;
        smooth_l1_term(x.d[j], beta, l1, dd1);
        loss += (double)l1;
        g_delta[j] = dd1;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
        for (int j = 0; j <= i; ++j) {
            float s = F[tri(i, 0)] * F[tri(j, 0)];
#pragma unroll
            for (int k = 1; k <= j; ++k) s += F[tri(i, k)] * F[tri(j, k)];
            float l2, dd2;
            smooth_l1_term(s - x.d[i] * x.d[j], beta, l2, dd2);
            loss += (double)l2;
            m[tri(i, j)] = dd2;
        }
    }
    // G = the symmetric extension of m with its diagonal doubled
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        float gd = 0.0f;
#pragma unroll
        for (int b = 0; b < 4; ++b) gd += (a == b ? 2.0f * m[a] : m[a > b ? tri(a, b) : tri(b, a)]) * x.d[b];
        g_delta[a] -= gd;
#pragma unroll
        for (int b = 0; b <= a; ++b) {
            float gl = 0.0f;
#pragma unroll
            for (int c = b; c < 4; ++c) gl += (a == c ? 2.0f * m[a] : m[a > c ? tri(a, c) : tri(c, a)]) * F[tri(c, b)];
            g[tri(a, b)] = gl;
        }
    }
    chain_to_channels(x, g);
    return loss;
}

template <int KIND>
__global__ void __launch_bounds__(LOSS_BLOCK) k_full_cov(const KScoreParams P) {
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
        const size_t v_base = (size_t)img * L.run_stride_reg + (size_t)(a * 10) * HW + cell;
        if (KIND != POD_FULL_COV_ENERGY && pos) {
            const FullCovAnchor x = load_full_cov(P, L, d_base, v_base, HW, r, mg);
            float g_delta[4], g[10];
            acc += KIND == POD_FULL_COV_NLL ? full_cov_nll(x, g_delta, g) : full_cov_moments(x, P.beta, g_delta, g);
            if (P.has_grads) store_full_cov(P.gr[l], d_base, v_base, HW, w2, g_delta, g);
        } else if (!pos) {
            if (P.has_grads && P.gr[l].reg_var)
                for (int k = 0; k < 10; ++k) P.gr[l].reg_var[v_base + (size_t)k * HW] = 0.0f;
            if (KIND == POD_FULL_COV_ENERGY && P.eps_out) score_zero_draws(P, row, n_rows);
        }
    }
    if (KIND == POD_FULL_COV_ENERGY) {
        const int n_pos = score_list_positives(pos, s_list, s_count);          // the workgroup's positives, in thread order
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
            const size_t v_base = (size_t)img * L.run_stride_reg + (size_t)(a * 10) * HW + cell;
            const FullCovAnchor x = load_full_cov(P, L, d_base, v_base, HW, r, P.matched_gt[row]);
            double a1 = 0.0, a2 = 0.0;                        // sums of sl1(u1), sl1(u2) of this lane's samples
            float gd[4] = {0.0f, 0.0f, 0.0f, 0.0f};           // sums of sl1'(u1_j)
            float gl[10];                                     // sums of 2 sl1'(u1_j) eps_k - sl1'(u2_j) (eps_k - eps'_k), tri(j, k)
#pragma unroll
            for (int k = 0; k < 10; ++k) gl[k] = 0.0f;
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
                        float e[4], de[4];                    // the sample's normals and their exact fp32 difference to the next sample's
#pragma unroll
                        for (int k = 0; k < 4; ++k) {
                            e[k] = cur.v[4 * h + k];
                            de[k] = e[k] - (h == 0 ? cur.v[4 + k] : e2[k]);
                        }
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            float u1 = x.d[j], u2 = 0.0f;
#pragma unroll
                            for (int k = 0; k <= j; ++k) {
                                u1 += x.F[tri(j, k)] * e[k];
                                u2 += x.F[tri(j, k)] * de[k];
                            }
                            float l1, dd1, l2, dd2;
                            smooth_l1_term(u1, P.beta, l1, dd1);
                            smooth_l1_term(u2, P.beta, l2, dd2);
                            a1 += (double)l1;
                            a2 += (double)l2;
                            gd[j] += dd1;
#pragma unroll
                            for (int k = 0; k <= j; ++k) gl[tri(j, k)] += (2.0f * dd1) * e[k] - dd2 * de[k];
                        }
                    }
                }
                cur = nxt;
            }
            a1 = wave_sum(a1);
            a2 = wave_sum(a2);
            if (lane == 0) acc += (2.0 * a1 - a2) / (double)P.M;
            if (P.has_grads) {                                // (uniform)
                float g_delta[4], g[10];
#pragma unroll
                for (int j = 0; j < 4; ++j) g_delta[j] = (2.0f * inv_m) * wave_sum(gd[j]);
#pragma unroll
                for (int k = 0; k < 10; ++k) g[k] = inv_m * wave_sum(gl[k]);
                chain_to_channels(x, g);
                if (lane == 0) store_full_cov(P.gr[l], d_base, v_base, HW, w2, g_delta, g);
            }
        }
    }
    score_block_sum(acc, s_part, P.partials);
}

}  // namespace pod

extern "C" int64_t pod_full_cov_partials(const PodConfig* cfg, const PodLevel* levels) { return pod::score_partials(cfg, levels); }

extern "C" int pod_full_cov_loss(const PodConfig* cfg, const PodLevel* levels, const PodLevelGrad* grads, const int32_t* labels,
                                 const int32_t* matched_gt, const float* gt_boxes, int32_t n_gt, const float* anchors, int32_t R,
                                 int32_t kind, int32_t num_samples, float smooth_l1_beta, const float* eps_reg, float* eps_out,
                                 const float* w, double* partials, double* sum, pod_stream_t stream) {
    pod::KScoreParams P;
    int64_t n_blocks = 0;
    // what pod_reg_score_loss refuses, with the full covariance head (ten channels) in place of the diagonal one and three kinds
    if (pod::score_params(cfg, levels, grads, labels, matched_gt, gt_boxes, n_gt, anchors, R, 10, kind, 3, POD_FULL_COV_ENERGY, num_samples,
                          smooth_l1_beta, eps_reg, eps_out, w, partials, sum, P, n_blocks) != POD_OK) return POD_E_INVALID;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)n_blocks, (unsigned)cfg->n_runs);
    if (kind == POD_FULL_COV_ENERGY)
        hipLaunchKernelGGL(pod::k_full_cov<POD_FULL_COV_ENERGY>, grid, dim3(pod::LOSS_BLOCK), 0, st, P);
    else if (kind == POD_FULL_COV_MOMENTS)
        hipLaunchKernelGGL(pod::k_full_cov<POD_FULL_COV_MOMENTS>, grid, dim3(pod::LOSS_BLOCK), 0, st, P);
    else
        hipLaunchKernelGGL(pod::k_full_cov<POD_FULL_COV_NLL>, grid, dim3(pod::LOSS_BLOCK), 0, st, P);
    POD_CHECK_LAUNCH();
    hipLaunchKernelGGL(pod::k_score_finish, dim3(1), dim3(pod::LOSS_BLOCK), 0, st, (const double*)partials, (int64_t)(n_blocks * cfg->n_runs), sum);
    POD_CHECK_LAUNCH();
    return POD_OK;
}
