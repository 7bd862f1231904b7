// K33: two bounded proper scoring rules of the evaluation beside the NLL -- the energy score and its marginal form, the CRPS -- of
// N(mean, cov + 1e-2 I) at the ground truth, per matched detection (the definitions are include/pod_mi355x.h's; the reference's
// scoring_rules.py defines neither).
//
// Serves: compute_reg_scores (SR:45-81) with the rules asked for beside `nll`; the rows are the ones pod_reg_nll takes.
//   k_eval_scores : one wavefront per row, four rows per workgroup.  Every lane factors the row's Sigma (pod_reg_sigma.h, k_reg_nll's loop:
//                   a few dozen fp64 operations, cheaper than a broadcast).  Lane 0 writes the closed-form CRPS.  For the energy score a lane
//                   owns the sample pairs (2c, 2c + 1), c = lane, lane + 64, ...: one Philox4x32-10 call is the eight normals of a pair,
//                   sample 2c + 2 comes from the neighbouring lane (lane 63: from lane 0 of the next trip, drawn one trip ahead) -- K27's
//                   walk.  fp32 normals, everything after them fp64; two fp64 partial sums per lane, a wavefront butterfly, lane 0 stores.
// No atomics, no LDS, no barrier: a row's bits depend on its inputs, its index, the seed and M alone -- not on n, the grid or other rows.
#include "pod_reg_sigma.h"

namespace pod {

constexpr int EVAL_SCORE_BLOCK = 256;
constexpr int EVAL_SCORE_ROWS = EVAL_SCORE_BLOCK / 64;

struct KEvalScoreParams {
    const float* means;
    const float* covs;
    const float* gt;
    const float* eps;
    float* eps_out;
    float* energy;
    float* crps;
    uint64_t seed;
    int32_t n, M;
};

// the eight normals of sample pair c of one row: samples 2c and 2c + 1, four coordinates each (zeros past sample M)
__device__ __forceinline__ f32x8n eval_score_pair(const KEvalScoreParams& P, int row, int c) {
    f32x8n o;
    if (P.eps) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int s = 2 * c + h;
            float4 v = float4{0.0f, 0.0f, 0.0f, 0.0f};
            if (s <= P.M) v = *reinterpret_cast<const float4*>(P.eps + ((size_t)s * P.n + row) * 4);
            o.v[4 * h] = v.x; o.v[4 * h + 1] = v.y; o.v[4 * h + 2] = v.z; o.v[4 * h + 3] = v.w;
        }
    } else if (2 * c <= P.M) {
        o = philox_normals8(P.seed, (uint32_t)row, 0u, (uint32_t)c, STREAM_EVAL_SCORE);
    } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) o.v[j] = 0.0f;
    }
    return o;
}

// |d + L e| for a lower-triangular L, fp64
__device__ __forceinline__ double eval_score_norm(const double (&L)[4][4], const double (&d)[4], const float (&e)[4]) {
    double q = 0.0;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        double u = d[r];
#pragma unroll
        for (int k = 0; k <= r; ++k) u += L[r][k] * (double)e[k];
        q += u * u;
    }
    return sqrt(q);
}

__global__ void __launch_bounds__(EVAL_SCORE_BLOCK) k_eval_scores(const KEvalScoreParams P) {
    const int lane = threadIdx.x & 63;
    const int row = (int)blockIdx.x * EVAL_SCORE_ROWS + ((int)threadIdx.x >> 6);
    if (row >= P.n) return;                                   // (uniform over the wavefront)
    double a[4][4], L[4][4], d[4];
    reg_sigma_factor(P.covs + (size_t)row * 16, a, L);
    const bool ok = reg_sigma_ok(L);
    const double nan = __longlong_as_double(0x7FF8000000000000ll);
#pragma unroll
    for (int j = 0; j < 4; ++j) d[j] = (double)P.means[(size_t)row * 4 + j] - (double)P.gt[(size_t)row * 4 + j];
    if (P.crps && lane == 0) {
        // (1/4) sum_j sd_j [z_j (2 Phi(z_j) - 1) + 2 phi(z_j) - 1 / sqrt(pi)], 2 Phi(z) - 1 = erf(z / sqrt 2)
        double sum = 0.0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const double sd = sqrt(a[j][j]);
            const double z = -d[j] / sd;
            const double pdf = 0.3989422804014327 * exp(-0.5 * z * z);
            sum += sd * (z * erf(z * 0.7071067811865476) + 2.0 * pdf - 0.5641895835477563);
        }
        P.crps[row] = ok ? (float)(0.25 * sum) : (float)nan;
    }
    if (!P.energy) return;
    const double zero[4] = {0.0, 0.0, 0.0, 0.0};
    double a1 = 0.0, a2 = 0.0;                                // sums of |u1_s|, |u2_s| of this lane's samples
    const int trips = (P.M / 2 + 1 + 63) / 64;
    f32x8n cur = eval_score_pair(P, row, lane);
    for (int i = 0; i < trips; ++i) {                         // (uniform over the wavefront: the shuffles below see every lane)
        const int c = i * 64 + lane;
        const f32x8n nxt = eval_score_pair(P, row, c + 64);
        float e2[4];                                          // sample 2c + 2: the first half of pair c + 1
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
                    *reinterpret_cast<float4*>(P.eps_out + ((size_t)(2 * c + h) * P.n + row) * 4) =
                        float4{cur.v[4 * h], cur.v[4 * h + 1], cur.v[4 * h + 2], cur.v[4 * h + 3]};
        }
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            if (2 * c + h < P.M) {
                float e[4], de[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    e[j] = cur.v[4 * h + j];
                    de[j] = e[j] - (h == 0 ? cur.v[4 + j] : e2[j]);      // the fp32 difference of the normals, never of two samples
                }
                a1 += eval_score_norm(L, d, e);
                a2 += eval_score_norm(L, zero, de);
            }
        }
        cur = nxt;
    }
    a1 = wave_sum(a1);
    a2 = wave_sum(a2);
    if (lane == 0) P.energy[row] = ok ? (float)(a1 / (double)P.M - a2 / (2.0 * (double)P.M)) : (float)nan;
}

}  // namespace pod

extern "C" int pod_reg_scores(const float* means, const float* covs, const float* gt, int32_t n, int32_t num_samples, uint64_t seed,
                              const float* eps_in, float* eps_out, float* energy, float* crps, pod_stream_t stream) {
    if (!means || !covs || !gt || (!energy && !crps) || n < 0) return POD_E_INVALID;
    if (energy && (num_samples < 1 || num_samples > POD_MAX_REG_SAMPLES)) return POD_E_INVALID;
    if (!energy && (eps_in || eps_out)) return POD_E_INVALID;
    if (!pod_aligned(16, eps_in, eps_out)) return POD_E_INVALID;
    if (n == 0) return POD_OK;
    pod::KEvalScoreParams P;
    P.means = means; P.covs = covs; P.gt = gt; P.eps = eps_in; P.eps_out = eps_out; P.energy = energy; P.crps = crps;
    P.seed = seed; P.n = n; P.M = energy ? num_samples : 0;
    const unsigned blocks = ((unsigned)n + pod::EVAL_SCORE_ROWS - 1) / pod::EVAL_SCORE_ROWS;
    hipLaunchKernelGGL(pod::k_eval_scores, dim3(blocks), dim3(pod::EVAL_SCORE_BLOCK), 0, (hipStream_t)stream, P);
    POD_CHECK_LAUNCH();
    return POD_OK;
}
