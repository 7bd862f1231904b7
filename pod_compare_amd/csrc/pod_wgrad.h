// What the weight-gradient kernels share (k22_conv3x3_wgrad.hip, k23_fpn_backward.hip): the bias gradient's fp64 column sums and the
// second launch that adds the slices' partial sums in slice order.  Templates, so that each file that launches them carries its own copy.
#pragma once
#include "pod_split_gemm.h"

namespace pod {

constexpr int WG_DB_CHUNK = 4096;  // pixels of one db partial

// fp64 column sums of dY over one chunk of pixels: dbp[chunk][k < Kpad]
template <int CHUNK>
__global__ void __launch_bounds__(256) k_wgrad_db(const float* __restrict__ dY, const int64_t pixels, const int Kpad, double* __restrict__ dbp) {
    __shared__ double red[16][64];
    const int t = threadIdx.x, q4 = t & 15, pr = t >> 4, k0 = blockIdx.y * 64;
    const int64_t p0 = (int64_t)blockIdx.x * CHUNK;
    const int64_t p1 = p0 + CHUNK < pixels ? p0 + CHUNK : pixels;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
    for (int64_t p = p0 + pr; p < p1; p += 16) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(dY + p * Kpad + k0 + 4 * q4);
        s0 += (double)v.x; s1 += (double)v.y; s2 += (double)v.z; s3 += (double)v.w;
    }
    red[pr][4 * q4 + 0] = s0; red[pr][4 * q4 + 1] = s1; red[pr][4 * q4 + 2] = s2; red[pr][4 * q4 + 3] = s3;
    __syncthreads();
    if (t < 64) {
        double a = 0.0;
#pragma unroll
        for (int q = 0; q < 16; ++q) a += red[q][t];
        dbp[(int64_t)blockIdx.x * Kpad + k0 + t] = a;
    }
}

// the slices' partials [slice][tap][k < Kpad][c < C] in slice order -> dW (K, C, TAPS); the chunks' column sums in chunk order -> db (K)
// (db null: no bias gradient is asked for)
template <int TAPS>
__global__ void __launch_bounds__(256) k_wgrad_reduce(const float* __restrict__ partials, const int n_slices, const double* __restrict__ dbp, const int n_chunks,
                                                      const int C, const int K, const int Kpad, float* __restrict__ dW, float* __restrict__ db) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, n_w = (int64_t)TAPS * K * C;
    if (i < n_w) {
        const int c = (int)(i % C), k = (int)((i / C) % K), tap = (int)(i / ((int64_t)C * K));
        double a = 0.0;
        for (int s = 0; s < n_slices; ++s) a += (double)partials[(((int64_t)s * TAPS + tap) * Kpad + k) * C + c];
        dW[((int64_t)k * C + c) * TAPS + tap] = (float)a;
    } else if (db && i - n_w < K) {
        const int k = (int)(i - n_w);
        double a = 0.0;
        for (int ch = 0; ch < n_chunks; ++ch) a += dbp[(int64_t)ch * Kpad + k];
        db[k] = (float)a;
    }
}

}  // namespace pod
