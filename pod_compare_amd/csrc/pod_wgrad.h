// What k22_conv3x3_wgrad.hip, k23_fpn_backward.hip and k24_resnet_backward.hip share.  The weight gradients: the bias gradient's fp64
// column sums, the second launch that adds the slices' partial sums in slice order, the partial buffer's layout (WgradLayout), the entries'
// argument checks and three launches (wgrad_launch), and the 1x1 kernel with its launcher (c1w_launch), which K23 runs on consecutive rows
// and K24 on the rows a stride selects.  The element-wise passes: the grid-stride loop over 16-byte quads with its abs-max record
// (quad_pass, map_quad_pass), the ReLU gate (gate4), the map gathers' host check and launch (map_gather).
// Templates and static functions, so that each file that launches them carries its own copy.
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

constexpr int C1W_STEP = 32;            // pixels of one step
constexpr int C1W_KT = 64, C1W_CT = 128;
constexpr int C1W_DS = C1W_KT + 4;      // LDS row strides, floats (16-byte rows; any stride serves the column reads)
constexpr int C1W_XS = C1W_CT + 4;
constexpr int C1W_MAX_C = 18432;        // p6's patch matrix: 9 x 2048

// Host and device agree on the slices through this function of the geometry alone.
static inline int c1w_slice_pixels(int64_t pixels, int C, int K) {
    const int64_t tiles = (int64_t)(K / C1W_KT) * ((C + C1W_CT - 1) / C1W_CT);
    int s = 1024;
    while (s > 128 && ((pixels + s - 1) / s) * tiles < 512) s >>= 1;
    return s;
}

// The rows of X that the output pixels pair with, for a 1x1 convolution of stride 1 or 2 (k24_resnet_backward.hip): output pixel
// p = (b, oy, ox) of a (Ho, Wo) map reads input row pin(p) = b H_in W_in + stride (oy W_in + ox).  Counts fit 30 bits (the host checks).
struct C1wGather {
    int Wo, HoWo, W_in, HWin, stride;
};

// GATHER = false: X's rows are the pixels as they lie there (K23; `g` is not read).  GATHER = true: row p of X is X + pin(p) C, taken in the
// staging loads and never materialised.
template <bool GATHER>
__global__ void __launch_bounds__(256, 2) k_conv1x1_wgrad(const float* __restrict__ X, const float* __restrict__ dY, const int64_t pixels, const int C, const int K,
                                                       const int slice_px, const float* __restrict__ x_amax, const float* __restrict__ dy_amax,
                                                       float* __restrict__ partials, const C1wGather g) {
    __shared__ __attribute__((aligned(16))) float ds[C1W_STEP * C1W_DS];
    __shared__ __attribute__((aligned(16))) float xs[C1W_STEP * C1W_XS];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int i32 = lane & 31, h = lane >> 5, kb = wave & 1, cw = wave >> 1;
    const int slice = blockIdx.x, k0 = blockIdx.y * C1W_KT, c0 = blockIdx.z * C1W_CT;
    const float sx = sg_activation_scale(x_amax), sd = sg_activation_scale(dy_amax);
    const int64_t p_begin = (int64_t)slice * slice_px;
    const int64_t p_end = p_begin + slice_px < pixels ? p_begin + slice_px : pixels;
    // staging: dY 32 pixels x 16 channel quads = 2 quads a thread, X 32 pixels x 32 quads = 4 quads a thread
    const int dq = t & 15, dp = t >> 4;          // dY: quad, pixel (+ 16 for the second)
    const int xq = t & 31, xp = t >> 5;          // X: quad, pixel (+ 8 j)
    const bool x_in = c0 + 4 * xq < C;           // (C % 16 == 0: a quad is inside or outside as a whole)

    const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
    f32x4 dreg[2], xreg[4];
    auto load = [&](int64_t p0) {                // the step's rows -> registers, zeros past the slice's last pixel and past C
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int64_t p = p0 + dp + 16 * j;
            dreg[j] = p < p_end ? *reinterpret_cast<const f32x4*>(dY + p * K + k0 + 4 * dq) : zero4;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int64_t p = p0 + xp + 8 * j;
            if constexpr (GATHER) {
                xreg[j] = zero4;
                if (p < p_end && x_in) {
                    const uint32_t up = (uint32_t)p, b = up / (uint32_t)g.HoWo, r = up - b * (uint32_t)g.HoWo, oy = r / (uint32_t)g.Wo, ox = r - oy * (uint32_t)g.Wo;
                    const int64_t pin = (int64_t)(b * (uint32_t)g.HWin + (uint32_t)g.stride * (oy * (uint32_t)g.W_in + ox));
                    xreg[j] = *reinterpret_cast<const f32x4*>(X + pin * C + c0 + 4 * xq);
                }
            } else {
                xreg[j] = (p < p_end && x_in) ? *reinterpret_cast<const f32x4*>(X + p * C + c0 + 4 * xq) : zero4;
            }
        }
    };

    const f32x16 zero16 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    f32x16 acc[2] = {zero16, zero16};

    load(p_begin);
    for (int64_t p0 = p_begin; p0 < p_end; p0 += C1W_STEP) {
#pragma unroll
        for (int j = 0; j < 2; ++j) *reinterpret_cast<f32x4*>(ds + (dp + 16 * j) * C1W_DS + 4 * dq) = dreg[j];
#pragma unroll
        for (int j = 0; j < 4; ++j) *reinterpret_cast<f32x4*>(xs + (xp + 8 * j) * C1W_XS + 4 * xq) = xreg[j];
        __syncthreads();
        if (p0 + C1W_STEP < p_end) load(p0 + C1W_STEP);      // (uniform) in flight behind the products below
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            if (p0 + 16 * s >= p_end) break;                 // (uniform) a half step of zeros
            // the lane's 8 pixels 16 s + 8 h .. + 7 of channel 32 kb + i32 of dY, split
            sg_u32x4 dyf[2];
            {
                const float* p = ds + (16 * s + 8 * h) * C1W_DS + 32 * kb + i32;
#pragma unroll
                for (int m = 0; m < 4; ++m) {
                    uint32_t w[2];
                    wino_f16_split2(p[(2 * m) * C1W_DS], p[(2 * m + 1) * C1W_DS], sd, w);
                    dyf[0][m] = w[0];
                    dyf[1][m] = w[1];
                }
            }
#pragma unroll
            for (int cb = 0; cb < 2; ++cb) {
                sg_u32x4 xf[2];
                const float* p = xs + (16 * s + 8 * h) * C1W_XS + 64 * cw + 32 * cb + i32;
#pragma unroll
                for (int m = 0; m < 4; ++m) {
                    uint32_t w[2];
                    wino_f16_split2(p[(2 * m) * C1W_XS], p[(2 * m + 1) * C1W_XS], sx, w);
                    xf[0][m] = w[0];
                    xf[1][m] = w[1];
                }
                // small products first (as k12 / k13 / k22)
                f32x16 a = acc[cb];
                a = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(wino_f16x8, dyf[0]), __builtin_bit_cast(wino_f16x8, xf[1]), a, 0, 0, 0);
                a = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(wino_f16x8, dyf[1]), __builtin_bit_cast(wino_f16x8, xf[0]), a, 0, 0, 0);
                a = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(wino_f16x8, dyf[0]), __builtin_bit_cast(wino_f16x8, xf[0]), a, 0, 0, 0);
                acc[cb] = a;
            }
        }
        __syncthreads();
    }

    // partial sums [slice][k < K][c < C]: accumulator register j of a lane is row (j & 3) + 8 (j >> 2) + 4 h, column i32
    const float inv = wino_pow2_inverse(sx) * wino_pow2_inverse(sd);
#pragma unroll
    for (int cb = 0; cb < 2; ++cb) {
        const int c = c0 + 64 * cw + 32 * cb + i32;
        if (c < C) {
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const int k = k0 + 32 * kb + (j & 3) + 8 * (j >> 2) + 4 * h;
                partials[((int64_t)slice * K + k) * C + c] = acc[cb][j] * inv;
            }
        }
    }
}

// Host.  The partial buffer of a weight gradient: the db partials [chunk][k < Kpad] in fp64 (two floats each), then the slices' partial sums
// [slice][tap][k < Kpad][c < C].
struct WgradLayout {
    int64_t n_slices, n_chunks, db_floats, floats;
    double* dbp(float* partials) const { return reinterpret_cast<double*>(partials); }
    float* wp(float* partials) const { return partials + db_floats; }
};
static inline WgradLayout wgrad_layout(int64_t pixels, int64_t n_slices, int Kpad, int taps, int C) {
    const int64_t n_chunks = (pixels + WG_DB_CHUNK - 1) / WG_DB_CHUNK, db_floats = 2 * n_chunks * Kpad;
    return WgradLayout{n_slices, n_chunks, db_floats, db_floats + n_slices * taps * Kpad * C};
}

// Host.  What every weight-gradient entry does behind its geometry check.  The arguments: only db may be null (no bias gradient); dW, db and
// partials alias neither each other nor an operand; the slices and chunks fit the grid's x.  Then the three launches: the db partials (if
// db), main(wp) -- the caller's kernel, which writes the slices' partials -- and the fixed-order fp64 reduction into dW (K, C, TAPS), db (K).
template <int TAPS, class Main>
static inline int wgrad_launch(const float* x, const float* dy, int64_t pixels, int C, int K, int Kpad, const float* x_amax, const float* dy_amax, const WgradLayout& L,
                               float* partials, float* dW, float* db, hipStream_t s, Main&& main) {
    if (!x || !dy || !x_amax || !dy_amax || !dW || !partials) return POD_E_INVALID;
    if (!pod_aligned(16, x, dy, partials) || !pod_aligned(4, x_amax, dy_amax, dW, db)) return POD_E_INVALID;
    if (dW == x || dW == dy || dW == partials || x == partials || dy == partials) return POD_E_INVALID;
    if (db && (db == dW || db == partials || db == x || db == dy)) return POD_E_INVALID;
    if (L.n_slices > 0x7FFFFFFF || L.n_chunks > 0x7FFFFFFF) return POD_E_INVALID;
    double* dbp = L.dbp(partials);
    float* wp = L.wp(partials);
    if (db) {
        hipLaunchKernelGGL(k_wgrad_db<WG_DB_CHUNK>, dim3((unsigned)L.n_chunks, (unsigned)(Kpad / 64)), dim3(256), 0, s, dy, pixels, Kpad, dbp);
        POD_CHECK_LAUNCH();
    }
    main(wp);
    POD_CHECK_LAUNCH();
    const int64_t n_out = (int64_t)TAPS * K * C + (db ? K : 0);
    hipLaunchKernelGGL(k_wgrad_reduce<TAPS>, dim3((unsigned)((n_out + 255) / 256)), dim3(256), 0, s, wp, (int)L.n_slices, dbp, (int)L.n_chunks, C, K, Kpad, dW, db);
    POD_CHECK_LAUNCH();
    return POD_OK;
}

// Host.  pod_conv1x1_wgrad (GATHER = false) and pod_conv1x1_wgrad_strided (false at stride 1, true at 2) behind their geometry checks.
static inline WgradLayout c1w_layout(int64_t pixels, int C, int K) {
    const int sp = c1w_slice_pixels(pixels, C, K);
    return wgrad_layout(pixels, (pixels + sp - 1) / sp, K, 1, C);
}
template <bool GATHER>
static inline int c1w_launch(const float* x, const float* dy, int64_t pixels, int C, int K, const C1wGather g, const float* x_amax, const float* dy_amax, float* dW,
                             float* db, float* partials, hipStream_t s) {
    const WgradLayout L = c1w_layout(pixels, C, K);
    return wgrad_launch<1>(x, dy, pixels, C, K, K, x_amax, dy_amax, L, partials, dW, db, s, [&](float* wp) {
        hipLaunchKernelGGL(k_conv1x1_wgrad<GATHER>, dim3((unsigned)L.n_slices, (unsigned)(K / C1W_KT), (unsigned)((C + C1W_CT - 1) / C1W_CT)), dim3(256), 0, s, x, dy, pixels,
                           C, K, c1w_slice_pixels(pixels, C, K), x_amax, dy_amax, wp, g);
    });
}

// scale v where the gate's activation was positive, zero elsewhere: the backward of a ReLU (and dropout's 1 / (1 - p)) read off its stored output
__device__ __forceinline__ f32x4 gate4(f32x4 v, const f32x4 g, const float scale = 1.0f) {
    v.x = g.x > 0.f ? v.x * scale : 0.f;
    v.y = g.y > 0.f ? v.y * scale : 0.f;
    v.z = g.z > 0.f ? v.z * scale : 0.f;
    v.w = g.w > 0.f ? v.w * scale : 0.f;
    return v;
}

// out quad i = value(i) for the n4 quads of a launch, by grid stride; the abs-max of what is stored goes to `amax` (null: no record; the
// publish is uniform: the whole workgroup calls this).  `out` may be what value() reads at quad i: the read comes first.
template <class F>
__device__ __forceinline__ void quad_pass(float* out, const int64_t n4, float* __restrict__ amax, F&& value) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    float m = 0.0f;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
        const f32x4 v = value(i);
        reinterpret_cast<f32x4*>(out)[i] = v;
        m = wino_absmax4(m, v);
    }
    if (amax) wino_publish_amax_block(amax, m);
}

// The same over a channels-last (H, W, 4 C4) map: value(i, c4, x, y) for quad c4 of pixel (y, x).
template <class F>
__device__ __forceinline__ void map_quad_pass(float* out, const int H, const int W, const int C4, float* __restrict__ amax, F&& value) {
    quad_pass(out, (int64_t)H * W * C4, amax, [&](const int64_t i) {
        const int c4 = (int)(i % C4);
        const int64_t pix = i / C4;
        return value(i, c4, (int)(pix % W), (int)(pix / W));
    });
}

// Host: the check and launch the three map gathers share: `src` into the (out_pixels, C) map `out` behind an optional gate and addend of
// out's shape (`out` may be the addend); H, W: the larger of the two maps; launch(grid) enqueues the kernel.
template <class Launch>
static inline int map_gather(const float* src, const float* gate, const float* add, const float* out, int32_t H, int32_t W, int32_t C, const float* amax,
                             int64_t out_pixels, Launch&& launch) {
    if (!src || !out || src == out || gate == out || H < 1 || W < 1 || H > 16384 || W > 16384 || C < 4 || (C & 3) != 0) return POD_E_INVALID;
    if (!pod_aligned(16, src, gate, add, out) || !pod_aligned(4, amax)) return POD_E_INVALID;
    launch(dim3(pod_grid_stride_blocks(out_pixels * (C / 4), 4096)));
    POD_CHECK_LAUNCH();
    return POD_OK;
}

}  // namespace pod
