// Element-wise passes of the conv-net side of the path, each kernel followed by its entry point (include/pod_mi355x.h says what each
// computes and why it exists; the dropout mask they share: pod_device.h):
//   pod_bias_act, pod_relu_dropout      x = dropout(relu((x + bias) + (residual + res_bias))) in place, every stage optional
//   pod_expand_dropout                  `copies` dropout-perturbed copies of one tensor, a mask per copy
//   pod_bias_act_to_nchw / _to_nhwc     the same tail as pod_bias_act, written in the other memory layout  } 64 x 64 tiles
//   pod_wino_reduce                     the partial sums of a split convolution -> bias, ReLU, NCHW planes } through LDS
//   pod_absmax                          the abs-max record of a tensor
#include "pod_split_gemm.h"

namespace pod {

// ---- pod_bias_act: x[n, c, :] = dropout(relu((x + bias[c]) + (residual + res_bias[c])), p) in place.  torch's conv on ROCm is MIOpen's
// kernel followed by a separate bias `add_`; with ReLU (+ dropout, + the residual add of a bottleneck) that is 2-4 element-wise passes
// over the activation.  The convolution is called without its bias and this ONE pass does the rest: 16 B per lane, HBM-bound.
// pod_relu_dropout -- the `nn.ReLU(), nn.Dropout(p)` pair behind every 3x3 conv of the head's subnets -- is the same kernel without
// bias and residual.
struct BiasActParams {
    float* x;
    const float* bias;       // [C] or NULL
    const float* residual;   // same shape as x or NULL
    const float* res_bias;   // [C] or NULL (bias of the shortcut conv that produced `residual`)
    int64_t n4, n, HW;
    int32_t C, relu;
    uint32_t thresh;         // 0 = no dropout
    float scale;
    uint64_t seed, offset;
};

// (v + b) + r, ReLU: what pod_bias_act and pod_bias_act_to_nchw do to an element ahead of the mask; the two must agree to the bit.
// (k_bias_act keeps its float4 and float arrays on purpose: its three forms are the instructions they were before the mask rule moved
// into dropout_mask4; written on f32x4 the loop branches on `relu` -- profiles/model_ops_shared.md.)
__device__ __forceinline__ float bias_act_one(float v, float b, float r, int relu) {
    v = (v + b) + r;
    return relu ? fmaxf(v, 0.0f) : v;
}

// LAYOUT 0: NCHW planes, H*W % 4 == 0 (4 elements share a channel); 1: NHWC, C % 4 == 0 (4 consecutive channels:
// one 16-byte bias load); 2: anything else (per-element channel).
template <int LAYOUT>
__global__ void __launch_bounds__(256) k_bias_act(const BiasActParams P) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < P.n4; i += stride) {
        uint32_t w0 = 0xFFFFFFFFu, w1 = 0xFFFFFFFFu;
        if (P.thresh) dropout_words(P.offset, (uint64_t)i, 0u, P.seed, w0, w1);
        float4 v = *reinterpret_cast<const float4*>(P.x + i * 4);
        float4 res = float4{0.f, 0.f, 0.f, 0.f};
        if (P.residual) res = *reinterpret_cast<const float4*>(P.residual + i * 4);
        float b[4] = {0.f, 0.f, 0.f, 0.f}, rb[4] = {0.f, 0.f, 0.f, 0.f};
        if (LAYOUT == 0) {
            const int c = (int)(((i * 4) / P.HW) % P.C);
            if (P.bias) b[0] = b[1] = b[2] = b[3] = P.bias[c];
            if (P.res_bias) rb[0] = rb[1] = rb[2] = rb[3] = P.res_bias[c];
        } else if (LAYOUT == 1) {
            const int c = (int)((i * 4) % P.C);
            if (P.bias) {
                const float4 t = *reinterpret_cast<const float4*>(P.bias + c);
                b[0] = t.x; b[1] = t.y; b[2] = t.z; b[3] = t.w;
            }
            if (P.res_bias) {
                const float4 t = *reinterpret_cast<const float4*>(P.res_bias + c);
                rb[0] = t.x; rb[1] = t.y; rb[2] = t.z; rb[3] = t.w;
            }
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int c = (int)(((i * 4 + j) / P.HW) % P.C);
                if (P.bias) b[j] = P.bias[c];
                if (P.res_bias) rb[j] = P.res_bias[c];
            }
        }
        v.x = bias_act_one(v.x, b[0], res.x + rb[0], P.relu);
        v.y = bias_act_one(v.y, b[1], res.y + rb[1], P.relu);
        v.z = bias_act_one(v.z, b[2], res.z + rb[2], P.relu);
        v.w = bias_act_one(v.w, b[3], res.w + rb[3], P.relu);
        dropout_mask4(v, w0, w1, P.thresh, P.scale);
        *reinterpret_cast<float4*>(P.x + i * 4) = v;
    }
    if (blockIdx.x == 0 && threadIdx.x < (P.n & 3)) {   // tail (n % 4 elements)
        const int64_t e = P.n4 * 4 + threadIdx.x;
        const bool keep = !P.thresh || dropout_tail_keep(P.offset, P.n4, threadIdx.x, P.seed, P.thresh);
        const int c = (int)((e / P.HW) % P.C);
        const float res = (P.residual ? P.residual[e] : 0.0f) + (P.res_bias ? P.res_bias[c] : 0.0f);
        const float v = bias_act_one(P.x[e], P.bias ? P.bias[c] : 0.0f, res, P.relu);
        P.x[e] = keep ? v * P.scale : 0.0f;
    }
}

// Host: the dropout fields and sizes of P, and the launch of one layout (grid-stride: at most 16 workgroups per CU)
static int bias_act_launch(BiasActParams& P, int layout, int64_t n, float p, uint64_t seed, uint64_t offset, pod_stream_t stream) {
    P.n4 = n / 4; P.n = n;
    P.thresh = POD_DROPOUT_THRESH16(p);   // keep iff 16-bit field >= p * 2^16
    P.scale = 1.0f / (1.0f - p);
    P.seed = seed; P.offset = offset;
    const dim3 grid(pod_grid_stride_blocks(P.n4, 4096));
    if (layout == 0) hipLaunchKernelGGL(k_bias_act<0>, grid, dim3(256), 0, (hipStream_t)stream, P);
    else if (layout == 1) hipLaunchKernelGGL(k_bias_act<1>, grid, dim3(256), 0, (hipStream_t)stream, P);
    else hipLaunchKernelGGL(k_bias_act<2>, grid, dim3(256), 0, (hipStream_t)stream, P);
    POD_CHECK_LAUNCH();
    return POD_OK;
}

}  // namespace pod

extern "C" int pod_bias_act(float* x, const float* bias, const float* residual, const float* res_bias, int64_t n, int32_t C,
                            int64_t HW, int32_t relu, float p, uint64_t seed, uint64_t offset, pod_stream_t stream) {
    if (!x || n < 0 || C < 1 || HW < 1 || !(p >= 0.0f && p < 1.0f)) return POD_E_INVALID;
    if (!pod_aligned(16, x, residual)) return POD_E_INVALID;
    if (res_bias && !residual) return POD_E_INVALID;
    if (n % ((int64_t)C * HW) != 0) return POD_E_INVALID;   // x is (N, C, H, W)
    if (n == 0) return POD_OK;
    pod::BiasActParams P;
    P.x = x; P.bias = bias; P.residual = residual; P.res_bias = res_bias;
    P.HW = HW; P.C = C; P.relu = relu;
    const int layout = HW % 4 == 0 ? 0 : HW == 1 && C % 4 == 0 && pod_aligned(16, bias, res_bias) ? 1 : 2;
    return pod::bias_act_launch(P, layout, n, p, seed, offset, stream);
}

extern "C" int pod_relu_dropout(float* x, int64_t n, float p, uint64_t seed, uint64_t offset, pod_stream_t stream) {
    if (!x || n < 0 || !(p >= 0.0f && p < 1.0f) || !pod_aligned(16, x)) return POD_E_INVALID;
    if (n == 0) return POD_OK;
    pod::BiasActParams P;
    P.x = x; P.bias = nullptr; P.residual = nullptr; P.res_bias = nullptr;
    P.HW = 4; P.C = 1; P.relu = 1;        // (one channel: without a bias nothing reads it)
    return pod::bias_act_launch(P, 0, n, p, seed, offset, stream);
}

// ---- pod_expand_dropout: dst[c][i] = dropout(src[i], p) for c < copies, an independent mask per copy.  The first conv of a head subnet
// sees the same input in every MC run, so it is evaluated once; this writes the `copies` dropout-perturbed inputs of the second conv in
// one pass (torch: expand + fused_dropout, which also writes a mask tensor).  Flat arrays: any memory format, as long as src and every
// dst copy use the same one.
namespace pod {
__global__ void __launch_bounds__(256) k_expand_dropout(const float* __restrict__ src, float* __restrict__ dst, int64_t n4, int32_t copies,
                                                        uint32_t thresh, float scale, uint64_t seed, uint64_t offset, const uint64_t* __restrict__ epoch) {
    seed = dropout_key(seed, epoch);
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(src + i * 4);
        for (int c = 0; c < copies; ++c) {
            uint32_t w0, w1;
            dropout_words(offset, (uint64_t)c * (uint64_t)n4 + (uint64_t)i, 2u, seed, w0, w1);
            f32x4 o = v;
            dropout_mask4(o, w0, w1, thresh, scale);
            *reinterpret_cast<f32x4*>(dst + ((int64_t)c * n4 + i) * 4) = o;
        }
    }
}
}  // namespace pod

extern "C" int pod_expand_dropout(const float* src, float* dst, int64_t n, int32_t copies, float p, uint64_t seed, uint64_t offset,
                                  const uint64_t* epoch, pod_stream_t stream) {
    if (!src || !dst || n < 0 || (n & 3) != 0 || copies < 1 || !(p >= 0.0f && p < 1.0f)) return POD_E_INVALID;
    if (!pod_aligned(16, src, dst)) return POD_E_INVALID;
    if (n == 0) return POD_OK;
    const int64_t n4 = n / 4;
    hipLaunchKernelGGL(pod::k_expand_dropout, dim3(pod_grid_stride_blocks(n4, 4096)), dim3(256), 0, (hipStream_t)stream, src, dst, n4, copies,
                       POD_DROPOUT_THRESH16(p), 1.0f / (1.0f - p), seed, offset, epoch);
    POD_CHECK_LAUNCH();
    return POD_OK;
}

// ---- The 64 x 64 transposes through LDS.  A workgroup (256 threads) moves one tile of 64 cells (along H*W) x 64 channels between a
// channels-last [cell][C] tensor and NCHW planes: 16-byte accesses along C on one side, along H*W on the other (scalar where H*W % 4
// != 0), the padded tile in between.  Thread -> row tid / 16 + 16 it (it = 0 .. 3) and the 4 columns at (tid % 16) * 4, on both sides.
namespace pod {
typedef float TileLds[64][65];
struct TilePos {
    int64_t n, hw0;      // image; first cell of the tile
    int c0;              // first channel
};
// workgroup -> tile: channel tiles fastest, then the cell tiles of an image, then the images (the grid fits 31 bits: tile_grid)
__device__ __forceinline__ TilePos tile_pos(int tiles_hw, int tiles_c) {
    unsigned t = blockIdx.x;
    TilePos T;
    T.c0 = (int)(t % (unsigned)tiles_c) * 64;
    t /= (unsigned)tiles_c;
    T.hw0 = (int64_t)(t % (unsigned)tiles_hw) * 64;
    T.n = t / (unsigned)tiles_hw;
    return T;
}
__device__ __forceinline__ int tile_row(int it) { return (int)(threadIdx.x >> 4) + 16 * it; }
__device__ __forceinline__ int tile_col4() { return (int)(threadIdx.x & 15) * 4; }
__device__ __forceinline__ void tile_scatter4(TileLds& tile, int row, int col4, const f32x4& v) {     // 4 values along a row
    tile[row][col4 + 0] = v.x; tile[row][col4 + 1] = v.y; tile[row][col4 + 2] = v.z; tile[row][col4 + 3] = v.w;
}
__device__ __forceinline__ f32x4 tile_gather4(const TileLds& tile, int row4, int col) {               // 4 values down a column
    return f32x4{tile[row4 + 0][col], tile[row4 + 1][col], tile[row4 + 2][col], tile[row4 + 3][col]};
}
// The 4 consecutive floats along H*W at p, `left` of them inside the plane (<= 0: none): one 16-byte access where the planes allow it
// (vec: H*W % 4 == 0 -- every plane then starts on 16 bytes and left is a multiple of 4), guarded scalars otherwise.
__device__ __forceinline__ f32x4 tile_load4_hw(const float* p, int64_t left, bool vec) {
    f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
    if (vec && left > 0) {
        v = *reinterpret_cast<const f32x4*>(p);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (j < left) v[j] = p[j];
    }
    return v;
}
__device__ __forceinline__ void tile_store4_hw(float* p, int64_t left, bool vec, const f32x4& v) {
    if (vec && left > 0) {
        *reinterpret_cast<f32x4*>(p) = v;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (j < left) p[j] = v[j];
    }
}
// Host: the grid of N images; -1: more workgroups than a grid holds
static int64_t tile_grid(int64_t N, int32_t C, int64_t HW, int32_t& tiles_hw, int32_t& tiles_c) {
    const int64_t th = (HW + 63) / 64, tc = (C + 63) / 64, blocks = N * th * tc;
    if (blocks > 0x7FFFFFFFLL || th > 0x7FFFFFFFLL) return -1;
    tiles_hw = (int32_t)th; tiles_c = (int32_t)tc;
    return blocks;
}

// pod_bias_act_to_nchw: the tail of pod_bias_act for a channels-last conv output, written as NCHW planes -- the layout change rides on
// the element-wise pass that exists anyway (a separate transposing copy of the 300 MB p3 trunk output costs 0.3 ms in torch).  Bias on
// load; ReLU and mask on store, the dropout fields those of pod_bias_act on the NCHW result (float4 group = NCHW float4 index), so the
// output equals "transpose, then pod_bias_act" bit for bit.  H*W % 4 == 0.
__global__ void __launch_bounds__(256) k_bias_act_to_nchw(const float* __restrict__ src, float* __restrict__ dst, const float* __restrict__ bias,
                                                          int32_t C, int64_t HW, int32_t relu, uint32_t thresh, float scale, uint64_t seed,
                                                          uint64_t offset, int32_t tiles_hw, int32_t tiles_c) {
    __shared__ TileLds tile;         // [cell][channel]
    const TilePos T = tile_pos(tiles_hw, tiles_c);
#pragma unroll
    for (int it = 0; it < 4; ++it) {
        const int r = tile_row(it), c4 = tile_col4();
        f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
        if (T.hw0 + r < HW && T.c0 + c4 < C) {
            v = *reinterpret_cast<const f32x4*>(src + ((T.n * HW + T.hw0 + r) * C + T.c0 + c4));
            if (bias) v += *reinterpret_cast<const f32x4*>(bias + T.c0 + c4);
        }
        tile_scatter4(tile, r, c4, v);
    }
    __syncthreads();
#pragma unroll
    for (int it = 0; it < 4; ++it) {
        const int c = tile_row(it), h4 = tile_col4();
        if (T.c0 + c >= C || T.hw0 + h4 >= HW) continue;
        const int64_t e = (T.n * C + T.c0 + c) * HW + T.hw0 + h4;   // NCHW element index, a multiple of 4
        uint32_t w0 = 0xFFFFFFFFu, w1 = 0xFFFFFFFFu;
        if (thresh) dropout_words(offset, (uint64_t)(e >> 2), 0u, seed, w0, w1);
        const f32x4 t = tile_gather4(tile, h4, c);
        f32x4 v = f32x4{bias_act_one(t.x, 0.0f, 0.0f, relu), bias_act_one(t.y, 0.0f, 0.0f, relu), bias_act_one(t.z, 0.0f, 0.0f, relu),
                        bias_act_one(t.w, 0.0f, 0.0f, relu)};      // (the bias went in on load)
        dropout_mask4(v, w0, w1, thresh, scale);
        *reinterpret_cast<f32x4*>(dst + e) = v;
    }
}
}  // namespace pod

extern "C" int pod_bias_act_to_nchw(const float* src, float* dst, const float* bias, int64_t N, int32_t C, int64_t HW, int32_t relu,
                                    float p, uint64_t seed, uint64_t offset, pod_stream_t stream) {
    if (!src || !dst || src == dst || N < 0 || C < 4 || (C & 3) != 0 || HW < 4 || (HW & 3) != 0 || !(p >= 0.0f && p < 1.0f)) return POD_E_INVALID;
    if (!pod_aligned(16, src, dst, bias)) return POD_E_INVALID;
    if (N == 0) return POD_OK;
    int32_t tiles_hw, tiles_c;
    const int64_t blocks = pod::tile_grid(N, C, HW, tiles_hw, tiles_c);
    if (blocks < 0) return POD_E_INVALID;
    hipLaunchKernelGGL(pod::k_bias_act_to_nchw, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, src, dst, bias, C, HW, relu,
                       POD_DROPOUT_THRESH16(p), 1.0f / (1.0f - p), seed, offset, tiles_hw, tiles_c);
    POD_CHECK_LAUNCH();
    return POD_OK;
}

// pod_bias_act_to_nhwc: the reverse trip, for a conv whose CONSUMER is pod_wino_conv3x3 (channels-last input): the bias + ReLU pass that
// follows an NCHW (MIOpen) conv anyway writes [cell][C] instead of planes.  Bias and ReLU on load.
namespace pod {
__global__ void __launch_bounds__(256) k_bias_act_to_nhwc(const float* __restrict__ src, float* __restrict__ dst, const float* __restrict__ bias,
                                                          int32_t C, int64_t HW, int32_t relu, int32_t tiles_hw, int32_t tiles_c) {
    __shared__ TileLds tile;         // [channel][cell]
    const TilePos T = tile_pos(tiles_hw, tiles_c);
    const bool vec = (HW & 3) == 0;
#pragma unroll
    for (int it = 0; it < 4; ++it) {
        const int c = tile_row(it), h4 = tile_col4();
        f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
        if (T.c0 + c < C) {
            v = tile_load4_hw(src + (T.n * C + T.c0 + c) * HW + T.hw0 + h4, HW - (T.hw0 + h4), vec);
            v += bias ? bias[T.c0 + c] : 0.0f;
            if (relu) wino_relu4(v);
        }
        tile_scatter4(tile, c, h4, v);
    }
    __syncthreads();
#pragma unroll
    for (int it = 0; it < 4; ++it) {
        const int r = tile_row(it), c4 = tile_col4();
        if (T.hw0 + r >= HW || T.c0 + c4 >= C) continue;
        *reinterpret_cast<f32x4*>(dst + ((T.n * HW + T.hw0 + r) * C + T.c0 + c4)) = tile_gather4(tile, c4, r);
    }
}
}  // namespace pod

extern "C" int pod_bias_act_to_nhwc(const float* src, float* dst, const float* bias, int64_t N, int32_t C, int64_t HW, int32_t relu,
                                    pod_stream_t stream) {
    if (!src || !dst || src == dst || N < 0 || C < 4 || (C & 3) != 0 || HW < 1) return POD_E_INVALID;
    if (!pod_aligned(16, src, dst)) return POD_E_INVALID;
    if (N == 0) return POD_OK;
    int32_t tiles_hw, tiles_c;
    const int64_t blocks = pod::tile_grid(N, C, HW, tiles_hw, tiles_c);
    if (blocks < 0) return POD_E_INVALID;
    hipLaunchKernelGGL(pod::k_bias_act_to_nhwc, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, src, dst, bias, C, HW, relu, tiles_hw, tiles_c);
    POD_CHECK_LAUNCH();
    return POD_OK;
}

// pod_wino_reduce: finishes a convolution that pod_wino_conv3x3_split_partial cut over its input channels -- the n_splits channels-last
// partial sums (pixels, Kpad) are added in a fixed order, bias and ReLU applied (pod_split_gemm.h: sg_split_sum4; Kpad bias values: the
// caller's bias is padded with zeros) and the abs-max taken on load; the K real channels are written as NCHW planes of one image
// (HW = pixels): what the consumer of a backbone convolution reads.
namespace pod {
__global__ void __launch_bounds__(256) k_wino_reduce(const float* __restrict__ partials, int32_t n_splits, int64_t split_stride, const float* __restrict__ bias,
                                                     float* __restrict__ planes, int64_t HW, int32_t Kpad, int32_t K, int32_t relu, int32_t tiles_hw,
                                                     int32_t tiles_c, float* __restrict__ out_amax) {
    float lmax = 0.0f;
    __shared__ TileLds tile;         // [pixel][channel]
    const TilePos T = tile_pos(tiles_hw, tiles_c);
#pragma unroll
    for (int it = 0; it < 4; ++it) {
        const int r = tile_row(it), c4 = tile_col4();
        f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
        if (T.hw0 + r < HW && T.c0 + c4 < Kpad)
            v = sg_split_sum4(partials, (T.hw0 + r) * Kpad + T.c0 + c4, n_splits, split_stride, bias, [&](int64_t) { return T.c0 + c4; }, nullptr, relu);
        tile_scatter4(tile, r, c4, v);
        lmax = wino_absmax4(lmax, v);     // (padded channels: 0 + 0)
    }
    if (out_amax) wino_publish_amax_block(out_amax, lmax);
    __syncthreads();
    const bool vec = (HW & 3) == 0;
#pragma unroll
    for (int it = 0; it < 4; ++it) {
        const int c = tile_row(it), h4 = tile_col4();
        if (T.c0 + c >= K || T.hw0 + h4 >= HW) continue;
        tile_store4_hw(planes + (int64_t)(T.c0 + c) * HW + T.hw0 + h4, HW - (T.hw0 + h4), vec, tile_gather4(tile, h4, c));
    }
}
}  // namespace pod

extern "C" int pod_wino_reduce(const float* partials, int32_t n_splits, int64_t split_stride, const float* bias, float* planes, int64_t HW,
                               int32_t Kpad, int32_t K, int32_t relu, float* out_amax, pod_stream_t stream) {
    if (!partials || !planes || n_splits < 1 || n_splits > 16 || HW < 1 || Kpad < 4 || (Kpad & 3) != 0 || K < 1 || K > Kpad) return POD_E_INVALID;
    if (n_splits > 1 && (split_stride < HW * Kpad || (split_stride & 3) != 0)) return POD_E_INVALID;
    if (!pod_aligned(16, partials, planes, bias)) return POD_E_INVALID;
    const int64_t tiles_hw = (HW + 63) / 64, tiles_c = (K + 63) / 64;
    hipLaunchKernelGGL(pod::k_wino_reduce, dim3((unsigned)(tiles_hw * tiles_c)), dim3(256), 0, (hipStream_t)stream, partials, n_splits, split_stride, bias,
                       planes, HW, Kpad, K, relu, (int32_t)tiles_hw, (int32_t)tiles_c, out_amax);
    POD_CHECK_LAUNCH();
    return POD_OK;
}

// ---- pod_absmax: the abs-max of a tensor, max'ed into *amax (pod_mi355x.h: operand abs-max words)
namespace pod {
__global__ void __launch_bounds__(256) k_absmax(const float* __restrict__ x, int64_t n, float* __restrict__ amax) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x * 4;
    float m = 0.0f;
    int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    for (; i + 3 < n; i += stride) m = wino_absmax4(m, *reinterpret_cast<const f32x4*>(x + i));
    for (; i < n; ++i) m = fmaxf(m, fabsf(x[i]));        // (the tail of an n that is not a multiple of 4: one thread)
    wino_publish_amax_block(amax, m);
}
}  // namespace pod

extern "C" int pod_absmax(const float* x, int64_t n, float* amax, pod_stream_t stream) {
    if (!x || !amax || n < 0 || !pod_aligned(16, x) || !pod_aligned(4, amax)) return POD_E_INVALID;
    if (n == 0) return POD_OK;
    hipLaunchKernelGGL(pod::k_absmax, dim3(pod_grid_stride_blocks(n / 4, 1024)), dim3(256), 0, (hipStream_t)stream, x, n, amax);
    POD_CHECK_LAUNCH();
    return POD_OK;
}
