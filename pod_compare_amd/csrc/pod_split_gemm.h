// The split GEMM's shared home: an fp32 product formed on the f16 matrix cores from the two-term f16 split of the power-of-two-scaled
// operands.  First what every split kernel uses (k12 through pod_wino.h; k8 / k10 for the abs-max records and the test hook): the f16
// split, the abs-max records, the four-lane ReLU and abs-max, the fixed-order sum of a split convolution's partials.  Then the 64-pixel x 64-channel GEMM TILE of k13_conv1x1_split.hip and
// k14_stem_conv.hip, each part written once: constants and types, the activation and inverse scales, the filter ring's load, the k-step
// (split + three partial products), the whole-line epilogue through LDS, and the filter preparation (abs-max kernel, term store, host
// sequence).  A kernel keeps what is its own: where its activations come from, and where its pixels go.
#pragma once
#include <type_traits>
#include <utility>

#include "pod_device.h"

namespace pod {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x2 __attribute__((ext_vector_type(2)));      // (f32x4: pod_device.h)

// ---- an fp32 value as the sum of two FP16 values (round 5: k12 / k13 / k14; pod_debug_f16_split2 exposes the same code to the tests)
// The f16 matrix cores run at the bf16 rate, and two f16 terms carry 11 + 1 (the sign of the residual) + 11 = 23 of an fp32's 24
// significand bits: x s = x0 + x1 + e, |e| <= 2^-23 |x s| in the worst case (exact whenever the residual has <= 11 significant bits), where
// x0 = f16(x s) (round to nearest even), r = x s - x0 EXACTLY (one fma), x1 = f16(r).  Three partial products (x0 u1, x1 u0, x0 u0) then form
// an fp32 product where the 3-way bf16 split needs six -- and with half as many roundings in the fp32 accumulation chain the result is
// CLOSER to the fp64 value than both the bf16 x 6 form and the fp32 MFMA (measured on the matrix cores: tools/f16_split_numerics.hip,
// profiles/r05_f16_split_numerics.txt).  What f16 lacks is range (2^-24 .. 65504): every operand tensor is therefore multiplied by a
// power of two s (exact) chosen from its abs-max, so that the largest scaled value lies in [2^14, 2^15) (filters; static) or below 2^15
// (activations: abs-max word of the producing launch x the largest gain of the transform); values more than ~2^29 below their tensor's
// abs-max fall into f16's denormals and keep an ABSOLUTE error of 2^-25 / s -- 2^-40 of the abs-max, against an fp32 rounding's 2^-24 |x|.
typedef _Float16 wino_f16x2 __attribute__((ext_vector_type(2)));
typedef _Float16 wino_f16x8 __attribute__((ext_vector_type(8)));
// 2^(top - floor(log2 amax)): the power of two that puts amax into [2^top, 2^(top+1)).  amax = 0 or absurdly small: the largest scale (the
// operand is zero / all products underflow anyway); inf / nan: the smallest (the products are inf / nan, as an fp32 product would be).
__device__ __forceinline__ float wino_pow2_scale(float amax, int top) {
    const int E = (int)((__float_as_uint(amax) >> 23) & 0xFFu);
    int b = 254 + top - E;
    b = b < 1 ? 1 : b > 254 ? 254 : b;
    return __uint_as_float((uint32_t)b << 23);
}
__device__ __forceinline__ float wino_pow2_inverse(float s) {        // 1 / s for a power of two s = 2^k, |k| <= 126: exact
    return __uint_as_float((254u << 23) - __float_as_uint(s));
}
// (lo s, hi s) -> the f16 pair nearest to them (v_fma_mixlo_f16 / v_fma_mixhi_f16: the scaling rides on the conversion)
__device__ __forceinline__ uint32_t wino_f16_pair_scaled(float lo, float hi, float s) {
    uint32_t w;
    asm("v_fma_mixlo_f16 %0, %1, %3, 0\n\tv_fma_mixhi_f16 %0, %2, %3, 0" : "=&v"(w) : "v"(lo), "v"(hi), "s"(s));
    return w;
}
__device__ __forceinline__ uint32_t wino_f16_pair(float lo, float hi) {              // v_cvt_pk_f16_f32: nearest even, lo in bits 15:0
    return __builtin_bit_cast(uint32_t, __builtin_convertvector(f32x2{lo, hi}, wino_f16x2));
}
// (lo, hi) <- (lo s, hi s) - the f16 pair w, exactly: one v_fma_mix_f32 per value (f32 x f32 - f16, a single rounding of a result that is
// representable: |x s - x0| <= 2^-11 |x s| and both are multiples of the last place of x s)
__device__ __forceinline__ void wino_f16_residual_scaled(uint32_t w, float& lo, float& hi, float s) {
    asm("v_fma_mix_f32 %0, %0, %1, -%2 op_sel_hi:[0,0,1]" : "+v"(lo) : "s"(s), "v"(w));
    asm("v_fma_mix_f32 %0, %0, %1, -%2 op_sel:[0,0,1] op_sel_hi:[0,0,1]" : "+v"(hi) : "s"(s), "v"(w));
}
__device__ __forceinline__ void wino_f16_split2(float lo, float hi, float s, uint32_t (&w)[2]) {
    w[0] = wino_f16_pair_scaled(lo, hi, s);
    wino_f16_residual_scaled(w[0], lo, hi, s);
    w[1] = wino_f16_pair(lo, hi);
}
// ---- operand abs-max RECORDS (include/pod_mi355x.h).  The abs-max of a tensor lives in POD_AMAX_SLOTS words POD_AMAX_STRIDE floats apart
// (one 128-byte line each); a producer max'es into slot (workgroup + wavefront) mod 16, a consumer takes the largest of the 16.  One word
// would do for the arithmetic -- but thousands of same-address atomics serialise in the L2 at ~10 ns each, and the wavefronts of a
// streaming launch all finish together (measured with one word: pod_absmax of 22 MB 109 us, a 5-us reduce launch 47 us).
// (POD_AMAX_SLOTS = 16, POD_AMAX_STRIDE = 32, POD_AMAX_FLOATS = 512: include/pod_mi355x.h)
// floats >= 0 order like their bit patterns: an integer atomic max.  One atomic per wavefront at most, skipped when the slot already holds more.
__device__ __forceinline__ void wino_publish_amax1(float* word, float lmax) {      // one wavefront's maximum into ONE word (a filter's trailer)
#pragma unroll
    for (int o = 32; o; o >>= 1) lmax = fmaxf(lmax, __shfl_xor(lmax, o));
    if ((threadIdx.x & 63) == 0 && lmax > 0.0f) {
        uint32_t* w = reinterpret_cast<uint32_t*>(word);
        const uint32_t bits = __float_as_uint(lmax);
        if (__hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < bits) atomicMax(w, bits);
    }
}
__device__ __forceinline__ void wino_publish_amax(float* rec, float lmax) {        // ... into its slot of a record
    const unsigned wg = blockIdx.x + blockIdx.y * gridDim.x;
    wino_publish_amax1(rec + ((wg * (blockDim.x >> 6) + (threadIdx.x >> 6)) & (POD_AMAX_SLOTS - 1)) * POD_AMAX_STRIDE, lmax);
}
// the same for a whole workgroup (every thread calls it; <= 16 wavefronts): ONE atomic per workgroup
__device__ __forceinline__ void wino_publish_amax_block(float* rec, float lmax) {
    __shared__ float wave_max[16];
#pragma unroll
    for (int o = 32; o; o >>= 1) lmax = fmaxf(lmax, __shfl_xor(lmax, o));
    if ((threadIdx.x & 63) == 0) wave_max[threadIdx.x >> 6] = lmax;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (unsigned w = 1; w < (blockDim.x >> 6); ++w) lmax = fmaxf(lmax, wave_max[w]);
        if (lmax > 0.0f) {
            uint32_t* word = reinterpret_cast<uint32_t*>(rec + ((blockIdx.x + blockIdx.y * gridDim.x) & (POD_AMAX_SLOTS - 1)) * POD_AMAX_STRIDE);
            const uint32_t bits = __float_as_uint(lmax);
            if (__hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < bits) atomicMax(word, bits);
        }
    }
}
__device__ __forceinline__ float wino_load_amax(const float* rec) {                // this lane's slot of the record (ask early, reduce late)
    const int lane = threadIdx.x & 63;
    return lane < POD_AMAX_SLOTS ? rec[lane * POD_AMAX_STRIDE] : 0.0f;
}
__device__ __forceinline__ float wino_reduce_amax(float v) {                       // the record's value, wave-uniform (a scalar register)
#pragma unroll
    for (int o = POD_AMAX_SLOTS / 2; o; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, v)));
}
__device__ __forceinline__ float wino_read_amax(const float* rec) { return wino_reduce_amax(wino_load_amax(rec)); }

template <typename F, int... Js>
__device__ __forceinline__ void wino_static_for(F&& f, std::integer_sequence<int, Js...>) {
    (f(std::integral_constant<int, Js>{}), ...);
}

// ---- four lanes at once: ReLU, and max(lmax, |v|)
__device__ __forceinline__ void wino_relu4(f32x4& v) {
    v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f);
}
__device__ __forceinline__ float wino_absmax4(float lmax, const f32x4& v) {
    return fmaxf(fmaxf(lmax, fabsf(v.x)), fmaxf(fmaxf(fabsf(v.y), fabsf(v.z)), fabsf(v.w)));
}

// ---- the end of a convolution cut over its input channels (k13's own reduce, pod_reduce_partials, pod_wino_reduce): the four values at
// element e of the n_splits channels-last partial sums, `split_stride` floats apart, added in a FIXED order -- split 0 first, then
// 1 .. n - 1, then the bias, then the residual (either may be null) -- so that the result does not depend on scheduling; then ReLU.
// channel(e) -> the first of the four channels of element e: asked for only with a bias (k13 pays a division for it; as a plain argument
// the division leaves `if (bias)` and k_conv1x1_reduce comes out as other code than before -- profiles/model_ops_shared.md).
template <typename Channel>
__device__ __forceinline__ f32x4 sg_split_sum4(const float* partials, int64_t e, int n_splits, int64_t split_stride, const float* bias, Channel&& channel,
                                               const float* residual, int relu) {
    f32x4 v = *reinterpret_cast<const f32x4*>(partials + e);
    for (int s = 1; s < n_splits; ++s) v += *reinterpret_cast<const f32x4*>(partials + (int64_t)s * split_stride + e);
    if (bias) v += *reinterpret_cast<const f32x4*>(bias + channel(e));
    if (residual) v += *reinterpret_cast<const f32x4*>(residual + e);
    if (relu) wino_relu4(v);
    return v;
}

// ==== The split-GEMM tile of k13 / k14 ================================================================================================
//
// One wavefront = 64 pixels x 64 output channels: NCB = 2 blocks of 32 channels (cb) x 2 blocks of 32 pixels (pb), K in k-steps of 16.
// The filter is the ROW operand of v_mfma_f32_32x32x16_f16: lane (i32 = lane & 31, h = lane >> 5) holds K-values 8 h .. 8 h + 7 of
// filter row i32 and of pixel i32 of each block, and its accumulator register r of block (cb, pb) is channel
// 32 cb + (r & 3) + 8 (r >> 2) + 4 h of pixel 32 pb + i32.  Pre-split filter Ws: [cout block 32][k-step][term 2][h 2][i32 32][8 f16] --
// a lane's fragment of a (block, k-step, term) is 16 contiguous bytes -- then the filter's abs-max word (16-byte trailer).
typedef uint32_t sg_u32x4 __attribute__((ext_vector_type(4)));
constexpr int SG_KS_U16 = 2 * 2 * 256;       // u16 values of one (32-channel block, k-step): [term 2][h 2][i32 32][8 f16]
constexpr int SG_TOP = 14;                   // both operands: scaled abs-max in [2^14, 2^15)
// Filter terms travel L2 -> registers through a ring of SG_RING buffers of one k-step each, SG_RING - 1 k-steps ahead.  3 leaves room for
// two wavefronts per SIMD.  Deeper rings were measured on the launches that have at most one wavefront per SIMD anyway (res4 / res5, the
// laterals: 1600 cycles per k-step against the 768 of its MFMAs) and change nothing (ring 4 / 5 / 6: 1.17 / 1.15 / 1.20 ms per image
// against 1.18): what those wavefronts wait for is not the distance of the loads but the L1's time for the activation fragments -- 32
// cache lines per instruction (profiles/r04_experiments.md, K13).
constexpr int SG_RING = 3;
template <int I>
using sg_ic = std::integral_constant<int, I>;

// the activations' scale from the launch's abs-max record, wave-uniform (a scalar register)
__device__ __forceinline__ float sg_activation_scale(const float* in_amax) {
    return __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, wino_pow2_scale(wino_read_amax(in_amax), SG_TOP))));
}
// The accumulators hold (s_w w) (s_x x) sums: what takes the two powers of two off again, exactly, inside the epilogue's multiply-add
// (s_w from the abs-max word behind the filter's n_terms f16 values).
__device__ __forceinline__ float sg_inverse_scale(float sx, const uint16_t* Ws, int64_t n_terms) {
    return wino_pow2_inverse(sx) * wino_pow2_inverse(wino_pow2_scale(*reinterpret_cast<const float*>(Ws + n_terms), SG_TOP));
}

// One k-step of filter terms into a ring buffer wf[cb][term] (ncb channel blocks).  wa: the lane's fragment of channel block 0, k-step 0,
// term 0 (Ws + ... + (h * 32 + i32) * 8); w_cb: u16 values between channel blocks.  (A statement macro, like pod_wino.h's fills: as a
// function taking the buffer by reference the same loads come out of k13's LDS kernels in another order and with four more scalar
// registers -- profiles/split_gemm_shared.md.)
#define SG_LOAD_FILTER(wf, ncb, wa, w_cb, ks)                                                                                         \
    _Pragma("unroll") for (int cb = 0; cb < (ncb); ++cb)                                                                              \
        _Pragma("unroll") for (int t = 0; t < 2; ++t)                                                                                 \
            (wf)[cb][t] = *reinterpret_cast<const sg_u32x4*>((wa) + cb * (w_cb) + (int64_t)(ks) * SG_KS_U16 + t * 512)

// One k-step.  pair(pb, i) -> the lane's K-values 2 i, 2 i + 1 (i = 0 .. 3) of its pixel of block pb, as the kernel has them (registers,
// LDS); they become two f16 term quads per pixel with the very function the filter was split with.  Then the 3 partial products that
// matter, small ones first (as k12): w0 x1, w1 x0, w0 x0.  FIRST: the accumulators start here (they need not be initialised).
template <bool FIRST, int NCB, typename Pair>
__device__ __forceinline__ void sg_kstep(f32x16 (&acc)[NCB][2], const sg_u32x4 (&wf)[NCB][2], float sx, Pair&& pair) {
    sg_u32x4 at[2][2];                // [pb][term]
#pragma unroll
    for (int pb = 0; pb < 2; ++pb)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const f32x2 v = pair(pb, i);
            uint32_t w[2];
            wino_f16_split2(v.x, v.y, sx, w);
            at[pb][0][i] = w[0];
            at[pb][1][i] = w[1];
        }
    const f32x16 zero16 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int prod = 0; prod < 3; ++prod) {
        const int sa = prod == 1 ? 1 : 0;
        const int sb = prod == 0 ? 1 : 0;
#pragma unroll
        for (int cb = 0; cb < NCB; ++cb)
#pragma unroll
            for (int pb = 0; pb < 2; ++pb)
                acc[cb][pb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(wino_f16x8, wf[cb][sa]), __builtin_bit_cast(wino_f16x8, at[pb][sb]),
                                                                     FIRST && prod == 0 ? zero16 : acc[cb][pb], 0, 0, 0);
    }
}

// The epilogue in whole lines: the accumulators (a lane: 4 consecutive channels of ONE pixel per register quad -- 32 pixels x 32 B per
// store instruction) go through 16 KB of LDS, [pixel 64][chunk position 16][16 B] with position = chunk ^ (pixel & 15), and come back as
// 4 pixels x 256 B per instruction: lane (oc = lane & 15, op = lane >> 4) finishes channels 4 oc .. 4 oc + 3 of pixels 4 j + op,
// j = 0 .. 15: v = acc * inv + b4 (+ r[j]), ReLU, store, abs-max of what was stored into `out_amax`.  From the caller: b4 (zero for
// partial sums); r, the 16 residual quads it asked for BEFORE this call (null: none); where(j, pix, dst) -> false: pixel 4 j + op is
// outside the image, or dst = where its quad goes.  One wavefront: no barrier, the LDS is this wavefront's alone.  (b4 by reference, and
// the destination asked for ahead of the arithmetic: the forms that keep k14's register count -- profiles/split_gemm_shared.md.)
template <typename Where>
__device__ __forceinline__ void sg_line_epilogue(float* lds, const f32x16 (&acc)[2][2], int lane, float inv1, const f32x4& b4, const f32x4* r, bool relu, float* out_amax,
                                                 Where&& where) {
    const int i32 = lane & 31, h = lane >> 5, oc = lane & 15, op = lane >> 4;
    const f32x4 inv = f32x4{inv1, inv1, inv1, inv1};
    float lmax = 0.0f;
#pragma unroll
    for (int pb = 0; pb < 2; ++pb)
#pragma unroll
        for (int cb = 0; cb < 2; ++cb)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int pix = 32 * pb + i32, c = 8 * cb + 2 * q + h;
                *reinterpret_cast<f32x4*>(lds + pix * 64 + 4 * (c ^ (i32 & 15))) =
                    f32x4{acc[cb][pb][4 * q], acc[cb][pb][4 * q + 1], acc[cb][pb][4 * q + 2], acc[cb][pb][4 * q + 3]};
            }
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const int pix = 4 * j + op;
        float* dst;
        const bool inside = where(j, pix, dst);
        f32x4 v = __builtin_elementwise_fma(*reinterpret_cast<const f32x4*>(lds + pix * 64 + 4 * (oc ^ (pix & 15))), inv, b4);
        if (r) v += r[j];
        if (relu) wino_relu4(v);
        if (inside) {
            *reinterpret_cast<f32x4*>(dst) = v;
            lmax = wino_absmax4(lmax, v);
        }
    }
    if (out_amax) wino_publish_amax(out_amax, lmax);
}

// ---- filter preparation: fp32 weights -> Ws, two nearest-even f16 terms per scaled value (w s = w0 + w1 to 2^-23), in the order a lane
// loads them; s = the power of two that puts the weight's abs-max (first pass, -> the trailer word) into [2^14, 2^15)
template <typename T>          // (a template so that only the files that prepare a filter carry the kernel)
__global__ void __launch_bounds__(256) k_sg_filter_amax(const T* __restrict__ w, int64_t n, float* __restrict__ amax) {
    float m = 0.0f;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) m = fmaxf(m, fabsf(w[i]));
    wino_publish_amax1(amax, m);
}
// the two terms of GEMM-matrix elements (co, k), (co, k + 1) (k even; nks k-steps per row) to their place in Ws
__device__ __forceinline__ void sg_store_filter_terms(uint16_t* __restrict__ Ws, int nks, int co, int k, float lo, float hi, const float* __restrict__ amax) {
    uint32_t terms[2];
    wino_f16_split2(lo, hi, wino_pow2_scale(*amax, SG_TOP), terms);
    const int cb = co >> 5, i32 = co & 31, ks = k >> 4, h = (k >> 3) & 1, e = k & 7;
#pragma unroll
    for (int term = 0; term < 2; ++term) {
        uint16_t* d = Ws + ((((int64_t)cb * nks + ks) * 2 + term) * 2 + h) * 256 + i32 * 8 + e;
        d[0] = (uint16_t)(terms[term] & 0xFFFFu);
        d[1] = (uint16_t)(terms[term] >> 16);
    }
}
// Host: trailer = 0 -> abs-max of the n weights into it -> launch_split(amax), the kernel's own split launch (it gathers its (lo, hi)
// pairs in its own order and stores them with sg_store_filter_terms).  n_terms: f16 values of Ws ahead of the trailer.
template <typename LaunchSplit>
inline int sg_filter_prepare(const float* weight, int64_t n, void* Ws, int64_t n_terms, hipStream_t stream, LaunchSplit&& launch_split) {
    float* amax = reinterpret_cast<float*>(reinterpret_cast<uint16_t*>(Ws) + n_terms);
    if (hipMemsetAsync(amax, 0, 16, stream) != hipSuccess) return POD_E_LAUNCH;
    const int64_t blocks = (n + 255) / 256;
    hipLaunchKernelGGL(k_sg_filter_amax<float>, dim3((unsigned)(blocks < 256 ? blocks : 256)), dim3(256), 0, stream, weight, n, amax);
    POD_CHECK_LAUNCH();
    launch_split(amax);
    POD_CHECK_LAUNCH();
    return POD_OK;
}

}  // namespace pod
