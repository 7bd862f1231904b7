// Synthetic image corruptions on the decoded frame (pod_corrupt_*; nothing in the reference: the test loader's frame, between decode
// and AN:83-84's resize).  uint8 (h, w, 3) RGB in, the same geometry out, a pure function of (frame bytes, kind, parameters, key).
// Every kind ends in the quantiser Q(v) = uint8(floor(min(max(v, 0), 1) * 255 + 0.5)).
//
//   k_corrupt_pointwise   : one thread per pixel, its three bytes; 256 pixels of one row per workgroup.
//                           gaussian_noise / speckle_noise: fp32, the normal of channel ch is component ch of Philox call 0 of the pixel
//                           (counter (x, y, 0, STREAM_CORRUPT)).  impulse_noise: call 1, integers only.  brightness / saturate: RGB -> HSV
//                           -> RGB in fp64, every operation rounded on its own.  contrast: fp64 about the channel means k_corrupt_means left.
//   k_corrupt_sums / k_corrupt_means : contrast's channel means.  A workgroup sums CORRUPT_SUM_PIXELS pixels per channel in 32 bits (integer
//                           adds: any order gives the same word); one workgroup then adds the partial sums in 64 bits and divides once.
//   k_corrupt_gauss_rows / k_corrupt_gauss_cols : gaussian_blur, separable, along the rows first (bytes -> fp32 intermediate in scratch, in
//                           byte units), then down the columns.  A thread forms 4 (rows pass) or 8 (columns pass) neighbouring outputs from
//                           one walk over their common inputs: each input is loaded once and meets the taps of all its outputs, a tap that
//                           falls outside -radius..radius counting as 0.  The tap index is the same in every lane: taps come through uniform
//                           addresses, one new tap per input (the outputs' taps are a window that slides).  The border clamps to the edge.
//   k_corrupt_defocus     : the dense stencil, 64 x 16 outputs per workgroup; the tile plus its halo (<= 88 x 40 pixels) sits in LDS as bytes,
//                           reflect-101 borders resolved in the fill; a thread owns 4 neighbouring outputs of a row, three channels each, and
//                           walks the stencil's rows as the rows pass above walks its one.
// Filters accumulate tap * float(byte) in fp32 with fmaf, taps in ascending order, and divide by 255 once before Q.
#include "pod_device.h"

namespace pod {

constexpr uint32_t STREAM_CORRUPT = 0x636f7200u;      // the counter's 4th word ("cor"): DESIGN section 19
constexpr int CORRUPT_SUM_PIXELS = 4096;              // 4096 * 255 < 2^32
constexpr int CORRUPT_GAUSS_MAX_RADIUS = 24, CORRUPT_DEFOCUS_MAX_RADIUS = 12;
constexpr int GAUSS_ROW_PX = 256;                     // rows pass: 64 threads x 4 outputs
constexpr int GAUSS_COL_TY = 8;                       // columns pass: outputs per thread
constexpr int DEFOCUS_TW = 64, DEFOCUS_TH = 16;       // defocus: a workgroup's outputs
constexpr int DEFOCUS_ROW_BYTES = 320;                // >= (64 + 24) * 3; 64 mod 128: the 2 x 16 lanes of a half-wave meet 32 different banks
constexpr int DEFOCUS_ROWS = DEFOCUS_TH + 2 * CORRUPT_DEFOCUS_MAX_RADIUS;

struct CorruptArgs {
    const uint8_t* src;
    uint8_t* dst;
    int64_t src_stride, dst_stride;
    int32_t h, w, kind, radius;
    double p0, p1;
    float f0;
    uint32_t threshold;
    uint64_t key;
    const float* taps;
    const double* mean;
};

__device__ __forceinline__ uint8_t quantise64(double v) {
    v = fmin(fmax(v, 0.0), 1.0);
    return (uint8_t)(int)floor(v * 255.0 + 0.5);
}
__device__ __forceinline__ uint8_t quantise32(float v) {
    v = fminf(fmaxf(v, 0.f), 1.f);
    return (uint8_t)(int)floorf(v * 255.0f + 0.5f);
}

// brightness / saturate: the contract's expressions, fp64, one rounding per operation (the library is built with -ffp-contract=off)
__device__ __forceinline__ void hsv_pixel(const uint8_t in[3], const bool brightness, const double c0, const double c1, uint8_t out[3]) {
    const double r = (double)in[0] / 255.0, g = (double)in[1] / 255.0, b = (double)in[2] / 255.0;
    double V = fmax(r, fmax(g, b));
    const double m = fmin(r, fmin(g, b)), d = V - m;
    double S = V > 0.0 ? d / V : 0.0;
    double h6 = 0.0;
    if (d != 0.0) {
        if (V == r) {
            h6 = (g - b) / d;
            if (h6 < 0.0) h6 = h6 + 6.0;
        } else if (V == g) {
            h6 = 2.0 + (b - r) / d;
        } else {
            h6 = 4.0 + (r - g) / d;
        }
    }
    if (brightness) V = fmin(V + c0, 1.0);
    else S = fmin(fmax(S * c0 + c1, 0.0), 1.0);
    const double fl = floor(h6), f = h6 - fl;
    int i = (int)fl;
    if (i >= 6) i -= 6;
    const double p = V * (1.0 - S), q = V * (1.0 - f * S), t = V * (1.0 - (1.0 - f) * S);
    double R, G, B;
    switch (i) {
        case 0: R = V; G = t; B = p; break;
        case 1: R = q; G = V; B = p; break;
        case 2: R = p; G = V; B = t; break;
        case 3: R = p; G = q; B = V; break;
        case 4: R = t; G = p; B = V; break;
        default: R = V; G = p; B = q; break;
    }
    out[0] = quantise64(R); out[1] = quantise64(G); out[2] = quantise64(B);
}

__global__ void __launch_bounds__(256) k_corrupt_pointwise(CorruptArgs a) {
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= a.w || y >= a.h) return;
    const uint8_t* s = a.src + (int64_t)y * a.src_stride + (int64_t)x * 3;
    uint8_t* o = a.dst + (int64_t)y * a.dst_stride + (int64_t)x * 3;
    const uint8_t in[3] = {s[0], s[1], s[2]};
    uint8_t out[3];
    switch (a.kind) {
        case POD_CORRUPT_GAUSSIAN_NOISE:
        case POD_CORRUPT_SPECKLE_NOISE: {
            const u32x4 r = philox4x32_10(u32x4{(uint32_t)x, (uint32_t)y, 0u, STREAM_CORRUPT}, (uint32_t)a.key, (uint32_t)(a.key >> 32));
            float z[4];
            box_muller16(r.x, z[0], z[1]);
            box_muller16(r.y, z[2], z[3]);
            for (int c = 0; c < 3; ++c) {
                const float xf = (float)in[c] / 255.0f;
                const float v = a.kind == POD_CORRUPT_GAUSSIAN_NOISE ? xf + a.f0 * z[c] : xf + (xf * a.f0) * z[c];
                out[c] = quantise32(v);
            }
            break;
        }
        case POD_CORRUPT_IMPULSE_NOISE: {
            const u32x4 r = philox4x32_10(u32x4{(uint32_t)x, (uint32_t)y, 1u, STREAM_CORRUPT}, (uint32_t)a.key, (uint32_t)(a.key >> 32));
            const uint32_t word[3] = {r.x, r.y, r.z};
            for (int c = 0; c < 3; ++c) out[c] = word[c] < a.threshold ? (((r.w >> c) & 1u) ? 255 : 0) : in[c];
            break;
        }
        case POD_CORRUPT_CONTRAST:
            for (int c = 0; c < 3; ++c) {
                const double mean = a.mean[c];
                out[c] = quantise64(((double)in[c] / 255.0 - mean) * a.p0 + mean);
            }
            break;
        default:      // POD_CORRUPT_BRIGHTNESS, POD_CORRUPT_SATURATE
            hsv_pixel(in, a.kind == POD_CORRUPT_BRIGHTNESS, a.p0, a.p1, out);
            break;
    }
    o[0] = out[0]; o[1] = out[1]; o[2] = out[2];
}

// partial[3 * workgroup + c]: the sum of channel c over the workgroup's CORRUPT_SUM_PIXELS pixels (row-major pixel order)
__global__ void __launch_bounds__(256) k_corrupt_sums(CorruptArgs a, uint32_t* partial) {
    __shared__ uint32_t total[3];
    if (threadIdx.x < 3) total[threadIdx.x] = 0u;
    __syncthreads();
    const int64_t n = (int64_t)a.h * a.w, first = (int64_t)blockIdx.x * CORRUPT_SUM_PIXELS;
    uint32_t sum[3] = {0u, 0u, 0u};
    for (int i = 0; i < CORRUPT_SUM_PIXELS / 256; ++i) {
        const int64_t p = first + i * 256 + threadIdx.x;
        if (p < n) {
            const int64_t y = p / a.w, x = p - y * a.w;
            const uint8_t* s = a.src + y * a.src_stride + x * 3;
            sum[0] += s[0]; sum[1] += s[1]; sum[2] += s[2];
        }
    }
    for (int c = 0; c < 3; ++c) {
        for (int off = 32; off > 0; off >>= 1) sum[c] += __shfl_xor(sum[c], off, 64);
        if ((threadIdx.x & 63) == 0) atomicAdd(&total[c], sum[c]);      // integers in LDS: the order cannot change the word
    }
    __syncthreads();
    if (threadIdx.x < 3) partial[3 * (int64_t)blockIdx.x + threadIdx.x] = total[threadIdx.x];
}

// mean[c] = (sum of channel c) / (255.0 h w): 64-bit integer sum of the partial sums, one division
__global__ void __launch_bounds__(256) k_corrupt_means(const uint32_t* partial, int32_t n_partial, int32_t h, int32_t w, double* mean) {
    __shared__ unsigned long long part[3][256];
    unsigned long long sum[3] = {0ull, 0ull, 0ull};
    for (int i = threadIdx.x; i < n_partial; i += 256)
        for (int c = 0; c < 3; ++c) sum[c] += partial[3 * (int64_t)i + c];
    for (int c = 0; c < 3; ++c) part[c][threadIdx.x] = sum[c];
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off)
            for (int c = 0; c < 3; ++c) part[c][threadIdx.x] += part[c][threadIdx.x + off];
        __syncthreads();
    }
    if (threadIdx.x < 3) mean[threadIdx.x] = (double)part[threadIdx.x][0] / (255.0 * (double)((int64_t)h * w));
}

// tap k of n + 1 (k the same in every lane); 0 outside
__device__ __forceinline__ float tap_or_zero(const float* __restrict__ taps, const int k, const int n) {
    return (k >= 0 && k <= n) ? taps[k] : 0.f;
}
// Output o of a thread's N neighbouring outputs meets input j with tap j - o: t[o] holds it, and one new tap enters per input.
template <int N>
__device__ __forceinline__ void slide_taps(float (&t)[N], const float next) {
#pragma unroll
    for (int o = N - 1; o > 0; --o) t[o] = t[o - 1];
    t[0] = next;
}

__global__ void __launch_bounds__(64) k_corrupt_gauss_rows(CorruptArgs a, float* __restrict__ mid) {
    __shared__ uint8_t row[(GAUSS_ROW_PX + 2 * CORRUPT_GAUSS_MAX_RADIUS) * 3];
    const int R = a.radius, y = blockIdx.y, x0 = blockIdx.x * GAUSS_ROW_PX;
    const uint8_t* s = a.src + (int64_t)y * a.src_stride;
    for (int i = threadIdx.x; i < (GAUSS_ROW_PX + 2 * R) * 3; i += 64) {
        const int px = i / 3, c = i - 3 * px;
        const int xx = min(max(x0 - R + px, 0), a.w - 1);
        row[i] = s[(int64_t)xx * 3 + c];
    }
    __syncthreads();
    const int lx = threadIdx.x * 4;
    float acc[4][3] = {}, t[4] = {};      // t[o]: tap j - o, the window sliding by one tap per input
    for (int j = 0; j < 4 + 2 * R; ++j) {
        const float p0 = (float)row[(lx + j) * 3], p1 = (float)row[(lx + j) * 3 + 1], p2 = (float)row[(lx + j) * 3 + 2];
        slide_taps<4>(t, tap_or_zero(a.taps, j, 2 * R));
#pragma unroll
        for (int o = 0; o < 4; ++o) {
            acc[o][0] = fmaf(t[o], p0, acc[o][0]); acc[o][1] = fmaf(t[o], p1, acc[o][1]); acc[o][2] = fmaf(t[o], p2, acc[o][2]);
        }
    }
#pragma unroll
    for (int o = 0; o < 4; ++o) {
        const int x = x0 + lx + o;
        if (x < a.w) {
            float* m = mid + ((int64_t)y * a.w + x) * 3;
            m[0] = acc[o][0]; m[1] = acc[o][1]; m[2] = acc[o][2];
        }
    }
}

__global__ void __launch_bounds__(256) k_corrupt_gauss_cols(CorruptArgs a, const float* __restrict__ mid) {
    const int R = a.radius, x = blockIdx.x * 64 + (threadIdx.x & 63), y0 = (blockIdx.y * 4 + (threadIdx.x >> 6)) * GAUSS_COL_TY;
    if (x >= a.w || y0 >= a.h) return;
    float acc[GAUSS_COL_TY][3] = {}, t[GAUSS_COL_TY] = {};
    for (int j = 0; j < GAUSS_COL_TY + 2 * R; ++j) {
        const int yy = min(max(y0 - R + j, 0), a.h - 1);
        const float* m = mid + ((int64_t)yy * a.w + x) * 3;
        const float p0 = m[0], p1 = m[1], p2 = m[2];
        slide_taps<GAUSS_COL_TY>(t, tap_or_zero(a.taps, j, 2 * R));
#pragma unroll
        for (int o = 0; o < GAUSS_COL_TY; ++o) {
            acc[o][0] = fmaf(t[o], p0, acc[o][0]); acc[o][1] = fmaf(t[o], p1, acc[o][1]); acc[o][2] = fmaf(t[o], p2, acc[o][2]);
        }
    }
#pragma unroll
    for (int o = 0; o < GAUSS_COL_TY; ++o) {
        const int y = y0 + o;
        if (y < a.h) {
            uint8_t* d = a.dst + (int64_t)y * a.dst_stride + (int64_t)x * 3;
            d[0] = quantise32(acc[o][0] / 255.0f); d[1] = quantise32(acc[o][1] / 255.0f); d[2] = quantise32(acc[o][2] / 255.0f);
        }
    }
}

// reflect-101 (d c b | a b c d | c b a), repeated until the index is inside
__device__ __forceinline__ int mirror101(int i, const int n) {
    if (n == 1) return 0;
    const int p = 2 * (n - 1);
    i %= p;
    if (i < 0) i += p;
    return i < n ? i : p - i;
}

__global__ void __launch_bounds__(256) k_corrupt_defocus(CorruptArgs a) {
    __shared__ __attribute__((aligned(16))) uint8_t tile[DEFOCUS_ROWS * DEFOCUS_ROW_BYTES];
    const int r = a.radius, n = 2 * r + 1;
    const int X0 = blockIdx.x * DEFOCUS_TW, Y0 = blockIdx.y * DEFOCUS_TH;
    const int tw = (DEFOCUS_TW + 2 * r) * 3, th = DEFOCUS_TH + 2 * r;
    for (int i = threadIdx.x; i < th * tw; i += 256) {
        const int trow = i / tw, b = i - trow * tw, px = b / 3, c = b - 3 * px;
        const int sx = mirror101(X0 - r + px, a.w), sy = mirror101(Y0 - r + trow, a.h);
        tile[trow * DEFOCUS_ROW_BYTES + b] = a.src[(int64_t)sy * a.src_stride + (int64_t)sx * 3 + c];
    }
    __syncthreads();
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    float acc[4][3] = {};
    for (int sy = 0; sy < n; ++sy) {
        const uint8_t* trow = tile + (ty + sy) * DEFOCUS_ROW_BYTES + tx * 12;
        const float* taps = a.taps + sy * n;
        float t[4] = {};
        for (int j = 0; j < 4 + 2 * r; ++j) {
            const float p0 = (float)trow[3 * j], p1 = (float)trow[3 * j + 1], p2 = (float)trow[3 * j + 2];
            slide_taps<4>(t, tap_or_zero(taps, j, 2 * r));
#pragma unroll
            for (int o = 0; o < 4; ++o) {
                acc[o][0] = fmaf(t[o], p0, acc[o][0]); acc[o][1] = fmaf(t[o], p1, acc[o][1]); acc[o][2] = fmaf(t[o], p2, acc[o][2]);
            }
        }
    }
    const int y = Y0 + ty;
    if (y >= a.h) return;
#pragma unroll
    for (int o = 0; o < 4; ++o) {
        const int x = X0 + tx * 4 + o;
        if (x < a.w) {
            uint8_t* d = a.dst + (int64_t)y * a.dst_stride + (int64_t)x * 3;
            d[0] = quantise32(acc[o][0] / 255.0f); d[1] = quantise32(acc[o][1] / 255.0f); d[2] = quantise32(acc[o][2] / 255.0f);
        }
    }
}

static inline int64_t corrupt_sum_groups(int32_t h, int32_t w) {
    return ((int64_t)h * w + CORRUPT_SUM_PIXELS - 1) / CORRUPT_SUM_PIXELS;
}
static inline bool corrupt_sides_ok(int32_t h, int32_t w) {
    return h >= 1 && w >= 1 && h <= POD_RESIZE_MAX_SIDE && w <= POD_RESIZE_MAX_SIDE;
}

}  // namespace pod

extern "C" size_t pod_corrupt_scratch_bytes(int32_t kind, int32_t h, int32_t w) {
    if (!pod::corrupt_sides_ok(h, w)) return 0;
    if (kind == POD_CORRUPT_CONTRAST) return 32 + 12 * (size_t)pod::corrupt_sum_groups(h, w);       // three means, then the partial sums
    if (kind == POD_CORRUPT_GAUSSIAN_BLUR) return (size_t)h * (size_t)w * 3 * sizeof(float);
    return 0;
}

extern "C" int pod_corrupt_frame_u8(const uint8_t* src, int32_t h, int32_t w, int64_t src_row_stride, uint8_t* dst, int64_t dst_row_stride,
                                    const PodCorruption* corruption, void* scratch, size_t scratch_bytes, pod_stream_t stream) {
    if (src == nullptr || dst == nullptr || corruption == nullptr || !pod::corrupt_sides_ok(h, w)) return POD_E_INVALID;
    if (src_row_stride < 3 * (int64_t)w || dst_row_stride < 3 * (int64_t)w) return POD_E_INVALID;
    const PodCorruption& k = *corruption;
    if (k.kind < 0 || k.kind >= POD_CORRUPT_KINDS) return POD_E_INVALID;
    if (k.kind == POD_CORRUPT_GAUSSIAN_BLUR && (k.radius < 0 || k.radius > pod::CORRUPT_GAUSS_MAX_RADIUS || k.taps == nullptr)) return POD_E_INVALID;
    if (k.kind == POD_CORRUPT_DEFOCUS_BLUR && (k.radius < 0 || k.radius > pod::CORRUPT_DEFOCUS_MAX_RADIUS || k.taps == nullptr)) return POD_E_INVALID;
    const size_t need = pod_corrupt_scratch_bytes(k.kind, h, w);
    if (need > 0 && (scratch == nullptr || scratch_bytes < need || !pod_aligned(8, scratch))) return POD_E_INVALID;
    const uintptr_t s0 = (uintptr_t)src, s1 = s0 + (uintptr_t)((int64_t)(h - 1) * src_row_stride + 3 * (int64_t)w);
    const uintptr_t d0 = (uintptr_t)dst, d1 = d0 + (uintptr_t)((int64_t)(h - 1) * dst_row_stride + 3 * (int64_t)w);
    if (s0 < d1 && d0 < s1) return POD_E_INVALID;
    if (need > 0) {
        const uintptr_t w0 = (uintptr_t)scratch, w1 = w0 + need;
        if ((w0 < d1 && d0 < w1) || (w0 < s1 && s0 < w1)) return POD_E_INVALID;
    }
    pod::CorruptArgs a;
    a.src = src; a.dst = dst; a.src_stride = src_row_stride; a.dst_stride = dst_row_stride;
    a.h = h; a.w = w; a.kind = k.kind; a.radius = k.radius;
    a.p0 = k.p0; a.p1 = k.p1; a.f0 = (float)k.p0;
    a.threshold = k.impulse_threshold; a.key = k.key; a.taps = k.taps; a.mean = nullptr;
    hipStream_t st = (hipStream_t)stream;
    if (k.kind == POD_CORRUPT_GAUSSIAN_BLUR) {
        float* mid = (float*)scratch;
        hipLaunchKernelGGL(pod::k_corrupt_gauss_rows, dim3((unsigned)((w + pod::GAUSS_ROW_PX - 1) / pod::GAUSS_ROW_PX), (unsigned)h), dim3(64), 0, st, a, mid);
        POD_CHECK_LAUNCH();
        hipLaunchKernelGGL(pod::k_corrupt_gauss_cols, dim3((unsigned)((w + 63) / 64), (unsigned)((h + 4 * pod::GAUSS_COL_TY - 1) / (4 * pod::GAUSS_COL_TY))),
                           dim3(256), 0, st, a, (const float*)mid);
        POD_CHECK_LAUNCH();
        return POD_OK;
    }
    if (k.kind == POD_CORRUPT_DEFOCUS_BLUR) {
        hipLaunchKernelGGL(pod::k_corrupt_defocus, dim3((unsigned)((w + pod::DEFOCUS_TW - 1) / pod::DEFOCUS_TW), (unsigned)((h + pod::DEFOCUS_TH - 1) / pod::DEFOCUS_TH)),
                           dim3(256), 0, st, a);
        POD_CHECK_LAUNCH();
        return POD_OK;
    }
    if (k.kind == POD_CORRUPT_CONTRAST) {
        double* mean = (double*)scratch;
        uint32_t* partial = (uint32_t*)((char*)scratch + 32);
        const int64_t groups = pod::corrupt_sum_groups(h, w);
        hipLaunchKernelGGL(pod::k_corrupt_sums, dim3((unsigned)groups), dim3(256), 0, st, a, partial);
        POD_CHECK_LAUNCH();
        hipLaunchKernelGGL(pod::k_corrupt_means, dim3(1), dim3(256), 0, st, (const uint32_t*)partial, (int32_t)groups, h, w, mean);
        POD_CHECK_LAUNCH();
        a.mean = mean;
    }
    hipLaunchKernelGGL(pod::k_corrupt_pointwise, dim3((unsigned)((w + 255) / 256), (unsigned)h), dim3(256), 0, st, a);
    POD_CHECK_LAUNCH();
    return POD_OK;
}
