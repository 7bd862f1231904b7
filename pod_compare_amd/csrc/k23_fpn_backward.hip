// K23: what the FPN's backward pass needs beyond K22 and the forward GEMM (include/pod_mi355x.h).
//
// pod_conv1x1_wgrad: dW[k][c] = sum over pixels of dY[p][k] X[p][c], db[k] = sum dY[.][k] -- the weight gradient of a 1x1 convolution
// (the laterals) and, on the patch matrix of pod_im2col3x3s2_cl, of the stride-2 convolutions p6 / p7.  K22's arithmetic without its taps:
// a GEMM with M = K, N = C and the PIXELS as the reduction on v_mfma_f32_32x32x16_f16, both operands split at run time into two f16
// terms of their power-of-two-scaled values (scales from their abs-max records), three partial products, small ones first, fp32 accumulate.
//
// A workgroup of four wavefronts owns 64 k x 128 c: wave (kb, cw) keeps two 32 x 32 accumulator blocks, k block kb against the two c
// blocks of c half cw, so a split dY fragment meets two X fragments (K22 has nine blocks per fragment pair, one per tap; here the width
// of the c tile is what a staged dY fragment is spread over).  The reduction unit is a STEP of 32 consecutive pixels: the step's rows come
// from memory as they lie there -- whole 256-byte (dY) and 512-byte (X) runs, 16 bytes a lane -- into LDS [pixel 32][channel + pad], and
// the MFMA's operand, 8 consecutive pixels of one channel per lane, is read back down the columns (8 ds_read_b32: the 32 lanes of a
// half-wave read 32 consecutive channels of one pixel, conflict-free whatever the row stride).  The next step's rows are asked for ahead of
// the current step's products.  A pixel tail and a channel-tile edge are zero-filled in the staging, never read.
//
// (The kernel, k_conv1x1_wgrad, and its launcher, c1w_launch, are in pod_wgrad.h: K24 runs them too, on the rows a stride selects.)
//
// Parallelism and determinism: the pixels are cut into SLICES of c1w_slice_pixels(pixels, C, K) consecutive pixels -- the geometry alone:
// 1024, halved down to 128 while the launch has fewer than 512 workgroups; grid = slices x k tiles x c tiles.  A slice writes its
// partial sums [slice][k][c], and pod_wgrad.h's second launch adds them in slice order, in fp64 (db: fp64 column sums over chunks of
// 4096 pixels).  No atomics: two launches give the same bits.
//
// pod_col2im3x3s2_cl, pod_upsample2_sum_cl: the two gathers of the backward pass -- the input gradient of pod_im2col3x3s2_cl (with the
// ReLU gate of p7's input and the gradient p6 already has), and the backward of the nearest top-down sum at factor two.  One thread per
// 16 bytes of the result, a fixed order of at most four terms, the result's abs-max record published by the same pass: the loop, the
// gate and the entries' shared check are pod_wgrad.h's (map_quad_pass, gate4, map_gather).
#include "pod_wgrad.h"

namespace pod {

// dx[(y, x)][c] = gate(sum of the entries of dcols that read pixel (y, x)) + add: tap (ty, tx) of output pixel (oy, ox) read input pixel
// (2 oy + ty - 1, 2 ox + tx - 1), so pixel (y, x) is met by oy = (y + 1 - ty) / 2 where that is integral and in range -- ty, tx ascending.
__global__ void __launch_bounds__(256) k_col2im3x3s2_cl(const float* __restrict__ dcols, const float* __restrict__ gate, const float* add, float* dx, const int H,
                                                        const int W, const int Ho, const int Wo, const int C4, float* __restrict__ amax) {
    map_quad_pass(dx, H, W, C4, amax, [&](const int64_t i, const int c4, const int x, const int y) {
        f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ty = 0; ty < 3; ++ty) {
            const int ny = y + 1 - ty, oy = ny >> 1;
            if (ny < 0 || (ny & 1) || oy >= Ho) continue;
#pragma unroll
            for (int tx = 0; tx < 3; ++tx) {
                const int nx = x + 1 - tx, ox = nx >> 1;
                if (nx < 0 || (nx & 1) || ox >= Wo) continue;
                v += *reinterpret_cast<const f32x4*>(dcols + ((((int64_t)oy * Wo + ox) * 9 + ty * 3 + tx) * C4 + c4) * 4);
            }
        }
        if (gate) v = gate4(v, *reinterpret_cast<const f32x4*>(gate + i * 4));
        if (add) v += *reinterpret_cast<const f32x4*>(add + i * 4);
        return v;
    });
}

// d_top[(Y, X)] = add[(Y, X)] + the children (2 Y + dy, 2 X + dx) of d_child that exist, dy then dx ascending
__global__ void __launch_bounds__(256) k_upsample2_sum_cl(const float* __restrict__ d_child, const int h, const int w, const float* add, float* d_top, const int Ht,
                                                          const int Wt, const int C4, float* __restrict__ amax) {
    map_quad_pass(d_top, Ht, Wt, C4, amax, [&](const int64_t i, const int c4, const int X, const int Y) {
        f32x4 v = *reinterpret_cast<const f32x4*>(add + i * 4);
#pragma unroll
        for (int dy = 0; dy < 2; ++dy)
#pragma unroll
            for (int dx = 0; dx < 2; ++dx) {
                const int y = 2 * Y + dy, x = 2 * X + dx;
                if (y < h && x < w) v += *reinterpret_cast<const f32x4*>(d_child + (((int64_t)y * w + x) * C4 + c4) * 4);
            }
        return v;
    });
}

// Host: false = outside what the kernel addresses.
static bool c1w_geometry(int64_t pixels, int32_t C, int32_t K) {
    return pixels >= 1 && pixels <= 0x3FFFFFFF && C >= 16 && (C & 15) == 0 && C <= C1W_MAX_C && K >= 64 && (K & 63) == 0 && K <= 512;
}

}  // namespace pod

extern "C" int64_t pod_conv1x1_wgrad_partials(int64_t pixels, int32_t C, int32_t K) {
    return pod::c1w_geometry(pixels, C, K) ? pod::c1w_layout(pixels, C, K).floats : 0;
}

extern "C" int pod_conv1x1_wgrad(const float* x, const float* dy, int64_t pixels, int32_t C, int32_t K, const float* x_amax, const float* dy_amax, float* dW,
                                 float* db, float* partials, pod_stream_t stream) {
    if (!pod::c1w_geometry(pixels, C, K)) return POD_E_INVALID;
    return pod::c1w_launch<false>(x, dy, pixels, C, K, pod::C1wGather{}, x_amax, dy_amax, dW, db, partials, (hipStream_t)stream);
}

extern "C" int pod_col2im3x3s2_cl(const float* dcols, const float* gate, const float* add, float* dx, int32_t H, int32_t W, int32_t C, float* dx_amax,
                                  pod_stream_t stream) {
    const int32_t Ho = (int32_t)(((int64_t)H - 1) / 2 + 1), Wo = (int32_t)(((int64_t)W - 1) / 2 + 1);      // (H, W are checked below)
    return pod::map_gather(dcols, gate, add, dx, H, W, C, dx_amax, (int64_t)H * W, [&](dim3 grid) {
        hipLaunchKernelGGL(pod::k_col2im3x3s2_cl, grid, dim3(256), 0, (hipStream_t)stream, dcols, gate, add, dx, H, W, Ho, Wo, C / 4, dx_amax);
    });
}

extern "C" int pod_upsample2_sum_cl(const float* d_child, int32_t h, int32_t w, const float* add, float* d_top, int32_t C, float* d_top_amax, pod_stream_t stream) {
    const int32_t Ht = (int32_t)(((int64_t)h + 1) / 2), Wt = (int32_t)(((int64_t)w + 1) / 2);      // (h, w are checked below)
    if (!add) return POD_E_INVALID;
    return pod::map_gather(d_child, nullptr, add, d_top, h, w, C, d_top_amax, (int64_t)Ht * Wt, [&](dim3 grid) {
        hipLaunchKernelGGL(pod::k_upsample2_sum_cl, grid, dim3(256), 0, (hipStream_t)stream, d_child, h, w, add, d_top, Ht, Wt, C / 4, d_top_amax);
    });
}
