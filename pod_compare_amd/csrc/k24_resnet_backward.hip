// K24: what the ResNet bottlenecks' backward pass needs beyond K13, K22 and K23 (include/pod_mi355x.h).
//
// pod_conv1x1_wgrad_strided: the weight gradient of a 1x1 convolution of stride 1 or 2 at the backbone's widths (conv3 and the shortcuts
// have 1024 and 2048 output channels; the first block of a stage has conv1 and its shortcut at stride 2, STRIDE_IN_1X1):
//     dW[k][c] = sum over (b, oy, ox) of dY[(b, oy, ox)][k] X[b H_in W_in + stride oy W_in + stride ox][c].
// K23's kernel (pod_wgrad.h: k_conv1x1_wgrad, the same arithmetic, slices -- of the OUTPUT pixels -- and fixed-order fp64 second launch);
// at stride 2 the staging loads take row pin(p) of X for output pixel p, so the subsampled map is never materialised, and at stride 1
// the instantiation is K23's own.  The k tiles ride on the grid's y, so K <= 2048 costs the kernel nothing.
//
// pod_subsample2_scatter_cl: the input gradient of that pixel selection for one image -- the half-resolution gradient lands on the
// pixels with even coordinates, the others get zero -- fused with what the full map needs anyway: the gradient it already carries
// (`add`, the FPN's lateral) and the ReLU gate of the block whose output the map is, which everything arriving there passes:
//     dx[(y, x)][c] = gate[(y, x)][c] > 0 ? (y, x even ? d_small[(y / 2) Wo + x / 2][c] : 0) + add[(y, x)][c] : 0.
// One thread per 16 bytes of the result, the result's abs-max record published by the same pass.
#include "pod_wgrad.h"

namespace pod {

constexpr int C1WS_MAX_K = 2048;

__global__ void __launch_bounds__(256) k_subsample2_scatter_cl(const float* __restrict__ d_small, const float* __restrict__ gate, const float* add, float* dx,
                                                               const int H, const int W, const int Wo, const int C4, float* __restrict__ amax) {
    const int64_t n = (int64_t)H * W * C4, stride = (int64_t)gridDim.x * blockDim.x;
    float m = 0.0f;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const int c4 = (int)(i % C4);
        const int64_t pix = i / C4;
        const int x = (int)(pix % W), y = (int)(pix / W);
        f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
        if (!((x | y) & 1)) v = *reinterpret_cast<const f32x4*>(d_small + (((int64_t)(y >> 1) * Wo + (x >> 1)) * C4 + c4) * 4);
        if (add) v += *reinterpret_cast<const f32x4*>(add + i * 4);
        if (gate) {
            const f32x4 g = *reinterpret_cast<const f32x4*>(gate + i * 4);
            v.x = g.x > 0.f ? v.x : 0.f;
            v.y = g.y > 0.f ? v.y : 0.f;
            v.z = g.z > 0.f ? v.z : 0.f;
            v.w = g.w > 0.f ? v.w : 0.f;
        }
        *reinterpret_cast<f32x4*>(dx + i * 4) = v;
        m = wino_absmax4(m, v);
    }
    if (amax) wino_publish_amax_block(amax, m);      // (uniform: every thread of the workgroup calls it)
}

// Host: the output pixel count, 0 = outside what the kernel addresses (30-bit pixel counts on both sides of the stride).
static int64_t c1ws_pixels(int32_t images, int32_t H_in, int32_t W_in, int32_t stride, int32_t C, int32_t K) {
    if (images < 1 || H_in < 1 || W_in < 1 || H_in > 16384 || W_in > 16384 || (stride != 1 && stride != 2)) return 0;
    if (C < 16 || (C & 15) != 0 || C > C1W_MAX_C || K < 64 || (K & 63) != 0 || K > C1WS_MAX_K) return 0;
    if ((int64_t)images * H_in * W_in > 0x3FFFFFFF) return 0;
    const int64_t Ho = (H_in - 1) / stride + 1, Wo = (W_in - 1) / stride + 1;
    return (int64_t)images * Ho * Wo;
}

}  // namespace pod

extern "C" int64_t pod_conv1x1_wgrad_strided_partials(int32_t images, int32_t H_in, int32_t W_in, int32_t stride, int32_t C, int32_t K) {
    const int64_t pixels = pod::c1ws_pixels(images, H_in, W_in, stride, C, K);
    if (pixels < 1) return 0;
    const int sp = pod::c1w_slice_pixels(pixels, C, K);
    const int64_t n_slices = (pixels + sp - 1) / sp, n_chunks = (pixels + pod::WG_DB_CHUNK - 1) / pod::WG_DB_CHUNK;
    return 2 * n_chunks * K + n_slices * K * C;
}

extern "C" int pod_conv1x1_wgrad_strided(const float* x, const float* dy, int32_t images, int32_t H_in, int32_t W_in, int32_t stride, int32_t C, int32_t K,
                                         const float* x_amax, const float* dy_amax, float* dW, float* db, float* partials, pod_stream_t stream) {
    if (!x || !dy || !x_amax || !dy_amax || !dW || !partials) return POD_E_INVALID;
    const int64_t pixels = pod::c1ws_pixels(images, H_in, W_in, stride, C, K);
    if (pixels < 1) return POD_E_INVALID;
    if (!pod_aligned(16, x, dy, partials) || !pod_aligned(4, x_amax, dy_amax, dW, db)) return POD_E_INVALID;
    if (dW == x || dW == dy || dW == partials || x == partials || dy == partials || (db && (db == dW || db == partials))) return POD_E_INVALID;
    const int sp = pod::c1w_slice_pixels(pixels, C, K);
    const int64_t n_slices = (pixels + sp - 1) / sp, n_chunks = (pixels + pod::WG_DB_CHUNK - 1) / pod::WG_DB_CHUNK;
    double* dbp = reinterpret_cast<double*>(partials);
    float* wp = partials + 2 * n_chunks * K;
    hipStream_t s = (hipStream_t)stream;
    if (db) {
        hipLaunchKernelGGL(pod::k_wgrad_db<pod::WG_DB_CHUNK>, dim3((unsigned)n_chunks, (unsigned)(K / 64)), dim3(256), 0, s, dy, pixels, K, dbp);
        POD_CHECK_LAUNCH();
    }
    const dim3 grid((unsigned)n_slices, (unsigned)(K / pod::C1W_KT), (unsigned)((C + pod::C1W_CT - 1) / pod::C1W_CT));
    if (stride == 1) {
        hipLaunchKernelGGL(pod::k_conv1x1_wgrad<false>, grid, dim3(256), 0, s, x, dy, pixels, C, K, sp, x_amax, dy_amax, wp, pod::C1wGather{});
    } else {
        const int32_t Ho = (H_in - 1) / stride + 1, Wo = (W_in - 1) / stride + 1;
        hipLaunchKernelGGL(pod::k_conv1x1_wgrad<true>, grid, dim3(256), 0, s, x, dy, pixels, C, K, sp, x_amax, dy_amax, wp,
                           pod::C1wGather{Wo, Ho * Wo, W_in, H_in * W_in, stride});
    }
    POD_CHECK_LAUNCH();
    const int64_t n_out = (int64_t)K * C + (db ? K : 0);
    hipLaunchKernelGGL(pod::k_wgrad_reduce<1>, dim3((unsigned)((n_out + 255) / 256)), dim3(256), 0, s, wp, (int)n_slices, dbp, (int)n_chunks, C, K, K, dW, db);
    POD_CHECK_LAUNCH();
    return POD_OK;
}

extern "C" int pod_subsample2_scatter_cl(const float* d_small, const float* gate, const float* add, float* dx, int32_t H, int32_t W, int32_t C, float* dx_amax,
                                         pod_stream_t stream) {
    if (!d_small || !dx || d_small == dx || gate == dx || H < 1 || W < 1 || H > 16384 || W > 16384 || C < 4 || (C & 3) != 0) return POD_E_INVALID;
    if (!pod_aligned(16, d_small, gate, add, dx) || !pod_aligned(4, dx_amax)) return POD_E_INVALID;
    const int32_t Wo = (W - 1) / 2 + 1;
    const int64_t n4 = (int64_t)H * W * (C / 4);
    hipLaunchKernelGGL(pod::k_subsample2_scatter_cl, dim3(pod_grid_stride_blocks(n4, 4096)), dim3(256), 0, (hipStream_t)stream, d_small, gate, add, dx, H, W, Wo, C / 4,
                       dx_amax);
    POD_CHECK_LAUNCH();
    return POD_OK;
}
