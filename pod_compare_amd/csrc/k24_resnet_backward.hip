// K24: what the ResNet bottlenecks' backward pass needs beyond K13, K22 and K23 (include/pod_mi355x.h).
//
// pod_conv1x1_wgrad_strided: the weight gradient of a 1x1 convolution of stride 1 or 2 at the backbone's widths (conv3 and the shortcuts
// have 1024 and 2048 output channels; the first block of a stage has conv1 and its shortcut at stride 2, STRIDE_IN_1X1):
//     dW[k][c] = sum over (b, oy, ox) of dY[(b, oy, ox)][k] X[b H_in W_in + stride oy W_in + stride ox][c].
// K23's kernel and launcher (pod_wgrad.h: k_conv1x1_wgrad and c1w_launch, the same arithmetic, argument checks, slices -- of the OUTPUT
// pixels -- and fixed-order fp64 second launch); at stride 2 the staging loads take row pin(p) of X for output pixel p, so the subsampled map
// is never materialised, and at stride 1 the instantiation is K23's own.  The k tiles ride on the grid's y, so K <= 2048 costs nothing.
//
// pod_subsample2_scatter_cl: the input gradient of that pixel selection for one image -- the half-resolution gradient lands on the
// pixels with even coordinates, the others get zero -- fused with what the full map needs anyway: the gradient it already carries
// (`add`, the FPN's lateral) and the ReLU gate of the block whose output the map is, which everything arriving there passes:
//     dx[(y, x)][c] = gate[(y, x)][c] > 0 ? (y, x even ? d_small[(y / 2) Wo + x / 2][c] : 0) + add[(y, x)][c] : 0.
// One thread per 16 bytes of the result, the result's abs-max record published by the same pass (pod_wgrad.h: map_quad_pass, gate4).
#include "pod_wgrad.h"

namespace pod {

constexpr int C1WS_MAX_K = 2048;

__global__ void __launch_bounds__(256) k_subsample2_scatter_cl(const float* __restrict__ d_small, const float* __restrict__ gate, const float* add, float* dx,
                                                               const int H, const int W, const int Wo, const int C4, float* __restrict__ amax) {
    map_quad_pass(dx, H, W, C4, amax, [&](const int64_t i, const int c4, const int x, const int y) {
        f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
        if (!((x | y) & 1)) v = *reinterpret_cast<const f32x4*>(d_small + (((int64_t)(y >> 1) * Wo + (x >> 1)) * C4 + c4) * 4);
        if (add) v += *reinterpret_cast<const f32x4*>(add + i * 4);
        if (gate) v = gate4(v, *reinterpret_cast<const f32x4*>(gate + i * 4));
        return v;
    });
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
    return pixels < 1 ? 0 : pod::c1w_layout(pixels, C, K).floats;
}

extern "C" int pod_conv1x1_wgrad_strided(const float* x, const float* dy, int32_t images, int32_t H_in, int32_t W_in, int32_t stride, int32_t C, int32_t K,
                                         const float* x_amax, const float* dy_amax, float* dW, float* db, float* partials, pod_stream_t stream) {
    const int64_t pixels = pod::c1ws_pixels(images, H_in, W_in, stride, C, K);
    if (pixels < 1) return POD_E_INVALID;
    if (stride == 1) return pod::c1w_launch<false>(x, dy, pixels, C, K, pod::C1wGather{}, x_amax, dy_amax, dW, db, partials, (hipStream_t)stream);
    const int32_t Ho = (H_in - 1) / stride + 1, Wo = (W_in - 1) / stride + 1;
    return pod::c1w_launch<true>(x, dy, pixels, C, K, pod::C1wGather{Wo, Ho * Wo, W_in, H_in * W_in, stride}, x_amax, dy_amax, dW, db, partials, (hipStream_t)stream);
}

extern "C" int pod_subsample2_scatter_cl(const float* d_small, const float* gate, const float* add, float* dx, int32_t H, int32_t W, int32_t C, float* dx_amax,
                                         pod_stream_t stream) {
    const int32_t Wo = (int32_t)(((int64_t)W - 1) / 2 + 1);      // (W is checked below)
    return pod::map_gather(d_small, gate, add, dx, H, W, C, dx_amax, (int64_t)H * W, [&](dim3 grid) {
        hipLaunchKernelGGL(pod::k_subsample2_scatter_cl, grid, dim3(256), 0, (hipStream_t)stream, d_small, gate, add, dx, H, W, Wo, C / 4, dx_amax);
    });
}
