// The loader's resize on the device (AN:83-84; apply_net.CocoImages): Pillow's 8-bit bilinear Image.resize on an RGB frame, the channel
// flip and the HWC -> CHW transpose, to the byte.
//
//   pod_resize_taps / pod_resize_coeffs : host.  Pillow's precompute_coeffs + normalize_coeffs_8bpc for one axis: per output index the
//                  first source index, the tap count and the 22-bit fixed-point coefficients (fp64, no contraction).
//   k_resize_u8  : one workgroup of 64 x 4 output positions, one thread per position, all three channels.  For each of its vertical taps a
//                  thread forms the horizontal sum of that source row and rounds it to uint8 -- Pillow's intermediate image -- then
//                  accumulates the vertical sum; either pass is skipped when its table is absent.  Tap counts are run-time values
//                  (2 - 3 when enlarging, 2 scale + 1 when reducing).  Three byte stores, one per output plane, coalesced along x.
#include "pod_resize_u8.h"

#include <cmath>
#include <vector>

namespace pod {

struct ResizeArgs {
    ResizeSource from;
    uint8_t* dst;
    int32_t out_h, out_w, flip, tiles_x;
};

// (the arithmetic of a position: pod_resize_u8.h, shared with K31)
__global__ void __launch_bounds__(RESIZE_TX * RESIZE_TY) k_resize_u8(ResizeArgs a) {
    const int x = (blockIdx.x % a.tiles_x) * RESIZE_TX + (threadIdx.x % RESIZE_TX);
    const int y = (blockIdx.x / a.tiles_x) * RESIZE_TY + (threadIdx.x / RESIZE_TX);
    if (x >= a.out_w || y >= a.out_h) return;
    int px[3];
    resize_position_u8(a.from, x, y, px);
    const int64_t plane = (int64_t)a.out_h * a.out_w, at = (int64_t)y * a.out_w + x;
    for (int c = 0; c < 3; ++c) a.dst[c * plane + at] = (uint8_t)px[a.flip ? 2 - c : c];
}

}  // namespace pod

extern "C" int pod_resize_taps(int32_t in_size, int32_t out_size) {
    if (!resize_sizes_ok(in_size, out_size)) return POD_E_INVALID;
    const double scale = (double)in_size / (double)out_size;
    const double support = 1.0 * (scale < 1.0 ? 1.0 : scale);
    return (int)std::ceil(support) * 2 + 1;
}

extern "C" int pod_resize_coeffs(int32_t in_size, int32_t out_size, int32_t* bounds, int32_t* coeffs) {
    if (!resize_sizes_ok(in_size, out_size) || bounds == nullptr || coeffs == nullptr) return POD_E_INVALID;
    const int ksize = pod_resize_taps(in_size, out_size);
    const double scale = (double)in_size / (double)out_size;
    const double fs = scale < 1.0 ? 1.0 : scale;
    const double support = 1.0 * fs, ss = 1.0 / fs;
    std::vector<double> w((size_t)ksize);
    for (int xx = 0; xx < out_size; ++xx) {
        const double center = (xx + 0.5) * scale;
        int xmin = (int)(center - support + 0.5);
        if (xmin < 0) xmin = 0;
        int xmax = (int)(center + support + 0.5);
        if (xmax > in_size) xmax = in_size;
        xmax -= xmin;
        double ww = 0.0;
        for (int x = 0; x < xmax; ++x) {
            double t = (x + xmin - center + 0.5) * ss;
            if (t < 0.0) t = -t;
            w[x] = t < 1.0 ? 1.0 - t : 0.0;
            ww += w[x];
        }
        int32_t* k = coeffs + (int64_t)xx * ksize;
        for (int x = 0; x < ksize; ++x) {
            double c = 0.0;
            if (x < xmax) c = ww != 0.0 ? w[x] / ww : w[x];
            k[x] = c < 0.0 ? (int32_t)(-0.5 + c * (double)(1 << pod::RESIZE_BITS)) : (int32_t)(0.5 + c * (double)(1 << pod::RESIZE_BITS));
        }
        bounds[2 * xx] = xmin;
        bounds[2 * xx + 1] = xmax;
    }
    return POD_OK;
}

extern "C" int pod_resize_frame_u8(const uint8_t* src, int32_t in_h, int32_t in_w, int64_t row_stride, const int32_t* xbounds,
                                   const int32_t* xcoeffs, int32_t xk, const int32_t* ybounds, const int32_t* ycoeffs, int32_t yk, uint8_t* dst,
                                   int32_t out_h, int32_t out_w, int32_t flip_channels, pod_stream_t stream) {
    if (!resize_frame_ok(src, in_h, in_w, row_stride, xbounds, xcoeffs, xk, ybounds, ycoeffs, yk, dst, out_h, out_w)) return POD_E_INVALID;
    pod::ResizeArgs a;
    a.from.src = src; a.dst = dst;
    a.from.xb = xbounds; a.from.xc = xcoeffs; a.from.yb = ybounds; a.from.yc = ycoeffs;
    a.from.row_stride = row_stride;
    a.from.in_h = in_h; a.from.in_w = in_w; a.out_h = out_h; a.out_w = out_w; a.from.xk = xk; a.from.yk = yk;
    a.flip = flip_channels != 0;
    a.tiles_x = (out_w + pod::RESIZE_TX - 1) / pod::RESIZE_TX;
    const int tiles_y = (out_h + pod::RESIZE_TY - 1) / pod::RESIZE_TY;
    hipLaunchKernelGGL(pod::k_resize_u8, dim3((unsigned)(a.tiles_x * tiles_y)), dim3(pod::RESIZE_TX * pod::RESIZE_TY), 0, (hipStream_t)stream, a);
    POD_CHECK_LAUNCH();
    return POD_OK;
}
