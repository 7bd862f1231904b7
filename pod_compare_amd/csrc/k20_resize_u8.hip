// The loader's resize on the device (AN:83-84; apply_net.CocoImages): Pillow's 8-bit bilinear Image.resize on an RGB frame, the channel
// flip and the HWC -> CHW transpose, to the byte.
//
//   pod_resize_taps / pod_resize_coeffs : host.  Pillow's precompute_coeffs + normalize_coeffs_8bpc for one axis: per output index the
//                  first source index, the tap count and the 22-bit fixed-point coefficients (fp64, no contraction).
//   k_resize_u8  : one workgroup of 64 x 4 output positions, one thread per position, all three channels.  For each of its vertical taps a
//                  thread forms the horizontal sum of that source row and rounds it to uint8 -- Pillow's intermediate image -- then
//                  accumulates the vertical sum; either pass is skipped when its table is absent.  Tap counts are run-time values
//                  (2 - 3 when enlarging, 2 scale + 1 when reducing).  Three byte stores, one per output plane, coalesced along x.
#include "pod_device.h"

#include <cmath>
#include <vector>

namespace pod {

constexpr int RESIZE_BITS = 22;                   // Pillow's PRECISION_BITS = 32 - 8 - 2
constexpr int RESIZE_TX = 64, RESIZE_TY = 4;

struct ResizeArgs {
    const uint8_t* src;
    uint8_t* dst;
    const int32_t *xb, *xc, *yb, *yc;
    int64_t row_stride;
    int32_t in_h, in_w, out_h, out_w, xk, yk, flip, tiles_x;
};

__device__ __forceinline__ int clip8(int v) {     // Pillow's clip8: the lookup table saturates
    v >>= RESIZE_BITS;
    return v < 0 ? 0 : (v > 255 ? 255 : v);
}

__global__ void __launch_bounds__(RESIZE_TX * RESIZE_TY) k_resize_u8(ResizeArgs a) {
    const int x = (blockIdx.x % a.tiles_x) * RESIZE_TX + (threadIdx.x % RESIZE_TX);
    const int y = (blockIdx.x / a.tiles_x) * RESIZE_TY + (threadIdx.x / RESIZE_TX);
    if (x >= a.out_w || y >= a.out_h) return;
    // taps of this position; clamped to the source, whatever the tables say
    int x0 = x, xn = 1, y0 = y, yn = 1;
    if (a.xb != nullptr) {
        x0 = min(max(a.xb[2 * x], 0), a.in_w - 1);
        xn = min(min(a.xb[2 * x + 1], a.xk), a.in_w - x0);
    }
    if (a.yb != nullptr) {
        y0 = min(max(a.yb[2 * y], 0), a.in_h - 1);
        yn = min(min(a.yb[2 * y + 1], a.yk), a.in_h - y0);
    }
    const int32_t* cx = a.xc != nullptr ? a.xc + (int64_t)x * a.xk : nullptr;
    const int32_t* cy = a.yc != nullptr ? a.yc + (int64_t)y * a.yk : nullptr;
    int v[3] = {1 << (RESIZE_BITS - 1), 1 << (RESIZE_BITS - 1), 1 << (RESIZE_BITS - 1)};
    int px[3] = {0, 0, 0};
    for (int ty = 0; ty < yn; ++ty) {
        const uint8_t* row = a.src + (int64_t)(y0 + ty) * a.row_stride + (int64_t)x0 * 3;
        if (cx != nullptr) {
            int h[3] = {1 << (RESIZE_BITS - 1), 1 << (RESIZE_BITS - 1), 1 << (RESIZE_BITS - 1)};
            for (int tx = 0; tx < xn; ++tx) {
                const int k = cx[tx];
                for (int c = 0; c < 3; ++c) h[c] += (int)row[3 * tx + c] * k;
            }
            for (int c = 0; c < 3; ++c) px[c] = clip8(h[c]);      // the uint8 intermediate
        } else {
            for (int c = 0; c < 3; ++c) px[c] = row[c];
        }
        if (cy != nullptr) {
            const int k = cy[ty];
            for (int c = 0; c < 3; ++c) v[c] += px[c] * k;
        }
    }
    const int64_t plane = (int64_t)a.out_h * a.out_w, at = (int64_t)y * a.out_w + x;
    for (int c = 0; c < 3; ++c) {
        const int s = a.flip ? 2 - c : c;
        a.dst[c * plane + at] = (uint8_t)(cy != nullptr ? clip8(v[s]) : px[s]);
    }
}

}  // namespace pod

static bool resize_sizes_ok(int32_t in_size, int32_t out_size) {
    return in_size >= 1 && out_size >= 1 && in_size <= POD_RESIZE_MAX_SIDE && out_size <= POD_RESIZE_MAX_SIDE;
}

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
    if (src == nullptr || dst == nullptr || !resize_sizes_ok(in_w, out_w) || !resize_sizes_ok(in_h, out_h) || row_stride < 3 * (int64_t)in_w)
        return POD_E_INVALID;
    if ((xbounds == nullptr) != (xcoeffs == nullptr) || (ybounds == nullptr) != (ycoeffs == nullptr)) return POD_E_INVALID;
    if (xbounds == nullptr ? (out_w != in_w || xk != 0) : xk != pod_resize_taps(in_w, out_w)) return POD_E_INVALID;
    if (ybounds == nullptr ? (out_h != in_h || yk != 0) : yk != pod_resize_taps(in_h, out_h)) return POD_E_INVALID;
    pod::ResizeArgs a;
    a.src = src; a.dst = dst;
    a.xb = xbounds; a.xc = xcoeffs; a.yb = ybounds; a.yc = ycoeffs;
    a.row_stride = row_stride;
    a.in_h = in_h; a.in_w = in_w; a.out_h = out_h; a.out_w = out_w; a.xk = xk; a.yk = yk;
    a.flip = flip_channels != 0;
    a.tiles_x = (out_w + pod::RESIZE_TX - 1) / pod::RESIZE_TX;
    const int tiles_y = (out_h + pod::RESIZE_TY - 1) / pod::RESIZE_TY;
    hipLaunchKernelGGL(pod::k_resize_u8, dim3((unsigned)(a.tiles_x * tiles_y)), dim3(pod::RESIZE_TX * pod::RESIZE_TY), 0, (hipStream_t)stream, a);
    POD_CHECK_LAUNCH();
    return POD_OK;
}
