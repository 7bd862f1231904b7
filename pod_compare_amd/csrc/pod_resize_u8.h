// What K20 (k20_resize_u8.hip, one frame per launch) and K31 (k31_train_batch.hip, a training batch per launch) share: Pillow's 8-bit
// bilinear resample of ONE output position -- the taps of the position, the horizontal sums of its source rows rounded to the uint8
// intermediate image, the vertical sum, clip8 -- and the host's check of a frame's sizes and tables.  One copy: the bytes of the two
// kernels cannot drift apart.
#pragma once
#include "pod_device.h"

namespace pod {

constexpr int RESIZE_BITS = 22;                   // Pillow's PRECISION_BITS = 32 - 8 - 2
constexpr int RESIZE_TX = 64, RESIZE_TY = 4;      // a workgroup's output positions

struct ResizeSource {                             // the frame read and its two axis tables (an axis without tables keeps its size)
    const uint8_t* src;
    const int32_t *xb, *xc, *yb, *yc;
    int64_t row_stride;
    int32_t in_h, in_w, xk, yk;
};

__device__ __forceinline__ int clip8(int v) {     // Pillow's clip8: the lookup table saturates
    v >>= RESIZE_BITS;
    return v < 0 ? 0 : (v > 255 ? 255 : v);
}

// The three channels (source order) of position (x, y) of the resized frame.
__device__ __forceinline__ void resize_position_u8(const ResizeSource& a, const int x, const int y, int out[3]) {
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
    for (int c = 0; c < 3; ++c) out[c] = cy != nullptr ? clip8(v[c]) : px[c];
}

}  // namespace pod

static inline bool resize_sizes_ok(int32_t in_size, int32_t out_size) {
    return in_size >= 1 && out_size >= 1 && in_size <= POD_RESIZE_MAX_SIDE && out_size <= POD_RESIZE_MAX_SIDE;
}

// What pod_resize_frame_u8 accepts of one frame (pod_resize_taps: k20_resize_u8.hip).
static inline bool resize_frame_ok(const uint8_t* src, int32_t in_h, int32_t in_w, int64_t row_stride, const int32_t* xbounds, const int32_t* xcoeffs,
                                   int32_t xk, const int32_t* ybounds, const int32_t* ycoeffs, int32_t yk, const uint8_t* dst, int32_t out_h, int32_t out_w) {
    if (src == nullptr || dst == nullptr || !resize_sizes_ok(in_w, out_w) || !resize_sizes_ok(in_h, out_h) || row_stride < 3 * (int64_t)in_w)
        return false;
    if ((xbounds == nullptr) != (xcoeffs == nullptr) || (ybounds == nullptr) != (ycoeffs == nullptr)) return false;
    if (xbounds == nullptr ? (out_w != in_w || xk != 0) : xk != pod_resize_taps(in_w, out_w)) return false;
    if (ybounds == nullptr ? (out_h != in_h || yk != 0) : yk != pod_resize_taps(in_h, out_h)) return false;
    return true;
}
