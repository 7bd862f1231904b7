// A training batch in ONE launch (train_head --train-loader --batch-on-gpu; pod_compare_amd/train_batch.py): every decoded frame of a
// rank's batch resized with Pillow's 8-bit bilinear filter at its own drawn size, mirrored where its flip was drawn (resize first, then
// flip: detectron2's order of transforms), its channels flipped to BGR and transposed to CHW -- K20's work per frame, to the byte
// (pod_resize_u8.h holds the one copy of the arithmetic).
//
//   k_train_batch_u8 : one workgroup of 64 x 4 output positions, as K20.  The table (PodTrainFrame per frame, at most
//                  POD_TRAIN_BATCH_MAX_FRAMES) lists every frame's first workgroup; a workgroup finds its frame by a search of those, takes
//                  its tile of that frame and writes the frame's own contiguous (3, out_h, out_w) tensor.  With hflip output column x holds
//                  the resized frame's column out_w - 1 - x.  There is no padded batch tensor: a zero byte is not zero after
//                  normalisation, the padding stays in the stem's load (pod_stem7x7_split, H_img <= H).
// The table travels as K25's and K26's do (pod_tensor_table.h): one copy from the caller's pinned host table, ordered on the stream
// before the launch; the caller keeps the host table unchanged until it has run.
#include "pod_resize_u8.h"

namespace pod {

__global__ void __launch_bounds__(RESIZE_TX * RESIZE_TY) k_train_batch_u8(const PodTrainFrame* __restrict__ frames, const int32_t n_frames) {
    // the last frame whose first tile is not behind this workgroup's (first_tile ascends from 0); uniform over the workgroup
    const int64_t tile_all = blockIdx.x;
    int lo = 0, hi = n_frames - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (frames[mid].first_tile <= tile_all) lo = mid; else hi = mid - 1;
    }
    const PodTrainFrame f = frames[lo];
    const int64_t tile = tile_all - f.first_tile;
    const int tiles_x = (f.out_w + RESIZE_TX - 1) / RESIZE_TX;
    const int x = (int)(tile % tiles_x) * RESIZE_TX + (threadIdx.x % RESIZE_TX);
    const int64_t y = (tile / tiles_x) * RESIZE_TY + (threadIdx.x / RESIZE_TX);
    if (tile < 0 || x >= f.out_w || y >= f.out_h) return;         // every store lies inside its frame's extent
    ResizeSource a;
    a.src = f.src; a.xb = f.xbounds; a.xc = f.xcoeffs; a.yb = f.ybounds; a.yc = f.ycoeffs;
    a.row_stride = f.row_stride; a.in_h = f.in_h; a.in_w = f.in_w; a.xk = f.xk; a.yk = f.yk;
    int px[3];
    resize_position_u8(a, f.hflip ? f.out_w - 1 - x : x, (int)y, px);
    const int64_t plane = (int64_t)f.out_h * f.out_w, at = y * f.out_w + x;
    for (int c = 0; c < 3; ++c) f.dst[c * plane + at] = (uint8_t)px[f.flip_channels ? 2 - c : c];
}

}  // namespace pod

static inline int64_t train_frame_tiles(const PodTrainFrame& f) {
    return (int64_t)((f.out_w + pod::RESIZE_TX - 1) / pod::RESIZE_TX) * ((f.out_h + pod::RESIZE_TY - 1) / pod::RESIZE_TY);
}

static inline bool ranges_overlap(const uint8_t* a, int64_t na, const uint8_t* b, int64_t nb) {
    const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
    return pa < pb + (uintptr_t)nb && pb < pa + (uintptr_t)na;
}

extern "C" int64_t pod_train_batch_tiles(const PodTrainFrame* frames, int32_t n_frames) {
    if (frames == nullptr || n_frames < 1 || n_frames > POD_TRAIN_BATCH_MAX_FRAMES) return POD_E_INVALID;
    int64_t n = 0;
    for (int i = 0; i < n_frames; ++i) {
        if (!resize_sizes_ok(1, frames[i].out_w) || !resize_sizes_ok(1, frames[i].out_h)) return POD_E_INVALID;
        n += train_frame_tiles(frames[i]);
    }
    return n;
}

extern "C" int pod_train_batch_u8(const PodTrainFrame* frames, PodTrainFrame* frames_dev, int32_t n_frames, int64_t n_tiles, pod_stream_t stream) {
    if (frames == nullptr || frames_dev == nullptr || n_frames < 1 || n_frames > POD_TRAIN_BATCH_MAX_FRAMES) return POD_E_INVALID;
    int64_t tiles = 0;
    for (int i = 0; i < n_frames; ++i) {
        const PodTrainFrame& f = frames[i];
        if (!resize_frame_ok(f.src, f.in_h, f.in_w, f.row_stride, f.xbounds, f.xcoeffs, f.xk, f.ybounds, f.ycoeffs, f.yk, f.dst, f.out_h, f.out_w))
            return POD_E_INVALID;
        if (f.first_tile != tiles) return POD_E_INVALID;
        tiles += train_frame_tiles(f);
    }
    if (n_tiles != tiles || tiles > 0x7fffffffLL) return POD_E_INVALID;
    for (int i = 0; i < n_frames; ++i) {
        const int64_t out_i = 3 * (int64_t)frames[i].out_h * frames[i].out_w;
        for (int j = 0; j < n_frames; ++j) {
            const PodTrainFrame& g = frames[j];
            if (j > i && ranges_overlap(frames[i].dst, out_i, g.dst, 3 * (int64_t)g.out_h * g.out_w)) return POD_E_INVALID;
            if (ranges_overlap(frames[i].dst, out_i, g.src, (int64_t)(g.in_h - 1) * g.row_stride + 3 * (int64_t)g.in_w)) return POD_E_INVALID;
        }
    }
    const hipStream_t s = (hipStream_t)stream;
    if (hipMemcpyAsync(frames_dev, frames, sizeof(PodTrainFrame) * (size_t)n_frames, hipMemcpyHostToDevice, s) != hipSuccess) return POD_E_LAUNCH;
    hipLaunchKernelGGL(pod::k_train_batch_u8, dim3((unsigned)tiles), dim3(pod::RESIZE_TX * pod::RESIZE_TY), 0, s, (const PodTrainFrame*)frames_dev, n_frames);
    POD_CHECK_LAUNCH();
    return POD_OK;
}
