// What the launches over a tensor table share (k25_sgd_step.hip, k26_grad_bucket.hip, k29_sgd_solver.hip; training only -- nothing on the
// inference path includes this): the walk over the table's chunk map, FrozenBN's s of a lane's trip, and the host tail of an entry -- the
// table's copy to the device and the launch.
// A table is PodSgdTensor per trained tensor; its chunk map (pod_sgd_chunk_map) lists (tensor, chunk of POD_SGD_CHUNK elements of it).
#pragma once
#include "pod_device.h"

namespace pod {

constexpr int TABLE_THREADS = 256;
constexpr int TABLE_MAX_BLOCKS = 2048;          // 256 CUs x 8 workgroups: the memory-bound grid cap, the rest by grid stride

// The workgroups walk the chunk map with a grid stride; a workgroup takes a chunk in 4 trips of 256 lanes x 16 bytes.  A lane's trip at
// element i of tensor t (descriptor d): st = trip(t, d, i), what the kernel needs of the trip, then quad(d, i, st) for a whole float4, or
// one(d, i, j, st) for each element i + j of the n % 4 behind a tensor's last whole float4, on the lane that would have held them.
// A chunk whose tensor has no gradient is left alone, and a map that does not belong to the table touches nothing.  done(ci), if given,
// is called by every lane of the workgroup behind the trips of map entry ci (K29's reduction of a chunk); a chunk left alone has no done.
template <class Trip, class Quad, class One, class Done>
__device__ __forceinline__ void table_chunk_walk(const PodSgdTensor* __restrict__ table, const int32_t n_tensors, const int32_t* __restrict__ chunk_map,
                                                 const int64_t n_chunks, Trip&& trip, Quad&& quad, One&& one, Done&& done) {
    for (int64_t ci = blockIdx.x; ci < n_chunks; ci += gridDim.x) {
        const int32_t t = chunk_map[2 * ci], chunk = chunk_map[2 * ci + 1];
        if (t < 0 || t >= n_tensors || chunk < 0) continue;
        const PodSgdTensor d = table[t];
        const int64_t first = (int64_t)chunk * POD_SGD_CHUNK;
        if (d.grad == nullptr || first >= d.n) continue;
        const int64_t end = first + POD_SGD_CHUNK < d.n ? first + POD_SGD_CHUNK : d.n;
        for (int64_t i = first + 4 * (int64_t)threadIdx.x; i < end; i += 4 * TABLE_THREADS) {
            const auto st = trip(t, d, i);
            if (i + 4 <= end) {
                quad(d, i, st);
            } else {
#pragma unroll
                for (int j = 0; j < 3; ++j) {
                    if (i + j >= end) break;
                    one(d, i, j, st);
                }
            }
        }
        done(ci);
    }
}
template <class Trip, class Quad, class One>
__device__ __forceinline__ void table_chunk_walk(const PodSgdTensor* __restrict__ table, const int32_t n_tensors, const int32_t* __restrict__ chunk_map,
                                                 const int64_t n_chunks, Trip&& trip, Quad&& quad, One&& one) {
    table_chunk_walk(table, n_tensors, chunk_map, n_chunks, trip, quad, one, [](int64_t) {});
}

// FrozenBN's s of the four elements at i of a tensor with a scale (1 where there is none): the channel of element i and how far into it i
// lies by one division per trip, then a walk (per_channel may be 1).
__device__ __forceinline__ f32x4 table_scale4(const PodSgdTensor& d, const int64_t i) {
    f32x4 s = {1.f, 1.f, 1.f, 1.f};
    if (d.scale) {
        int64_t c;
        if (((uint64_t)i | (uint64_t)d.per_channel) >> 32) {
            c = i / d.per_channel;
        } else {
            c = (int64_t)((uint32_t)i / (uint32_t)d.per_channel);
        }
        int64_t r = i - c * d.per_channel;
        const int64_t c_last = (d.n - 1) / d.per_channel;                      // (never read behind the last channel for lanes past a tail)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            s[j] = d.scale[c < c_last ? c : c_last];
            if (++r == d.per_channel) {
                r = 0;
                ++c;
            }
        }
    }
    return s;
}

// Host: the common tail of pod_sgd_step and pod_grad_pack.  The table changes every step (gradients are fresh allocations): one copy, ordered
// on the stream before launch(blocks, table on the device).  From pinned memory it is asynchronous, and the caller keeps `tensors`
// unchanged until it has run (an event after the entry's return).
template <class Launch>
static inline int table_copy_and_launch(const PodSgdTensor* tensors, PodSgdTensor* tensors_dev, int32_t n_tensors, int64_t n_chunks, hipStream_t s, Launch&& launch) {
    if (hipMemcpyAsync(tensors_dev, tensors, sizeof(PodSgdTensor) * (size_t)n_tensors, hipMemcpyHostToDevice, s) != hipSuccess) return POD_E_LAUNCH;
    launch(dim3((unsigned)(n_chunks < TABLE_MAX_BLOCKS ? n_chunks : TABLE_MAX_BLOCKS)), (const PodSgdTensor*)tensors_dev);
    POD_CHECK_LAUNCH();
    return POD_OK;
}

}  // namespace pod
