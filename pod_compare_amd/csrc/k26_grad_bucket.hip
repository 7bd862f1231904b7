// K26 -- the gradient bucket of data-parallel training: every trained tensor's gradient packed into ONE flat fp32 buffer in ONE launch, scaled
// by 1 / world on the way, so that one collective averages all of them and K25 steps straight from the buffer.
//     bucket[offsets[t] + i] = scale * grad_t[i]
// The layout (pod_grad_bucket_layout) puts tensor t at the running sum of the previous tensors' n, each rounded up to 4 floats: every
// tensor starts on 16 bytes, and what K25 needs of a gradient pointer holds for the slice.  The padding floats between tensors are never
// written: the owner zeroes the bucket once, and a SUM over ranks keeps them zero.  Work is cut as K25 cuts it: the chunk map of the same
// table (pod_sgd_chunk_map), walked by pod_tensor_table.h.  Plain vector loads and stores, nothing shared between lanes: two launches give
// the same bits, and with scale == 1 the bucket holds the gradients' own bits.
#include <cmath>

#include "pod_tensor_table.h"

namespace pod {

// (the chunk walk: pod_tensor_table.h)
__global__ void __launch_bounds__(TABLE_THREADS) k_grad_pack(const PodSgdTensor* __restrict__ table, const int32_t n_tensors, const int32_t* __restrict__ chunk_map,
                                                             const int64_t n_chunks, const int64_t* __restrict__ offsets, float* __restrict__ bucket,
                                                             const int64_t bucket_floats, const float scale) {
    table_chunk_walk(
        table, n_tensors, chunk_map, n_chunks,
        [&](const int32_t t, const PodSgdTensor& d, int64_t) -> float* {       // the tensor's slice (offsets of another table: never a store outside the bucket)
            const int64_t o = offsets[t];
            return (o < 0 || (o & 3) || o > bucket_floats - d.n) ? nullptr : bucket + o;
        },
        [&](const PodSgdTensor& d, const int64_t i, float* dst) {
            if (!dst) return;
            const f32x4 g = *reinterpret_cast<const f32x4*>(d.grad + i);
            *reinterpret_cast<f32x4*>(dst + i) = f32x4{scale * g.x, scale * g.y, scale * g.z, scale * g.w};
        },
        [&](const PodSgdTensor& d, const int64_t i, const int j, float* dst) {
            if (dst) dst[i + j] = scale * d.grad[i + j];
        });
}

}  // namespace pod

extern "C" int64_t pod_grad_bucket_layout(const PodSgdTensor* tensors, int32_t n_tensors, int64_t* offsets) {
    if (pod_sgd_chunk_map(tensors, n_tensors, nullptr, 0) < 0) return -1;     // one rule for what a table is: K25's
    int64_t total = 0;
    for (int32_t t = 0; t < n_tensors; ++t) {
        if (offsets) offsets[t] = total;
        total += (tensors[t].n + 3) / 4 * 4;
    }
    return total;
}

extern "C" int pod_grad_pack(const PodSgdTensor* tensors, PodSgdTensor* tensors_dev, int32_t n_tensors, const int32_t* chunk_map, int64_t n_chunks,
                             const int64_t* offsets_dev, float* bucket, int64_t bucket_floats, float scale, pod_stream_t stream) {
    if (!std::isfinite(scale) || scale <= 0.0f) return POD_E_INVALID;
    const int64_t total = pod_grad_bucket_layout(tensors, n_tensors, nullptr);
    if (total < 0 || bucket_floats != total) return POD_E_INVALID;
    if (n_chunks != pod_sgd_chunk_map(tensors, n_tensors, nullptr, 0)) return POD_E_INVALID;
    for (int32_t t = 0; t < n_tensors; ++t) {
        const PodSgdTensor& d = tensors[t];
        if (d.n == 0) continue;
        if (!d.grad) return POD_E_INVALID;                                     // every trained tensor has a gradient on every rank: not K25's skip
        if (bucket) {
            const uintptr_t b0 = reinterpret_cast<uintptr_t>(bucket), b1 = b0 + sizeof(float) * (uintptr_t)total;
            const uintptr_t g0 = reinterpret_cast<uintptr_t>(d.grad), g1 = g0 + sizeof(float) * (uintptr_t)d.n;
            if (g0 < b1 && b0 < g1) return POD_E_INVALID;
        }
    }
    if (n_chunks == 0) return POD_OK;
    if (!bucket || !tensors_dev || !chunk_map || !offsets_dev) return POD_E_INVALID;
    if (!pod_aligned(16, bucket) || !pod_aligned(8, tensors_dev, offsets_dev) || !pod_aligned(4, chunk_map)) return POD_E_INVALID;
    return pod::table_copy_and_launch(tensors, tensors_dev, n_tensors, n_chunks, (hipStream_t)stream, [&](dim3 blocks, const PodSgdTensor* table) {
        hipLaunchKernelGGL(pod::k_grad_pack, blocks, dim3(pod::TABLE_THREADS), 0, (hipStream_t)stream, table, n_tensors, chunk_map, n_chunks, offsets_dev, bucket,
                           bucket_floats, scale);
    });
}
