// K25 -- the optimiser's step for every trained tensor in ONE launch: SGD with momentum and weight decay as torch.optim.SGD computes it
// (the reference's solver, train_net.py under detectron2's build_optimizer), with FoldedMasters' two side passes folded in: the gradient
// of a FOLDED filter is scaled by FrozenBN's s on the way in (W.grad = s dW') and the folded filter is rewritten from the stepped master
// on the way out (W' = W s).  Per element, fp32, every operation rounded on its own (the library is built with -ffp-contract=off):
//     a = scale ? s[i / per_channel] * g[i] : g[i];  g' = a + wd * w[i];  m' = mu * m[i] + g';  w' = w[i] - lr * m'
//     m[i] = m';  w[i] = w';  folded[i] = w' * s[i / per_channel]
// Work is cut into chunks of POD_SGD_CHUNK elements of ONE tensor, listed in a chunk map (tensor, chunk of that tensor) that is built once
// per parameter set (pod_sgd_chunk_map) and stays on the device: a 2.4 M-element filter is 576 chunks, a 36-float bias one.  The walk over
// the map, shared with K26, is pod_tensor_table.h's: whole float4s, then a tensor's last n % 4 floats (the 63-float bias of cls_score) one
// at a time.  A chunk whose tensor has no gradient this step is left alone, weight decay and momentum decay included, as torch leaves a
// parameter whose .grad is None.  Plain vector loads and stores; nothing is shared between lanes, so two launches give the same bits.
#include <cmath>

#include "pod_tensor_table.h"

namespace pod {

struct SgdHyper {
    float lr, mu, wd;
};

__device__ __forceinline__ void sgd_one(float& w, float& m, const float a, const SgdHyper h) {
    const float g = a + h.wd * w;
    m = h.mu * m + g;
    w = w - h.lr * m;
}

// (the chunk walk: pod_tensor_table.h)
__global__ void __launch_bounds__(TABLE_THREADS) k_sgd_step(const PodSgdTensor* __restrict__ table, const int32_t n_tensors, const int32_t* __restrict__ chunk_map,
                                                            const int64_t n_chunks, const SgdHyper h) {
    table_chunk_walk(
        table, n_tensors, chunk_map, n_chunks,
        [&](int32_t, const PodSgdTensor& d, const int64_t i) { return table_scale4(d, i); },      // FrozenBN's s of the four elements at i
        [&](const PodSgdTensor& d, const int64_t i, const f32x4 s) {
            const f32x4 g = *reinterpret_cast<const f32x4*>(d.grad + i);
            const f32x4 w4 = *reinterpret_cast<const f32x4*>(d.w + i);
            const f32x4 m4 = *reinterpret_cast<const f32x4*>(d.momentum + i);
            float w[4] = {w4.x, w4.y, w4.z, w4.w}, m[4] = {m4.x, m4.y, m4.z, m4.w};
            const float a[4] = {g.x, g.y, g.z, g.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) sgd_one(w[j], m[j], d.scale ? s[j] * a[j] : a[j], h);
            *reinterpret_cast<f32x4*>(d.momentum + i) = f32x4{m[0], m[1], m[2], m[3]};
            *reinterpret_cast<f32x4*>(d.w + i) = f32x4{w[0], w[1], w[2], w[3]};
            if (d.folded) *reinterpret_cast<f32x4*>(d.folded + i) = f32x4{w[0] * s[0], w[1] * s[1], w[2] * s[2], w[3] * s[3]};
        },
        [&](const PodSgdTensor& d, const int64_t i, const int j, const f32x4 s) {
            float w = d.w[i + j], m = d.momentum[i + j];
            const float g = d.grad[i + j];
            sgd_one(w, m, d.scale ? s[j] * g : g, h);
            d.momentum[i + j] = m;
            d.w[i + j] = w;
            if (d.folded) d.folded[i + j] = w * s[j];
        });
}

}  // namespace pod

static bool sgd_tensor_ok(const PodSgdTensor& d) {
    if (!d.w || !d.momentum || d.n < 0 || d.w == d.momentum) return false;
    if (!pod_aligned(16, d.w, d.grad, d.momentum, d.folded, d.scale)) return false;
    if (d.scale && (d.per_channel <= 0 || d.n % d.per_channel != 0)) return false;
    if (d.folded && (!d.scale || d.folded == d.w || d.folded == d.momentum)) return false;
    return d.n <= (int64_t)INT32_MAX * POD_SGD_CHUNK;                          // (the chunk map holds a tensor's chunk as an int32)
}

extern "C" int64_t pod_sgd_chunk_map(const PodSgdTensor* tensors, int32_t n_tensors, int32_t* map, int64_t capacity) {
    if (n_tensors < 0 || (n_tensors > 0 && !tensors)) return -1;
    int64_t total = 0;
    for (int32_t t = 0; t < n_tensors; ++t) {
        if (!sgd_tensor_ok(tensors[t])) return -1;
        total += (tensors[t].n + POD_SGD_CHUNK - 1) / POD_SGD_CHUNK;
    }
    if (!map || capacity < total) return total;                                // (a map too small for the whole list is left alone)
    int64_t k = 0;
    for (int32_t t = 0; t < n_tensors; ++t)
        for (int64_t c = 0; c * POD_SGD_CHUNK < tensors[t].n; ++c, ++k) {
            map[2 * k] = t;
            map[2 * k + 1] = (int32_t)c;
        }
    return total;
}

extern "C" int pod_sgd_step(const PodSgdTensor* tensors, PodSgdTensor* tensors_dev, int32_t n_tensors, const int32_t* chunk_map, int64_t n_chunks,
                            float lr, float momentum, float weight_decay, pod_stream_t stream) {
    if (!std::isfinite(lr) || !std::isfinite(momentum) || !std::isfinite(weight_decay)) return POD_E_INVALID;
    if (momentum < 0.0f || momentum >= 1.0f || weight_decay < 0.0f) return POD_E_INVALID;
    const int64_t expect = pod_sgd_chunk_map(tensors, n_tensors, nullptr, 0);
    if (expect < 0 || n_chunks != expect) return POD_E_INVALID;
    if (n_chunks == 0) return POD_OK;
    if (!tensors_dev || !chunk_map || !pod_aligned(8, tensors_dev) || !pod_aligned(4, chunk_map)) return POD_E_INVALID;
    return pod::table_copy_and_launch(tensors, tensors_dev, n_tensors, n_chunks, (hipStream_t)stream, [&](dim3 blocks, const PodSgdTensor* table) {
        hipLaunchKernelGGL(pod::k_sgd_step, blocks, dim3(pod::TABLE_THREADS), 0, (hipStream_t)stream, table, n_tensors, chunk_map, n_chunks,
                           pod::SgdHyper{lr, momentum, weight_decay});
    });
}
