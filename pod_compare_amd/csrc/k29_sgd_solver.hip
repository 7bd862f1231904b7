// K29 -- K25's step under the whole SOLVER section: gradient clipping (by value or by norm per parameter tensor, or by one norm over the full
// model), parameter groups with their own learning rate and weight decay (detectron2's BIAS_LR_FACTOR / WEIGHT_DECAY_BIAS), Nesterov momentum,
// and a guard that turns a step with a non-finite gradient or loss, and every step after it, into a no-op.  Per element, fp32, every
// operation rounded on its own (the library is built with -ffp-contract=off), G = group[t]:
//     a0 = scale ? s[i / per_channel] * g[i] : g[i]                       (K25's)
//     a  = a0 | a0 < -v ? -v : a0 > v ? v : a0 | coef[t] * a0 | coef[n_tensors] * a0        (off | value | norm | full_model)
//     g' = a + wd[G] * w[i];  m' = mu * m[i] + g';  d = nesterov ? g' + mu * m' : m';  w' = w[i] - lr[G] * d
//     m[i] = m';  w[i] = w';  folded[i] = w' * s[i / per_channel]
// Off or value without the guard is ONE launch, k_sgd_step_solver.  A norm or the guard makes it three plain launches on one stream:
//     k_grad_sumsq   the walk of K25 over the same chunk map; per chunk ONE fp64 partial = sum a0^2, summed per lane in index order, by
//                    wave_sum over the 64 lanes, then over the four wavefronts in order -- an order the grid has no part in
//     k_clip_coef    ONE workgroup: a tensor's partials in chunk order (one lane per tensor), the tensors in table order (lane 0); writes
//                    coef[t], coef[n_tensors], the norm and -- a non-finite N_t^2 or watched scalar -- the status
//     k_sgd_step_solver   reads coef and, first of all, status.poisoned: a poisoned workspace is left before the first store
// No atomics, no grid barrier, no read-back: two calls from one state give the same bits, partial and coef included.  The reduce pass
// reads the gradients (and s of the folded entries) once more; the step streams K25's bytes.
#include <cmath>

#include "pod_tensor_table.h"

namespace pod {

struct SolverHyper {
    float lr[POD_SGD_MAX_GROUPS], wd[POD_SGD_MAX_GROUPS];
    float mu, clip_value;
};
struct SolverTrip {                                                            // what a lane's trip needs: s of its four elements, its tensor's rates
    f32x4 s;
    float lr, wd, coef;
};
struct SolverReduce {
    float clip_value;
    int32_t guard;
    int64_t iteration;
    const float* watch[4];
};

template <int CLIP, bool NESTEROV>
__device__ __forceinline__ void solver_one(float& w, float& m, float a, const SolverTrip& st, const float mu, const float v) {
    if (CLIP == POD_SGD_CLIP_VALUE) {
        a = a < -v ? -v : a;                                                   // (comparisons: a NaN passes through, as torch's clamp leaves it)
        a = a > v ? v : a;
    } else if (CLIP != POD_SGD_CLIP_OFF) {
        a = st.coef * a;
    }
    const float g = a + st.wd * w;
    m = mu * m + g;
    const float d = NESTEROV ? g + mu * m : m;
    w = w - st.lr * d;
}

// (the chunk walk: pod_tensor_table.h)  GROUPS false: one group, its rates straight from the kernel's arguments; true: group[t] and the
// rates it indexes are two dependent loads per trip (profiles/solver_step.md has what they cost).  The default record -- one group, no
// clipping, no Nesterov, no guard -- never comes here: the entry hands it to pod_sgd_step, K25's own launch.
template <int CLIP, bool NESTEROV, bool GROUPS>
__global__ void __launch_bounds__(TABLE_THREADS) k_sgd_step_solver(const PodSgdTensor* __restrict__ table, const int32_t n_tensors, const int32_t* __restrict__ chunk_map,
                                                                   const int64_t n_chunks, const uint8_t* __restrict__ group, const float* __restrict__ coef,
                                                                   const int32_t* __restrict__ poisoned, const SolverHyper h) {
    if (poisoned && *poisoned) return;
    table_chunk_walk(
        table, n_tensors, chunk_map, n_chunks,
        [&](const int32_t t, const PodSgdTensor& d, const int64_t i) {
            const int G = GROUPS ? group[t] & (POD_SGD_MAX_GROUPS - 1) : 0;    // (the host checked group[t] < n_groups on its copy)
            return SolverTrip{table_scale4(d, i), h.lr[G], h.wd[G],
                              CLIP == POD_SGD_CLIP_NORM ? coef[t] : CLIP == POD_SGD_CLIP_FULL_MODEL ? coef[n_tensors] : 1.f};
        },
        [&](const PodSgdTensor& d, const int64_t i, const SolverTrip& st) {
            const f32x4 g = *reinterpret_cast<const f32x4*>(d.grad + i);
            const f32x4 w4 = *reinterpret_cast<const f32x4*>(d.w + i);
            const f32x4 m4 = *reinterpret_cast<const f32x4*>(d.momentum + i);
            float w[4] = {w4.x, w4.y, w4.z, w4.w}, m[4] = {m4.x, m4.y, m4.z, m4.w};
            const float a[4] = {g.x, g.y, g.z, g.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) solver_one<CLIP, NESTEROV>(w[j], m[j], d.scale ? st.s[j] * a[j] : a[j], st, h.mu, h.clip_value);
            *reinterpret_cast<f32x4*>(d.momentum + i) = f32x4{m[0], m[1], m[2], m[3]};
            *reinterpret_cast<f32x4*>(d.w + i) = f32x4{w[0], w[1], w[2], w[3]};
            if (d.folded) *reinterpret_cast<f32x4*>(d.folded + i) = f32x4{w[0] * st.s[0], w[1] * st.s[1], w[2] * st.s[2], w[3] * st.s[3]};
        },
        [&](const PodSgdTensor& d, const int64_t i, const int j, const SolverTrip& st) {
            float w = d.w[i + j], m = d.momentum[i + j];
            const float g = d.grad[i + j];
            solver_one<CLIP, NESTEROV>(w, m, d.scale ? st.s[j] * g : g, st, h.mu, h.clip_value);
            d.momentum[i + j] = m;
            d.w[i + j] = w;
            if (d.folded) d.folded[i + j] = w * st.s[j];
        });
}

// partial[ci] = sum of a0^2 over the chunk of map entry ci, fp64.  A chunk the walk leaves alone (no gradient) gets no partial.
__global__ void __launch_bounds__(TABLE_THREADS) k_grad_sumsq(const PodSgdTensor* __restrict__ table, const int32_t n_tensors, const int32_t* __restrict__ chunk_map,
                                                              const int64_t n_chunks, double* __restrict__ partial) {
    __shared__ double by_wave[TABLE_THREADS / 64];
    double acc = 0.0;                                                          // this lane's elements of the chunk in hand, in index order
    table_chunk_walk(
        table, n_tensors, chunk_map, n_chunks, [&](int32_t, const PodSgdTensor& d, const int64_t i) { return table_scale4(d, i); },
        [&](const PodSgdTensor& d, const int64_t i, const f32x4 s) {
            const f32x4 g = *reinterpret_cast<const f32x4*>(d.grad + i);
            const float a[4] = {g.x, g.y, g.z, g.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const double a0 = (double)(d.scale ? s[j] * a[j] : a[j]);
                acc += a0 * a0;
            }
        },
        [&](const PodSgdTensor& d, const int64_t i, const int j, const f32x4 s) {
            const double a0 = (double)(d.scale ? s[j] * d.grad[i + j] : d.grad[i + j]);
            acc += a0 * a0;
        },
        [&](const int64_t ci) {
            const double w = wave_sum(acc);
            acc = 0.0;
            if ((threadIdx.x & 63) == 0) by_wave[threadIdx.x >> 6] = w;
            __syncthreads();
            if (threadIdx.x == 0) partial[ci] = ((by_wave[0] + by_wave[1]) + by_wave[2]) + by_wave[3];
            __syncthreads();                                                   // (by_wave is rewritten by the next chunk)
        });
}

constexpr int COEF_TILE = 1024;                                                // tensors per pass of k_clip_coef (a table has some hundred)

__device__ __forceinline__ float clip_coef(const double sumsq, const float v) {
    const double c = (double)v / (sqrt(sumsq) + 1e-6);
    return (float)(c > 1.0 ? 1.0 : c);                                         // (a NaN stays a NaN)
}

// ONE workgroup.  Per pass of COEF_TILE tensors: where each tensor's chunks start in the map (its entry with chunk 0), one lane per tensor
// over its partials in chunk order, then lane 0 over the tensors in table order.
__global__ void __launch_bounds__(TABLE_THREADS) k_clip_coef(const PodSgdTensor* __restrict__ table, const int32_t n_tensors, const int32_t* __restrict__ chunk_map,
                                                             const int64_t n_chunks, const double* __restrict__ partial, float* __restrict__ coef,
                                                             PodSgdSolverStatus* __restrict__ status, const SolverReduce p) {
    __shared__ int64_t first[COEF_TILE];
    __shared__ double sumsq[COEF_TILE];
    if (status->poisoned) return;                                              // (read by every lane before any lane writes: uniform)
    double total = 0.0;                                                        // lane 0's
    bool bad = false;
    for (int32_t t0 = 0; t0 < n_tensors; t0 += COEF_TILE) {
        const int32_t nt = n_tensors - t0 < COEF_TILE ? n_tensors - t0 : COEF_TILE;
        for (int32_t k = threadIdx.x; k < nt; k += TABLE_THREADS) first[k] = -1;
        __syncthreads();
        for (int64_t ci = threadIdx.x; ci < n_chunks; ci += TABLE_THREADS) {
            const int32_t t = chunk_map[2 * ci];
            if (chunk_map[2 * ci + 1] == 0 && t >= t0 && t < t0 + nt) first[t - t0] = ci;
        }
        __syncthreads();
        for (int32_t k = threadIdx.x; k < nt; k += TABLE_THREADS) {
            const PodSgdTensor d = table[t0 + k];
            const int64_t chunks = (d.n + POD_SGD_CHUNK - 1) / POD_SGD_CHUNK, f = first[k];
            const bool live = d.grad != nullptr && (chunks == 0 || (f >= 0 && f <= n_chunks - chunks));      // (a map of another table: nothing is read outside partial)
            double s = 0.0;
            if (live) {
#pragma unroll 8
                for (int64_t c = 0; c < chunks; ++c) s += partial[f + c];
            }
            sumsq[k] = s;                                                      // (0 of a tensor without a gradient: it changes no sum)
            coef[t0 + k] = live ? clip_coef(s, p.clip_value) : 1.f;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            for (int32_t k = 0; k < nt; ++k) {
                total += sumsq[k];
                bad = bad || !std::isfinite(sumsq[k]);
            }
        }
        __syncthreads();
    }
    if (threadIdx.x != 0) return;
#pragma unroll
    for (int q = 0; q < 4; ++q)
        if (p.watch[q]) bad = bad || !std::isfinite(*p.watch[q]);
    coef[n_tensors] = clip_coef(total, p.clip_value);
    status->last_norm = sqrt(total);
    if (bad) {
        if (status->bad_steps == 0) status->first_bad_iteration = p.iteration;
        status->bad_steps += 1;
        if (p.guard) status->poisoned = 1;
    }
}

__global__ void k_solver_reset(PodSgdSolverStatus* status) {
    if (threadIdx.x == 0) *status = PodSgdSolverStatus{0, 0, 0.0, 0, 0};
}

using StepKernel = void (*)(const PodSgdTensor*, int32_t, const int32_t*, int64_t, const uint8_t*, const float*, const int32_t*, SolverHyper);
template <int CLIP>
static StepKernel step_kernel_of(bool nesterov, bool groups) {
    return nesterov ? (groups ? k_sgd_step_solver<CLIP, true, true> : k_sgd_step_solver<CLIP, true, false>)
                    : (groups ? k_sgd_step_solver<CLIP, false, true> : k_sgd_step_solver<CLIP, false, false>);
}

}  // namespace pod

static constexpr size_t SOLVER_STATUS_BYTES = 32;
static_assert(sizeof(PodSgdSolverStatus) == SOLVER_STATUS_BYTES, "the workspace starts with the status record");

extern "C" size_t pod_sgd_solver_workspace_bytes(int32_t n_tensors, int64_t n_chunks) {
    if (n_tensors < 0 || n_chunks < 0) return 0;
    const size_t bytes = SOLVER_STATUS_BYTES + sizeof(double) * (size_t)n_chunks + sizeof(float) * ((size_t)n_tensors + 1);
    return (bytes + 15) / 16 * 16;
}

extern "C" int pod_sgd_solver_reset(void* workspace, pod_stream_t stream) {
    if (!workspace || !pod_aligned(16, workspace)) return POD_E_INVALID;
    hipLaunchKernelGGL(pod::k_solver_reset, dim3(1), dim3(64), 0, (hipStream_t)stream, (PodSgdSolverStatus*)workspace);
    POD_CHECK_LAUNCH();
    return POD_OK;
}

extern "C" int pod_sgd_step_solver(const PodSgdTensor* tensors, PodSgdTensor* tensors_dev, int32_t n_tensors, const int32_t* chunk_map, int64_t n_chunks,
                                   const uint8_t* group, const uint8_t* group_dev, const PodSgdSolver* solver, void* workspace, pod_stream_t stream) {
    if (!solver || solver->n_groups < 1 || solver->n_groups > POD_SGD_MAX_GROUPS) return POD_E_INVALID;
    const PodSgdSolver& sv = *solver;
    for (int g = 0; g < sv.n_groups; ++g)
        if (!std::isfinite(sv.lr[g]) || !std::isfinite(sv.wd[g]) || sv.lr[g] < 0.0f || sv.wd[g] < 0.0f) return POD_E_INVALID;
    if (!std::isfinite(sv.momentum) || sv.momentum < 0.0f || sv.momentum >= 1.0f) return POD_E_INVALID;
    if (sv.nesterov && sv.momentum == 0.0f) return POD_E_INVALID;
    if (sv.clip_type < POD_SGD_CLIP_OFF || sv.clip_type > POD_SGD_CLIP_FULL_MODEL) return POD_E_INVALID;
    if (sv.clip_type != POD_SGD_CLIP_OFF && !(std::isfinite(sv.clip_value) && sv.clip_value > 0.0f)) return POD_E_INVALID;
    const int64_t expect = pod_sgd_chunk_map(tensors, n_tensors, nullptr, 0);  // (one rule for what a table is: K25's)
    if (expect < 0 || n_chunks != expect) return POD_E_INVALID;
    if (n_tensors > 0 && !group) return POD_E_INVALID;
    for (int32_t t = 0; t < n_tensors; ++t)
        if (group[t] >= sv.n_groups) return POD_E_INVALID;
    if (n_chunks == 0) return POD_OK;
    if (!tensors_dev || !chunk_map || !pod_aligned(8, tensors_dev) || !pod_aligned(4, chunk_map)) return POD_E_INVALID;
    if (!workspace || !group_dev || !pod_aligned(16, workspace) || !pod_aligned(4, sv.watch[0], sv.watch[1], sv.watch[2], sv.watch[3])) return POD_E_INVALID;

    const bool reduce = sv.guard || sv.clip_type == POD_SGD_CLIP_NORM || sv.clip_type == POD_SGD_CLIP_FULL_MODEL;
    // the default record IS K25: its own kernel, launched by its own entry (every check above holds for it)
    if (!reduce && sv.n_groups == 1 && sv.clip_type == POD_SGD_CLIP_OFF && !sv.nesterov)
        return pod_sgd_step(tensors, tensors_dev, n_tensors, chunk_map, n_chunks, sv.lr[0], sv.momentum, sv.wd[0], stream);

    auto* status = (PodSgdSolverStatus*)workspace;
    auto* partial = (double*)((char*)workspace + SOLVER_STATUS_BYTES);
    auto* coef = (float*)(partial + n_chunks);
    pod::SolverHyper h{};
    for (int g = 0; g < POD_SGD_MAX_GROUPS; ++g) h.lr[g] = g < sv.n_groups ? sv.lr[g] : 0.0f, h.wd[g] = g < sv.n_groups ? sv.wd[g] : 0.0f;
    h.mu = sv.momentum;
    h.clip_value = sv.clip_value;
    const bool nesterov = sv.nesterov != 0, groups = sv.n_groups > 1;
    const pod::StepKernel step = sv.clip_type == POD_SGD_CLIP_VALUE  ? pod::step_kernel_of<POD_SGD_CLIP_VALUE>(nesterov, groups)
                                 : sv.clip_type == POD_SGD_CLIP_NORM ? pod::step_kernel_of<POD_SGD_CLIP_NORM>(nesterov, groups)
                                 : sv.clip_type == POD_SGD_CLIP_FULL_MODEL ? pod::step_kernel_of<POD_SGD_CLIP_FULL_MODEL>(nesterov, groups)
                                                                           : pod::step_kernel_of<POD_SGD_CLIP_OFF>(nesterov, groups);
    const hipStream_t s = (hipStream_t)stream;
    return pod::table_copy_and_launch(tensors, tensors_dev, n_tensors, n_chunks, s, [&](dim3 blocks, const PodSgdTensor* table) {
        if (reduce) {
            hipLaunchKernelGGL(pod::k_grad_sumsq, blocks, dim3(pod::TABLE_THREADS), 0, s, table, n_tensors, chunk_map, n_chunks, partial);
            hipLaunchKernelGGL(pod::k_clip_coef, dim3(1), dim3(pod::TABLE_THREADS), 0, s, table, n_tensors, chunk_map, n_chunks, (const double*)partial, coef, status,
                               pod::SolverReduce{sv.clip_value, sv.guard, sv.iteration, {sv.watch[0], sv.watch[1], sv.watch[2], sv.watch[3]}});
        }
        hipLaunchKernelGGL(step, blocks, dim3(pod::TABLE_THREADS), 0, s, table, n_tensors, chunk_map, n_chunks, group_dev, (const float*)coef,
                           reduce ? (const int32_t*)&status->poisoned : (const int32_t*)nullptr, h);
    });
}
