// K36: post-hoc recalibration -- the sums of a temperature fit, the standardised regression residuals, their moment and
// calibration-error fits of per-coordinate variance scales, and the map applied to K7's record table (include/pod_mi355x.h has the
// definitions; the reference recalibrates nothing).
//
//   k_recal_cls_chunks   : one wavefront per 256-score chunk: every lane forms four terms of L, g and h in fp64 (one exp, one log1p; the
//                          logit x is computed once and kept in the caller's fp64 buffer for the later Newton steps), LDS, then lanes
//                          0 - 2 add the chunk's terms of one sum each in index order.
//   k_recal_final_sums   : one thread per sum adds the chunk partials in chunk order.
//   k_recal_reg_z        : one thread per (matched row, coordinate): z, its segment id, the invalid rows counted per workgroup (integer
//                          ballots), k_recal_invalid_total adds the workgroups' counts.
//   k_recal_group_keys, segsort, k_recal_seg_bounds, k_recal_gather : the values grouped by segment, stably (row order kept), the segment
//                          offsets by binary search in the sorted ids.
//   k_recal_seg_chunks, k_recal_seg_final : per segment the chunk partials of z^2 and their sum, in the order above.
//   k_recal_z_keys, segsort, k_recal_ece_obj, k_recal_ece_best : z sorted inside each segment; one thread per (segment, grid scale) makes
//                          the 14 counts by binary search and adds the 14 terms in order; one wavefront per segment takes the arg-min under
//                          the total order (objective, |j - j_one|, j), which no reduction order can change.
//   k_recal_apply        : 256 records per workgroup through LDS (coalesced loads and stores of the 6 + K + 16 floats), one thread per row.
// No atomics.  Every fp64 sum is added in an order the grid has no part in; only + - * / sqrt outside the temperature map.
#include "pod_device.h"
#include "pod_segsort.h"

namespace pod {

constexpr int RECAL_CHUNK = POD_RECAL_CHUNK;
constexpr int RECAL_WAVES = 4;
constexpr int RECAL_MAX_BLOCKS = 1024;
constexpr int RECAL_MAX_WIDTH = 6 + POD_MAX_CLASSES + 16;          // the widest record K7 writes
constexpr double RECAL_P_LO = 1.0 / 1073741824.0;                  // 2^-30

static size_t recal_align(size_t x) { return (x + 255) & ~(size_t)255; }

// x = logit(clamp(double(p), 2^-30, 1 - 2^-30)); a NaN stays a NaN
__device__ __forceinline__ double recal_logit(float p) {
    double c = (double)p;
    c = c < RECAL_P_LO ? RECAL_P_LO : c;
    c = c > 1.0 - RECAL_P_LO ? 1.0 - RECAL_P_LO : c;
    return log(c / (1.0 - c));
}

// e = exp(-|t|), s = sigmoid(t) without cancellation on either side
__device__ __forceinline__ double recal_sigmoid(double t, double& e) {
    e = exp(-fabs(t));
    const double d = 1.0 + e;
    return t >= 0.0 ? 1.0 / d : e / d;
}

// a chunk's terms are in term[0 .. m): one lane adds them in index order, starting from +0.0
__device__ __forceinline__ double recal_chunk_sum(const double* term, int m) {
    double a = 0.0;
    for (int i = 0; i < m; ++i) a += term[i];
    return a;
}

__global__ void __launch_bounds__(64 * RECAL_WAVES) k_recal_cls_chunks(const float* __restrict__ p, double* x, int x_ready,
                                                                         const uint8_t* __restrict__ y, int64_t n, double beta,
                                                                         int64_t n_chunks, double* partial) {
    __shared__ double term[RECAL_WAVES][3][RECAL_CHUNK];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int64_t c0 = (int64_t)blockIdx.x * RECAL_WAVES; c0 < n_chunks; c0 += (int64_t)gridDim.x * RECAL_WAVES) {   // (uniform over the workgroup)
        const int64_t c = c0 + wave;
        const bool live = c < n_chunks;
        const int64_t base = c * RECAL_CHUNK;
        const int m = live ? (int)min((int64_t)RECAL_CHUNK, n - base) : 0;
        for (int i = lane; i < m; i += 64) {
            double xi;
            if (x_ready) {
                xi = x[base + i];
            } else {
                xi = recal_logit(p[base + i]);
                if (x) x[base + i] = xi;
            }
            const double yi = (double)y[base + i];
            const double t = beta * xi;
            double e;
            const double s = recal_sigmoid(t, e);
            term[wave][0][i] = (fmax(t, 0.0) + log1p(e)) - yi * t;          // softplus(t) - y t
            term[wave][1][i] = (s - yi) * xi;
            term[wave][2][i] = (e / ((1.0 + e) * (1.0 + e))) * (xi * xi);    // s (1 - s) x^2
        }
        __syncthreads();
        if (live && lane < 3) partial[(int64_t)lane * n_chunks + c] = recal_chunk_sum(term[wave][lane], m);
        __syncthreads();
    }
}

__global__ void k_recal_final_sums(const double* partial, int64_t n_chunks, int n_sums, double* out) {
    const int j = threadIdx.x;
    if (blockIdx.x != 0 || j >= n_sums) return;
    double a = 0.0;
    for (int64_t c = 0; c < n_chunks; ++c) a += partial[(int64_t)j * n_chunks + c];
    out[j] = a;
}

__global__ void __launch_bounds__(256) k_recal_reg_z(const float* __restrict__ means, const float* __restrict__ cov,
                                                     const float* __restrict__ gt, const int32_t* __restrict__ det_class, int64_t n_values,
                                                     int per_class, int n_class, double* z, int32_t* seg, int32_t* blk_invalid) {
    __shared__ int cnt[4][4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int d = threadIdx.x & 3;                                          // the stride below is a multiple of 4: a thread keeps its coordinate
    int bad = 0;
    for (int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; v < n_values; v += (int64_t)gridDim.x * blockDim.x) {
        const int64_t i = v >> 2;
        const double var = (double)cov[i * 16 + 5 * d];
        const double r = (double)gt[v] - (double)means[v];
        const int c = per_class ? det_class[i] : 0;
        const bool ok = var > 0.0 && var < __longlong_as_double(0x7ff0000000000000ll) && fabs(r) < __longlong_as_double(0x7ff0000000000000ll)
                        && c >= 0 && c < n_class;
        z[v] = ok ? r / sqrt(var) : 0.0;
        seg[v] = ok ? 4 * c + d : -1;
        bad += ok ? 0 : 1;
    }
#pragma unroll
    for (int dd = 0; dd < 4; ++dd) {
        const int t = wave_sum(d == dd ? bad : 0);
        if (lane == 0) cnt[wave][dd] = t;
    }
    __syncthreads();
    if (threadIdx.x < 4) blk_invalid[blockIdx.x * 4 + threadIdx.x] = ((cnt[0][threadIdx.x] + cnt[1][threadIdx.x]) + cnt[2][threadIdx.x]) + cnt[3][threadIdx.x];
}

__global__ void k_recal_invalid_total(const int32_t* blk_invalid, int n_blocks, int64_t* invalid) {
    const int d = threadIdx.x;
    if (blockIdx.x != 0 || d >= 4) return;
    int64_t t = 0;
    for (int b = 0; b < n_blocks; ++b) t += blk_invalid[b * 4 + d];
    invalid[d] = t;
}

__global__ void __launch_bounds__(256) k_recal_group_keys(const int32_t* seg, int64_t n, int n_seg, uint64_t* key, int64_t* whole) {
    if (blockIdx.x == 0 && threadIdx.x < 2) whole[threadIdx.x] = threadIdx.x ? n : 0;      // one segment [0, n)
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int32_t s = seg[i];
        key[i] = (uint64_t)(s >= 0 && s < n_seg ? s : n_seg);                // left-out values behind every segment
    }
}

// seg_off[s] = the number of sorted ids below s, s <= n_seg
__global__ void k_recal_seg_bounds(const uint64_t* keys, int64_t n, int n_seg, int64_t* seg_off) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s > n_seg) return;
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (keys[mid] < (uint64_t)s) lo = mid + 1;
        else hi = mid;
    }
    seg_off[s] = lo;
}

__global__ void __launch_bounds__(256) k_recal_gather(const double* z, const int32_t* order, const int64_t* seg_off, int n_seg, int64_t n,
                                                      double* zg) {
    const int64_t live = seg_off[n_seg];
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        zg[i] = i < live ? z[order[i]] : 0.0;
}

// chunk c of segment s: its partial lives at seg_off[s] / 256 + s + c (distinct and in order over all segments)
__global__ void __launch_bounds__(64 * RECAL_WAVES) k_recal_seg_chunks(const double* __restrict__ zg, const int64_t* __restrict__ seg_off,
                                                                         double* partial) {
    __shared__ double term[RECAL_WAVES][RECAL_CHUNK];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int s = blockIdx.y;
    const int64_t s0 = seg_off[s], len = seg_off[s + 1] - s0;
    const int64_t n_chunks = (len + RECAL_CHUNK - 1) / RECAL_CHUNK, slot0 = s0 / RECAL_CHUNK + s;
    for (int64_t c0 = (int64_t)blockIdx.x * RECAL_WAVES; c0 < n_chunks; c0 += (int64_t)gridDim.x * RECAL_WAVES) {   // (uniform over the workgroup)
        const int64_t c = c0 + wave;
        const bool live = c < n_chunks;
        const int64_t base = c * RECAL_CHUNK;
        const int m = live ? (int)min((int64_t)RECAL_CHUNK, len - base) : 0;
        for (int i = lane; i < m; i += 64) {
            const double v = zg[s0 + base + i];
            term[wave][i] = v * v;
        }
        __syncthreads();
        if (live && lane == 0) partial[slot0 + c] = recal_chunk_sum(term[wave], m);
        __syncthreads();
    }
}

__global__ void k_recal_seg_final(const int64_t* seg_off, const double* partial, int n_seg, int64_t* count, double* sum) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n_seg) return;
    const int64_t s0 = seg_off[s], len = seg_off[s + 1] - s0;
    const int64_t n_chunks = (len + RECAL_CHUNK - 1) / RECAL_CHUNK, slot0 = s0 / RECAL_CHUNK + s;
    double a = 0.0;
    for (int64_t c = 0; c < n_chunks; ++c) a += partial[slot0 + c];
    count[s] = len;
    sum[s] = a;
}

__global__ void __launch_bounds__(256) k_recal_z_keys(const double* zg, int64_t n, uint64_t* key) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) key[i] = asc_key(zg[i]);
}

struct KRecalEce {
    const uint64_t* keys;          // z ascending inside each segment, as asc_key
    const int64_t* seg_off;
    const double* scales;          // [n_grid]
    const double* q;               // [n_q]
    int32_t n_seg, n_grid, n_q, j_one;
    double* obj;                   // [n_seg][n_grid]
    int32_t* best_j;
    double* best_obj;
    double* one_obj;
};

__global__ void __launch_bounds__(256) k_recal_ece_obj(const KRecalEce P) {
    const int s = blockIdx.y;
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= P.n_grid) return;
    const int64_t s0 = P.seg_off[s], m = P.seg_off[s + 1] - s0;
    double acc = 0.0;
    if (m > 0) {
        const double sj = P.scales[j], dm = (double)m, bins = (double)(P.n_q + 1);
        for (int i = 1; i <= P.n_q; ++i) {
            const double t = sj * P.q[i - 1];
            int64_t lo = 0, hi = m;                                          // the number of z < t
            while (lo < hi) {
                const int64_t mid = (lo + hi) >> 1;
                if (asc_key_value(P.keys[s0 + mid]) < t) lo = mid + 1;
                else hi = mid;
            }
            const double dlt = (double)lo / dm - (double)i / bins;
            acc += dlt * dlt;
        }
        acc = acc / (double)P.n_q;
    }
    P.obj[(int64_t)s * P.n_grid + j] = acc;
}

// (objective, |j - j_one|, j) ascending: a total order on the grid points of a segment
__device__ __forceinline__ bool recal_better(double oa, int ja, double ob, int jb, int j_one) {
    if (oa != ob) return oa < ob;
    const int da = ja > j_one ? ja - j_one : j_one - ja, db = jb > j_one ? jb - j_one : j_one - jb;
    return da != db ? da < db : ja < jb;
}

__global__ void __launch_bounds__(64) k_recal_ece_best(const KRecalEce P) {
    const int s = blockIdx.x, lane = threadIdx.x;
    const double* o = P.obj + (int64_t)s * P.n_grid;
    double bo = o[P.j_one];
    int bj = P.j_one;
    for (int j = lane; j < P.n_grid; j += 64)
        if (recal_better(o[j], j, bo, bj, P.j_one)) { bo = o[j]; bj = j; }
#pragma unroll
    for (int w = 32; w > 0; w >>= 1) {
        const double oo = __shfl_xor(bo, w, 64);
        const int oj = __shfl_xor(bj, w, 64);
        if (recal_better(oo, oj, bo, bj, P.j_one)) { bo = oo; bj = oj; }
    }
    if (lane == 0) {
        P.best_j[s] = bj;
        P.best_obj[s] = bo;
        P.one_obj[s] = o[P.j_one];
    }
}

struct KRecalApply {
    const float* rec;
    const int32_t* counts;
    float* out;
    const double* scales;          // [n_scale_rows][4]
    double beta;
    int64_t n_rows;
    int32_t max_det, K, W, n_scale_rows;
};

__device__ __forceinline__ float recal_temper(float p, double beta) {
    double e;
    return (float)recal_sigmoid(beta * recal_logit(p), e);
}

__global__ void __launch_bounds__(256) k_recal_apply(const KRecalApply P) {
    __shared__ float tile[256 * RECAL_MAX_WIDTH];
    const int W = P.W;
    const int64_t row0 = (int64_t)blockIdx.x * 256;
    const int rows = (int)min((int64_t)256, P.n_rows - row0);
    const float* src = P.rec + row0 * W;
    for (int k = threadIdx.x; k < rows * W; k += 256) tile[k] = src[k];
    __syncthreads();
    if ((int)threadIdx.x < rows) {
        const int64_t row = row0 + threadIdx.x;
        const int64_t img = row / P.max_det;
        const int slot = (int)(row - img * P.max_det);
        float* r = tile + threadIdx.x * W;
        if (slot >= P.counts[img]) {
            for (int k = 0; k < W; ++k) r[k] = 0.0f;                          // rows behind the count: zeros
        } else {
            if (P.beta != 1.0) {
                r[4] = recal_temper(r[4], P.beta);
                for (int k = 0; k < P.K; ++k) r[6 + k] = recal_temper(r[6 + k], P.beta);
            }
            int c = 0;
            if (P.n_scale_rows > 1) c = (int)r[5];
            double s0 = 1.0, s1 = 1.0, s2 = 1.0, s3 = 1.0;
            if (c >= 0 && c < P.n_scale_rows) {                               // a class without scales keeps its covariance
                s0 = P.scales[4 * c]; s1 = P.scales[4 * c + 1]; s2 = P.scales[4 * c + 2]; s3 = P.scales[4 * c + 3];
            }
            if (!(s0 == 1.0 && s1 == 1.0 && s2 == 1.0 && s3 == 1.0)) {
                // C' = M C M^T, M = T diag(s) T^-1 = [[s0,0,0,0],[0,s1,0,0],[s2-s0,0,s2,0],[0,s3-s1,0,s3]]: A = M C by rows, then A M^T by columns
                float* C = r + 6 + P.K;
                const double m20 = s2 - s0, m31 = s3 - s1;
                double A[4][4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const double c0 = (double)C[k], c1 = (double)C[4 + k], c2 = (double)C[8 + k], c3 = (double)C[12 + k];
                    A[0][k] = s0 * c0;
                    A[1][k] = s1 * c1;
                    A[2][k] = m20 * c0 + s2 * c2;
                    A[3][k] = m31 * c1 + s3 * c3;
                }
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    C[4 * k + 0] = (float)(A[k][0] * s0);
                    C[4 * k + 1] = (float)(A[k][1] * s1);
                    C[4 * k + 2] = (float)(A[k][0] * m20 + A[k][2] * s2);
                    C[4 * k + 3] = (float)(A[k][1] * m31 + A[k][3] * s3);
                }
            }
        }
    }
    __syncthreads();
    float* dst = P.out + row0 * W;
    for (int k = threadIdx.x; k < rows * W; k += 256) dst[k] = tile[k];
}

struct RecalWorkspace {
    uint64_t *key0, *key1;
    int32_t *idx0, *idx1;
    double* partial;
    int32_t* blk_invalid;
    int64_t* whole;
};

static size_t recal_partials(int64_t n, int32_t n_seg) { return 3 * (size_t)((n + RECAL_CHUNK - 1) / RECAL_CHUNK) + (size_t)n_seg + 3; }

static RecalWorkspace recal_carve(void* workspace, int64_t n, int32_t n_seg) {
    RecalWorkspace w;
    unsigned char* p = (unsigned char*)workspace;
    const size_t m = (size_t)n;
    w.key0 = (uint64_t*)p;
    w.key1 = (uint64_t*)(p += recal_align(8 * m));
    w.idx0 = (int32_t*)(p += recal_align(8 * m));
    w.idx1 = (int32_t*)(p += recal_align(4 * m));
    w.partial = (double*)(p += recal_align(4 * m));
    w.blk_invalid = (int32_t*)(p += recal_align(8 * recal_partials(n, n_seg)));
    w.whole = (int64_t*)(p + recal_align(16 * RECAL_MAX_BLOCKS));
    return w;
}

static unsigned recal_blocks(int64_t n, int per_block) {
    const int64_t b = (n + per_block - 1) / per_block;
    return (unsigned)(b < 1 ? 1 : b > RECAL_MAX_BLOCKS ? RECAL_MAX_BLOCKS : b);
}

static bool recal_sizes_ok(int64_t n, int32_t n_seg) { return n >= 0 && n <= 0x7fffffffll && n_seg >= 0 && n_seg <= POD_RECAL_MAX_SEGMENTS; }

}  // namespace pod

extern "C" size_t pod_recal_workspace_bytes(int64_t n, int32_t n_seg) {
    if (!pod::recal_sizes_ok(n, n_seg)) return 0;
    const size_t m = (size_t)n;
    return 2 * pod::recal_align(8 * m) + 2 * pod::recal_align(4 * m) + pod::recal_align(8 * pod::recal_partials(n, n_seg))
           + pod::recal_align(16 * pod::RECAL_MAX_BLOCKS) + pod::recal_align(16);
}

extern "C" int pod_recal_cls_sums(const float* p, const uint8_t* y, int64_t n, double beta, double* x, int32_t x_ready, void* workspace,
                                  double* sums, pod_stream_t stream) {
    if (!pod::recal_sizes_ok(n, 0) || !sums || !(beta == beta) || (x_ready && !x)) return POD_E_INVALID;
    if (n > 0 && (!y || !workspace || (!x_ready && !p))) return POD_E_INVALID;
    if (!pod_aligned(8, x, workspace, sums)) return POD_E_INVALID;
    const hipStream_t st = (hipStream_t)stream;
    const pod::RecalWorkspace w = pod::recal_carve(workspace, n, 0);
    const int64_t n_chunks = (n + pod::RECAL_CHUNK - 1) / pod::RECAL_CHUNK;
    if (n > 0) {
        hipLaunchKernelGGL(pod::k_recal_cls_chunks, dim3(pod::recal_blocks(n_chunks, pod::RECAL_WAVES)), dim3(64 * pod::RECAL_WAVES), 0, st,
                           p, x, (int)(x_ready != 0), y, n, beta, n_chunks, w.partial);
        POD_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(pod::k_recal_final_sums, dim3(1), dim3(64), 0, st, (const double*)w.partial, n_chunks, 3, sums);
    POD_CHECK_LAUNCH();
    return POD_OK;
}

extern "C" int pod_recal_reg_z(const float* means, const float* covs, const float* gt, const int32_t* det_class, int32_t n_matched,
                               int32_t n_class, void* workspace, double* z, int32_t* seg, int64_t* invalid, pod_stream_t stream) {
    if (n_matched < 0 || n_matched > 0x7fffffff / 4 || n_class < 0 || n_class > POD_MAX_CLASSES || !invalid) return POD_E_INVALID;
    if (n_matched > 0 && (!means || !covs || !gt || !z || !seg || !workspace || (n_class > 0 && !det_class))) return POD_E_INVALID;
    if (!pod_aligned(8, z, workspace, invalid)) return POD_E_INVALID;
    const hipStream_t st = (hipStream_t)stream;
    const int64_t n = 4 * (int64_t)n_matched;
    const unsigned blocks = n ? pod::recal_blocks(n, 256) : 0;
    const pod::RecalWorkspace w = pod::recal_carve(workspace, n, 0);
    if (n > 0) {
        hipLaunchKernelGGL(pod::k_recal_reg_z, dim3(blocks), dim3(256), 0, st, means, covs, gt, det_class, n, (int)(n_class > 0),
                           n_class > 0 ? n_class : 1, z, seg, w.blk_invalid);
        POD_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(pod::k_recal_invalid_total, dim3(1), dim3(64), 0, st, (const int32_t*)w.blk_invalid, (int)blocks, invalid);
    POD_CHECK_LAUNCH();
    return POD_OK;
}

extern "C" int pod_recal_moment(const double* z, const int32_t* seg, int64_t n, int32_t n_seg, void* workspace, double* zg, int64_t* seg_off,
                                int64_t* count, double* sum, pod_stream_t stream) {
    if (!pod::recal_sizes_ok(n, n_seg) || n_seg < 1 || !seg_off || !count || !sum) return POD_E_INVALID;
    if (n > 0 && (!z || !seg || !zg || !workspace)) return POD_E_INVALID;
    if (!pod_aligned(8, z, zg, workspace, seg_off, count, sum)) return POD_E_INVALID;
    const hipStream_t st = (hipStream_t)stream;
    if (n == 0) {
        if (hipMemsetAsync(seg_off, 0, sizeof(int64_t) * ((size_t)n_seg + 1), st) != hipSuccess) return POD_E_LAUNCH;
    } else {
        const pod::RecalWorkspace w = pod::recal_carve(workspace, n, n_seg);
        const unsigned blocks = pod::recal_blocks(n, 256);
        hipLaunchKernelGGL(pod::k_recal_group_keys, dim3(blocks), dim3(256), 0, st, seg, n, n_seg, w.key0, w.whole);
        POD_CHECK_LAUNCH();
        uint64_t* keys;
        int32_t* order;
        if (pod::segsort(w.whole, 1, (int32_t)n, nullptr, w.key0, w.idx0, w.key1, w.idx1, &keys, &order, st) != POD_OK) return POD_E_LAUNCH;
        hipLaunchKernelGGL(pod::k_recal_seg_bounds, dim3((n_seg + 1 + 63) / 64), dim3(64), 0, st, (const uint64_t*)keys, n, n_seg, seg_off);
        POD_CHECK_LAUNCH();
        hipLaunchKernelGGL(pod::k_recal_gather, dim3(blocks), dim3(256), 0, st, z, (const int32_t*)order, (const int64_t*)seg_off, n_seg, n, zg);
        POD_CHECK_LAUNCH();
        const unsigned gx = pod::recal_blocks((n + pod::RECAL_CHUNK - 1) / pod::RECAL_CHUNK, pod::RECAL_WAVES);
        hipLaunchKernelGGL(pod::k_recal_seg_chunks, dim3(gx < 256 ? gx : 256, n_seg), dim3(64 * pod::RECAL_WAVES), 0, st, (const double*)zg,
                           (const int64_t*)seg_off, w.partial);
        POD_CHECK_LAUNCH();
        hipLaunchKernelGGL(pod::k_recal_seg_final, dim3((n_seg + 63) / 64), dim3(64), 0, st, (const int64_t*)seg_off, (const double*)w.partial,
                           n_seg, count, sum);
        POD_CHECK_LAUNCH();
        return POD_OK;
    }
    hipLaunchKernelGGL(pod::k_recal_seg_final, dim3((n_seg + 63) / 64), dim3(64), 0, st, (const int64_t*)seg_off, (const double*)nullptr, n_seg,
                       count, sum);
    POD_CHECK_LAUNCH();
    return POD_OK;
}

extern "C" int pod_recal_ece_grid(const double* zg, const int64_t* seg_off, int64_t n, int32_t n_seg, int32_t max_seg, const double* scales,
                                  int32_t n_grid, int32_t j_one, const double* q, int32_t n_q, void* workspace, double* obj, int32_t* best_j,
                                  double* best_obj, double* one_obj, pod_stream_t stream) {
    if (!pod::recal_sizes_ok(n, n_seg) || n_seg < 1 || max_seg < 0 || max_seg > n || n_grid < 1 || n_grid > POD_RECAL_MAX_GRID || j_one < 0
        || j_one >= n_grid || n_q < 1 || n_q > POD_RECAL_MAX_QUANTILES)
        return POD_E_INVALID;
    if (!seg_off || !scales || !q || !obj || !best_j || !best_obj || !one_obj || (n > 0 && (!zg || !workspace))) return POD_E_INVALID;
    if (!pod_aligned(8, zg, seg_off, scales, q, workspace, obj, best_obj, one_obj)) return POD_E_INVALID;
    const hipStream_t st = (hipStream_t)stream;
    pod::KRecalEce P;
    P.keys = nullptr; P.seg_off = seg_off; P.scales = scales; P.q = q; P.n_seg = n_seg; P.n_grid = n_grid; P.n_q = n_q; P.j_one = j_one;
    P.obj = obj; P.best_j = best_j; P.best_obj = best_obj; P.one_obj = one_obj;
    if (n > 0) {
        const pod::RecalWorkspace w = pod::recal_carve(workspace, n, n_seg);
        hipLaunchKernelGGL(pod::k_recal_z_keys, dim3(pod::recal_blocks(n, 256)), dim3(256), 0, st, zg, n, w.key0);
        POD_CHECK_LAUNCH();
        uint64_t* keys;
        int32_t* order;
        if (pod::segsort(seg_off, n_seg, max_seg, nullptr, w.key0, w.idx0, w.key1, w.idx1, &keys, &order, st) != POD_OK) return POD_E_LAUNCH;
        P.keys = keys;
    }
    hipLaunchKernelGGL(pod::k_recal_ece_obj, dim3((n_grid + 255) / 256, n_seg), dim3(256), 0, st, P);
    POD_CHECK_LAUNCH();
    hipLaunchKernelGGL(pod::k_recal_ece_best, dim3(n_seg), dim3(64), 0, st, P);
    POD_CHECK_LAUNCH();
    return POD_OK;
}

extern "C" int pod_recal_apply(const float* records, const int32_t* counts, int32_t n_images, int32_t max_det, int32_t num_classes, double beta,
                               const double* scales, int32_t n_scale_rows, float* out, pod_stream_t stream) {
    if (n_images < 0 || max_det < 1 || num_classes < 1 || 6 + num_classes + 16 > pod::RECAL_MAX_WIDTH || !(beta > 0.0) || !(beta < 1e300)
        || n_scale_rows < 1 || n_scale_rows > POD_MAX_CLASSES || !scales)
        return POD_E_INVALID;
    const int64_t n_rows = (int64_t)n_images * max_det;
    if (n_rows > 0x7fffffffll) return POD_E_INVALID;
    if (n_rows > 0 && (!records || !counts || !out || records == out)) return POD_E_INVALID;
    if (!pod_aligned(8, scales) || !pod_aligned(4, records, out, counts)) return POD_E_INVALID;
    if (n_rows == 0) return POD_OK;
    pod::KRecalApply P;
    P.rec = records; P.counts = counts; P.out = out; P.scales = scales; P.beta = beta; P.n_rows = n_rows; P.max_det = max_det;
    P.K = num_classes; P.W = 6 + num_classes + 16; P.n_scale_rows = n_scale_rows;
    hipLaunchKernelGGL(pod::k_recal_apply, dim3((unsigned)((n_rows + 255) / 256)), dim3(256), 0, (hipStream_t)stream, P);
    POD_CHECK_LAUNCH();
    return POD_OK;
}
