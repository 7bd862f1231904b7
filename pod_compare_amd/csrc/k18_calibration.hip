// The calibration pass of the offline calibration errors (compute_calibration_errors.py `calibration_errors`, CE:86-297).
//
//   k_calib_keys        : one thread per row -- the classification entropy -log(max p) (CE:166-167), the entropy of
//                         MVN(0, cov + 1e-4 I) through a 4x4 Cholesky in registers (CE:263-276, torch's 0.5 D (1 + log 2 pi) + sum log diag L),
//                         the row's class and the per-class row counts (LDS, then one integer add per class).
//   k_calib_reg_counts  : the Normal cdf of every matched coordinate (CE:206-261), binned against the 14 edges in LDS, one integer add
//                         per bin and workgroup.
//   k_calib_class_keys, k_calib_gather, segsort, k_calib_min_err : the minimum-uncertainty errors (CE:160-178, CE:279-292).  The rows
//                         are grouped by class (a stable sort on the class), each (class, key) segment gathered through the host's
//                         randperm, sorted stably by key (pod_segsort.h: K17's tile sort + merge passes), and one workgroup per segment
//                         scans the true-positive flags and takes the NaN-propagating min of the fp64 errors.
//   k_calib_score_keys, segsort, k_calib_sorted, k_calib_bin_count, k_calib_bin_starts, k_calib_bin_terms, k_calib_bin_total : the
//                         marginal calibration error (CE:117-136, marginal_calibration_error): sorted scores, bin starts (distinct
//                         values or searchsorted bins), per-bin fp64 sums, the debiased terms added in bin order by one thread.
#include "pod_device.h"
#include "pod_segsort.h"

namespace pod {

constexpr int CAL_BLOCK = POD_CALIB_BLOCK;
constexpr int CAL_BINS = POD_CALIB_MAX_EDGES + 1;

__device__ inline double nan_min(double a, double b) { return (a != a || b != b) ? __longlong_as_double(0x7ff8000000000000ll) : fmin(a, b); }

// inclusive block scan of ints (blockDim.x a multiple of 64, <= 1024); total: the block's sum
__device__ inline int block_scan(int v, int* lds, int& total) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, nw = blockDim.x >> 6;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(v, o, 64);
        if (lane >= o) v += t;
    }
    if (lane == 63) lds[wid] = v;
    __syncthreads();
    int off = 0;
    total = 0;
    for (int w = 0; w < nw; ++w) {
        const int t = lds[w];
        off += w < wid ? t : 0;
        total += t;
    }
    __syncthreads();
    return v + off;
}

__global__ void __launch_bounds__(256) k_calib_keys(const float* __restrict__ probs, int k1, const float* __restrict__ cov,
                                                    const int32_t* __restrict__ gt_class, int n_matched, int n, float* cls_ent,
                                                    float* reg_ent, int32_t* det_class, int32_t* class_count) {
    __shared__ int cnt[POD_MAX_CLASSES];
    if (threadIdx.x < POD_MAX_CLASSES) cnt[threadIdx.x] = 0;
    __syncthreads();
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        const float* p = probs + (int64_t)i * k1;
        float best = p[0];
        int arg = 0;
        for (int j = 1; j < k1 - 1; ++j) {                                  // torch.max: the first maximum, NaN wins
            const float v = p[j];
            if (best == best && (v != v || v > best)) { best = v; arg = j; }
        }
        cls_ent[i] = -logf(best);
        const float* a = cov + (int64_t)i * 16;
        const float e = 1e-4f;                                              // cov + 1e-4 * eye(4), then torch.linalg.cholesky
        const float a00 = a[0] + e, a11 = a[5] + e, a22 = a[10] + e, a33 = a[15] + e;
        const float l00 = sqrtf(a00);
        const float l10 = a[4] / l00, l20 = a[8] / l00, l30 = a[12] / l00;
        const float l11 = sqrtf(a11 - l10 * l10);
        const float l21 = (a[9] - l20 * l10) / l11, l31 = (a[13] - l30 * l10) / l11;
        const float l22 = sqrtf(a22 - (l20 * l20 + l21 * l21));
        const float l32 = (a[14] - (l30 * l20 + l31 * l21)) / l22;
        const float l33 = sqrtf(a33 - ((l30 * l30 + l31 * l31) + l32 * l32));
        const float half_log_det = ((logf(l00) + logf(l11)) + logf(l22)) + logf(l33);
        reg_ent[i] = 5.675754132818691f + half_log_det;                   // 0.5 * 4 * (1 + log(2 pi))
        const int c = i < n_matched ? gt_class[i] : arg;
        det_class[i] = c;
        if (c >= 0 && c < POD_MAX_CLASSES) atomicAdd(&cnt[c], 1);
    }
    __syncthreads();
    if (threadIdx.x < POD_MAX_CLASSES && cnt[threadIdx.x]) atomicAdd(&class_count[threadIdx.x], cnt[threadIdx.x]);
}

struct KCalibEdges {
    float e[POD_CALIB_MAX_EDGES];
};

__global__ void __launch_bounds__(256) k_calib_reg_counts(const float* __restrict__ means, const float* __restrict__ cov,
                                                          const float* __restrict__ gt, const int32_t* __restrict__ det_class,
                                                          int n_matched, KCalibEdges E, int n_edges, int32_t* counts) {
    __shared__ int hist[POD_MAX_CLASSES * 4 * CAL_BINS];
    const int nb = n_edges + 1;
    for (int j = threadIdx.x; j < POD_MAX_CLASSES * 4 * nb; j += blockDim.x) hist[j] = 0;
    __syncthreads();
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n_matched; i += gridDim.x * blockDim.x) {
        const int c = det_class[i];
        if (c < 0 || c >= POD_MAX_CLASSES) continue;
        for (int d = 0; d < 4; ++d) {
            const float scale = sqrtf(cov[(int64_t)i * 16 + 5 * d]);
            // torch Normal.cdf: 0.5 * (1 + erf((value - loc) * scale.reciprocal() / sqrt(2)))
            const float z = ((gt[(int64_t)i * 4 + d] - means[(int64_t)i * 4 + d]) * (1.0f / scale)) / 1.41421356237309515f;
            const float cdf = 0.5f * (1.0f + erff(z));
            int b = 0;
            while (b < n_edges && !(cdf < E.e[b])) ++b;
            atomicAdd(&hist[(c * 4 + d) * nb + b], 1);
        }
    }
    __syncthreads();
    for (int j = threadIdx.x; j < POD_MAX_CLASSES * 4 * nb; j += blockDim.x)
        if (hist[j]) atomicAdd(&counts[j], hist[j]);
}

__global__ void __launch_bounds__(256) k_calib_class_keys(const int32_t* det_class, int n, uint64_t* key, int32_t* idx, int64_t* seg) {
    if (blockIdx.x == 0 && threadIdx.x < 2) seg[threadIdx.x] = threadIdx.x ? n : 0;      // one segment [0, n)
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        key[i] = (uint64_t)(uint32_t)det_class[i];
        idx[i] = i;
    }
}

struct KCalibGather {
    const float* cls_ent;
    const float* reg_ent;
    const int32_t* grouped;        // rows in (class, row) order
    const int32_t* class_off;
    const int64_t* seg_off;
    const int32_t* seg_class;
    const int64_t* perm;
    int32_t n_tp;
    uint64_t* key;
    unsigned char* is_tp;
};

// segment blockIdx.y, position q: member perm[q] of the class -> its key and true-positive flag (torch: entropy[perm], is_tp[perm])
__global__ void __launch_bounds__(256) k_calib_gather(const KCalibGather P) {
    const int s = blockIdx.y;
    const int64_t s0 = P.seg_off[s];
    const int64_t n = P.seg_off[s + 1] - s0;
    const int sc = P.seg_class[s];
    const float* ent = (sc & 1) ? P.reg_ent : P.cls_ent;
    const int32_t base = P.class_off[sc >> 1];
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < n; q += (int64_t)gridDim.x * blockDim.x) {
        const int32_t row = P.grouped[base + P.perm[s0 + q]];
        P.key[s0 + q] = asc_key((double)ent[row]);
        P.is_tp[s0 + q] = row < P.n_tp;
    }
}

__global__ void __launch_bounds__(1024) k_calib_min_err(const int64_t* seg_off, const int32_t* order, const unsigned char* is_tp,
                                                        double* min_err) {
    __shared__ int lds[16];
    __shared__ double red[16];
    const int s = blockIdx.x;
    const int64_t s0 = seg_off[s];
    const int n = (int)(seg_off[s + 1] - s0);
    int t = 0;
    for (int p = threadIdx.x; p < n; p += blockDim.x) t += is_tp[order[s0 + p]];
    int T;
    block_scan(t, lds, T);
    const double dT = (double)T, dF = (double)(n - T);
    double m = __longlong_as_double(0x7ff0000000000000ll);
    int carry = 0;
    for (int b0 = 0; b0 < n; b0 += blockDim.x) {
        const int p = b0 + threadIdx.x;
        const int f = p < n ? is_tp[order[s0 + p]] : 0;
        int tot;
        const int cum_tp = carry + block_scan(f, lds, tot);
        carry += tot;
        if (p < n) {
            const double a = 0.5 * (dT - (double)cum_tp) / dT;
            const double b = 0.5 * (double)(p + 1 - cum_tp) / dF;
            m = nan_min(m, a + b);
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = nan_min(m, __shfl_xor(m, o, 64));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        double r = red[0];
        for (int w = 1; w < (int)(blockDim.x >> 6); ++w) r = nan_min(r, red[w]);
        min_err[s] = n > 0 ? r : __longlong_as_double(0x7ff8000000000000ll);
    }
}

__global__ void __launch_bounds__(256) k_calib_score_keys(const float* scores, int n, uint64_t* key, int64_t* seg) {
    if (blockIdx.x == 0 && threadIdx.x < 2) seg[threadIdx.x] = threadIdx.x ? n : 0;      // one segment [0, n)
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) key[i] = asc_key((double)scores[i]);
}

__global__ void __launch_bounds__(256) k_calib_sorted(const float* scores, const int32_t* order, int n, double* sorted) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) sorted[i] = (double)scores[order[i]];
}

struct KCalibBins {
    const double* sorted;
    const int32_t* order;
    const int64_t* labels;
    int32_t n;
    int32_t n_edges;               // 0: one bin per distinct value
    double e[POD_CALIB_MAX_EDGES];
    const int64_t* blk_off;
    int32_t* blk_cnt;
    int32_t* starts;               // [n_bins + 1]
    double* terms;                 // [n_bins]
    int32_t n_bins;
    double* total;
};

// searchsorted(edges, v, 'left') = number of edges below v
__device__ inline int calib_bin(const KCalibBins& P, double v) {
    int b = 0;
    while (b < P.n_edges && P.e[b] < v) ++b;
    return b;
}

__device__ inline int calib_flag(const KCalibBins& P, int i) {
    if (i == 0) return 1;
    if (i >= P.n) return 0;
    const double a = P.sorted[i - 1], b = P.sorted[i];
    return P.n_edges ? (calib_bin(P, a) != calib_bin(P, b)) : (a != b);
}

__global__ void __launch_bounds__(CAL_BLOCK) k_calib_bin_count(const KCalibBins P) {
    __shared__ int lds[16];
    int tot;
    block_scan(calib_flag(P, blockIdx.x * CAL_BLOCK + threadIdx.x), lds, tot);
    if (threadIdx.x == 0) P.blk_cnt[blockIdx.x] = tot;
}

__global__ void __launch_bounds__(CAL_BLOCK) k_calib_bin_starts(const KCalibBins P) {
    __shared__ int lds[16];
    const int i = blockIdx.x * CAL_BLOCK + threadIdx.x;
    const int f = calib_flag(P, i);
    int tot;
    const int r = block_scan(f, lds, tot) - f;
    if (f) P.starts[P.blk_off[blockIdx.x] + r] = i;
    if (i == 0) P.starts[P.n_bins] = P.n;
}

// one workgroup per bin (grid-stride): fp64 sums of labels and scores in a fixed order, then the bin's debiased term
__global__ void __launch_bounds__(256) k_calib_bin_terms(const KCalibBins P) {
    __shared__ double rs[4], rl[4];
    for (int b = blockIdx.x; b < P.n_bins; b += gridDim.x) {
        const int lo = P.starts[b], hi = P.starts[b + 1], cnt = hi - lo;
        const bool skip = cnt < 2 || (P.n_edges ? calib_bin(P, P.sorted[lo]) >= P.n_edges : !(P.sorted[lo] <= 1.0));
        if (skip) {                                                           // (uniform over the workgroup)
            if (threadIdx.x == 0) P.terms[b] = 0.0;
            continue;
        }
        double s = 0.0, l = 0.0;
        for (int i = lo + threadIdx.x; i < hi; i += blockDim.x) {
            s += P.sorted[i];
            l += (double)P.labels[P.order[i]];
        }
        s = wave_sum(s);
        l = wave_sum(l);
        if ((threadIdx.x & 63) == 0) { rs[threadIdx.x >> 6] = s; rl[threadIdx.x >> 6] = l; }
        __syncthreads();
        if (threadIdx.x == 0) {
            const double S = ((rs[0] + rs[1]) + rs[2]) + rs[3], L = ((rl[0] + rl[1]) + rl[2]) + rl[3];
            const double n = (double)cnt, ml = L / n, mp = S / n;
            const double err = (ml - mp) * (ml - mp) - ml * (1.0 - ml) / (n - 1.0);
            P.terms[b] = n / (double)P.n * err;
        }
        __syncthreads();
    }
}

__global__ void k_calib_bin_total(const KCalibBins P) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    double t = 0.0;
    for (int b = 0; b < P.n_bins; ++b) t += P.terms[b];                   // bin order, as the host loop adds them
    P.total[0] = t;
}

static size_t calib_align(size_t x) { return (x + 255) & ~(size_t)255; }

}  // namespace pod

extern "C" int pod_calib_keys(const float* cls_probs, int32_t k1, const float* cov, const int32_t* gt_class, int32_t n_matched, int32_t n,
                              float* cls_entropy, float* reg_entropy, int32_t* det_class, int32_t* class_count, pod_stream_t stream) {
    if (n < 0 || n_matched < 0 || n_matched > n || k1 < 2 || !class_count) return POD_E_INVALID;
    if (n > 0 && (!cls_probs || !cov || !cls_entropy || !reg_entropy || !det_class || (n_matched > 0 && !gt_class))) return POD_E_INVALID;
    const hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(class_count, 0, sizeof(int32_t) * POD_MAX_CLASSES, st) != hipSuccess) return POD_E_LAUNCH;
    if (n == 0) return POD_OK;
    hipLaunchKernelGGL(pod::k_calib_keys, dim3((n + 255) / 256), dim3(256), 0, st, cls_probs, k1, cov, gt_class, n_matched, n,
                       cls_entropy, reg_entropy, det_class, class_count);
    POD_CHECK_LAUNCH();
    return POD_OK;
}

extern "C" int pod_calib_reg_counts(const float* means, const float* cov, const float* gt, const int32_t* det_class, int32_t n_matched,
                                    const float* edges, int32_t n_edges, int32_t* counts, pod_stream_t stream) {
    if (n_matched < 0 || n_edges < 1 || n_edges > POD_CALIB_MAX_EDGES || !edges || !counts) return POD_E_INVALID;
    if (n_matched > 0 && (!means || !cov || !gt || !det_class)) return POD_E_INVALID;
    const hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(counts, 0, sizeof(int32_t) * POD_MAX_CLASSES * 4 * (n_edges + 1), st) != hipSuccess) return POD_E_LAUNCH;
    if (n_matched == 0) return POD_OK;
    pod::KCalibEdges E;
    for (int j = 0; j < POD_CALIB_MAX_EDGES; ++j) E.e[j] = j < n_edges ? edges[j] : 0.0f;
    const int blocks = (n_matched + 255) / 256;
    hipLaunchKernelGGL(pod::k_calib_reg_counts, dim3(blocks < 1024 ? blocks : 1024), dim3(256), 0, st, means, cov, gt, det_class,
                       n_matched, E, n_edges, counts);
    POD_CHECK_LAUNCH();
    return POD_OK;
}

extern "C" size_t pod_calib_min_uncertainty_workspace_bytes(int32_t n, int64_t n_pos) {
    if (n < 0 || n_pos < 0) return 0;
    const size_t m = (size_t)(n > n_pos ? n : n_pos);
    return 2 * pod::calib_align(8 * m) + 2 * pod::calib_align(4 * m) + pod::calib_align(4 * (size_t)n) + pod::calib_align((size_t)n_pos)
           + pod::calib_align(16);
}

extern "C" int pod_calib_min_uncertainty(const float* cls_entropy, const float* reg_entropy, const int32_t* det_class, int32_t n, int32_t n_tp,
                                         const int32_t* class_off, const int64_t* seg_off, const int32_t* seg_class, int32_t n_seg,
                                         int32_t max_seg, int64_t n_pos, const int64_t* perm, void* workspace, double* min_err,
                                         pod_stream_t stream) {
    if (n < 0 || n_tp < 0 || n_tp > n || n_seg < 0 || max_seg < 0 || max_seg > n || n_pos < 0 || n_pos > 2 * (int64_t)n) return POD_E_INVALID;
    if (n_seg == 0) return POD_OK;
    if (!seg_off || !seg_class || !min_err || (max_seg > 0 && (!class_off || !cls_entropy || !reg_entropy || !det_class || !perm || !workspace)))
        return POD_E_INVALID;
    const hipStream_t st = (hipStream_t)stream;
    if (max_seg == 0) {                                                      // every segment empty: NaN
        hipLaunchKernelGGL(pod::k_calib_min_err, dim3(n_seg), dim3(1024), 0, st, seg_off, (const int32_t*)nullptr,
                           (const unsigned char*)nullptr, min_err);
        POD_CHECK_LAUNCH();
        return POD_OK;
    }
    const size_t m = (size_t)(n > n_pos ? n : n_pos);
    unsigned char* ws = (unsigned char*)workspace;
    uint64_t* key0 = (uint64_t*)ws;
    uint64_t* key1 = (uint64_t*)(ws += pod::calib_align(8 * m));
    int32_t* idx0 = (int32_t*)(ws += pod::calib_align(8 * m));
    int32_t* idx1 = (int32_t*)(ws += pod::calib_align(4 * m));
    int32_t* grouped = (int32_t*)(ws += pod::calib_align(4 * m));
    unsigned char* is_tp = (unsigned char*)(ws += pod::calib_align(4 * (size_t)n));
    int64_t* whole = (int64_t*)(ws + pod::calib_align((size_t)n_pos));
    uint64_t* keys;
    int32_t* order;
    // rows grouped by class, stably (one segment [0, n)), then the (class, key) segments
    const int blocks = (n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096;
    hipLaunchKernelGGL(pod::k_calib_class_keys, dim3(blocks), dim3(256), 0, st, det_class, n, key0, idx0, whole);
    POD_CHECK_LAUNCH();
    if (pod::segsort(whole, 1, n, nullptr, key0, idx0, key1, idx1, &keys, &order, st) != POD_OK) return POD_E_LAUNCH;
    if (hipMemcpyAsync(grouped, order, sizeof(int32_t) * n, hipMemcpyDeviceToDevice, st) != hipSuccess) return POD_E_LAUNCH;
    pod::KCalibGather G;
    G.cls_ent = cls_entropy; G.reg_ent = reg_entropy; G.grouped = grouped; G.class_off = class_off; G.seg_off = seg_off;
    G.seg_class = seg_class; G.perm = perm; G.n_tp = n_tp; G.key = key0; G.is_tp = is_tp;
    const int gx = (max_seg + 255) / 256;
    hipLaunchKernelGGL(pod::k_calib_gather, dim3(gx < 1024 ? gx : 1024, n_seg), dim3(256), 0, st, G);
    POD_CHECK_LAUNCH();
    if (pod::segsort(seg_off, n_seg, max_seg, nullptr, key0, idx0, key1, idx1, &keys, &order, st) != POD_OK) return POD_E_LAUNCH;
    hipLaunchKernelGGL(pod::k_calib_min_err, dim3(n_seg), dim3(1024), 0, st, seg_off, order, is_tp, min_err);
    POD_CHECK_LAUNCH();
    return POD_OK;
}

extern "C" size_t pod_calib_marginal_sort_workspace_bytes(int32_t n) {
    if (n <= 0) return 0;
    const size_t m = (size_t)n;
    return 2 * pod::calib_align(8 * m) + 2 * pod::calib_align(4 * m) + pod::calib_align(16);
}

extern "C" int pod_calib_marginal_sort(const float* scores, int32_t n, void* workspace, double* sorted, int32_t* order, pod_stream_t stream) {
    if (n < 0) return POD_E_INVALID;
    if (n == 0) return POD_OK;
    if (!scores || !workspace || !sorted || !order) return POD_E_INVALID;
    const hipStream_t st = (hipStream_t)stream;
    const size_t m = (size_t)n;
    unsigned char* ws = (unsigned char*)workspace;
    uint64_t* key0 = (uint64_t*)ws;
    uint64_t* key1 = (uint64_t*)(ws += pod::calib_align(8 * m));
    int32_t* idx0 = (int32_t*)(ws += pod::calib_align(8 * m));
    int32_t* idx1 = (int32_t*)(ws += pod::calib_align(4 * m));
    int64_t* seg = (int64_t*)(ws += pod::calib_align(4 * m));
    const int blocks = (n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096;
    hipLaunchKernelGGL(pod::k_calib_score_keys, dim3(blocks), dim3(256), 0, st, scores, n, key0, seg);
    POD_CHECK_LAUNCH();
    uint64_t* keys;
    int32_t* ord;
    if (pod::segsort(seg, 1, n, nullptr, key0, idx0, key1, idx1, &keys, &ord, st) != POD_OK) return POD_E_LAUNCH;
    if (hipMemcpyAsync(order, ord, sizeof(int32_t) * m, hipMemcpyDeviceToDevice, st) != hipSuccess) return POD_E_LAUNCH;
    hipLaunchKernelGGL(pod::k_calib_sorted, dim3(blocks), dim3(256), 0, st, scores, ord, n, sorted);
    POD_CHECK_LAUNCH();
    return POD_OK;
}

static bool calib_bins_args(pod::KCalibBins& P, const double* sorted, int32_t n, const double* edges, int32_t n_edges) {
    if (n < 0 || n_edges < 0 || n_edges > POD_CALIB_MAX_EDGES || (n_edges > 0 && !edges) || (n > 0 && !sorted)) return false;
    P = pod::KCalibBins{};
    P.sorted = sorted; P.n = n; P.n_edges = n_edges;
    for (int j = 0; j < n_edges; ++j) P.e[j] = edges[j];
    return true;
}

extern "C" int pod_calib_marginal_bins(const double* sorted, int32_t n, const double* edges, int32_t n_edges, int32_t* blk_cnt,
                                       pod_stream_t stream) {
    pod::KCalibBins P;
    if (!calib_bins_args(P, sorted, n, edges, n_edges) || (n > 0 && !blk_cnt)) return POD_E_INVALID;
    if (n == 0) return POD_OK;
    P.blk_cnt = blk_cnt;
    hipLaunchKernelGGL(pod::k_calib_bin_count, dim3((n + pod::CAL_BLOCK - 1) / pod::CAL_BLOCK), dim3(pod::CAL_BLOCK), 0, (hipStream_t)stream, P);
    POD_CHECK_LAUNCH();
    return POD_OK;
}

extern "C" size_t pod_calib_marginal_error_workspace_bytes(int32_t n_bins) {
    if (n_bins < 0) return 0;
    return pod::calib_align(4 * ((size_t)n_bins + 1)) + pod::calib_align(8 * (size_t)n_bins);
}

extern "C" int pod_calib_marginal_error(const double* sorted, const int32_t* order, const int64_t* labels, int32_t n, const double* edges,
                                        int32_t n_edges, const int64_t* blk_off, int32_t n_bins, void* workspace, double* total,
                                        pod_stream_t stream) {
    pod::KCalibBins P;
    if (!calib_bins_args(P, sorted, n, edges, n_edges) || !total || n_bins < 0 || n_bins > n) return POD_E_INVALID;
    if (n > 0 && (!order || !labels || !blk_off || !workspace || n_bins < 1)) return POD_E_INVALID;
    const hipStream_t st = (hipStream_t)stream;
    P.order = order; P.labels = labels; P.blk_off = blk_off; P.n_bins = n_bins; P.total = total;
    unsigned char* ws = (unsigned char*)workspace;
    P.starts = (int32_t*)ws;
    P.terms = (double*)(ws + pod::calib_align(4 * ((size_t)n_bins + 1)));
    if (n > 0) {
        hipLaunchKernelGGL(pod::k_calib_bin_starts, dim3((n + pod::CAL_BLOCK - 1) / pod::CAL_BLOCK), dim3(pod::CAL_BLOCK), 0, st, P);
        POD_CHECK_LAUNCH();
        hipLaunchKernelGGL(pod::k_calib_bin_terms, dim3(n_bins < 4096 ? n_bins : 4096), dim3(256), 0, st, P);
        POD_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(pod::k_calib_bin_total, dim3(1), dim3(64), 0, st, P);
    POD_CHECK_LAUNCH();
    return POD_OK;
}
