// COCO bbox evaluation (pycocotools COCOeval, iouType 'bbox', default Params) for the offline average precision.
//
// Replaces: COCOeval.evaluate -> evaluateImg (a Python loop over image x category x area range with a serial greedy match
// inside) and COCOeval.accumulate (a Python loop over category x area x maxDets x IoU threshold), the two loops behind
// compute_average_precision.py:41-43 ("AP").  fp64 throughout, as numpy computes; the host generates iouThrs / recThrs.
//
//   k_coco_eval_images : one workgroup per (image, category) pair with a ground-truth box or a detection.  Detections ranked by
//                        score (descending, stable = pycocotools' mergesort) and cut at maxDets[-1]; the (kept x G) IoU matrix of
//                        maskUtils.iou in LDS (in caller scratch when G > POD_COCO_LDS_GT); then the T x A greedy matches, one
//                        lane each, run the evaluateImg loop as written.  Matches are ground-truth IDS: a match to id 0 reads as
//                        "unmatched" to the area-range test and to accumulate, as it does in pycocotools.
//   k_coco_sort_tiles  : per category, 1024-element tiles of the kept detections sorted in LDS (bitonic) by (score desc, position).
//   k_coco_merge       : merge passes of sorted runs (each element's output slot by binary search in the partner run).
//                        The two are the library's stable segmented sort (pod_segsort.h: K18 sorts its own keys with them).
//   k_coco_gather      : the kept arrays in that order.  Position = (image position in sorted imgIds, rank), so the order is the
//                        one argsort(-concatenated scores, kind='mergesort') gives.
//   k_coco_accumulate  : one workgroup per (category, area, maxDet, IoU threshold): prefix counts of tp / fp, rc, pr, the
//                        right-to-left precision envelope and searchsorted(rc, recThrs, 'left') cut at nd -- without storing rc or
//                        pr: element i lies at or after searchsorted index j iff recThrs[j] <= rc[i], so the envelope at j is the
//                        max of pr over the "buckets" >= j, and the score at j is the first element reaching bucket j.
#include "pod_device.h"
#include "pod_segsort.h"

namespace pod {

constexpr int COCO_KEEP = POD_COCO_MAX_KEEP;     // kept detections per pair (maxDets[-1] <= 128)
constexpr int COCO_LDS_GT = POD_COCO_LDS_GT;     // ground-truth boxes per pair whose IoU matrix lives in LDS
constexpr int COCO_TILE = 1024;                  // k_coco_sort_tiles run length
constexpr int COCO_FLAG_CROWD = 1, COCO_FLAG_ID = 0x40;   // per-GT flag bits; bit 1 + a: ignored in area range a

struct KCocoImages {
    PodCocoParams prm;
    const int64_t* pairs;
    const double* dt_boxes;
    const double* dt_score;
    const double* gt_boxes;
    const double* gt_area;
    const int32_t* gt_crowd;
    const int64_t* gt_id;
    unsigned char* scratch;
    double* kept_score;
    uint64_t* kept_match;
    uint64_t* kept_ignore;
    int32_t* kept_rank;
    int32_t* npig;
};

// maskUtils.iou (bbIou) for one xywh pair in fp64, the same operations in the same order
__device__ inline double coco_iou(const double* D, const double* G, bool crowd) {
    const double ga = G[2] * G[3], da = D[2] * D[3];
    const double w = fmin(D[2] + D[0], G[2] + G[0]) - fmax(D[0], G[0]);
    if (w <= 0) return 0.0;
    const double h = fmin(D[3] + D[1], G[3] + G[1]) - fmax(D[1], G[1]);
    if (h <= 0) return 0.0;
    const double i = w * h;
    const double u = crowd ? da : da + ga - i;
    return i / u;
}

__device__ inline bool coco_out_of_range(double area, const double* rng) { return area < rng[0] || area > rng[1]; }

__global__ void __launch_bounds__(256) k_coco_eval_images(const KCocoImages P) {
    __shared__ double s_iou[COCO_KEEP * COCO_LDS_GT];
    __shared__ uint64_t s_gtm[64];
    __shared__ int32_t s_sel[COCO_KEEP];
    __shared__ unsigned char s_flag[COCO_LDS_GT];
    __shared__ int32_t s_cnt[POD_COCO_MAX_AREA];
    const int tid = threadIdx.x;
    const int64_t* pr = P.pairs + (size_t)blockIdx.x * 8;
    const int k = (int)pr[0];
    const int64_t g0 = pr[2], d0 = pr[4], o0 = pr[6];
    const int G = (int)pr[3], ND = (int)pr[5];
    const int T = P.prm.n_iou, A = P.prm.n_area;
    const int nd = min(ND, P.prm.max_dets[P.prm.n_maxdet - 1]);
    const bool big = G > COCO_LDS_GT;
    const int W = (G + 63) / 64;
    unsigned char* sp = P.scratch + (big ? pr[7] : 0);
    double* iou = big ? (double*)sp : s_iou;
    const size_t flag_at = (size_t)nd * G * 8;
    unsigned char* flag = big ? sp + flag_at : s_flag;
    uint64_t* gtm = big ? (uint64_t*)(sp + ((flag_at + G + 7) & ~(size_t)7)) : s_gtm;

    if (tid < A) s_cnt[tid] = 0;
    // stable descending rank of every detection of the pair; the first nd are kept
    for (int i = tid; i < ND; i += blockDim.x) {
        const double s = P.dt_score[d0 + i];
        int r = 0;
        for (int j = 0; j < ND; ++j) {
            const double q = P.dt_score[d0 + j];
            r += (q > s || (q == s && j < i)) ? 1 : 0;
        }
        if (r < nd) s_sel[r] = i;
    }
    for (int i = tid; i < 64 * W; i += blockDim.x) gtm[i] = 0ull;
    __syncthreads();
    for (int g = tid; g < G; g += blockDim.x) {
        const double area = P.gt_area[g0 + g];
        const bool crowd = P.gt_crowd[g0 + g] != 0;
        int f = (crowd ? COCO_FLAG_CROWD : 0) | (P.gt_id[g0 + g] != 0 ? COCO_FLAG_ID : 0);
        for (int a = 0; a < A; ++a) {
            const bool ig = crowd || coco_out_of_range(area, P.prm.area_rng + 2 * a);
            f |= ig ? (2 << a) : 0;
            if (!ig) atomicAdd(&s_cnt[a], 1);
        }
        flag[g] = (unsigned char)f;
    }
    for (int r = tid; r < nd; r += blockDim.x) {
        const int i = s_sel[r];
        P.kept_score[o0 + r] = P.dt_score[d0 + i];
        P.kept_rank[o0 + r] = r;
    }
    for (int e = tid; e < nd * G; e += blockDim.x) {
        const int d = e / G, g = e - d * G;
        iou[e] = coco_iou(P.dt_boxes + (size_t)(d0 + s_sel[d]) * 4, P.gt_boxes + (size_t)(g0 + g) * 4, P.gt_crowd[g0 + g] != 0);
    }
    __syncthreads();
    if (tid < A && s_cnt[tid] > 0) atomicAdd(&P.npig[k * A + tid], s_cnt[tid]);
    if (tid >= 64) return;
    // wave 0: lane L = a * T + t runs evaluateImg's greedy match for IoU threshold t in area range a
    const int L = tid;
    const bool active = L < T * A;
    const int a = active ? L / T : 0, t = active ? L - a * T : 0;
    const int igbit = 2 << a;
    const double lim = 1.0 - 1e-10;
    const double th = lim < P.prm.iou_thrs[t] ? lim : P.prm.iou_thrs[t];      // min([t, 1 - 1e-10])
    uint64_t* mine = gtm + (size_t)L * W;
    const double* rng = P.prm.area_rng + 2 * a;
    for (int d = 0; d < nd; ++d) {
        bool matched = false, ignored = false;
        if (active) {
            const double* row = iou + (size_t)d * G;
            double best = th;
            int m = -1;
            // ground truth in evaluateImg's order: the non-ignored boxes, then the ignored ones; once a non-ignored box is
            // matched the loop breaks at the first ignored one, so the second pass only runs when the first found nothing
            for (int pass = 0; pass < 2 && m < 0; ++pass) {
                for (int g = 0; g < G; ++g) {
                    const int f = flag[g];
                    if (((f & igbit) != 0) != (pass == 1)) continue;
                    if (((mine[g >> 6] >> (g & 63)) & 1ull) && !(f & COCO_FLAG_CROWD)) continue;
                    const double v = row[g];
                    if (v < best) continue;
                    best = v;
                    m = g;
                }
            }
            if (m >= 0) {
                mine[m >> 6] |= 1ull << (m & 63);            // gtm = detection id (>= 1: loadRes numbers detections from 1)
                ignored = (flag[m] & igbit) != 0;
                matched = (flag[m] & COCO_FLAG_ID) != 0;    // dtm = ground-truth id: id 0 reads as unmatched
            }
            const double* D = P.dt_boxes + (size_t)(d0 + s_sel[d]) * 4;
            if (!matched && coco_out_of_range(D[2] * D[3], rng)) ignored = true;
        }
        const uint64_t mb = __ballot(matched), ib = __ballot(ignored);
        if (L == 0) {
            P.kept_match[o0 + d] = mb;
            P.kept_ignore[o0 + d] = ib;
        }
    }
}

// (score descending, position ascending) as one ascending order: a 64-bit key of the score plus the position as tie-break
__device__ inline uint64_t coco_desc_key(double s) {
    if (s == 0.0) s = 0.0;                                                   // -0.0 == 0.0 for numpy's comparison
    uint64_t u = (uint64_t)__double_as_longlong(s);
    u = (u >> 63) ? ~u : (u | 0x8000000000000000ull);
    return ~u;
}

__device__ inline bool coco_less(uint64_t ka, int32_t ia, uint64_t kb, int32_t ib) { return ka < kb || (ka == kb && ia < ib); }

struct KCocoSort {
    const int64_t* cat_off;
    const double* kept_score;
    uint64_t* key_in;
    int32_t* idx_in;
    uint64_t* key_out;
    int32_t* idx_out;
    int32_t w;
};

__global__ void __launch_bounds__(512) k_coco_sort_tiles(const KCocoSort P) {
    __shared__ uint64_t sk[COCO_TILE];
    __shared__ int32_t si[COCO_TILE];
    const int k = blockIdx.y, tid = threadIdx.x;
    const int64_t c0 = P.cat_off[k];
    const int n = (int)(P.cat_off[k + 1] - c0);
    const int base = blockIdx.x * COCO_TILE;
    if (base >= n) return;
    for (int i = tid; i < COCO_TILE; i += blockDim.x) {
        const int p = base + i;
        sk[i] = p < n ? (P.kept_score ? coco_desc_key(P.kept_score[c0 + p]) : P.key_in[c0 + p]) : ~0ull;
        si[i] = p < n ? (int32_t)(c0 + p) : 0x7fffffff;
    }
    for (int size = 2; size <= COCO_TILE; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            __syncthreads();
            const int lo = 2 * tid - (tid & (stride - 1)), hi = lo + stride;
            const bool up = (lo & size) == 0;
            if (coco_less(sk[hi], si[hi], sk[lo], si[lo]) == up) {
                const uint64_t kk = sk[lo];
                sk[lo] = sk[hi];
                sk[hi] = kk;
                const int32_t ii = si[lo];
                si[lo] = si[hi];
                si[hi] = ii;
            }
        }
    }
    __syncthreads();
    for (int i = tid; i < COCO_TILE; i += blockDim.x) {
        const int p = base + i;
        if (p < n) {
            P.key_out[c0 + p] = sk[i];
            P.idx_out[c0 + p] = si[i];
        }
    }
}

__global__ void __launch_bounds__(256) k_coco_merge(const KCocoSort P) {
    const int k = blockIdx.y;
    const int64_t c0 = P.cat_off[k];
    const int n = (int)(P.cat_off[k + 1] - c0);
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n) return;
    const int w = P.w, r = q / w, i = q - r * w, partner = r ^ 1;
    const int64_t ps = (int64_t)partner * w;
    const uint64_t key = P.key_in[c0 + q];
    const int32_t id = P.idx_in[c0 + q];
    int pos = q;
    if (ps < n) {
        int lo = 0, hi = (int)min((int64_t)w, n - ps);
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (coco_less(P.key_in[c0 + ps + mid], P.idx_in[c0 + ps + mid], key, id)) lo = mid + 1;
            else hi = mid;
        }
        pos = min(r, partner) * w + i + lo;
    }
    P.key_out[c0 + pos] = key;
    P.idx_out[c0 + pos] = id;
}

struct KCocoAcc {
    PodCocoParams prm;
    const int64_t* cat_off;
    const int32_t* order;
    const double* kept_score;
    const uint64_t* kept_match;
    const uint64_t* kept_ignore;
    const int32_t* kept_rank;
    double* s_score;
    uint64_t* s_match;
    uint64_t* s_ignore;
    int32_t* s_rank;
    const int32_t* npig;
    double* precision;
    double* recall;
    double* scores;
    int64_t n_kept;
};

__global__ void __launch_bounds__(256) k_coco_gather(const KCocoAcc P) {
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < P.n_kept; p += (int64_t)gridDim.x * blockDim.x) {
        const int32_t o = P.order[p];
        P.s_score[p] = P.kept_score[o];
        P.s_match[p] = P.kept_match[o];
        P.s_ignore[p] = P.kept_ignore[o];
        P.s_rank[p] = P.kept_rank[o];
    }
}

__global__ void __launch_bounds__(256) k_coco_fill(double* p, int64_t n, double v) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) p[i] = v;
}

// number of recall thresholds <= rc, minus one: the last searchsorted index this recall has reached
__device__ inline int coco_bucket(const double* rec, int R, double rc) {
    int lo = 0, hi = R;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (rec[mid] <= rc) lo = mid + 1;
        else hi = mid;
    }
    return lo - 1;
}

__global__ void __launch_bounds__(256) k_coco_accumulate(const KCocoAcc P) {
    __shared__ double s_rec[POD_COCO_MAX_REC];
    __shared__ unsigned long long s_max[POD_COCO_MAX_REC];
    __shared__ int64_t s_cnt[256 * 3];
    __shared__ int64_t s_tot[3];
    const int T = P.prm.n_iou, R = P.prm.n_rec, K = P.prm.n_cat, A = P.prm.n_area, M = P.prm.n_maxdet;
    const int b = blockIdx.x, tid = threadIdx.x;
    const int t = b % T, m = (b / T) % M, a = (b / (T * M)) % A, k = b / (T * M * A);
    const int npig = P.npig[k * A + a];
    if (npig == 0) return;                                          // pycocotools leaves -1
    const int64_t c0 = P.cat_off[k], n = P.cat_off[k + 1] - c0;
    const int max_det = P.prm.max_dets[m], bit = a * T + t;
    for (int j = tid; j < R; j += blockDim.x) {
        s_rec[j] = P.prm.rec_thrs[j];
        s_max[j] = 0ull;
    }
    const int64_t per = (n + blockDim.x - 1) / blockDim.x;
    const int64_t s0 = min((int64_t)tid * per, n), s1 = min(s0 + per, n);
    int64_t nd = 0, tp = 0, fp = 0;
    for (int64_t i = c0 + s0; i < c0 + s1; ++i) {
        if (P.s_rank[i] >= max_det) continue;
        ++nd;
        if ((P.s_ignore[i] >> bit) & 1ull) continue;
        if ((P.s_match[i] >> bit) & 1ull) ++tp;
        else ++fp;
    }
    s_cnt[tid * 3 + 0] = nd;
    s_cnt[tid * 3 + 1] = tp;
    s_cnt[tid * 3 + 2] = fp;
    __syncthreads();
    if (tid == 0) {
        int64_t run[3] = {0, 0, 0};
        for (int q = 0; q < (int)blockDim.x; ++q)
            for (int c = 0; c < 3; ++c) {
                const int64_t v = s_cnt[q * 3 + c];
                s_cnt[q * 3 + c] = run[c];
                run[c] += v;
            }
        for (int c = 0; c < 3; ++c) s_tot[c] = run[c];
    }
    __syncthreads();
    nd = s_cnt[tid * 3 + 0];
    tp = s_cnt[tid * 3 + 1];
    fp = s_cnt[tid * 3 + 2];
    const double dn = (double)npig, eps = 2.220446049250313e-16;     // np.spacing(1)
    const size_t sR = (size_t)K * A * M, sT = (size_t)R * sR, base = (size_t)t * sT + ((size_t)k * A + a) * M + m;
    int prev = nd ? coco_bucket(s_rec, R, (double)tp / dn) : -1;    // bucket of the element before this slice
    int cur = prev;
    int64_t tp_seen = -1;
    int bi = prev;
    double run_max = 0.0;
    for (int64_t i = c0 + s0; i < c0 + s1; ++i) {
        if (P.s_rank[i] >= max_det) continue;
        if (!((P.s_ignore[i] >> bit) & 1ull)) {
            if ((P.s_match[i] >> bit) & 1ull) ++tp;
            else ++fp;
        }
        if (tp != tp_seen) {
            bi = coco_bucket(s_rec, R, (double)tp / dn);
            tp_seen = tp;
        }
        const double pr = (double)tp / (((double)fp + (double)tp) + eps);
        if (bi != cur) {
            if (cur >= 0) atomicMax(&s_max[cur], (unsigned long long)__double_as_longlong(run_max));
            cur = bi;
            run_max = 0.0;
        }
        run_max = fmax(run_max, pr);
        for (int j = prev + 1; j <= bi; ++j) P.scores[base + (size_t)j * sR] = P.s_score[i];
        if (bi > prev) prev = bi;
    }
    if (cur >= 0) atomicMax(&s_max[cur], (unsigned long long)__double_as_longlong(run_max));
    __syncthreads();
    if (tid == 0) {
        const int64_t ndt = s_tot[0], tpt = s_tot[1];
        P.recall[((size_t)t * K + k) * A * M + (size_t)a * M + m] = ndt ? (double)tpt / dn : 0.0;
        const int last = ndt ? coco_bucket(s_rec, R, (double)tpt / dn) : -1;
        double env = 0.0;
        for (int j = R - 1; j >= 0; --j) {
            if (j > last) {                                         // searchsorted index >= nd: the bare except leaves 0
                P.precision[base + (size_t)j * sR] = 0.0;
                P.scores[base + (size_t)j * sR] = 0.0;
            } else {
                env = fmax(env, __longlong_as_double((long long)s_max[j]));
                P.precision[base + (size_t)j * sR] = env;
            }
        }
    }
}

static bool coco_params_ok(const PodCocoParams* p) {
    if (!p) return false;
    if (p->n_iou < 1 || p->n_iou > POD_COCO_MAX_IOU || p->n_area < 1 || p->n_area > POD_COCO_MAX_AREA || p->n_iou * p->n_area > 64)
        return false;
    if (p->n_rec < 1 || p->n_rec > POD_COCO_MAX_REC || p->n_maxdet < 1 || p->n_maxdet > POD_COCO_MAX_MAXDET || p->n_cat < 1) return false;
    for (int m = 0; m < p->n_maxdet; ++m)
        if (p->max_dets[m] < 1 || p->max_dets[m] > p->max_dets[p->n_maxdet - 1]) return false;
    return p->max_dets[p->n_maxdet - 1] <= POD_COCO_MAX_KEEP;
}

static size_t coco_align(size_t x) { return (x + 255) & ~(size_t)255; }

int segsort(const int64_t* seg_off, int32_t n_seg, int32_t max_seg, const double* desc_scores, uint64_t* key0, int32_t* idx0,
            uint64_t* key1, int32_t* idx1, uint64_t** keys, int32_t** order, hipStream_t st) {
    KCocoSort S;
    S.cat_off = seg_off; S.kept_score = desc_scores; S.key_in = key0; S.idx_in = idx0; S.key_out = key0; S.idx_out = idx0; S.w = 0;
    if (max_seg > 0 && n_seg > 0) {
        hipLaunchKernelGGL(k_coco_sort_tiles, dim3((max_seg + COCO_TILE - 1) / COCO_TILE, n_seg), dim3(512), 0, st, S);
        POD_CHECK_LAUNCH();
        for (int w = COCO_TILE; w < max_seg; w *= 2) {
            S.key_out = S.key_in == key0 ? key1 : key0;
            S.idx_out = S.idx_in == idx0 ? idx1 : idx0;
            S.w = w;
            hipLaunchKernelGGL(k_coco_merge, dim3((max_seg + 255) / 256, n_seg), dim3(256), 0, st, S);
            POD_CHECK_LAUNCH();
            S.key_in = S.key_out;
            S.idx_in = S.idx_out;
        }
    }
    *keys = S.key_in;
    *order = S.idx_in;
    return POD_OK;
}

}  // namespace pod

extern "C" size_t pod_coco_eval_scratch_bytes(int32_t n_keep, int32_t n_gt) {
    if (n_gt <= POD_COCO_LDS_GT || n_keep < 0) return 0;
    const size_t G = (size_t)n_gt, nd = (size_t)(n_keep < POD_COCO_MAX_KEEP ? n_keep : POD_COCO_MAX_KEEP);
    const size_t flags_end = ((nd * G * 8 + G) + 7) & ~(size_t)7;
    return (flags_end + 64 * ((G + 63) / 64) * 8 + 15) & ~(size_t)15;
}

extern "C" int pod_coco_eval_images(const PodCocoParams* prm, const int64_t* pairs, int32_t n_pairs, const double* dt_boxes,
                                    const double* dt_score, const double* gt_boxes, const double* gt_area, const int32_t* gt_crowd,
                                    const int64_t* gt_id, void* scratch, double* kept_score, uint64_t* kept_match,
                                    uint64_t* kept_ignore, int32_t* kept_rank, int32_t* npig, pod_stream_t stream) {
    if (!pod::coco_params_ok(prm) || n_pairs < 0 || !npig) return POD_E_INVALID;
    if (n_pairs > 0 && (!pairs || !kept_score || !kept_match || !kept_ignore || !kept_rank)) return POD_E_INVALID;
    if (hipMemsetAsync(npig, 0, sizeof(int32_t) * prm->n_cat * prm->n_area, (hipStream_t)stream) != hipSuccess) return POD_E_LAUNCH;
    if (n_pairs == 0) return POD_OK;
    pod::KCocoImages P;
    P.prm = *prm; P.pairs = pairs; P.dt_boxes = dt_boxes; P.dt_score = dt_score; P.gt_boxes = gt_boxes; P.gt_area = gt_area;
    P.gt_crowd = gt_crowd; P.gt_id = gt_id; P.scratch = (unsigned char*)scratch; P.kept_score = kept_score; P.kept_match = kept_match;
    P.kept_ignore = kept_ignore; P.kept_rank = kept_rank; P.npig = npig;
    hipLaunchKernelGGL(pod::k_coco_eval_images, dim3(n_pairs), dim3(256), 0, (hipStream_t)stream, P);
    POD_CHECK_LAUNCH();
    return POD_OK;
}

extern "C" size_t pod_coco_accumulate_workspace_bytes(int64_t n_kept) {
    if (n_kept <= 0) return 0;
    const size_t n = (size_t)n_kept;
    return 2 * pod::coco_align(8 * n) + 2 * pod::coco_align(4 * n) + 3 * pod::coco_align(8 * n) + pod::coco_align(4 * n);
}

extern "C" int pod_coco_accumulate(const PodCocoParams* prm, const int64_t* cat_off, int32_t max_seg, int64_t n_kept,
                                   const double* kept_score, const uint64_t* kept_match, const uint64_t* kept_ignore,
                                   const int32_t* kept_rank, const int32_t* npig, void* workspace, double* precision, double* recall,
                                   double* scores, pod_stream_t stream) {
    if (!pod::coco_params_ok(prm) || !cat_off || !npig || !precision || !recall || !scores) return POD_E_INVALID;
    if (n_kept < 0 || n_kept >= 0x7fffffff || max_seg < 0 || max_seg > n_kept) return POD_E_INVALID;
    if (n_kept > 0 && (!kept_score || !kept_match || !kept_ignore || !kept_rank || !workspace)) return POD_E_INVALID;
    const hipStream_t st = (hipStream_t)stream;
    const int T = prm->n_iou, R = prm->n_rec, K = prm->n_cat, A = prm->n_area, M = prm->n_maxdet;
    const int64_t n_prec = (int64_t)T * R * K * A * M, n_rec = (int64_t)T * K * A * M;
    hipLaunchKernelGGL(pod::k_coco_fill, dim3((unsigned)((n_prec + 255) / 256)), dim3(256), 0, st, precision, n_prec, -1.0);
    hipLaunchKernelGGL(pod::k_coco_fill, dim3((unsigned)((n_prec + 255) / 256)), dim3(256), 0, st, scores, n_prec, -1.0);
    hipLaunchKernelGGL(pod::k_coco_fill, dim3((unsigned)((n_rec + 255) / 256)), dim3(256), 0, st, recall, n_rec, -1.0);
    POD_CHECK_LAUNCH();
    const size_t n = (size_t)n_kept;
    unsigned char* ws = (unsigned char*)workspace;
    uint64_t* key0 = (uint64_t*)ws;
    uint64_t* key1 = (uint64_t*)(ws += pod::coco_align(8 * n));
    int32_t* idx0 = (int32_t*)(ws += pod::coco_align(8 * n));
    int32_t* idx1 = (int32_t*)(ws += pod::coco_align(4 * n));
    double* s_score = (double*)(ws += pod::coco_align(4 * n));
    uint64_t* s_match = (uint64_t*)(ws += pod::coco_align(8 * n));
    uint64_t* s_ignore = (uint64_t*)(ws += pod::coco_align(8 * n));
    int32_t* s_rank = (int32_t*)(ws += pod::coco_align(8 * n));
    pod::KCocoAcc P;
    P.prm = *prm; P.cat_off = cat_off; P.order = idx0; P.kept_score = kept_score; P.kept_match = kept_match; P.kept_ignore = kept_ignore;
    P.kept_rank = kept_rank; P.s_score = s_score; P.s_match = s_match; P.s_ignore = s_ignore; P.s_rank = s_rank; P.npig = npig;
    P.precision = precision; P.recall = recall; P.scores = scores; P.n_kept = n_kept;
    if (max_seg > 0) {
        uint64_t* keys;
        int32_t* order;
        if (pod::segsort(cat_off, K, max_seg, kept_score, key0, idx0, key1, idx1, &keys, &order, st) != POD_OK) return POD_E_LAUNCH;
        P.order = order;
        const int64_t blocks = (n_kept + 255) / 256;
        hipLaunchKernelGGL(pod::k_coco_gather, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, st, P);
        POD_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(pod::k_coco_accumulate, dim3(K * A * M * T), dim3(256), 0, st, P);
    POD_CHECK_LAUNCH();
    return POD_OK;
}
