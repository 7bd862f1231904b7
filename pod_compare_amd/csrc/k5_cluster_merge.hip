// The post-NMS tail: K5 bayes_fuse, K6 anchor_stats (also the cluster kernel of the post-NMS ensemble merge), K7 finalize, the ensemble
// merge's seed sweep and append kernel, reg_nll.
//
// Replaces:
//   K5  probabilistic_inference.py:562-636 (post_processing_bayes_od cluster loop, one host
//       round-trip per cluster at :591-601) + inference_utils.py:292-334
//       (bounding_box_bayesian_inference: numpy fp32 LAPACK inv/det).
//   K6  inference_utils.py:91-154 (general_anchor_statistics_postprocessing cluster loop); with ensemble_rule = 1 the cluster
//       moments of inference_utils.py:216-247, behind k_ensemble_seeds (:203-215) and k_append_rows (torch.cat of :191-196).
//   K7  inference_utils.py:42-53 (keep-gather of the standard-NMS path) and :374-425
//       (probabilistic_detector_postprocess), plus the XYWH records of :428-502.
//   NLL core/evaluation_tools/scoring_rules.py:68-74.
//
// K5 / K6: one 256-thread workgroup per kept cluster centre.  Only the <= 100 needed rows of the IoU
// matrix are evaluated, members are streamed once per pass, every lane inverts its
// members' 4x4 covariances in fp64 registers, and the Gaussian moments / precisions are
// combined with wavefront butterflies plus one LDS hop across the 4 waves.  K6's parts have names (cluster_prologue,
// FOR_EACH_MEMBER, centre_fallback); K5 is written out (see there); the host checks and fills both through cluster_params.
#include "pod_device.h"
#include "pod_reg_sigma.h"

namespace pod {

// ---- 4x4 helpers (fp64 registers) ---------------------------------------------------------------
struct M4 {
    double a[16];
};

// The twelve 2x2 minors of a 4x4 matrix -- s: rows 0, 1; c: rows 2, 3 -- and the Laplace expansion over them.
struct Minors4 {
    double s[6], c[6];
    __device__ __forceinline__ explicit Minors4(const double* a) {
        s[0] = a[0] * a[5] - a[4] * a[1]; s[1] = a[0] * a[6] - a[4] * a[2]; s[2] = a[0] * a[7] - a[4] * a[3];
        s[3] = a[1] * a[6] - a[5] * a[2]; s[4] = a[1] * a[7] - a[5] * a[3]; s[5] = a[2] * a[7] - a[6] * a[3];
        c[5] = a[10] * a[15] - a[14] * a[11]; c[4] = a[9] * a[15] - a[13] * a[11]; c[3] = a[9] * a[14] - a[13] * a[10];
        c[2] = a[8] * a[15] - a[12] * a[11]; c[1] = a[8] * a[14] - a[12] * a[10]; c[0] = a[8] * a[13] - a[12] * a[9];
    }
    __device__ __forceinline__ double det() const {
        return s[0] * c[5] - s[1] * c[4] + s[2] * c[3] + s[3] * c[2] - s[4] * c[1] + s[5] * c[0];
    }
};

__device__ __forceinline__ double inv4(const M4& m, M4& o) {
    const double* a = m.a;
    const Minors4 k(a);
    const double *s = k.s, *c = k.c;
    const double det = k.det(), id = 1.0 / det;
    o.a[0] = (a[5] * c[5] - a[6] * c[4] + a[7] * c[3]) * id;
    o.a[1] = (-a[1] * c[5] + a[2] * c[4] - a[3] * c[3]) * id;
    o.a[2] = (a[13] * s[5] - a[14] * s[4] + a[15] * s[3]) * id;
    o.a[3] = (-a[9] * s[5] + a[10] * s[4] - a[11] * s[3]) * id;
    o.a[4] = (-a[4] * c[5] + a[6] * c[2] - a[7] * c[1]) * id;
    o.a[5] = (a[0] * c[5] - a[2] * c[2] + a[3] * c[1]) * id;
    o.a[6] = (-a[12] * s[5] + a[14] * s[2] - a[15] * s[1]) * id;
    o.a[7] = (a[8] * s[5] - a[10] * s[2] + a[11] * s[1]) * id;
    o.a[8] = (a[4] * c[4] - a[5] * c[2] + a[7] * c[0]) * id;
    o.a[9] = (-a[0] * c[4] + a[1] * c[2] - a[3] * c[0]) * id;
    o.a[10] = (a[12] * s[4] - a[13] * s[2] + a[15] * s[0]) * id;
    o.a[11] = (-a[8] * s[4] + a[9] * s[2] - a[11] * s[0]) * id;
    o.a[12] = (-a[4] * c[3] + a[5] * c[1] - a[6] * c[0]) * id;
    o.a[13] = (a[0] * c[3] - a[1] * c[1] + a[2] * c[0]) * id;
    o.a[14] = (-a[12] * s[3] + a[13] * s[1] - a[14] * s[0]) * id;
    o.a[15] = (a[8] * s[3] - a[9] * s[1] + a[10] * s[0]) * id;
    return det;
}

__device__ __forceinline__ double det4(const M4& m) { return Minors4(m.a).det(); }

__device__ __forceinline__ void load_m4(const float* p, M4& m) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const float4 v = *reinterpret_cast<const float4*>(p + q * 4);
        m.a[q * 4 + 0] = v.x; m.a[q * 4 + 1] = v.y; m.a[q * 4 + 2] = v.z; m.a[q * 4 + 3] = v.w;
    }
}

// Block-wide sum of NV doubles per thread (256 threads = 4 waves); result valid in every thread.
template <int NV>
__device__ __forceinline__ void block_sum(double* v, double* lds /* [4][NV] */) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int q = 0; q < NV; ++q) v[q] = wave_sum(v[q]);
    __syncthreads();   // protect lds from the previous use
    if (lane == 0)
#pragma unroll
        for (int q = 0; q < NV; ++q) lds[wave * NV + q] = v[q];
    __syncthreads();
#pragma unroll
    for (int q = 0; q < NV; ++q) v[q] = (lds[q] + lds[NV + q]) + (lds[2 * NV + q] + lds[3 * NV + q]);
}

__device__ __forceinline__ int argmax_probs(const float* p, int K) {
    float best = p[0];
    int bk = 0;
    for (int k = 1; k < K; ++k)
        if (p[k] > best) {
            best = p[k];
            bk = k;
        }
    return bk;
}

struct K7Params {
    const int32_t* keep;   // may be null (identity)
    const int32_t* n_rows;
    const float* boxes;
    const float* cov;      // may be null -> zeros (IU:52-53)
    const float* scores;
    const int32_t* classes;
    const float* probs;
    int32_t K, max_det;
    float sx, sy, out_h, out_w;
    float* det_boxes;
    float* det_cov;
    float* det_scores;
    int32_t* det_classes;
    float* det_probs;
    float* records;
    int32_t* n_det;
};

// K7 body: thread t < POD_MAX_DETECTIONS owns input row t; every thread of the workgroup must call it (one barrier).
// s_flag: POD_MAX_DETECTIONS ints of LDS.
__device__ __forceinline__ void finalize_rows(const K7Params& P, int t, int rows, int* s_flag) {
    const int K = P.K;
    const bool live = t < rows && t < POD_MAX_DETECTIONS;
    const int src = live ? (P.keep ? P.keep[t] : t) : 0;
    float x1 = 0, y1 = 0, x2 = 0, y2 = 0;
    if (live) {
        const float* b = P.boxes + (size_t)src * 4;
        // Boxes.scale (IU:402) then Boxes.clip (IU:403)
        x1 = fminf(fmaxf(*(b + 0) * P.sx, 0.0f), P.out_w);
        y1 = fminf(fmaxf(*(b + 1) * P.sy, 0.0f), P.out_h);
        x2 = fminf(fmaxf(*(b + 2) * P.sx, 0.0f), P.out_w);
        y2 = fminf(fmaxf(*(b + 3) * P.sy, 0.0f), P.out_h);
    }
    const bool ok = live && ((x2 - x1) > 0.0f) && ((y2 - y1) > 0.0f);   // Boxes.nonempty (IU:404)
    // output row = number of non-empty rows before this one: ballots, not a walk over LDS flags (thread 127 paid 127
    // dependent LDS reads, ~5 us of this kernel's 7)
    static_assert(POD_MAX_DETECTIONS == 128, "two wavefronts of rows");
    const unsigned long long mask = __ballot(ok);
    if ((t & 63) == 0 && t < POD_MAX_DETECTIONS) s_flag[t >> 6] = __popcll(mask);
    __syncthreads();
    if (t >= POD_MAX_DETECTIONS) return;
    const int pos = __popcll(mask & ((1ull << (t & 63)) - 1ull)) + (t >= 64 ? s_flag[0] : 0);
    if (t == 0) *P.n_det = s_flag[0] + s_flag[1];
    if (!ok) return;
    *reinterpret_cast<float4*>(P.det_boxes + (size_t)pos * 4) = float4{x1, y1, x2, y2};
    const float score = *(P.scores + src);
    const int32_t cls = *(P.classes + src);
    P.det_scores[pos] = score;
    P.det_classes[pos] = cls;
    float pr[POD_MAX_CLASSES];
#pragma unroll
    for (int k = 0; k < POD_MAX_CLASSES; ++k)
        if (k < K) {
            pr[k] = *(P.probs + (size_t)src * K + k);
            P.det_probs[(size_t)pos * K + k] = pr[k];
        }
    const float s[4] = {P.sx, P.sy, P.sx, P.sy};
    float cv[16];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            float v = P.cov ? *(P.cov + (size_t)src * 16 + a * 4 + b) : 0.0f;
            v = v + ((a == b) ? 1e-4f : 0.0f);                        // IU:409
            v = (s[a] * v) * s[b];                                    // IU:411-424  S cov S^T
            cv[a * 4 + b] = v;
            P.det_cov[(size_t)pos * 16 + a * 4 + b] = v;
        }
    if (P.records) {
        // instances_to_json IU:471-499: XYWH box, T cov T^T with T = [[1,0,0,0],[0,1,0,0],[-1,0,1,0],[0,-1,0,1]]
        float* r = P.records + (size_t)pos * (6 + K + 16);
        r[0] = x1; r[1] = y1; r[2] = x2 - x1; r[3] = y2 - y1;
        r[4] = score;
        r[5] = (float)cls;
#pragma unroll
        for (int k = 0; k < POD_MAX_CLASSES; ++k)
            if (k < K) r[6 + k] = pr[k];
        float tc[16];
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            tc[0 * 4 + b] = cv[0 * 4 + b];
            tc[1 * 4 + b] = cv[1 * 4 + b];
            tc[2 * 4 + b] = cv[2 * 4 + b] - cv[0 * 4 + b];
            tc[3 * 4 + b] = cv[3 * 4 + b] - cv[1 * 4 + b];
        }
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            r[6 + K + a * 4 + 0] = tc[a * 4 + 0];
            r[6 + K + a * 4 + 1] = tc[a * 4 + 1];
            r[6 + K + a * 4 + 2] = tc[a * 4 + 2] - tc[a * 4 + 0];
            r[6 + K + a * 4 + 3] = tc[a * 4 + 3] - tc[a * 4 + 1];
        }
    }
}

__global__ void __launch_bounds__(POD_MAX_DETECTIONS) k7_finalize(const K7Params P) {
    __shared__ int s_flag[POD_MAX_DETECTIONS];
    finalize_rows(P, threadIdx.x, min(*P.n_rows, P.max_det), s_flag);
}

// ---- K6's parts, and what K5 and K6 share ---------------------------------------------------------------------------------------
struct ClusterParams {
    const int32_t *n_total, *keep, *n_keep, *classes;
    const float *boxes, *cov, *probs;   // cov: may be null in K6
    int32_t K, n_capacity;
    int32_t n_alloc;         // rows the candidate arrays really hold (speculative first loads stay inside)
    int32_t n_keep_alloc;    // entries of keep[] = workgroups of the grid (the entry point sets it)
    float aff;
    float *out_boxes, *out_cov, *out_scores, *out_probs;
    int32_t* out_classes;
};

constexpr int RED_SLOTS = 40;   // doubles per wavefront in the reduction buffer: the widest block_sum of either kernel

// What a workgroup knows after round trips 1 and 2: the centre's candidate row and box, the candidate rows to walk, and this
// thread's first two candidate boxes (rows tid, tid + 256; zeros beyond n_alloc).
struct Cluster {
    int ctr, n;
    Box bc, pre[2];
};

// K6's round trip 1 -- everything that does not depend on the centre, issued together: the two counts, this cluster's centre index
// (guarded: the grid may be larger than keep[]) and the first two candidate boxes of this thread (the kernel loads their classes in
// front of this call).  The kernels are chains of HBM / L2 round trips with a few hundred instructions in between: what counts is how
// many.  Round trip 2 -- the centre's box.  false: no cluster for this workgroup.
__device__ __forceinline__ bool cluster_prologue(const ClusterParams& P, Cluster& cl) {
    const int c = blockIdx.x, tid = threadIdx.x;
    const int n_live = *P.n_keep, n_raw = *P.n_total;
    cl.ctr = c < P.n_keep_alloc ? P.keep[c] : 0;
    cl.pre[0] = tid < P.n_alloc ? load_box(P.boxes, tid) : Box{0.f, 0.f, 0.f, 0.f};
    cl.pre[1] = tid + 256 < P.n_alloc ? load_box(P.boxes, tid + 256) : Box{0.f, 0.f, 0.f, 0.f};
    if (c >= n_live) return false;
    cl.n = min(n_raw, P.n_capacity);
    cl.bc = load_box(P.boxes, cl.ctr);
    return true;
}

// Does bj belong to the centre's cluster by IoU?  ge: IoU >= aff (black-box ensembles, IU:211-212), else IoU > aff (PI:565-566, IU:91-92).
__device__ __forceinline__ bool iou_member(const Box& bc, const Box& bj, bool ge, float aff) {
    const float iou = iou_pair(bc, bj);
    return ge ? iou >= aff : iou > aff;
}

// The member walk of K6's two passes: the block behind it runs for this thread's rows j = tid, tid + 256, ... < n, in that order,
// whose box bj passes iou_member; `it` counts the rows visited, and `continue` leaves a member.  PREFETCHED: rows 0 and 1 are cl.pre.
// (A statement macro, like SG_LOAD_FILTER in pod_split_gemm.h: as a template taking the block as a lambda the compiler no longer
// peels the two prefetched iterations out of pass 1 and the launch measures slower -- profiles/cluster_merge_shared.md.)
#define FOR_EACH_MEMBER(P, cl, ge, PREFETCHED, j, it, bj)                                                                 \
    for (int j = threadIdx.x, it = 0; j < (cl).n; j += 256, ++it)                                                        \
        if (const Box bj = (PREFETCHED) ? (it == 0 ? (cl).pre[0] : (it == 1 ? (cl).pre[1] : load_box((P).boxes, j)))    \
                                        : load_box((P).boxes, j);                                                       \
            !iou_member((cl).bc, bj, ge, (P).aff))                                                                       \
            continue;                                                                                                    \
        else

// The cluster is empty or degenerate: the centre's own box and covariance (IU:127-133; without candidate covariances 1e-4 I).
__device__ __forceinline__ void centre_fallback(const ClusterParams& P, int ctr, bool has_cov, float* ob, float* oc) {
#pragma unroll
    for (int r = 0; r < 4; ++r) ob[r] = P.boxes[(size_t)ctr * 4 + r];
#pragma unroll
    for (int e = 0; e < 16; ++e) oc[e] = has_cov ? P.cov[(size_t)ctr * 16 + e] : ((e % 5 == 0) ? 1e-4f : 0.0f);
}

// ---- K5 ------------------------------------------------------------------------------------------------------------------------
// K5 is the kernel it was before K6's parts got names, statement for statement, on the argument block it had: every form of it that
// took the shared prologue, the walk macro, centre_fallback or ClusterParams measured 0.05 - 0.3 us slower per launch, and this one
// compiles to the same instructions as before (profiles/cluster_merge_shared.md).  What it shares: inv4 / det4's minors, the named
// accumulator slots, the reduction buffer's size and, on the host, cluster_params.
struct K5Params {
    const int32_t* n_total;
    const int32_t* keep;
    const int32_t* n_keep;
    const float* boxes;
    const float* cov;
    const float* scores;
    const int32_t* classes;
    const float* probs;
    int32_t K, box_mode, cls_mode, n_capacity;
    int32_t n_alloc;       // rows the candidate arrays really hold (speculative first loads stay inside)
    float aff;
    float* out_boxes;
    float* out_cov;
    float* out_scores;
    int32_t* out_classes;
    float* out_probs;
};

// K5's accumulators.  The Gaussian moments: [16] sum of w P, [4] sum of w P mu -- pass A's acc with w = 1, and wsum, which holds these
// MOM_N slots and no more, with the covariance-intersection weights.  Behind them in acc only: same-class members, IoU members,
// [POD_MAX_CLASSES] probability sums over the IoU members.
enum { MOM_P = 0, MOM_PMU = 16, MOM_N = 20 };
enum { K5_SAME = MOM_N, K5_IOU, K5_PROBS, K5_N = K5_PROBS + POD_MAX_CLASSES };

__global__ void __launch_bounds__(256) k5_bayes_fuse(const K5Params P) {
    __shared__ double s_red[4 * RED_SLOTS];
    const int c = blockIdx.x;
    const int tid = threadIdx.x;
    // Round trip 1 -- everything that does not depend on the centre, issued together: the two counts, this cluster's
    // centre index (keep[] has a slot for every workgroup of the grid) and the first two candidate boxes of this thread.
    // The kernel is a chain of HBM / L2 round trips with a few hundred instructions in between: what counts is how many.
    const int n_live = *P.n_keep;
    const int n_raw = *P.n_total;
    const int ctr = P.keep[c];
    Box pre[2];
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        const int j = tid + q * 256;
        pre[q] = j < P.n_alloc ? load_box(P.boxes, j) : Box{0.f, 0.f, 0.f, 0.f};
    }
    if (c >= n_live) return;
    const int n = min(n_raw, P.n_capacity);
    const int K = P.K;
    // round trip 2 -- the centre
    const Box bc = load_box(P.boxes, ctr);
    const int ccls = argmax_probs(P.probs + (size_t)ctr * K, K);     // PI:578-579

    // pass A: total precision, precision-weighted mean, member count, prob sums
    double acc[K5_N];
#pragma unroll
    for (int q = 0; q < K5_N; ++q) acc[q] = 0.0;
    for (int j = tid, it = 0; j < n; j += 256, ++it) {
        const Box bj = it == 0 ? pre[0] : (it == 1 ? pre[1] : load_box(P.boxes, j));
        if (!(iou_pair(bc, bj) > P.aff)) continue;                    // PI:565-566
        // round trip 3 -- the members' probabilities and covariances (a handful of rows per cluster)
        if (P.cls_mode == 1) {                                        // PI:583-585: mean over ALL IoU members
#pragma unroll
            for (int k = 0; k < POD_MAX_CLASSES; ++k)             // static indices: the accumulators stay in registers
                if (k < K) acc[K5_PROBS + k] += (double)P.probs[(size_t)j * K + k];
            acc[K5_IOU] += 1.0;
        }
        M4 cv;
        load_m4(P.cov + (size_t)j * 16, cv);                          // issued with the probability loads of argmax_probs
        if (argmax_probs(P.probs + (size_t)j * K, K) != ccls) continue;   // PI:580-582
        M4 pr;
        inv4(cv, pr);                                                 // IU:306
        const double mu[4] = {bj.x1, bj.y1, bj.x2, bj.y2};
#pragma unroll
        for (int q = 0; q < 16; ++q) acc[q] += pr.a[q];
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[16 + r] += pr.a[r * 4 + 0] * mu[0] + pr.a[r * 4 + 1] * mu[1] + pr.a[r * 4 + 2] * mu[2] + pr.a[r * 4 + 3] * mu[3];
        acc[K5_SAME] += 1.0;
    }
    // the class-probability sums are only needed (and only accumulated) in cls_mode 1: 22 instead of 38 fp64 butterflies otherwise
    if (P.cls_mode == 1) block_sum<K5_N>(acc, s_red);
    else block_sum<K5_PROBS>(acc, s_red);
    const double m_same = acc[K5_SAME];
    M4 total;
#pragma unroll
    for (int q = 0; q < 16; ++q) total.a[q] = acc[q];

    double wsum[MOM_N];   // weighted precision sum + weighted P*mu (covariance intersection)
    if (P.box_mode == 1 && m_same > 0.0) {
        // IU:313-332: omega_i = (det(T) - det(T - P_i) + det(P_i)) / (m det(T) + sum_i (det(P_i) - det(T - P_i)))
        const double d_tot = det4(total);
        double dsum[1] = {0.0};
        for (int j = tid; j < n; j += 256) {
            const Box bj = load_box(P.boxes, j);
            if (!(iou_pair(bc, bj) > P.aff)) continue;
            if (argmax_probs(P.probs + (size_t)j * K, K) != ccls) continue;
            M4 cv, pr, rest;
            load_m4(P.cov + (size_t)j * 16, cv);
            inv4(cv, pr);
#pragma unroll
            for (int q = 0; q < 16; ++q) rest.a[q] = total.a[q] - pr.a[q];
            dsum[0] += det4(pr) - det4(rest);
        }
        block_sum<1>(dsum, s_red);
        const double denom = m_same * d_tot + dsum[0];
#pragma unroll
        for (int q = 0; q < MOM_N; ++q) wsum[q] = 0.0;
        for (int j = tid; j < n; j += 256) {
            const Box bj = load_box(P.boxes, j);
            if (!(iou_pair(bc, bj) > P.aff)) continue;
            if (argmax_probs(P.probs + (size_t)j * K, K) != ccls) continue;
            M4 cv, pr, rest;
            load_m4(P.cov + (size_t)j * 16, cv);
            inv4(cv, pr);
#pragma unroll
            for (int q = 0; q < 16; ++q) rest.a[q] = total.a[q] - pr.a[q];
            const double omega = (d_tot - det4(rest) + det4(pr)) / denom;
            const double mu[4] = {bj.x1, bj.y1, bj.x2, bj.y2};
#pragma unroll
            for (int q = 0; q < 16; ++q) wsum[q] += omega * pr.a[q];
#pragma unroll
            for (int r = 0; r < 4; ++r)
                wsum[16 + r] += omega * (pr.a[r * 4 + 0] * mu[0] + pr.a[r * 4 + 1] * mu[1] + pr.a[r * 4 + 2] * mu[2] + pr.a[r * 4 + 3] * mu[3]);
        }
        block_sum<MOM_N>(wsum, s_red);
    } else {
#pragma unroll
        for (int q = 0; q < MOM_N; ++q) wsum[q] = acc[q];
    }

    if (tid == 0) {
        float* ob = P.out_boxes + (size_t)c * 4;
        float* oc = P.out_cov + (size_t)c * 16;
        if (m_same > 0.0) {
            M4 psum, fused;
#pragma unroll
            for (int q = 0; q < 16; ++q) psum.a[q] = wsum[q];
            inv4(psum, fused);                                        // IU:308 / IU:326
#pragma unroll
            for (int r = 0; r < 4; ++r)
                ob[r] = (float)(fused.a[r * 4 + 0] * wsum[16] + fused.a[r * 4 + 1] * wsum[17] + fused.a[r * 4 + 2] * wsum[18] + fused.a[r * 4 + 3] * wsum[19]);
#pragma unroll
            for (int q = 0; q < 16; ++q) oc[q] = (float)fused.a[q];
        } else {   // degenerate centre (self-IoU 0, Q12): keep the centre's own estimate
#pragma unroll
            for (int r = 0; r < 4; ++r) ob[r] = P.boxes[(size_t)ctr * 4 + r];
#pragma unroll
            for (int q = 0; q < 16; ++q) oc[q] = P.cov[(size_t)ctr * 16 + q];
        }
        float* op = P.out_probs + (size_t)c * K;
        if (P.cls_mode == 1 && acc[K5_IOU] > 0.0) {                       // PI:583-585, :609-613
            float best = 0.0f;
            int bk = 0;
#pragma unroll
            for (int k = 0; k < POD_MAX_CLASSES; ++k) {
                if (k < K) {
                    const float p = (float)(acc[K5_PROBS + k] / acc[K5_IOU]);
                    op[k] = p;
                    if (k == 0 || p > best) {
                        best = p;
                        bk = k;
                    }
                }
            }
            P.out_scores[c] = best;
            P.out_classes[c] = bk;
        } else {                                                      // PI:614-617 max_score
            for (int k = 0; k < K; ++k) op[k] = P.probs[(size_t)ctr * K + k];
            P.out_scores[c] = P.scores[ctr];
            P.out_classes[c] = P.classes[ctr];
        }
    }
}

// ---- K6 ------------------------------------------------------------------------------------------------------------------------
struct K6Params : ClusterParams {
    int32_t ensemble_rule;   // 0: anchor statistics (IoU > aff, IU:102 singleton rule); 1: black-box ensembles (IoU >= aff, IU:211-247)
};

// K6's pass-1 accumulators: IoU members, same-class members, then over the latter [4] box sum, [POD_MAX_CLASSES] probability sums,
// [16] covariance sum.  Pass 2: the K6_RR entries of the upper triangle of the residuals' outer-product sum.
enum { K6_IOU = 0, K6_SAME, K6_BOX, K6_PROBS = K6_BOX + 4, K6_COV = K6_PROBS + POD_MAX_CLASSES, K6_N = K6_COV + 16, K6_RR = 10 };
static_assert(K5_N <= RED_SLOTS && K6_N <= RED_SLOTS, "reduction buffer");

__global__ void __launch_bounds__(256) k6_anchor_stats(const K6Params P) {
    __shared__ double s_red[4 * RED_SLOTS];
    const int c = blockIdx.x, tid = threadIdx.x;
    // round trip 1 also brings the classes of this thread's first two candidate rows
    const int pre_cls[2] = {tid < P.n_alloc ? P.classes[tid] : -1, tid + 256 < P.n_alloc ? P.classes[tid + 256] : -1};
    Cluster cl;
    if (!cluster_prologue(P, cl)) return;
    const int ctr = cl.ctr, K = P.K;
    const int ccls = P.classes[ctr];                                 // IU:104
    const bool has_cov = P.cov != nullptr;

    // pass 1: member counts, box sum, prob sum, covariance sum of same-class members
    double acc[K6_N] = {};
    const bool ens = P.ensemble_rule != 0;                           // IU:91-92 (>) / IU:211-212 (>=)
    FOR_EACH_MEMBER(P, cl, ens, true, j, it, bj) {
        acc[K6_IOU] += 1.0;                                           // IU:102 counts every IoU member
        const int cj = it == 0 ? pre_cls[0] : (it == 1 ? pre_cls[1] : P.classes[j]);   // rows 0 and 1: prefetched
        if (cj != ccls) continue;                                       // IU:104-106
        acc[K6_SAME] += 1.0;
        acc[K6_BOX] += bj.x1; acc[K6_BOX + 1] += bj.y1; acc[K6_BOX + 2] += bj.x2; acc[K6_BOX + 3] += bj.y2;
#pragma unroll
        for (int k = 0; k < POD_MAX_CLASSES; ++k)                 // static indices: the accumulators stay in registers
            if (k < K) acc[K6_PROBS + k] += (double)P.probs[(size_t)j * K + k];
        if (has_cov)
#pragma unroll
            for (int q = 0; q < 16; ++q) acc[K6_COV + q] += (double)P.cov[(size_t)j * 16 + q];
    }
    block_sum<K6_N>(acc, s_red);
    const double m_all = acc[K6_IOU], m = acc[K6_SAME];
    const bool cluster = ens ? (m >= 1.0) : (m_all >= 2.0 && m >= 1.0);   // IU:226-247: a 1-member cluster is its own mean
    // the reference forms the mean in fp32 and subtracts it from fp32 boxes (IU:112-114)
    float mu[4] = {0, 0, 0, 0};
    if (cluster)
#pragma unroll
        for (int r = 0; r < 4; ++r) mu[r] = (float)(acc[K6_BOX + r] / m);
    double rr[K6_RR] = {};
    if (cluster) {
        FOR_EACH_MEMBER(P, cl, ens, false, j, it, bj) {
            if (P.classes[j] != ccls) continue;
            const float r[4] = {bj.x1 - mu[0], bj.y1 - mu[1], bj.x2 - mu[2], bj.y2 - mu[3]};
            int q = 0;
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = a; b < 4; ++b, ++q) rr[q] += (double)(r[a] * r[b]);
        }
    }
    block_sum<K6_RR>(rr, s_red);
    if (tid == 0) {
        float* ob = P.out_boxes + (size_t)c * 4;
        float* oc = P.out_cov + (size_t)c * 16;
        float* op = P.out_probs + (size_t)c * K;
        if (cluster) {
            const double denom = fmax(m - 1.0, 1.0);                  // IU:116
            int q = 0;
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = a; b < 4; ++b, ++q) {
                    float v = (float)(rr[q] / denom);
                    oc[a * 4 + b] = v;
                    oc[b * 4 + a] = v;
                }
            if (has_cov)                                              // IU:120-123
#pragma unroll
                for (int e = 0; e < 16; ++e) oc[e] = oc[e] + (float)(acc[K6_COV + e] / m);
#pragma unroll
            for (int r = 0; r < 4; ++r) ob[r] = mu[r];
#pragma unroll
            for (int k = 0; k < POD_MAX_CLASSES; ++k)
                if (k < K) op[k] = (float)(acc[K6_PROBS + k] / m);    // IU:126
        } else {                                                      // IU:127-133
            centre_fallback(P, ctr, has_cov, ob, oc);
            for (int k = 0; k < K; ++k) op[k] = P.probs[(size_t)ctr * K + k];
        }
        const int bk = argmax_probs(op, K);                           // IU:146-152 (Q10)
        P.out_scores[c] = op[bk];
        P.out_classes[c] = bk;
    }
}

// ---- post-NMS ensemble merge: sequential same-class clustering IU:203-215 ------------------------
// Box i seeds a cluster unless an EARLIER seed's cluster already contains it (IoU >= aff and same class): a greedy sweep
// in index order.  One 1024-thread workgroup, LDS "covered" bitmap, thread 0 finds the next uncovered index.
struct KSeedParams {
    const int32_t* m_total;
    int32_t capacity;
    float aff;
    const float* boxes;
    const int32_t* classes;
    int32_t* seeds;
    int32_t* n_seeds;
};

__global__ void __launch_bounds__(1024) k_ensemble_seeds(const KSeedParams P) {
    __shared__ unsigned long long s_cov[POD_MAX_CANDIDATES / 64];
    __shared__ int s_cur, s_n;
    const int tid = threadIdx.x;
    const int M = min(*P.m_total, P.capacity);
    for (int i = tid; i < POD_MAX_CANDIDATES / 64; i += 1024) s_cov[i] = 0ull;
    if (tid == 0) {
        s_cur = -1;
        s_n = 0;
    }
    __syncthreads();
    const int nwords = (M + 63) >> 6;
    while (true) {
        if (tid == 0) {
            int next = -1;
            const int start = s_cur + 1;
            for (int w = start >> 6; w < nwords; ++w) {
                unsigned long long live = ~s_cov[w];
                if (w == (start >> 6)) live &= ~0ull << (start & 63);
                if (live) {
                    const int cand = (w << 6) + __ffsll((long long)live) - 1;
                    if (cand < M) next = cand;
                    break;
                }
            }
            if (next >= 0) {
                P.seeds[s_n] = next;
                s_n = s_n + 1;
            }
            s_cur = next;
        }
        __syncthreads();
        const int i = s_cur;
        if (i < 0) break;
        const Box bi = load_box(P.boxes, i);
        const int ci = P.classes[i];
        for (int j = i + 1 + tid; j < M; j += 1024)
            if (P.classes[j] == ci && iou_pair(bi, load_box(P.boxes, j)) >= P.aff) atomicOr(&s_cov[j >> 6], 1ull << (j & 63));
        __syncthreads();
    }
    if (tid == 0) *P.n_seeds = s_n;
}

// Appends the rows `keep[0:n_keep)` of one ensemble member's candidate arrays to the concatenated member-detection
// arrays (torch.cat of IU:191-196); `total` is the running row count on the device.
struct KAppendParams {
    const int32_t* keep;
    const int32_t* n_keep;
    const float* boxes;
    const float* cov;      // may be null -> zeros (IU:52-53)
    const int32_t* classes;
    const float* probs;
    int32_t K, capacity;
    float* dst_boxes;
    float* dst_cov;
    int32_t* dst_classes;
    float* dst_probs;
    int32_t* total;
};

__global__ void __launch_bounds__(POD_MAX_DETECTIONS) k_append_rows(const KAppendParams P) {
    const int t = threadIdx.x;
    const int n = *P.n_keep;
    const int base = *P.total;
    __syncthreads();
    if (t < n && base + t < P.capacity) {
        const int src = P.keep[t], dst = base + t;
        *reinterpret_cast<float4*>(P.dst_boxes + (size_t)dst * 4) = *reinterpret_cast<const float4*>(P.boxes + (size_t)src * 4);
        for (int e = 0; e < 16; ++e) P.dst_cov[(size_t)dst * 16 + e] = P.cov ? P.cov[(size_t)src * 16 + e] : 0.0f;
        P.dst_classes[dst] = P.classes[src];
        for (int k = 0; k < P.K; ++k) P.dst_probs[(size_t)dst * P.K + k] = P.probs[(size_t)src * P.K + k];
    }
    __syncthreads();
    if (t == 0) *P.total = min(base + n, P.capacity);
}

__global__ void __launch_bounds__(256) k_reg_nll(const float* means, const float* covs, const float* gt, int n, float* nll) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    // -log N(gt; mean, cov + 1e-2 I) through a 4x4 Cholesky factor
    double a[4][4], L[4][4];
    reg_sigma_factor(covs + (size_t)i * 16, a, L);
    double logdet = 0.0;
    for (int r = 0; r < 4; ++r) logdet += log(L[r][r]);
    double y[4], maha = 0.0;
    for (int r = 0; r < 4; ++r) {
        double s = (double)gt[(size_t)i * 4 + r] - (double)means[(size_t)i * 4 + r];
        for (int k = 0; k < r; ++k) s -= L[r][k] * y[k];
        y[r] = s / L[r][r];
        maha += y[r] * y[r];
    }
    nll[i] = (float)(0.5 * maha + logdet + 2.0 * 1.8378770664093453);   // 0.5 * 4 * log(2 pi)
}

}  // namespace pod
// What pod_bayes_fuse, pod_anchor_stats_merge and pod_ensemble_merge check and fill alike, for ClusterParams or K5Params.  `ensemble`:
// the rows are an ensemble's concatenated member detections, `capacity` rows and as many centres at most; else the hot path's
// candidate arrays (n_levels * topk rows) and cfg->max_detections centres.  Returns the number of centres -- the grid, and K6's
// n_keep_alloc -- or 0 for invalid arguments.  `cov` may be null here: an entry point that needs it says so itself.
template <typename Params>
static int32_t cluster_params(Params& P, const PodConfig* cfg, bool ensemble, int32_t capacity, int32_t max_classes,
                              const int32_t* n_total, const int32_t* keep, const int32_t* n_keep, const float* boxes,
                              const float* cov, const int32_t* classes, const float* probs, float* out_boxes, float* out_cov,
                              float* out_scores, int32_t* out_classes, float* out_probs) {
    if (!cfg || !n_total || !keep || !n_keep || !boxes || !classes || !probs || !out_boxes || !out_cov || !out_scores ||
        !out_classes || !out_probs)
        return 0;
    if (cfg->num_classes < 1 || cfg->num_classes > max_classes) return 0;
    if (ensemble && (capacity < 1 || capacity > POD_MAX_CANDIDATES)) return 0;
    if (!ensemble && (cfg->max_detections < 1 || cfg->max_detections > POD_MAX_DETECTIONS)) return 0;
    P.n_total = n_total; P.keep = keep; P.n_keep = n_keep; P.boxes = boxes; P.cov = cov; P.classes = classes; P.probs = probs;
    P.K = cfg->num_classes; P.aff = cfg->affinity_thresh;
    P.n_capacity = ensemble ? capacity : POD_MAX_CANDIDATES;
    P.n_alloc = ensemble ? capacity : cfg->n_levels * cfg->topk;
    P.out_boxes = out_boxes; P.out_cov = out_cov; P.out_scores = out_scores; P.out_classes = out_classes; P.out_probs = out_probs;
    return ensemble ? capacity : cfg->max_detections;
}

extern "C" int pod_bayes_fuse(const PodConfig* cfg, const int32_t* n_total, const int32_t* keep, const int32_t* n_keep,
                              const float* boxes, const float* cov, const float* scores, const int32_t* classes,
                              const float* probs, int32_t box_mode, int32_t cls_mode, float* out_boxes, float* out_cov,
                              float* out_scores, int32_t* out_classes, float* out_probs, pod_stream_t stream) {
    if (!cov || !scores) return POD_E_INVALID;
    if (box_mode < 0 || box_mode > 1 || cls_mode < 0 || cls_mode > 1) return POD_E_INVALID;
    // One class fewer than the other two entry points accept.  That is pod_nms_cluster's limit (its prefix scan over POD_MAX_CLASSES
    // lanes keeps entry num_classes for the total), whose keep list K5 reads.  Nothing in k5_bayes_fuse needs it: its accumulators
    // and the reduction buffer hold POD_MAX_CLASSES classes.  Kept as it is: what an entry point accepts is part of its contract.
    pod::K5Params P;
    const int32_t centres = cluster_params(P, cfg, false, 0, POD_MAX_CLASSES - 1, n_total, keep, n_keep, boxes, cov, classes, probs,
                                           out_boxes, out_cov, out_scores, out_classes, out_probs);
    if (!centres) return POD_E_INVALID;
    P.scores = scores; P.box_mode = box_mode; P.cls_mode = cls_mode;
    hipLaunchKernelGGL(pod::k5_bayes_fuse, dim3(centres), dim3(256), 0, (hipStream_t)stream, P);
    POD_CHECK_LAUNCH();
    return POD_OK;
}

extern "C" int pod_anchor_stats_merge(const PodConfig* cfg, const int32_t* n_total, const int32_t* keep,
                                      const int32_t* n_keep, const float* boxes, const float* cov, const int32_t* classes,
                                      const float* probs, float* out_boxes, float* out_cov, float* out_scores,
                                      int32_t* out_classes, float* out_probs, pod_stream_t stream) {
    pod::K6Params P;
    const int32_t centres = cluster_params(P, cfg, false, 0, POD_MAX_CLASSES, n_total, keep, n_keep, boxes, cov, classes, probs,
                                           out_boxes, out_cov, out_scores, out_classes, out_probs);
    if (!centres) return POD_E_INVALID;
    P.n_keep_alloc = centres; P.ensemble_rule = 0;
    hipLaunchKernelGGL(pod::k6_anchor_stats, dim3(centres), dim3(256), 0, (hipStream_t)stream, P);
    POD_CHECK_LAUNCH();
    return POD_OK;
}

extern "C" int pod_ensemble_append(const PodConfig* cfg, const int32_t* keep, const int32_t* n_keep, const float* boxes,
                                   const float* cov, const int32_t* classes, const float* probs, int32_t capacity,
                                   float* dst_boxes, float* dst_cov, int32_t* dst_classes, float* dst_probs, int32_t* total,
                                   pod_stream_t stream) {
    if (!cfg || !keep || !n_keep || !boxes || !classes || !probs || !dst_boxes || !dst_cov || !dst_classes || !dst_probs || !total)
        return POD_E_INVALID;
    if (capacity < 1 || capacity > POD_MAX_CANDIDATES || cfg->num_classes < 1 || cfg->num_classes > POD_MAX_CLASSES) return POD_E_INVALID;
    pod::KAppendParams P;
    P.keep = keep; P.n_keep = n_keep; P.boxes = boxes; P.cov = cov; P.classes = classes; P.probs = probs; P.K = cfg->num_classes;
    P.capacity = capacity; P.dst_boxes = dst_boxes; P.dst_cov = dst_cov; P.dst_classes = dst_classes; P.dst_probs = dst_probs; P.total = total;
    hipLaunchKernelGGL(pod::k_append_rows, dim3(1), dim3(POD_MAX_DETECTIONS), 0, (hipStream_t)stream, P);
    POD_CHECK_LAUNCH();
    return POD_OK;
}

extern "C" int pod_ensemble_merge(const PodConfig* cfg, const int32_t* m_total, int32_t capacity, const float* boxes,
                                  const float* cov, const int32_t* classes, const float* probs, int32_t* seeds, int32_t* n_seeds,
                                  float* out_boxes, float* out_cov, float* out_scores, int32_t* out_classes, float* out_probs,
                                  pod_stream_t stream) {
    if (!cov) return POD_E_INVALID;
    pod::K6Params P;   // the seeds are the centres
    const int32_t centres = cluster_params(P, cfg, true, capacity, POD_MAX_CLASSES, m_total, seeds, n_seeds, boxes, cov, classes, probs,
                                           out_boxes, out_cov, out_scores, out_classes, out_probs);
    if (!centres) return POD_E_INVALID;
    P.n_keep_alloc = centres; P.ensemble_rule = 1;
    pod::KSeedParams S;
    S.m_total = m_total; S.capacity = capacity; S.aff = cfg->affinity_thresh; S.boxes = boxes; S.classes = classes; S.seeds = seeds;
    S.n_seeds = n_seeds;
    hipLaunchKernelGGL(pod::k_ensemble_seeds, dim3(1), dim3(1024), 0, (hipStream_t)stream, S);
    POD_CHECK_LAUNCH();
    hipLaunchKernelGGL(pod::k6_anchor_stats, dim3(centres), dim3(256), 0, (hipStream_t)stream, P);
    POD_CHECK_LAUNCH();
    return POD_OK;
}

extern "C" int pod_finalize(const PodConfig* cfg, const int32_t* keep, const int32_t* n_rows, const float* boxes,
                            const float* cov, const float* scores, const int32_t* classes, const float* probs,
                            float scale_x, float scale_y, float out_h, float out_w, float* det_boxes, float* det_cov,
                            float* det_scores, int32_t* det_classes, float* det_probs, float* records, int32_t* n_det,
                            pod_stream_t stream) {
    if (!cfg || !n_rows || !boxes || !scores || !classes || !probs || !det_boxes || !det_cov || !det_scores || !det_classes ||
        !det_probs || !n_det)
        return POD_E_INVALID;
    if (cfg->num_classes < 1 || cfg->num_classes > POD_MAX_CLASSES) return POD_E_INVALID;
    if (cfg->max_detections < 1 || cfg->max_detections > POD_MAX_DETECTIONS) return POD_E_INVALID;
    pod::K7Params P;
    P.keep = keep; P.n_rows = n_rows; P.boxes = boxes; P.cov = cov; P.scores = scores; P.classes = classes; P.probs = probs;
    P.K = cfg->num_classes; P.max_det = cfg->max_detections; P.sx = scale_x; P.sy = scale_y; P.out_h = out_h; P.out_w = out_w;
    P.det_boxes = det_boxes; P.det_cov = det_cov; P.det_scores = det_scores; P.det_classes = det_classes;
    P.det_probs = det_probs; P.records = records; P.n_det = n_det;
    hipLaunchKernelGGL(pod::k7_finalize, dim3(1), dim3(POD_MAX_DETECTIONS), 0, (hipStream_t)stream, P);
    POD_CHECK_LAUNCH();
    return POD_OK;
}

extern "C" int pod_reg_nll(const float* means, const float* covs, const float* gt, int32_t n, float* nll, pod_stream_t stream) {
    if (!means || !covs || !gt || !nll || n < 0) return POD_E_INVALID;
    if (n == 0) return POD_OK;
    hipLaunchKernelGGL(pod::k_reg_nll, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, means, covs, gt, n, nll);
    POD_CHECK_LAUNCH();
    return POD_OK;
}
