// K1f merge_score_fused -- merge AND score in ONE streaming launch (the production form of SURVEY 8 rows a3 + a4 since round 4).
//
// Replaces (reference, /root/reference/src/probabilistic_inference/probabilistic_inference.py):
//   :211-270  merge of the N MC-dropout runs / ensemble members of box_cls and box_cls_var (incl. the quirk of :216-222)
//   :289-297  classification sampling  mean_s sigmoid(logit + eps_s * sqrt(exp(var)))
//   :301,:304 max over classes and the score-threshold test (top-k itself is K2)
// i.e. what pod_mc_merge_score (prune mode) + pod_score_maybe do in two launches with a bitmap between them.
//
// Why the first fusion (round 3) lost and what is different here.  There a lane owned ONE class of its cells: an anchor that might
// pass had to be claimed, its other classes re-loaded from HBM (18 scattered loads per class lane) and scored by the wavefront that
// found it -- and flagged anchors are spatially clustered, so a few wavefronts carried all the scoring after everybody else had
// finished.  Here a LANE OWNS ALL K CLASSES OF ITS CELL(S): 2K accumulators stay in registers through the run loop
// (the run loop is outside, every load instruction of a wavefront still reads 1 KiB of one plane of one run: the streaming pattern
// of the flat kernel), the prune test runs on the merged values where they are, and nothing is ever re-loaded.  The cells that may
// pass are parked in LDS with their 2K merged values, and the WHOLE WORKGROUP -- whose wavefronts stream chunks that lie far apart
// in the level, so that a cluster of objects is spread over many workgroups -- scores the parked cells 8 lanes per cell (lane =
// class), by the scoring group K1b uses (score_group, pod_merge_score.h): the same keys, the same stored probabilities.  No bitmap,
// no second launch, no claim atomics; one aggregated global atomic per level and workgroup.
//
// Geometry at BASELINE size (R = 193 374, A = 9, K = 7, N = 10): ONE cell per lane -- 3 060 wave-units of 64 cells x one anchor shape,
// every lane with 2 runs x 14 planes = 28 independent non-temporal loads in flight, 12 wavefronts per CU.  (Four cells per lane --
// 16-byte loads, 765 wavefronts, less than one per SIMD -- walk their 9 runs as a chain of dependent round trips: 36 us; what hides the
// HBM latency is wavefronts in flight.  Measured on one box, planted image: K1 + K1b 24.7 + 11.9 us; this kernel 25.9 us, of which the
// streaming part alone 21 us -- profiles/r04_experiments.md.)  No MFMA: element-wise + reductions.

#include "pod_merge_score.h"

namespace pod {

// Launch geometry.  Twelve were measured (profiles/r05_k1f_variants.txt: cells per lane, runs in flight, occupancy, workgroup size); this is
// the fastest of them.
constexpr int K1F_WAVES = 4;   // wavefronts per workgroup (each streams its own, distant, chunk; all of them score the parked cells)
constexpr int K1F_WPE = 3;     // wavefronts per SIMD the register allocation aims at: 12 per CU = all 3 060 wavefronts of a BASELINE launch resident
constexpr int K1F_BATCH = 2;   // runs whose loads are in flight together: 2 x 2K loads per lane
constexpr int K1F_THREADS = 64 * K1F_WAVES;

struct K1fParams {
    PodLevel lv[POD_MAX_LEVELS];
    int32_t unit_begin[POD_MAX_LEVELS + 1];   // wave-units (anchor shape a, 64-cell chunk): level l = [unit_begin[l], unit_begin[l+1])
    int32_t chunks[POD_MAX_LEVELS];           // 64-cell chunks per anchor shape
    int32_t n_levels, n_runs, A, K, quirk, cls_samples;
    float score_thresh, skip_logit;
    uint64_t seed;
    float* mean_cls;         // merged planes, level-concatenated (level l at anchor_base_l * K), or null: not stored
    float* mean_cls_var;
    uint64_t* cand_keys;
    int32_t* cand_count;
    float* probs_dense;      // (R, K): the K probabilities of every anchor emitted, or null
};
struct K1fStat {
    float c, v;   // merged logit, merged log-variance of one class
};

// The accumulator merge_runs (pod_merge_score.h) walks: the 2K planes of one (anchor shape, cell) -- ONE cell per lane, 4-byte non-temporal
// loads (the runs are read exactly once), a wavefront instruction reads 64 contiguous floats of one plane of one run.  Fewer cells per
// lane = more wavefronts with fewer registers each: what hides the HBM latency here is wavefronts in flight, as in the flat kernel -- with
// 4 cells per lane the launch is 765 wavefronts, less than one per SIMD, and every one of them walks its 9 runs as a chain of dependent
// round trips (measured: 36 us against 25 for K1 alone).  add<CNT>: CNT runs x (1 or 2) tensors x K planes of independent loads, then
// the adds in the reference's order (run after run).  It REFERS to the caller's 2 x KP floats: owning them, it had the compiler fetch the
// level's pointers again before every pair of loads, and the runs of a batch waited for one another (profiles/merge_score_shared.md).
template <bool VAR, int KP>
struct K1fAcc {
    K1fStat (&m)[KP];
    const PodLevel& lv;
    int K;
    int64_t i0, plane_stride;   // element of plane (a, k = 0) in run 0; plane (a, k) is k * plane_stride further
    __device__ __forceinline__ void first() {
#pragma unroll
        for (int k = 0; k < KP; ++k) {
            m[k].c = m[k].v = 0.0f;
            if (k < K) {
                m[k].c = __builtin_nontemporal_load(lv.cls + (i0 + k * plane_stride));
                if (VAR) m[k].v = __builtin_nontemporal_load(lv.cls_var + (i0 + k * plane_stride));
            }
        }
    }
    __device__ __forceinline__ void twice() {
#pragma unroll
        for (int k = 0; k < KP; ++k) {
            m[k].c = m[k].c + m[k].c;
            m[k].v = m[k].v + m[k].v;
        }
    }
    template <int CNT>
    __device__ __forceinline__ void add(int run0) {
        K1fStat x[CNT][KP];
        const float *cls = lv.cls, *cls_var = lv.cls_var;      // fetched once per batch, not once per plane
        const int64_t rs = lv.run_stride_cls;
#pragma unroll
        for (int j = 0; j < CNT; ++j)
#pragma unroll
            for (int k = 0; k < KP; ++k)
                if (k < K) {
                    x[j][k].c = __builtin_nontemporal_load(cls + (int64_t)(run0 + j) * rs + (i0 + k * plane_stride));
                    if (VAR) x[j][k].v = __builtin_nontemporal_load(cls_var + (int64_t)(run0 + j) * rs + (i0 + k * plane_stride));
                }
#pragma unroll
        for (int j = 0; j < CNT; ++j)
#pragma unroll
            for (int k = 0; k < KP; ++k)
                if (k < K) {
                    m[k].c = m[k].c + x[j][k].c;
                    if (VAR) m[k].v = m[k].v + x[j][k].v;
                }
    }
    __device__ __forceinline__ void div(float d) {
#pragma unroll
        for (int k = 0; k < KP; ++k) {
            m[k].c = __fdiv_rn(m[k].c, d);
            m[k].v = __fdiv_rn(m[k].v, d);
        }
    }
};

template <int KP>
struct K1fLds {
    static constexpr int CAP = K1F_THREADS;          // every cell of the workgroup may be parked
    float val[CAP][2 * KP];                          // merged logits, merged log-variances of a parked cell
    int32_t meta[CAP][2];                            // level << 8 | a, hw
    uint64_t key[CAP];                               // keys above the threshold ...
    int32_t key_info[CAP];                           // ... level << 16 | rank inside (workgroup, level)
    int32_t n_parked, n_keys;
    int32_t lvl_count[POD_MAX_LEVELS], lvl_base[POD_MAX_LEVELS];
};

// Occupancy target: K1F_WPE wavefronts per SIMD for K <= 8 classes (2K accumulators + 2 runs x 2K loads in flight fit 170 registers);
// K > 8 (KP = 16) needs twice the registers per lane -- at 3 per SIMD it spilled 153 VGPRs to scratch (round 4) -- and runs 2 per SIMD.
template <int KP, bool VAR>
__global__ void __launch_bounds__(K1F_THREADS) __attribute__((amdgpu_waves_per_eu(KP <= 8 ? K1F_WPE : 2, KP <= 8 ? K1F_WPE : 2))) k1f_merge_score(const K1fParams P) {
    extern __shared__ __attribute__((aligned(16))) unsigned char k1f_lds_raw[];
    K1fLds<KP>& S = *reinterpret_cast<K1fLds<KP>*>(k1f_lds_raw);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int L = P.n_levels, K = P.K, A = P.A;
    if (tid == 0) {
        S.n_parked = 0;
        S.n_keys = 0;
    }
    if (tid < POD_MAX_LEVELS) S.lvl_count[tid] = 0;
    __syncthreads();

    // ---- stream: wavefront w of workgroup b takes wave-unit b + w * gridDim.x (units of one workgroup lie far apart) -----------------
    // (adjacent units instead, or rotating the quarters against each other so that the four units of a workgroup lie in different parts of
    //  the IMAGE as well: measured, no difference -- the 4 us this kernel takes beyond its streaming part are the barrier, one scoring
    //  round and the emission, not a cluster that piled up in one workgroup)
    const int u = (int)blockIdx.x + wave * (int)gridDim.x;
    if (u < P.unit_begin[L]) {
        const int l = find_segment(P.unit_begin, L, u);
        const PodLevel& lv = P.lv[l];
        const int local = u - P.unit_begin[l];
        const int a = local / P.chunks[l], chunk = local - a * P.chunks[l];
        const int HW = lv.H * lv.W;
        const int hw = chunk * 64 + lane;
        if (hw < HW) {
            const int64_t i0 = (int64_t)a * K * HW + hw;
            K1fStat m[KP];
            K1fAcc<VAR, KP> acc = {m, lv, K, i0, HW};
            merge_runs<K1F_BATCH>(acc, P.n_runs, P.quirk);
            if (P.n_runs > 1 && P.mean_cls) {
                const int64_t off = (int64_t)lv.anchor_base * K + i0;
#pragma unroll
                for (int k = 0; k < KP; ++k)
                    if (k < K) {
                        __builtin_nontemporal_store(m[k].c, P.mean_cls + off + (int64_t)k * HW);
                        if (VAR && P.mean_cls_var) __builtin_nontemporal_store(m[k].v, P.mean_cls_var + off + (int64_t)k * HW);
                    }
            }
            // prune test on the merged values where they are (may_pass: exact superset of the candidates)
            bool flag = false;
#pragma unroll
            for (int k = 0; k < KP; ++k)
                if (k < K && may_pass(m[k].c, m[k].v, VAR, P.skip_logit)) flag = true;
            // park the flagged cells with their 2K merged values
            const unsigned long long fm = __ballot(flag);
            if (fm != 0ull) {
                int base = 0;
                if (lane == (int)(__ffsll((long long)fm) - 1)) base = atomicAdd(&S.n_parked, __popcll(fm));
                base = __shfl(base, __ffsll((long long)fm) - 1, 64);
                if (flag) {
                    const int slot = base + __popcll(fm & ((1ull << lane) - 1ull));
                    S.meta[slot][0] = (l << 8) | a;
                    S.meta[slot][1] = hw;
#pragma unroll
                    for (int k = 0; k < KP; ++k) {
                        S.val[slot][k] = m[k].c;
                        S.val[slot][KP + k] = m[k].v;
                    }
                }
            }
        }
    }
    __syncthreads();

    // ---- score the parked cells: KP lanes per cell (lane = class), K1b's scoring group ----------------------------------------------
    const int total = S.n_parked;
    if (total == 0) return;
    const int k = tid % KP;
    for (int s0 = 0; s0 < total; s0 += K1F_THREADS / KP) {
        const int s = s0 + tid / KP;
        const bool valid = s < total;
        int l = 0, a = 0, hw = 0;
        float lg = 0.0f, vr = 0.0f;
        if (valid) {
            l = S.meta[s][0] >> 8;
            a = S.meta[s][0] & 0xFF;
            hw = S.meta[s][1];
            if (k < K) {
                lg = S.val[s][k];
                vr = S.val[s][KP + k];
            }
        }
        uint64_t key;
        if (score_group<KP>(P, lg, vr, VAR, valid, l, hw, a, k, key)) {
            const int rank = atomicAdd(&S.lvl_count[l], 1);
            const int at = atomicAdd(&S.n_keys, 1);
            S.key[at] = key;
            S.key_info[at] = (l << 16) | rank;
        }
    }
    __syncthreads();
    if (tid < L && S.lvl_count[tid] > 0) S.lvl_base[tid] = atomicAdd(&P.cand_count[tid], S.lvl_count[tid]);
    __syncthreads();
    for (int i = tid; i < S.n_keys; i += K1F_THREADS) {
        const int l = S.key_info[i] >> 16, at = S.lvl_base[l] + (S.key_info[i] & 0xFFFF);
        // (at < level size always holds when cand_count was zero on entry; the bound keeps a stale counter from writing into the next level's slots)
        if (at < P.lv[l].H * P.lv[l].W * A) P.cand_keys[(int64_t)P.lv[l].anchor_base + at] = S.key[i];
    }
}

}  // namespace pod

template <int KP, bool VAR>
static int k1f_launch(const pod::K1fParams& P, int units, hipStream_t stream) {
    constexpr size_t lds = sizeof(pod::K1fLds<KP>);
    if (pod_lds_opt_in<pod::k1f_merge_score<KP, VAR>>((int)lds) != POD_OK) return POD_E_LAUNCH;
    const int blocks = (units + pod::K1F_WAVES - 1) / pod::K1F_WAVES;
    hipLaunchKernelGGL((pod::k1f_merge_score<KP, VAR>), dim3(blocks), dim3(pod::K1F_THREADS), lds, stream, P);
    POD_CHECK_LAUNCH();
    return POD_OK;
}

extern "C" int pod_merge_score_fused(const PodConfig* cfg, const PodLevel* levels, float* mean_cls, float* mean_cls_var, uint64_t* cand_keys,
                                     int32_t* cand_count, float* probs_dense, pod_stream_t stream) {
    if (!cfg || !levels || !cand_keys || !cand_count) return POD_E_INVALID;
    const int L = cfg->n_levels, K = cfg->num_classes, A = cfg->num_anchors;
    if (!pod_merge_score_cfg_ok(cfg) || A > 255) return POD_E_INVALID;      // a: 8 bits of K1fLds::meta
    if ((mean_cls == nullptr) != (mean_cls_var == nullptr) && cfg->has_cls_var) return POD_E_INVALID;
    pod::K1fParams P;
    int32_t ub = 0;
    for (int l = 0; l < L; ++l) {
        const PodLevel& lv = levels[l];
        if (!lv.cls || lv.H < 1 || lv.W < 1 || lv.eps_cls) return POD_E_INVALID;      // native draws only: the prune bound needs |eps| < POD_EPS_MAX
        if (cfg->has_cls_var && !lv.cls_var) return POD_E_INVALID;
        const int64_t HW = (int64_t)lv.H * lv.W;
        if ((int64_t)A * K * HW >= (int64_t)1 << 31) return POD_E_INVALID;
        P.lv[l] = lv;
        P.chunks[l] = (int32_t)((HW + 63) / 64);
        P.unit_begin[l] = ub;
        ub += A * P.chunks[l];
    }
    P.unit_begin[L] = ub;
    P.n_levels = L; P.n_runs = cfg->n_runs; P.A = A; P.K = K; P.quirk = cfg->merge_quirk; P.cls_samples = cfg->cls_samples;
    P.score_thresh = cfg->score_thresh; P.seed = cfg->philox_seed; P.skip_logit = pod_prune_logit(cfg->score_thresh);
    P.mean_cls = mean_cls; P.mean_cls_var = mean_cls_var; P.cand_keys = cand_keys; P.cand_count = cand_count; P.probs_dense = probs_dense;
    const hipStream_t st = (hipStream_t)stream;
    if (cfg->has_cls_var) return K <= 8 ? k1f_launch<8, true>(P, ub, st) : k1f_launch<16, true>(P, ub, st);
    return K <= 8 ? k1f_launch<8, false>(P, ub, st) : k1f_launch<16, false>(P, ub, st);
}
