// K32 retinanet_inference -- detectron2's RetinaNet.inference for one image: what the reference model runs in EVAL mode.
//
// Replaces (reference, /root/reference/src/probabilistic_modeling/probabilistic_retinanet.py:156-166): `self.inference(box_cls, box_delta,
// anchors, images.image_sizes)` and `detector_postprocess(results_per_image, height, width)`, i.e. detectron2's
//   RetinaNet.inference_single_image : per level  box_cls_i.flatten().sigmoid_(), sort(descending)[:topk], > score_thresh,
//                                      anchor = idx // K, class = idx % K, Box2BoxTransform.apply_deltas; then cat over the levels,
//                                      batched_nms, [:max_detections_per_image]
//   detector_postprocess            : Boxes.scale, Boxes.clip, Boxes.nonempty
// This is the routine train_net.py:67-76 (`Trainer.test`, --eval-only, TEST.EVAL_PERIOD) evaluates -- not PI's probabilistic paths.
//
// Four kernels on one stream, three of them here:
//   k32_score        ONE streaming pass over cls (one read of 4 * R * K bytes; latency-, not bandwidth-bound at 5 MB): K1f's wave-units -- a wavefront owns (anchor shape a, 64
//                    cells), a lane ALL K classes of its cell, K independent non-temporal 4-byte loads in flight per lane, every load
//                    instruction of a wavefront reads 256 contiguous bytes of one plane -- and one 64-bit key per (anchor, class) above the
//                    threshold, appended through an LDS ticket per wavefront and ONE global ticket per workgroup and level.
//   k2_level_topk    (k2_topk_gather.hip, through pod_level_topk, unchanged) exact per-level top-k of the keys: its radix select + bitonic sort.
//   k32_decode       a thread per selected entry: f -> (anchor, class), four delta loads, apply_deltas, sigmoid of the key's own logit.
//   k4 (pod_nms_cluster, unchanged), then
//   k32_postprocess  one workgroup: scale, clip, drop empty boxes, compact in keep order.
//
// The ordering contract: rank by descending LOGIT, ties to the lower flat index f = (cell * A + a) * K + k.  sigmoid is
// monotone, so this is one of the orders detectron2's unstable sort of the scores may return, and the only deterministic one; where
// two different logits round to the same fp32 score detectron2 may order them either way, this kernel by the logit.
#include "pod_merge_score.h"

namespace pod {

constexpr int K32_WAVES = 16;                   // wavefronts per workgroup: 192 workgroups at BASELINE size, all resident, one global ticket each
constexpr int K32_THREADS = 64 * K32_WAVES;
constexpr int K32_DECODE_THREADS = 256;

// float -> unsigned with the same order (-0.0 and 0.0 are one value: torch compares them equal), and back.
__device__ __forceinline__ uint32_t order_bits(float x) {
    const uint32_t u = __float_as_uint(x + 0.0f);      // -0.0 + 0.0 = +0.0
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float order_value(uint32_t o) { return __uint_as_float((o & 0x80000000u) ? (o & 0x7FFFFFFFu) : ~o); }

struct K32ScoreParams {
    PodLevel lv[POD_MAX_LEVELS];
    int32_t unit_begin[POD_MAX_LEVELS + 1];   // wave-units (anchor shape a, 64-cell chunk): level l = [unit_begin[l], unit_begin[l+1])
    int32_t chunks[POD_MAX_LEVELS];           // 64-cell chunks per anchor shape
    int32_t n_levels, A, K;
    float score_thresh, skip_logit;
    uint64_t* cand_keys;                      // level l's list at anchor_base_l * K, H*W*A*K slots
    int32_t* cand_count;
};

template <int KP>
__global__ void __launch_bounds__(K32_THREADS) k32_score(const K32ScoreParams P) {
    __shared__ int32_t lvl_count[POD_MAX_LEVELS], lvl_base[POD_MAX_LEVELS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int L = P.n_levels, K = P.K, A = P.A;
    if (tid < POD_MAX_LEVELS) lvl_count[tid] = 0;
    __syncthreads();
    // wavefront w of workgroup b takes wave-unit b * K32_WAVES + w: a workgroup's units are neighbours, nearly always of one level
    const int u = (int)blockIdx.x * K32_WAVES + wave;
    const bool active = u < P.unit_begin[L];
    int l = 0, HW = 1, hw = 0, a = 0, c = 0, incl = 0, wave_at = 0;
    uint32_t pass = 0u;
    float x[KP];
    if (active) {
        l = find_segment(P.unit_begin, L, u);
        const PodLevel& lv = P.lv[l];
        const int local = u - P.unit_begin[l];
        a = local / P.chunks[l];
        HW = lv.H * lv.W;
        hw = (local - a * P.chunks[l]) * 64 + lane;
        const bool in = hw < HW;
        // the K logits of the anchor, read once: K independent loads before the first test
        const float* src = lv.cls + ((int64_t)a * K * HW + (in ? hw : 0));
#pragma unroll
        for (int k = 0; k < KP; ++k) {
            x[k] = -INFINITY;
            if (k < K) x[k] = __builtin_nontemporal_load(src + (int64_t)k * HW);
        }
        // candidate iff sigmoid(logit) > score_thresh in fp32; skip_logit lies safely below logit(score_thresh), so almost no entry pays the exp
#pragma unroll
        for (int k = 0; k < KP; ++k)
            if (k < K && in && x[k] >= P.skip_logit && sigmoid_ref(x[k]) > P.score_thresh) pass |= 1u << k;
        c = __popc(pass);
        incl = c;                               // inclusive scan of the lanes' counts
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int up = __shfl_up(incl, o, 64);
            if (lane >= o) incl += up;
        }
        const int total = __shfl(incl, 63, 64);
        // the list-append tickets: one LDS ticket per wavefront that found any, then ONE global ticket per workgroup and level (a global
        // ticket per wavefront -- 2 000 returning atomics on one address at BASELINE size -- serialised in the L2 and WAS the kernel: 40 us)
        if (lane == 0 && total > 0) wave_at = atomicAdd(&lvl_count[l], total);
        wave_at = __shfl(wave_at, 0, 64);
    }
    __syncthreads();
    if (tid < L && lvl_count[tid] > 0) lvl_base[tid] = atomicAdd(&P.cand_count[tid], lvl_count[tid]);
    __syncthreads();
    if (c == 0) return;
    int at = lvl_base[l] + wave_at + incl - c;
    const int cap = HW * A * K;                 // (at < cap always holds when cand_count was zero on entry; the bound keeps a stale counter inside the level's slots)
    uint64_t* list = P.cand_keys + (int64_t)P.lv[l].anchor_base * K;
    const uint32_t f0 = (uint32_t)(hw * A + a) * (uint32_t)K;
#pragma unroll
    for (int k = 0; k < KP; ++k)
        if ((pass >> k) & 1u) {
            if (at < cap) list[at] = ((uint64_t)order_bits(x[k]) << 32) | (uint64_t)(0xFFFFFFFFu - (f0 + (uint32_t)k));
            ++at;
        }
}

struct K32DecodeParams {
    PodLevel lv[POD_MAX_LEVELS];
    int32_t n_levels, A, K, n_capacity;
    float wts[4];
    const float* anchors;
    const uint64_t* cat_keys;
    const int32_t* cat_level;
    const int32_t* n_total;
    int32_t* cand_count;      // consumed (zeroed) here, as the gather kernels consume K1's
    int32_t* cand_flat;
    int32_t* cand_level;
    float* boxes;
    float* scores;
    int32_t* classes;
};

__global__ void __launch_bounds__(K32_DECODE_THREADS) k32_decode(const K32DecodeParams P) {
    const int i = (int)blockIdx.x * K32_DECODE_THREADS + (int)threadIdx.x;
    if (blockIdx.x == 0 && (int)threadIdx.x < P.n_levels) P.cand_count[threadIdx.x] = 0;
    const int n = *P.n_total;
    if (i >= n || i >= P.n_capacity) return;
    const uint64_t key = P.cat_keys[i];
    const int l = P.cat_level[i];
    const uint32_t f = 0xFFFFFFFFu - (uint32_t)key;
    float4 out = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    float score = 0.0f;
    int cls = 0;
    if (l >= 0 && l < P.n_levels) {
        const PodLevel& lv = P.lv[l];
        const int HW = lv.H * lv.W, A = P.A, K = P.K;
        if (f < (uint32_t)(HW * A * K)) {           // always, for a key the scoring pass wrote
            const int anchor = (int)(f / (uint32_t)K);
            cls = (int)f - anchor * K;
            const int hw = anchor / A, a = anchor - hw * A;
            const float* d = lv.delta + ((int64_t)a * 4 * HW + hw);
            const float d0 = d[0], d1 = d[HW], d2 = d[2 * (int64_t)HW], d3 = d[3 * (int64_t)HW];
            const Box anc = load_box(P.anchors, lv.anchor_base + anchor);
            const Box b = decode_box(d0, d1, d2, d3, anc, P.wts);
            out = make_float4(b.x1, b.y1, b.x2, b.y2);
            score = sigmoid_ref(order_value((uint32_t)(key >> 32)));
        }
    }
    *reinterpret_cast<float4*>(P.boxes + (int64_t)i * 4) = out;
    P.scores[i] = score;
    P.classes[i] = cls;
    P.cand_flat[i] = (int32_t)f;
    P.cand_level[i] = l;
}

struct K32PostParams {
    const int32_t* keep;
    const int32_t* n_keep;
    const float* boxes;
    const float* scores;
    const int32_t* classes;
    int32_t max_det, n_capacity;
    float sx, sy, oh, ow;
    float* det_boxes;
    float* det_scores;
    int32_t* det_classes;
    int32_t* n_det;
};

// detector_postprocess on the <= POD_MAX_DETECTIONS kept rows: one workgroup, thread = kept row.
__global__ void __launch_bounds__(POD_MAX_DETECTIONS) k32_postprocess(const K32PostParams P) {
    __shared__ int32_t wave_n[POD_MAX_DETECTIONS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = min(*P.n_keep, P.max_det);
    bool valid = false;
    Box b = {0.0f, 0.0f, 0.0f, 0.0f};
    int r = 0;
    if (tid < n) {
        r = P.keep[tid];
        if (r >= 0 && r < P.n_capacity) {
            b = load_box(P.boxes, r);
            b.x1 = fminf(fmaxf(b.x1 * P.sx, 0.0f), P.ow);      // Boxes.scale, then Boxes.clip
            b.x2 = fminf(fmaxf(b.x2 * P.sx, 0.0f), P.ow);
            b.y1 = fminf(fmaxf(b.y1 * P.sy, 0.0f), P.oh);
            b.y2 = fminf(fmaxf(b.y2 * P.sy, 0.0f), P.oh);
            valid = (b.x2 - b.x1) > 0.0f && (b.y2 - b.y1) > 0.0f;   // Boxes.nonempty(threshold = 0)
        }
    }
    const unsigned long long m = __ballot(valid);
    if (lane == 0) wave_n[wave] = __popcll(m);
    __syncthreads();
    int slot = __popcll(m & ((1ull << lane) - 1ull));
    int total = 0;
#pragma unroll
    for (int w = 0; w < POD_MAX_DETECTIONS / 64; ++w) {
        if (w < wave) slot += wave_n[w];
        total += wave_n[w];
    }
    if (valid) {
        *reinterpret_cast<float4*>(P.det_boxes + (int64_t)slot * 4) = make_float4(b.x1, b.y1, b.x2, b.y2);
        P.det_scores[slot] = P.scores[r];
        P.det_classes[slot] = P.classes[r];
    }
    if (tid == 0) *P.n_det = total;
}

}  // namespace pod

// ---- host ----------------------------------------------------------------------------------------------------------------------
// The cfg / geometry ranges every K32 entry point relies on; *keys_total = slots of the level-concatenated key buffer (R * K).
static bool k32_geometry_ok(const PodConfig* cfg, const PodLevel* levels, int64_t* keys_total) {
    const int L = cfg->n_levels, K = cfg->num_classes, A = cfg->num_anchors;
    if (L < 1 || L > POD_MAX_LEVELS || K < 1 || K >= POD_MAX_CLASSES || A < 1 || cfg->n_runs != 1) return false;
    if (cfg->topk < 1 || cfg->topk > POD_MAX_TOPK || (int64_t)L * cfg->topk > POD_MAX_CANDIDATES) return false;
    if (cfg->max_detections < 1 || cfg->max_detections > POD_MAX_DETECTIONS) return false;
    int64_t anchors = 0;
    for (int l = 0; l < L; ++l) {
        if (levels[l].H < 1 || levels[l].W < 1 || levels[l].anchor_base != anchors) return false;   // level-concatenated, no gaps: the lists tile the key buffer
        const int64_t r = (int64_t)levels[l].H * levels[l].W * A;
        if (r * K >= (int64_t)1 << 31) return false;
        anchors += r;
    }
    if (anchors * K >= (int64_t)1 << 31) return false;      // K2 addresses a level's list with a 32-bit offset
    if (keys_total) *keys_total = anchors * K;
    return true;
}

extern "C" int64_t pod_retinanet_infer_workspace(const PodConfig* cfg, const PodLevel* levels, PodRetinaNetLayout* layout) {
    int64_t keys = 0;
    if (!cfg || !levels || !k32_geometry_ok(cfg, levels, &keys)) return POD_E_INVALID;
    const int64_t n = (int64_t)cfg->n_levels * cfg->topk;
    PodRetinaNetLayout lo;
    int64_t off = 0;
    auto take = [&off](int64_t bytes) {
        const int64_t at = off;
        off += (bytes + 255) / 256 * 256;
        return at;
    };
    lo.cand_keys = take(8 * keys);
    lo.cand_count = take(4 * 2 * POD_MAX_LEVELS);
    lo.sel_keys = take(8 * n);
    lo.sel_count = take(4 * POD_MAX_LEVELS);
    lo.cat_keys = take(8 * n);
    lo.cat_level = take(4 * n);
    lo.n_total = take(4);
    lo.cand_flat = take(4 * n);
    lo.cand_level = take(4 * n);
    lo.boxes = take(16 * n);
    lo.scores = take(4 * n);
    lo.classes = take(4 * n);
    lo.keep = take(4 * POD_MAX_DETECTIONS);
    lo.n_keep = take(4);
    lo.nms_scratch = take((int64_t)pod_nms_scratch_bytes((int32_t)n));
    lo.total = off;
    if (layout) *layout = lo;
    return off;
}

extern "C" int pod_retinanet_score(const PodConfig* cfg, const PodLevel* levels, uint64_t* cand_keys, int32_t* cand_count, pod_stream_t stream) {
    if (!cfg || !levels || !cand_keys || !cand_count || !k32_geometry_ok(cfg, levels, nullptr)) return POD_E_INVALID;
    pod::K32ScoreParams P;
    int32_t ub = 0;
    for (int l = 0; l < cfg->n_levels; ++l) {
        if (!levels[l].cls) return POD_E_INVALID;
        P.lv[l] = levels[l];
        P.chunks[l] = (int32_t)(((int64_t)levels[l].H * levels[l].W + 63) / 64);
        P.unit_begin[l] = ub;
        ub += cfg->num_anchors * P.chunks[l];
    }
    P.unit_begin[cfg->n_levels] = ub;
    P.n_levels = cfg->n_levels; P.A = cfg->num_anchors; P.K = cfg->num_classes;
    P.score_thresh = cfg->score_thresh; P.skip_logit = pod_prune_logit(cfg->score_thresh);
    P.cand_keys = cand_keys; P.cand_count = cand_count;
    const int blocks = (ub + pod::K32_WAVES - 1) / pod::K32_WAVES;
    if (cfg->num_classes <= 8)
        hipLaunchKernelGGL(pod::k32_score<8>, dim3(blocks), dim3(pod::K32_THREADS), 0, (hipStream_t)stream, P);
    else
        hipLaunchKernelGGL(pod::k32_score<16>, dim3(blocks), dim3(pod::K32_THREADS), 0, (hipStream_t)stream, P);
    POD_CHECK_LAUNCH();
    return POD_OK;
}

extern "C" int pod_retinanet_topk(const PodConfig* cfg, const PodLevel* levels, uint64_t* cand_keys, int32_t* cand_count, uint64_t* sel_keys,
                                  int32_t* sel_count, uint64_t* cat_keys, int32_t* cat_level, int32_t* n_total, pod_stream_t stream) {
    if (!cfg || !levels || !k32_geometry_ok(cfg, levels, nullptr)) return POD_E_INVALID;
    // K2 finds level l's list at cand_keys + anchor_base_l: here a list holds K keys per anchor
    PodLevel lists[POD_MAX_LEVELS];
    for (int l = 0; l < cfg->n_levels; ++l) {
        lists[l] = levels[l];
        lists[l].anchor_base = levels[l].anchor_base * cfg->num_classes;
    }
    return pod_level_topk(cfg, lists, cand_keys, cand_count, sel_keys, sel_count, cat_keys, cat_level, n_total, stream);
}

extern "C" int pod_retinanet_decode(const PodConfig* cfg, const PodLevel* levels, const float* anchors, const uint64_t* cat_keys,
                                    const int32_t* cat_level, const int32_t* n_total, int32_t* cand_count, int32_t* cand_flat,
                                    int32_t* cand_level, float* boxes, float* scores, int32_t* classes, pod_stream_t stream) {
    if (!cfg || !levels || !anchors || !cat_keys || !cat_level || !n_total || !cand_count || !cand_flat || !cand_level || !boxes || !scores ||
        !classes || !k32_geometry_ok(cfg, levels, nullptr) || !pod_aligned(16, anchors, boxes))
        return POD_E_INVALID;
    pod::K32DecodeParams P;
    for (int l = 0; l < cfg->n_levels; ++l) {
        if (!levels[l].delta) return POD_E_INVALID;
        P.lv[l] = levels[l];
    }
    P.n_levels = cfg->n_levels; P.A = cfg->num_anchors; P.K = cfg->num_classes; P.n_capacity = cfg->n_levels * cfg->topk;
    for (int i = 0; i < 4; ++i) P.wts[i] = cfg->box_weights[i];
    P.anchors = anchors; P.cat_keys = cat_keys; P.cat_level = cat_level; P.n_total = n_total; P.cand_count = cand_count;
    P.cand_flat = cand_flat; P.cand_level = cand_level; P.boxes = boxes; P.scores = scores; P.classes = classes;
    const int blocks = (P.n_capacity + pod::K32_DECODE_THREADS - 1) / pod::K32_DECODE_THREADS;
    hipLaunchKernelGGL(pod::k32_decode, dim3(blocks), dim3(pod::K32_DECODE_THREADS), 0, (hipStream_t)stream, P);
    POD_CHECK_LAUNCH();
    return POD_OK;
}

extern "C" int pod_retinanet_postprocess(const PodConfig* cfg, const int32_t* keep, const int32_t* n_keep, const float* boxes,
                                         const float* scores, const int32_t* classes, float scale_x, float scale_y, float out_h, float out_w,
                                         float* det_boxes, float* det_scores, int32_t* det_classes, int32_t* n_det, pod_stream_t stream) {
    if (!cfg || !keep || !n_keep || !boxes || !scores || !classes || !det_boxes || !det_scores || !det_classes || !n_det) return POD_E_INVALID;
    if (cfg->max_detections < 1 || cfg->max_detections > POD_MAX_DETECTIONS || cfg->n_levels < 1 || cfg->n_levels > POD_MAX_LEVELS ||
        cfg->topk < 1 || cfg->topk > POD_MAX_TOPK || !pod_aligned(16, boxes, det_boxes))
        return POD_E_INVALID;
    pod::K32PostParams P;
    P.keep = keep; P.n_keep = n_keep; P.boxes = boxes; P.scores = scores; P.classes = classes;
    P.max_det = cfg->max_detections; P.n_capacity = cfg->n_levels * cfg->topk;
    P.sx = scale_x; P.sy = scale_y; P.oh = out_h; P.ow = out_w;
    P.det_boxes = det_boxes; P.det_scores = det_scores; P.det_classes = det_classes; P.n_det = n_det;
    hipLaunchKernelGGL(pod::k32_postprocess, dim3(1), dim3(POD_MAX_DETECTIONS), 0, (hipStream_t)stream, P);
    POD_CHECK_LAUNCH();
    return POD_OK;
}

#define K32_TRY(call)                  \
    do {                               \
        const int rc_ = (call);        \
        if (rc_ != POD_OK) return rc_; \
    } while (0)

extern "C" int pod_retinanet_infer_image(const PodConfig* cfg, const PodLevel* levels, const float* anchors, void* workspace, int32_t image_h,
                                         int32_t image_w, int32_t out_h, int32_t out_w, float* det_boxes, float* det_scores,
                                         int32_t* det_classes, int32_t* n_det, pod_stream_t stream) {
    if (!cfg || !levels || !anchors || !workspace || !det_boxes || !det_scores || !det_classes || !n_det) return POD_E_INVALID;
    if (image_h < 1 || image_w < 1 || out_h < 1 || out_w < 1 || !pod_aligned(16, workspace)) return POD_E_INVALID;
    PodRetinaNetLayout lo;
    if (pod_retinanet_infer_workspace(cfg, levels, &lo) < 0) return POD_E_INVALID;
    char* w = static_cast<char*>(workspace);
    uint64_t* cand_keys = reinterpret_cast<uint64_t*>(w + lo.cand_keys);
    int32_t* cand_count = reinterpret_cast<int32_t*>(w + lo.cand_count);
    uint64_t* cat_keys = reinterpret_cast<uint64_t*>(w + lo.cat_keys);
    int32_t* cat_level = reinterpret_cast<int32_t*>(w + lo.cat_level);
    int32_t* n_total = reinterpret_cast<int32_t*>(w + lo.n_total);
    float* boxes = reinterpret_cast<float*>(w + lo.boxes);
    float* scores = reinterpret_cast<float*>(w + lo.scores);
    int32_t* classes = reinterpret_cast<int32_t*>(w + lo.classes);
    int32_t* keep = reinterpret_cast<int32_t*>(w + lo.keep);
    int32_t* n_keep = reinterpret_cast<int32_t*>(w + lo.n_keep);
    K32_TRY(pod_retinanet_score(cfg, levels, cand_keys, cand_count, stream));
    K32_TRY(pod_retinanet_topk(cfg, levels, cand_keys, cand_count, reinterpret_cast<uint64_t*>(w + lo.sel_keys),
                               reinterpret_cast<int32_t*>(w + lo.sel_count), cat_keys, cat_level, n_total, stream));
    K32_TRY(pod_retinanet_decode(cfg, levels, anchors, cat_keys, cat_level, n_total, cand_count, reinterpret_cast<int32_t*>(w + lo.cand_flat),
                                 reinterpret_cast<int32_t*>(w + lo.cand_level), boxes, scores, classes, stream));
    K32_TRY(pod_nms_cluster(cfg, n_total, cfg->n_levels * cfg->topk, boxes, scores, classes, keep, n_keep, w + lo.nms_scratch, stream));
    // detector_postprocess: the scale factors are Python floats (doubles), rounded once to fp32 when they meet the fp32 boxes
    const float sx = (float)((double)out_w / (double)image_w), sy = (float)((double)out_h / (double)image_h);
    return pod_retinanet_postprocess(cfg, keep, n_keep, boxes, scores, classes, sx, sy, (float)out_h, (float)out_w, det_boxes, det_scores,
                                     det_classes, n_det, stream);
}
