/*
 * pod_mi355x.h -- C ABI of the MI355X-native probabilistic-inference hot path.
 *
 * Drop-in boundary for asharakeh/pod_compare's `probabilistic_inference` plugin
 * (reference files, relative to /root/reference/src):
 *   PI = probabilistic_inference/probabilistic_inference.py
 *   IU = probabilistic_inference/inference_utils.py
 *   MU = probabilistic_modeling/modeling_utils.py
 *   PR = probabilistic_modeling/probabilistic_retinanet.py
 *
 * Conventions
 *   - every pointer marked "dev" is a DEVICE pointer (HBM); everything else is host memory;
 *   - all floating point is fp32 (the COCO evaluation entries, K17: fp64), anchor indices int32, class ids int32 (the Python
 *     boundary widens them to the reference's int64);
 *   - outputs and scratch are caller-allocated; the library never allocates device memory,
 *     never synchronises the device and holds no global state; distinct streams may be used
 *     concurrently from distinct threads;
 *   - every entry point takes the `hipStream_t` to launch on (passed as `void*` so that this
 *     header needs no HIP include), is asynchronous and hipGraph-capturable, and returns
 *     0 on success or a negative POD_E_* code (it never throws across the ABI);
 *   - counts that are only known on the device (number of candidates, detections ...) live in
 *     device int32 words; kernels are launched for the worst case and exit early.
 *
 * HBM data layout
 *   dense head tensors, per FPN level l (what the conv head writes, NCHW, PR:486-537):
 *       cls, cls_var : (n_runs, A*K, H_l, W_l)      delta : (n_runs, A*4, H_l, W_l)
 *       reg_var      : (n_runs, A*D, H_l, W_l), D = 4 (diagonal) or 10 (full), MU:4-22
 *     run r of a tensor starts `run_stride` elements after run r-1 (MC-dropout runs batched
 *     on the batch dim, or ensemble members stacked / gathered over RCCL).
 *   reference anchor index inside a level (permute_to_N_HWA_K, PR:343-349):
 *       r = (h*W + w)*A + a,   channel of class k = a*K + k.
 *   "plane layout" outputs keep the input's (A*C, H, W) order (coalesced, no transpose).
 */
#ifndef POD_MI355X_H
#define POD_MI355X_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define POD_ABI_VERSION 18
#define POD_MAX_LEVELS 8
#define POD_MAX_CLASSES 16       /* K: BDD = 7 (Base-BDD-RetinaNet.yaml:11-12) */
#define POD_MAX_RUNS 64          /* MC-dropout runs / ensemble members */
#define POD_MAX_TOPK 2048        /* model.test_topk_candidates (detectron2 default 1000, PI:300) */
#define POD_MAX_PROP_SAMPLES 1024 /* PI:355 hard-codes 1000 */
#define POD_MAX_CLS_SAMPLES 64   /* CLS_VAR_LOSS.NUM_SAMPLES (10 in the reg_cls_var yamls) */
#define POD_MAX_CANDIDATES 8192  /* n = sum over levels of kept top-k; 5 x 1000 at BASELINE */
#define POD_MAX_DETECTIONS 128   /* model.max_detections_per_image (100) */
#define POD_COCO_MAX_IOU 16      /* COCO evaluation: IoU thresholds (pycocotools Params: 10) */
#define POD_COCO_MAX_REC 128     /*   recall thresholds (101) */
#define POD_COCO_MAX_AREA 4      /*   area ranges (all / small / medium / large) */
#define POD_COCO_MAX_MAXDET 4    /*   maxDets entries ([1, 10, 100]) */
#define POD_COCO_MAX_KEEP 128    /*   detections kept per (image, category): maxDets[-1] (100) */
#define POD_COCO_LDS_GT 64       /*   ground-truth boxes per (image, category) whose IoU matrix fits LDS; more use scratch */
#define POD_CALIB_MAX_EDGES 15   /* calibration pass: regression cdf edges (torch.arange(0, 1 - 1/15, 1/15) + 1/15: 14) */
#define POD_CALIB_BLOCK 1024     /*   sorted positions per block of the marginal-error bin counts */

#define POD_OK 0
#define POD_E_INVALID (-1)       /* bad argument / unsupported size */
#define POD_E_LAUNCH (-2)        /* HIP launch error (see hipGetLastError) */

typedef void* pod_stream_t;      /* hipStream_t */

/* One FPN level of the dense head output (device pointers, NCHW). */
typedef struct PodLevel {
    const float* cls;            /* dev (n_runs, A*K, H, W) logits               PR:352-361 'box_cls'     */
    const float* cls_var;        /* dev (n_runs, A*K, H, W) log-variances or NULL            'box_cls_var' */
    const float* delta;          /* dev (n_runs, A*4, H, W)                                   'box_delta'   */
    const float* reg_var;        /* dev (n_runs, A*D, H, W) or NULL                           'box_reg_var' */
    const float* eps_cls;        /* dev (cls_samples, H*W*A, K) replayed normals in REFERENCE layout, or NULL
                                    (NULL = in-kernel Philox4x32-10; replay is the parity mode)            */
    int64_t run_stride_cls;      /* elements between consecutive runs of cls / cls_var */
    int64_t run_stride_delta;
    int64_t run_stride_reg;
    int32_t H, W;
    int32_t anchor_base;         /* index of this level's first anchor in the level-concatenated order */
    int32_t reserved;
} PodLevel;

/* Static description of the path (model attributes + config keys). */
typedef struct PodConfig {
    int32_t n_levels;            /* <= POD_MAX_LEVELS */
    int32_t n_runs;              /* N >= 1; > 1 merges runs (PI:211-270) and adds epistemic covariance */
    int32_t num_anchors;         /* A (9) */
    int32_t num_classes;         /* K (7) */
    int32_t cov_dims;            /* D: 0 (no reg_var head), 4 or 10 */
    int32_t has_cls_var;         /* 0/1 */
    int32_t merge_quirk;         /* 1 = reference behaviour (2*x0+x1+..+x_{n-2})/n, PI:216-222; 0 = true mean */
    int32_t cls_samples;         /* model.cls_var_num_samples, PI:294 */
    int32_t prop_samples;        /* 1000, PI:355 */
    int32_t topk;                /* model.test_topk_candidates, PI:300 */
    int32_t max_detections;      /* model.max_detections_per_image */
    float score_thresh;          /* model.test_score_thresh, PI:304 */
    float nms_thresh;            /* model.test_nms_thresh */
    float affinity_thresh;       /* PROBABILISTIC_INFERENCE.AFFINITY_THRESHOLD */
    float box_weights[4];        /* Box2BoxTransform weights (cfg.MODEL.RPN.BBOX_REG_WEIGHTS, PI:175-176) */
    uint64_t philox_seed;        /* native-RNG mode only */
} PodConfig;

int pod_abi_version(void);

/* ---- K1  mc_merge_score -------------------------------------------------------------------
 * Replaces: the dense MC-dropout / ensemble merge PI:211-270, the classification sampling
 * PI:289-297 and the max-over-classes + score-threshold test PI:301-304.
 * Streams every run of every level once (coalesced 16-byte loads along W), writes the merged
 * tensors in plane layout (skipped when n_runs == 1 or the pointer is NULL) and appends one
 * 64-bit key per anchor whose score exceeds `score_thresh` to its level's candidate list:
 *     key = (float_bits(score) << 32) | (0xFFFFFFFF - r)      (descending key = score desc, r asc)
 * mean_* : dev, level-concatenated plane layout: level l starts at anchor_base_l * C elements.
 * cand_keys : dev uint64[R_total], level l's list starts at anchor_base_l.
 * cand_count: dev int32[2 * n_levels] (counts, then pod_level_topk's tickets), MUST be zero on entry
 *             (pod_reset_counters once after allocation; pod_gather_candidates / pod_gather_decode leave it zeroed again).
 * HBM-bound; algorithmic bytes per image = 4 * R * (2K + 4 + D) * (N + 1)  (SURVEY 8d). */
int pod_mc_merge_score(const PodConfig* cfg, const PodLevel* levels,
                       float* mean_cls, float* mean_cls_var, float* mean_delta, float* mean_reg_var,
                       uint64_t* cand_keys, int32_t* cand_count,
                       uint64_t* maybe_bits, pod_stream_t stream);

/* ---- K1b score_maybe ------------------------------------------------------------------------
 * Sparse companion of K1's prune mode (native RNG + cls_var head): when `maybe_bits`
 * (dev uint64[pod_maybe_words()] = one word per (anchor shape, class, 64 cells), all zero on entry; pod_score_maybe leaves it
 * zeroed again) is passed to pod_mc_merge_score, the dense pass
 * draws no samples; it writes a bitmap of the anchors that can still reach `score_thresh` under the sampler's
 * hard bound |eps| < 4.9 (an exact superset of the candidates) and this kernel evaluates
 * mean_s sigmoid(logit + eps_s*sigma) (PI:289-295) for those only, appending the keys of the anchors
 * above the threshold to `cand_keys` / `cand_count` exactly as K1 does otherwise. */
int64_t pod_maybe_words(const PodConfig* cfg, const PodLevel* levels);
/* probs_dense : dev float (R_total, K) in level-concatenated anchor order, or NULL: the K class probabilities of every anchor
 *               emitted here are stored at its row, so that the gather kernel does not evaluate them a second time. */
int pod_score_maybe(const PodConfig* cfg, const PodLevel* levels, const float* mean_cls, const float* mean_cls_var,
                    uint64_t* maybe_bits, uint64_t* cand_keys, int32_t* cand_count, float* probs_dense, pod_stream_t stream);

/* ---- K1f merge_score_fused (round 4): pod_mc_merge_score's prune mode + pod_score_maybe in ONE streaming launch ---------------
 * Replaces: PI:211-270 for box_cls / box_cls_var, PI:289-297, PI:301, PI:304 -- the job SURVEY 8 a3 + a4 defines ("merge and score").
 * Native draws only (every levels[l].eps_cls NULL: the prune bound needs the sampler's |eps| < 4.9); with or without a variance head.
 * A lane keeps all K classes of its 4 cells in registers through the run loop; cells that may pass are parked in LDS and scored by the
 * whole workgroup exactly as pod_score_maybe scores them: identical candidate keys (any order inside a level), identical probs_dense rows.
 * mean_cls / mean_cls_var : merged class planes as pod_mc_merge_score writes them, or both NULL: not stored (nothing downstream of the
 *                           product path reads them; the gather kernel merges box_delta / box_reg_var at the candidates).
 * cand_keys / cand_count / probs_dense : as for pod_mc_merge_score / pod_score_maybe (cand_count zero on entry).
 * HBM-bound; algorithmic bytes per image = 4 * R * 2K * (N - 1) read (quirk on) [+ 4 * R * 2K written when the planes are asked for]. */
int pod_merge_score_fused(const PodConfig* cfg, const PodLevel* levels, float* mean_cls, float* mean_cls_var, uint64_t* cand_keys,
                          int32_t* cand_count, float* probs_dense, pod_stream_t stream);

/* Zeroes `n` int32 device words on the stream (graph-capturable memset node). */
int pod_reset_counters(int32_t* counters, int32_t n, pod_stream_t stream);

/* ---- K2  level_topk ------------------------------------------------------------------------
 * Replaces: `predicted_prob.topk(num_topk)` + `> test_score_thresh` filter PI:300-308, per level.
 * Exact top-`topk` of each level's candidate list, sorted by descending key (ties: lower anchor
 * index first).  A level with at most POD_MAX_TOPK candidates: one workgroup, LDS bitonic sort.
 * A bigger level: 16 workgroups select the top-k of one slice each (MSB radix select + sort), the
 * last one to finish selects the final top-k from their survivors (no spinning).
 * sel_keys : dev uint64[n_levels * topk];  sel_count : dev int32[n_levels] (written).
 * cat_keys / cat_level / n_total (all three or none): the same selection level-concatenated -- row offset_l + i of cat_keys
 *   = sel_keys[l][i], cat_level its level, n_total = number of rows -- dev uint64 / int32 [n_levels * topk] / int32.  This is
 *   what the gather kernels read: one workgroup per row finds its key, its level and the row count with three independent loads.
 * cand_keys is CONSUMED (big levels are compacted in place); cand_count is only READ here -- pod_gather_candidates /
 * pod_gather_decode consume it (leave it ZERO, ready for the next image's pod_mc_merge_score; no pod_reset_counters between
 * images).  cand_count : dev int32[2 * n_levels]: the counts, then n_levels ticket words (zero on entry, left zero). */
int pod_level_topk(const PodConfig* cfg, const PodLevel* levels, uint64_t* cand_keys,
                   int32_t* cand_count, uint64_t* sel_keys, int32_t* sel_count,
                   uint64_t* cat_keys, int32_t* cat_level, int32_t* n_total, pod_stream_t stream);

/* ---- K2b gather_candidates -----------------------------------------------------------------
 * Replaces: the index gathers PI:305-338 and the level concatenation PI:341-342, 387-388.
 * Candidate i of the level-concatenated list gets: anchor index inside its level, level id,
 * score, class, K probabilities (recomputed bit-identically to K1), merged delta, merged
 * reg_var (D values), its anchor box and every run's raw delta (for the epistemic term).
 * anchors : dev (R_total, 4) level-concatenated XYXY anchors (PR:101).
 * cat_keys / cat_level / n_total : pod_level_topk's level-concatenated selection (read).
 * cand_count : the counters pod_mc_merge_score / pod_score_maybe appended with; ZEROED here (consumed).
 * probs_dense : the array pod_score_maybe filled (native draws + variance head), or NULL = evaluate the probabilities here. */
int pod_gather_candidates(const PodConfig* cfg, const PodLevel* levels, const float* anchors,
                          const uint64_t* cat_keys, const int32_t* cat_level, const int32_t* n_total,
                          int32_t* cand_count, const float* probs_dense,
                          int32_t* cand_anchor_idx, int32_t* cand_level, float* cand_score, int32_t* cand_class,
                          float* cand_probs, float* cand_delta, float* cand_reg_var, float* cand_anchor,
                          float* cand_run_delta /* (n, n_runs, 4) or NULL when n_runs == 1 */,
                          pod_stream_t stream);

/* ---- K3  decode_cov ------------------------------------------------------------------------
 * Replaces: covariance_output_to_cholesky MU:4-22, the 1000-sample propagation PI:344-368
 * (MVN rsample, SampleBox2BoxTransform.apply_samples_deltas IU:510-547,
 * compute_mean_covariance_torch IU:337-371), the epistemic covariance PI:323-331 (+= PI:369-374)
 * and the deterministic decode PI:375-385.  One wavefront per candidate; samples live in
 * registers; two-pass moments with the CPU reference's 16-row block summation order.
 * eps_prop : dev (prop_samples, n_replay, 4) replayed normals (reference layout) or NULL (Philox).
 * boxes : dev (n,4)   cov : dev (n,4,4) (zeros when the model has neither reg_var nor runs). */
int pod_decode_cov(const PodConfig* cfg, const PodLevel* levels, const int32_t* n_total, int32_t n_capacity,
                   const float* cand_delta, const float* cand_reg_var, const float* cand_anchor,
                   const float* cand_run_delta, const int32_t* cand_anchor_idx, const int32_t* cand_level,
                   const float* eps_prop, int32_t n_replay,
                   float* boxes, float* cov, pod_stream_t stream);

/* ---- K2b + K3 in one launch (in-kernel draws only) ------------------------------------------------
 * pod_gather_candidates followed by pod_decode_cov, same arguments, same outputs (the candidate arrays are still written
 * for the later kernels), bit-identical results: one 256-thread workgroup per candidate -- wavefront 0 gathers, all four draw
 * and decode the 1000 samples into LDS, wavefront 0 forms the moments in the reference's summation order; merged deltas /
 * log-variances / per-run deltas never leave LDS.  n_capacity = n_levels * topk. */
int pod_gather_decode(const PodConfig* cfg, const PodLevel* levels, const float* anchors, const uint64_t* cat_keys,
                      const int32_t* cat_level, const int32_t* n_total, int32_t* cand_count, const float* probs_dense,
                      int32_t* cand_anchor_idx, int32_t* cand_level, float* cand_score,
                      int32_t* cand_class, float* cand_probs, float* cand_delta, float* cand_reg_var, float* cand_anchor,
                      float* cand_run_delta, float* boxes, float* cov, pod_stream_t stream);

/* ---- K4  nms_cluster -----------------------------------------------------------------------
 * Replaces: detectron2 batched_nms -> torchvision coordinate-trick NMS (call sites PI:554-560,
 * IU:31-36, IU:83-89): boxes + class*(max_coord+1), stable descending-score order, suppress
 * iff IoU > nms_thresh, first `max_detections` survivors.
 * classes : dev int32[n] in [0, cfg->num_classes) (other ids are honoured, on a slower single-workgroup route).
 * keep : dev int32[max_detections] candidate indices in keep order;  n_keep : dev int32 (written).
 * scratch : dev, 16-byte aligned, pod_nms_scratch_bytes(n_capacity) bytes, ZEROED ONCE after allocation and then owned
 *           by this entry point (per-class survivor lists between the two launches; a call-generation word and the
 *           survivor scores the class sweeps publish to each other so that a class stops as soon as max_detections
 *           higher-scoring survivors exist overall).  boxes must be 16-byte aligned. */
size_t pod_nms_scratch_bytes(int32_t n_capacity);
int pod_nms_cluster(const PodConfig* cfg, const int32_t* n_total, int32_t n_capacity,
                    const float* boxes, const float* scores, const int32_t* classes,
                    int32_t* keep, int32_t* n_keep, void* scratch, pod_stream_t stream);

/* ---- K5  bayes_fuse ------------------------------------------------------------------------
 * Replaces: post_processing_bayes_od PI:562-636 + bounding_box_bayesian_inference IU:292-334.
 * One workgroup per kept centre: members = {j : IoU(centre, j) > affinity (pairwise_iou, Q8:
 * only the <=100 needed rows) and argmax(probs_j) == argmax(probs_centre)}; 4x4 SPD inverses
 * in fp64 registers, wavefront reductions of the precisions.
 * box_mode: 0 = bayesian_inference, 1 = covariance_intersection;
 * cls_mode: 0 = max_score (centre's score/class/probs), 1 = bayesian_inference (mean of member probs).
 * Degenerate cluster (no member, Q12): falls back to the centre's box/covariance.
 * out_* : dev, max_detections rows.
 * CAPACITIES: boxes / cov / scores / classes / probs must hold cfg->n_levels * cfg->topk rows and keep cfg->max_detections
 * entries, whatever *n_total / *n_keep say: the first rows are loaded in the same round trip as the counts (rows past the
 * counts are read, never used). */
int pod_bayes_fuse(const PodConfig* cfg, const int32_t* n_total, const int32_t* keep, const int32_t* n_keep,
                   const float* boxes, const float* cov, const float* scores, const int32_t* classes,
                   const float* probs, int32_t box_mode, int32_t cls_mode,
                   float* out_boxes, float* out_cov, float* out_scores, int32_t* out_classes, float* out_probs,
                   pod_stream_t stream);

/* ---- K6  anchor_stats_merge ----------------------------------------------------------------
 * Replaces: general_anchor_statistics_postprocessing IU:91-154 (cluster mean, residual outer
 * products / max(m-1,1), + mean member covariance when the net provides one, mean prob vector,
 * singleton rule IU:127-133, score/class re-derived from the merged prob vector IU:146-152).
 * cov may be NULL (no network covariance).
 * CAPACITIES as for pod_bayes_fuse: candidate arrays of cfg->n_levels * cfg->topk rows, keep of cfg->max_detections entries
 * (speculative loads run ahead of the counts). */
int pod_anchor_stats_merge(const PodConfig* cfg, const int32_t* n_total, const int32_t* keep, const int32_t* n_keep,
                           const float* boxes, const float* cov, const int32_t* classes, const float* probs,
                           float* out_boxes, float* out_cov, float* out_scores, int32_t* out_classes, float* out_probs,
                           pod_stream_t stream);

/* ---- post-NMS ensemble merge ---------------------------------------------------
 * Replaces: general_black_box_ensembles_post_processing IU:165-289 (callers PI:444-481 MC-dropout post-NMS,
 * PI:506-534 ensembles post-NMS).
 * pod_ensemble_append: appends rows keep[0:n_keep) of one member's standard-NMS result (IU:42-53) to the
 *   concatenated member arrays (torch.cat IU:191-196); `total` (dev int32, zero before the first member) is the
 *   running row count; cov == NULL appends zeros.
 * pod_ensemble_merge: sequential same-class clustering IU:203-215 (greedy sweep in index order, IoU >= affinity),
 *   then per-cluster mean box, residual covariance / (m-1) + mean member covariance, mean prob vector IU:223-247
 *   and score/class = max of the merged prob vector IU:262-263.  seeds/n_seeds: dev int32[capacity] / int32.
 *   out_*: dev, `capacity` rows (one per cluster).  The second NMS (IU:269-274) is pod_nms_cluster on the output
 *   with n_total = n_seeds, then pod_finalize gathers through its keep list. */
int pod_ensemble_append(const PodConfig* cfg, const int32_t* keep, const int32_t* n_keep, const float* boxes, const float* cov,
                        const int32_t* classes, const float* probs, int32_t capacity,
                        float* dst_boxes, float* dst_cov, int32_t* dst_classes, float* dst_probs, int32_t* total,
                        pod_stream_t stream);
int pod_ensemble_merge(const PodConfig* cfg, const int32_t* m_total, int32_t capacity, const float* boxes, const float* cov,
                       const int32_t* classes, const float* probs, int32_t* seeds, int32_t* n_seeds,
                       float* out_boxes, float* out_cov, float* out_scores, int32_t* out_classes, float* out_probs,
                       pod_stream_t stream);

/* ---- K7  finalize --------------------------------------------------------------------------
 * Replaces: the keep-gather of general_standard_nms_postprocessing IU:42-53 (when `keep` is
 * non-NULL rows are gathered through it; cov == NULL gives the zeros of IU:52-53) and
 * probabilistic_detector_postprocess IU:374-425 (scale, clip, drop empty boxes, cov + 1e-4 I,
 * S cov S^T).  Also emits, per detection, the XYWH box and T cov T^T of instances_to_json /
 * covar_xyxy_to_xywh IU:428-502 as a fixed-stride record:
 *     records[i] = { x, y, w, h, score, class, probs[K], cov_xywh[16] }   (6 + K + 16 floats)
 * det_* : dev, max_detections rows;  n_det : dev int32 (written). */
int pod_finalize(const PodConfig* cfg, const int32_t* keep, const int32_t* n_rows,
                 const float* boxes, const float* cov, const float* scores, const int32_t* classes,
                 const float* probs, float scale_x, float scale_y, float out_h, float out_w,
                 float* det_boxes, float* det_cov, float* det_scores, int32_t* det_classes, float* det_probs,
                 float* records, int32_t* n_det, pod_stream_t stream);

typedef struct PodDetections {     /* pod_finalize's outputs */
    float* boxes;  float* cov;  float* scores;  int32_t* classes;  float* probs;  float* records;  int32_t* n_det;
} PodDetections;

/* ---- conv-net side: fused ReLU + dropout -------------------------------------------------------
 * Replaces: the `nn.ReLU(), nn.Dropout(p)` pair after every 3x3 conv of the head subnets (PR:403-424) in
 * MC-dropout mode (PR:103-108), in place, one pass.  x: dev fp32, 16-byte aligned, n elements.
 * Element e uses 16 bits of the Philox4x32-10 call with counter (offset + e/8): keep iff field >= p * 2^16; pass a different
 * `offset` (or seed) per call. */
int pod_relu_dropout(float* x, int64_t n, float p, uint64_t seed, uint64_t offset, pod_stream_t stream);

/* ---- conv-net side: bias + residual + ReLU + dropout in one pass ------------------------------------
 * Replaces: the element-wise tail of every convolution of the model (PR:403-424 head subnets; detectron2's
 * ResNet bottleneck `relu(conv3(x) + shortcut(x))` and FrozenBN-folded `relu(conv(x) + b)` of the backbone):
 * x (N, C, H, W) fp32, in place:  x = dropout(relu((x + bias[c]) + (residual + res_bias[c])), p).
 * torch runs the conv bias as a separate add, then clamp, then dropout (2-4 passes over the activation); the
 * conv is called without bias and this is the only pass.  bias / residual / res_bias may be NULL, relu 0/1,
 * p = 0 disables dropout; Philox counters as pod_relu_dropout.  n = N*C*H*W, HW = H*W.
 * A channels-last (NHWC) activation is the same call with HW = 1 (channel = element index mod C). */
int pod_bias_act(float* x, const float* bias, const float* residual, const float* res_bias, int64_t n, int32_t C,
                 int64_t HW, int32_t relu, float p, uint64_t seed, uint64_t offset, pod_stream_t stream);

/* Same tail for a channels-last (N, H*W, C) conv output, written as NCHW planes: dst = dropout(relu(src + bias[c]), p)
 * transposed through LDS tiles, so leaving the channels-last trunk costs no extra pass.  C % 4 == 0, HW % 4 == 0,
 * src != dst; dropout counters are those of pod_bias_act on the NCHW result. */
int pod_bias_act_to_nchw(const float* src, float* dst, const float* bias, int64_t N, int32_t C, int64_t HW, int32_t relu,
                         float p, uint64_t seed, uint64_t offset, pod_stream_t stream);
/* The reverse layout change, for an NCHW conv (MIOpen) whose consumer is pod_wino_conv3x3: dst[(n*HW + hw)*C + c] =
 * act(src[(n*C + c)*HW + hw] + bias[c]), the bias + ReLU pass of detectron2's bottleneck conv1 (the reference model's
 * backbone, probabilistic_retinanet.py:20-60 via build_retinanet_resnet_fpn_backbone) writing channels-last.  C % 4 == 0. */
int pod_bias_act_to_nhwc(const float* src, float* dst, const float* bias, int64_t N, int32_t C, int64_t HW, int32_t relu,
                         pod_stream_t stream);

/* ---- conv-net side: broadcast + dropout -------------------------------------------------------------
 * Replaces: feeding the SAME first-conv activation to every MC run's `nn.Dropout(p)` (PR:104-106 replicates the feature
 * lists N times; PR:403-424).  dst[c][i] = dropout(src[i], p), c < copies, independent masks; n % 4 == 0, flat arrays
 * (any memory format shared by src and each copy).  * epoch (pod_expand_dropout, pod_wino_conv3x3, pod_wino_conv3x3_split; ABI 7): NULL, or a device word: the Philox key of the masks is then
 * seed ^ (*epoch * 0x9E3779B97F4A7C15).  seed and offset are launch arguments -- constants of a launch captured in a HIP graph -- so a
 * replayed MC-dropout forward bumps this word (one captured add at the start of the forward) to draw fresh masks for every image. */
int pod_expand_dropout(const float* src, float* dst, int64_t n, int32_t copies, float p, uint64_t seed, uint64_t offset,
                       const uint64_t* epoch, pod_stream_t stream);

/* ---- conv-net side: the head subnets' 3x3 convolutions -------------------------------------------------
 * Replaces: the `nn.Conv2d(256, 256, 3, padding=1), nn.ReLU(), nn.Dropout(p)` triples of cls_subnet / bbox_subnet
 * (probabilistic_retinanet.py:403-427) and their evaluation "for every MC run, for every FPN level" (PR:95-108, detectron2
 * RetinaNetHead.forward's loop over features): ONE launch covers all levels and all runs.  fp32 Winograd (F(2,3) down the rows, F(4,3) along
 * the columns: 24 multiply-adds per 2x4 outputs where the direct form has 72) on the fp32 matrix cores, bias + ReLU + dropout fused into the store.
 *
 * Activations are channels-last: in[pixel][C], out[pixel][K]; all images of the launch live in the two buffers.  `blocks`
 * (device, 16-byte aligned) holds n_blocks int32x4 records {first pixel of image 0 in `in`, first pixel of image 0 in `out`,
 * grid_cols << 24 | H << 12 | W, n_images << 24 | block_row << 12 | block_col}, one per 16x16-pixel block of a CANVAS of n_images
 * (1..127) consecutive H x W images (H, W < 4096) standing in a grid of grid_cols (1..255) columns: image i occupies canvas rows
 * (i / grid_cols) * (H + 1) .. + H - 1 and columns (i % grid_cols) * (W + 1) .. + W - 1 -- one zero row / column between neighbours,
 * the padding of both; block (r, c) covers canvas rows 16r.. and columns 16c.. and may lie across image borders (n_images = 1: the
 * plain ceil(H/16) x ceil(W/16) tiling of one image).  Blocks that touch no image need not be listed.
 * C % 8 == 0, K in {64, 128, 256, 512}.  U = pod_wino_filter_transform(weight): 24 * round_up(K, 64) * C floats; weight is
 * (K, C, 3, 3), output channels past K are zero (so a K = 63 predictor runs as K = 64; bias then has round_up(K, 64) entries).
 * k_planes == 0: out is channels-last.  k_planes > 0 (the predictor convs cls_score / bbox_pred / cls_var / bbox_cov,
 * PR:430-484): out is NCHW, image = k_planes planes of H*W starting at float `k_planes * first pixel`: the (N, A*K, H, W)
 * tensors pod_mc_merge_score streams; p must be 0.  Dropout: 16 Philox4x32-10 bits per element, keep iff field >= p * 2^16, counter
 * = offset + (flat index of the output element >> 3): the mask pod_bias_act draws on the same tensor. */
int pod_wino_filter_transform(const float* weight, float* U, int32_t K, int32_t C, pod_stream_t stream);
int pod_wino_conv3x3(const float* in, float* out, const float* U, const float* bias, const int32_t* blocks, int32_t n_blocks,
                     int32_t C, int32_t K, int32_t k_planes, int32_t relu, float p, uint64_t seed, uint64_t offset,
                     const uint64_t* epoch, pod_stream_t stream);

/* ---- operand abs-max records (round 5; ABI 12) ----------------------------------------------------------------------------------
 * The split convolutions below form every fp32 product from TWO F16 terms per operand; f16 has fp32's precision budget here (11 + 1 + 11
 * bits, pod_split_gemm.h) but not its range, so every operand tensor is scaled by a power of two derived from its abs-max.  Filters: static,
 * inside the *_filter_split transforms.  Activations: a device RECORD `in_amax` of POD_AMAX_FLOATS floats whose largest element is
 * >= max |x| over what the launch reads (only elements k * POD_AMAX_STRIDE, k < POD_AMAX_SLOTS, are read or written: producers spread
 * their atomics over 16 cache lines -- thousands of same-address atomics serialise in the L2) -- an upper bound is
 * enough (a looser bound costs low-order bits of tiny values only; a bound BELOW the true maximum overflows f16: the outputs are inf /
 * nan, never silently wrong).  Producers publish it: every pod_* convolution takes `out_amax` (NULL, or a device record it max'es
 * atomically with |every value it stores| -- the caller zeroes the record before the launch); pod_absmax computes it for any other tensor
 * (the same max'ing: zero the record first; x may itself be a record: that is how two bounds are joined).  A NaN is ignored by the max
 * (its products are nan in the consumer as they would be in fp32).  An inf is NOT: it enters the record as written, by pod_absmax and
 * by every producer alike, and the consumer then takes the smallest scale it has -- the products of the inf are inf / nan as they would
 * be in fp32, and the finite values of that tensor fall below f16's smallest number and are read as 0.0 by that launch. */
#define POD_AMAX_SLOTS 16
#define POD_AMAX_STRIDE 32
#define POD_AMAX_FLOATS (POD_AMAX_SLOTS * POD_AMAX_STRIDE)
int pod_absmax(const float* x, int64_t n, float* amax, pod_stream_t stream);

/* The same convolution with every fp32 product formed on the 16-BIT matrix cores (csrc/k12_wino_conv_split.hip).  Rounds 3-4: exact 3-way
 * bf16 splits, six partial products.  Round 5: 2-way F16 splits of the power-of-two-scaled operands, THREE partial products
 * (v_mfma_f32_32x32x16_f16, fp32 accumulate) -- half the matrix instructions, and measured against fp64 on the matrix cores a smaller
 * error than both the bf16 form and the fp32 MFMA (the fp32 accumulation chain is half as long; tools/f16_split_numerics.hip).
 * Us = pod_wino_filter_transform_split(weight): pod_wino_filter_split_bytes(K, C) bytes (2 * 24 * round_up(K, 64) * C f16 terms + a 16-byte
 * trailer holding the transformed filter's abs-max), 16-byte aligned.  C % 16 == 0.
 *
 * ONE entry for every form of the launch (rounds 3-4 exported pod_wino_conv3x3_split{,_replicas,_grouped,_partial}; they could not carry
 * the abs-max words and are gone -- ABI 12):
 *   - n_sets = 1..4 convolutions of ONE shape (C, K, relu, p, seed, epoch shared) in one grid: the cls- and the bbox-subnet layer l of the
 *     head (PR:403-427), their first layers with the replicas, the four predictors (PR:430-484).  The kernel runs one workgroup per CU,
 *     so a launch costs whole rounds of 256 workgroups: two launches of 1.5 rounds cost 4, one of 3.0 costs 3.  `blocks` = the sets' tables
 *     concatenated; set s owns blocks [sets[s].first_block, sets[s + 1].first_block) (first_block of set 0 = 0) and its records stay
 *     relative to ITS in / out.  Bit for bit the n_sets separate launches.
 *   - sets[s].replicas = r >= 1: the first conv of an MC-dropout subnet and the replication behind it (PR:403-427's first Conv2d + ReLU +
 *     Dropout under PR:95-108's run loop): every MC run sees the same features, so the conv is evaluated once and the store pass writes
 *     the runs' r (<= 127) dropout-masked copies -- replica i = image i of the record's output canvas (table: one input image per record,
 *     r output images).  Bit for bit p = 0 followed per level by pod_expand_dropout(copies = r, p, seed, offset + (index of the level's
 *     first output float) / 8, epoch).
 *   - sets[s].k_planes > 0: NCHW planes (the predictor convs); then p = 0 and no replicas.
 *   - n_splits > 1 (small maps; one set): a res5 convolution of the backbone is 48 workgroups of 32 chunks for 256 CUs.  The INPUT channels
 *     are cut into n_splits ranges of whole 32-channel super-chunks, one workgroup set each (grid.y): sets[0].out receives n_splits
 *     channels-last (out_pixels, K) arrays of partial sums (no bias / ReLU / dropout), split_stride floats apart; pod_wino_reduce /
 *     pod_reduce_partials add them in a fixed order. */
/* PodWinoConv.reserved: must be 0 (POD_E_INVALID otherwise).  Up to ABI 15 it was `form`, which selected a workgroup form of the kernel; the
 * eight-wavefront form was an experiment, measured 5 - 8 % slower and never shipped (profiles/r06_k16_two_wavefronts_per_simd.md). */
typedef struct PodConvSet {
    const float* in;        /* channels-last activations [pixel][C] */
    float* out;             /* channels-last [pixel][K], NCHW planes (k_planes > 0) or partial sums (n_splits > 1) */
    const void* Us;         /* pod_wino_filter_transform_split */
    const float* bias;      /* K floats (zero-padded) or NULL */
    const float* in_amax;   /* device record (POD_AMAX_FLOATS floats) bounding max |in| (see above); required */
    float* out_amax;        /* NULL, or a zeroed device record: max'ed with |every value stored| */
    uint64_t offset;        /* Philox offset of this set's dropout masks */
    int32_t first_block;    /* first record of the set in `blocks` */
    int32_t replicas;       /* 0: an ordinary launch; r >= 1: r masked replicas per input image */
    int32_t k_planes;       /* 0: channels-last out; > 0: NCHW planes of k_planes real channels */
    int32_t reserved;
} PodConvSet;
typedef struct PodWinoConv {
    const int32_t* blocks;  /* device, 16-byte aligned int32x4 records (pod_wino_conv3x3) */
    int32_t n_blocks, n_sets;
    int32_t C, K, relu;
    float p;                /* dropout rate of the store pass, [0, 1) */
    uint64_t seed;
    const uint64_t* epoch;  /* NULL or the device word folded into the Philox key (pod_expand_dropout) */
    int32_t n_splits;       /* <= 1: off */
    int32_t reserved;       /* 0 (see above) */
    int64_t split_stride;
    const int32_t* live_blocks; /* NULL, or pod_sparse_live_blocks' device list {count, ..., entries {record, need bits}}: only those records are
                                   computed, and the patch pixels whose need bit is clear are read as 0.0 */
    PodConvSet sets[4];
} PodWinoConv;
int64_t pod_wino_filter_split_bytes(int32_t K, int32_t C);
int pod_wino_filter_transform_split(const float* weight, void* Us, int32_t K, int32_t C, pod_stream_t stream);
int pod_wino_conv3x3_split(const PodWinoConv* conv, pod_stream_t stream);

/* ---- sparse bbox tower (round 5; csrc/k15_sparse_blocks.hip) ------------------------------------------------------------------------
 * probabilistic_inference.py:310-331 reads box_delta / box_reg_var only at the candidates of :300-308, while the head
 * (probabilistic_retinanet.py:518-537) evaluates bbox_subnet / bbox_pred / bbox_cov densely for every run.  With the cls tower evaluated
 * first: pod_sparse_reach turns pod_level_topk's selection into a per-cell map (one byte per cell of every level, level after level;
 * `scratch` as large) of how many convolution layers below the predictors a cell is still needed (0: a candidate's own cell .. 5; 255:
 * never -- Winograd tiles taken into account); pod_sparse_live_blocks lists the records of a pod_wino_conv3x3 table that hold a cell of
 * reach <= max_reach (rec_level[r] = FPN level of record r) for PodWinoConv.live_blocks: int32 word 0 = the count, then from word
 * POD_SPARSE_LIVE_HEAD one entry of POD_SPARSE_LIVE_STRIDE words per live record (order unspecified): {record index, 11 words of NEED
 * bits: bit 18 py + px <=> pixel (py, px) of the record's 18 x 18 input patch is an image cell of reach <= in_reach}.  The convolution
 * reads a patch pixel whose bit is clear as 0.0: with in_reach = max_reach + 1 (the reach the layer below was launched with; 255 for a
 * dense input) a launch never reads what an earlier image left in a buffer, every abs-max record is per image, and the tower's outputs
 * are a function of the image alone (ABI 14).  Needed cells depend on needed cells only: the detections equal the dense tower's (to the
 * last bits where an abs-max record differs in its binade). */
#define POD_SPARSE_LIVE_HEAD 4
#define POD_SPARSE_LIVE_STRIDE 12
int pod_sparse_reach(const PodConfig* cfg, const PodLevel* levels, const uint64_t* cat_keys, const int32_t* cat_level, const int32_t* n_total,
                     uint8_t* reach, uint8_t* scratch, pod_stream_t stream);
int pod_sparse_live_blocks(const PodConfig* cfg, const PodLevel* levels, const int32_t* records, const int32_t* rec_level, int32_t n_records,
                           const uint8_t* reach, int32_t max_reach, int32_t in_reach, int32_t* live, pod_stream_t stream);
/* pod_wino_reduce: the partial sums of an n_splits launch -> bias (K values, zero-padded) + ReLU -> the k_real planes of ONE NCHW image (HW =
 * out_pixels).  Replaces the same reference lines as pod_wino_conv3x3 (detectron2 BottleneckBlock.conv2, FPN.output_convs). */
int pod_wino_reduce(const float* partials, int32_t n_splits, int64_t split_stride, const float* bias, float* planes, int64_t HW,
                    int32_t K, int32_t k_real, int32_t relu, float* out_amax, pod_stream_t stream);

/* ---- the ResNet stem, channels-last (round 4; ABI 10; csrc/k14_stem_conv.hip) -------------------------------------------
 * Replaces detectron2's BasicStem as probabilistic_retinanet.py:96-100 runs it (`features = self.backbone(images.tensor)`):
 * conv1 (7x7, stride 2, padding 3, 3 -> 64 channels, FrozenBN folded into weight + bias) + ReLU, then max_pool2d(3, 2, 1).
 * pod_stem7x7_filter_split: weight (64, 3, 7, 7) fp32 -> Ws, 2 * 64 * 192 f16 values (the window padded to 8 x 8 with zeros, two f16
 * terms per scaled value) + a 16-byte trailer (the weight's abs-max): 64 * 192 * 4 + 16 bytes.  pod_stem7x7_split: x = the frame as (3, H_img, W_img) planes, fp32 or uint8 (x_is_u8); mean / stddev non-null:
 * the kernel normalises on load, (x - mean[c]) / stddev[c] in fp32 as PR:96's `self.normalizer` does (null: x is normalised already);
 * H x W >= H_img x W_img is the padded extent ImageList.from_tensors gives the frame (zeros outside the frame, as its padding and the
 * conv's own are) -> y ((H-1)/2+1) x ((W-1)/2+1) pixels x 64 channels, channels-last; every fp32 product from 2-way f16 splits of the
 * scaled operands (pod_conv1x1_split's arithmetic); in_amax: a device word >= max |normalised x| (operand abs-max words, above), out_amax:
 * NULL or the zeroed word that receives max |y|.  pod_maxpool3x3s2_cl: (H * W, C) channels-last -> ((H-1)/2+1) x ((W-1)/2+1) x C,
 * C % 4 == 0; taps outside the map do not take part (torch's -inf padding). */
int pod_stem7x7_filter_split(const float* weight, void* Ws, pod_stream_t stream);
int pod_stem7x7_split(const void* x, int32_t x_is_u8, int32_t H_img, int32_t W_img, const float* mean, const float* stddev, float* y, const void* Ws,
                      const float* bias, int32_t H, int32_t W, int32_t relu, const float* in_amax, float* out_amax, pod_stream_t stream);
int pod_maxpool3x3s2_cl(const float* x, float* y, int32_t H, int32_t W, int32_t C, pod_stream_t stream);
/* pod_im2col3x3s2_cl (ABI 13): the patch matrix of a 3x3 / stride 2 / padding 1 convolution on a channels-last map -- x (H * W, C) ->
 * y (((H-1)/2+1) * ((W-1)/2+1), 9 C), row (oy, ox) = the C-vectors of the nine taps in (ty, tx) order, zeros where a tap falls outside
 * the map; relu != 0: max(x, 0) on the way.  pod_conv1x1_split on y with the weight laid out (Cout, ty, tx, Cin) is then the convolution:
 * detectron2's LastLevelP6P7 (p6 = conv(res5), p7 = conv(relu(p6)); the last two convolutions of `self.backbone(images.tensor)`,
 * probabilistic_retinanet.py:96-100) without MIOpen, bit-reproducible run to run.  C % 4 == 0; an upper bound of |x| bounds |y|. */
int pod_im2col3x3s2_cl(const float* x, float* y, int32_t H, int32_t W, int32_t C, int32_t relu, pod_stream_t stream);

/* ---- ground-truth matching (offline metrics, SURVEY f-1) ------------------------------------------
 * Replaces: match_predictions_to_groundtruth core/evaluation_tools/evaluation_utils.py:191-367 for a whole data set
 * in one call.  Images are concatenated: image m owns detections [det_off[m], det_off[m+1]) and ground-truth boxes
 * [gt_off[m], gt_off[m+1]) (<= 128 detections per image); det_img / gt_img give the image slot of every row.
 * Outputs: gt_fn[g] = 1 iff every IoU <= iou_min (EU:245); gt_match_count[g] detections with IoU >= iou_correct, their
 * global indices / IoUs in gt_match_idx / gt_match_iou (n_gt x 128) ordered by descending max class probability
 * (entry 0 = the true positive, the rest duplicates, EU:282-299); det_fp[d] = 1 iff IoU <= iou_min with every
 * ground truth of its image (EU:255; an image without ground truth makes all its detections false positives).
 * Pinned by tests/eval_instrument: equal max class probabilities rank by lower detection index; entries of gt_match_idx / gt_match_iou at
 * rank >= gt_match_count[g] are not written; the IoU is detectron2's pairwise_iou in fp32, that operation order (bit-equal to a CPU
 * evaluation), compared as fp32 with >= iou_correct and <= iou_min; a detection may be the match of several boxes. */
int pod_match_groundtruth(const float* det_boxes, const float* det_probs, const int32_t* det_off, const int32_t* det_img,
                          int32_t n_det, const float* gt_boxes, const int32_t* gt_off, const int32_t* gt_img, int32_t n_gt,
                          int32_t num_classes, float iou_min, float iou_correct, int32_t* gt_fn, int32_t* gt_match_count,
                          int32_t* gt_match_idx, float* gt_match_iou, int32_t* det_fp, pod_stream_t stream);

/* ---- NLL scoring rule ----------------------------------------------------------------------
 * Replaces: compute_reg_scores core/evaluation_tools/scoring_rules.py:68-74
 * (-MVN(mean, cov + 1e-2 I).log_prob(gt), the "NLL parity" half of the metric). */
int pod_reg_nll(const float* means, const float* covs, const float* gt, int32_t n, float* nll, pod_stream_t stream);

/* ---- K17  COCO bbox evaluation (offline average precision) -------------------------------------
 * Replaces: pycocotools COCOeval.evaluate / evaluateImg (cocoeval.py, the per image x category x area-range greedy match) and
 * COCOeval.accumulate (the per category x area x maxDets x IoU-threshold precision / recall / score tables), which
 * compute_average_precision.py AP:41-43 runs for iouType 'bbox' with the default Params.  fp64 throughout, numpy's arithmetic:
 * the results equal a numpy restatement bit for bit.  summarize() and the F-1 threshold (AP:43-59) stay on the host. */
typedef struct PodCocoParams {
    int32_t n_iou, n_rec, n_area, n_maxdet;   /* T <= 16 (T * A <= 64), R <= 128, A <= 4, M <= 4 */
    int32_t n_cat;               /* K: evaluated category ids (params.catIds, AP:38) */
    int32_t reserved;
    double iou_thrs[POD_COCO_MAX_IOU];        /* np.linspace(.5, .95, 10), generated by the caller */
    double rec_thrs[POD_COCO_MAX_REC];        /* np.linspace(0, 1, 101), ascending */
    double area_rng[2 * POD_COCO_MAX_AREA];   /* [lo, hi] per range */
    int32_t max_dets[POD_COCO_MAX_MAXDET];    /* ascending; the last one cuts every (image, category) */
} PodCocoParams;

/* evaluateImg for every (image, category) pair with a ground-truth box or a detection, one workgroup each.
 * pairs   : dev int64[n_pairs][8] = {category index k, image position, gt_off, gt_n, dt_off, dt_n, out_off, scratch_off},
 *           sorted by (k, image position in sorted imgIds); a pair's boxes are contiguous, in annotation / result-file order.
 * dt_*    : dev, detections (xywh fp64 boxes, fp64 scores); gt_*: dev, ground truth (xywh, `area`, iscrowd, id).
 * scratch : dev, pairs with gt_n > POD_COCO_LDS_GT keep their IoU matrix at scratch + scratch_off,
 *           pod_coco_eval_scratch_bytes(min(dt_n, maxDets[-1]), gt_n) bytes (0 for the others).
 * kept_*  : dev, min(dt_n, maxDets[-1]) entries per pair at out_off, in score order: score, rank, and bit (a * T + t) of
 *           kept_match (matched to a ground-truth id != 0: pycocotools' dtm) and kept_ignore (dtIgnore).
 * npig    : dev int32[K * A], non-ignored ground truth per (category, area); zeroed by this call. */
size_t pod_coco_eval_scratch_bytes(int32_t n_keep, int32_t n_gt);
int pod_coco_eval_images(const PodCocoParams* prm, const int64_t* pairs, int32_t n_pairs, const double* dt_boxes,
                         const double* dt_score, const double* gt_boxes, const double* gt_area, const int32_t* gt_crowd,
                         const int64_t* gt_id, void* scratch, double* kept_score, uint64_t* kept_match, uint64_t* kept_ignore,
                         int32_t* kept_rank, int32_t* npig, pod_stream_t stream);

/* accumulate over pod_coco_eval_images' outputs.  cat_off: dev int64[K + 1], category k's kept detections are
 * [cat_off[k], cat_off[k+1]) (the pair order makes them contiguous); max_seg: the largest of those counts.
 * workspace: dev, pod_coco_accumulate_workspace_bytes(n_kept) bytes, 256-byte aligned.
 * precision, scores: dev fp64 [T][R][K][A][M]; recall: dev fp64 [T][K][A][M] (pycocotools' eval layouts, -1 where npig == 0). */
size_t pod_coco_accumulate_workspace_bytes(int64_t n_kept);
int pod_coco_accumulate(const PodCocoParams* prm, const int64_t* cat_off, int32_t max_seg, int64_t n_kept, const double* kept_score,
                        const uint64_t* kept_match, const uint64_t* kept_ignore, const int32_t* kept_rank, const int32_t* npig,
                        void* workspace, double* precision, double* recall, double* scores, pod_stream_t stream);

/* ---- K18  calibration pass (offline calibration errors) ----------------------------------------
 * Replaces the O(detections) work of compute_calibration_errors.py `calibration_errors` (CE:86-297).  Rows are the matched
 * partitions concatenated: true positives, then duplicates (n_matched rows with a ground truth), then false positives.  Integer
 * counts only cross workgroups; sums are in a fixed order: results are bit-identical run to run.  The O(classes x 4 x 14) tail
 * stays on the host with the host function's expressions. */

/* CE:86-103, CE:166-167, CE:263-276.  cls_probs dev (n, k1) fp32 (k1 - 1 classes + background), cov dev (n, 4, 4) fp32,
 * gt_class dev int32[n_matched]: the converted (contiguous) ground-truth class of the matched rows.
 * cls_entropy = -log(max of the first k1 - 1 columns); reg_entropy = entropy of MVN(0, cov + 1e-4 I) (4x4 Cholesky, fp32);
 * det_class = gt_class for matched rows, the first arg-max of those columns for false positives; class_count dev int32[POD_MAX_CLASSES]
 * rows per det_class, zeroed by this call. */
int pod_calib_keys(const float* cls_probs, int32_t k1, const float* cov, const int32_t* gt_class, int32_t n_matched, int32_t n,
                   float* cls_entropy, float* reg_entropy, int32_t* det_class, int32_t* class_count, pod_stream_t stream);

/* CE:206-261: cdf = Normal(mean_d, sqrt(cov_dd)).cdf(gt_d) of the matched rows, fp32 as torch computes it.  edges: host fp32[n_edges]
 * ascending (i + step).  counts dev int32[POD_MAX_CLASSES][4][n_edges + 1], zeroed by this call: bin j < n_edges counts the cdf values
 * below edge j but not below edge j - 1, bin n_edges the rest (NaN included); "cdf < edge i" is the prefix sum up to i. */
int pod_calib_reg_counts(const float* means, const float* cov, const float* gt, const int32_t* det_class, int32_t n_matched,
                         const float* edges, int32_t n_edges, int32_t* counts, pod_stream_t stream);

/* CE:160-178, CE:279-292: the minimum-uncertainty error of n_seg segments.  Segment s = [seg_off[s], seg_off[s + 1]) holds
 * class c = seg_class[s] >> 1 (key: cls_entropy if bit 0 is clear, else reg_entropy); its rows are those of det_class c in row
 * order, starting at class_off[c] (dev int32[POD_MAX_CLASSES], exclusive offsets of pod_calib_keys' counts).  perm: dev int64,
 * the host's torch.randperm draws at seg_off.  Gathered by perm, sorted stably by key, prefix counts of true positives (rows
 * < n_tp) and of the rest, errs = 0.5 (T - cumTP) / T + 0.5 cumFP / F in fp64; min_err dev fp64[n_seg]: the NaN-propagating min
 * (NaN for an empty segment).  max_seg: the longest segment, n_pos = seg_off[n_seg]; workspace: pod_calib_min_uncertainty_workspace_bytes(n, n_pos). */
size_t pod_calib_min_uncertainty_workspace_bytes(int32_t n, int64_t n_pos);
int pod_calib_min_uncertainty(const float* cls_entropy, const float* reg_entropy, const int32_t* det_class, int32_t n, int32_t n_tp,
                              const int32_t* class_off, const int64_t* seg_off, const int32_t* seg_class, int32_t n_seg, int32_t max_seg,
                              int64_t n_pos, const int64_t* perm, void* workspace, double* min_err, pod_stream_t stream);

/* CE:117-136 `calibration.get_calibration_error` as compute_calibration_errors.marginal_calibration_error restates it, in three calls
 * with the host choosing the path in between.  1) sort: scores dev fp32[n] -> sorted dev fp64[n] ascending, order dev int32[n] (stable).
 * 2) bin starts per block of POD_CALIB_BLOCK sorted positions, blk_cnt dev int32[ceil(n / POD_CALIB_BLOCK)]: edges == NULL, one bin per
 * distinct value (their sum is the number of distinct scores); else the bins of searchsorted(edges, v, 'left'), edges host fp64[n_edges <= POD_CALIB_MAX_EDGES].
 * 3) error: blk_off dev int64, exclusive offsets of blk_cnt, n_bins their total; labels dev int64[n] in {0, 1}; per bin fp64 sums of
 * labels and scores, bins with n < 2 or past the last edge (scores > 1.0 on the discrete path) skipped, the debiased L2 terms added in
 * bin order: total dev fp64[1] (the error is sqrt(max(total, 0))).  workspaces: pod_calib_marginal_*_workspace_bytes. */
size_t pod_calib_marginal_sort_workspace_bytes(int32_t n);
int pod_calib_marginal_sort(const float* scores, int32_t n, void* workspace, double* sorted, int32_t* order, pod_stream_t stream);
int pod_calib_marginal_bins(const double* sorted, int32_t n, const double* edges, int32_t n_edges, int32_t* blk_cnt, pod_stream_t stream);
size_t pod_calib_marginal_error_workspace_bytes(int32_t n_bins);
int pod_calib_marginal_error(const double* sorted, const int32_t* order, const int64_t* labels, int32_t n, const double* edges,
                             int32_t n_edges, const int64_t* blk_off, int32_t n_bins, void* workspace, double* total, pod_stream_t stream);

/* ---- K19  visualisation (annotated frames) ----------------------------------------------------
 * Replaces: ProbabilisticVisualizer.overlay_covariance_instances / draw_ellipse / cov_ellipse
 * (core/visualization_tools/probabilistic_visualizer.py PV:22-125, PV:127-195, PV:322-354) with detectron2's Visualizer.draw_box /
 * draw_text / VisImage underneath, as visualize_predictions.py (VP:62-142) and ProbabilisticPredictor.visualize_inference (PI:113-146)
 * drive them; matplotlib's rasteriser is replaced by the library's own.  Two calls:
 *
 * pod_vis_layout: one workgroup per list (one overlay_covariance_instances call), n = min(*count, max_n) instances (count NULL: max_n).
 *   out (dev, max_n rows of POD_VIS_INST_WORDS 4-byte words) receives them in DRAW ORDER: descending box area, ties by input index
 *   (PV:66-75), NaN areas last.  Words (i = int32, f = fp32):
 *     0 i input index | 1-4 f x0 y0 x1 y1 (frame pixels) | 5-7 f colour rgb | 8 f alpha
 *     9-12 i ellipse at (x0, y0): drawn (0 = a NaN, PV:155), width, height, rotation (int32-truncated, + 180: PV:156-158)
 *     13-16 i ellipse at (x1, y1): the same from cov[2:4, 2:4] | 17-20 f cos, sin of the two rotations
 *     21-22 f label anchor (frame pixels, PV:89-106) | 23 f font size in points before the scale (PV:108-116) | 24-26 f text colour
 *     27 f area | 28-31 zero.
 *   Colours: POD_VIS_COLOUR_ENTROPY = cm.autumn(binary entropy of the top probability, base 2) (VP:99-107); FIXED = colour[0..2];
 *   PALETTE = a fixed deterministic palette by input index (the reference's random_color is not reproducible); ARRAY = colours[input index].
 *   Ellipses: PV:70-86 sorts boxes, labels and colours by area but NOT covariance_matrices, so the box drawn k-th gets covariance k:
 *   POD_VIS_COV_BY_RANK reproduces that pairing, POD_VIS_COV_OWN gives every box its own covariance (cov[input index]).
 * pod_vis_render: one launch per POD_VIS_LAUNCH_FRAMES frames, one 16 x 16-pixel tile per workgroup.  The canvas (out_h, out_w, 3)
 *   uint8 RGB is the frame at `scale` (nearest, VisImage's imshow), or -- bilinear != 0 -- the source resampled to (frame_h, frame_w)
 *   first (cv2.resize of PI:135, fp32, rounded to uint8), then every instance of inst[0] and inst[1] (box, ellipse, ellipse; in that
 *   order), then the n_labels host-built label primitives (POD_VIS_PRIM_WORDS fp32 words each: kind (POD_VIS_LABEL_BOX: filled
 *   rectangle | POD_VIS_LABEL_GLYPH: atlas quad), X0 Y0 X1 Y1 in canvas pixels, r g b, alpha, atlas byte offset, glyph row length, 0),
 *   composited with dst += (colour - dst) alpha coverage.  Source pixel (y, x) channel c: src[y sy + x sx + c sc]; bgr: channel 0 is blue.
 *   stroke: line width in canvas pixels.  The layout's outputs must be complete (same stream) before the render reads them. */
#define POD_VIS_MAX_INSTANCES 256
#define POD_VIS_INST_WORDS 32
#define POD_VIS_PRIM_WORDS 12
#define POD_VIS_LAUNCH_LISTS 16
#define POD_VIS_LAUNCH_FRAMES 8
#define POD_VIS_COLOUR_ENTROPY 0
#define POD_VIS_COLOUR_FIXED 1
#define POD_VIS_COLOUR_PALETTE 2
#define POD_VIS_COLOUR_ARRAY 3
#define POD_VIS_COV_BY_RANK 0
#define POD_VIS_COV_OWN 1
#define POD_VIS_LABEL_BOX 3
#define POD_VIS_LABEL_GLYPH 4

typedef struct PodVisList {
    const float* boxes;          /* dev (n, box_stride) XYXY in frame pixels */
    const float* cov;            /* dev (n, cov_stride) row-major 4x4 corner covariances, or NULL: no ellipses */
    const float* probs;          /* dev (n, prob_stride): POD_VIS_COLOUR_ENTROPY takes the max of the first n_probs */
    const float* colours;        /* dev (n, colour_stride >= 3) rgb: POD_VIS_COLOUR_ARRAY */
    const int32_t* count;        /* dev int32 or NULL */
    float* out;                  /* dev (max_n, POD_VIS_INST_WORDS) */
    int32_t* n_out;              /* dev int32: n */
    int32_t max_n, box_stride, cov_stride, prob_stride, n_probs, colour_mode, colour_stride;
    int32_t cov_pairing;         /* POD_VIS_COV_BY_RANK (PV) or POD_VIS_COV_OWN */
    float colour[4];
    int32_t frame_h, frame_w;    /* the visualiser's image size (label rules, default font size) */
    float scale, alpha;
} PodVisList;

typedef struct PodVisFrame {
    const uint8_t* src;
    int64_t sy, sx, sc;
    int32_t src_h, src_w, bgr, bilinear;
    int32_t frame_h, frame_w, out_h, out_w;
    uint8_t* dst;                /* dev (out_h, out_w, 3) RGB */
    float scale, stroke;
    const float* inst[2];        /* pod_vis_layout outputs, or NULL */
    const int32_t* n_inst[2];    /* their n_out words */
    const float* labels;         /* dev (n_labels, POD_VIS_PRIM_WORDS), or NULL */
    const uint8_t* atlas;        /* dev glyph coverage (0..255) */
    int32_t n_labels, reserved;
} PodVisFrame;

int pod_vis_layout(const PodVisList* lists, int32_t n_lists, pod_stream_t stream);
int pod_vis_render(const PodVisFrame* frames, int32_t n_frames, pod_stream_t stream);

/* ---- K20  the loader's resize (uint8, PIL-exact) ------------------------------------------------
 * Replaces: what the reference's test loader does to a decoded frame on a host worker (AN:83-84, build_detection_test_loader ->
 * DatasetMapper(is_train=False): ResizeShortestEdge applied by ResizeTransform with PIL's Image.resize(BILINEAR) on the uint8 HWC array,
 * the RGB -> BGR flip of cfg.INPUT.FORMAT and the HWC -> CHW transpose), i.e. apply_net.CocoImages.__getitem__ after the decode.
 *
 * The arithmetic is Pillow's 8-bit separable resample: a horizontal pass into a uint8 intermediate, then a vertical pass; a pass is
 * skipped when its axis keeps its size.  Per axis (in -> out pixels), in fp64: scale = in / out, fs = max(scale, 1), support = fs,
 * ksize = (int)ceil(support) * 2 + 1; for output index i: center = (i + 0.5) scale, xmin = max((int)(center - support + 0.5), 0),
 * count = min((int)(center + support + 0.5), in) - xmin, weights w_x = max(1 - |(x + xmin - center + 0.5) / fs|, 0) normalised by their sum,
 * coefficient (int)(w 2^22 + 0.5).  A pixel of a pass is clip8((2^21 + sum pixel * coefficient) >> 22), summed in int32.  Integer
 * arithmetic on the device: the bytes are Pillow's.
 *
 * pod_resize_taps   (host only): ksize of one axis, or -1 when a size is < 1 or > POD_RESIZE_MAX_SIDE.
 * pod_resize_coeffs (host only): fills HOST arrays bounds[out][2] = (xmin, count) and coeffs[out][ksize] (zero beyond count).
 * pod_resize_frame_u8: one launch, one thread per output position.  src dev uint8 (in_h, in_w, 3) with rows `row_stride` bytes apart
 *   (>= 3 in_w); dst dev uint8 planar (3, out_h, out_w); flip_channels != 0: plane c receives source channel 2 - c (RGB -> BGR).
 *   xbounds / xcoeffs (dev, as pod_resize_coeffs(in_w, out_w) fills them, xk = its ksize) and ybounds / ycoeffs / yk for the rows.  Both
 *   tables of an axis NULL (and its k 0): the axis keeps its size and its pass is skipped; a table for an axis of equal size gives the
 *   same bytes (its coefficients are the identity).  A table entry that points outside the source is clamped to it, never followed.
 * Three new symbols under POD_ABI_VERSION 18: no entry or structure that existed changed, so the number stands. */
#define POD_RESIZE_MAX_SIDE 32768
int pod_resize_taps(int32_t in_size, int32_t out_size);
int pod_resize_coeffs(int32_t in_size, int32_t out_size, int32_t* bounds, int32_t* coeffs);
int pod_resize_frame_u8(const uint8_t* src, int32_t in_h, int32_t in_w, int64_t row_stride, const int32_t* xbounds, const int32_t* xcoeffs,
                        int32_t xk, const int32_t* ybounds, const int32_t* ycoeffs, int32_t yk, uint8_t* dst, int32_t out_h, int32_t out_w,
                        int32_t flip_channels, pod_stream_t stream);

/* ---- K21  training objective (csrc/k21_train_loss.hip) ----------------------------------------------
 * Replaces: the anchor labelling probabilistic_retinanet.py:129-130 calls (detectron2 RetinaNet.label_anchors with
 * Matcher(IOU_THRESHOLDS, [0, -1, 1], allow_low_quality_matches=True)) and ProbabilisticRetinaNet.losses, PR:168-333, evaluated at the
 * four head outputs together with their gradients.  No convolution has a backward pass: the gradients stop at the head outputs.
 * Three new symbols and one new structure under POD_ABI_VERSION 18, as for K20: no entry or structure that existed changed, so the number stands.
 *
 * pod_label_anchors: replaces PR:129-130.  anchors dev (R, 4) level-concatenated XYXY; images are concatenated as in pod_match_groundtruth:
 *   image i owns the boxes [gt_off[i], gt_off[i + 1]) of gt_boxes dev (n_gt, 4) XYXY / gt_classes dev int32[n_gt]; gt_off dev int32[n_images + 1].
 *   IoU = inter / ((area_gt + area_anchor) - inter) if inter > 0 else 0 (detectron2 pairwise_iou, fp32, that operation order: the labels
 *   equal a torch evaluation bit for bit).  Per anchor v = max over the image's boxes, m = the first arg-max; match = 1 if v >= iou_high,
 *   -1 if iou_low <= v < iou_high, else 0; then every anchor whose IoU with a box EQUALS that box's best IoU over all anchors gets match 1
 *   (literally, also when the best is 0; its m stays).  labels dev int32 (n_images, R): gt_classes[m] | num_classes (background) | -1
 *   (ignored); matched_gt dev int32 (n_images, R): m as a row of gt_boxes (-1 for an image without boxes, whose labels are all
 *   num_classes); num_pos dev int32[n_images]: labels in [0, num_classes).  scratch: dev, n_gt 4-byte words (the boxes' best IoUs, taken
 *   with an unsigned atomic max on the float's bits: IoU >= 0, a max is order-independent). */
int pod_label_anchors(const float* anchors, int32_t R, const float* gt_boxes, const int32_t* gt_classes, const int32_t* gt_off,
                      int32_t n_images, int32_t n_gt, int32_t num_classes, float iou_low, float iou_high, int32_t* labels,
                      int32_t* matched_gt, int32_t* num_pos, uint32_t* scratch, pod_stream_t stream);

/* pod_train_loss: replaces PR:168-333 (PR:194 get_deltas, PR:223-282 classification, PR:285-331 regression; the normaliser, the annealing
 *   weight and the division by the sample count, PR:201-203 / 268 / 320-322, are the caller's three weights).
 *   levels: the head outputs, cfg->n_runs = the IMAGE count and the run strides the image strides; cfg->cov_dims 0 or 4 (10: POD_E_INVALID,
 *   the reference defines no loss for the full covariance: pod_full_cov_loss, K28, below); cfg->num_classes <= 15.  labels / matched_gt dev int32 (n_images, R) as
 *   pod_label_anchors writes them, gt_boxes dev (n_gt, 4), anchors dev (R, 4), R = the levels' anchors.
 *   Classification, anchors with label >= 0, one-hot target without the background column: fvcore's sigmoid focal loss
 *   (p = sigmoid(x), ce = BCE-with-logits, p_t = p t + (1 - p)(1 - t), ce (1 - p_t)^gamma (alpha t + (1 - alpha)(1 - t)); alpha < 0: no
 *   alpha weight) of the logit, or -- cfg->has_cls_var -- summed over s < cfg->cls_samples at logit + sqrt(exp(logvar)) eps[s] (PR:231-268).
 *   eps_cls: dev (cls_samples, n_images * R, K) replayed normals, dense by anchor, or NULL: in-kernel Philox4x32-10 draws keyed by
 *   cfg->philox_seed and (image, anchor, class, sample); eps_out: NULL or a buffer of that shape receiving the normals used (zeros at
 *   ignored anchors).  Regression, anchors with label in [0, K): d = delta - get_deltas(anchor, gt_boxes[matched_gt]) with
 *   cfg->box_weights; smooth_l1 = |d| if beta < 1e-5, else 0.5 d^2 / beta below beta, else |d| - 0.5 beta; with cov_dims = 4 also
 *   0.5 exp(-c) smooth_l1 + 0.5 c, c = clamp(logvar, -7, 7) (PR:295-307).
 *   sums dev double[4]: classification sum, standard regression sum, NLL regression sum, positives.  fp32 terms accumulated in fp64 through
 *   per-workgroup partials (partials: dev double[pod_train_loss_partials(cfg, levels)]) added in a fixed order: the same bits every run.
 *   grads: NULL, or per level the planes (each NULL or laid out and strided exactly as the input of the same name) that receive
 *   d(w[0] cls_sum + w[1] std_reg_sum + w[2] nll_reg_sum) / d input, w dev float[3]; every element is written, exactly zero where an
 *   anchor contributes nothing; d clamp = 1 on [-7, 7], 0 outside. */
typedef struct PodLevelGrad {
    float* cls;  float* cls_var;  float* delta;  float* reg_var;
} PodLevelGrad;
int64_t pod_train_loss_partials(const PodConfig* cfg, const PodLevel* levels);
int pod_train_loss(const PodConfig* cfg, const PodLevel* levels, const PodLevelGrad* grads, const int32_t* labels,
                   const int32_t* matched_gt, const float* gt_boxes, int32_t n_gt, const float* anchors, int32_t R,
                   float alpha, float gamma, float smooth_l1_beta, const float* eps_cls, float* eps_out, const float* w,
                   double* partials, double* sums, pod_stream_t stream);

/* ---- K22  backward of the head's 3x3 convolutions (csrc/k22_conv3x3_wgrad.hip) ----------------------------------------
 * Serves: the backward pass of the convolutions of ProbabilisticRetinaNetHead (probabilistic_retinanet.py:403-484) under train_net.py's
 * training loop -- the reference gets it from autograd; here the weight and bias gradients are a kernel, the input gradient is a GEMM
 * (pod_conv1x1_split) of the gradient's patch matrix with the flipped, transposed filter.  Three new symbols under POD_ABI_VERSION 18, as for K20 / K21: no
 * entry or structure that existed changed, so the number stands.
 *
 * pod_conv3x3_wgrad: x dev (pixels, C) and dy dev (pixels, Kpad), channels-last, the images of a pod_wino_conv3x3 launch: level_hw HOST
 *   int32 (n_levels, 2) = (H, W) per level, `copies` images per level, level-major.  dW dev fp32 (K, C, 3, 3):
 *   dW[k][c][ky][kx] = sum over images and pixels of dy[(y, x)][k] x[(y + ky - 1, x + kx - 1)][c], taps outside the image contributing
 *   zero; db dev fp32 (K): the column sums of dy.  Channels K .. Kpad - 1 of dy are never used and nothing is written for them.
 *   C % 16 == 0, Kpad % 64 == 0, Kpad <= 512, K <= Kpad.  Every product is formed on the f16 matrix cores from the two-term f16 splits of
 *   BOTH operands, scaled by the powers of two their abs-max records give (x_amax / dy_amax: operand abs-max words, above), three partial
 *   products, fp32 accumulate.  The pixel reduction is cut into slices of 256 row segments of 16 pixels, enumerated by the geometry alone
 *   (level, image, column strip, row); each slice writes partial sums into `partials` (dev, 16-byte aligned,
 *   pod_conv3x3_wgrad_partials(...) floats; 0 = invalid geometry) and a second launch adds them in slice order in fp64 (db: fp64 column
 *   sums over chunks of 4096 pixels, added in chunk order): no atomics, two launches give the same bits.  POD_E_INVALID before any
 *   launch, as for every weight gradient (K22 - K24): a NULL pointer (db too, here); x, dy or partials off 16 bytes; a record, dW or db off
 *   4 bytes; dW, db or partials aliasing each other or an operand; more slices or chunks than a grid's x holds.
 * pod_relu_dropout_backward: the gate of conv + bias + ReLU + dropout(p) as pod_wino_conv3x3_split's store pass computes it: the stored
 *   output is relu(z) keep / (1 - p) with exact zeros where ReLU or the mask killed the element, so d_z = d_out (out > 0) / (1 - p)
 *   (1.0f / (1.0f - p) in fp32, the forward's factor).  n % 4 == 0; d_z may be d_out; dz_amax: NULL or the zeroed record that receives
 *   max |d_z|. */
int64_t pod_conv3x3_wgrad_partials(const int32_t* level_hw, int32_t n_levels, int32_t copies, int32_t C, int32_t K, int32_t Kpad);
int pod_conv3x3_wgrad(const float* x, const float* dy, const int32_t* level_hw, int32_t n_levels, int32_t copies, int32_t C, int32_t K,
                      int32_t Kpad, const float* x_amax, const float* dy_amax, float* dW, float* db, float* partials, pod_stream_t stream);
int pod_relu_dropout_backward(const float* out, const float* d_out, float* d_z, int64_t n, float p, float* dz_amax, pod_stream_t stream);

/* ---- K23  backward of the FPN (csrc/k23_fpn_backward.hip) ------------------------------------------------------------
 * Serves: the backward pass of detectron2's FPN + LastLevelP6P7 under train_net.py's training loop (the reference gets it from autograd).
 * The output convolutions are K22's; their input gradients and p7's run on pod_conv1x1_split.  What is new: a weight gradient whose
 * reduction runs over pixels with no taps, and the two gathers of the top-down path and of p7's input.  Four new symbols under
 * POD_ABI_VERSION 18, as for K20 - K22: no entry or structure that existed changed, so the number stands.
 *
 * pod_conv1x1_wgrad: x dev (pixels, C) and dy dev (pixels, K), channels-last fp32.  dW dev fp32 (K, C): dW[k][c] = sum over pixels of
 *   dy[p][k] x[p][c]; db dev fp32 (K) or NULL: the column sums of dy.  The weight gradient of a 1x1 convolution -- and, with x the patch
 *   matrix of pod_im2col3x3s2_cl, of a 3x3 / stride-2 one, laid out (K, ty, tx, Cin).  C % 16 == 0, C <= 18432, K % 64 == 0, K <= 512,
 *   pixels >= 1.  Arithmetic as pod_conv3x3_wgrad: every product on the f16 matrix cores from the two-term f16 splits of BOTH operands,
 *   scaled by the powers of two their abs-max records give (x_amax / dy_amax), three partial products, fp32 accumulate.  The pixels are cut
 *   into slices of 1024 pixels, halved down to 128 while slices x (K / 64) x ceil(C / 128) < 512 -- the geometry alone; each slice writes
 *   partial sums into `partials` (dev, 16-byte aligned, pod_conv1x1_wgrad_partials(...) floats; 0 = invalid geometry) and a second launch
 *   adds them in slice order in fp64 (db: fp64 column sums over chunks of 4096 pixels, added in chunk order): no atomics, two launches
 *   give the same bits.  POD_E_INVALID before any launch as pod_conv3x3_wgrad's (db may be NULL): NULL or misaligned pointers (16 bytes:
 *   x, dy, partials; 4 bytes: the records, dW, db), dW, db or partials aliasing each other or an operand.
 * pod_col2im3x3s2_cl: the input gradient of pod_im2col3x3s2_cl for one image.  dcols dev (Ho * Wo, 9 C), Ho = (H - 1) / 2 + 1,
 *   Wo = (W - 1) / 2 + 1, taps in (ty, tx) order; dx dev (H * W, C):
 *   dx[(y, x)][c] = (gate == NULL or gate[(y, x)][c] > 0 ? sum of dcols[(oy, ox)][(ty, tx, c)] over the taps with 2 oy + ty - 1 == y and
 *   2 ox + tx - 1 == x : 0) + (add == NULL ? 0 : add[(y, x)][c]) -- at most four terms, ty then tx ascending.  gate, add: dev (H * W, C);
 *   add may be dx.  C % 4 == 0.  dx_amax: NULL or the zeroed record that receives max |dx|.
 * pod_upsample2_sum_cl: the backward of `lateral + F.interpolate(top_down, scale_factor=2, mode="nearest")` towards top_down (the
 *   inverse of POD_C1_RESIDUAL_UP2).  d_child dev (h * w, C); add, d_top dev (((h + 1) / 2) * ((w + 1) / 2), C):
 *   d_top[(Y, X)] = add[(Y, X)] + sum of d_child[(y, x)] over y >> 1 == Y, x >> 1 == X, y < h, x < w, y then x ascending.  add may be
 *   d_top.  C % 4 == 0.  d_top_amax: NULL or the zeroed record that receives max |d_top|. */
int64_t pod_conv1x1_wgrad_partials(int64_t pixels, int32_t C, int32_t K);
int pod_conv1x1_wgrad(const float* x, const float* dy, int64_t pixels, int32_t C, int32_t K, const float* x_amax, const float* dy_amax, float* dW,
                      float* db, float* partials, pod_stream_t stream);
int pod_col2im3x3s2_cl(const float* dcols, const float* gate, const float* add, float* dx, int32_t H, int32_t W, int32_t C, float* dx_amax,
                       pod_stream_t stream);
int pod_upsample2_sum_cl(const float* d_child, int32_t h, int32_t w, const float* add, float* d_top, int32_t C, float* d_top_amax, pod_stream_t stream);

/* ---- K24  backward of the ResNet bottlenecks (csrc/k24_resnet_backward.hip) -------------------------------------------------
 * Serves: the backward pass of detectron2's BottleneckBlock (1x1 with STRIDE_IN_1X1, 3x3, 1x1, shortcut; FrozenBN) in res3 - res5 under
 * train_net.py:18-81 (`Trainer(DefaultTrainer)`, `trainer.train()`: every parameter above MODEL.BACKBONE.FREEZE_AT = 2 moves), behind
 * `self.backbone(images.tensor)` (probabilistic_retinanet.py:96-100); the reference gets it from autograd.  The 1x1 input gradients run on
 * pod_conv1x1_split with the transposed filter, the 3x3 ones on K22 and the patch-matrix GEMM, the gates on pod_relu_dropout_backward.
 * What is new: the 1x1 weight gradient at the backbone's widths and strides, and the input gradient of the stride's pixel selection.  Three
 * new symbols under POD_ABI_VERSION 18, as for K20 - K23: no entry or structure that existed changed, so the number stands.
 *
 * pod_conv1x1_wgrad_strided: x dev (images * H_in * W_in, C), dy dev (images * Ho * Wo, K), channels-last fp32, Ho = (H_in - 1) / stride + 1,
 *   Wo = (W_in - 1) / stride + 1.  dW dev fp32 (K, C):
 *   dW[k][c] = sum over (b, oy, ox) of dy[(b, oy, ox)][k] x[b H_in W_in + stride oy W_in + stride ox][c]; db dev fp32 (K) or NULL: the column
 *   sums of dy.  stride 1 or 2, C % 16 == 0, C <= 18432, K % 64 == 0, K <= 2048, images * H_in * W_in < 2^30.  Arithmetic, slices (of the
 *   images * Ho * Wo OUTPUT pixels), `partials` (pod_conv1x1_wgrad_strided_partials(...) floats, 16-byte aligned; 0 = invalid geometry) and
 *   the fixed-order fp64 second launch as pod_conv1x1_wgrad: on the same pixels the two give the same bits.  The rows a stride selects are
 *   gathered in the kernel's loads, never materialised.  Argument checks: pod_conv1x1_wgrad's.
 * pod_subsample2_scatter_cl: the input gradient of the stride-2 pixel selection for one image, with the gate and the sum the full map needs
 *   in the same pass.  d_small dev (Ho * Wo, C), Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1; gate, add, dx dev (H * W, C):
 *   dx[(y, x)][c] = (gate == NULL or gate[(y, x)][c] > 0) ? ((y and x even ? d_small[(y / 2) Wo + x / 2][c] : 0) + (add == NULL ? 0 :
 *   add[(y, x)][c])) : 0 -- `add` sits INSIDE the gate, unlike pod_col2im3x3s2_cl: the gate is the ReLU that closes the block whose output the
 *   map is.  add may be dx; dx may be neither d_small nor gate.  C % 4 == 0.  dx_amax: NULL or the zeroed record that receives max |dx|. */
int64_t pod_conv1x1_wgrad_strided_partials(int32_t images, int32_t H_in, int32_t W_in, int32_t stride, int32_t C, int32_t K);
int pod_conv1x1_wgrad_strided(const float* x, const float* dy, int32_t images, int32_t H_in, int32_t W_in, int32_t stride, int32_t C, int32_t K,
                              const float* x_amax, const float* dy_amax, float* dW, float* db, float* partials, pod_stream_t stream);
int pod_subsample2_scatter_cl(const float* d_small, const float* gate, const float* add, float* dx, int32_t H, int32_t W, int32_t C, float* dx_amax,
                              pod_stream_t stream);

/* ---- K25  the optimiser's step, every trained tensor in one launch (csrc/k25_sgd_step.hip) ------------------------------------
 * Serves: detectron2's build_optimizer / torch.optim.SGD (momentum, weight decay, one parameter group) under train_net.py's loop, together
 * with the two passes a FrozenBN-folded filter needs around it (W.grad = s dW' before, W' = W s after).  Two new symbols and one new
 * structure under POD_ABI_VERSION 18, as for K20 - K24: no entry or structure that existed changed, so the number stands.
 *
 * For every element i of every tensor of the table, in fp32, each operation rounded on its own:
 *     a  = scale ? scale[i / per_channel] * grad[i] : grad[i]
 *     g' = a + weight_decay * w[i];   m' = momentum * m[i] + g';   w' = w[i] - lr * m'
 *     m[i] = m';  w[i] = w';  if (folded) folded[i] = w' * scale[i / per_channel]
 * (zeroed momentum before the first step gives torch's first step, buf = g').  A tensor whose grad is NULL is skipped entirely -- no weight
 * decay, no momentum decay -- as torch skips a parameter without .grad.  w, grad, momentum, folded: dev fp32, n elements, 16-byte aligned,
 * no two overlapping; scale: dev fp32, n / per_channel floats (FrozenBN's s per OUTPUT channel), 16-byte aligned.
 * pod_sgd_chunk_map: the work list of a table -- per tensor ceil(n / POD_SGD_CHUNK) pairs (tensor, chunk of that tensor), int32, in table
 *   order -- written to HOST `map` if it is not NULL and holds `capacity` >= the result's pairs.  Returns the number of pairs, -1 for a
 *   table pod_sgd_step would refuse.  It depends on the n alone: built once per parameter set and kept on the device.
 * pod_sgd_step: `tensors` HOST (n_tensors descriptors; pinned memory makes the copy asynchronous), `tensors_dev` dev room for as many,
 *   `chunk_map` dev (n_chunks, 2) from pod_sgd_chunk_map of the same n.  Enqueues ONE host-to-device copy of the table and ONE launch on
 *   `stream`; no synchronisation, no read-back.  The caller leaves `tensors` unchanged until the copy has run (an event recorded after
 *   the call).  POD_E_INVALID before anything is enqueued: tensors NULL with n_tensors > 0, n_tensors < 0, a descriptor with w or momentum
 *   NULL, n < 0, a misaligned pointer, scale without per_channel > 0 or with n % per_channel != 0, folded without scale, folded == w,
 *   w == momentum, n_chunks other than the table's, lr / momentum / weight_decay not finite, momentum outside [0, 1), weight_decay < 0,
 *   tensors_dev or chunk_map NULL with n_chunks > 0.  n_tensors == 0, or every n == 0: POD_OK, nothing enqueued. */
#define POD_SGD_CHUNK 4096
typedef struct PodSgdTensor {
    float* w;  const float* grad;  float* momentum;  float* folded;  const float* scale;
    int64_t n;  int64_t per_channel;
} PodSgdTensor;
int64_t pod_sgd_chunk_map(const PodSgdTensor* tensors, int32_t n_tensors, int32_t* map, int64_t capacity);
int pod_sgd_step(const PodSgdTensor* tensors, PodSgdTensor* tensors_dev, int32_t n_tensors, const int32_t* chunk_map, int64_t n_chunks,
                 float lr, float momentum, float weight_decay, pod_stream_t stream);

/* ---- K26  the gradient bucket of data-parallel training, every gradient packed in one launch (csrc/k26_grad_bucket.hip) ----------
 * Serves: the gradient averaging of detectron2's launch + DistributedDataParallel under train_net.py -- one flat fp32 buffer that ONE
 * all-reduce averages and pod_sgd_step then steps from.  Two new symbols under POD_ABI_VERSION 18, no new structure: the table is K25's
 * PodSgdTensor (the pack reads `grad` and `n` alone; the rest only has to make a table pod_sgd_chunk_map accepts), cut by K25's chunk map.
 * pod_grad_bucket_layout: tensor t starts at the sum of the previous tensors' n, each rounded up to a multiple of 4 floats (every start is
 *   16-byte aligned), written to HOST `offsets` (n_tensors) if it is not NULL.  Returns the total number of floats, a multiple of 4; -1 for
 *   a table pod_sgd_chunk_map would refuse.  It depends on the n alone.
 * pod_grad_pack: bucket[offsets[t] + i] = scale * grad_t[i], fp32, one rounding.  `tensors` HOST (pinned memory makes the copy
 *   asynchronous), `tensors_dev` dev room for as many, `chunk_map` dev (n_chunks, 2) from pod_sgd_chunk_map and `offsets_dev` dev int64
 *   from pod_grad_bucket_layout of the same n, `bucket` dev, bucket_floats floats, 16-byte aligned.  Enqueues ONE host-to-device copy of
 *   the table and ONE launch on `stream`; no synchronisation, no read-back, no atomics: two launches give the same bits.  The caller leaves
 *   `tensors` unchanged until the copy has run, as for pod_sgd_step.  The padding floats between tensors are never written (the owner zeroes
 *   the bucket once).  POD_E_INVALID before anything is enqueued: a table pod_sgd_chunk_map refuses (a misaligned pointer among them), a
 *   tensor with n > 0 whose grad is NULL (every trained tensor has a gradient on every rank: not K25's skip), bucket overlapping a
 *   gradient, bucket_floats other than the layout's total, n_chunks other than the table's, scale not finite or <= 0, and with
 *   n_chunks > 0: bucket, tensors_dev, chunk_map or offsets_dev NULL, bucket misaligned.  n_tensors == 0, or every n == 0: POD_OK,
 *   nothing enqueued. */
int64_t pod_grad_bucket_layout(const PodSgdTensor* tensors, int32_t n_tensors, int64_t* offsets);
int pod_grad_pack(const PodSgdTensor* tensors, PodSgdTensor* tensors_dev, int32_t n_tensors, const int32_t* chunk_map, int64_t n_chunks,
                  const int64_t* offsets_dev, float* bucket, int64_t bucket_floats, float scale, pod_stream_t stream);

/* ---- K27  the box covariance trained with the energy score or by moment matching (csrc/k27_reg_score_loss.hip) ----------------
 * Serves: ProbabilisticRetinaNet.losses, probabilistic_retinanet.py:285-331, for BBOX_COV_LOSS.NAME `second_moment_matching` and
 * `energy_loss` -- names the reference's model YAMLs list (with NUM_SAMPLES = 1000, core/setup.py:107, read at PR:35) and its `losses`
 * refuses (PR:308-311); the reference defines neither, so the definitions are the ones below.  Either sum takes the NLL sum's place: the
 * caller divides it by the normaliser and mixes it with the standard regression loss by the annealing weight (PR:313-322) through w[2].
 * Two new symbols and three constants under POD_ABI_VERSION 18, as for K20 - K26: no entry or structure that existed changed, so the number
 * stands.
 *
 * Both losses act on the anchors with a label in [0, K) (and a matched box) and need the diagonal head.  Per anchor and coordinate j:
 * t = get_deltas(anchor, matched box) with cfg->box_weights, formed as pod_train_loss forms it; delta the predicted delta, lv the
 * predicted log-variance, c = clamp(lv, -7, 7) (d clamp = 1 on [-7, 7], 0 outside); sl1 = pod_train_loss's smooth-L1 term (|u| with
 * derivative sign(u), sign(0) = 0, below beta < 1e-5).
 *   POD_REG_LOSS_MOMENTS: d = delta - t, v = exp(c); loss = sum_j sl1(d_j) + sl1(v_j - d_j^2);
 *     d / d delta_j = sl1'(d_j) - 2 d_j sl1'(v_j - d_j^2) (the error is not detached);  d / d lv_j = sl1'(v_j - d_j^2) v_j 1[-7 <= lv_j <= 7].
 *   POD_REG_LOSS_ENERGY: M = num_samples, sigma = exp(0.5 c), z_s = delta + sigma eps_s for s = 0 .. M (M + 1 samples, eps iid N(0, 1));
 *     ES = (2 / M) sum_{s < M} sum_j sl1(z_sj - t_j)  -  (1 / M) sum_{s < M} sum_j sl1(sigma_j (eps_sj - eps_{s+1,j}))
 *     d / d delta_j = (2 / M) sum_s sl1'(u1),  u1 = (delta_j - t_j) + sigma_j eps_sj;
 *     d / d lv_j = 0.5 sigma_j [(2 / M) sum_s sl1'(u1) eps_sj - (1 / M) sum_s sl1'(u2) (eps_sj - eps_{s+1,j})] 1[-7 <= lv_j <= 7],
 *     u2 = sigma_j (eps_sj - eps_{s+1,j}), formed so and never as z_s - z_{s+1}: its sign is that of an exact fp32 difference.
 * pod_reg_score_loss: cfg / levels / labels / matched_gt / gt_boxes / anchors / R as pod_train_loss takes them (cfg->n_runs = the image
 *   count); every condition pod_train_loss refuses is refused here, and: cfg->cov_dims other than 4, a level without reg_var, `kind` outside
 *   {1, 2}, for the energy loss num_samples < 1 or > POD_MAX_REG_SAMPLES, eps_reg / eps_out off 16 bytes -- POD_E_INVALID before anything is
 *   enqueued.  sum dev double[1]: the loss over all positives of all images; fp32 terms accumulated in fp64, lanes -> wavefront butterfly ->
 *   workgroup -> partials[workgroup] (partials: dev double[pod_reg_score_partials(cfg, levels)]) -> one pass in index order.  No
 *   floating-point atomics: two launches give the same bits.
 *   grads: NULL, or the planes pod_train_loss has written earlier on the same stream (w: the same dev float[3]).  To each `delta` plane the
 *   launch adds w[2] d / d delta at the positive anchors -- one owner per element: load, add, store -- and touches no other element; it
 *   writes EVERY element of each `reg_var` plane, w[2] d / d lv at the positives and exact zeros elsewhere; cls / cls_var are ignored.
 *   Draws (energy loss): eps_reg NULL = in-kernel Philox4x32-10 normals on a stream word of their own, keyed by cfg->philox_seed and
 *   (image, anchor index within R, sample, coordinate) ALONE -- eight normals per call = the samples (2c, 2c + 1) of one anchor -- so a
 *   normal depends neither on the grid, nor on the batch size, nor on which other anchors are positive; or dev (num_samples + 1,
 *   n_images * R, 4) normals to replay, dense by anchor.  eps_out: NULL or a buffer of that shape receiving the normals used, zeros at every
 *   row that is not a positive anchor.  The dense arrays are a test and replay facility for small R: the product passes NULL for both. */
#define POD_REG_LOSS_MOMENTS 1
#define POD_REG_LOSS_ENERGY  2
#define POD_MAX_REG_SAMPLES  4096   /* BBOX_COV_LOSS.NUM_SAMPLES (1000 by default) */
int64_t pod_reg_score_partials(const PodConfig* cfg, const PodLevel* levels);
int pod_reg_score_loss(const PodConfig* cfg, const PodLevel* levels, const PodLevelGrad* grads, const int32_t* labels,
                       const int32_t* matched_gt, const float* gt_boxes, int32_t n_gt, const float* anchors, int32_t R,
                       int32_t kind, int32_t num_samples, float smooth_l1_beta, const float* eps_reg, float* eps_out,
                       const float* w, double* partials, double* sum, pod_stream_t stream);

/* ---- K28  the FULL box covariance trained: the Gaussian NLL, moment matching, the energy score (csrc/k28_full_cov_loss.hip) -----
 * Serves: ProbabilisticRetinaNet.losses, probabilistic_retinanet.py:285-331, for BBOX_COV_LOSS.COVARIANCE_TYPE `full` -- a choice the
 * reference's model YAMLs list (`'full', 'diagonal'`), whose ten-channel predictor it builds (PR:37-44) and whose output its inference turns
 * into a Cholesky factor (covariance_output_to_cholesky, MU:4-22), but for which its `losses` has no branch (PR:289 falls through, PR:322
 * dies on an unbound name).  The definitions are therefore the ones below, as K27's are.  One of the three sums takes the NLL sum's place
 * through w[2].  Two new symbols and three constants under POD_ABI_VERSION 18, as for K20 - K27: no entry or structure that existed
 * changed, so the number stands; pod_train_loss and pod_reg_score_loss refuse cfg->cov_dims = 10 as before.
 *
 * Per anchor with a label in [0, K) and a matched box (K27's selection): t = get_deltas(anchor, box) with cfg->box_weights, formed as
 * pod_train_loss forms it; d = delta - t; rv[0..9] the anchor's ten reg_var channels (channel a * 10 + j of a plane belongs to anchor
 * shape a); c_j = clamp(rv_j, -7, 7) for j < 4 (d clamp = 1 on [-7, 7], 0 outside); L lower triangular, L_jj = exp(0.5 c_j), its strict
 * lower triangle in torch.tril_indices(4, 4, -1) order T = (1,0) (2,0) (2,1) (3,0) (3,1) (3,2) = rv[4..9], unclamped -- the order
 * cholesky_from_head reads; sl1 / sl1' = pod_train_loss's smooth-L1 term and its derivative.  For all three kinds
 * d / d rv_j = 0.5 L_jj (d / d L_jj) 1[-7 <= rv_j <= 7] for j < 4 and d / d rv_{4+k} = d / d L_{T[k]}.
 *   POD_FULL_COV_NLL: the Gaussian's negative log-likelihood without its constant.  y solves L y = d (forward substitution, fp32,
 *     correctly rounded divisions), loss = 0.5 sum_j y_j^2 + 0.5 sum_j c_j; q solves L^T q = y;
 *     d / d delta_j = q_j;  d / d rv_j = 0.5 (1 - L_jj q_j y_j) 1[-7 <= rv_j <= 7] (j < 4);  d / d rv_{4+k} = - q_i y_j, (i, j) = T[k].
 *     This does NOT reduce to pod_train_loss's diagonal form (PR:298-304) at zero off-diagonals: that form puts a smooth-L1 term where the
 *     Gaussian has a square.  The diagonal path is unchanged.
 *   POD_FULL_COV_MOMENTS: Sigma = L L^T, E = Sigma - d d^T; loss = sum_j sl1(d_j) + sum_{i >= j} sl1(E_ij) (ten terms);
 *     m_ij = sl1'(E_ij) (i >= j), G = the symmetric extension of m plus diag(m_00 .. m_33);
 *     d / d delta_a = sl1'(d_a) - (G d)_a;  d / d L_ab = (G L)_ab for b <= a.
 *   POD_FULL_COV_ENERGY: M = num_samples, eps_s in R^4 for s = 0 .. M (iid N(0, 1));  u1_s = d + L eps_s,
 *     u2_s = L (eps_s - eps_{s+1}), formed from the exact fp32 difference of the normals and never as a difference of samples;
 *     ES = (2 / M) sum_{s < M} sum_j sl1(u1_sj)  -  (1 / M) sum_{s < M} sum_j sl1(u2_sj);
 *     d / d delta_j = (2 / M) sum_s sl1'(u1_sj);
 *     d / d L_jk = (2 / M) sum_s sl1'(u1_sj) eps_sk - (1 / M) sum_s sl1'(u2_sj) (eps_sk - eps_{s+1,k}) for k <= j.
 * pod_full_cov_loss: pod_reg_score_loss's argument list, same order and meaning.  It refuses everything pod_reg_score_loss refuses, except
 *   that it requires cfg->cov_dims == 10 (4 and 0: POD_E_INVALID) and `kind` in {1, 2, 3}; num_samples is checked for the energy kind only.
 *   POD_E_INVALID before anything is enqueued.  sum dev double[1]; partials: dev double[pod_full_cov_partials(cfg, levels)]; fp32 terms
 *   accumulated in fp64, lanes -> wavefront butterfly -> workgroup -> partials[workgroup] -> one pass in index order.  No floating-point
 *   atomics: two launches give the same bits.
 *   grads: NULL, or the planes pod_train_loss has written earlier on the same stream, run with cov_dims = 0 and no reg_var (w: the same dev
 *   float[3]).  To each `delta` plane the launch adds w[2] d / d delta at the positive anchors -- one owner per element: load, add, store
 *   -- and touches no other element; it writes EVERY element of each ten-channel `reg_var` plane, w[2] d / d rv at the positives and
 *   exact zeros elsewhere; cls / cls_var are ignored.
 *   Draws (energy kind): K27's -- the same stream word, keyed by cfg->philox_seed and (image, anchor index within R, sample pair) alone, so
 *   under one seed an anchor sees the normals pod_reg_score_loss would give it; eps_reg / eps_out: dense (num_samples + 1, n_images * R, 4),
 *   as for K27. */
#define POD_FULL_COV_NLL     1
#define POD_FULL_COV_MOMENTS 2
#define POD_FULL_COV_ENERGY  3
int64_t pod_full_cov_partials(const PodConfig* cfg, const PodLevel* levels);
int pod_full_cov_loss(const PodConfig* cfg, const PodLevel* levels, const PodLevelGrad* grads, const int32_t* labels,
                      const int32_t* matched_gt, const float* gt_boxes, int32_t n_gt, const float* anchors, int32_t R,
                      int32_t kind, int32_t num_samples, float smooth_l1_beta, const float* eps_reg, float* eps_out,
                      const float* w, double* partials, double* sum, pod_stream_t stream);

/* ---- K29  the optimiser's step under the whole SOLVER section: clipping, parameter groups, Nesterov, a guard (csrc/k29_sgd_solver.hip) ----
 * Serves: detectron2's build_optimizer with SOLVER.NESTEROV, BIAS_LR_FACTOR, WEIGHT_DECAY_BIAS and CLIP_GRADIENTS.* (maybe_add_gradient_clipping:
 * `value` and `norm` per parameter tensor; `full_model`: one norm over all of them) and the trainer's stop at the first non-finite loss, on
 * K25's table and chunk map.  Four new symbols, two new structures and four constants under POD_ABI_VERSION 18, as for K20 - K28: no entry or
 * structure that existed changed, so the number stands.  pod_sgd_step, pod_sgd_chunk_map, pod_grad_pack and PodSgdTensor are what they were.
 *
 * For every element i of every tensor t of the table with a gradient, G = group[t], in fp32, each operation rounded on its own:
 *     a0 = scale ? scale[i / per_channel] * grad[i] : grad[i]                       (K25's)
 *     a  = a0                                          clip_type POD_SGD_CLIP_OFF
 *        | a0 < -v ? -v : a0 > v ? v : a0              POD_SGD_CLIP_VALUE, v = clip_value (a NaN stays a NaN)
 *        | coef[t] * a0                                POD_SGD_CLIP_NORM
 *        | coef[n_tensors] * a0                        POD_SGD_CLIP_FULL_MODEL
 *     g' = a + wd[G] * w[i];   m' = momentum * m[i] + g';   d = nesterov ? g' + momentum * m' : m';   w' = w[i] - lr[G] * d
 *     m[i] = m';  w[i] = w';  if (folded) folded[i] = w' * scale[i / per_channel]
 * With N_t^2 = sum_i a0_i^2: coef[t] = (float)c, c = clip_value / (sqrt(N_t^2) + 1e-6) in fp64, replaced by 1 where c > 1 (a NaN stays a NaN:
 * torch's clip_grad_norm_, which always multiplies); coef[n_tensors] the same of N^2 = sum_t N_t^2 over the tensors with a gradient.  A
 * tensor whose grad is NULL is in no norm, has coef 1 and is not stepped.  The squares and sums are fp64, of the fp32 a0, in an order that
 * does not depend on the grid: per chunk of POD_SGD_CHUNK elements each lane in index order, wave_sum over the 64 lanes, the four
 * wavefronts in order; a tensor's chunks in chunk order; the tensors in table order.  fp32 squares summed in fp64 cannot overflow: a finite
 * gradient has a finite norm.
 * The guard: a step is BAD when the N_t^2 of a tensor with a gradient, or a watched scalar, is not finite.  A bad step counts in
 * status.bad_steps, the first one's `iteration` stays in status.first_bad_iteration; with `guard` set it also sets status.poisoned, and
 * the step kernel of a poisoned workspace returns before its first store -- that step and every later one write no weight, momentum or
 * folded filter, and leave the status as it is, until pod_sgd_solver_reset.  Nothing is read back: the owner reads the status when it likes.
 * The workspace (device, 16-byte aligned, pod_sgd_solver_workspace_bytes(n_tensors, n_chunks) bytes, zeroed ONCE by its owner):
 *     [0, 32) PodSgdSolverStatus;  [32, 32 + 8 n_chunks) partial, fp64, one per map entry;  then coef, fp32, n_tensors + 1.
 * pod_sgd_step_solver: the table, its device room and the chunk map as for pod_sgd_step; `group` HOST and `group_dev` dev, n_tensors uint8
 *   each, the same values (built once; the host copy is what is checked); `solver` HOST; `workspace` dev.  After K25's one table copy:
 *   clip_type OFF or VALUE without guard is ONE launch, the step; otherwise THREE on `stream`, ordered by it: the squares per chunk
 *   (partial), ONE workgroup that sums them per tensor and over the tensors and writes coef, status.last_norm = sqrt(N^2) and the rest of
 *   the status, and the step, which reads coef and status.poisoned.  No atomics, no cooperative launch, no grid barrier, no read-back, no
 *   scratch memory; two calls from one state give the same bits.  The default record (one group, OFF, no nesterov, no guard) is
 *   handed to pod_sgd_step: K25's own launch, its bits and its time.  POD_E_INVALID before anything is enqueued: everything pod_sgd_step refuses (with lr[g], wd[g] in place of its lr
 *   and weight_decay), solver NULL, n_groups outside 1..POD_SGD_MAX_GROUPS, group NULL with n_tensors > 0 or group[t] >= n_groups, lr[g] or
 *   wd[g] (g < n_groups) negative or not finite, momentum outside [0, 1), nesterov with momentum 0, clip_type outside 0..3, clip_type != OFF
 *   with a clip_value that is not finite and > 0, and with n_chunks > 0: workspace or group_dev NULL, workspace not on 16 bytes, a watch
 *   pointer not on 4.  n_tensors == 0, or every n == 0: POD_OK, nothing enqueued.
 * pod_sgd_solver_reset: zeroes the status (not partial or coef) on `stream`; POD_E_INVALID for a NULL or misaligned workspace. */
#define POD_SGD_MAX_GROUPS 8
#define POD_SGD_CLIP_OFF        0
#define POD_SGD_CLIP_VALUE      1
#define POD_SGD_CLIP_NORM       2
#define POD_SGD_CLIP_FULL_MODEL 3
typedef struct PodSgdSolver {
    int32_t n_groups;  int32_t nesterov;  int32_t clip_type;  int32_t guard;
    float lr[POD_SGD_MAX_GROUPS];  float wd[POD_SGD_MAX_GROUPS];
    float momentum;  float clip_value;
    int64_t iteration;                 /* what a bad step leaves in status.first_bad_iteration */
    const float* watch[4];             /* dev fp32 scalars that must be finite (the step's losses), NULL where unused */
} PodSgdSolver;
typedef struct PodSgdSolverStatus {
    int64_t bad_steps;  int64_t first_bad_iteration;  double last_norm;  int32_t poisoned;  int32_t reserved;
} PodSgdSolverStatus;
size_t pod_sgd_solver_workspace_bytes(int32_t n_tensors, int64_t n_chunks);
int pod_sgd_step_solver(const PodSgdTensor* tensors, PodSgdTensor* tensors_dev, int32_t n_tensors, const int32_t* chunk_map, int64_t n_chunks,
                        const uint8_t* group, const uint8_t* group_dev, const PodSgdSolver* solver, void* workspace, pod_stream_t stream);
int pod_sgd_solver_reset(void* workspace, pod_stream_t stream);

/* ---- K30  backward of the ResNet stem and its max-pool (csrc/k30_stem_backward.hip) ---------------------------------------------
 * Serves: the backward pass of detectron2's BasicStem (conv1 7x7 / stride 2 / pad 3 + FrozenBN + ReLU + max_pool2d(3, 2, 1)) in train
 * mode behind `self.backbone(images.tensor)` (probabilistic_retinanet.py:96-100) under train_net.py's loop at MODEL.BACKBONE.FREEZE_AT
 * 0; the reference gets it from autograd.  res2 (FREEZE_AT 1) runs on K13 / K22 / K24 at 64 channels.  Three new symbols under
 * POD_ABI_VERSION 18, as for K20 - K29: no entry or structure that existed changed, so the number stands.
 *
 * pod_stem7x7_wgrad: x dev (images, 3, H_img, W_img) contiguous, uint8 (x_is_u8) or fp32: the frames as pod_stem7x7_split takes them,
 *   normalised on load as there, (v - mean[c]) / stddev[c] in fp32 (mean, stddev dev, 3 floats each, both NULL: already normalised), zero
 *   outside H_img x W_img -- the convolution's padding and the frame's padding up to (H, W).  dS dev (images * Ho * Wo, 64) channels-last
 *   fp32, Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1.  dW dev fp32 (64, 3, 7, 7):
 *   dW[k][c][dy][dx] = sum over (b, oy, ox) of dS[(b, oy, ox)][k] xn[b][c][2 oy - 3 + dy][2 ox - 3 + dx].  No bias gradient: the bias is
 *   FrozenBN's shift.  K22's arithmetic: both operands split at run time into two f16 terms of their power-of-two-scaled values (x_amax: the
 *   record that bounds the NORMALISED input, pod_stem7x7_split's in_amax; ds_amax: dS's), three partial products on
 *   v_mfma_f32_32x32x16_f16, fp32 accumulation inside a slice -- a run of 8 x 8 output tiles whose length depends on the tile count alone --
 *   and the slices' partial sums (`partials`: pod_stem7x7_wgrad_partials(...) floats, 16-byte aligned, 64 * 192 per slice; 0 = invalid
 *   geometry) added in slice order in fp64 by a second launch.  No atomics: the same bits on every run.  Every extent pod_stem7x7_split
 *   accepts (1 <= H_img <= H <= 16384, the same for W) with images >= 1 and images * Ho * Wo < 2^30; POD_E_INVALID before any launch for
 *   anything else, a NULL pointer (mean and stddev only together), dS or partials off 16 bytes, a record, dW, mean, stddev or an fp32 x off
 *   4, or two of x, dS, dW and partials at one address.
 * pod_maxpool3x3s2_backward_cl: the backward of pod_maxpool3x3s2_cl and of the stem's ReLU for one image.  s dev (H * W, C): the stem's
 *   stored output; dP dev (Hq * Wq, C), Hq = (H - 1) / 2 + 1, Wq = (W - 1) / 2 + 1; dS dev (H * W, C):
 *   dS[(y, x)][c] = s[(y, x)][c] > 0 ? the sum of dP[(oy, ox)][c] over the at most four windows (oy, ox) that hold (y, x) and whose arg-max
 *   is (y, x) : 0, added in window order (oy ascending, then ox).  The arg-max is torch's: the window's pixels inside the map scanned
 *   row-major, a new maximum only on strict >, so the first maximum wins.  C % 4 == 0, 1 <= H, W <= 16384; dS may be neither s nor dP.
 *   ds_amax: NULL or the zeroed record that receives max |dS|. */
int64_t pod_stem7x7_wgrad_partials(int32_t images, int32_t H_img, int32_t W_img, int32_t H, int32_t W);
int pod_stem7x7_wgrad(const void* x, int32_t x_is_u8, int32_t images, int32_t H_img, int32_t W_img, const float* mean, const float* stddev, const float* dS,
                      int32_t H, int32_t W, const float* x_amax, const float* ds_amax, float* dW, float* partials, pod_stream_t stream);
int pod_maxpool3x3s2_backward_cl(const float* s, const float* dP, float* dS, int32_t H, int32_t W, int32_t C, float* ds_amax, pod_stream_t stream);

/* ---- K31  a training batch in one launch (csrc/k31_train_batch.hip) -------------------------------------------------------------
 * Serves: what detectron2's DatasetMapper(is_train=True) does to the decoded frames of a batch behind build_detection_train_loader(cfg)
 * (train_net.py's loop): ResizeShortestEdge at the frame's own drawn size with PIL's bilinear filter, then RandomFlip(horizontal), the
 * RGB -> BGR flip and the HWC -> CHW transpose -- K20's work for every frame of the batch, in ONE launch, to the byte (the two kernels
 * share one copy of the arithmetic, csrc/pod_resize_u8.h).  Two new symbols, one new structure and one constant under POD_ABI_VERSION 18,
 * as for K20 - K30: no entry or structure that existed changed, so the number stands.
 *
 * PodTrainFrame: pod_resize_frame_u8's arguments for one frame (src .. flip_channels, each as documented there), `hflip` != 0: output
 *   column x holds the RESIZED frame's column out_w - 1 - x (resize first, then flip), and `first_tile`: the index of the frame's first
 *   workgroup -- 0 for frame 0, and for frame i + 1 frame i's plus ceil(out_w / 64) * ceil(out_h / 4) of frame i.
 * pod_train_batch_tiles (host only): the launch's workgroup count, the sum of the frames' tiles, from out_h / out_w alone; -1 for a NULL
 *   table, n_frames outside 1 .. POD_TRAIN_BATCH_MAX_FRAMES or a size outside 1 .. POD_RESIZE_MAX_SIDE.
 * pod_train_batch_u8: frames HOST (pinned: the copy is then asynchronous; the caller keeps the table unchanged until it has run, an event
 *   after the entry's return), frames_dev dev, room for n_frames records.  One copy of the table and one launch on `stream`; every frame
 *   writes its own contiguous planar (3, out_h, out_w) uint8 tensor at `dst`, and no byte outside it.  POD_E_INVALID before anything is
 *   enqueued for a NULL table, n_frames out of range, a frame pod_resize_frame_u8 would refuse, a first_tile sequence or n_tiles other
 *   than the sizes give, more than 2^31 - 1 tiles, two outputs that overlap, or an output that overlaps any frame's source. */
#define POD_TRAIN_BATCH_MAX_FRAMES 64
typedef struct PodTrainFrame {
    const uint8_t* src;  int32_t in_h;  int32_t in_w;  int64_t row_stride;
    const int32_t* xbounds;  const int32_t* xcoeffs;  int32_t xk;  int32_t reserved0;
    const int32_t* ybounds;  const int32_t* ycoeffs;  int32_t yk;  int32_t reserved1;
    uint8_t* dst;  int32_t out_h;  int32_t out_w;  int32_t flip_channels;  int32_t hflip;
    int64_t first_tile;
} PodTrainFrame;
int64_t pod_train_batch_tiles(const PodTrainFrame* frames, int32_t n_frames);
int pod_train_batch_u8(const PodTrainFrame* frames, PodTrainFrame* frames_dev, int32_t n_frames, int64_t n_tiles, pod_stream_t stream);

/* (test support -- the dumps of the in-kernel Philox draws, of the generator itself and of the f16 split -- is declared in
 * include/pod_mi355x_test.h: the library exports those entry points for tests/ and tools/, they are not part of the drop-in boundary.) */

/* ---- K13 conv1x1_split (round 4): the 1x1 convolutions of the backbone / FPN as a channels-last GEMM ------------------------
 * Replaces: detectron2 BottleneckBlock.conv1 / conv3 / shortcut (1x1, stride 1 or 2, FrozenBN folded, ReLU, residual add) and
 * FPN.lateral_convs as `self.backbone(images.tensor)` runs them (probabilistic_retinanet.py:96-100): 39 calls per image that PyTorch-ROCm
 * executes as fp32 GEMMs + one element-wise pass each.  Same arithmetic contract as pod_wino_conv3x3_split (round 5: 2-way f16 splits of
 * the power-of-two-scaled operands, 3 partial products, fp32 accumulate; in_amax / out_amax: operand abs-max words, above).
 *   y[p][k] = act(sum_c x[pin(p)][c] w[k][c] + bias[k] (+ residual[p][k])),  p = oy * W_out + ox,  pin = (stride oy) * W_in + stride ox
 * x dev (H_in * W_in, Cin), y / residual dev (H_out * W_out, Cout): channels-last.  Cin % 16 == 0, Cout % 64 == 0.
 * Ws = pod_conv1x1_filter_split(weight (Cout, Cin) fp32): pod_conv1x1_filter_split_bytes(Cout, Cin) bytes (2 * Cout * Cin f16 terms + a 16-byte trailer: the
 * weight's abs-max), 16-byte aligned.
 * n_splits > 1 (small maps): the input channels cut over workgroup sets, partial sums in `partials` (n_splits * H_out * W_out * Cout
 * floats), added in a fixed order with bias / residual / ReLU by a second launch.  waves (round 5): 1, 2 or 4 wavefronts of ONE workgroup
 * share a tile's K range and add their accumulators in LDS in a fixed order -- split-K without the partial sums' trip through HBM or a
 * second launch, to the bit the result of the same cut over workgroup sets; 0: chosen by the library (what the model uses).
 * flags: POD_C1_RELU (1) = ReLU; POD_C1_RESIDUAL_UP2 (2, n_splits == 1 only) = `residual` is the HALF-resolution map, ((H_out + 1) / 2) x
 * ((W_out + 1) / 2) pixels, and pixel (y, x) adds residual[(y >> 1) * ((W_out + 1) / 2) + (x >> 1)]: detectron2 FPN's top-down path,
 * `lateral + F.interpolate(top_down, scale_factor=2, mode="nearest")`, without materialising the upsampled map. */
#define POD_C1_RELU 1
#define POD_C1_RESIDUAL_UP2 2
int64_t pod_conv1x1_filter_split_bytes(int32_t Cout, int32_t Cin);
int pod_conv1x1_filter_split(const float* weight, void* Ws, int32_t Cout, int32_t Cin, pod_stream_t stream);
int pod_reduce_partials(const float* partials, int32_t n_splits, int64_t split_stride, const float* bias, const float* residual, float* y,
                        int64_t n, int32_t Cout, int32_t relu, float* out_amax, pod_stream_t stream);   /* y = act(sum_s partials[s] + bias + residual), channels-last */
int pod_conv1x1_split(const float* x, float* y, const void* Ws, const float* bias, const float* residual, int32_t H_out, int32_t W_out,
                      int32_t H_in, int32_t W_in, int32_t stride, int32_t Cin, int32_t Cout, int32_t flags, int32_t n_splits, float* partials,
                      int32_t waves, const float* in_amax, float* out_amax, pod_stream_t stream);

/* ---- one image, one call --------------------------------------------------------------------
 * Replaces: everything `RetinaNetProbabilisticPredictor.__call__` does after the conv net
 * (PI:86-111 -> PI:178-388 -> the mode's post-processing -> IU:374-425), i.e. the launch sequence
 *   pod_merge_score_fused (= pod_mc_merge_score + pod_score_maybe) -> pod_level_topk -> pod_gather_decode (= pod_gather_candidates + pod_decode_cov)
 *   -> pod_nms_cluster -> {pod_bayes_fuse | pod_anchor_stats_merge | -} -> pod_finalize
 * enqueued from C on `stream`, in-kernel Philox draws (levels[].eps_cls must be NULL: the eps-replay parity
 * mode needs the host between launches and uses the individual entry points).  Nothing here
 * synchronises or allocates; the workspace is caller-owned, every pointer is device memory sized as the
 * individual entry points document, n_capacity = n_levels * topk.  mean_delta / mean_reg_var may be NULL
 * (the merged box planes are not needed downstream), mean_cls / mean_cls_var only when n_runs == 1. */
typedef struct PodWorkspace {
    const float* anchors;          /* (R, 4) level-concatenated */
    float* mean_cls;  float* mean_cls_var;  float* mean_delta;  float* mean_reg_var;
    uint64_t* cand_keys;  int32_t* cand_count;  uint64_t* maybe_bits;
    uint64_t* sel_keys;   int32_t* sel_count;
    uint64_t* cat_keys;   int32_t* cat_level;          /* level-concatenated selection, n_capacity rows each */
    float* probs_dense;                                /* (R, K) or NULL when the model has no variance head */
    int32_t* n_total;     int32_t* cand_anchor_idx;  int32_t* cand_level;  int32_t* cand_class;
    float* cand_score;    float* cand_probs;  float* cand_delta;  float* cand_reg_var;  float* cand_anchor;
    float* cand_run_delta;
    float* boxes;  float* cov;
    int32_t* keep;  int32_t* n_keep;  void* nms_scratch;
    float* m_boxes;  float* m_cov;  float* m_scores;  int32_t* m_classes;  float* m_probs;
    int32_t n_capacity;  int32_t reserved;
} PodWorkspace;

#define POD_MODE_STANDARD_NMS 0    /* also the pre-NMS MC-dropout / ensemble modes (PI:402-442, PI:483-505) */
#define POD_MODE_BAYES_OD 1
#define POD_MODE_ANCHOR_STATISTICS 2

/* image_h/w: network input size (IU:39-41), out_h/w: output resolution (PI:106-107);
 * box_merge_mode / cls_merge_mode as in pod_bayes_fuse (ignored by the other modes). */
int pod_run_image(const PodConfig* cfg, const PodLevel* levels, const PodWorkspace* ws, int32_t mode,
                  int32_t box_merge_mode, int32_t cls_merge_mode, int32_t image_h, int32_t image_w,
                  int32_t out_h, int32_t out_w, const PodDetections* out, pod_stream_t stream);
/* The same in two parts (round 5): parts = 1 SELECT (merge + score + per-level top-k, PI:211-308: the candidates stand in ws->cat_keys /
 * cat_level / n_total afterwards; levels[l].delta / reg_var are not read and may be NULL, `out` too), 2 FINISH (gather + decode + NMS / fusion +
 * finalize, PI:310-636), 3 both.  The sparse bbox tower runs between 1 and 2. */
int pod_run_image_part(const PodConfig* cfg, const PodLevel* levels, const PodWorkspace* ws, int32_t mode,
                  int32_t box_merge_mode, int32_t cls_merge_mode, int32_t image_h, int32_t image_w,
                  int32_t out_h, int32_t out_w, const PodDetections* out, int32_t parts, pod_stream_t stream);
/* FINISH is itself two parts, for several inference configs on one image: 4 CANDIDATES (gather + decode + NMS: what no mode changes; `out`
 * may be NULL), 8 TAIL (the mode's fusion launch, none for standard NMS, + pod_finalize: reads the candidate arrays and the keep list
 * CANDIDATES left and leaves them as they were; writes ws->m_* and `out`), 5 FRONT = SELECT + CANDIDATES.  2 = 4 then 8.  Values 1, 2 and 3
 * are what they were. */
#define POD_PART_SELECT 1
#define POD_PART_FINISH 2
#define POD_PART_CANDIDATES 4
#define POD_PART_FRONT 5
#define POD_PART_TAIL 8

/* Several inference configs of one image on one front (the comparison pass, DESIGN.md "Comparison pass"): the front -- pod_merge_score_fused
 * -> pod_level_topk -> pod_gather_decode -> pod_nms_cluster -- is enqueued ONCE, then per tail, in order, that mode's fusion launch and
 * pod_finalize into the tail's own PodDetections.  tails[t].out holds what pod_run_image(mode, box_merge_mode, cls_merge_mode) on the same
 * inputs and cfg->philox_seed writes, bit for bit.  ws->m_* is scratch the tails share: stream order serialises them.  Nothing synchronises
 * or allocates; graph-capturable as pod_run_image is.  POD_E_INVALID, with nothing enqueued: n_tails < 1 or > POD_MAX_MODE_TAILS, an unknown
 * mode, a POD_MODE_BAYES_OD tail without covariances (cfg->cov_dims == 0 and cfg->n_runs == 1) or with a merge mode pod_bayes_fuse refuses,
 * a NULL output, and whatever pod_run_image refuses.  One new symbol, one new structure and six constants under POD_ABI_VERSION 18: no
 * entry or structure that existed changed, so the number stands. */
#define POD_MAX_MODE_TAILS 8
typedef struct PodModeTail {
    int32_t mode, box_merge_mode, cls_merge_mode, reserved;
    PodDetections out;
} PodModeTail;
int pod_run_image_modes(const PodConfig* cfg, const PodLevel* levels, const PodWorkspace* ws, const PodModeTail* tails, int32_t n_tails,
                        int32_t image_h, int32_t image_w, int32_t out_h, int32_t out_w, pod_stream_t stream);

/* ---- K32  retinanet_inference (csrc/k32_retinanet_inference.hip) ----------------------------------------------------------------
 * Replaces: what the reference model runs in EVAL mode (PR:156-166: `self.inference(...)`, then `detector_postprocess`), i.e. detectron2's
 * RetinaNet.inference_single_image (modeling/meta_arch/retinanet.py of the v0.1 line the reference was written against) and
 * detector_postprocess (modeling/postprocessing.py) -- the routine `Trainer.test` / `--eval-only` of train_net.py:67-76 evaluates, NOT the
 * probabilistic post-processing of PI.  It differs from pod_run_image's path: a level ranks its FLATTENED (anchor, class) scores, so one
 * anchor may yield several detections of different classes; means only are decoded, no covariance.
 * Input: the eval-mode head output as PodLevel planes, cfg->n_runs == 1; cls_var / reg_var / eps_cls are ignored.
 *
 * Ordering contract (DESIGN.md "K32"): the flat index of an entry inside its level is f = (cell * A + a) * K + k -- the order of
 * permute_to_N_HWA_K(...).flatten() -- an entry is a candidate iff sigmoid(logit) > cfg->score_thresh (fp32), candidates rank by DESCENDING
 * LOGIT (-0.0 == 0.0), ties to the lower f; a level keeps its first min(cfg->topk, candidates) ranked candidates.  The key of a candidate:
 *     key = (order_bits(logit) << 32) | (0xFFFFFFFF - f),   order_bits = float bits with the sign bit flipped (negative: all bits flipped)
 * -- K1's key convention with the logit in place of the score (sigmoid is monotone), so pod_level_topk's select and sort rank it unchanged.
 *
 * pod_retinanet_score : ONE streaming read of cls (4 * R * K bytes); appends the keys of level l to cand_keys + anchor_base_l * K, count
 *                       in cand_count[l].  cand_keys : dev uint64[R_total * K];  cand_count : dev int32[2 * n_levels], zero on entry (as K1).
 * pod_retinanet_topk  : pod_level_topk (K2's shared radix select and bitonic sort) on those lists; arguments and outputs as pod_level_topk.
 * pod_retinanet_decode: one thread per row of the level-concatenated selection: anchor = f / K, class = f % K, Box2BoxTransform.apply_deltas
 *                       (cfg->box_weights, dw / dh clamped at log(1000 / 16)), score = sigmoid of the key's logit.  cand_flat / cand_level /
 *                       scores / classes : n_levels * topk entries, boxes (n_levels * topk, 4), 16-byte aligned.  cand_count is consumed (zeroed).
 * pod_nms_cluster     : batched_nms + [:max_detections], unchanged, on (boxes, scores, classes).
 * pod_retinanet_postprocess: rows keep[0 : n_keep) scaled by (scale_x, scale_y) (fp32 roundings of out / image size), clipped to
 *                       [0, out_w] x [0, out_h], rows that are empty afterwards (Boxes.nonempty, threshold 0) dropped, compacted in keep order
 *                       into det_boxes (max_detections, 4) / det_scores / det_classes; n_det dev int32.  Rows >= n_det are not written.
 * pod_retinanet_infer_image: the five launches enqueued on `stream`; graph-capturable, reads nothing back; the only atomics are the
 *                       list-append tickets of the scoring pass and K2's.  `workspace`: dev, 16-byte aligned,
 *                       pod_retinanet_infer_workspace(cfg, levels, NULL) bytes, ZEROED ONCE after allocation (counters, NMS scratch) and
 *                       then owned by this entry point; `layout` (may be NULL) receives the byte offsets of its parts.
 * Limits (POD_E_INVALID otherwise): n_runs == 1, K <= POD_MAX_CLASSES - 1, topk <= POD_MAX_TOPK, n_levels * topk <= POD_MAX_CANDIDATES,
 * max_detections <= POD_MAX_DETECTIONS, A * K * H * W < 2^31 per level. */
typedef struct PodRetinaNetLayout {   /* byte offsets into the workspace; the arrays as the stage entry points document them */
    int64_t cand_keys, cand_count, sel_keys, sel_count, cat_keys, cat_level, n_total, cand_flat, cand_level, boxes, scores, classes,
        keep, n_keep, nms_scratch, total;
} PodRetinaNetLayout;
int64_t pod_retinanet_infer_workspace(const PodConfig* cfg, const PodLevel* levels, PodRetinaNetLayout* layout);
int pod_retinanet_score(const PodConfig* cfg, const PodLevel* levels, uint64_t* cand_keys, int32_t* cand_count, pod_stream_t stream);
int pod_retinanet_topk(const PodConfig* cfg, const PodLevel* levels, uint64_t* cand_keys, int32_t* cand_count, uint64_t* sel_keys,
                       int32_t* sel_count, uint64_t* cat_keys, int32_t* cat_level, int32_t* n_total, pod_stream_t stream);
int pod_retinanet_decode(const PodConfig* cfg, const PodLevel* levels, const float* anchors, const uint64_t* cat_keys,
                         const int32_t* cat_level, const int32_t* n_total, int32_t* cand_count, int32_t* cand_flat, int32_t* cand_level,
                         float* boxes, float* scores, int32_t* classes, pod_stream_t stream);
int pod_retinanet_postprocess(const PodConfig* cfg, const int32_t* keep, const int32_t* n_keep, const float* boxes, const float* scores,
                              const int32_t* classes, float scale_x, float scale_y, float out_h, float out_w, float* det_boxes,
                              float* det_scores, int32_t* det_classes, int32_t* n_det, pod_stream_t stream);
int pod_retinanet_infer_image(const PodConfig* cfg, const PodLevel* levels, const float* anchors, void* workspace, int32_t image_h,
                              int32_t image_w, int32_t out_h, int32_t out_w, float* det_boxes, float* det_scores, int32_t* det_classes,
                              int32_t* n_det, pod_stream_t stream);

/* ---- K33  the evaluation's bounded scoring rules: energy score and CRPS (csrc/k33_eval_scores.hip) ----------------------------
 * Serves: compute_reg_scores (scoring_rules.py:45-81) when asked for more than the NLL.  The reference's scoring_rules.py defines the
 * ignorance score and the MSE and NEITHER of these rules; the definitions are the ones below, in box space (no smooth-L1 term, no division
 * by the coordinate count: this is not K27's training loss, which lives in delta space).  One new symbol and one new stream word under
 * POD_ABI_VERSION 18, as for K20 - K32: no entry or structure that existed changed, so the number stands.
 *
 * Rows i < n: means (n, 4), covs (n, 4, 4), gt (n, 4), dev fp32, as pod_reg_nll takes them.  Sigma = cov + 1e-2 I, the sum formed in fp32 and
 * then widened; L its Cholesky factor in fp64, the lower triangle read -- pod_reg_nll's factorisation, one copy shared by both kernels.
 *   Energy score, M = num_samples, eps_s in R^4 for s = 0 .. M (M + 1 draws, iid N(0, 1), fp32):
 *     u1_s = (mean - gt) + L eps_s;   u2_s = L (eps_s - eps_{s+1}), formed from the fp32 difference of the normals, widened, and never as a
 *     difference of samples (K27's and K28's rule);   energy[i] = (1 / M) sum_{s < M} |u1_s|_2  -  (1 / (2 M)) sum_{s < M} |u2_s|_2.
 *   CRPS, the marginal rule, closed form, no draws: sd_j = sqrt(Sigma_jj), z_j = (gt_j - mean_j) / sd_j,
 *     crps[i] = (1 / 4) sum_j sd_j [z_j (2 Phi(z_j) - 1) + 2 phi(z_j) - 1 / sqrt(pi)],  Phi through erf.
 *   Everything after the fp32 normals is fp64; each output rounds to fp32 once, at its store.  A row whose Sigma is not positive definite
 *   gets NaN in both outputs and affects no other row (pod_reg_nll behaves so).
 * One wavefront per row; a lane owns the sample pairs c = lane, lane + 64, ..., keeps two fp64 partial sums, a butterfly in a fixed order
 * adds them.  No atomics: two launches give the same bits, and a row's result depends on that row's inputs, its index i, `seed` and M alone
 * -- not on n, the grid or the other rows.
 * Draws: eps_in NULL = in-kernel Philox4x32-10 normals on a stream word of their own (0x65767300, "evs"): samples 2c and 2c + 1 of row i are
 *   components 0..3 and 4..7 of the call with counter (i, 0, c, stream word) and key `seed` (K27's map); or dev (num_samples + 1, n, 4) normals
 *   to replay.  eps_out: NULL or a buffer of that shape receiving the normals used.  Both are a test and replay facility.
 * energy / crps: dev float[n]; either may be NULL (not both) and is then not computed; with energy NULL num_samples is ignored.
 * POD_E_INVALID before anything is enqueued: means, covs or gt NULL; energy and crps both NULL; n < 0; energy given and num_samples outside
 *   [1, POD_MAX_REG_SAMPLES]; eps_in or eps_out given while energy is NULL, or off 16 bytes.  n == 0: POD_OK, nothing launched. */
int pod_reg_scores(const float* means, const float* covs, const float* gt, int32_t n, int32_t num_samples, uint64_t seed,
                   const float* eps_in, float* eps_out, float* energy, float* crps, pod_stream_t stream);

/* ---- K34  PDQ, the probability-based detection quality: pairwise quality and assignment (csrc/k34_pdq.hip) ---------------------
 * Replaces: nothing the reference runs -- its README's line "For evaluating with PDQ, please use the official PDQ code" sends the user to a
 * separate CPU tool.  PDQ (Hall et al., "Probabilistic Object Detection: Definition and Evaluation") is DEFINED here, every discretisation
 * choice stated; numbers are comparable with that tool's only up to these choices.  Three new symbols under POD_ABI_VERSION 18, as for
 * K20 - K33: no entry or structure that existed changed.
 *
 * Per image m < n_images: a frame (W, H) = frames[2 m], frames[2 m + 1]; detections j < D = det_off[m + 1] - det_off[m] (xyxy mean, 4x4
 * covariance, a class probability row of K = num_classes); ground truths i < G = gt_off[m + 1] - gt_off[m] (xyxy box, contiguous class c_i).
 *   Pixel (u, v), 0 <= u < W, 0 <= v < H, has the centre (u + 0.5, v + 0.5).  The ground-truth segment S_i: the pixels whose centre lies in
 *   [x1, x2) x [y1, y2) (no masks); n_i = |S_i|.
 *   Corner blocks: S_tl the (x1, y1) and S_br the (x2, y2) 2x2 block of cov + 1e-2 I, the sum formed in fp32 and then widened (K33's rule;
 *   the lower triangle is read; cross-corner covariance is ignored, as PDQ's probabilistic box does).  sd = sqrt of the diagonal, rho
 *   clamped to [-0.99, 0.99].  A detection is INVALID when a diagonal entry of a block is not positive or not finite, a mean is not finite
 *   or a correlation is not finite: quality 0 against every ground truth, det_invalid[j] = 1, no effect on any other detection.
 *   P(pixel in box) = A B,  A = Phi2((cx - mu_x1) / sd_x1, (cy - mu_y1) / sd_y1; rho_tl),  B = Phi2((mu_x2 - cx) / sd_x2, (mu_y2 - cy) / sd_y2; rho_br),
 *   Phi2(h, k; rho) = Phi(h) Phi(k) + (1 / 2 pi) int_0^{asin rho} exp(-(h^2 + k^2 - 2 h k sin t) / (2 cos^2 t)) dt, fp64, Phi through erfc; the
 *   integral by 20-point Gauss-Legendre on equal panels no wider than asin(0.99) / 4 (four at |rho| = 0.99, none at rho = 0).
 *   The complement is never 1 - P:  Ac = Phi(-h) + Phi(-k) - Phi2(-h, -k; rho), Bc likewise, Q = Ac + A Bc.
 *   The detection's segment T_j = {P >= p_min}.  small = 1e-14.
 *     sum_fg(i, j) = sum_{x in S_i} log max(P'(x), small), P' = P on T_j and 0 elsewhere;   L_FG = -sum_fg / n_i
 *     sum_bg(i, j) = sum_{x in T_j \ S_i} log max(Q(x), small);                              L_BG = -sum_bg / n_i
 *     q_fg = exp(-L_FG), q_bg = exp(-L_BG), q_spatial = exp(-(L_FG + L_BG)), q_label = p_j[c_i] (0 for c_i outside [0, K)),
 *     pPDQ = sqrt(q_spatial q_label).  n_i = 0, S_i and T_j disjoint, or the detection invalid: all five and both sums are 0 -- a pair
 *     without overlap can never be a true positive, which is also what makes skipping the pixels outside the region of interest exact.
 *   One workgroup per detection evaluates P and Q once per pixel of the region of interest (columns with cx < mu_x1 + z sd_x1 or
 *   cx > mu_x2 - z sd_x2, z = Phi^-1(p_min), hold no pixel of T_j since P <= Phi of each single argument; rows likewise; one pixel wider,
 *   clipped to the frame) and gives every ground truth of the image its sums from that pass: compensated fp64 sums in pixel order, no atomics.  A
 *   pair's numbers depend on that detection, that ground truth, the frame and p_min alone -- not on the grid, the other images or pairs.
 * pod_pdq_pairs: frames (n_images, 2), det_off, gt_off (n_images + 1, from 0) int32 and pair_off (n_images + 1, from 0) int64 are HOST
 *   tables, pair_off[m + 1] - pair_off[m] = G D; the call copies them into `workspace` (dev, pod_pdq_workspace_bytes(n_images) bytes).
 *   det_means (D_total, 4), det_covs (D_total, 4, 4), det_probs (D_total, K), gt_boxes (G_total, 4) dev fp32, gt_classes dev int32[G_total].
 *   quality: dev double[5][n_pairs], n_pairs = pair_off[n_images], the planes pPDQ, q_spatial, q_label, q_fg, q_bg; pair (i, j) of image m at
 *   pair_off[m] + i D + j.  sums: NULL or dev double[2][n_pairs] (sum_fg, sum_bg).  det_invalid: NULL or dev int32[D_total].
 * pod_pdq_assign: per image the maximum-weight assignment on the G x D matrix of pPDQ (plane 0 of `quality`), padded with zeros to
 *   n = max(G, D): shortest augmenting paths with potentials in fp64 on cost -pPDQ over the G real rows, one wavefront per image, ties to the
 *   lowest column -- additions, subtractions and comparisons only.  A true positive is an assigned pair with pPDQ > 0; a pPDQ that is not
 *   positive and finite counts as 0.
 *   gt_match: dev int32[G_total], the detection (index inside its image) of a ground truth's true positive, else -1.  counts: dev
 *   int32[n_images][3] = TP, FP = D - TP, FN = G - TP.  image_sums: dev double[n_images][5], the sums over the image's true positives of the
 *   five planes, added in ground-truth order.  The data set's PDQ = sum pPDQ / (TP + FP + FN) (0 when that is 0) is the caller's, in image order.
 * POD_E_INVALID before anything is enqueued: a needed pointer NULL (frames, the offsets; the packed arrays, quality and workspace where there
 *   is something to read or write), n_images < 0, offsets not starting at 0, decreasing, or pair_off not the running sum of G D, a side
 *   G or D above POD_PDQ_MAX_SIDE, num_classes outside [1, POD_MAX_CLASSES], a frame dimension below 1 or above POD_PDQ_MAX_FRAME, p_min
 *   outside (0, 1), workspace / quality / sums / image_sums off 8 bytes.  No detection (pairs) / no image (assign): POD_OK, nothing launched. */
#define POD_PDQ_MAX_SIDE   256     /* ground truths / detections of one image */
#define POD_PDQ_MAX_FRAME  32768   /* frame width / height */
size_t pod_pdq_workspace_bytes(int32_t n_images);
int pod_pdq_pairs(const int32_t* frames, const int32_t* det_off, const int32_t* gt_off, const int64_t* pair_off, int32_t n_images,
                  const float* det_means, const float* det_covs, const float* det_probs, int32_t num_classes, const float* gt_boxes,
                  const int32_t* gt_classes, double p_min, void* workspace, double* quality, double* sums, int32_t* det_invalid,
                  pod_stream_t stream);
int pod_pdq_assign(const int32_t* det_off, const int32_t* gt_off, const int64_t* pair_off, int32_t n_images, const double* quality,
                   void* workspace, int32_t* gt_match, int32_t* counts, double* image_sums, pod_stream_t stream);

/* ---- K35  synthetic corruptions of the decoded frame (csrc/k35_corrupt_u8.hip) ---------------------------------------------------
 * Replaces: nothing in the reference: the test loader's frame, between decode and AN:83-84's resize.  The reference measures data-set
 * shift with a second and a third data set; this is the controlled shift of Hendrycks and Dietterich's ImageNet-C, eight kinds, the
 * constants of the five severities this project's own (pod_compare_amd/corruptions.py): parity with no package is claimed.
 * Two new symbols and one new structure under POD_ABI_VERSION 18, as for K20 - K34: no entry or structure that existed changed.
 *
 * Input and output: uint8 (h, w, 3) RGB, rows `row_stride` bytes apart (>= 3 w), two buffers that do not overlap.  The output is a pure
 * function of (frame bytes, kind, parameters, key).  Every kind ends in Q(v) = uint8(floor(min(max(v, 0), 1) * 255 + 0.5)): round to
 * nearest, where the public implementations truncate -- a flat region stays flat under a filter whose taps sum to 1 +- an ulp.
 *   GAUSSIAN_NOISE  fp32: xf = float(x) / 255, v = xf + sigma z             (sigma = (float)p0; the product first, then the sum)
 *   SPECKLE_NOISE   fp32: v = xf + (xf * c) * z                             (c = (float)p0)
 *     z of channel ch at pixel (x, y): Philox4x32-10 with counter (x, y, 0, 0x636f7200 "cor") and key `key` (low word, high word);
 *     normal ch & 1 of output word ch >> 1 through box_muller16 (csrc/pod_device.h).
 *   IMPULSE_NOISE   integers: counter (x, y, 1, 0x636f7200); byte ch becomes 255 / 0 (bit ch of word 3 set / clear) iff word ch <
 *     impulse_threshold = min(floor(amount 2^32), 2^32 - 1), and passes unchanged otherwise.
 *   BRIGHTNESS, SATURATE  fp64, every operation rounded on its own: r, g, b = x / 255.0; V = max, m = min, d = V - m; S = d / V (0 when
 *     V = 0); h6 = 0 when d = 0, else (g - b) / d (+ 6 when negative) when V = r, else 2 + (b - r) / d when V = g, else 4 + (r - g) / d.
 *     BRIGHTNESS: V <- min(V + p0, 1).  SATURATE: S <- min(max(S p0 + p1, 0), 1).  Back: i = floor(h6) (6 reads as 0), f = h6 - i,
 *     p = V (1 - S), q = V (1 - f S), t = V (1 - (1 - f) S); (r, g, b) by sextant: (V,t,p) (q,V,p) (p,V,t) (p,q,V) (t,p,V) (V,p,q).
 *   CONTRAST        fp64: mean_c = (integer sum of channel c) / (255.0 h w); v = (x / 255.0 - mean_c) p0 + mean_c.  The sums are 32-bit
 *     integers per workgroup, added in 64 bits by a second launch: the bytes cannot depend on the grid.  No float atomics.
 *   GAUSSIAN_BLUR   taps: dev float[2 radius + 1], radius <= 24.  Separable, along the rows, then down the columns; border clamped to the
 *     edge.  fp32: acc = fmaf(tap, float(byte), acc) in ascending tap order, the intermediate kept in byte units in `scratch`; v = acc / 255.
 *   DEFOCUS_BLUR    taps: dev float[(2 radius + 1)^2] row-major, radius <= 12: a dense correlation, the same stencil for the three
 *     channels, reflect-101 borders repeated until the index is inside; fp32 as above, stencil rows then columns ascending.
 * pod_corrupt_scratch_bytes: bytes of `scratch` (dev, 8-byte aligned) a call needs -- GAUSSIAN_BLUR 12 h w, CONTRAST 32 + 12 ceil(h w / 4096),
 *   0 for the other kinds (scratch may then be NULL) and for a side outside [1, POD_RESIZE_MAX_SIDE].
 * pod_corrupt_frame_u8: enqueues on `stream` (one launch; CONTRAST three, GAUSSIAN_BLUR two), never synchronises.  POD_E_INVALID and nothing
 *   enqueued: src, dst or corruption NULL; a side < 1 or > POD_RESIZE_MAX_SIDE; a row stride < 3 w; kind outside [0, POD_CORRUPT_KINDS); a
 *   filter's radius < 0 or above its cap, or its taps NULL; scratch NULL, off 8 bytes or smaller than pod_corrupt_scratch_bytes says; src,
 *   dst and the needed scratch overlapping one another. */
#define POD_CORRUPT_GAUSSIAN_NOISE 0
#define POD_CORRUPT_SPECKLE_NOISE  1
#define POD_CORRUPT_IMPULSE_NOISE  2
#define POD_CORRUPT_GAUSSIAN_BLUR  3
#define POD_CORRUPT_DEFOCUS_BLUR   4
#define POD_CORRUPT_BRIGHTNESS     5
#define POD_CORRUPT_CONTRAST       6
#define POD_CORRUPT_SATURATE       7
#define POD_CORRUPT_KINDS          8      /* the rest of ImageNet-C would continue here */
typedef struct PodCorruption {
    int32_t kind;                 /* POD_CORRUPT_* */
    int32_t radius;               /* the filters: taps reach -radius .. radius */
    double p0, p1;                /* the kind's parameters (above); unused ones ignored */
    const float* taps;            /* dev; the filters */
    uint32_t impulse_threshold;   /* IMPULSE_NOISE */
    uint32_t reserved;
    uint64_t key;                 /* the noises: Philox key */
} PodCorruption;
size_t pod_corrupt_scratch_bytes(int32_t kind, int32_t h, int32_t w);
int pod_corrupt_frame_u8(const uint8_t* src, int32_t h, int32_t w, int64_t src_row_stride, uint8_t* dst, int64_t dst_row_stride,
                         const PodCorruption* corruption, void* scratch, size_t scratch_bytes, pod_stream_t stream);

/* ---- K36  post-hoc recalibration: one temperature, per-coordinate variance scales (csrc/k36_recalibrate.hip) -------------------
 * Replaces: nothing in the reference, which measures calibration (CE:86-297) and stops.  Fits a two-parameter-family map on matched
 * detections and applies it to K7's record table: every probability p -> sigmoid(beta logit p), the xyxy covariance Sigma -> D Sigma D,
 * D = diag(s).  Six new symbols under POD_ABI_VERSION 18, as for K20 - K35: no entry or structure that existed changed.
 *
 * Sums.  No atomics.  Every fp64 sum of this section is added in ONE order, whatever the grid: the values of a sequence (a segment's, in
 *   index order) are cut into chunks of POD_RECAL_CHUNK = 256 consecutive values, the last one shorter; a chunk's partial is
 *   ((0.0 + v_0) + v_1) + ... in index order; the sum is ((0.0 + partial_0) + partial_1) + ... in chunk order.  The library is built with
 *   -ffp-contract=off: a host that adds fp64 values in this order gets the same bits.
 * pod_recal_workspace_bytes(n, n_seg): bytes of `workspace` (dev, 8-byte aligned) for any call below on n values and up to n_seg
 *   segments; 0 for n outside [0, 2^31 - 1] or n_seg outside [0, POD_RECAL_MAX_SEGMENTS].
 * pod_recal_cls_sums: p dev float[n] scores, y dev uint8[n] labels in {0, 1}.  x_i = logit(c_i) = log(c_i / (1 - c_i)),
 *   c_i = min(max(double(p_i), 2^-30), 1 - 2^-30) (only exact 0 and 1 and scores below 2^-30 move: the largest fp32 below 1 is 1 - 2^-24);
 *   t_i = beta x_i, e_i = exp(-|t_i|), s_i = 1 / (1 + e_i) for t_i >= 0, else e_i / (1 + e_i).  sums[0 .. 2], dev double:
 *     L = sum (max(t_i, 0) + log1p(e_i)) - y_i t_i,   g = dL/dbeta = sum (s_i - y_i) x_i,   h = sum (e_i / (1 + e_i)^2) x_i^2.
 *   x: NULL, or dev double[n] that receives the x_i (x_ready == 0) or holds them from an earlier call on the same p (x_ready != 0: p is
 *   not read, no logarithm is taken) -- a Newton loop computes them once.  workspace: pod_recal_workspace_bytes(n, 0).  n == 0: three zeros.
 * pod_recal_reg_z: the n_matched matched rows' xyxy means, (4, 4) covariances and ground-truth boxes, dev fp32.  Value 4 i + d, d < 4:
 *   z = (double(gt_d) - double(mean_d)) / sqrt(double(cov_dd)) and its segment id seg = d (n_class == 0: global scales) or
 *   4 det_class[i] + d (n_class >= 1: per-class scales; det_class dev int32[n_matched], the row's class as pod_calib_keys writes it).  A value whose
 *   cov_dd is not finite or <= 0, whose residual is not finite, or whose class lies outside [0, n_class) is left out: z = 0, seg = -1, and
 *   it is counted in invalid[d] (dev int64[4]).  z dev double[4 n_matched], seg dev int32[4 n_matched].  Only + - / sqrt: bit-equal to
 *   the same fp64 expression on a host.  workspace: pod_recal_workspace_bytes(4 n_matched, 0).
 * pod_recal_moment: n values z with segment ids seg (< 0 or >= n_seg: left out) -> zg dev double[n], the values grouped by segment in
 *   ascending id, row order kept inside a segment (the left-out tail zeros); seg_off dev int64[n_seg + 1], the segments' offsets in zg;
 *   count dev int64[n_seg]; sum dev double[n_seg], the sum of z^2 over the segment's values in zg order, added as above.  sum / count is
 *   the maximum-likelihood variance scale s^2 of the marginal Gaussian; the square root and the empty segment (s = 1) are the caller's.
 * pod_recal_ece_grid: zg / seg_off as pod_recal_moment wrote them, max_seg the longest segment (from count; a host value).  Each
 *   segment's values are sorted ascending; for every segment and every grid scale scales[j], j < n_grid (dev double), with m the segment's count,
 *     obj[s][j] = (sum_{i = 1 .. n_q} (count(z < scales[j] * q[i - 1]) / m - i / (n_q + 1))^2) / n_q
 *   -- the reference's regression calibration objective (CE:206-261) at variance scale scales[j]: q dev double[n_q] are the caller's
 *   Phi^-1(i / (n_q + 1)), the counts by binary search, the n_q terms added in i order from 0.0, every operation one fp64 rounding.  An empty
 *   segment's objectives are 0.  best_j[s]: the arg-min, ties to the smaller |j - j_one|, then to the smaller j (j_one: the grid point of
 *   scale 1); best_obj[s] = obj[s][best_j[s]], one_obj[s] = obj[s][j_one].  obj dev double[n_seg][n_grid], best_j dev int32[n_seg].
 *   workspace: pod_recal_workspace_bytes(n, n_seg), as for pod_recal_moment.
 * pod_recal_apply: records dev float[n_images][max_det][6 + K + 16] (K7's rows: x, y, w, h, score, class, probs[K], C = T Sigma T^T row-major in
 *   xywh form), counts dev int32[n_images]; out another buffer of the records' shape.  A row behind its image's count is written as zeros.  A
 *   live row: box and class copied; score and every probability p -> float(s(beta x(p))) with x and s as in pod_recal_cls_sums (beta == 1.0:
 *   copied bit for bit); C -> M C M^T, M = T diag(s) T^-1 = [[s0,0,0,0],[0,s1,0,0],[s2-s0,0,s2,0],[0,s3-s1,0,s3]], s = scales[0] (n_scale_rows
 *   == 1) or scales[class] (per class; a class outside [0, n_scale_rows) keeps its covariance): A = M C, A[0][k] = s0 C[0][k],
 *   A[1][k] = s1 C[1][k], A[2][k] = (s2 - s0) C[0][k] + s2 C[2][k], A[3][k] = (s3 - s1) C[1][k] + s3 C[3][k]; then C'[k][0] = A[k][0] s0,
 *   C'[k][1] = A[k][1] s1, C'[k][2] = A[k][0] (s2 - s0) + A[k][2] s2, C'[k][3] = A[k][1] (s3 - s1) + A[k][3] s3 -- fp64, each product and
 *   sum rounded on its own, the result rounded once to fp32.  Four scales of 1.0 copy C bit for bit.  scales dev double[n_scale_rows][4].
 * POD_E_INVALID before anything is enqueued: a needed pointer NULL, a size negative or above its limit (n > 2^31 - 1, 4 n_matched likewise,
 *   n_class / n_scale_rows above POD_MAX_CLASSES, n_seg outside [1, POD_RECAL_MAX_SEGMENTS], n_grid outside [1, POD_RECAL_MAX_GRID], j_one
 *   outside the grid, n_q outside [1, POD_RECAL_MAX_QUANTILES], max_seg outside [0, n], max_det < 1, K outside [1, POD_MAX_CLASSES], n_scale_rows
 *   < 1), beta NaN (pod_recal_apply: not positive and finite), x_ready without x, records == out, an fp64 / int64 buffer off 8 bytes. */
#define POD_RECAL_CHUNK          256
#define POD_RECAL_MAX_SEGMENTS   64      /* 4 POD_MAX_CLASSES */
#define POD_RECAL_MAX_GRID       4096
#define POD_RECAL_MAX_QUANTILES  64
size_t pod_recal_workspace_bytes(int64_t n, int32_t n_seg);
int pod_recal_cls_sums(const float* p, const uint8_t* y, int64_t n, double beta, double* x, int32_t x_ready, void* workspace, double* sums,
                       pod_stream_t stream);
int pod_recal_reg_z(const float* means, const float* covs, const float* gt, const int32_t* det_class, int32_t n_matched, int32_t n_class,
                    void* workspace, double* z, int32_t* seg, int64_t* invalid, pod_stream_t stream);
int pod_recal_moment(const double* z, const int32_t* seg, int64_t n, int32_t n_seg, void* workspace, double* zg, int64_t* seg_off,
                     int64_t* count, double* sum, pod_stream_t stream);
int pod_recal_ece_grid(const double* zg, const int64_t* seg_off, int64_t n, int32_t n_seg, int32_t max_seg, const double* scales,
                       int32_t n_grid, int32_t j_one, const double* q, int32_t n_q, void* workspace, double* obj, int32_t* best_j,
                       double* best_obj, double* one_obj, pod_stream_t stream);
int pod_recal_apply(const float* records, const int32_t* counts, int32_t n_images, int32_t max_det, int32_t num_classes, double beta,
                    const double* scales, int32_t n_scale_rows, float* out, pod_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* POD_MI355X_H */
