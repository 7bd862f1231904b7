// K21: the reference's training objective on the head outputs -- anchor labelling and the probabilistic losses with their gradients.
//
// Replaces: detectron2 RetinaNet.label_anchors + Matcher(allow_low_quality_matches=True) as probabilistic_retinanet.py:129-130 calls
// them, and ProbabilisticRetinaNet.losses, probabilistic_retinanet.py:168-333 (fvcore's sigmoid_focal_loss / smooth_l1_loss restated).
//   k_label_best   : one thread per (image, anchor): the best IoU of every ground-truth box over the anchors (Matcher.set_low_quality_matches_)
//                    -- a wavefront max, then one unsigned atomic max on the float's bits per (wavefront, box).  IoU >= 0 and a max is
//                    order-independent: deterministic.
//   k_label_assign : one thread per (image, anchor): the IoUs again (the same instructions, the same bits), max / first arg-max over the
//                    boxes, the threshold labels, the low-quality promotion (IoU == best of that box, literally), the output label.
//   k_train_loss   : one thread per (image, level, anchor shape, cell): consecutive lanes read consecutive cells of a plane (coalesced).
//                    K x S focal-loss terms, 4 smooth-L1 terms, every gradient element of the anchor written (zeros where it adds nothing).
//                    fp32 terms, fp64 accumulation: lane -> wavefront butterfly -> workgroup -> partials[workgroup].
//   k_loss_finish  : one workgroup adds the partials in a fixed order.  No floating-point atomics anywhere: the same bits every run.
#include "pod_train_loss.h"

namespace pod {

constexpr uint32_t STREAM_LOSS = 0x6c6f7300u;   // classification logit samples of the loss (PR:245-246)

// ---------------------------------------------------------------------------------------------------------------------------------
// labelling
// ---------------------------------------------------------------------------------------------------------------------------------
struct KLabelParams {
    const float* anchors;
    const float* gt_boxes;
    const int32_t* gt_classes;
    const int32_t* gt_off;
    int32_t R, K;
    float lo, hi;
    int32_t* labels;
    int32_t* matched_gt;
    int32_t* num_pos;
    uint32_t* best;
};

__global__ void __launch_bounds__(LOSS_BLOCK) k_label_best(const KLabelParams P) {
    const int img = blockIdx.y;
    const int r = blockIdx.x * LOSS_BLOCK + threadIdx.x;
    const int g0 = P.gt_off[img], g1 = P.gt_off[img + 1];
    const bool live = r < P.R;
    Box a = Box{0.0f, 0.0f, 0.0f, 0.0f};
    if (live) a = load_box(P.anchors, r);
    for (int g = g0; g < g1; ++g) {          // uniform over the workgroup
        const float iou = live ? iou_pair(load_box(P.gt_boxes, g), a) : 0.0f;
        const float m = wave_max(iou);
        if ((threadIdx.x & 63) == 0 && m > 0.0f) atomicMax(P.best + g, __float_as_uint(m));
    }
}

__global__ void __launch_bounds__(LOSS_BLOCK) k_label_assign(const KLabelParams P) {
    const int img = blockIdx.y;
    const int r = blockIdx.x * LOSS_BLOCK + threadIdx.x;
    const int g0 = P.gt_off[img], g1 = P.gt_off[img + 1];
    int pos = 0;
    if (r < P.R) {
        const Box a = load_box(P.anchors, r);
        float v = 0.0f;
        int m = -1;
        bool promoted = false;
        for (int g = g0; g < g1; ++g) {
            const float iou = iou_pair(load_box(P.gt_boxes, g), a);
            if (m < 0 || iou > v) {          // first maximum: the lowest box index on ties
                v = iou;
                m = g;
            }
            promoted = promoted || iou == __uint_as_float(P.best[g]);
        }
        int label = P.K;
        if (m >= 0) {
            const int match = (v >= P.hi || promoted) ? 1 : (v >= P.lo ? -1 : 0);
            label = match == 1 ? P.gt_classes[m] : (match == 0 ? P.K : -1);
        }
        const size_t o = (size_t)img * P.R + r;
        P.labels[o] = label;
        P.matched_gt[o] = m;
        pos = (label >= 0 && label < P.K) ? 1 : 0;
    }
    const int n = wave_sum(pos);
    if ((threadIdx.x & 63) == 0 && n > 0) atomicAdd(P.num_pos + img, n);      // integers: order-independent
}

// ---------------------------------------------------------------------------------------------------------------------------------
// losses
// ---------------------------------------------------------------------------------------------------------------------------------
struct KLossParams {
    PodLevel lv[POD_MAX_LEVELS];
    PodLevelGrad gr[POD_MAX_LEVELS];
    int32_t first_block[POD_MAX_LEVELS + 1];
    int32_t n_levels, A, K, D, S, R, n_images, n_gt, has_cls_var, has_grads;
    float alpha, gamma, beta;
    float wts[4];
    uint64_t seed;
    const int32_t* labels;
    const int32_t* matched_gt;
    const float* gt_boxes;
    const float* anchors;
    const float* eps;
    float* eps_out;
    const float* w;
    double* partials;
};

// fvcore sigmoid_focal_loss on one logit, written in z = x for a negative target and z = -x for a positive one:
// 1 - p_t = sigmoid(z) =: q, BCE-with-logits = softplus(z); loss = alpha_t q^gamma softplus(z) -- the same function without the cancellation of
// 1 - p near p = 1.  d loss / d z = alpha_t q^gamma (gamma (1 - q) softplus(z) + q).
__device__ __forceinline__ void focal_term(float x, bool positive, float alpha, float gamma, float& loss, float& dx) {
    const float z = positive ? -x : x;
    const float e = expf(-fabsf(z));
    const float sp = fmaxf(z, 0.0f) + log1pf(e);
    const float q = z >= 0.0f ? __fdiv_rn(1.0f, 1.0f + e) : __fdiv_rn(e, 1.0f + e);
    const float at = alpha >= 0.0f ? (positive ? alpha : 1.0f - alpha) : 1.0f;
    const float qg = gamma == 2.0f ? q * q : (gamma == 0.0f ? 1.0f : powf(q, gamma));
    loss = at * qg * sp;
    const float dz = at * qg * (gamma * (1.0f - q) * sp + q);
    dx = positive ? -dz : dz;
}

__global__ void __launch_bounds__(LOSS_BLOCK) k_train_loss(const KLossParams P) {
    __shared__ double s_part[4][LOSS_BLOCK / 64];
    const int img = blockIdx.y;
    int l = 0;
    while (l + 1 < P.n_levels && (int)blockIdx.x >= P.first_block[l + 1]) ++l;
    const PodLevel& L = P.lv[l];
    const int HW = L.H * L.W;
    const int t = ((int)blockIdx.x - P.first_block[l]) * LOSS_BLOCK + threadIdx.x;
    double acc_cls = 0.0, acc_std = 0.0, acc_nll = 0.0, acc_pos = 0.0;
    if (t < P.A * HW) {
        const int a = t / HW, cell = t - a * HW;
        const int r = L.anchor_base + cell * P.A + a;
        const size_t row = (size_t)img * P.R + r;
        const int label = P.labels[row];
        const bool valid = label >= 0;
        const bool fg = valid && label < P.K;
        float w0 = 0.0f, w1 = 0.0f, w2 = 0.0f;
        if (P.has_grads) {
            w0 = P.w[0];
            w1 = P.w[1];
            w2 = P.w[2];
        }
        // ---- classification, PR:223-282
        const size_t cls_base = (size_t)img * L.run_stride_cls + (size_t)(a * P.K) * HW + cell;
        const size_t n_rows = (size_t)P.n_images * P.R;
        for (int k = 0; k < P.K; ++k) {
            const size_t o = cls_base + (size_t)k * HW;
            float g_logit = 0.0f, g_var = 0.0f;
            if (valid) {
                const float x = L.cls[o];
                const bool positive = k == label;
                if (!P.has_cls_var) {
                    float f, df;
                    focal_term(x, positive, P.alpha, P.gamma, f, df);
                    acc_cls += (double)f;
                    g_logit = w0 * df;
                } else {
                    const float sd = sqrtf(expf(L.cls_var[o]));          // PR:234-235
                    float sum_df = 0.0f, sum_dv = 0.0f;
                    for (int s0 = 0; s0 < P.S; s0 += 8) {
                        f32x8n nat;
                        if (!P.eps) nat = philox_normals8(P.seed, (uint32_t)r, (uint32_t)img, (uint32_t)k | ((uint32_t)(s0 >> 3) << 8), STREAM_LOSS);
#pragma unroll
                        for (int j = 0; j < 8; ++j) {          // (unrolled: the eight normals stay in registers)
                            if (s0 + j >= P.S) break;
                            const size_t eo = ((size_t)(s0 + j) * n_rows + row) * P.K + k;
                            const float e = P.eps ? P.eps[eo] : nat.v[j];
                            if (P.eps_out) P.eps_out[eo] = e;
                            float f, df;
                            focal_term(x + sd * e, positive, P.alpha, P.gamma, f, df);
                            acc_cls += (double)f;
                            sum_df += df;
                            sum_dv += df * e;
                        }
                    }
                    g_logit = w0 * sum_df;
                    g_var = w0 * (sum_dv * (0.5f * sd));              // d std / d logvar = 0.5 std
                }
            } else if (P.eps_out && P.has_cls_var) {
                for (int s = 0; s < P.S; ++s) P.eps_out[((size_t)s * n_rows + row) * P.K + k] = 0.0f;      // ignored anchors draw nothing
            }
            if (P.has_grads) {
                if (P.gr[l].cls) P.gr[l].cls[o] = g_logit;
                if (P.gr[l].cls_var) P.gr[l].cls_var[o] = g_var;
            }
        }
        // ---- regression, PR:194, PR:285-331
        const int mg = fg ? P.matched_gt[row] : -1;
        const bool reg = fg && mg >= 0 && mg < P.n_gt;
        float tgt[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (reg) box_deltas(load_box(P.anchors, r), load_box(P.gt_boxes, mg), P.wts, tgt);
        if (fg) acc_pos = 1.0;
        const size_t d_base = (size_t)img * L.run_stride_delta + (size_t)(a * 4) * HW + cell;
        const size_t v_base = (size_t)img * L.run_stride_reg + (size_t)(a * 4) * HW + cell;
        for (int j = 0; j < 4; ++j) {
            float g_d = 0.0f, g_v = 0.0f;
            if (reg) {
                float sl, dd;
                smooth_l1_term(L.delta[d_base + (size_t)j * HW] - tgt[j], P.beta, sl, dd);
                acc_std += (double)sl;
                g_d = w1 * dd;
                if (P.D == 4) {          // PR:295-307
                    const float lvj = L.reg_var[v_base + (size_t)j * HW];
                    const float c = fminf(fmaxf(lvj, -7.0f), 7.0f);
                    const float h = 0.5f * expf(-c);
                    acc_nll += (double)(h * sl + 0.5f * c);
                    g_d += w2 * (h * dd);
                    g_v = (lvj >= -7.0f && lvj <= 7.0f) ? w2 * (0.5f - h * sl) : 0.0f;
                }
            }
            if (P.has_grads) {
                if (P.gr[l].delta) P.gr[l].delta[d_base + (size_t)j * HW] = g_d;
                if (P.D == 4 && P.gr[l].reg_var) P.gr[l].reg_var[v_base + (size_t)j * HW] = g_v;
            }
        }
    }
    acc_cls = wave_sum(acc_cls);
    acc_std = wave_sum(acc_std);
    acc_nll = wave_sum(acc_nll);
    acc_pos = wave_sum(acc_pos);
    const int wv = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        s_part[0][wv] = acc_cls;
        s_part[1][wv] = acc_std;
        s_part[2][wv] = acc_nll;
        s_part[3][wv] = acc_pos;
    }
    __syncthreads();
    if (threadIdx.x < 4) {
        double s = s_part[threadIdx.x][0];
        for (int i = 1; i < LOSS_BLOCK / 64; ++i) s += s_part[threadIdx.x][i];
        P.partials[((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 4 + threadIdx.x] = s;
    }
}

__global__ void __launch_bounds__(LOSS_BLOCK) k_loss_finish(const double* partials, int64_t n, double* sums) {
    __shared__ double s_sum[4][LOSS_BLOCK];
    double a[4] = {0.0, 0.0, 0.0, 0.0};
    for (int64_t i = threadIdx.x; i < n; i += LOSS_BLOCK)
        for (int q = 0; q < 4; ++q) a[q] += partials[i * 4 + q];
    for (int q = 0; q < 4; ++q) s_sum[q][threadIdx.x] = a[q];
    __syncthreads();
    for (int step = LOSS_BLOCK / 2; step > 0; step >>= 1) {
        if ((int)threadIdx.x < step)
            for (int q = 0; q < 4; ++q) s_sum[q][threadIdx.x] += s_sum[q][threadIdx.x + step];
        __syncthreads();
    }
    if (threadIdx.x < 4) sums[threadIdx.x] = s_sum[threadIdx.x][0];
}

}  // namespace pod

extern "C" int pod_label_anchors(const float* anchors, int32_t R, const float* gt_boxes, const int32_t* gt_classes, const int32_t* gt_off,
                                 int32_t n_images, int32_t n_gt, int32_t num_classes, float iou_low, float iou_high, int32_t* labels,
                                 int32_t* matched_gt, int32_t* num_pos, uint32_t* scratch, pod_stream_t stream) {
    if (!anchors || R < 1 || n_images < 1 || n_images > 65535 || n_gt < 0 || num_classes < 1 || !gt_off || !labels || !matched_gt || !num_pos)
        return POD_E_INVALID;
    if (n_gt > 0 && (!gt_boxes || !gt_classes || !scratch)) return POD_E_INVALID;
    if (!(iou_low <= iou_high)) return POD_E_INVALID;
    pod::KLabelParams P;
    P.anchors = anchors; P.gt_boxes = gt_boxes; P.gt_classes = gt_classes; P.gt_off = gt_off; P.R = R; P.K = num_classes;
    P.lo = iou_low; P.hi = iou_high; P.labels = labels; P.matched_gt = matched_gt; P.num_pos = num_pos; P.best = scratch;
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(num_pos, 0, sizeof(int32_t) * (size_t)n_images, st) != hipSuccess) return POD_E_LAUNCH;
    const dim3 grid((R + pod::LOSS_BLOCK - 1) / pod::LOSS_BLOCK, n_images);
    if (n_gt > 0) {
        if (hipMemsetAsync(scratch, 0, sizeof(uint32_t) * (size_t)n_gt, st) != hipSuccess) return POD_E_LAUNCH;
        hipLaunchKernelGGL(pod::k_label_best, grid, dim3(pod::LOSS_BLOCK), 0, st, P);
        POD_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(pod::k_label_assign, grid, dim3(pod::LOSS_BLOCK), 0, st, P);
    POD_CHECK_LAUNCH();
    return POD_OK;
}

extern "C" int64_t pod_train_loss_partials(const PodConfig* cfg, const PodLevel* levels) {
    if (!pod::loss_cfg_ok(cfg, levels)) return 0;
    const int64_t n = pod::loss_blocks(cfg, levels, nullptr);
    return n < 0 ? 0 : 4 * n * cfg->n_runs;
}

extern "C" int pod_train_loss(const PodConfig* cfg, const PodLevel* levels, const PodLevelGrad* grads, const int32_t* labels,
                              const int32_t* matched_gt, const float* gt_boxes, int32_t n_gt, const float* anchors, int32_t R,
                              float alpha, float gamma, float smooth_l1_beta, const float* eps_cls, float* eps_out, const float* w,
                              double* partials, double* sums, pod_stream_t stream) {
    if (!pod::loss_cfg_ok(cfg, levels) || !labels || !matched_gt || !anchors || !partials || !sums || R < 1 || n_gt < 0) return POD_E_INVALID;
    if (cfg->cov_dims != 0 && cfg->cov_dims != 4) return POD_E_INVALID;      // the reference defines no loss for the full covariance
    if (n_gt > 0 && !gt_boxes) return POD_E_INVALID;
    if (grads && !w) return POD_E_INVALID;
    if (cfg->has_cls_var && (cfg->cls_samples < 1 || cfg->cls_samples > POD_MAX_CLS_SAMPLES)) return POD_E_INVALID;
    if (!(gamma >= 0.0f) || !(smooth_l1_beta >= 0.0f)) return POD_E_INVALID;
    pod::KLossParams P;
    const int64_t n_blocks = pod::loss_blocks(cfg, levels, P.first_block);
    if (n_blocks < 1) return POD_E_INVALID;
    int64_t anchors_seen = 0;
    for (int l = 0; l < cfg->n_levels; ++l) {
        const PodLevel& L = levels[l];
        if (!L.cls || !L.delta || (cfg->has_cls_var && !L.cls_var) || (cfg->cov_dims == 4 && !L.reg_var)) return POD_E_INVALID;
        const int64_t n_l = (int64_t)cfg->num_anchors * L.H * L.W;
        if (L.anchor_base < 0 || (int64_t)L.anchor_base + n_l > R) return POD_E_INVALID;      // every label / anchor row the kernel reads exists
        anchors_seen += n_l;
        P.lv[l] = L;
        P.gr[l] = grads ? grads[l] : PodLevelGrad{nullptr, nullptr, nullptr, nullptr};
    }
    if (anchors_seen != R) return POD_E_INVALID;
    P.n_levels = cfg->n_levels; P.A = cfg->num_anchors; P.K = cfg->num_classes; P.D = cfg->cov_dims; P.S = cfg->has_cls_var ? cfg->cls_samples : 0;
    P.R = R; P.n_images = cfg->n_runs; P.n_gt = n_gt; P.has_cls_var = cfg->has_cls_var ? 1 : 0; P.has_grads = grads ? 1 : 0;
    P.alpha = alpha; P.gamma = gamma; P.beta = smooth_l1_beta;
    for (int i = 0; i < 4; ++i) P.wts[i] = cfg->box_weights[i];
    P.seed = cfg->philox_seed;
    P.labels = labels; P.matched_gt = matched_gt; P.gt_boxes = gt_boxes; P.anchors = anchors;
    P.eps = cfg->has_cls_var ? eps_cls : nullptr; P.eps_out = cfg->has_cls_var ? eps_out : nullptr; P.w = w; P.partials = partials;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(pod::k_train_loss, dim3((unsigned)n_blocks, (unsigned)cfg->n_runs), dim3(pod::LOSS_BLOCK), 0, st, P);
    POD_CHECK_LAUNCH();
    hipLaunchKernelGGL(pod::k_loss_finish, dim3(1), dim3(pod::LOSS_BLOCK), 0, st, (const double*)partials, (int64_t)(n_blocks * cfg->n_runs), sums);
    POD_CHECK_LAUNCH();
    return POD_OK;
}
