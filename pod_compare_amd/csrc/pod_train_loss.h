// What the kernels of the training objective share (k21_train_loss.hip, k27_reg_score_loss.hip): the regression target, the smooth-L1
// term, the workgroup enumeration over the levels and the configuration check.  One copy, so that the score losses of K27 see the bits
// K21's regression terms see.
#pragma once

#include "pod_device.h"

namespace pod {

constexpr int LOSS_BLOCK = 256;

__device__ __forceinline__ void smooth_l1_term(float d, float beta, float& loss, float& dd) {
    const float ad = fabsf(d);
    const float sgn = d > 0.0f ? 1.0f : (d < 0.0f ? -1.0f : 0.0f);
    if (beta < 1e-5f) {
        loss = ad;
        dd = sgn;
    } else if (ad < beta) {
        loss = __fdiv_rn(0.5f * d * d, beta);
        dd = __fdiv_rn(d, beta);
    } else {
        loss = ad - 0.5f * beta;
        dd = sgn;
    }
}

// Box2BoxTransform.get_deltas of anchor s towards box g
__device__ __forceinline__ void box_deltas(const Box& s, const Box& g, const float* wts, float* tgt) {
    const float sw = s.x2 - s.x1, sh = s.y2 - s.y1;
    const float scx = s.x1 + 0.5f * sw, scy = s.y1 + 0.5f * sh;
    const float tw = g.x2 - g.x1, th = g.y2 - g.y1;
    const float tcx = g.x1 + 0.5f * tw, tcy = g.y1 + 0.5f * th;
    tgt[0] = __fdiv_rn(wts[0] * (tcx - scx), sw);
    tgt[1] = __fdiv_rn(wts[1] * (tcy - scy), sh);
    tgt[2] = wts[2] * logf(__fdiv_rn(tw, sw));
    tgt[3] = wts[3] * logf(__fdiv_rn(th, sh));
}

// Host: the workgroups of a launch with one thread per (level, anchor shape, cell), level after level; first_block (n_levels + 1) or NULL.
static int64_t loss_blocks(const PodConfig* cfg, const PodLevel* levels, int32_t* first_block) {
    int64_t n = 0;
    for (int l = 0; l < cfg->n_levels; ++l) {
        if (first_block) first_block[l] = (int32_t)n;
        if (levels[l].H < 1 || levels[l].W < 1) return -1;
        n += ((int64_t)cfg->num_anchors * levels[l].H * levels[l].W + LOSS_BLOCK - 1) / LOSS_BLOCK;
        if (n > 0x7FFFFFFF) return -1;
    }
    if (first_block) first_block[cfg->n_levels] = (int32_t)n;
    return n;
}

static bool loss_cfg_ok(const PodConfig* cfg, const PodLevel* levels) {
    return cfg && levels && cfg->n_levels >= 1 && cfg->n_levels <= POD_MAX_LEVELS && cfg->n_runs >= 1 && cfg->n_runs <= 65535 &&
           cfg->num_anchors >= 1 && cfg->num_classes >= 1 && cfg->num_classes < POD_MAX_CLASSES;
}

}  // namespace pod
