// K27: the two box-covariance objectives the reference's configuration names beside the NLL -- `second_moment_matching` and `energy_loss`
// (BBOX_COV_LOSS.NAME; the definitions are include/pod_mi355x.h's, the reference names them and defines neither) -- on the positive
// anchors, with their gradients added to the planes pod_train_loss has written.
//
// Serves: ProbabilisticRetinaNet.losses, probabilistic_retinanet.py:285-331, where one of these sums takes the place of the NLL sum.
//   k_reg_score<POD_REG_LOSS_MOMENTS> : one thread per (image, level, anchor shape, cell), K21's enumeration: a positive anchor's four terms,
//                                       its gradients, zeros in the reg_var planes everywhere else.
//   k_reg_score<POD_REG_LOSS_ENERGY>  : the same threads first list the workgroup's positives in LDS in thread order (ballot + prefix, no
//                                       atomics) and write the zeros; the four wavefronts then take the listed positives in turn.  A lane
//                                       owns the sample pairs (2c, 2c + 1), c = lane, lane + 64, ...: one Philox4x32-10 call is the eight
//                                       normals of a pair, sample 2c + 2 comes from the neighbouring lane (lane 63: from lane 0 of the next
//                                       trip, drawn one trip ahead).  Butterfly sums, one lane stores the anchor's gradient.
//   k_score_finish                    : one workgroup adds the partials in index order.
// The launch record, the pair fetch, the listing, the workgroup sum and the finish kernel are pod_train_loss.h's: K28 (the full covariance)
// runs on the same ones.
// fp32 terms, fp64 accumulation: lane -> wavefront butterfly -> workgroup -> partials[workgroup].  No floating-point atomics: the same bits
// every run.  A draw depends on (seed, image, anchor, sample, coordinate) alone -- not on the grid, the batch or the other positives.
#include "pod_train_loss.h"

namespace pod {

template <int KIND>
__global__ void __launch_bounds__(LOSS_BLOCK) k_reg_score(const KScoreParams P) {
    __shared__ double s_part[SCORE_WAVES];
    __shared__ int s_list[LOSS_BLOCK];
    __shared__ int s_count[SCORE_WAVES];
    const int img = blockIdx.y;
    int l = 0;
    while (l + 1 < P.n_levels && (int)blockIdx.x >= P.first_block[l + 1]) ++l;
    const PodLevel& L = P.lv[l];
    const int HW = L.H * L.W;
    const int t = ((int)blockIdx.x - P.first_block[l]) * LOSS_BLOCK + threadIdx.x;
    const size_t n_rows = (size_t)P.n_images * P.R;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    float w2 = 0.0f;
    if (P.has_grads) w2 = P.w[2];
    double acc = 0.0;
    bool pos = false;
    if (t < P.A * HW) {
        const int a = t / HW, cell = t - a * HW;
        const int r = L.anchor_base + cell * P.A + a;
        const size_t row = (size_t)img * P.R + r;
        const int label = P.labels[row];
        const int mg = (label >= 0 && label < P.K) ? P.matched_gt[row] : -1;
        pos = mg >= 0 && mg < P.n_gt;
        const size_t d_base = (size_t)img * L.run_stride_delta + (size_t)(a * 4) * HW + cell;
        const size_t v_base = (size_t)img * L.run_stride_reg + (size_t)(a * 4) * HW + cell;
        if (KIND == POD_REG_LOSS_MOMENTS) {
            float tgt[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            if (pos) box_deltas(load_box(P.anchors, r), load_box(P.gt_boxes, mg), P.wts, tgt);
            for (int j = 0; j < 4; ++j) {
                float g_v = 0.0f;
                if (pos) {
                    const float lvj = L.reg_var[v_base + (size_t)j * HW];
                    const float d = L.delta[d_base + (size_t)j * HW] - tgt[j];
                    const float v = expf(fminf(fmaxf(lvj, -7.0f), 7.0f));
                    float l1, dd1, l2, dd2;
                    smooth_l1_term(d, P.beta, l1, dd1);
                    smooth_l1_term(v - d * d, P.beta, l2, dd2);
                    acc += (double)l1;
                    acc += (double)l2;
                    g_v = (lvj >= -7.0f && lvj <= 7.0f) ? w2 * (dd2 * v) : 0.0f;
                    if (P.has_grads && P.gr[l].delta) {
                        float* gd = P.gr[l].delta + d_base + (size_t)j * HW;
                        *gd = *gd + w2 * (dd1 - (2.0f * d) * dd2);
                    }
                }
                if (P.has_grads && P.gr[l].reg_var) P.gr[l].reg_var[v_base + (size_t)j * HW] = g_v;
            }
        } else if (!pos) {
            if (P.has_grads && P.gr[l].reg_var)
                for (int j = 0; j < 4; ++j) P.gr[l].reg_var[v_base + (size_t)j * HW] = 0.0f;
            if (P.eps_out) score_zero_draws(P, row, n_rows);
        }
    }
    if (KIND == POD_REG_LOSS_ENERGY) {
        const int n_pos = score_list_positives(pos, s_list, s_count);          // the workgroup's positives, in thread order
        // ---- a wavefront per listed positive, a lane per sample pair
        const float inv_m = __fdiv_rn(1.0f, (float)P.M);
        const int trips = (P.M / 2 + 1 + 63) / 64;
        for (int p = wv; p < n_pos; p += SCORE_WAVES) {
            const int tl = __builtin_amdgcn_readfirstlane(s_list[p]);
            const int tp = ((int)blockIdx.x - P.first_block[l]) * LOSS_BLOCK + tl;
            const int a = tp / HW, cell = tp - a * HW;
            const int r = L.anchor_base + cell * P.A + a;
            const size_t row = (size_t)img * P.R + r;
            const size_t d_base = (size_t)img * L.run_stride_delta + (size_t)(a * 4) * HW + cell;
            const size_t v_base = (size_t)img * L.run_stride_reg + (size_t)(a * 4) * HW + cell;
            float tgt[4], d[4], sg[4], lvj[4];
            box_deltas(load_box(P.anchors, r), load_box(P.gt_boxes, P.matched_gt[row]), P.wts, tgt);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                lvj[j] = L.reg_var[v_base + (size_t)j * HW];
                d[j] = L.delta[d_base + (size_t)j * HW] - tgt[j];
                sg[j] = expf(0.5f * fminf(fmaxf(lvj[j], -7.0f), 7.0f));
            }
            double a1 = 0.0, a2 = 0.0;                        // sums of sl1(u1), sl1(u2) of this lane's samples
            float gd[4] = {0.0f, 0.0f, 0.0f, 0.0f}, gv1[4] = {0.0f, 0.0f, 0.0f, 0.0f}, gv2[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            f32x8n cur = score_pair(P, r, img, row, n_rows, lane);
            for (int i = 0; i < trips; ++i) {                 // (uniform over the wavefront: the shuffles below see every lane)
                const int c = i * 64 + lane;
                const f32x8n nxt = score_pair(P, r, img, row, n_rows, c + 64);
                float e2[4];                                  // sample 2c + 2: the first half of pair c + 1
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float from_next_lane = __shfl_down(cur.v[j], 1, 64);
                    const float from_next_trip = __shfl(nxt.v[j], 0, 64);
                    e2[j] = lane == 63 ? from_next_trip : from_next_lane;
                }
                if (P.eps_out) {
#pragma unroll
                    for (int h = 0; h < 2; ++h)
                        if (2 * c + h <= P.M)
                            *reinterpret_cast<float4*>(P.eps_out + ((size_t)(2 * c + h) * n_rows + row) * 4) =
                                float4{cur.v[4 * h], cur.v[4 * h + 1], cur.v[4 * h + 2], cur.v[4 * h + 3]};
                }
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    if (2 * c + h < P.M) {
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            const float e = cur.v[4 * h + j];
                            const float de = e - (h == 0 ? cur.v[4 + j] : e2[j]);
                            float l1, dd1, l2, dd2;
                            smooth_l1_term(d[j] + sg[j] * e, P.beta, l1, dd1);
                            smooth_l1_term(sg[j] * de, P.beta, l2, dd2);
                            a1 += (double)l1;
                            a2 += (double)l2;
                            gd[j] += dd1;
                            gv1[j] += dd1 * e;
                            gv2[j] += dd2 * de;
                        }
                    }
                }
                cur = nxt;
            }
            a1 = wave_sum(a1);
            a2 = wave_sum(a2);
            if (lane == 0) acc += (2.0 * a1 - a2) / (double)P.M;
            if (P.has_grads) {                                // (uniform)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float s_d = wave_sum(gd[j]), s_v1 = wave_sum(gv1[j]), s_v2 = wave_sum(gv2[j]);
                    if (lane == 0) {
                        if (P.gr[l].delta) {
                            float* g = P.gr[l].delta + d_base + (size_t)j * HW;
                            *g = *g + w2 * ((2.0f * inv_m) * s_d);
                        }
                        if (P.gr[l].reg_var) {
                            const float dv = (0.5f * sg[j]) * ((2.0f * inv_m) * s_v1 - inv_m * s_v2);
                            P.gr[l].reg_var[v_base + (size_t)j * HW] = (lvj[j] >= -7.0f && lvj[j] <= 7.0f) ? w2 * dv : 0.0f;
                        }
                    }
                }
            }
        }
    }
    score_block_sum(acc, s_part, P.partials);
}

}  // namespace pod

extern "C" int64_t pod_reg_score_partials(const PodConfig* cfg, const PodLevel* levels) { return pod::score_partials(cfg, levels); }

extern "C" int pod_reg_score_loss(const PodConfig* cfg, const PodLevel* levels, const PodLevelGrad* grads, const int32_t* labels,
                                  const int32_t* matched_gt, const float* gt_boxes, int32_t n_gt, const float* anchors, int32_t R,
                                  int32_t kind, int32_t num_samples, float smooth_l1_beta, const float* eps_reg, float* eps_out,
                                  const float* w, double* partials, double* sum, pod_stream_t stream) {
    pod::KScoreParams P;
    int64_t n_blocks = 0;
    // what pod_train_loss refuses, and: both losses need the diagonal covariance head
    if (pod::score_params(cfg, levels, grads, labels, matched_gt, gt_boxes, n_gt, anchors, R, 4, kind, 2, POD_REG_LOSS_ENERGY, num_samples,
                          smooth_l1_beta, eps_reg, eps_out, w, partials, sum, P, n_blocks) != POD_OK) return POD_E_INVALID;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)n_blocks, (unsigned)cfg->n_runs);
    if (kind == POD_REG_LOSS_ENERGY)
        hipLaunchKernelGGL(pod::k_reg_score<POD_REG_LOSS_ENERGY>, grid, dim3(pod::LOSS_BLOCK), 0, st, P);
    else
        hipLaunchKernelGGL(pod::k_reg_score<POD_REG_LOSS_MOMENTS>, grid, dim3(pod::LOSS_BLOCK), 0, st, P);
    POD_CHECK_LAUNCH();
    hipLaunchKernelGGL(pod::k_score_finish, dim3(1), dim3(pod::LOSS_BLOCK), 0, st, (const double*)partials, (int64_t)(n_blocks * cfg->n_runs), sum);
    POD_CHECK_LAUNCH();
    return POD_OK;
}
