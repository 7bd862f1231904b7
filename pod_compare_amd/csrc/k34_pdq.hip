// K34: PDQ, the probability-based detection quality (Hall et al.), as include/pod_mi355x.h defines it -- the reference's README sends the
// user to a separate CPU tool for it.  Two kernels:
//   k_pdq_pairs  : one workgroup per (image, detection).  The detection's two corner Gaussians give P(pixel in box) = A B and its
//                  complement Q = Ac + A Bc (never 1 - P) ONCE per pixel of the detection's region of interest, a superset of the segment
//                  T = {P >= p_min} clipped to the frame.  Columns go in chunks of 256 (a thread owns a column: its four Phi are hoisted
//                  out of the row loop), rows ascending inside a chunk.  Per row the chunk's log P, log max(Q, small) and the segment flag
//                  go to LDS; thread i owns ground truth i's accumulators and adds, in column order, the part of the row left of its box
//                  and right of it to the background sum and the part inside to the foreground sum -- sequential compensated fp64 sums,
//                  no difference of prefix sums, so a three-pixel box loses nothing to a row's total.  Phi2's integral is Gauss-Legendre,
//                  20 points a panel, panels of at most asin(0.99) / 4 (1 .. 4 of them, none at rho = 0); its nodes are a table in LDS.
//   k_pdq_assign : one wavefront per image.  Shortest augmenting paths with potentials on cost -pPDQ, the G real rows against
//                  n = max(G, D) columns (the zero rows of the padded square matrix change no real row's cost), lanes over the columns,
//                  ties to the lowest column: additions, subtractions and comparisons only, so a host restatement is bit-equal.
// No atomics anywhere: a pair's numbers depend on its detection, its ground truth, the frame and p_min alone.
#include "pod_device.h"

namespace pod {

constexpr int PDQ_BLOCK = 256;
constexpr int PDQ_GL = 20;                       // points per panel
constexpr int PDQ_MAX_PANELS = 4;
constexpr int PDQ_MAX_NODES = PDQ_GL * PDQ_MAX_PANELS;
constexpr double PDQ_SMALL = 1e-14;
constexpr double PDQ_RHO_MAX = 0.99;
constexpr double PDQ_INV_SQRT2 = 0.70710678118654752440;
constexpr double PDQ_INV_2PI = 0.15915494309189533577;

// the positive half of the 20-point Gauss-Legendre rule on [-1, 1]
__constant__ double PDQ_GL_X[PDQ_GL / 2] = {0.076526521133497338, 0.2277858511416451, 0.37370608871541955, 0.51086700195082713, 0.63605368072651502,
                                            0.7463319064601508, 0.83911697182221878, 0.91223442825132584, 0.96397192727791381, 0.99312859918509488};
__constant__ double PDQ_GL_W[PDQ_GL / 2] = {0.15275338713072578, 0.14917298647260366, 0.14209610931838187, 0.13168863844917653, 0.11819453196151825,
                                            0.10193011981724026, 0.083276741576704671, 0.062672048334109443, 0.040601429800386217, 0.017614007139153273};

struct KPdqPairsParams {
    const int32_t* frames;      // workspace copies of the host tables
    const int32_t* det_off;
    const int32_t* gt_off;
    const int64_t* pair_off;
    const float* means;
    const float* covs;
    const float* probs;
    const float* gt_boxes;
    const int32_t* gt_classes;
    double* quality;
    double* sums;
    int32_t* det_invalid;
    double p_min, z;            // z = Phi^-1(p_min)
    int64_t n_pairs;
    int32_t n_images, K;
};

__device__ __forceinline__ double pdq_phi(double x) { return 0.5 * erfc(-x * PDQ_INV_SQRT2); }

// pixel index bound: v clamped into [0, hi] (NaN -> 0), as an int
__device__ __forceinline__ int pdq_clamp_index(double v, int hi) { return (int)fmin(fmax(v, 0.0), (double)hi); }

// the image of global detection d: the last m with det_off[m] <= d
__device__ __forceinline__ int pdq_image_of(const int32_t* det_off, int n_images, int d) {
    int lo = 0, hi = n_images - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (det_off[mid] <= d) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// Phi2's integral term (1 / 2 pi) int_0^{asin rho} exp(-(h^2 + k^2 - 2 h k sin t) / (2 cos^2 t)) dt from the corner's node table
__device__ __forceinline__ double pdq_integral(const double* ts, const double* tc, const double* tw, int n, double h, double k) {
    const double a = h * h + k * k, b = 2.0 * h * k;
    double s = 0.0;
    for (int q = 0; q < n; ++q) s += tw[q] * exp(-(a - b * ts[q]) * tc[q]);
    return s;
}

// s += x, compensated (Kahan): a sum of thousands of terms near log small = -32 stays within a few ulp of its value, whatever their count
__device__ __forceinline__ void pdq_add(double& s, double& comp, double x) {
    const double y = x - comp;
    const double t = s + y;
    comp = (t - s) - y;
    s = t;
}

__global__ void __launch_bounds__(PDQ_BLOCK) k_pdq_pairs(const KPdqPairsParams P) {
    __shared__ double t_sin[2][PDQ_MAX_NODES], t_inv[2][PDQ_MAX_NODES], t_w[2][PDQ_MAX_NODES];
    __shared__ double row_lp[PDQ_BLOCK], row_lq[PDQ_BLOCK];
    __shared__ int row_in[PDQ_BLOCK];
    const int tid = (int)threadIdx.x;
    const int d = (int)blockIdx.x;
    const int m = pdq_image_of(P.det_off, P.n_images, d);
    const int W = P.frames[2 * m], H = P.frames[2 * m + 1];
    const int G = P.gt_off[m + 1] - P.gt_off[m], D = P.det_off[m + 1] - P.det_off[m], j = d - P.det_off[m];

    // the two corner blocks of cov + 1e-2 I: the sum in fp32, then widened; the lower triangle is read
    const float* cv = P.covs + (size_t)d * 16;
    double mu[4], sd[4], rho[2];
    bool valid = true;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        mu[c] = (double)P.means[(size_t)d * 4 + c];
        const double var = (double)(cv[5 * c] + 1e-2f);
        valid = valid && isfinite(mu[c]) && isfinite(var) && var > 0.0;
        sd[c] = sqrt(var);
    }
#pragma unroll
    for (int b = 0; b < 2; ++b) {
        const double r = (double)cv[(2 * b + 1) * 4 + 2 * b] / (sd[2 * b] * sd[2 * b + 1]);
        valid = valid && isfinite(r);
        rho[b] = fmin(fmax(r, -PDQ_RHO_MAX), PDQ_RHO_MAX);
    }
    if (tid == 0 && P.det_invalid) P.det_invalid[d] = valid ? 0 : 1;
    if (G == 0) return;

    // the node tables of the two corners: panels of equal width, at most asin(0.99) / 4 each
    int nodes[2];
#pragma unroll
    for (int b = 0; b < 2; ++b) {
        const double top = valid ? asin(rho[b]) : 0.0;
        const int panels = top == 0.0 ? 0 : min(PDQ_MAX_PANELS, (int)ceil(fabs(top) / (asin(PDQ_RHO_MAX) / PDQ_MAX_PANELS)));
        nodes[b] = panels * PDQ_GL;
        if (tid < nodes[b]) {
            const int panel = tid / PDQ_GL, q = tid % PDQ_GL;
            const double half = 0.5 * top / (double)panels;
            const double x = q < PDQ_GL / 2 ? -PDQ_GL_X[PDQ_GL / 2 - 1 - q] : PDQ_GL_X[q - PDQ_GL / 2];
            const double w = q < PDQ_GL / 2 ? PDQ_GL_W[PDQ_GL / 2 - 1 - q] : PDQ_GL_W[q - PDQ_GL / 2];
            const double t = half * (2.0 * (double)panel + 1.0) + half * x;
            const double c = cos(t);
            t_sin[b][tid] = sin(t);
            t_inv[b][tid] = 1.0 / (2.0 * c * c);
            t_w[b][tid] = w * half * PDQ_INV_2PI;
        }
    }

    // this thread's ground truth: its pixel ranges [ga, gb) x [gc, gd) (centres in [x1, x2) x [y1, y2), clipped to the frame)
    int ga = 0, gb = 0, gc = 0, gd = 0;
    if (tid < G) {
        const float* g = P.gt_boxes + (size_t)(P.gt_off[m] + tid) * 4;
        ga = pdq_clamp_index(ceil((double)g[0] - 0.5), W);
        gb = pdq_clamp_index(ceil((double)g[2] - 0.5), W);
        gc = pdq_clamp_index(ceil((double)g[1] - 0.5), H);
        gd = pdq_clamp_index(ceil((double)g[3] - 0.5), H);
    }
    const long long n_i = (long long)max(gb - ga, 0) * (long long)max(gd - gc, 0);

    // the region of interest: P <= Phi of each single argument, so a column with cx < mu_x1 + z sd_x1 or cx > mu_x2 - z sd_x2 holds no
    // pixel of T (rows likewise); one pixel wider on every side, clipped to the frame.  Inclusive bounds.
    int u0 = 0, u1 = -1, v0 = 0, v1 = -1;
    if (valid) {
        u0 = pdq_clamp_index(floor(mu[0] + P.z * sd[0] - 0.5) - 1.0, W);
        u1 = pdq_clamp_index(ceil(mu[2] - P.z * sd[2] - 0.5) + 2.0, W) - 1;
        v0 = pdq_clamp_index(floor(mu[1] + P.z * sd[1] - 0.5) - 1.0, H);
        v1 = pdq_clamp_index(ceil(mu[3] - P.z * sd[3] - 0.5) + 2.0, H) - 1;
    }
    __syncthreads();

    const double log_small = log(PDQ_SMALL);
    double fg = 0.0, bg = 0.0;          // sum of log P over S_i and T; sum of log max(Q, small) over T \ S_i
    double fg_c = 0.0, bg_c = 0.0;      // their compensation terms
    long long cnt = 0;                  // |S_i and T|
    if (v0 <= v1) {
        for (int ub = u0; ub <= u1; ub += PDQ_BLOCK) {
            const int n = min(PDQ_BLOCK, u1 - ub + 1);
            const bool active = tid < n;
            const double cx = (double)(ub + tid) + 0.5;
            const double hx1 = (cx - mu[0]) / sd[0], hx2 = (mu[2] - cx) / sd[2];
            const double px1 = pdq_phi(hx1), nx1 = pdq_phi(-hx1), px2 = pdq_phi(hx2), nx2 = pdq_phi(-hx2);
            const int lo_i = min(max(ga - ub, 0), n), hi_i = max(min(max(gb - ub, 0), n), lo_i);
            for (int v = v0; v <= v1; ++v) {
                if (active) {
                    const double cy = (double)v + 0.5;
                    const double ky1 = (cy - mu[1]) / sd[1], ky2 = (mu[3] - cy) / sd[3];
                    const double py1 = pdq_phi(ky1), ny1 = pdq_phi(-ky1), py2 = pdq_phi(ky2), ny2 = pdq_phi(-ky2);
                    const double i_tl = pdq_integral(t_sin[0], t_inv[0], t_w[0], nodes[0], hx1, ky1);
                    const double i_br = pdq_integral(t_sin[1], t_inv[1], t_w[1], nodes[1], hx2, ky2);
                    const double A = px1 * py1 + i_tl, B = px2 * py2 + i_br;
                    const double p = A * B;
                    const bool in_t = p >= P.p_min;
                    double lp = 0.0, lq = 0.0;
                    if (in_t) {
                        // Phi2(-h, -k; rho) has the same integral term: h^2 + k^2 and h k do not change
                        const double Ac = nx1 + ny1 - (nx1 * ny1 + i_tl), Bc = nx2 + ny2 - (nx2 * ny2 + i_br);
                        lp = log(fmax(p, PDQ_SMALL));
                        lq = log(fmax(Ac + A * Bc, PDQ_SMALL));
                    }
                    row_lp[tid] = lp;
                    row_lq[tid] = lq;
                    row_in[tid] = in_t ? 1 : 0;
                }
                __syncthreads();
                if (tid < G) {
                    const bool in_rows = v >= gc && v < gd;
                    const int lo = in_rows ? lo_i : 0, hi = in_rows ? hi_i : 0;
                    for (int c = 0; c < lo; ++c) pdq_add(bg, bg_c, row_lq[c]);
                    for (int c = lo; c < hi; ++c) {
                        pdq_add(fg, fg_c, row_lp[c]);
                        cnt += row_in[c];
                    }
                    for (int c = hi; c < n; ++c) pdq_add(bg, bg_c, row_lq[c]);
                }
                __syncthreads();
            }
        }
    }
    if (tid >= G) return;
    double out[5] = {0.0, 0.0, 0.0, 0.0, 0.0}, s_fg = 0.0, s_bg = 0.0;
    if (valid && n_i > 0 && cnt > 0) {
        const int cls = P.gt_classes[P.gt_off[m] + tid];
        const double q_label = cls >= 0 && cls < P.K ? (double)P.probs[(size_t)d * P.K + cls] : 0.0;
        s_fg = fg + log_small * (double)(n_i - cnt);          // the pixels of S_i outside T count log small each
        s_bg = bg;
        const double l_fg = -s_fg / (double)n_i, l_bg = -s_bg / (double)n_i;
        out[1] = exp(-(l_fg + l_bg));
        out[2] = q_label;
        out[3] = exp(-l_fg);
        out[4] = exp(-l_bg);
        out[0] = sqrt(out[1] * q_label);
    }
    const int64_t at = P.pair_off[m] + (int64_t)tid * D + j;
#pragma unroll
    for (int q = 0; q < 5; ++q) P.quality[(int64_t)q * P.n_pairs + at] = out[q];
    if (P.sums) {
        P.sums[at] = s_fg;
        P.sums[P.n_pairs + at] = s_bg;
    }
}

struct KPdqAssignParams {
    const int32_t* det_off;
    const int32_t* gt_off;
    const int64_t* pair_off;
    const double* quality;
    int32_t* gt_match;
    int32_t* counts;
    double* image_sums;
    int64_t n_pairs;
};

constexpr int PDQ_SIDE = POD_PDQ_MAX_SIDE;

__global__ void __launch_bounds__(64) k_pdq_assign(const KPdqAssignParams P) {
    // columns 1 .. n, column 0 the virtual start of a path; rows 1 .. G
    __shared__ double u[PDQ_SIDE + 1], vv[PDQ_SIDE + 1], minv[PDQ_SIDE + 1];
    __shared__ int p[PDQ_SIDE + 1], way[PDQ_SIDE + 1], used[PDQ_SIDE + 1];
    const int lane = (int)threadIdx.x;
    const int m = (int)blockIdx.x;
    const int G = P.gt_off[m + 1] - P.gt_off[m], D = P.det_off[m + 1] - P.det_off[m];
    const int n = max(G, D);
    const double* q0 = P.quality + P.pair_off[m];
    const double inf = __longlong_as_double(0x7FF0000000000000ll);
    for (int c = lane; c <= n; c += 64) {
        u[c] = 0.0;
        vv[c] = 0.0;
        p[c] = 0;
    }
    __syncthreads();
    for (int i = 1; i <= G; ++i) {
        if (lane == 0) p[0] = i;
        for (int c = lane; c <= n; c += 64) {
            minv[c] = inf;
            used[c] = 0;
        }
        __syncthreads();
        int j0 = 0;
        while (true) {
            if (lane == 0) used[j0] = 1;
            __syncthreads();
            const int i0 = p[j0];
            const double ui0 = u[i0];
            double best = inf;
            int bestj = 0x7FFFFFFF;
            for (int c = 1 + lane; c <= n; c += 64) {          // ascending inside a lane: a tie keeps the lower column
                if (used[c]) continue;
                const double w = c <= D ? q0[(int64_t)(i0 - 1) * D + (c - 1)] : 0.0;
                const double cost = w > 0.0 && w < inf ? -w : 0.0;          // a quality that is not positive and finite counts as 0
                const double cur = (cost - ui0) - vv[c];
                double mv = minv[c];
                if (cur < mv) {
                    mv = cur;
                    minv[c] = cur;
                    way[c] = j0;
                }
                if (mv < best) {
                    best = mv;
                    bestj = c;
                }
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const double ob = __shfl_xor(best, o, 64);
                const int oj = __shfl_xor(bestj, o, 64);
                if (ob < best || (ob == best && oj < bestj)) {
                    best = ob;
                    bestj = oj;
                }
            }
            __syncthreads();
            for (int c = lane; c <= n; c += 64) {
                if (used[c]) {
                    u[p[c]] += best;          // (the rows of the used columns are distinct)
                    vv[c] -= best;
                } else {
                    minv[c] -= best;
                }
            }
            __syncthreads();
            j0 = bestj;
            if (j0 > n || p[j0] == 0) break;          // (j0 > n: no free column, which G <= n rules out)
        }
        if (lane == 0 && j0 <= n) {
            do {
                const int j1 = way[j0];
                p[j0] = p[j1];
                j0 = j1;
            } while (j0 != 0);
        }
        __syncthreads();
    }
    // rows -> columns (way is free now), then the true positives in ground-truth order
    for (int c = lane; c <= n; c += 64) way[c] = 0;
    __syncthreads();
    for (int c = 1 + lane; c <= n; c += 64)
        if (p[c] != 0) way[p[c]] = c;
    __syncthreads();
    if (lane != 0) return;
    double s[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    int tp = 0;
    for (int i = 1; i <= G; ++i) {
        const int det = way[i] - 1;
        const double w = det >= 0 && det < D ? q0[(int64_t)(i - 1) * D + det] : 0.0;
        const bool hit = w > 0.0 && w < inf;
        P.gt_match[P.gt_off[m] + i - 1] = hit ? det : -1;
        if (!hit) continue;
        ++tp;
#pragma unroll
        for (int q = 0; q < 5; ++q) s[q] += q0[(int64_t)q * P.n_pairs + (int64_t)(i - 1) * D + det];
    }
    P.counts[3 * m] = tp;
    P.counts[3 * m + 1] = D - tp;
    P.counts[3 * m + 2] = G - tp;
#pragma unroll
    for (int q = 0; q < 5; ++q) P.image_sums[5 * m + q] = s[q];
}

// the workspace: frames (2 n int32), det_off, gt_off (n + 1 int32 each), then pair_off (n + 1 int64) at a multiple of 8
static inline size_t pdq_pair_off_at(int32_t n_images) { return ((size_t)(4 * (size_t)n_images + 2) * 4 + 7) & ~(size_t)7; }

// the tables every entry takes: counts, monotone offsets, sides and the pair offsets that follow from them
static bool pdq_tables_ok(const int32_t* det_off, const int32_t* gt_off, const int64_t* pair_off, int32_t n_images) {
    if (!det_off || !gt_off || !pair_off || n_images < 0) return false;
    if (det_off[0] != 0 || gt_off[0] != 0 || pair_off[0] != 0) return false;
    for (int32_t m = 0; m < n_images; ++m) {
        const int64_t D = (int64_t)det_off[m + 1] - det_off[m], G = (int64_t)gt_off[m + 1] - gt_off[m];
        if (D < 0 || G < 0 || D > POD_PDQ_MAX_SIDE || G > POD_PDQ_MAX_SIDE) return false;
        if (pair_off[m + 1] - pair_off[m] != D * G) return false;
    }
    return true;
}

static int pdq_upload_tables(void* workspace, const int32_t* frames, const int32_t* det_off, const int32_t* gt_off, const int64_t* pair_off,
                             int32_t n_images, hipStream_t s) {
    char* w = (char*)workspace;
    const size_t n = (size_t)n_images;
    if (frames && hipMemcpyAsync(w, frames, 8 * n, hipMemcpyHostToDevice, s) != hipSuccess) return POD_E_LAUNCH;
    if (hipMemcpyAsync(w + 8 * n, det_off, 4 * (n + 1), hipMemcpyHostToDevice, s) != hipSuccess) return POD_E_LAUNCH;
    if (hipMemcpyAsync(w + 8 * n + 4 * (n + 1), gt_off, 4 * (n + 1), hipMemcpyHostToDevice, s) != hipSuccess) return POD_E_LAUNCH;
    if (hipMemcpyAsync(w + pdq_pair_off_at(n_images), pair_off, 8 * (n + 1), hipMemcpyHostToDevice, s) != hipSuccess) return POD_E_LAUNCH;
    return POD_OK;
}

// Phi^-1(p), 0 < p < 1, by bisection on Phi through erfc: the region of interest is widened by a pixel, so the last bits do not matter
static double pdq_inverse_phi(double p) {
    double lo = -40.0, hi = 40.0;
    for (int it = 0; it < 200; ++it) {
        const double mid = 0.5 * (lo + hi);
        if (0.5 * erfc(-mid * PDQ_INV_SQRT2) < p) lo = mid; else hi = mid;
    }
    return 0.5 * (lo + hi);
}

}  // namespace pod

extern "C" size_t pod_pdq_workspace_bytes(int32_t n_images) {
    if (n_images < 0) return 0;
    return pod::pdq_pair_off_at(n_images) + 8 * ((size_t)n_images + 1);
}

extern "C" int pod_pdq_pairs(const int32_t* frames, const int32_t* det_off, const int32_t* gt_off, const int64_t* pair_off, int32_t n_images,
                             const float* det_means, const float* det_covs, const float* det_probs, int32_t num_classes, const float* gt_boxes,
                             const int32_t* gt_classes, double p_min, void* workspace, double* quality, double* sums, int32_t* det_invalid,
                             pod_stream_t stream) {
    if (!frames || !pod::pdq_tables_ok(det_off, gt_off, pair_off, n_images)) return POD_E_INVALID;
    if (num_classes < 1 || num_classes > POD_MAX_CLASSES || !(p_min > 0.0 && p_min < 1.0)) return POD_E_INVALID;
    for (int32_t m = 0; m < n_images; ++m)
        if (frames[2 * m] < 1 || frames[2 * m + 1] < 1 || frames[2 * m] > POD_PDQ_MAX_FRAME || frames[2 * m + 1] > POD_PDQ_MAX_FRAME) return POD_E_INVALID;
    const int32_t n_det = n_images ? det_off[n_images] : 0, n_gt = n_images ? gt_off[n_images] : 0;
    const int64_t n_pairs = n_images ? pair_off[n_images] : 0;
    if (n_det > 0 && (!det_means || !det_covs || !det_probs)) return POD_E_INVALID;
    if (n_gt > 0 && (!gt_boxes || !gt_classes)) return POD_E_INVALID;
    if (n_pairs > 0 && !quality) return POD_E_INVALID;
    if (n_det > 0 && !workspace) return POD_E_INVALID;
    if (!pod_aligned(8, workspace, quality, sums)) return POD_E_INVALID;
    if (n_det == 0) return POD_OK;          // nothing to evaluate: no pair, no detection to flag
    const hipStream_t s = (hipStream_t)stream;
    const int rc = pod::pdq_upload_tables(workspace, frames, det_off, gt_off, pair_off, n_images, s);
    if (rc != POD_OK) return rc;
    const char* w = (const char*)workspace;
    pod::KPdqPairsParams P;
    P.frames = (const int32_t*)w;
    P.det_off = P.frames + 2 * (size_t)n_images;
    P.gt_off = P.det_off + n_images + 1;
    P.pair_off = (const int64_t*)(w + pod::pdq_pair_off_at(n_images));
    P.means = det_means; P.covs = det_covs; P.probs = det_probs; P.gt_boxes = gt_boxes; P.gt_classes = gt_classes;
    P.quality = quality; P.sums = sums; P.det_invalid = det_invalid;
    P.p_min = p_min; P.z = pod::pdq_inverse_phi(p_min); P.n_pairs = n_pairs; P.n_images = n_images; P.K = num_classes;
    hipLaunchKernelGGL(pod::k_pdq_pairs, dim3((unsigned)n_det), dim3(pod::PDQ_BLOCK), 0, s, P);
    POD_CHECK_LAUNCH();
    return POD_OK;
}

extern "C" int pod_pdq_assign(const int32_t* det_off, const int32_t* gt_off, const int64_t* pair_off, int32_t n_images, const double* quality,
                              void* workspace, int32_t* gt_match, int32_t* counts, double* image_sums, pod_stream_t stream) {
    if (!pod::pdq_tables_ok(det_off, gt_off, pair_off, n_images)) return POD_E_INVALID;
    const int32_t n_gt = n_images ? gt_off[n_images] : 0;
    const int64_t n_pairs = n_images ? pair_off[n_images] : 0;
    if (n_images > 0 && (!workspace || !counts || !image_sums)) return POD_E_INVALID;
    if (n_pairs > 0 && !quality) return POD_E_INVALID;
    if (n_gt > 0 && !gt_match) return POD_E_INVALID;
    if (!pod_aligned(8, workspace, quality, image_sums)) return POD_E_INVALID;
    if (n_images == 0) return POD_OK;
    const hipStream_t s = (hipStream_t)stream;
    const int rc = pod::pdq_upload_tables(workspace, nullptr, det_off, gt_off, pair_off, n_images, s);
    if (rc != POD_OK) return rc;
    const char* w = (const char*)workspace;
    pod::KPdqAssignParams P;
    P.det_off = (const int32_t*)w + 2 * (size_t)n_images;
    P.gt_off = P.det_off + n_images + 1;
    P.pair_off = (const int64_t*)(w + pod::pdq_pair_off_at(n_images));
    P.quality = quality; P.gt_match = gt_match; P.counts = counts; P.image_sums = image_sums; P.n_pairs = n_pairs;
    hipLaunchKernelGGL(pod::k_pdq_assign, dim3((unsigned)n_images), dim3(64), 0, s, P);
    POD_CHECK_LAUNCH();
    return POD_OK;
}
