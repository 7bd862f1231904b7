// Visualisation of probabilistic detections (visualize_predictions.py VP:20-142, ProbabilisticPredictor.visualize_inference PI:113-146,
// ProbabilisticVisualizer PV): boxes and their 2-sigma corner-covariance ellipses drawn over the frame.
//
//   k_vis_layout : one workgroup per instance list (one `overlay_covariance_instances` call).  Draw order = descending box area (PV:66-75,
//                  ties by input index), the two corner ellipses of `cov_ellipse` (PV:148-193, PV:323-354) in fp64, the instance colour
//                  (cm.autumn of the top score's binary entropy, a fixed colour, per-instance colours or the palette), the label anchor /
//                  font size / text colour
//                  (PV:87-122 with detectron2's Visualizer constants).  One record of POD_VIS_INST_WORDS words per instance.
//   k_vis_render : one workgroup of 256 lanes per 16 x 16 canvas tile, one pixel per lane.  The frame is sampled (nearest, or bilinear to
//                  the output size first), then the frame's primitives are streamed in draw order in chunks of 256: every lane builds one
//                  primitive, tests its padded bounding box against the tile, the hits are compacted into LDS in order (ballot + prefix
//                  count), and every lane composites its pixel over them in fp32 registers.  Labels (host-built background boxes and
//                  glyph quads) come after every box and ellipse of the frame, as matplotlib's zorder = 10 puts them.  One uint8 store
//                  per channel at the end.
#include "pod_device.h"

namespace pod {

constexpr int VIS_TILE = 16;
constexpr int VIS_LANES = VIS_TILE * VIS_TILE;
constexpr int VIS_PRIM = 16;                      // floats per primitive in LDS: kind, 7 params, rgb (0..255), alpha, bbox
constexpr double VIS_R2 = 6.180074306244173;      // chi2.ppf(2 Phi(2) - 1, 2) = -2 ln(1 - q) (PV:345-348)

struct VisListArgs {
    PodVisList l[POD_VIS_LAUNCH_LISTS];
    int n;
};
struct VisFrameArgs {
    PodVisFrame f[POD_VIS_LAUNCH_FRAMES];
    int tile_off[POD_VIS_LAUNCH_FRAMES + 1];
    int n;
};

// Python's float `x % 1.0` (sign of the divisor)
__device__ inline double pymod1(double x) {
    double r = fmod(x, 1.0);
    if (r != 0.0 && r < 0.0) r += 1.0;
    return r == 0.0 ? 0.0 : r;
}

// Python's float floor division a // b (b > 0): CPython's float_floor_div
__device__ inline double pyfloordiv(double a, double b) {
    double mod = fmod(a, b);
    double div = (a - mod) / b;
    if (mod != 0.0 && ((b < 0.0) != (mod < 0.0))) div -= 1.0;
    double fl = floor(div);
    if (div - fl > 0.5) fl += 1.0;
    return fl;
}

__device__ inline double hls_v(double m1, double m2, double hue) {   // colorsys._v
    hue = pymod1(hue);
    if (hue < 1.0 / 6.0) return m1 + (m2 - m1) * hue * 6.0;
    if (hue < 0.5) return m2;
    if (hue < 2.0 / 3.0) return m1 + (m2 - m1) * (2.0 / 3.0 - hue) * 6.0;
    return m1;
}

// detectron2 Visualizer._change_color_brightness(c, 0.7) (colorsys HLS, lightness x 1.7 clamped), then draw_text's adjustment
// (channels floored at 0.2, the first largest raised to >= 0.8)
__device__ inline void text_colour(const double c[3], double out[3]) {
    const double r = c[0], g = c[1], b = c[2];
    const double maxc = fmax(fmax(r, g), b), minc = fmin(fmin(r, g), b);
    const double sumc = maxc + minc, rangec = maxc - minc, l = sumc / 2.0;
    double h = 0.0, s = 0.0;
    if (minc != maxc) {
        s = l <= 0.5 ? rangec / sumc : rangec / (2.0 - sumc);
        const double rc = (maxc - r) / rangec, gc = (maxc - g) / rangec, bc = (maxc - b) / rangec;
        if (r == maxc) h = bc - gc;
        else if (g == maxc) h = 2.0 + rc - bc;
        else h = 4.0 + gc - rc;
        h = pymod1(h / 6.0);
    }
    double nl = l + 0.7 * l;
    nl = nl < 0.0 ? 0.0 : nl;
    nl = nl > 1.0 ? 1.0 : nl;
    if (s == 0.0) {
        out[0] = out[1] = out[2] = nl;
    } else {
        const double m2 = nl <= 0.5 ? nl * (1.0 + s) : nl + s - (nl * s);
        const double m1 = 2.0 * nl - m2;
        out[0] = hls_v(m1, m2, h + 1.0 / 3.0);
        out[1] = hls_v(m1, m2, h);
        out[2] = hls_v(m1, m2, h - 1.0 / 3.0);
    }
    int am = 0;
    for (int k = 0; k < 3; ++k) {
        out[k] = fmax(out[k], 0.2);
        if (out[k] > out[am]) am = k;
    }
    out[am] = fmax(0.8, out[am]);
}

// PV:323-354 + PV:150-158: width along the eigenvector of the smaller eigenvalue; int32 truncation, +180 on the rotation; 0 = NaN (skip)
__device__ inline int cov_ellipse(double a, double b, double c, int& w, int& h, int& rot, float& cs, float& sn) {
    const double half_tr = 0.5 * (a + c), d = 0.5 * (a - c);
    const double rad = sqrt(d * d + b * b);
    const double lmax = half_tr + rad;
    double lmin = half_tr - rad;
    const double det = a * c - b * b;
    if (lmax != 0.0 && fabs(lmin) < 0.5 * fabs(lmax)) lmin = det / lmax;      // no cancellation for the small one
    // eigenvector of lmin: (lmin - c, b) or (b, lmin - a), whichever is longer
    double vx = lmin - c, vy = b;
    const double ux = b, uy = lmin - a;
    if (ux * ux + uy * uy > vx * vx + vy * vy) { vx = ux; vy = uy; }
    if (vx == 0.0 && vy == 0.0) { vx = 1.0; vy = 0.0; }
    const double width = 2.0 * sqrt(lmin * VIS_R2), height = 2.0 * sqrt(lmax * VIS_R2);
    const double rotation = atan2(vy, vx) * (180.0 / M_PI);
    if (width != width || height != height || rotation != rotation) return 0;
    w = width < 2147483647.0 ? (int)width : 2147483647;
    h = height < 2147483647.0 ? (int)height : 2147483647;
    rot = (int)rotation + 180;
    const double t = (double)rot * (M_PI / 180.0);
    cs = (float)cos(t);
    sn = (float)sin(t);
    return 1;
}

__global__ void __launch_bounds__(POD_VIS_MAX_INSTANCES) k_vis_layout(VisListArgs args) {
    const PodVisList& L = args.l[blockIdx.x];
    __shared__ float area[POD_VIS_MAX_INSTANCES];
    int n = L.max_n;
    if (L.count != nullptr) n = min(n, max(*L.count, 0));
    const int i = threadIdx.x;
    if (i == 0) *L.n_out = n;
    float x0 = 0.f, y0 = 0.f, x1 = 0.f, y1 = 0.f;
    if (i < n) {
        const float* bx = L.boxes + (int64_t)i * L.box_stride;
        x0 = bx[0]; y0 = bx[1]; x1 = bx[2]; y1 = bx[3];
        area[i] = (x1 - x0) * (y1 - y0);
    }
    __syncthreads();
    if (i >= n) return;
    // np.argsort(-areas) with ties by input index; NaN areas last
    const float ai = area[i];
    int rank = 0;
    for (int j = 0; j < n; ++j) {
        const float aj = area[j];
        const bool before = (ai != ai) ? (aj == aj || j < i) : (aj == aj && (aj > ai || (aj == ai && j < i)));
        rank += before ? 1 : 0;
    }
    float* o = L.out + (int64_t)rank * POD_VIS_INST_WORDS;
    int* oi = reinterpret_cast<int*>(o);
    for (int k = 0; k < POD_VIS_INST_WORDS; ++k) o[k] = 0.f;
    oi[0] = i;
    o[1] = x0; o[2] = y0; o[3] = x1; o[4] = y1;
    double col[3];
    if (L.colour_mode == POD_VIS_COLOUR_ENTROPY) {
        // VP:99-107: scipy.stats.entropy((s, 1 - s), base=2) of the top score, in its float32 steps, then cm.autumn's 256-entry table
        const float* p = L.probs + (int64_t)i * L.prob_stride;
        float s = p[0];
        for (int k = 1; k < L.n_probs; ++k) s = fmaxf(s, p[k]);
        const float t = 1.0f - s, sum = s + t, ps = s / sum, pt = t / sum;
        const float es = ps > 0.f ? (float)(-(double)ps * log((double)ps)) : (ps == 0.f ? 0.f : -INFINITY);
        const float et = pt > 0.f ? (float)(-(double)pt * log((double)pt)) : (pt == 0.f ? 0.f : -INFINITY);
        const float e = (float)((double)(es + et) / log(2.0));
        float x = e * 256.0f;
        x = x == 256.0f ? 255.0f : x;
        x = fminf(fmaxf(x, -1.0f), 256.0f);
        int idx = (int)x;                                   // matplotlib Colormap.__call__: truncation, then over / under
        idx = x < 0.f ? 0 : (idx > 255 ? 255 : idx);        // (autumn's under / over colours are its end entries)
        col[0] = 1.0; col[1] = idx == 255 ? 1.0 : (double)idx * (1.0 / 255.0); col[2] = 0.0;     // the table is np.linspace(0, 1, 256)
    } else if (L.colour_mode == POD_VIS_COLOUR_PALETTE) {
        // fixed palette (a stated deviation: the reference's random_color is not reproducible): golden-ratio hues, HSV s = 0.75, v = 1
        const double hh = pymod1((double)i * 0.6180339887498949) * 6.0;
        const int sec = (int)hh;
        const double f = hh - sec, v = 1.0, pp = v * 0.25, q = v * (1.0 - 0.75 * f), tt = v * (1.0 - 0.75 * (1.0 - f));
        const int k6 = sec % 6;                            // colorsys.hsv_to_rgb's six sectors
        col[0] = (k6 == 0 || k6 == 5) ? v : k6 == 1 ? q : k6 == 4 ? tt : pp;
        col[1] = k6 == 0 ? tt : (k6 == 1 || k6 == 2) ? v : k6 == 3 ? q : pp;
        col[2] = k6 == 2 ? tt : (k6 == 3 || k6 == 4) ? v : k6 == 5 ? q : pp;
    } else if (L.colour_mode == POD_VIS_COLOUR_ARRAY) {
        const float* c = L.colours + (int64_t)i * L.colour_stride;
        col[0] = c[0]; col[1] = c[1]; col[2] = c[2];
    } else {
        col[0] = L.colour[0]; col[1] = L.colour[1]; col[2] = L.colour[2];
    }
    o[5] = (float)col[0]; o[6] = (float)col[1]; o[7] = (float)col[2]; o[8] = L.alpha;
    if (L.cov != nullptr) {
        // PV:70-86 sorts boxes / labels / colours but not covariance_matrices: the k-th drawn box gets covariance k (BY_RANK)
        const float* cv = L.cov + (int64_t)(L.cov_pairing == POD_VIS_COV_OWN ? i : rank) * L.cov_stride;
        for (int e = 0; e < 2; ++e) {
            const int r0 = 2 * e;
            int w = 0, h = 0, rot = 0;
            float cs = 0.f, sn = 0.f;
            // np.linalg.eigh reads the lower triangle
            const int ok = cov_ellipse(cv[r0 * 4 + r0], cv[(r0 + 1) * 4 + r0], cv[(r0 + 1) * 4 + r0 + 1], w, h, rot, cs, sn);
            oi[9 + 4 * e] = ok; oi[10 + 4 * e] = w; oi[11 + 4 * e] = h; oi[12 + 4 * e] = rot;
            o[17 + 2 * e] = cs; o[18 + 2 * e] = sn;
        }
    }
    // PV:99-116 with detectron2's constants (_SMALL_OBJECT_AREA_THRESH = 1000, default font size max(sqrt(H W) // 90, 10 // scale))
    const double H = L.frame_h, W = L.frame_w, sc = L.scale;
    const double sq = sqrt(H * W);
    const double dfs = fmax(pyfloordiv(sq, 90.0), pyfloordiv(10.0, sc));
    float tx = x0, ty = y0;
    const float ia = (y1 - y0) * (x1 - x0);
    if ((double)ia < 1000.0 * sc || (double)(y1 - y0) < 40.0 * sc) {
        if ((double)y1 >= H - 5.0) { tx = x1; ty = y0; }
        else { tx = x0; ty = y1; }
    }
    const double hr = (double)(y1 - y0) / sq;
    double fs = (hr - 0.02) / 0.08 + 1.0;
    fs = fs < 1.2 ? 1.2 : (fs > 2.0 ? 2.0 : fs);
    fs = fs * 0.5 * dfs;
    double tc[3];
    text_colour(col, tc);
    o[21] = tx; o[22] = ty; o[23] = (float)fs;
    o[24] = (float)tc[0]; o[25] = (float)tc[1]; o[26] = (float)tc[2];
    o[27] = area[i];
}

// one primitive of the frame's draw list into LDS words p[0..15]; returns 0 when it draws nothing
__device__ inline int build_prim(const PodVisFrame& F, int g, int n0, int n1, float* p) {
    const float s = F.scale, hw = 0.5f * F.stroke, pad = hw + 1.0f;
    if (g < 3 * (n0 + n1)) {
        const int li = g < 3 * n0 ? 0 : 1;
        const int k = li == 0 ? g : g - 3 * n0;
        const float* r = F.inst[li] + (int64_t)(k / 3) * POD_VIS_INST_WORDS;
        const int* ri = reinterpret_cast<const int*>(r);
        const int part = k % 3;
        p[8] = r[5] * 255.0f; p[9] = r[6] * 255.0f; p[10] = r[7] * 255.0f; p[11] = r[8];
        if (part == 0) {                                   // box outline (detectron2 draw_box)
            p[0] = 1.f;
            p[1] = r[1] * s; p[2] = r[2] * s; p[3] = r[3] * s; p[4] = r[4] * s; p[5] = hw;
            p[12] = fminf(p[1], p[3]) - pad; p[13] = fminf(p[2], p[4]) - pad; p[14] = fmaxf(p[1], p[3]) + pad; p[15] = fmaxf(p[2], p[4]) + pad;
            return 1;
        }
        const int e = part - 1;
        if (ri[9 + 4 * e] == 0) return 0;
        const float cx = (e == 0 ? r[1] : r[3]) * s, cy = (e == 0 ? r[2] : r[4]) * s;
        const float a = fmaxf((float)ri[10 + 4 * e] * 0.5f * s, 0.5f), b = fmaxf((float)ri[11 + 4 * e] * 0.5f * s, 0.5f);
        const float cs = r[17 + 2 * e], sn = r[18 + 2 * e];
        p[0] = 2.f; p[1] = cx; p[2] = cy; p[3] = a; p[4] = b; p[5] = cs; p[6] = sn; p[7] = hw;
        const float ex = sqrtf((a * cs) * (a * cs) + (b * sn) * (b * sn)), ey = sqrtf((a * sn) * (a * sn) + (b * cs) * (b * cs));
        p[12] = cx - ex - pad; p[13] = cy - ey - pad; p[14] = cx + ex + pad; p[15] = cy + ey + pad;
        return 1;
    }
    const float* q = F.labels + (int64_t)(g - 3 * (n0 + n1)) * POD_VIS_PRIM_WORDS;
    for (int k = 0; k < 12; ++k) p[k] = q[k];
    p[5] = q[5] * 255.0f; p[6] = q[6] * 255.0f; p[7] = q[7] * 255.0f;   // (label words: kind, X0, Y0, X1, Y1, r, g, b, alpha, off, w, -)
    const float grow = (int)q[0] == POD_VIS_LABEL_BOX ? 0.5f : 0.f;      // the box's anti-aliased edge reaches half a pixel out
    p[12] = q[1] - grow; p[13] = q[2] - grow; p[14] = q[3] + grow; p[15] = q[4] + grow;
    return 1;
}

__device__ inline float prim_coverage(const float* p, float px, float py, int cx, int cy, const uint8_t* atlas) {
    if (px < p[12] || px > p[14] || py < p[13] || py > p[15]) return 0.f;
    const int kind = (int)p[0];
    if (kind == 1) {
        const float X0 = fminf(p[1], p[3]), X1 = fmaxf(p[1], p[3]), Y0 = fminf(p[2], p[4]), Y1 = fmaxf(p[2], p[4]);
        const float ox = fmaxf(fmaxf(X0 - px, px - X1), 0.f), oy = fmaxf(fmaxf(Y0 - py, py - Y1), 0.f);
        float d;
        if (ox > 0.f || oy > 0.f) d = sqrtf(ox * ox + oy * oy);
        else d = fminf(fminf(px - X0, X1 - px), fminf(py - Y0, Y1 - py));
        return fminf(fmaxf(p[5] + 0.5f - d, 0.f), 1.f);
    }
    if (kind == 2) {
        const float dx = px - p[1], dy = py - p[2];
        const float u = p[5] * dx + p[6] * dy, v = p[5] * dy - p[6] * dx;
        const float ua = u / p[3], vb = v / p[4];
        const float gval = ua * ua + vb * vb - 1.0f;
        const float gu = 2.0f * (ua / p[3]), gv = 2.0f * (vb / p[4]);
        const float nrm = sqrtf(gu * gu + gv * gv);
        if (!(nrm > 0.f)) return 0.f;
        const float d = fabsf(gval) / nrm;
        return fminf(fmaxf(p[7] + 0.5f - d, 0.f), 1.f);
    }
    if (kind == POD_VIS_LABEL_BOX) {
        const float d = fminf(fminf(px - p[1], p[3] - px), fminf(py - p[2], p[4] - py));
        return fminf(fmaxf(d + 0.5f, 0.f), 1.f);
    }
    // glyph: integer quad [X0, X1) x [Y0, Y1) of the atlas, from byte word 9, rows of word 10 bytes
    const int gx = cx - (int)p[1], gy = cy - (int)p[2], gw = (int)p[10];
    if (gx < 0 || gy < 0 || gx >= (int)p[3] - (int)p[1] || gy >= (int)p[4] - (int)p[2] || gx >= gw) return 0.f;
    return (float)atlas[(int64_t)p[9] + (int64_t)gy * gw + gx] * (1.0f / 255.0f);
}

__device__ inline float sample_channel(const PodVisFrame& F, int fx, int fy, int c) {
    const int ch = F.bgr ? 2 - c : c;
    if (!F.bilinear) return (float)F.src[(int64_t)fy * F.sy + (int64_t)fx * F.sx + (int64_t)ch * F.sc];
    // cv2.resize(INTER_LINEAR) restated in fp32 (PI:135), rounded to uint8 as cv2's output is
    const float rx = (float)F.src_w / (float)F.frame_w, ry = (float)F.src_h / (float)F.frame_h;
    const float sx = fmaxf(((float)fx + 0.5f) * rx - 0.5f, 0.f), sy = fmaxf(((float)fy + 0.5f) * ry - 0.5f, 0.f);
    int x0 = (int)sx, y0 = (int)sy;
    x0 = min(x0, F.src_w - 1); y0 = min(y0, F.src_h - 1);
    const int x1 = min(x0 + 1, F.src_w - 1), y1 = min(y0 + 1, F.src_h - 1);
    const float wx = sx - (float)x0, wy = sy - (float)y0;
    auto at = [&](int y, int x) { return (float)F.src[(int64_t)y * F.sy + (int64_t)x * F.sx + (int64_t)ch * F.sc]; };
    const float top = at(y0, x0) * (1.0f - wx) + at(y0, x1) * wx, bot = at(y1, x0) * (1.0f - wx) + at(y1, x1) * wx;
    const float v = top * (1.0f - wy) + bot * wy;
    return fminf(fmaxf(rintf(v), 0.f), 255.f);
}

__global__ void __launch_bounds__(VIS_LANES) k_vis_render(VisFrameArgs args) {
    __shared__ float prim[VIS_LANES * VIS_PRIM];
    __shared__ int wave_cnt[VIS_LANES / POD_WAVE];
    const int tile = blockIdx.x;
    int fi = 0;
    while (fi + 1 < args.n && tile >= args.tile_off[fi + 1]) ++fi;
    const PodVisFrame& F = args.f[fi];
    const int tiles_x = (F.out_w + VIS_TILE - 1) / VIS_TILE;
    const int t = tile - args.tile_off[fi];
    const int tx0 = (t % tiles_x) * VIS_TILE, ty0 = (t / tiles_x) * VIS_TILE;
    const int cx = tx0 + (threadIdx.x % VIS_TILE), cy = ty0 + (threadIdx.x / VIS_TILE);
    const bool inside = cx < F.out_w && cy < F.out_h;
    const float px = (float)cx + 0.5f, py = (float)cy + 0.5f;
    // the tile's extent (pixel centres) for the binning test
    const float bx0 = (float)tx0 + 0.5f, by0 = (float)ty0 + 0.5f, bx1 = (float)(tx0 + VIS_TILE) - 0.5f, by1 = (float)(ty0 + VIS_TILE) - 0.5f;
    float dst[3] = {0.f, 0.f, 0.f};
    if (inside) {
        const int fx = min((int)floorf(px / F.scale), F.frame_w - 1), fy = min((int)floorf(py / F.scale), F.frame_h - 1);
        for (int c = 0; c < 3; ++c) dst[c] = sample_channel(F, fx, fy, c);
    }
    const int n0 = F.inst[0] ? *F.n_inst[0] : 0, n1 = F.inst[1] ? *F.n_inst[1] : 0;
    const int total = 3 * (n0 + n1) + F.n_labels;
    const int lane = threadIdx.x & (POD_WAVE - 1), wid = threadIdx.x / POD_WAVE;
    for (int base = 0; base < total; base += VIS_LANES) {
        const int g = base + threadIdx.x;
        float p[VIS_PRIM];
        int hit = 0;
        if (g < total && build_prim(F, g, n0, n1, p))
            hit = !(p[14] < bx0 || p[12] > bx1 || p[15] < by0 || p[13] > by1);
        const unsigned long long m = __ballot(hit);
        const int before = __popcll(m & ((1ull << lane) - 1ull));
        if (lane == 0) wave_cnt[wid] = __popcll(m);
        __syncthreads();
        int off = 0, n_hit = 0;
        for (int w = 0; w < VIS_LANES / POD_WAVE; ++w) {
            off += w < wid ? wave_cnt[w] : 0;
            n_hit += wave_cnt[w];
        }
        if (hit)
            for (int k = 0; k < VIS_PRIM; ++k) prim[(off + before) * VIS_PRIM + k] = p[k];
        __syncthreads();
        if (inside) {
            for (int h = 0; h < n_hit; ++h) {
                const float* q = prim + h * VIS_PRIM;
                const float cov = prim_coverage(q, px, py, cx, cy, F.atlas);
                if (cov > 0.f) {
                    const int kind = (int)q[0];
                    const float* rgb = kind >= POD_VIS_LABEL_BOX ? q + 5 : q + 8;
                    const float w = (kind >= POD_VIS_LABEL_BOX ? q[8] : q[11]) * cov;
                    for (int c = 0; c < 3; ++c) dst[c] = dst[c] + (rgb[c] - dst[c]) * w;
                }
            }
        }
        __syncthreads();
    }
    if (inside) {
        uint8_t* o = F.dst + ((int64_t)cy * F.out_w + cx) * 3;
        for (int c = 0; c < 3; ++c) o[c] = (uint8_t)fminf(fmaxf(rintf(dst[c]), 0.f), 255.f);
    }
}

}  // namespace pod

extern "C" int pod_vis_layout(const PodVisList* lists, int32_t n_lists, pod_stream_t stream) {
    if (n_lists < 0 || (n_lists > 0 && lists == nullptr)) return POD_E_INVALID;
    for (int i = 0; i < n_lists; ++i) {
        const PodVisList& L = lists[i];
        if (L.max_n < 0 || L.max_n > POD_VIS_MAX_INSTANCES || L.out == nullptr || L.n_out == nullptr || (L.max_n > 0 && L.boxes == nullptr) ||
            L.box_stride < 4 || (L.cov != nullptr && L.cov_stride < 16) || L.frame_h <= 0 || L.frame_w <= 0 || !(L.scale > 0.f))
            return POD_E_INVALID;
        if (L.colour_mode == POD_VIS_COLOUR_ENTROPY && (L.probs == nullptr || L.n_probs < 1 || L.prob_stride < L.n_probs)) return POD_E_INVALID;
        if (L.colour_mode == POD_VIS_COLOUR_ARRAY && (L.colours == nullptr || L.colour_stride < 3)) return POD_E_INVALID;
        if (L.colour_mode < POD_VIS_COLOUR_ENTROPY || L.colour_mode > POD_VIS_COLOUR_ARRAY) return POD_E_INVALID;
        if (L.cov_pairing != POD_VIS_COV_BY_RANK && L.cov_pairing != POD_VIS_COV_OWN) return POD_E_INVALID;
    }
    hipStream_t st = (hipStream_t)stream;
    for (int a = 0; a < n_lists; a += POD_VIS_LAUNCH_LISTS) {
        pod::VisListArgs args;
        args.n = n_lists - a < POD_VIS_LAUNCH_LISTS ? n_lists - a : POD_VIS_LAUNCH_LISTS;
        for (int k = 0; k < args.n; ++k) args.l[k] = lists[a + k];
        hipLaunchKernelGGL(pod::k_vis_layout, dim3(args.n), dim3(POD_VIS_MAX_INSTANCES), 0, st, args);
        POD_CHECK_LAUNCH();
    }
    return POD_OK;
}

extern "C" int pod_vis_render(const PodVisFrame* frames, int32_t n_frames, pod_stream_t stream) {
    if (n_frames < 0 || (n_frames > 0 && frames == nullptr)) return POD_E_INVALID;
    for (int i = 0; i < n_frames; ++i) {
        const PodVisFrame& F = frames[i];
        if (F.src == nullptr || F.dst == nullptr || F.src_h <= 0 || F.src_w <= 0 || F.frame_h <= 0 || F.frame_w <= 0 || F.out_h <= 0 ||
            F.out_w <= 0 || !(F.scale > 0.f) || !(F.stroke >= 0.f) || F.n_labels < 0 || (F.n_labels > 0 && (F.labels == nullptr || F.atlas == nullptr)))
            return POD_E_INVALID;
        if (!F.bilinear && (F.src_h != F.frame_h || F.src_w != F.frame_w)) return POD_E_INVALID;
        for (int k = 0; k < 2; ++k)
            if ((F.inst[k] == nullptr) != (F.n_inst[k] == nullptr)) return POD_E_INVALID;
    }
    hipStream_t st = (hipStream_t)stream;
    for (int a = 0; a < n_frames; a += POD_VIS_LAUNCH_FRAMES) {
        pod::VisFrameArgs args;
        args.n = n_frames - a < POD_VIS_LAUNCH_FRAMES ? n_frames - a : POD_VIS_LAUNCH_FRAMES;
        args.tile_off[0] = 0;
        for (int k = 0; k < args.n; ++k) {
            const PodVisFrame& F = frames[a + k];
            args.f[k] = F;
            args.tile_off[k + 1] = args.tile_off[k] + ((F.out_w + pod::VIS_TILE - 1) / pod::VIS_TILE) * ((F.out_h + pod::VIS_TILE - 1) / pod::VIS_TILE);
        }
        for (int k = args.n; k < POD_VIS_LAUNCH_FRAMES; ++k) args.tile_off[k + 1] = args.tile_off[args.n];
        hipLaunchKernelGGL(pod::k_vis_render, dim3(args.tile_off[args.n]), dim3(pod::VIS_LANES), 0, st, args);
        POD_CHECK_LAUNCH();
    }
    return POD_OK;
}
