// K30: what training the whole ResNet (MODEL.BACKBONE.FREEZE_AT 0 and 1) needs below res2 (include/pod_mi355x.h).
//
// Replaces (reference: detectron2's BasicStem as probabilistic_retinanet.py:96-100 runs it in train mode, `features = self.backbone(images.tensor)`,
// under train_net.py's loop): autograd's backward of conv1 + FrozenBN + ReLU + max_pool2d(3, 2, 1).
//
// pod_stem7x7_wgrad: the gradient of the folded 7x7 / stride 2 / pad 3 filter,
//     dW[k][c][dy][dx] = sum over (b, oy, ox) of dS[b, oy, ox, k] xn[b, c, 2 oy - 3 + dy, 2 ox - 3 + dx],
// xn the frame normalised on load exactly as k14's patch load normalises it and zero outside Hi x Wi.  K22's arithmetic: both operands
// split at run time into two f16 terms of their power-of-two-scaled values (dS's record is its producer's, x's the word that bounds the
// normalised input: the forward's in_amax), three partial products on v_mfma_f32_32x32x16_f16, fp32 accumulation inside a slice, the slices'
// partial sums added in slice order in fp64 by a second launch.  A slice is a run of 8 x 8 output tiles of the batch (tile order: image, tile
// row, tile column); its length is a function of the tile count alone.  A workgroup (four wavefronts) owns one slice: per tile it stages the
// 22 x 24 x 3 input patch (k14's) and the 64 pixels x 64 channels of dS in LDS once and multiplies dS^T (64 channels x 64 pixels) against
// the patch's 192 windows -- tap t = (c 8 + dy) 8 + dx, the 7 x 7 window padded to 8 x 8; a lane's 8 k values are the 8 pixels of one tile
// row, two floats apart in the patch.  Wavefront (kb, cw) holds channels 32 kb .. + 31 against taps 96 cw .. + 95.  The padded taps (dy = 7
// or dx = 7) read inside the patch and are dropped by the second launch.  No atomics: the same bits on every run.
//
// pod_maxpool3x3s2_backward_cl: the max-pool's backward and the stem's ReLU gate in one pass over one image,
//     dS[y, x, c] = (s[y, x, c] > 0) * sum of dP[oy, ox, c] over the windows (oy, ox) whose arg-max is (y, x),
// a gather per input pixel over the at most four windows that hold it, in window order (oy ascending, then ox).  The arg-max is torch's:
// the window's in-bounds pixels scanned row-major, a new maximum only on strict >, so the first maximum wins -- (y, x) is the arg-max of a
// window iff every pixel before it is smaller and none after it is larger.  One thread per 16 bytes of dS, its abs-max record published by
// the same pass (pod_wgrad.h: map_quad_pass).
#include "pod_wgrad.h"

namespace pod {

constexpr int SW_PR = 22, SW_PC = 24;             // k14's patch: rows 2 * 7 + 7 + 1, columns 2 * 7 + 8 padded to 24
constexpr int SW_PATCH = 3 * SW_PR * SW_PC;       // 1584 floats
constexpr int SW_PATCH_IT = (SW_PATCH + 255) / 256;
constexpr int SW_TAPS = 192;                      // 3 channels x 8 x 8
constexpr int SW_DS = 64 + 4;                     // LDS row stride of the dS tile, floats (16-byte rows)
constexpr int SW_MAX_SLICES = 512;

// Host and device agree on the slices through this function of the tile count alone.
static inline int sw_run_tiles(int64_t tiles) {
    int r = 16;
    while (r < 4096 && (tiles + r - 1) / r > SW_MAX_SLICES) r <<= 1;
    return r;
}

struct StemWgradParams {
    const void* x;            // (images, 3, Hi, Wi): fp32, or uint8 (x_u8)
    const float* mean;        // (x - mean[c]) / std[c] on load, as k_stem7x7_split; null: x is already normalised
    const float* std_;
    const float* dS;          // (images * Ho * Wo, 64) channels-last
    const float* x_amax;      // record >= max |normalised input|
    const float* ds_amax;
    float* partials;          // [slice][k 64][tap 192]
    int32_t Hi, Wi, x_u8, Ho, Wo, tiles_x, tiles_img, run;
    int64_t tiles;
};

__global__ void __launch_bounds__(256, 2) k_stem7x7_wgrad(const StemWgradParams P) {
    __shared__ __attribute__((aligned(16))) float patch[SW_PATCH];
    __shared__ __attribute__((aligned(16))) float ds[64 * SW_DS];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int i32 = lane & 31, h = lane >> 5, kb = wave & 1, cw = wave >> 1;
    const int slice = blockIdx.x;
    const float sx = sg_activation_scale(P.x_amax), sd = sg_activation_scale(P.ds_amax);
    const int64_t g_begin = (int64_t)slice * P.run;
    const int64_t g_end = g_begin + P.run < P.tiles ? g_begin + P.run : P.tiles;
    const int dq = t & 15, dp = t >> 4;               // dS staging: quad, tile pixel (+ 16 j)

    const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
    float preg[SW_PATCH_IT];
    f32x4 dreg[4];
    int oy0 = 0;
    auto origin = [&](int64_t g, int& b, int& ty, int& tx) {
        b = (int)(g / P.tiles_img);
        const int r = (int)(g - (int64_t)b * P.tiles_img);
        ty = r / P.tiles_x;
        tx = r - ty * P.tiles_x;
    };
    auto load = [&](int64_t g) {                      // tile g's patch and dS rows -> registers, zeros outside the frame / the map
        int b, ty, tx;
        origin(g, b, ty, tx);
        const int iy0 = 16 * ty - 3, ix0 = 16 * tx - 3;
#pragma unroll
        for (int it = 0; it < SW_PATCH_IT; ++it) {
            const int e = t + 256 * it;
            const int c = e / (SW_PR * SW_PC), r = (e - c * SW_PR * SW_PC) / SW_PC, col = e - c * SW_PR * SW_PC - r * SW_PC;
            const int iy = iy0 + r, ix = ix0 + col;
            float v = 0.f;
            if (e < SW_PATCH && iy >= 0 && iy < P.Hi && ix >= 0 && ix < P.Wi) {
                const int64_t at = (((int64_t)b * 3 + c) * P.Hi + iy) * P.Wi + ix;
                v = P.x_u8 ? (float)static_cast<const uint8_t*>(P.x)[at] : static_cast<const float*>(P.x)[at];
                if (P.mean) v = (v - P.mean[c]) / P.std_[c];
            }
            preg[it] = v;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int pix = dp + 16 * j, oy = 8 * ty + (pix >> 3), ox = 8 * tx + (pix & 7);
            dreg[j] = (oy < P.Ho && ox < P.Wo) ? *reinterpret_cast<const f32x4*>(P.dS + (((int64_t)b * P.Ho + oy) * P.Wo + ox) * 64 + 4 * dq) : zero4;
        }
    };

    // this lane's window in the patch for each of its three tap blocks: tap (c 8 + dy) 8 + dx starts at patch[c][dy][dx]
    int woff[3];
#pragma unroll
    for (int cb = 0; cb < 3; ++cb) {
        const int tap = 96 * cw + 32 * cb + i32;
        woff[cb] = (tap >> 6) * (SW_PR * SW_PC) + ((tap >> 3) & 7) * SW_PC + (tap & 7);
    }
    const f32x16 zero16 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    f32x16 acc[3] = {zero16, zero16, zero16};

    if (g_begin < g_end) load(g_begin);
    for (int64_t g = g_begin; g < g_end; ++g) {
        {
            int b, ty, tx;
            origin(g, b, ty, tx);
            oy0 = 8 * ty;
        }
#pragma unroll
        for (int it = 0; it < SW_PATCH_IT; ++it)
            if (t + 256 * it < SW_PATCH) patch[t + 256 * it] = preg[it];
#pragma unroll
        for (int j = 0; j < 4; ++j) *reinterpret_cast<f32x4*>(ds + (dp + 16 * j) * SW_DS + 4 * dq) = dreg[j];
        __syncthreads();
        if (g + 1 < g_end) load(g + 1);                      // (uniform) in flight behind the products below
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            if (oy0 + 2 * s >= P.Ho) break;                  // (uniform) tile rows below the map: zeros
            const int r = 2 * s + h;                         // the lane's tile row: its 8 k values are the row's 8 pixels
            sg_u32x4 dyf[2];
            {
                const float* p = ds + (8 * r) * SW_DS + 32 * kb + i32;
#pragma unroll
                for (int m = 0; m < 4; ++m) {
                    uint32_t w[2];
                    wino_f16_split2(p[(2 * m) * SW_DS], p[(2 * m + 1) * SW_DS], sd, w);
                    dyf[0][m] = w[0];
                    dyf[1][m] = w[1];
                }
            }
#pragma unroll
            for (int cb = 0; cb < 3; ++cb) {
                sg_u32x4 xf[2];
                const float* p = patch + woff[cb] + (2 * r) * SW_PC;
#pragma unroll
                for (int m = 0; m < 4; ++m) {
                    uint32_t w[2];
                    wino_f16_split2(p[4 * m], p[4 * m + 2], sx, w);
                    xf[0][m] = w[0];
                    xf[1][m] = w[1];
                }
                // small products first (as k12 / k13 / k22)
                f32x16 a = acc[cb];
                a = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(wino_f16x8, dyf[0]), __builtin_bit_cast(wino_f16x8, xf[1]), a, 0, 0, 0);
                a = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(wino_f16x8, dyf[1]), __builtin_bit_cast(wino_f16x8, xf[0]), a, 0, 0, 0);
                a = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(wino_f16x8, dyf[0]), __builtin_bit_cast(wino_f16x8, xf[0]), a, 0, 0, 0);
                acc[cb] = a;
            }
        }
        __syncthreads();
    }

    // partial sums [slice][k 64][tap 192]: accumulator register j of a lane is row (j & 3) + 8 (j >> 2) + 4 h, column i32
    const float inv = wino_pow2_inverse(sx) * wino_pow2_inverse(sd);
#pragma unroll
    for (int cb = 0; cb < 3; ++cb) {
        const int tap = 96 * cw + 32 * cb + i32;
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int k = 32 * kb + (j & 3) + 8 * (j >> 2) + 4 * h;
            P.partials[((int64_t)slice * 64 + k) * SW_TAPS + tap] = acc[cb][j] * inv;
        }
    }
}

// the slices' partials [slice][k 64][tap 192] in slice order -> dW (64, 3, 7, 7); the padded taps are dropped (k_wgrad_reduce's sibling)
__global__ void __launch_bounds__(256) k_stem7x7_wgrad_reduce(const float* __restrict__ partials, const int n_slices, float* __restrict__ dW) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= 64 * 147) return;
    const int k = i / 147, r = i - k * 147, c = r / 49, dy = (r - c * 49) / 7, dx = r - c * 49 - dy * 7;
    double a = 0.0;
    for (int s = 0; s < n_slices; ++s) a += (double)partials[((int64_t)s * 64 + k) * SW_TAPS + (c * 8 + dy) * 8 + dx];
    dW[i] = (float)a;
}

__global__ void __launch_bounds__(256) k_maxpool3x3s2_backward_cl(const float* __restrict__ s, const float* __restrict__ dP, float* __restrict__ dS, const int H,
                                                                  const int W, const int Hq, const int Wq, const int C4, float* __restrict__ amax) {
    map_quad_pass(dS, H, W, C4, amax, [&](const int64_t i, const int c4, const int x, const int y) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(s + i * 4);
        f32x4 sum = f32x4{0.f, 0.f, 0.f, 0.f};
        // the windows that hold (y, x): rows 2 oy - 1 .. 2 oy + 1 -- one window along an even coordinate, two along an odd one
        const int oy_lo = y >> 1, oy_hi = (y + 1) >> 1, ox_lo = x >> 1, ox_hi = (x + 1) >> 1;
        for (int oy = oy_lo; oy <= oy_hi && oy < Hq; ++oy)
            for (int ox = ox_lo; ox <= ox_hi && ox < Wq; ++ox) {
                bool w0 = true, w1 = true, w2 = true, w3 = true;
#pragma unroll
                for (int dy = -1; dy <= 1; ++dy) {
                    const int iy = 2 * oy + dy;
                    if (iy < 0 || iy >= H) continue;
#pragma unroll
                    for (int dx = -1; dx <= 1; ++dx) {
                        const int ix = 2 * ox + dx;
                        if (ix < 0 || ix >= W || (iy == y && ix == x)) continue;
                        const f32x4 u = *reinterpret_cast<const f32x4*>(s + (((int64_t)iy * W + ix) * C4 + c4) * 4);
                        if (iy < y || (iy == y && ix < x)) {         // scanned before (y, x): it keeps the maximum unless (y, x) is larger
                            w0 = w0 && u.x < v.x; w1 = w1 && u.y < v.y; w2 = w2 && u.z < v.z; w3 = w3 && u.w < v.w;
                        } else {                                     // scanned after: it takes the maximum only if larger
                            w0 = w0 && u.x <= v.x; w1 = w1 && u.y <= v.y; w2 = w2 && u.z <= v.z; w3 = w3 && u.w <= v.w;
                        }
                    }
                }
                const f32x4 d = *reinterpret_cast<const f32x4*>(dP + (((int64_t)oy * Wq + ox) * C4 + c4) * 4);
                if (w0) sum.x += d.x;
                if (w1) sum.y += d.y;
                if (w2) sum.z += d.z;
                if (w3) sum.w += d.w;
            }
        return gate4(sum, v);
    });
}

// Host: the tile count of a stem weight gradient, 0 = outside what pod_stem7x7_split accepts or the kernel addresses
static int64_t sw_tiles(int32_t images, int32_t H_img, int32_t W_img, int32_t H, int32_t W) {
    if (images < 1 || H < 1 || W < 1 || H > 16384 || W > 16384 || H_img < 1 || W_img < 1 || H_img > H || W_img > W) return 0;
    const int64_t Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
    if ((int64_t)images * Ho * Wo > 0x3FFFFFFF) return 0;
    return (int64_t)images * ((Ho + 7) / 8) * ((Wo + 7) / 8);
}

}  // namespace pod

extern "C" int64_t pod_stem7x7_wgrad_partials(int32_t images, int32_t H_img, int32_t W_img, int32_t H, int32_t W) {
    const int64_t tiles = pod::sw_tiles(images, H_img, W_img, H, W);
    if (tiles < 1) return 0;
    const int run = pod::sw_run_tiles(tiles);
    return ((tiles + run - 1) / run) * 64 * pod::SW_TAPS;
}

extern "C" int pod_stem7x7_wgrad(const void* x, int32_t x_is_u8, int32_t images, int32_t H_img, int32_t W_img, const float* mean, const float* stddev, const float* dS,
                                 int32_t H, int32_t W, const float* x_amax, const float* ds_amax, float* dW, float* partials, pod_stream_t stream) {
    const int64_t tiles = pod::sw_tiles(images, H_img, W_img, H, W);
    if (tiles < 1) return POD_E_INVALID;
    if (!x || !dS || !x_amax || !ds_amax || !dW || !partials || (mean == nullptr) != (stddev == nullptr)) return POD_E_INVALID;
    if (!pod_aligned(16, dS, partials) || !pod_aligned(4, x_amax, ds_amax, dW, mean, stddev) || (!x_is_u8 && !pod_aligned(4, x))) return POD_E_INVALID;
    if (dW == dS || dW == partials || dS == partials || x == static_cast<const void*>(dW) || x == static_cast<const void*>(partials) || x == static_cast<const void*>(dS))
        return POD_E_INVALID;
    pod::StemWgradParams P;
    P.x = x; P.x_u8 = x_is_u8 ? 1 : 0; P.Hi = H_img; P.Wi = W_img; P.mean = mean; P.std_ = stddev; P.dS = dS; P.x_amax = x_amax; P.ds_amax = ds_amax;
    P.partials = partials;
    P.Ho = (H - 1) / 2 + 1; P.Wo = (W - 1) / 2 + 1;
    P.tiles_x = (P.Wo + 7) / 8; P.tiles_img = P.tiles_x * ((P.Ho + 7) / 8); P.tiles = tiles; P.run = pod::sw_run_tiles(tiles);
    const int64_t n_slices = (tiles + P.run - 1) / P.run;
    if (n_slices > 0x7FFFFFFF) return POD_E_INVALID;
    hipLaunchKernelGGL(pod::k_stem7x7_wgrad, dim3((unsigned)n_slices), dim3(256), 0, (hipStream_t)stream, P);
    POD_CHECK_LAUNCH();
    hipLaunchKernelGGL(pod::k_stem7x7_wgrad_reduce, dim3((64 * 147 + 255) / 256), dim3(256), 0, (hipStream_t)stream, partials, (int)n_slices, dW);
    POD_CHECK_LAUNCH();
    return POD_OK;
}

extern "C" int pod_maxpool3x3s2_backward_cl(const float* s, const float* dP, float* dS, int32_t H, int32_t W, int32_t C, float* ds_amax, pod_stream_t stream) {
    if (!s || dP == s) return POD_E_INVALID;
    const int32_t Hq = (int32_t)(((int64_t)H - 1) / 2 + 1), Wq = (int32_t)(((int64_t)W - 1) / 2 + 1);      // (H, W are checked below)
    return pod::map_gather(dP, s, nullptr, dS, H, W, C, ds_amax, (int64_t)H * W, [&](dim3 grid) {
        hipLaunchKernelGGL(pod::k_maxpool3x3s2_backward_cl, grid, dim3(256), 0, (hipStream_t)stream, s, dP, dS, H, W, Hq, Wq, C / 4, ds_amax);
    });
}
