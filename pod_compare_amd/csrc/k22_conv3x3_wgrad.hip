// K22: the backward pass of the head's 3x3 / stride-1 / pad-1 convolutions that is not itself a forward convolution (include/pod_mi355x.h).
//
// pod_conv3x3_wgrad: dW[k][c][ky][kx] = sum over images and pixels of dY[(y, x)][k] X[(y + ky - 1, x + kx - 1)][c], db[k] = sum dY[.][k].
// A GEMM with M = K, N = 9 C and the PIXELS as the reduction, on v_mfma_f32_32x32x16_f16 with pod_split_gemm.h's products: both operands
// are split at run time into two f16 terms of their power-of-two-scaled values (scales from their abs-max records), three partial
// products, fp32 accumulate.
//
// The reduction unit is a STEP: one image row r of one 16-pixel column strip.  The MFMA wants a lane to hold 8 consecutive reduction
// values (pixels) of one channel, channels-last memory has consecutive channels of one pixel: a step's operands go through LDS,
// transposed, [channel 64][WG_LS = 18 floats].  18 = the 16 pixels + the halo of X; as a row stride it makes the fragment reads
// (ds_read_b64 at channel * 18 + 8 h + 2 m) conflict-free: channel * 18 mod 64 takes 32 distinct even values for 32 channels.
// A lane reads the 10 X values at pixels 8 h - 1 .. 8 h + 8 of its channel ONCE and forms the three kx windows from them (9 pair splits
// instead of 12: kx = 0 and kx = 2 share their pairs); the X row r serves the three ky taps against the dY rows r + 1, r, r - 1, whose
// split fragments stay in registers from one step to the next (a strip is walked top to bottom), so a step stages ONE row of each
// operand.  A workgroup of four wavefronts owns 64 k x 64 c: wave (kb, cb) keeps nine 32 x 32 accumulator blocks, one per tap.
//
// Parallelism and determinism: the steps of a launch are enumerated by the geometry alone -- level, image, strip, row -- and cut into
// SLICES of WG_STEPS consecutive steps; grid = slices x k tiles x c tiles.  A slice owns its X rows (all three taps of them), writes its
// partial sums, and a second launch adds the slices' partials in slice order, in fp64.  No atomics: two launches give the same bits.
// db: fp64 partial column sums over chunks of 4096 pixels (a launch of its own), added by the same second launch.  Both of them, the
// partial buffer's layout, the argument checks and the launch sequence are pod_wgrad.h's (wgrad_launch), shared with K23 and K24.
//
// pod_relu_dropout_backward: the gate of a trunk layer.  The layer's stored output is relu(z) keep / (1 - p) (pod_wino.h's store pass:
// scale = 1.0f / (1.0f - p), exact zeros where dropped), so it is its own mask: dZ = dOut (out > 0) / (1 - p) (pod_wgrad.h: quad_pass, gate4).
#include "pod_wgrad.h"

namespace pod {

constexpr int WG_STEPS = 256;      // steps (16-pixel row segments) of one slice: a function of nothing
constexpr int WG_LS = 18;          // LDS row stride, floats

struct WgradGeom {
    int32_t n_levels, copies, total_steps, reserved;
    int32_t H[POD_MAX_LEVELS], W[POD_MAX_LEVELS], strips[POD_MAX_LEVELS];
    int32_t first_step[POD_MAX_LEVELS + 1];      // [n_levels]: the total
    int64_t first_pixel[POD_MAX_LEVELS];
};

__global__ void __launch_bounds__(256, 2) k_conv3x3_wgrad(const float* __restrict__ X, const float* __restrict__ dY, const WgradGeom G, const int C, const int K,
                                                       const int Kpad, const float* __restrict__ x_amax, const float* __restrict__ dy_amax,
                                                       float* __restrict__ partials) {
    __shared__ __attribute__((aligned(16))) float xs[64 * WG_LS];
    __shared__ __attribute__((aligned(16))) float ds[64 * WG_LS];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int i32 = lane & 31, h = lane >> 5, kb = wave & 1, cb = wave >> 1;
    const int pi = t & 15, q4 = t >> 4;                 // staging: pixel of the segment, channel quad of the tile
    const int slice = blockIdx.x, k0 = blockIdx.y * 64, c0 = blockIdx.z * 64;
    const float sx = sg_activation_scale(x_amax), sd = sg_activation_scale(dy_amax);
    const int total = G.total_steps;

    const f32x16 zero16 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    f32x16 acc[3][3];
#pragma unroll
    for (int ky = 0; ky < 3; ++ky)
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) acc[ky][kx] = zero16;
    sg_u32x4 dyf[3][2] = {};          // [dY row r - 1, r, r + 1][term]

    for (int it = 0; it < WG_STEPS; ++it) {
        const int s = slice * WG_STEPS + it;
        if (s >= total) break;        // (uniform)
        // the step: level, image, strip, row -- scalar arithmetic on the geometry
        int H = G.H[0], W = G.W[0], strips = G.strips[0], first = 0;
        int64_t pix0 = G.first_pixel[0];
#pragma unroll
        for (int j = 1; j < POD_MAX_LEVELS; ++j)
            if (j < G.n_levels && s >= G.first_step[j]) {
                H = G.H[j]; W = G.W[j]; strips = G.strips[j]; first = G.first_step[j]; pix0 = G.first_pixel[j];
            }
        const int local = s - first, per_img = strips * H;
        const int img = local / per_img, rem = local - img * per_img;
        const int strip = rem / H, r = rem - strip * H;
        const int x0 = strip * 16;
        const int64_t img_pix = pix0 + (int64_t)img * H * W;
        const bool fresh = it == 0 || r == 0;

        auto stage_dy = [&](int row) {          // dY row `row`, pixels x0 .. x0 + 15, channels k0 .. k0 + 63 -> ds[k][pixel]
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            const int x = x0 + pi, k = k0 + 4 * q4;
            if (row >= 0 && row < H && x < W) {
                v = *reinterpret_cast<const f32x4*>(dY + (img_pix + (int64_t)row * W + x) * Kpad + k);
                if (k + 0 >= K) v.x = 0.f;      // a predictor's padded channels contribute nothing
                if (k + 1 >= K) v.y = 0.f;
                if (k + 2 >= K) v.z = 0.f;
                if (k + 3 >= K) v.w = 0.f;
            }
            ds[(4 * q4 + 0) * WG_LS + pi] = v.x;
            ds[(4 * q4 + 1) * WG_LS + pi] = v.y;
            ds[(4 * q4 + 2) * WG_LS + pi] = v.z;
            ds[(4 * q4 + 3) * WG_LS + pi] = v.w;
        };
        auto stage_x1 = [&](int i, int cq) {    // X row r, pixel x0 - 1 + i, channels c0 + 4 cq .. + 3 -> xs[c][i]
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            const int x = x0 - 1 + i, c = c0 + 4 * cq;
            if (x >= 0 && x < W && c < C) v = *reinterpret_cast<const f32x4*>(X + (img_pix + (int64_t)r * W + x) * C + c);
            xs[(4 * cq + 0) * WG_LS + i] = v.x;
            xs[(4 * cq + 1) * WG_LS + i] = v.y;
            xs[(4 * cq + 2) * WG_LS + i] = v.z;
            xs[(4 * cq + 3) * WG_LS + i] = v.w;
        };
        auto read_dy = [&](sg_u32x4 (&f)[2]) {  // the lane's 8 pixels of channel 32 kb + i32, split
            const float* p = ds + (32 * kb + i32) * WG_LS + 8 * h;
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                const f32x2 v = *reinterpret_cast<const f32x2*>(p + 2 * m);
                uint32_t w[2];
                wino_f16_split2(v.x, v.y, sd, w);
                f[0][m] = w[0];
                f[1][m] = w[1];
            }
        };

        if (fresh) {                            // the first step of a slice or of a strip: the two rows a running strip carries along
            stage_dy(r - 1);
            __syncthreads();
            read_dy(dyf[0]);
            __syncthreads();
            stage_dy(r);
            __syncthreads();
            read_dy(dyf[1]);
            __syncthreads();
        } else {
#pragma unroll
            for (int tm = 0; tm < 2; ++tm) {
                dyf[0][tm] = dyf[1][tm];
                dyf[1][tm] = dyf[2][tm];
            }
        }
        stage_dy(r + 1);
        stage_x1(pi, q4);
        if (t < 32) stage_x1(16 + (t & 1), t >> 1);
        __syncthreads();
        read_dy(dyf[2]);
        sg_u32x4 xf[3][2];                      // [kx][term]
        {
            const float* p = xs + (32 * cb + i32) * WG_LS + 8 * h;
            float v[10];
#pragma unroll
            for (int m = 0; m < 5; ++m) {
                const f32x2 u = *reinterpret_cast<const f32x2*>(p + 2 * m);
                v[2 * m] = u.x;
                v[2 * m + 1] = u.y;
            }
            uint32_t e[5][2], o[4][2];
#pragma unroll
            for (int m = 0; m < 5; ++m) wino_f16_split2(v[2 * m], v[2 * m + 1], sx, e[m]);
#pragma unroll
            for (int m = 0; m < 4; ++m) wino_f16_split2(v[2 * m + 1], v[2 * m + 2], sx, o[m]);
#pragma unroll
            for (int tm = 0; tm < 2; ++tm)
#pragma unroll
                for (int m = 0; m < 4; ++m) {
                    xf[0][tm][m] = e[m][tm];
                    xf[1][tm][m] = o[m][tm];
                    xf[2][tm][m] = e[m + 1][tm];
                }
        }
        __syncthreads();
        // tap (ky, kx): dY row r + 1 - ky against the window of X row r shifted by kx; small products first (as k12 / k13)
#pragma unroll
        for (int ky = 0; ky < 3; ++ky)
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
                f32x16 a = acc[ky][kx];
                a = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(wino_f16x8, dyf[2 - ky][0]), __builtin_bit_cast(wino_f16x8, xf[kx][1]), a, 0, 0, 0);
                a = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(wino_f16x8, dyf[2 - ky][1]), __builtin_bit_cast(wino_f16x8, xf[kx][0]), a, 0, 0, 0);
                a = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(wino_f16x8, dyf[2 - ky][0]), __builtin_bit_cast(wino_f16x8, xf[kx][0]), a, 0, 0, 0);
                acc[ky][kx] = a;
            }
    }

    // partial sums [slice][tap][k < Kpad][c < C]: accumulator register j of a lane is row (j & 3) + 8 (j >> 2) + 4 h, column i32
    const float inv = wino_pow2_inverse(sx) * wino_pow2_inverse(sd);
    const int c = c0 + 32 * cb + i32;
    if (c < C) {
#pragma unroll
        for (int ky = 0; ky < 3; ++ky)
#pragma unroll
            for (int kx = 0; kx < 3; ++kx)
#pragma unroll
                for (int j = 0; j < 16; ++j) {
                    const int k = k0 + 32 * kb + (j & 3) + 8 * (j >> 2) + 4 * h;
                    partials[(((int64_t)slice * 9 + ky * 3 + kx) * Kpad + k) * C + c] = acc[ky][kx][j] * inv;
                }
    }
}

__global__ void __launch_bounds__(256) k_relu_dropout_backward(const float* __restrict__ out, const float* d_out, float* d_z, const int64_t n4, const float scale,
                                                               float* __restrict__ amax) {
    quad_pass(d_z, n4, amax, [&](const int64_t i) { return gate4(reinterpret_cast<const f32x4*>(d_out)[i], reinterpret_cast<const f32x4*>(out)[i], scale); });
}

// Host: the geometry of a launch.  false: outside what the kernel addresses.
static bool wgrad_geometry(const int32_t* level_hw, int32_t n_levels, int32_t copies, int32_t C, int32_t K, int32_t Kpad, WgradGeom& G, int64_t& pixels) {
    if (!level_hw || n_levels < 1 || n_levels > POD_MAX_LEVELS || copies < 1 || copies > 4096) return false;
    if (C < 16 || (C & 15) != 0 || C > 4096 || K < 1 || K > Kpad || (Kpad & 63) != 0 || Kpad > 512) return false;
    G = WgradGeom{};
    G.n_levels = n_levels;
    G.copies = copies;
    int64_t steps = 0;
    pixels = 0;
    for (int l = 0; l < n_levels; ++l) {
        const int32_t H = level_hw[2 * l], W = level_hw[2 * l + 1];
        if (H < 1 || H > 4095 || W < 1 || W > 4095) return false;
        G.H[l] = H;
        G.W[l] = W;
        G.strips[l] = (W + 15) / 16;
        G.first_step[l] = (int32_t)steps;
        G.first_pixel[l] = pixels;
        steps += (int64_t)copies * G.strips[l] * H;
        pixels += (int64_t)copies * H * W;
        if (steps > 0x3FFFFFFF) return false;
    }
    G.first_step[n_levels] = G.total_steps = (int32_t)steps;
    return true;
}

static WgradLayout wgrad3x3_layout(const WgradGeom& G, int64_t pixels, int32_t C, int32_t Kpad) {
    return wgrad_layout(pixels, (G.total_steps + WG_STEPS - 1) / WG_STEPS, Kpad, 9, C);
}

}  // namespace pod

extern "C" int64_t pod_conv3x3_wgrad_partials(const int32_t* level_hw, int32_t n_levels, int32_t copies, int32_t C, int32_t K, int32_t Kpad) {
    pod::WgradGeom G;
    int64_t pixels;
    if (!pod::wgrad_geometry(level_hw, n_levels, copies, C, K, Kpad, G, pixels)) return 0;
    return pod::wgrad3x3_layout(G, pixels, C, Kpad).floats;
}

extern "C" int pod_conv3x3_wgrad(const float* x, const float* dy, const int32_t* level_hw, int32_t n_levels, int32_t copies, int32_t C, int32_t K,
                                 int32_t Kpad, const float* x_amax, const float* dy_amax, float* dW, float* db, float* partials, pod_stream_t stream) {
    pod::WgradGeom G;
    int64_t pixels;
    if (!db || !pod::wgrad_geometry(level_hw, n_levels, copies, C, K, Kpad, G, pixels)) return POD_E_INVALID;
    const pod::WgradLayout L = pod::wgrad3x3_layout(G, pixels, C, Kpad);
    hipStream_t s = (hipStream_t)stream;
    return pod::wgrad_launch<9>(x, dy, pixels, C, K, Kpad, x_amax, dy_amax, L, partials, dW, db, s, [&](float* wp) {
        hipLaunchKernelGGL(pod::k_conv3x3_wgrad, dim3((unsigned)L.n_slices, (unsigned)(Kpad / 64), (unsigned)((C + 63) / 64)), dim3(256), 0, s, x, dy, G, C, K, Kpad, x_amax,
                           dy_amax, wp);
    });
}

extern "C" int pod_relu_dropout_backward(const float* out, const float* d_out, float* d_z, int64_t n, float p, float* dz_amax, pod_stream_t stream) {
    if (!out || !d_out || !d_z || n < 0 || (n & 3) != 0 || !(p >= 0.0f && p < 1.0f)) return POD_E_INVALID;
    if (!pod_aligned(16, out, d_out, d_z)) return POD_E_INVALID;
    if (n == 0) return POD_OK;
    const int64_t n4 = n / 4;
    hipLaunchKernelGGL(pod::k_relu_dropout_backward, dim3(pod_grid_stride_blocks(n4, 4096)), dim3(256), 0, (hipStream_t)stream, out, d_out, d_z, n4, 1.0f / (1.0f - p), dz_amax);
    POD_CHECK_LAUNCH();
    return POD_OK;
}
