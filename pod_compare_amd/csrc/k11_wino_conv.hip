// 3x3 / stride 1 / pad 1 fp32 convolution of the probabilistic RetinaNet head's subnets (probabilistic_retinanet.py:403-427:
// four conv3x3(256 -> 256) + ReLU + Dropout per subnet, evaluated for every MC run on every FPN level) and predictors
// (PR:430-484) as ONE launch per conv layer over all levels and all runs: fp32 Winograd on the fp32 matrix cores
// (v_mfma_f32_32x32x2_f32), bias + ReLU + dropout fused into the store.
//
// Why Winograd: a direct fp32 convolution is bounded by the 157 TFLOP/s fp32 MFMA peak (MIOpen's implicit GEMM reaches
// 0.83 of it on the p3 maps and nothing can reach more than 1.0).  F(2,3) down the rows x F(4,3) along the columns needs
// 4 x 6 = 24 multiply-adds per 2x4 outputs and (c, k) pair instead of 72, so the same matrix cores deliver up to 3x the
// direct-convolution rate, in fp32 throughout.  Error vs a direct fp32 convolution: ~4e-6 of the output scale at C = 256
// (F(2x2,3x3), the first version: 2e-6 and 16 / 36 of the multiply-adds).
//
// Formulation, canvas of block records, patch-in-LDS layout, output staging and the store passes are shared with the split kernel
// (k12_wino_conv_split.hip) and described next to that code in pod_wino.h; this file holds the fp32 inner product.  Filters are
// transformed once (pod_wino_filter_transform) into the order the kernel's lanes load them in.  The predictor convolutions (cls_score,
// bbox_pred, cls_var, bbox_cov: K = 63 / 36 / 90 real channels) write NCHW planes, the layout K1 streams, straight from the staging tile.
//
// Workgroup = 256 threads = 4 waves, one per SIMD: 32 tiles (8 x 4 tiles of 2x4 = 16x16 output pixels) x 64 output
// channels x the 24 Winograd positions.  Wave a owns ROW a of the 4x6 position grid for the 32 tiles and all 64 channels:
// 6 positions x 2 channel blocks of 32x32 = 12 MFMA blocks = 192 accumulator registers.  A row of Bt4 d is one sum or
// difference of two patch rows, then the 6-point column transform: 20 four-channel operations per chunk, and every
// transformed value feeds two MFMAs.  Per chunk of 8 input channels (48 MFMAs per wave) the raw 18x18-pixel input patch is
// staged in LDS by LDS-DMA (no transformed copy exists anywhere; two 12 KB stages) and the filter operands go from L2
// straight into registers (each wave needs only its row's positions: the four waves read each slab byte once).
// With one wave per SIMD every non-MFMA instruction costs issue time on top of the MFMA time (fp32 MFMA and the other pipes
// do not overlap within a wave: measured), so the design minimises them: 27 memory instructions and 40 packed VALU per 48
// MFMAs.  The output transform applies At4 to each wave's row in registers, parks the result in LDS (128 KB) and combines the
// four rows (At2) in the store pass.
//
// Launch: blockIdx & 7 is the XCD (round-robin dispatch); an XCD always works on the same TWO 64-channel filter slices (3 MB for
// C = 256), which therefore stay in that XCD's 4 MB L2, and takes a block with both slices back to back, so that the second
// workgroup's patch comes out of the L2 as well (wino_schedule, pod_wino.h).
#include "pod_wino.h"

namespace pod {

// Filter transform (wino_filter_values), written in the order the main kernel's lanes load it:
// U[ks][chunk][q = 6 a + p][h][j][s] = U_q[c = 8 chunk + 4 h + s][k = 64 ks + j] (16 bytes per lane and position); channels >= K are zero.
__global__ void __launch_bounds__(256) k_wino_filter(const float* __restrict__ w, float* __restrict__ U, int32_t K, int32_t C, int32_t Kpad) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (int64_t)Kpad * C) return;
    const int k = (int)(t / C), c = (int)(t % C);
    float u[4][6];
    wino_filter_values(w, k, c, K, C, u);
    const int nchunk = C / 8, ks = k >> 6, j64 = k & 63, ch = c >> 3, cc = c & 7;
    const int h = cc >> 2, sc = cc & 3;
    float* dst = U + ((int64_t)ks * nchunk + ch) * WINO_U_FLOATS + (h * 64 + j64) * 4 + sc;
#pragma unroll
    for (int q = 0; q < 24; ++q) dst[q * 512] = u[q / 6][q % 6];
}

__global__ void __launch_bounds__(256, 1) k_wino_conv3x3(const WinoParams P) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int ks, tb;
    wino_schedule(P.KS, P.n_blocks, ks, tb);
    if (tb >= P.n_blocks) return;
    WINO_STAMP(0);
    WINO_STAMP_WALL(12);
    uint32_t slot_e[12];
    int mini_pidx[3], dmini[3], doff[12];                                 // the lane's fills: pod_wino.h
    WINO_FILL_SLOTS(slot_e, mini_pidx, tid);
    // the filter operands of chunk 0 do not depend on the block record either: straight from L2 into registers, asked for now
    const int nchunk = P.C >> 3;
    const int i32 = lane & 31, h = lane >> 5;
    const int a = __builtin_amdgcn_readfirstlane(wave);
    const auto u_rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(P.sets.U[0] + ((int64_t)ks * nchunk) * WINO_U_FLOATS), 0,
                                                          nchunk * WINO_U_FLOATS * 4, 0x00020000);
    const int u_off = ((a * 6 * 2 + h) * 64 + i32) * 16;                               // + (p*2*64 + kb*32)*16 bytes, + chunk*48 KB
    f32x4 uA[12];
    // a lane needs U_q[its 4 channels][its output channel] for its row's 6 positions and both channel blocks = 12 x 16 bytes per chunk of
    // 8 input channels, one chunk ahead (one buffer_load_dwordx4 each); the four waves together read each slab byte exactly once
    auto filter_piece = [&](int ch, f32x4(&u)[12], int i) {
        u[i] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(u_rsrc, u_off, ch * (WINO_U_FLOATS * 4) + ((i >> 1) * 128 + (i & 1) * 32) * 16, 0));
    };
#pragma unroll
    for (int i = 0; i < 12; ++i) filter_piece(0, uA, i);
    const WinoBlock B = wino_block(P.blocks[tb]);
    int row0, row1;
    float sgn;
    wino_rows(a, row0, row1, sgn);
    const int ty = i32 >> 2, tx = i32 & 3;
    const uint32_t lds_base = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) float*)lds;
    uint32_t areg[2][2][4];                                               // LDS byte address in stage 0: [row0 / row1][columns 0-3 / 4-5][chunk of the super-chunk]
#pragma unroll
    for (int rs = 0; rs < 2; ++rs) {
        const int py = 2 * ty + (rs ? row1 : row0);
        const int p0 = 2 * (((py & 3) + 4 * (py >> 3)) * 18 + 4 * tx) + ((py >> 2) & 1);   // slot of column 0 of the tile; column c: + 2 c
#pragma unroll
        for (int cl = 0; cl < 2; ++cl) {
            const int rot = ((tx + cl) & 3) + 4 * ((py >> 1) & 1);
#pragma unroll
            for (int c = 0; c < 4; ++c) areg[rs][cl][c] = lds_base + p0 * 128 + ((2 * c + h + rot) & 7) * 16;
        }
    }
    uint32_t amini[2];                                                    // LDS byte address in mini stage 0: [row0 / row1]; column c: + ((c & 3) 5 + (c >> 2)) 32
#pragma unroll
    for (int rs = 0; rs < 2; ++rs) amini[rs] = lds_base + 2 * WINO_SB_FLOATS * 4 + ((2 * ty + (rs ? row1 : row0)) * 21 + tx) * 32 + h * 16;
    const auto r_rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(P.sets.in[0] + B.base_px * P.in_stride), 0,
                                                          B.n_img * B.HWi * P.in_stride * 4, 0x00020000);
    int* const pix_tab = wino_pixel_table(lds);
    const uint32_t need[2] = {~0u, ~0u};                                  // need bits of the patch pixels: all (no sparse launches)
    WINO_FILL_PIXEL_TABLE(pix_tab, B, need, tid);
    wino_mini_offsets(&P, pix_tab, mini_pidx, dmini, lane);
    auto main_offsets = [&]() {
#pragma unroll
        for (int i = 0; i < 12; ++i) doff[i] = pix_tab[slot_e[i] & 0xFFFF];                  // 12 independent LDS reads, one round trip
#pragma unroll
        for (int i = 0; i < 12; ++i) doff[i] = wino_byte_offset(&P, doff[i], 4 * (((lane & 7) - (int)(slot_e[i] >> 16)) & 7));
    };

    f32x16 acc[12];                                                      // [p][kb]; never cleared: chunk 0's first k-step multiplies into a zero C

    f32x4 x[12], uB[12], vA[6], vB[6], t[6], w6[4];                      // x[row][c], u[p][kb] (uA: above), v[p]: 4 channels each
    if (POD_WINO_ELIM) {                                                  // (elimination builds: operands that were never loaded still need values)
#pragma unroll
        for (int i = 0; i < 12; ++i) x[i] = uA[i] = uB[i] = f32x4{1e-3f, 2e-3f, 3e-3f, 4e-3f} * (float)(lane + i);
#pragma unroll
        for (int i = 0; i < 6; ++i) vA[i] = vB[i] = f32x4{1e-3f, 2e-3f, 3e-3f, 4e-3f} * (float)(lane - i);
    }
    // 12 pieces: one ds_read_b128 each, stage par, chunk c of its super-chunk.  Issued as asm: hipcc orders every LDS read it can
    // see behind ALL pending LDS-DMA (vmcnt(0): it cannot tell the two stages apart), which would drain the pieces flying into the
    // other stage; so the reads are hidden from it and their completion is counted by hand (WINO_WAIT_LGKM0 before the transform).
#define WINO_READ(par, c, i)                                                                                                        \
    asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(x[i]) : "v"(areg[(i) / 6][((i) % 6) >> 2][c]), "i"((par) * WINO_SB_FLOATS * 4 + ((i) % 6) * 256))
#define WINO_READ_MINI(which, i)                                                                                                     \
    asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(x[i]) : "v"(amini[(i) / 6]), "i"((which) * 12288 + ((((i) % 6) & 3) * 5 + (((i) % 6) >> 2)) * 32))
    // packed fp32 arithmetic on the halves of a 4-channel value: r = q * k + p
    auto pk_fma = [](f32x2 k2, f32x2 q, f32x2 p) {
        f32x2 r;
        asm volatile("v_pk_fma_f32 %0, %1, %2, %3" : "=v"(r) : "v"(k2), "v"(q), "v"(p));
        return r;
    };
    auto pk_add = [](f32x2 p, f32x2 q) {
        f32x2 r;
        asm volatile("v_pk_add_f32 %0, %1, %2" : "=v"(r) : "v"(p), "v"(q));
        return r;
    };
    auto pk_sub = [](f32x2 p, f32x2 q) {
        f32x2 r;
        asm volatile("v_pk_add_f32 %0, %1, %2 neg_lo:[0,1] neg_hi:[0,1]" : "=v"(r) : "v"(p), "v"(q));
        return r;
    };
    auto fma4 = [&](float k, f32x4 q, f32x4 p) {   // q * k + p
        const f32x2 k2 = f32x2{k, k};
        const f32x2 l = pk_fma(k2, f32x2{q.x, q.y}, f32x2{p.x, p.y}), hq = pk_fma(k2, f32x2{q.z, q.w}, f32x2{p.z, p.w});
        return f32x4{l.x, l.y, hq.x, hq.y};
    };
    auto add4 = [&](f32x4 p, f32x4 q) { const f32x2 l = pk_add(f32x2{p.x, p.y}, f32x2{q.x, q.y}), hq = pk_add(f32x2{p.z, p.w}, f32x2{q.z, q.w}); return f32x4{l.x, l.y, hq.x, hq.y}; };
    auto sub4 = [&](f32x4 p, f32x4 q) { const f32x2 l = pk_sub(f32x2{p.x, p.y}, f32x2{q.x, q.y}), hq = pk_sub(f32x2{p.z, p.w}, f32x2{q.z, q.w}); return f32x4{l.x, l.y, hq.x, hq.y}; };
    // row a of V = Bt4 d Bt6^T for the lane's tile, 10 pieces of two 4-channel operations:
    //   t_c = x0_c + s x1_c (6);  V0 = 4 t0 - 5 t2 + t4;  V5 = 4 t1 - 5 t3 + t5;  e = t4 - 4 t2, o = t3 - 4 t1: V1 = e + o, V2 = e - o;
    //   f = t4 - t2, g = 2 (t3 - t1): V3 = f + g, V4 = f - g
    auto transform_piece = [&](f32x4(&v)[6], int i) {
        if (i < 3) {
#pragma unroll
            for (int c = 2 * i; c < 2 * i + 2; ++c) t[c] = fma4(sgn, x[6 + c], x[c]);
        } else if (i == 3) {
            w6[0] = fma4(-5.0f, t[2], t[4]);          // t4 - 5 t2
            w6[1] = fma4(-5.0f, t[3], t[5]);          // t5 - 5 t3
        } else if (i == 4) {
            v[0] = fma4(4.0f, t[0], w6[0]);
            v[5] = fma4(4.0f, t[1], w6[1]);
        } else if (i == 5) {
            w6[0] = fma4(-4.0f, t[2], t[4]);          // e
            w6[1] = fma4(-4.0f, t[1], t[3]);          // o
        } else if (i == 6) {
            v[1] = add4(w6[0], w6[1]);
            v[2] = sub4(w6[0], w6[1]);
        } else if (i == 7) {
            w6[2] = sub4(t[4], t[2]);                 // f
            w6[3] = sub4(t[3], t[1]);                 // g / 2
        } else if (i == 8) {
            v[3] = fma4(2.0f, w6[3], w6[2]);
        } else if (i == 9) {
            v[4] = fma4(-2.0f, w6[3], w6[2]);
        }
    };

    // One chunk = 8 input channels = 48 MFMAs (k-step j / 12 = channel of the lane's four, accumulator j % 12 = (p, kb)) with the next
    // chunk's work slotted behind them, at most one memory instruction per MFMA (the order is pinned in the source: the four waves
    // of the workgroup run in lock step, memory instructions issued in a burst queue behind each other and stall the in-order
    // instruction streams): patch reads of chunk ch+1 (LDS), filter loads of chunk ch+1 (L2), its transform, and a quarter of the
    // LDS-DMA of a later SUPER-CHUNK (4 chunks, two stages).  Chunk c of super-chunk s reads stage s & 1 (c = 3: the first chunk of
    // s + 1 from the other stage).  Super-chunk s + 1 is fetched into the stage s - 1 left behind, 4 instructions per wave during
    // each of the chunks (s-1, 3), (s, 0), (s, 1) -- every piece has a whole chunk to land before the barrier that publishes it.
#define WINO_MFMA(V, U, j)                                                                                                   \
    acc[(j) % 12] = __builtin_amdgcn_mfma_f32_32x32x2f32(U[(j) % 12][(j) / 12], V[((j) % 12) >> 1][(j) / 12], acc[(j) % 12], 0, 0, 0)
    const int last = nchunk - 1, last_s = last >> 2;
#pragma unroll
    for (int r = 0; r < 3; ++r) wino_mini_piece(r_rsrc, lds, a, 0, r, dmini[r]);
#pragma unroll
    for (int r = 0; r < 3; ++r) wino_mini_piece(r_rsrc, lds, a, last < 1 ? 0 : 1, r, dmini[r]);
    WINO_STAMP(9);
    main_offsets();                                    // (behind the first loads: their latency hides it)
    WINO_STAMP(10);
#pragma unroll
    for (int i = 0; i < 12; ++i) wino_patch_piece(r_rsrc, lds, a, 0, i, doff[i]);
#pragma unroll
    for (int i = 0; i < 4; ++i) wino_patch_piece(r_rsrc, lds + WINO_SB_FLOATS, a, last_s < 1 ? last_s : 1, i, doff[i]);
    WINO_STAMP(11);
    __builtin_amdgcn_s_waitcnt(WINO_WAIT_VM16);        // the mini stages and the filters of chunk 0 have landed; the 16 pieces of the stages fly on
    __builtin_amdgcn_s_barrier();
    WINO_STAMP(1);
    WINO_READ_MINI(0, 0); WINO_READ_MINI(0, 1); WINO_READ_MINI(0, 2); WINO_READ_MINI(0, 3); WINO_READ_MINI(0, 4); WINO_READ_MINI(0, 5);
    WINO_READ_MINI(0, 6); WINO_READ_MINI(0, 7); WINO_READ_MINI(0, 8); WINO_READ_MINI(0, 9); WINO_READ_MINI(0, 10); WINO_READ_MINI(0, 11);
    __builtin_amdgcn_s_waitcnt(WINO_WAIT_LGKM0);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int i = 0; i < 10; ++i) transform_piece(vA, i);
    // the transform's packed instructions are asm: hipcc neither pads the VALU-write -> MFMA-operand hazard behind them nor keeps the
    // first MFMA from being scheduled up among them (it reads a stale operand then: measured) -- fence and pad by hand
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("s_nop 1");
    WINO_STAMP(2);
    const f32x16 zero16 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    auto chunk = [&](auto first, auto c_t, auto par_t, int sc, f32x4(&vC)[6], f32x4(&uC)[12], f32x4(&vN)[6], f32x4(&uN)[12]) {
        constexpr int c = decltype(c_t)::value, par = decltype(par_t)::value;
        constexpr int rc = (c + 1) & 3, rpar = c == 3 ? par ^ 1 : par;            // what the reads fetch: the NEXT chunk's patch
        constexpr int ph = c == 3 ? 0 : c + 1, dpar = c == 3 ? par : par ^ 1;     // fill phase (c == 2: none) and the stage being filled
        const int ch = 4 * sc + c, c1 = ch + 1 < nchunk ? ch + 1 : last;
        const int fs0 = c == 3 ? sc + 2 : sc + 1, fs = fs0 < last_s ? fs0 : last_s;
        float* wr = lds + dpar * WINO_SB_FLOATS;
        wino_static_for([&](auto J) __attribute__((always_inline)) {
            constexpr int j = decltype(J)::value;
            if constexpr (decltype(first)::value && j < 12) acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(uC[j][0], vC[j >> 1][0], zero16, 0, 0, 0);
            else WINO_MFMA(vC, uC, j);
            if constexpr (j < 12) {
                if constexpr (decltype(first)::value) WINO_READ_MINI(1, j);                  // chunk 1's patch: the second mini stage
                else if (!(POD_WINO_ELIM & 1)) WINO_READ(rpar, rc, j);
            }
            else if constexpr (j < 24) { if (!(POD_WINO_ELIM & 2)) filter_piece(c1, uN, j - 12); }
            else if constexpr (j == 24) __builtin_amdgcn_s_waitcnt(WINO_WAIT_LGKM0);         // the 12 reads (issued 12+ MFMAs ago)
            else if constexpr (j >= 25 && j < 35) { if (!(POD_WINO_ELIM & 8)) transform_piece(vN, j - 25); }
            else if constexpr (j >= 36 && j <= 45 && (j - 36) % 3 == 0 && c != 2) { if (!(POD_WINO_ELIM & 4)) wino_patch_piece(r_rsrc, wr, a, fs, 4 * ph + (j - 36) / 3, doff[4 * ph + (j - 36) / 3]); }
            __builtin_amdgcn_sched_barrier(0);
        }, std::make_integer_sequence<int, 48>{});
        if (!(POD_WINO_ELIM & 16)) {
            // the filters of the next chunk and every patch piece issued before this chunk have landed; this chunk's 4 pieces may fly on
            __builtin_amdgcn_s_waitcnt(c != 2 ? WINO_WAIT_VM4 : WINO_WAIT_VM0);
            __builtin_amdgcn_s_barrier();
        }
    };
    using std::integral_constant;
    chunk(std::true_type{}, integral_constant<int, 0>{}, integral_constant<int, 0>{}, 0, vA, uA, vB, uB);
    for (int base = 0;; base += 8) {
#define WINO_CHUNK(t)                                                                                                              \
    if (base + (t) >= nchunk) break;                                                                                               \
    if ((t) & 1) chunk(std::false_type{}, integral_constant<int, (t) & 3>{}, integral_constant<int, ((t) >> 2) & 1>{}, (base + (t)) >> 2, vB, uB, vA, uA); \
    else chunk(std::false_type{}, integral_constant<int, (t) & 3>{}, integral_constant<int, ((t) >> 2) & 1>{}, (base + (t)) >> 2, vA, uA, vB, uB);
        WINO_CHUNK(1) WINO_CHUNK(2) WINO_CHUNK(3) WINO_CHUNK(4) WINO_CHUNK(5) WINO_CHUNK(6) WINO_CHUNK(7) WINO_CHUNK(8)
#undef WINO_CHUNK
    }
#undef WINO_MFMA
    __syncthreads();                                   // every wave is done reading the stages, no DMA in flight: they become the output staging
    WINO_STAMP(3);

    if (!wino_output_stage(acc, lds, a, i32, h)) return;
    // fp32 operands: nothing to scale back (inv = 1: the fma is a plain + bias), no abs-max record, no replicas
    const WinoStore S{P.sets.out[0], P.sets.bias[0], nullptr, 1.0f, P.sets.offset[0], 0, P.sets.k_planes[0]};
    if (S.k_planes > 0) wino_store_planes(P, B, S, lds, ks);
    else wino_store_channels_last(P, B, S, lds, ks);
    WINO_STAMP_END();
}

}  // namespace pod

#ifdef POD_TRACE
extern "C" int pod_wino_trace_dump(long long* host, int32_t n_workgroups) { return pod::wino_trace_dump(host, n_workgroups); }   // diagnostics build only
#endif

extern "C" int pod_wino_filter_transform(const float* weight, float* U, int32_t K, int32_t C, pod_stream_t stream) {
    if (!weight || !U || K < 1 || C < 8 || (C & 7) != 0) return POD_E_INVALID;
    const int32_t Kpad = (K + 63) / 64 * 64;
    const int64_t n = (int64_t)Kpad * C;
    hipLaunchKernelGGL(pod::k_wino_filter, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, weight, U, K, C, Kpad);
    POD_CHECK_LAUNCH();
    return POD_OK;
}

extern "C" int pod_wino_conv3x3(const float* in, float* out, const float* U, const float* bias, const int32_t* blocks, int32_t n_blocks,
                                int32_t C, int32_t K, int32_t k_planes, int32_t relu, float p, uint64_t seed, uint64_t offset,
                                const uint64_t* epoch, pod_stream_t stream) {
    if (!in || !out || in == out || !U || !blocks || n_blocks < 0 || C < 8 || (C & 7) != 0 || K < 64 || (K & 63) != 0 ||
        !(p >= 0.0f && p < 1.0f) || k_planes < 0 || k_planes > K || (k_planes > 0 && p != 0.0f))
        return POD_E_INVALID;
    pod::WinoParams P{};
    const int64_t grid = pod::wino_params_launch(P, blocks, n_blocks, C, K, relu, p, seed, epoch);
    if (grid < 0) return POD_E_INVALID;
    if (!pod_aligned(16, in, out, U, bias, blocks))
        return POD_E_INVALID;
    if (n_blocks == 0) return POD_OK;
    if (pod_lds_opt_in<pod::k_wino_conv3x3>(pod::WINO_LDS_BYTES) != POD_OK) return POD_E_LAUNCH;
    pod::wino_params_set(P, 0, 0, in, out, U, bias, nullptr, nullptr, offset, 0, k_planes);
    hipLaunchKernelGGL(pod::k_wino_conv3x3, dim3((unsigned)grid), dim3(256), pod::WINO_LDS_BYTES, (hipStream_t)stream, P);
    POD_CHECK_LAUNCH();
    return POD_OK;
}
