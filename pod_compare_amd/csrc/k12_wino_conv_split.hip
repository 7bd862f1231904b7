// The head's 3x3 convolutions (probabilistic_retinanet.py:403-484) once more -- same Winograd F(2,3) x F(4,3) formulation, same data
// path (patch as full 128-byte lines by LDS-DMA, filters from L2; prologue, output staging and store passes are the code of pod_wino.h,
// which also explains the canvas and the LDS layouts) and the same results to fp32 rounding as pod_wino_conv3x3 (k11_wino_conv.hip) --
// with every fp32 product formed on the 16-BIT matrix cores.
// Round 5: both operands are scaled by a power of two and split into TWO f16 terms (x s = x0 + x1 to 2^-23 |x s|, pod_wino.h) and the
// three partial products that matter (x0 u1, x1 u0, x0 u0) are accumulated in fp32 by v_mfma_f32_32x32x16_f16: half the matrix
// instructions of rounds 3-4's 3-way bf16 split (six products), two thirds of its filter bytes and 4/7 of its split arithmetic -- and,
// measured on the matrix cores against fp64 (tools/f16_split_numerics.hip), a SMALLER error than both the bf16 x 6 form and the fp32
// MFMA: the fp32 accumulation chain, not the products, is where these kernels lose bits, and it is half as long.
// The end of the K loop is peeled (chunk counts that are multiples of 4): its last four chunks prepare nothing for a chunk that never comes.
#include "pod_wino.h"

namespace pod {

typedef uint32_t vu32x4 __attribute__((ext_vector_type(4)));
constexpr int WINO_US_BYTES = 24 * 2 * 2 * 64 * 16;      // pre-split filter terms of a 16-channel chunk: [24 positions][kb][term][h][j][8 f16]  96 KB
constexpr int WINO_U_TOP = 14, WINO_V_TOP = 9;           // scaled filter abs-max in [2^14, 2^15); activations: 2^9 <= s amax < 2^10, x gain of Bt4 (x) Bt6 < 32
constexpr int WINO_WAIT_VM24 = 0x4078;                    // lgkmcnt(0) vmcnt(24)
constexpr int WINO_TAIL_NO_LOAD = 1, WINO_TAIL_NO_PARK = 2, WINO_TAIL_LAST = 4;      // what a chunk at the end of the K loop leaves out (`chunk` in k_wino_conv3x3_split)

// Filter transform U = G4 g G6t (wino_filter_values).  Two passes: the abs-max of U (-> the trailer word of Us, behind the terms), then
// every value times the power of two that puts that abs-max into [2^14, 2^15) split into two f16 terms (round to nearest even) and
// written in the order the kernel's lanes load them:
// Us[ks][chunk16][q = 6 a + p][kb][term][h][j][e] = term(s U_q[c = 16 chunk16 + 8 h + e][k = 64 ks + 32 kb + j]); channels >= K are zero.
__global__ void __launch_bounds__(256) k_wino_filter_amax(const float* __restrict__ w, float* __restrict__ amax, int32_t K, int32_t C, int32_t Kpad) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    float m = 0.0f;
    if (t < (int64_t)Kpad * C) {
        float u[4][6];
        wino_filter_values(w, (int)(t / C), (int)(t % C), K, C, u);
#pragma unroll
        for (int i = 0; i < 24; ++i) m = fmaxf(m, fabsf(u[i / 6][i % 6]));
    }
    wino_publish_amax1(amax, m);
}
__global__ void __launch_bounds__(256) k_wino_filter_split(const float* __restrict__ w, uint16_t* __restrict__ Us, const float* __restrict__ amax,
                                                           int32_t K, int32_t C, int32_t Kpad) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (int64_t)Kpad * C) return;
    const int k = (int)(t / C), c = (int)(t % C);
    float u[4][6];
    wino_filter_values(w, k, c, K, C, u);
    const float sc = wino_pow2_scale(*amax, WINO_U_TOP);
    const int nchunk = C / 16, ks = k >> 6, kb = (k >> 5) & 1, j32 = k & 31, ch = c >> 4, hh = (c >> 3) & 1, e = c & 7;
    uint16_t* dst = Us + (((int64_t)ks * nchunk + ch) * (int64_t)WINO_US_BYTES) / 2 + (hh * 32 + j32) * 8 + e;
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int p = 0; p < 6; ++p) {
            const float x = u[a][p] * sc;                                        // exact
            const _Float16 h0 = (_Float16)x;                                     // v_cvt_f16_f32: round to nearest even
            const _Float16 h1 = (_Float16)(x - (float)h0);
            uint16_t* d = dst + (((a * 6 + p) * 2 + kb) * 2) * 512;            // 512 f16 = 64 lanes x 8 per (position, kb, term)
            d[0] = __builtin_bit_cast(uint16_t, h0);
            d[512] = __builtin_bit_cast(uint16_t, h1);
        }
}

__global__ void __launch_bounds__(256, 1) k_wino_conv3x3_split(const WinoParams P) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int ks, tb;
    wino_schedule(P.KS, P.n_blocks, ks, tb);
    if (tb >= P.n_blocks) return;
    uint32_t need[2] = {~0u, ~0u};                                        // need bits of this thread's patch pixels (tid, tid + 256): all, unless sparse
    if (P.live) {                                                         // sparse launch: slot -> live entry {record, need bits} (uniform: scalar loads)
        if (tb >= P.live[0]) return;
        const int32_t* const ent = P.live + POD_SPARSE_LIVE_HEAD + (int64_t)POD_SPARSE_LIVE_STRIDE * tb;
        tb = ent[0];
        // a patch pixel the layer below did not have to compute for this image reads as 0.0 (k15_sparse_blocks.hip): nothing an earlier
        // image left in the buffer is ever read, so the launch -- its abs-max record included -- is a function of this image alone
        need[0] = (uint32_t)ent[1 + (tid >> 5)];
        need[1] = (uint32_t)ent[9 + (tid >> 5 < 3 ? tid >> 5 : 2)];
    }
    WINO_STAMP(0);
    WINO_STAMP_WALL(12);
    uint32_t slot_e[12];
    int mini_pidx[3], dmini[3], doff[12];                                 // the lane's fills: pod_wino.h
    WINO_FILL_SLOTS(slot_e, mini_pidx, tid);
    // the filter operands of the first position of chunk 0 do not depend on the block record either: asked for now
    const int nchunk_all = P.C >> 4;                                      // chunks of 16 input channels (one bf16 MFMA k-step)
    const int nchunk = P.c_split ? P.c_split : nchunk_all;                // ... of which this workgroup set (blockIdx.y) accumulates its own range
    const int chunk0 = (int)blockIdx.y * nchunk;
    const int i32 = lane & 31, h = lane >> 5;
    const int a = __builtin_amdgcn_readfirstlane(wave);
    // which convolution of a grouped launch this block belongs to: read off the block index alone (no memory in the way of the first
    // filter loads below)
    const int set = (tb >= P.sets.first[1] ? 1 : 0) + (tb >= P.sets.first[2] ? 1 : 0) + (tb >= P.sets.first[3] ? 1 : 0);
    const float* const set_U = P.sets.U[set];
    const float* const set_in = P.sets.in[set];
    float* const set_out = P.sets.out[set];
    const float* const set_bias = P.sets.bias[set];
    // operand scales of the f16 split (pod_wino.h): two scalar loads, asked for first and needed only when the first patch is split
    const float in_amax_slot = wino_load_amax(P.sets.in_amax[set]);
    const float u_amax = *reinterpret_cast<const float*>(reinterpret_cast<const char*>(set_U) + (int64_t)P.KS * (P.C >> 4) * WINO_US_BYTES);
    float* const set_out_amax = P.sets.out_amax[set];
    const uint64_t set_offset = P.sets.offset[set];
    const int set_replicas = P.sets.replicas[set], set_k_planes = P.sets.k_planes[set];
    const auto u_rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(reinterpret_cast<const char*>(set_U) + ((int64_t)ks * nchunk_all + chunk0) * WINO_US_BYTES), 0,
                                                          nchunk * WINO_US_BYTES, 0x00020000);
    const int u_off = (a * 6 * 4 * 64 + h * 32 + i32) * 16;              // + ((p*2 + kb)*2 + term) KB, + chunk * 96 KB
    constexpr int WINO_U_LEAD = 3;   // positions the filter loads run ahead of their MFMAs (a position's 6 MFMAs last 192 cycles, an L2 round trip under load ~3x that)
    vu32x4 uP[6][4];                                                       // the filter terms of position p live in uP[p % 3]: [kb][term]; loaded TWO positions ahead (a position's
                                                                          // 6 MFMAs last 192 cycles, an L2 round trip under load longer)
    auto filter_piece = [&](int q16, int p, vu32x4(&u)[4], int i) {       // i = kb*2 + term: one buffer_load_dwordx4 (8 f16) each
        u[i] = __builtin_bit_cast(vu32x4, __builtin_amdgcn_raw_buffer_load_b128(u_rsrc, u_off, q16 * WINO_US_BYTES + (p * 4 + i) * 1024, 0));
    };
#pragma unroll
    for (int pp = 0; pp < WINO_U_LEAD; ++pp)
#pragma unroll
        for (int i = 0; i < 4; ++i) filter_piece(0, pp, uP[pp], i);
    const WinoBlock B = wino_block(P.blocks[tb]);
    int row0, row1;
    float sgn;
    wino_rows(a, row0, row1, sgn);
    const int ty = i32 >> 2, tx = i32 & 3;
    const uint32_t lds_base = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) float*)lds;
    uint32_t areg[2][2][2][2];                                            // LDS byte address in stage 0: [row0 / row1][columns 0-3 / 4-5][16-channel half of the super-chunk][4-channel half of the lane's 8]
    uint32_t amini[2];                                                    // LDS byte address in mini stage h (the lane's 8 channels of chunk 0): [row0 / row1]; + 16: second half
#pragma unroll
    for (int rs = 0; rs < 2; ++rs) {
        const int py = 2 * ty + (rs ? row1 : row0);
        const int p0 = 2 * (((py & 3) + 4 * (py >> 3)) * 18 + 4 * tx) + ((py >> 2) & 1);   // slot of column 0 of the tile; column c: + 2 c
#pragma unroll
        for (int cl = 0; cl < 2; ++cl) {
            const int rot = ((tx + cl) & 3) + 4 * ((py >> 1) & 1);
#pragma unroll
            for (int c16 = 0; c16 < 2; ++c16)
#pragma unroll
                for (int hf = 0; hf < 2; ++hf) areg[rs][cl][c16][hf] = lds_base + p0 * 128 + ((4 * c16 + 2 * h + hf + rot) & 7) * 16;
        }
    }
#pragma unroll
    for (int rs = 0; rs < 2; ++rs) amini[rs] = lds_base + 2 * WINO_SB_FLOATS * 4 + h * 12288 + ((2 * ty + (rs ? row1 : row0)) * 21 + tx) * 32;
    // the workgroup's own range of input channels starts at chunk0 (input-channel splits): so does its buffer
    const auto r_rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(set_in + B.base_px * P.in_stride + chunk0 * 16), 0,
                                                          B.n_img * B.HWi * P.in_stride * 4 - chunk0 * 64, 0x00020000);
    int* const pix_tab = wino_pixel_table(lds);
    WINO_FILL_PIXEL_TABLE(pix_tab, B, need, tid);
    wino_mini_offsets(&P, pix_tab, mini_pidx, dmini, lane);
    auto main_offsets = [&]() {
#pragma unroll
        for (int i = 0; i < 12; ++i) doff[i] = pix_tab[slot_e[i] & 0xFFFF];                  // 12 independent LDS reads, one round trip
#pragma unroll
        for (int i = 0; i < 12; ++i) doff[i] = wino_byte_offset(&P, doff[i], 4 * (((lane & 7) - (int)(slot_e[i] >> 16)) & 7));
    };

    // Between the 32-cycle bf16 MFMAs an LDS-DMA piece costs its ~100 issue cycles in full (behind the 64-cycle fp32 MFMAs most of it
    // hides), so the K loop fills the stages through registers: every chunk loads 6 pieces (one buffer_load_dwordx4 each) and parks the
    // 6 it loaded a chunk earlier (ds_write_b128: free).
    f32x4 stg[6];
    const uint32_t stg_addr = lds_base + a * 12288 + lane * 16;          // + stage * 48 KB + piece * 1 KB
    auto stage_load = [&](int k, int sc, int i) {
        stg[k] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r_rsrc, doff[i], sc * 128, 0));
    };
    auto stage_write = [&](int par, int k, int i) {
        *reinterpret_cast<__attribute__((address_space(3))) f32x4*>((uintptr_t)(stg_addr + par * (WINO_SB_FLOATS * 4) + i * 1024)) = stg[k];
    };

    f32x16 acc[12];                                                      // [p][kb]; never cleared: chunk 0's first product multiplies into a zero C
    f32x4 x[12];                                                         // raw patch, one 4-channel half at a time: x[row][c]
    vu32x4 Vb[6][2];                                                      // the transformed patch as f16 operands: [position][term], 8 channels (regs 0-1: channels 0-3, 2-3: 4-7)
    float tN[6][4], vN[2][6][4];                                         // the NEXT chunk's transform in flight: row-combined columns; transformed values [half][position] (fp32, split later)
    if (POD_WINO_ELIM) {                                                  // (elimination builds: operands that were never loaded still need values)
#pragma unroll
    for (int i = 0; i < 12; ++i) Vb[i / 2][i % 2] = vu32x4{0x3c003c00u + i, 0x3c003c00u, 0x3c003c00u, 0x3c003c00u + lane};
#pragma unroll
    for (int i = 0; i < 12; ++i) x[i] = f32x4{1e-3f, 2e-3f, 3e-3f, 4e-3f} * (float)(lane + i);
#pragma unroll
    for (int i = 0; i < 48; ++i) vN[i / 24][(i / 4) % 6][i % 4] = x[i / 4][i % 4];
#pragma unroll
    for (int i = 0; i < 24; ++i) tN[i / 4][i % 4] = x[i / 4][i % 4];
    }
    // (reads as asm with hand-counted completion: see k11_wino_conv.hip)
#define WINO_READ(par, c16, hf, i)                                                                                                  \
    asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(x[i]) : "v"(areg[(i) / 6][((i) % 6) >> 2][c16][hf]), "i"((par) * WINO_SB_FLOATS * 4 + ((i) % 6) * 256))
#define WINO_READ_MINI(hf, i)                                                                                                        \
    asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(x[i]) : "v"(amini[(i) / 6]), "i"((hf) * 16 + ((((i) % 6) & 3) * 5 + (((i) % 6) >> 2)) * 32))
#define WINO_READ12(M, ...)                                                                                                          \
    M(__VA_ARGS__, 0); M(__VA_ARGS__, 1); M(__VA_ARGS__, 2); M(__VA_ARGS__, 3); M(__VA_ARGS__, 4); M(__VA_ARGS__, 5);                \
    M(__VA_ARGS__, 6); M(__VA_ARGS__, 7); M(__VA_ARGS__, 8); M(__VA_ARGS__, 9); M(__VA_ARGS__, 10); M(__VA_ARGS__, 11)
    // the reads have landed: the wait is tied to the twelve values, so that nothing computed from them can be scheduled above it
#define WINO_READS_LANDED()                                                                                                           \
    asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(x[0]), "+v"(x[1]), "+v"(x[2]), "+v"(x[3]), "+v"(x[4]), "+v"(x[5]), "+v"(x[6]), "+v"(x[7]), \
                 "+v"(x[8]), "+v"(x[9]), "+v"(x[10]), "+v"(x[11]))
    // Row a of V = Bt4 d Bt6^T for the lane's tile and 4 channels -- the SAME operations in the same order as the fp32 kernel's
    // packed transform (fused multiply-adds where it has them), but as scalar instructions (this file is compiled with
    // -fno-slp-vectorize): beside bf16 MFMAs a packed fp32 instruction costs ~40 cycles (profiles/r04_experiments.md), an ordinary one
    // nothing --, then every value split into three bf16 terms by round-to-nearest (v = v0 + v1 + v2 to 2^-26 |v|; truncation would
    // make the dropped partial products one-signed: a bias the Winograd cancellation amplifies -- measured) and packed pairwise.
    //
    // The pieces of that work, so that they can be slotted behind MFMAs one small unit at a time (`unit` below) or run back to back
    // (`make_v`: the first two chunks).  The units keep their slots through the sched_barrier behind every MFMA (round 4 also pinned their
    // inputs and results with empty volatile asm: measured in round 5 to change nothing but +65 s_nop per chunk, deleted in round 6).
    auto rows_combine = [&](int c0, int c1) __attribute__((always_inline)) {              // tN[c] = x0[c] + s x1[c]
#pragma unroll
        for (int c = c0; c < c1; ++c) {
#pragma unroll
            for (int e = 0; e < 4; ++e) tN[c][e] = __builtin_fmaf(sgn, x[6 + c][e], x[c][e]);
        }
    };
    float w0s[4], w1s[4], evs[4], ods[4], fs[4], gs[4];                                   // column transform, first level (per channel e)
    auto columns_level1 = [&](int e) __attribute__((always_inline)) {
        w0s[e] = __builtin_fmaf(-5.0f, tN[2][e], tN[4][e]);
        w1s[e] = __builtin_fmaf(-5.0f, tN[3][e], tN[5][e]);
        evs[e] = __builtin_fmaf(-4.0f, tN[2][e], tN[4][e]);
        ods[e] = __builtin_fmaf(-4.0f, tN[1][e], tN[3][e]);
        fs[e] = tN[4][e] - tN[2][e];
        gs[e] = tN[3][e] - tN[1][e];
    };
    auto columns_level2 = [&](int hf, int e) __attribute__((always_inline)) {
        vN[hf][0][e] = __builtin_fmaf(4.0f, tN[0][e], w0s[e]);
        vN[hf][5][e] = __builtin_fmaf(4.0f, tN[1][e], w1s[e]);
        vN[hf][1][e] = evs[e] + ods[e];
        vN[hf][2][e] = evs[e] - ods[e];
        vN[hf][3][e] = __builtin_fmaf(2.0f, gs[e], fs[e]);
        vN[hf][4][e] = __builtin_fmaf(-2.0f, gs[e], fs[e]);
    };
    // The two f16 terms of position p's 8 values (4 channel pairs: pair i = half i >> 1, channels 2 (i & 1) ..), in three steps whose
    // operations are independent of each other inside a step (a pair's own chain is convert -> residual -> convert):
    // w = nearest-even f16 pair of (v s) (v_fma_mixlo/hi_f16), residual r = v s - w exactly (v_fma_mix_f32, in place: vN is dead
    // afterwards), second term = nearest-even f16 pair of r (v_cvt_pk_f16_f32).
    const float sv = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, wino_pow2_scale(wino_reduce_amax(in_amax_slot), WINO_V_TOP))));
    auto split_convert = [&](int p, int term) __attribute__((always_inline)) {
        vu32x4 w;
#pragma unroll
        for (int i = 0; i < 4; ++i) {                                                      // i = 2 hf + pair: regs 0-1 channels 0-3, 2-3 channels 4-7
            w[i] = term == 0 ? wino_f16_pair_scaled(vN[i >> 1][p][2 * (i & 1)], vN[i >> 1][p][2 * (i & 1) + 1], sv)
                             : wino_f16_pair(vN[i >> 1][p][2 * (i & 1)], vN[i >> 1][p][2 * (i & 1) + 1]);
        }
        Vb[p][term] = w;
    };
    auto split_residual = [&](int p, int i0, int i1) __attribute__((always_inline)) {      // v <- v s - the first term, exactly
#pragma unroll
        for (int i = i0; i < i1; ++i) {
            float& lo = vN[i >> 1][p][2 * (i & 1)];
            float& hi = vN[i >> 1][p][2 * (i & 1) + 1];
            wino_f16_residual_scaled(Vb[p][0][i], lo, hi, sv);
        }
    };
    auto split_position = [&](int p) __attribute__((always_inline)) {                      // all three steps back to back
        split_convert(p, 0); split_residual(p, 0, 4); split_convert(p, 1);
    };
    auto make_v = [&](int hf) __attribute__((always_inline)) {                             // serial form: x (12 reads of half hf) -> vN[hf]
        if (POD_WINO_ELIM & 8) return;
        rows_combine(0, 6);
#pragma unroll
        for (int e = 0; e < 4; ++e) columns_level1(e);
#pragma unroll
        for (int e = 0; e < 4; ++e) columns_level2(hf, e);
    };
    auto split_all = [&]() __attribute__((always_inline)) {
        if (POD_WINO_ELIM & 8) return;
#pragma unroll
        for (int p = 0; p < 6; ++p) split_position(p);
    };

    // One chunk = 16 input channels = one k-step of v_mfma_f32_32x32x16_f16.  Every fp32 product x * u is formed from the two f16 terms
    // of each (scaled) operand: the 3 partial products that matter (x1 u0, x0 u1, x0 u0: small ones first), fp32 accumulate.  36 MFMAs
    // per chunk: positions p = 0..5 of the wave's row, two channel blocks, 3 products; the filter terms of position p + 2 (4 x 16 B per
    // lane, pre-split, from L2) are loaded behind the first four MFMAs of position p.
    //
    // SOFTWARE PIPELINE (round 4, re-slotted for 36 MFMAs in round 5).  The VALU instructions that turn the next chunk's raw patch into f16
    // operands sit BEHIND the MFMAs of the running chunk, one unit of <= 6 independent instructions at a time:
    //     R0      12 LDS reads of the next chunk's first 4-channel half
    //     A       the two terms of the running chunk's own position 5 (its values were computed during the previous chunk; Vb[5] is read
    //             last, and could not be overwritten while the previous chunk's position 5 was still to come)
    //     T0      the row combination of the first half                                             (x -> tN)
    //     R1 V0   the second half's reads; the first half's column transform                       (tN -> vN[0])
    //     T1 V1   the same for the second half                                                      (-> vN[1])
    //     C0..C4  the two terms of the next chunk's positions 0..4 -- each after the running chunk's MFMAs of that position have issued
    // which needs the next chunk's patch to stand in a PUBLISHED stage when the chunk begins: super-chunk s + 1 is therefore complete one
    // chunk earlier than before -- chunk (s - 1, 1) parks its pieces 0..5, chunk (s, 0) pieces 6..11 -- in the stage whose last read (for
    // chunk (s - 1, 1), issued during (s - 1, 0)) lies a barrier behind.
    constexpr int N_UNITS = 58, N_SLOTS = 36;
    auto unit = [&](auto U, auto npar_t, auto n16_t, auto hasA_t) __attribute__((always_inline)) {
        constexpr int u = decltype(U)::value, npar = decltype(npar_t)::value, n16 = decltype(n16_t)::value;
        if constexpr (POD_WINO_ELIM & 8) { if constexpr (u >= 3 && !(u >= 13 && u < 16)) return; }
        if constexpr (u < 3) {                                                             // R0
            if constexpr (!(POD_WINO_ELIM & 1)) { WINO_READ(npar, n16, 0, 4 * u); WINO_READ(npar, n16, 0, 4 * u + 1); WINO_READ(npar, n16, 0, 4 * u + 2); WINO_READ(npar, n16, 0, 4 * u + 3); }
        } else if constexpr (u < 7) {                                                      // A (4 units)
            if constexpr (decltype(hasA_t)::value) {
                constexpr int k = u - 3;
                if constexpr (k == 0) split_convert(5, 0);
                else if constexpr (k == 1) split_residual(5, 0, 2);
                else if constexpr (k == 2) split_residual(5, 2, 4);
                else split_convert(5, 1);
            }
        } else if constexpr (u < 13) {                                                     // T0 (6 units: one column each)
            if constexpr (u == 7) WINO_READS_LANDED();
            rows_combine(u - 7, u - 6);
        } else if constexpr (u < 16) {                                                     // R1
            if constexpr (!(POD_WINO_ELIM & 1)) { WINO_READ(npar, n16, 1, 4 * (u - 13)); WINO_READ(npar, n16, 1, 4 * (u - 13) + 1); WINO_READ(npar, n16, 1, 4 * (u - 13) + 2); WINO_READ(npar, n16, 1, 4 * (u - 13) + 3); }
        } else if constexpr (u < 24) {                                                     // V0 (8 units: level 1 and level 2 of each channel, 6 ops each)
            constexpr int k = u - 16;
            if constexpr (k < 4) columns_level1(k);
            else columns_level2(0, k - 4);
        } else if constexpr (u < 30) {                                                     // T1
            if constexpr (u == 24) WINO_READS_LANDED();
            rows_combine(u - 24, u - 23);
        } else if constexpr (u < 38) {                                                     // V1
            constexpr int k = u - 30;
            if constexpr (k < 4) columns_level1(k);
            else columns_level2(1, k - 4);
        } else {                                                                           // C0..C4
            constexpr int p = (u - 38) / 4, k = (u - 38) % 4;
            if constexpr (k == 0) split_convert(p, 0);
            else if constexpr (k == 1) split_residual(p, 0, 2);
            else if constexpr (k == 2) split_residual(p, 2, 4);
            else split_convert(p, 1);
        }
    };
    // units of slot j: [j * 58 / 36, (j + 1) * 58 / 36) -- C(p) starts at unit 38 + 4 p = slot >= 23 + 2 p >= 6 (p + 1): behind position p's MFMAs
    const int last = nchunk - 1, last_s = last >> 1;
    const int sc1 = last_s < 1 ? last_s : 1;
#pragma unroll
    for (int r = 0; r < 3; ++r) wino_mini_piece(r_rsrc, lds, a, 0, r, dmini[r]);
#pragma unroll
    for (int r = 0; r < 3; ++r) wino_mini_piece(r_rsrc, lds, a, 1, r, dmini[r]);
    WINO_STAMP(9);
    main_offsets();                                    // (behind the first loads: their latency hides it)
    WINO_STAMP(10);
#pragma unroll
    for (int i = 0; i < 12; ++i) wino_patch_piece(r_rsrc, lds, a, 0, i, doff[i]);
#pragma unroll
    for (int i = 0; i < 6; ++i) wino_patch_piece(r_rsrc, lds + WINO_SB_FLOATS, a, sc1, i, doff[i]);       // pieces 0..5 of super-chunk 1 straight into stage 1 ...
#pragma unroll
    for (int i = 0; i < 6; ++i) stage_load(i, sc1, 6 + i);                       // ... its pieces 6..11 through registers (chunk 0 parks them)
    WINO_STAMP(11);
    __builtin_amdgcn_s_waitcnt(WINO_WAIT_VM24);        // the mini stages and the first filter terms have landed; the 18 DMA pieces and the 6 register pieces fly on
    __builtin_amdgcn_s_barrier();
    WINO_STAMP(1);
    WINO_READ12(WINO_READ_MINI, 0);
    WINO_READS_LANDED();
    __builtin_amdgcn_sched_barrier(0);
    make_v(0);
    __builtin_amdgcn_sched_barrier(0);
    WINO_READ12(WINO_READ_MINI, 1);
    WINO_READS_LANDED();
    __builtin_amdgcn_sched_barrier(0);
    make_v(1);
    split_all();
    __builtin_amdgcn_sched_barrier(0);
    WINO_STAMP(2);
    const f32x16 zero16 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    // chunk q = (super-chunk q >> 1, half c16 = q & 1), stage parity par = (q >> 1) & 1.
    //   mode 0: the first chunk (accumulators start from zero; nothing of the next chunk behind its MFMAs: stage 0 is still landing)
    //   mode 1: chunk 1 (operands made back to back after chunk 0; runs units R0 .. C4 for chunk 2)
    //   mode 2: steady state (units A .. C4)
    // tail (the end of the loop, peeled below): what a chunk near the end leaves out because nothing behind the last chunk wants it --
    //   WINO_TAIL_NO_LOAD: no stage loads (the pieces would be of a super-chunk past the last one)
    //   WINO_TAIL_NO_PARK: no stage parks (the registers hold no such pieces), and no barrier at its end: nobody parks into a stage any more
    //   WINO_TAIL_LAST:    the last chunk: the filter terms of its own positions 3..5, the A units and the MFMAs, nothing of a next chunk
    auto chunk = [&](auto mode_t, auto c16_t, auto par_t, auto tail_t, int q) {
        constexpr int mode = decltype(mode_t)::value, c16 = decltype(c16_t)::value, par = decltype(par_t)::value, tail = decltype(tail_t)::value;
        constexpr bool do_load = !(tail & WINO_TAIL_NO_LOAD), do_park = !(tail & WINO_TAIL_NO_PARK), is_last = (tail & WINO_TAIL_LAST) != 0;
        static_assert((tail == 0 || mode == 2) && (!is_last || (!do_load && !do_park)), "tail forms are steady-state chunks; the last one has no stage traffic");
        constexpr int n16 = c16 ^ 1, npar = c16 == 1 ? par ^ 1 : par;             // the NEXT chunk's half and stage
        const int qn = q + 1 <= last ? q + 1 : last;
        // stage traffic: chunk (s, 0) parks pieces 6..11 of super-chunk s + 1 (other stage) and loads 0..5 of s + 2; chunk (s, 1) parks those in
        // its OWN stage (nobody reads it any more: the next chunk's operands come from the other one) and loads 6..11 of s + 2
        const int ls0 = (q >> 1) + 2, ls = ls0 < last_s ? ls0 : last_s;
        wino_static_for([&](auto J) __attribute__((always_inline)) {
            constexpr int j = decltype(J)::value, p = j / 6, m = j % 6, kb = m & 1, prod = m >> 1;
            constexpr int sa = prod == 1 ? 1 : 0;      // filter term of the product
            constexpr int sb = prod == 0 ? 1 : 0;      // patch term:  x1 u0, x0 u1, x0 u0
            if constexpr (mode == 0 && prod == 0)
                acc[p * 2 + kb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(wino_f16x8, uP[p][kb * 2 + sa]), __builtin_bit_cast(wino_f16x8, Vb[p][sb]), zero16, 0, 0, 0);
            else
                acc[p * 2 + kb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(wino_f16x8, uP[p][kb * 2 + sa]), __builtin_bit_cast(wino_f16x8, Vb[p][sb]), acc[p * 2 + kb], 0, 0, 0);
            if constexpr (m < 4 && (!is_last || p + WINO_U_LEAD < 6)) { if (!(POD_WINO_ELIM & 2)) filter_piece(p + WINO_U_LEAD >= 6 ? qn : q, (p + WINO_U_LEAD) % 6, uP[(p + WINO_U_LEAD) % 6], m); }
            if constexpr (m == 4 && do_park) { if (!(POD_WINO_ELIM & 4)) stage_write(c16 == 0 ? par ^ 1 : par, p, c16 == 0 ? 6 + p : p); }
            if constexpr (p == 5 && m >= 4 && do_load) {                    // the 6 stage loads (HBM) sit BEHIND the chunk's last filter loads: loads return in
                if (!(POD_WINO_ELIM & 4)) {                      // order, and every filter term ahead is needed soon
                    stage_load(3 * (m - 4), ls, 6 * c16 + 3 * (m - 4));
                    stage_load(3 * (m - 4) + 1, ls, 6 * c16 + 3 * (m - 4) + 1);
                    stage_load(3 * (m - 4) + 2, ls, 6 * c16 + 3 * (m - 4) + 2);
                }
            }
            if constexpr (mode != 0) {
                constexpr int u0 = j * N_UNITS / N_SLOTS, u1 = (j + 1) * N_UNITS / N_SLOTS;
                wino_static_for([&](auto K) __attribute__((always_inline)) {
                    constexpr int u = u0 + decltype(K)::value;
                    if constexpr (!is_last || (u >= 3 && u < 7))          // (the last chunk: its own A units only)
                        unit(std::integral_constant<int, u>{}, std::integral_constant<int, npar>{}, std::integral_constant<int, n16>{}, std::integral_constant<bool, mode == 2>{});
                }, std::make_integer_sequence<int, u1 - u0>{});
            }
            __builtin_amdgcn_sched_barrier(0);
        }, std::make_integer_sequence<int, N_SLOTS>{});
        // No vmcnt wait: the pieces this chunk parked were loaded a chunk ago (hipcc waits for them where they are stored), the DMA pieces of
        // the prologue were issued before filter terms this chunk's MFMAs have consumed, and loads return in order.  The barrier publishes the
        // stage and retires this chunk's LDS reads.  A chunk that parks nothing, in a tail where no later chunk parks either, publishes nothing and
        // protects no stage: its LDS reads were waited for where their values were used (WINO_READS_LANDED), and the stage the next chunk reads
        // was published by the last chunk that parked.  Behind the last chunk stands the __syncthreads() of the loop's end.
        if constexpr (do_park) {
            __builtin_amdgcn_s_waitcnt(WINO_WAIT_LGKM0);
            __builtin_amdgcn_s_barrier();
        }
        if constexpr (mode == 0) {
            if (q >= last) return;
            // chunk 1's operands, back to back (stage 0 has landed and was published just now)
            if constexpr (!(POD_WINO_ELIM & 1)) WINO_READ12(WINO_READ, npar, n16, 0);
            WINO_READS_LANDED();
            __builtin_amdgcn_sched_barrier(0);
            make_v(0);
            __builtin_amdgcn_sched_barrier(0);
            if constexpr (!(POD_WINO_ELIM & 1)) WINO_READ12(WINO_READ, npar, n16, 1);
            WINO_READS_LANDED();
            __builtin_amdgcn_sched_barrier(0);
            make_v(1);
            split_all();
            __builtin_amdgcn_sched_barrier(0);
            __builtin_amdgcn_s_barrier();               // chunk 1 parks pieces in stage 0: every wave must have read its operands out of it
        }
    };
    // THE END OF THE LOOP IS PEELED when the chunk count is a multiple of 4 (every count the model runs: C = 64 .. 512 whole or cut into
    // partial sums): the last four chunks then have the static (half, stage) of loop instances 4, 5, 2, 3 and follow the loop as straight-line
    // tail forms that issue nothing for data past the last chunk -- chunk n - 4 loads no stage pieces (super-chunk s + 2 does not exist),
    // n - 3 and n - 2 neither load nor park, n - 1 is the last form.  With 4 chunks only n - 2 and n - 1 are tail forms: chunks 0 and 1 keep
    // their (clamped) stage traffic -- a second instance of either, or a run-time switch inside them, costs registers: 512 and scratch, or 480
    // against 440.  Every other count (1, 2, 3, 5, 6, 7, ...) keeps the clamped path throughout: the same instances, re-loading the last
    // super-chunk and the last chunk's filter terms instead of skipping.  Same arithmetic in the same order either way.
    using std::integral_constant;
    constexpr integral_constant<int, 0> I0{};
    constexpr integral_constant<int, 1> I1{};
    constexpr integral_constant<int, 2> I2{};
    const bool peel = (nchunk & 3) == 0;
    const int nloop = peel ? nchunk - 4 : nchunk;                        // the chunks in front of the tail
    chunk(I0, I0, I0, I0, 0);
    if (nchunk > 1) chunk(I1, I1, I0, I0, 1);
    for (int base = 0;; base += 4) {
#define WINO_CHUNK(t)                                                                                                              \
    if (base + (t) >= nloop) break;                                                                                                \
    chunk(I2, integral_constant<int, (t) & 1>{}, integral_constant<int, ((t) >> 1) & 1>{}, I0, base + (t));
        WINO_CHUNK(2) WINO_CHUNK(3) WINO_CHUNK(4) WINO_CHUNK(5)
#undef WINO_CHUNK
    }
    if (peel) {
        if (nchunk > 4) {
            chunk(I2, I0, I0, integral_constant<int, WINO_TAIL_NO_LOAD>{}, nchunk - 4);
            chunk(I2, I1, I0, integral_constant<int, WINO_TAIL_NO_LOAD | WINO_TAIL_NO_PARK>{}, nchunk - 3);
        }
        chunk(I2, I0, I1, integral_constant<int, WINO_TAIL_NO_LOAD | WINO_TAIL_NO_PARK>{}, nchunk - 2);
        chunk(I2, I1, I1, integral_constant<int, WINO_TAIL_NO_LOAD | WINO_TAIL_NO_PARK | WINO_TAIL_LAST>{}, nchunk - 1);
    }
    __syncthreads();                                   // every wave is done reading the stages, no DMA in flight: they become the output staging
    WINO_STAMP(3);

    if (!wino_output_stage(acc, lds, a, i32, h)) return;
    // the accumulators hold (s_u U) (s_v V) sums: the two powers of two come off again in the store pass -- exactly, inside the
    // fused multiply-add that adds the bias
    const float inv = wino_pow2_inverse(sv) * wino_pow2_inverse(wino_pow2_scale(u_amax, WINO_U_TOP));
    const WinoStore S{set_out + (int64_t)blockIdx.y * P.split_out_stride, set_bias, set_out_amax, inv, set_offset, set_replicas, set_k_planes};
    // abs-max of what this thread stores (-> out_amax: the next convolution's operand scale)
    const float lmax = S.k_planes > 0 ? wino_store_planes(P, B, S, lds, ks) : wino_store_channels_last(P, B, S, lds, ks);
    if (set_out_amax) wino_publish_amax_block(set_out_amax, lmax);          // (set: uniform over the workgroup)
    WINO_STAMP_END();
}

}  // namespace pod

#ifdef POD_TRACE
extern "C" int pod_wino_trace_dump_split(long long* host, int32_t n_workgroups) { return pod::wino_trace_dump(host, n_workgroups); }   // diagnostics build only
#endif

extern "C" int64_t pod_wino_filter_split_bytes(int32_t K, int32_t C) {           // size of Us: the terms + the 16-byte trailer (abs-max word)
    if (K < 1 || C < 16 || (C & 15) != 0) return 0;
    const int64_t Kpad = (K + 63) / 64 * 64;
    return Kpad / 64 * (C / 16) * (int64_t)pod::WINO_US_BYTES + 16;
}

extern "C" int pod_wino_filter_transform_split(const float* weight, void* Us, int32_t K, int32_t C, pod_stream_t stream) {
    if (!weight || !Us || K < 1 || C < 16 || (C & 15) != 0 || !pod_aligned(16, Us)) return POD_E_INVALID;
    const int32_t Kpad = (K + 63) / 64 * 64;
    const int64_t n = (int64_t)Kpad * C;
    float* amax = reinterpret_cast<float*>(reinterpret_cast<char*>(Us) + pod_wino_filter_split_bytes(K, C) - 16);
    if (hipMemsetAsync(amax, 0, 16, (hipStream_t)stream) != hipSuccess) return POD_E_LAUNCH;
    hipLaunchKernelGGL(pod::k_wino_filter_amax, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, weight, amax, K, C, Kpad);
    POD_CHECK_LAUNCH();
    hipLaunchKernelGGL(pod::k_wino_filter_split, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, weight,
                       reinterpret_cast<uint16_t*>(Us), amax, K, C, Kpad);
    POD_CHECK_LAUNCH();
    return POD_OK;
}

// ONE entry for every form of the launch (round 5; rounds 3-4 had a symbol per form): 1..4 convolutions of one shape in one grid, each
// with its own buffers, filter, bias, operand abs-max words, Philox offset, replica count and plane count; or (n_splits > 1) one
// convolution cut over its input channels into partial sums.  See include/pod_mi355x.h: PodWinoConv.
extern "C" int pod_wino_conv3x3_split(const PodWinoConv* d, pod_stream_t stream) {
    if (!d || d->n_sets < 1 || d->n_sets > 4 || !d->blocks || d->n_blocks < 0 || d->C < 16 || (d->C & 15) != 0 || d->K < 64 || (d->K & 63) != 0 ||
        !(d->p >= 0.0f && d->p < 1.0f) || d->sets[0].first_block != 0 || !pod_aligned(16, d->blocks) ||
        d->reserved != 0)
        return POD_E_INVALID;
    const int32_t C = d->C, K = d->K;
    pod::WinoParams P{};
    const int64_t grid = pod::wino_params_launch(P, d->blocks, d->n_blocks, C, K, d->relu, d->p, d->seed, d->epoch);
    if (grid < 0) return POD_E_INVALID;
    const bool partial = d->n_splits > 1;
    if (partial) {
        // whole 32-channel super-chunks (full 128-byte lines) per split; partial sums carry no bias / ReLU / dropout / replicas / planes
        if (d->n_sets != 1 || d->n_splits > 16 || (C / 16) % d->n_splits != 0 || ((C / 16 / d->n_splits) & 1) != 0 || d->split_stride < 0 || (d->split_stride & 3) != 0 ||
            d->p != 0.0f || d->relu || d->sets[0].bias || d->sets[0].replicas || d->sets[0].k_planes || d->sets[0].out_amax)
            return POD_E_INVALID;
    }
    for (int s = 0; s < 4; ++s) {
        const PodConvSet& q = d->sets[s < d->n_sets ? s : 0];
        if (s < d->n_sets) {
            if (!q.in || !q.out || q.in == q.out || !q.Us || !q.in_amax || q.replicas < 0 || q.replicas > 127 || q.k_planes < 0 || q.k_planes > K ||
                (q.k_planes > 0 && (d->p != 0.0f || q.replicas != 0)) || (s > 0 && q.first_block < d->sets[s - 1].first_block) || q.first_block > d->n_blocks)
                return POD_E_INVALID;
            if (!pod_aligned(16, q.in, q.out, q.Us, q.bias) || !pod_aligned(4, q.in_amax, q.out_amax))
                return POD_E_INVALID;
        }
        pod::wino_params_set(P, s, s < d->n_sets ? q.first_block : INT32_MAX, q.in, q.out, q.Us, q.bias, q.in_amax, q.out_amax, q.offset, q.replicas, q.k_planes);
    }
    if (d->n_blocks == 0) return POD_OK;
    if (pod_lds_opt_in<pod::k_wino_conv3x3_split>(pod::WINO_LDS_BYTES) != POD_OK) return POD_E_LAUNCH;
    P.c_split = partial ? C / 16 / d->n_splits : 0; P.split_out_stride = partial ? d->split_stride : 0;
    P.live = d->live_blocks;
    hipLaunchKernelGGL(pod::k_wino_conv3x3_split, dim3((unsigned)grid, partial ? (unsigned)d->n_splits : 1u), dim3(256), pod::WINO_LDS_BYTES, (hipStream_t)stream, P);
    POD_CHECK_LAUNCH();
    return POD_OK;
}
