// The shared home of the Winograd convolution kernels: k11_wino_conv.hip (fp32 MFMA, the reference leg) and k12_wino_conv_split.hip
// (production: every fp32 product formed on the f16 matrix cores from the two-term f16 split of the power-of-two-scaled operands) are
// the same convolution around different inner products.  Here: the parameters and their host-side fill, the LDS geometry, the workgroup
// schedule, the block record and the canvas, the pixel table and the patch fills, the output staging, the dropout mask, the two store
// passes, wait immediates and the diagnostics hooks (the f16 split and the abs-max records: pod_split_gemm.h).  A kernel body
// reads: schedule -> shared prologue -> its OWN filter loads, K loop and transforms -> wino_output_stage -> wino_store_*.
#pragma once
#include "pod_experiments.h"
#include "pod_split_gemm.h"

namespace pod {

constexpr int WINO_U_FLOATS = 24 * 2 * 64 * 4;          // filter slab of a chunk: [24 positions][h][j][4 channels]  48 KB
constexpr int WINO_SB_FLOATS = 384 * 32;                 // raw patch stage of a SUPER-CHUNK (32 input channels): [pixel slot 360 (+24: 48 whole DMA instructions)][8 parts of 16 B], 48 KB
constexpr int WINO_LDS_BYTES = 4 * 32 * 4 * 65 * 4;      // 133 120 B of the CU's 160 KB: the output staging (the K loop needs 24 KB)

// -DPOD_TRACE (diagnostics build, tools/wino_trace.py): s_memtime stamps of every workgroup's phases
#ifdef POD_TRACE
static __device__ long long g_wino_trace[8192 * 16];
#define WINO_STAMP(k)                                                                                          \
    do {                                                                                                       \
        if (threadIdx.x == 0 && blockIdx.x < 8192) g_wino_trace[blockIdx.x * 16 + (k)] = __builtin_readcyclecounter(); \
    } while (0)
#define WINO_STAMP_WALL(k)                                                                                     \
    do {                                                                                                       \
        if (threadIdx.x == 0 && blockIdx.x < 8192) g_wino_trace[blockIdx.x * 16 + (k)] = wall_clock64();       \
    } while (0)
// a kernel's last words: the stores have left, end stamps, where the workgroup ran (XCC / HW id)
#define WINO_STAMP_END()                                                                                       \
    do {                                                                                                       \
        __builtin_amdgcn_s_waitcnt(0);                                                                         \
        WINO_STAMP(5);                                                                                         \
        WINO_STAMP_WALL(13);                                                                                   \
        if (threadIdx.x == 0 && blockIdx.x < 8192) {                                                           \
            uint32_t hw, xcc;                                                                                  \
            asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));                                   \
            asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));                                 \
            g_wino_trace[blockIdx.x * 16 + 6] = ((long long)xcc << 32) | hw;                                   \
        }                                                                                                      \
    } while (0)
// host: this translation unit's stamps (each kernel file exports it under a name of its own; not in include/pod_mi355x.h)
static inline int wino_trace_dump(long long* host, int32_t n_workgroups) {
    if (hipDeviceSynchronize() != hipSuccess) return POD_E_LAUNCH;
    if (n_workgroups > 8192) n_workgroups = 8192;
    if (hipMemcpyFromSymbol(host, HIP_SYMBOL(g_wino_trace), (size_t)n_workgroups * 16 * sizeof(long long)) != hipSuccess) return POD_E_LAUNCH;
    return POD_OK;
}
#else
#define WINO_STAMP(k)
#define WINO_STAMP_WALL(k)
#define WINO_STAMP_END()
#endif

// s_waitcnt immediates (gfx9 encoding: vmcnt[3:0] | expcnt[6:4] | lgkmcnt[11:8] | vmcnt[5:4] << 14): lgkmcnt(0) with vmcnt(4) / vmcnt(0)
constexpr int WINO_WAIT_VM4 = 0x0074, WINO_WAIT_VM0 = 0x0070, WINO_WAIT_VM16 = 0x4070, WINO_WAIT_LGKM0 = 0xC07F;

// One launch = 1..4 convolutions ("sets") of the same shape in one grid -- layer l of the cls- and the bbox-subnet, the four predictors
// (PodWinoConv with n_sets > 1, include/pod_mi355x.h).  Blocks [first[s], first[s + 1]) of the concatenated table belong to set s (its
// records are relative to ITS buffers).  k11 serves one convolution and reads set 0 only.
struct WinoParams {
    const int4* blocks;
    int32_t n_blocks, C, K, KS, in_stride, out_stride, relu;
    uint32_t thresh;
    float scale;
    uint64_t seed;
    // split over the input channels (PodWinoConv with n_splits > 1; small maps: a res5 convolution is 48 workgroups of 32 chunks each):
    // grid.y = C / (16 c_split) workgroup sets, set z accumulates chunks [z c_split, (z + 1) c_split) and stores its partial sums at
    // out + z split_out_stride (channels-last, no bias / ReLU / dropout); pod_wino_reduce adds the partials in a fixed order.  0: no split.
    int32_t c_split;
    int64_t split_out_stride;
    // dropout masks of a REPLAYED launch (HIP graph): the Philox key is seed ^ mix(*epoch), epoch a device word the graph itself bumps
    // at the start of every replay -- seed and offset are launch arguments, i.e. constants of a captured launch.  null: key = seed.
    const uint64_t* epoch;
    // Sparse launch (k15_sparse_blocks.hip): null, or pod_sparse_live_blocks' device list of the LIVE blocks: live[0] = count, then from
    // word POD_SPARSE_LIVE_HEAD one entry of POD_SPARSE_LIVE_STRIDE words each, {record, 11 words of need bits} (include/pod_mi355x.h).
    // Workgroup slot t takes entry t and slots >= live[0] exit at once (the grid is sized for the whole table: the count never visits the host).
    const int32_t* live;
    struct Sets {
        int32_t first[4];         // first block of set s (first[0] = 0; unused sets: INT32_MAX)
        const float* in[4];
        float* out[4];
        const float* U[4];        // k11: fp32 slabs; k12: the pre-split f16 terms + the abs-max trailer
        const float* bias[4];
        const float* in_amax[4];  // device word >= max |in| of the set (the f16 split's operand scale is derived from it)
        float* out_amax[4];       // null, or a device word the store pass max'es with |every value it stores|
        uint64_t offset[4];       // Philox counter of the set's first 8 output floats
        // > 0 (PodWinoConv with replicas; channels-last, one input image per record): the store pass writes that many copies of the image,
        // replica r as image r of the output canvas, each under its own dropout mask -- the mask pod_expand_dropout would draw for it
        int32_t replicas[4];
        int32_t k_planes[4];      // > 0: NCHW planes of k_planes real channels
    } sets;
};

// What lane l3 = pixel slot, q = sub-slot of an LDS-DMA instruction fetches (see the layout in the kernel): per pixel slot 0..383
// (py 18 + px) | rot << 16 (pixel 324: the slot holds no pixel), computed at compile time.
struct WinoSlotTable {
    uint32_t v[384];
    constexpr WinoSlotTable() : v() {
        for (int p = 0; p < 384; ++p) {
            const int cls = p & 1, k = p >> 1, rr = k / 18, px = k - rr * 18;
            const int py = cls ? (rr < 4 ? rr + 4 : rr + 8) : (rr < 4 ? rr : rr < 8 ? rr + 4 : rr + 8);
            const bool ok = cls ? rr < 8 : rr < 10;
            v[p] = ok ? (uint32_t)((py * 18 + px) | ((((px >> 2) & 3) + 4 * ((py >> 1) & 1)) << 16)) : 324u;
        }
    }
};
static __device__ const WinoSlotTable g_wino_slots{};

// Workgroup -> (filter slice ks, block tb).  blockIdx & 7 is the XCD (round-robin dispatch).  An XCD serves TWO of the KS 64-channel
// filter slices (one when KS == 1) for its share of the blocks, and consecutive workgroups of an XCD take the SAME block with its two
// slices: the second one's patch comes out of that XCD's L2 instead of HBM (fp32 kernel, four slices: 2.39 -> 1.68 GB fetched per
// bench launch), while the two slices' filters (3 MB at C = 256) still stay resident in the 4 MB L2.
__device__ __forceinline__ void wino_schedule(int KS, int n_blocks, int& ks, int& tb) {
    const int xcd = blockIdx.x & 7, wi = (int)(blockIdx.x >> 3);
    const int SP = KS >= 2 ? 2 : 1, G = KS / SP;            // slices per XCD; XCD groups with different slice pairs
    ks = SP * (xcd % G) + (wi % SP);
    tb = (wi / SP) * (8 / G) + xcd / G;
}
inline int64_t wino_grid(int KS, int64_t n_blocks) {
    const int SP = KS >= 2 ? 2 : 1, G = KS / SP;
    return 8 * SP * ((n_blocks * G + 7) / 8);
}
// Host: the launch-wide fields of P (the caller value-initialises it and sets c_split / split_out_stride / live where it has them) and
// the grid's x extent; -1: K is not 64 x {1, 2, 4, 8}, or the grid does not fit.
inline int64_t wino_params_launch(WinoParams& P, const int32_t* blocks, int32_t n_blocks, int32_t C, int32_t K, int32_t relu, float p, uint64_t seed,
                                  const uint64_t* epoch) {
    const int32_t KS = K / 64;
    if (KS != 1 && KS != 2 && KS != 4 && KS != 8) return -1;
    P.blocks = reinterpret_cast<const int4*>(blocks);
    P.n_blocks = n_blocks; P.C = C; P.K = K; P.KS = KS; P.in_stride = C; P.out_stride = K; P.relu = relu;
    P.thresh = POD_DROPOUT_THRESH16(p);
    P.scale = 1.0f / (1.0f - p);
    P.seed = seed; P.epoch = epoch;
    const int64_t grid = wino_grid(KS, n_blocks);
    return grid > 0x7FFFFFFFLL ? -1 : grid;
}
inline void wino_params_set(WinoParams& P, int s, int32_t first, const float* in, float* out, const void* U, const float* bias, const float* in_amax,
                            float* out_amax, uint64_t offset, int32_t replicas, int32_t k_planes) {
    P.sets.first[s] = first;
    P.sets.in[s] = in; P.sets.out[s] = out; P.sets.U[s] = reinterpret_cast<const float*>(U); P.sets.bias[s] = bias;
    P.sets.in_amax[s] = in_amax; P.sets.out_amax[s] = out_amax;
    P.sets.offset[s] = offset; P.sets.replicas[s] = replicas; P.sets.k_planes[s] = k_planes;
}

// Ties values into the instruction order at this point (no instruction is emitted): what was computed before cannot sink below, what
// is computed from them cannot rise above.
template <typename T>
__device__ __forceinline__ void wino_pin_one(T& v) {
    asm volatile("" : "+v"(v));
}
template <typename... T>
__device__ __forceinline__ void wino_pin(T&... v) {
    (wino_pin_one(v), ...);
}

// ---- the filter transform U = G4 g G6t of one (k, c) pair (4 x 6 positions: F(2,3) down the rows, F(4,3) along the columns),
//   G4 = [[1,0,0],[.5,.5,.5],[.5,-.5,.5],[0,0,1]],  G6 = [[1/4,0,0],[-1/6,-1/6,-1/6],[-1/6,1/6,-1/6],[1/24,1/12,1/6],[1/24,-1/12,1/6],[0,0,1]];
// output channels >= K are zero
__device__ __forceinline__ void wino_filter_values(const float* __restrict__ w, int k, int c, int K, int C, float (&u)[4][6]) {
    float g[3][3];
#pragma unroll
    for (int i = 0; i < 9; ++i) g[i / 3][i % 3] = k < K ? w[((int64_t)k * C + c) * 9 + i] : 0.0f;
    float t0[4][3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        t0[0][j] = g[0][j];
        t0[1][j] = 0.5f * (g[0][j] + g[1][j] + g[2][j]);
        t0[2][j] = 0.5f * (g[0][j] - g[1][j] + g[2][j]);
        t0[3][j] = g[2][j];
    }
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        const float x0 = t0[a][0], x1 = t0[a][1], x2 = t0[a][2];
        u[a][0] = 0.25f * x0;
        u[a][1] = (-1.0f / 6.0f) * (x0 + x1 + x2);
        u[a][2] = (-1.0f / 6.0f) * (x0 - x1 + x2);
        u[a][3] = (1.0f / 24.0f) * x0 + (1.0f / 12.0f) * x1 + (1.0f / 6.0f) * x2;
        u[a][4] = (1.0f / 24.0f) * x0 - (1.0f / 12.0f) * x1 + (1.0f / 6.0f) * x2;
        u[a][5] = x2;
    }
}

// ==== What the two convolution kernels share around their K loops ====================================================================
//
//   Y = At2 [ (G4 g G6^T) . (Bt4 d Bt6^T) ] At4^T     d: 4x6 input patch, g: 3x3 filter, Y: 2x4 outputs, "." summed over c
//
// Tiles are 2 rows x 4 columns of outputs (F(2,3) down the rows: 4 patch rows; F(4,3) along the columns: 6 patch columns), 24 Winograd
// positions per tile and (c, k) pair where the direct convolution has 72 multiply-adds.  A workgroup (256 threads, one wavefront per
// SIMD) computes a 16x16-pixel block = 8 x 4 = 32 tiles = one MFMA block of rows, for 64 output channels.  Wavefront `a` owns ROW a of the
// 4 x 6 position grid (positions 6a .. 6a+5) for the 32 tiles and all 64 output channels (two 32-channel blocks, kb): 6 x 2 = 12 MFMA
// blocks = 192 accumulators.  Row a of Bt4 d is one sum or difference of two patch rows (wino_rows), followed by the 6-point column
// transform Bt6; every transformed value feeds two MFMAs (kb).  Filter operands never touch LDS (L2 -> registers, each kernel in its own
// layout); the raw 18x18-pixel patch goes global -> LDS and is read from there, no transformed copy exists anywhere.
//
// CANVAS.  Activations are channels-last [pixel][C] fp32.  The images of a (level, launch) stand in a GRID on a virtual canvas, image i
// at grid cell (i / gcols, i % gcols), top-left canvas pixel (row (H + 1), col (W + 1)): one zero row / column between neighbours is the
// convolution's padding for both (reads outside an image return 0.0), and 16x16 blocks are cut from the canvas without regard to image
// boundaries -- the partial blocks at the right and bottom edges are paid once per level instead of once per image.  A table of block
// records (int4 {first pixel of image 0 in `in`, in `out`, gcols << 24 | H << 12 | W, n_images << 24 | by << 12 | bx}) says where.
struct WinoBlock {
    int64_t base_px, out_px;              // first pixel of image 0 in `in` / `out`
    int gcols, H, W, n_img, y0, x0, Hv, Wv, HWi;
    float rHv, rWv;
};
__device__ __forceinline__ WinoBlock wino_block(const int4 desc) {
    WinoBlock B;
    B.base_px = desc.x; B.out_px = desc.y;
    B.gcols = (desc.z >> 24) & 0xFF; B.H = (desc.z >> 12) & 0xFFF; B.W = desc.z & 0xFFF; B.n_img = (desc.w >> 24) & 0xFF;
    B.y0 = ((desc.w >> 12) & 0xFFF) * 16; B.x0 = (desc.w & 0xFFF) * 16; B.Wv = B.W + 1; B.Hv = B.H + 1; B.HWi = B.H * B.W;
    B.rWv = 1.0f / (float)B.Wv; B.rHv = 1.0f / (float)B.Hv;
    return B;
}
// canvas coordinate v >= 0 -> (grid index, coordinate inside the cell); canvas extents < 2^16: exact after the fix-up
__device__ __forceinline__ int wino_cell(int v, int step, float rstep, int& idx) {
    int n = (int)((float)v * rstep);
    n -= n * step > v ? 1 : 0;
    n += (n + 1) * step <= v ? 1 : 0;
    idx = n;
    return v - n * step;
}

// Row a of Bt4 d = x[row0] + sgn x[row1], wave-uniform:   a = 0: d0 - d2      a = 1: d1 + d2      a = 2: d2 - d1      a = 3: d1 - d3
__device__ __forceinline__ void wino_rows(int a, int& row0, int& row1, float& sgn) {
    row0 = a == 0 ? 0 : a == 2 ? 2 : 1;
    row1 = a == 2 ? 1 : a == 3 ? 3 : 2;
    sgn = a == 1 ? 1.0f : -1.0f;
}

// PATCH IN LDS, one stage (WINO_SB_FLOATS; two of them) per SUPER-CHUNK of 32 input channels = the 128-byte line a pixel owns in the
// channels-last source: [pixel slot][8 parts of 16 B], so that 8 consecutive lanes of an LDS-DMA instruction fetch ONE full line
// (measured, profiles/r03_experiments.md: a pixel per lane -- 64 lines per instruction, each line fetched again by the next three
// 8-channel chunks -- stalls the in-order instruction streams by ~400 cycles per chunk once the lines come from HBM; full lines cost 55).
// Pixel slot of patch pixel (py, px): 2 (rank(py) 18 + px) + ((py >> 2) & 1), rank = (py & 3) + 4 (py >> 3) (rows 0-3, 8-11, 16, 17
// on the even slots, rows 4-7, 12-15 on the odd ones); part P of that pixel sits at sub-slot (P + rot) & 7,
// rot = ((px >> 2) & 3) + 4 ((py >> 1) & 1): the 16 lanes a ds_read_b128 serves per LDS cycle (4 tile rows x 4 tile columns,
// one part) then hit 16 different 16-byte bank groups -- conflict-free for every (row, column, chunk).
// (The kernels keep their tables of these addresses themselves, `areg` / `amini`: a lane of k11 reads the 4 chunks of a super-chunk in
// 4-channel parts, a lane of k12 its 2 x 2 halves.)
// The first 16 input channels come from two MINI stages behind the two stages (8 channels each, 324 pixels x 32 B, 3 LDS-DMA
// instructions per wave each), so the matrix cores start after 20 KB have landed instead of a 48 KB super-chunk; super-chunk 0 lands
// behind the first MFMAs.  Mini layout: 16-byte slot 2 (py 21 + (px & 3) 5 + (px >> 2)) + half: the 16 lanes of a ds_read_b128 group hit
// every bank group twice.  Behind the mini stages: the pixel table.
//
// Where a patch pixel lives in the source: thread t works out pixel t (and t + 256) of the 18 x 18 patch ONCE -- canvas row -> (grid
// row, row inside the image), canvas column -> (grid column, column) -- and parks its pixel index in LDS (-1: outside every image, or a
// pixel whose need bit is off (sparse launches; need[i]: the bits of pixels t = tid + 256 i): the loads then use a buffer offset past the
// resource, which reads 0.0 -- that IS the zero padding of the convolution); the lanes look their pieces up there: two divisions per
// thread instead of two per lane and piece.  WINO_FILL_PIXEL_TABLE fills the table and publishes it (a barrier).
__device__ __forceinline__ int* wino_pixel_table(float* lds) { return reinterpret_cast<int*>(lds + 2 * WINO_SB_FLOATS + 2 * 3072); }
// (A statement macro, like WINO_FILL_SLOTS below: as functions the two are simplified on their own before they are inlined -- without
// the kernel's bound on threadIdx and with their arguments in place of the kernel's values -- and come out as different, if equivalent,
// integer arithmetic, which reschedules the prologue of k12's hand-pinned instruction stream.  tid: the thread index.)
#define WINO_FILL_PIXEL_TABLE(pix_tab, B, need, tid)                                                                                  \
    _Pragma("unroll") for (int it_ = 0; it_ < 2; ++it_) {                                                                             \
        const int t = (tid) + 256 * it_;                                                                                              \
        if (t >= 325) break;                                                                                                          \
        const int py = t / 18, px = t - py * 18, vy = (B).y0 - 1 + py, vx = (B).x0 - 1 + px;                                          \
        int m, n;                                                                                                                     \
        const int gy = wino_cell(vy < 0 ? 0 : vy, (B).Hv, (B).rHv, m), gx = wino_cell(vx < 0 ? 0 : vx, (B).Wv, (B).rWv, n), img = m * (B).gcols + n; \
        const bool ok = (t < 324) & (vy >= 0) & (gy < (B).H) & (vx >= 0) & (gx < (B).W) & (n < (B).gcols) & (img < (B).n_img) & ((((need)[it_] >> (t & 31)) & 1u) != 0); \
        (pix_tab)[t] = ok ? img * (B).HWi + gy * (B).W + gx : -1;      /* entry 324 = -1: the "no pixel" slots of the fills point here */ \
    }                                                                                                                                 \
    __syncthreads();                                                                                                                  \
    WINO_STAMP(8)                                      /* (the block record has arrived, the pixel table stands) */

// The fills of a lane.  LDS-DMA of a stage: 48 instructions of 8 pixel slots x 8 parts (the last 3 fetch nothing), wave a issues
// 12 a .. 12 a + 11.  Lane (l3 = lane >> 3, q = lane & 7) of instruction I fills sub-slot q of pixel slot 8 I + l3 with part
// (q - rot) & 7 of its pixel.  The buffer resource (the record's images, from the first channel the workgroup reads) is the caller's.
// What does not depend on the block record -- slot_e: the lane's 12 pixel slots of a stage fill, patch pixel | rot << 16 (a constant
// table: asked for first, so that nothing queues behind the patch loads that follow); mini_pidx: the patch pixel of its 3 slots of a
// mini-stage fill (324: none).
#define WINO_FILL_SLOTS(slot_e, mini_pidx, tid)                                                                                       \
    _Pragma("unroll") for (int i = 0; i < 12; ++i) (slot_e)[i] = g_wino_slots.v[96 * ((tid) >> 6) + 8 * i + (((tid) & 63) >> 3)];     \
    _Pragma("unroll") for (int r = 0; r < 3; ++r) {                                                                                   \
        const int pp = ((((tid) >> 6) * 3 + r) * 64 + ((tid) & 63)) >> 1, py = pp / 21, pi = pp - py * 21, px = 4 * (pi % 5) + pi / 5; \
        (mini_pidx)[r] = py < 18 && pi < 20 && px < 18 ? py * 18 + px : 324;                                                          \
    }
// pixel index of the table -> byte offset of its 4-float part in the source.  (P by pointer, not by reference, on purpose: behind a
// reference the load of in_stride is known to be safe, the compiler then turns the branch into a select, and k12's prologue comes out
// in another order than the one its instruction stream was measured with.)
__device__ __forceinline__ int wino_byte_offset(const WinoParams* P, int pix, int part4) {
    return pix >= 0 ? (pix * P->in_stride + part4) * 4 : 0x7FFFFF00;
}
__device__ __forceinline__ void wino_mini_offsets(const WinoParams* P, const int* pix_tab, const int (&mini_pidx)[3], int (&dmini)[3], int lane) {
#pragma unroll
    for (int r = 0; r < 3; ++r) dmini[r] = pix_tab[mini_pidx[r]];
#pragma unroll
    for (int r = 0; r < 3; ++r) dmini[r] = wino_byte_offset(P, dmini[r], 4 * (lane & 1));
}
// (the 12 offsets of a stage fill, doff[i] = wino_byte_offset(P, pix_tab[slot_e[i] & 0xFFFF], 4 (((lane & 7) - (slot_e[i] >> 16)) & 7)),
// are a lambda of each kernel, defined here and called behind the first loads: every shared form of it reorders k12's prologue)
typedef __attribute__((address_space(3))) void wino_lds_void;
// wave a's piece r (1 KB) of the 8-channel patch `which` (0 / 1) into its mini stage
__device__ __forceinline__ void wino_mini_piece(__amdgpu_buffer_rsrc_t rsrc, float* lds, int a, int which, int r, int dmini_r) {
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, (wino_lds_void*)(lds + 2 * WINO_SB_FLOATS + which * 3072 + (a * 3 + r) * 256), 16, dmini_r, which * 32, 0, 0);
}
// wave a's piece i (1 KB: 8 pixels x 32 channels) of super-chunk sc, straight into LDS
__device__ __forceinline__ void wino_patch_piece(__amdgpu_buffer_rsrc_t rsrc, float* stage, int a, int sc, int i, int doff_i) {
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, (wino_lds_void*)(stage + (a * 12 + i) * 256), 16, doff_i, sc * 128, 0, 0);
}

// OUTPUT TRANSFORM Y = At2 M At4^T, At2 = [[1,1,1,0],[0,1,-1,-1]], At4 = [[1,1,1,1,1,0],[0,1,-1,2,-2,0],[0,1,1,4,4,0],[0,1,-1,8,-8,1]].
// Every wave applies At4 to its row of 6 positions in registers (4 output columns) and parks Z[a][tile][column][channel] in LDS (the
// stages have been read out: they become the staging); the store pass combines the four rows in a fixed order:
// Y[0][x] = (Z[0][x] + Z[1][x]) + Z[2][x],  Y[1][x] = (Z[1][x] - Z[2][x]) - Z[3][x].
// The MFMAs run with the FILTER as the row operand: a lane's accumulator register reg of block (p, kb) is channel
// 32 kb + (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5) of tile lane & 31 -- four consecutive channels per register quad, so the
// transform runs on packed pairs and a 16-byte store parks 4 channels.  Staging: Z[a][tile][column e][64 channels], a tile's 4 x 64
// floats + 4 pad (1040 B: the 8 tiles of a store's lane group hit 8 different 16-byte bank groups), 4 x 32 x 1040 B = WINO_LDS_BYTES.
constexpr int WINO_TS = 260;               // floats per (a, tile)
constexpr int WINO_ZA = 32 * WINO_TS;      // floats per position row a
// -> false: an elimination build (POD_WINO_ELIM & 128 / & 32) that ends here
__device__ __forceinline__ bool wino_output_stage(const f32x16 (&acc)[12], float* lds, int a, int i32, int h) {
    if (POD_WINO_ELIM & 128) {
#pragma unroll
        for (int i = 0; i < 12; ++i) asm volatile("" ::"v"(acc[i]));
        return false;
    }
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            f32x4 m[6];
#pragma unroll
            for (int p6 = 0; p6 < 6; ++p6) m[p6] = f32x4{acc[p6 * 2 + kb][4 * g], acc[p6 * 2 + kb][4 * g + 1], acc[p6 * 2 + kb][4 * g + 2], acc[p6 * 2 + kb][4 * g + 3]};
            const f32x4 s1 = m[1] + m[2], d1 = m[1] - m[2], s2 = m[3] + m[4], d2 = m[3] - m[4];
            float* o = lds + (a * 32 + i32) * WINO_TS + kb * 32 + 8 * g + 4 * h;
            *reinterpret_cast<f32x4*>(o) = (m[0] + s1) + s2;
            *reinterpret_cast<f32x4*>(o + 64) = __builtin_elementwise_fma(f32x4{2.f, 2.f, 2.f, 2.f}, d2, d1);
            *reinterpret_cast<f32x4*>(o + 128) = __builtin_elementwise_fma(f32x4{4.f, 4.f, 4.f, 4.f}, s2, s1);
            *reinterpret_cast<f32x4*>(o + 192) = __builtin_elementwise_fma(f32x4{8.f, 8.f, 8.f, 8.f}, d2, d1) + m[5];
        }
    __syncthreads();
    WINO_STAMP(4);
    return !(POD_WINO_ELIM & 32);
}

// STORE PASSES: staging -> y = (row combination) * inv + bias -> ReLU -> dropout -> memory.
struct WinoStore {
    float* out;               // of the workgroup's set (and input-channel split)
    const float* bias;        // null: none
    float* out_amax;          // null, or: the pass returns the abs-max of what the thread stores (the caller publishes it)
    float inv;                // what takes the operand scales of the f16 split off again -- a power of two, exact inside the fma; 1: fp32 operands
    uint64_t offset;          // Philox counter of the set's first 8 floats
    int replicas, k_planes;
};
// Dropout of the 8 consecutive floats at e (a multiple of 8): ONE Philox call for the two quads (pod_device.h: the mask rule) --
// pod_bias_act's mask with counter word 0, pod_expand_dropout's (the replicas) with word 2.
__device__ __forceinline__ void wino_dropout8(f32x4& v0, f32x4& v1, int64_t e, uint64_t offset, uint32_t word, uint64_t key, uint32_t thresh, float scale) {
    const uint64_t ctr = offset + (uint64_t)(e >> 3);
    const u32x4 r4 = philox4x32_10(u32x4{(uint32_t)ctr, (uint32_t)(ctr >> 32), word, STREAM_DROPOUT}, (uint32_t)key, (uint32_t)(key >> 32));
    dropout_mask4(v0, r4.x, r4.y, thresh, scale);
    dropout_mask4(v1, r4.z, r4.w, thresh, scale);
}

// Both store passes take the launch's uniform decisions (ReLU, dropout, abs-max record) ONCE, as template parameters behind one dispatch,
// and keep their loops straight-line: a thread's arithmetic and Philox calls run for every row, valid or not, only the stores and the
// abs-max contribution are predicated; the row combination takes the parity as an operand (x - y == fma(-1, y, x), one rounding either
// way); addresses are stepped, not rebuilt.  (Measured on the ISA of the form before: one exec region and 9 integer multiplies per row,
// the four Philox chains of a batch one behind the other, ~1 100 instructions per trip of the layers-2-4 form: profiles/store_pass_ab.md.)

// NCHW planes (the predictors: the layout K1 streams): thread -> (channel, row of the block, 4 pixels along x = one tile's columns);
// 64-byte runs per (channel, row).  No dropout, no replicas.  Wave w serves channels ks 64 + 4 it + w, it = 0..15, in batches of four
// (the 48 LDS reads of a batch in one round trip); lane `it` of the wave holds iteration it's bias -- one load in front of the loop,
// nothing in the loop waits on vmcnt behind its own stores.  Iterations past k_planes (the last batch) compute and store nothing.
template <bool RELU, bool AMAX>
__device__ __forceinline__ float wino_store_planes_form(const WinoBlock& B, const WinoStore& S, const float* lds, int ks) {
    const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    float lmax = 0.0f;
    const f32x4 inv = f32x4{S.inv, S.inv, S.inv, S.inv};
    const int oy = (tid >> 2) & 15, ox = (tid & 3) * 4, odd = oy & 1;
    const float sg = odd ? -1.0f : 1.0f;
    const int kg0 = ks * 64 + wave;
    const int n_it = (S.k_planes - kg0 + 3) >> 2;     // channels kg0 + 4 it < k_planes: it < n_it
    const float bias_l = S.bias ? S.bias[kg0 + 4 * (tid & 15)] : 0.0f;
    int m;
    const int gy = wino_cell(B.y0 + oy, B.Hv, B.rHv, m);
    int64_t px0[4];                                   // output pixel (of plane 0) per column, -1: not a pixel of any image
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        int n;
        const int gx = wino_cell(B.x0 + ox + e, B.Wv, B.rWv, n), img = m * B.gcols + n;
        px0[e] = (n < B.gcols && img < B.n_img && gx < B.W && gy < B.H) ? (B.out_px + (int64_t)img * B.HWi) * S.k_planes + (int64_t)gy * B.W + gx : -1;
    }
    const bool vec = px0[0] >= 0 && px0[3] == px0[0] + 3 && (px0[0] & 3) == 0 && (B.HWi & 3) == 0;
    const bool ok[4] = {px0[0] >= 0, px0[1] >= 0, px0[2] >= 0, px0[3] >= 0};
    int64_t q[4];                                     // the thread's 4 pixels in the plane of the batch's first channel: + 4 planes per iteration
#pragma unroll
    for (int e = 0; e < 4; ++e) q[e] = (int64_t)kg0 * B.HWi + px0[e];
    const int64_t q_it = (int64_t)4 * B.HWi;
    const int tile = (oy >> 1) * 4 + (tid & 3);
    const float* r = lds + tile * WINO_TS + wave + (odd ? WINO_ZA : 0);     // Z[a][tile][e][k] at + a WINO_ZA + 64 e: rows a = odd .. odd + 2
#pragma unroll 1
    for (int it0 = 0; it0 < 16 && it0 < n_it; it0 += 4, r += 16) {
        float z[4][4][3];
        f32x4 v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int a = 0; a < 3; ++a) z[j][e][a] = r[4 * j + e * 64 + a * WINO_ZA];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float bias = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, bias_l), it0 + j));
            f32x4 y;
#pragma unroll
            for (int e = 0; e < 4; ++e) y[e] = __builtin_fmaf(sg, z[j][e][2], __builtin_fmaf(sg, z[j][e][1], z[j][e][0]));      // even rows (Z0 + Z1) + Z2, odd rows (Z1 - Z2) - Z3
            v[j] = __builtin_elementwise_fma(y, inv, f32x4{bias, bias, bias, bias});
            if (RELU) wino_relu4(v[j]);
            if (AMAX) {
                const float mx = wino_absmax4(0.0f, f32x4{ok[0] ? v[j].x : 0.f, ok[1] ? v[j].y : 0.f, ok[2] ? v[j].z : 0.f, ok[3] ? v[j].w : 0.f});
                lmax = fmaxf(lmax, it0 + j < n_it ? mx : 0.0f);
            }
        }
        wino_pin(v[0], v[1], v[2], v[3]);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const bool live = it0 + j < n_it;
            if (live && vec) {
                *reinterpret_cast<f32x4*>(S.out + q[0]) = v[j];
            } else if (live) {
                if (ok[0]) S.out[q[0]] = v[j].x;
                if (ok[1]) S.out[q[1]] = v[j].y;
                if (ok[2]) S.out[q[2]] = v[j].z;
                if (ok[3]) S.out[q[3]] = v[j].w;
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) q[e] += q_it;
        }
    }
    return lmax;
}
// (The abs-max forms: wino.py never asks a planes launch for a record, but PodWinoConv accepts out_amax with k_planes > 0 and that stays
// served -- tests/wino_store_pass covers it through a grouped launch.)
__device__ __forceinline__ float wino_store_planes(const WinoParams& P, const WinoBlock& B, const WinoStore& S, const float* lds, int ks) {
    switch ((P.relu ? 1 : 0) | (S.out_amax ? 2 : 0)) {
        case 0: return wino_store_planes_form<false, false>(B, S, lds, ks);
        case 1: return wino_store_planes_form<true, false>(B, S, lds, ks);
        case 2: return wino_store_planes_form<false, true>(B, S, lds, ks);
        default: return wino_store_planes_form<true, true>(B, S, lds, ks);
    }
}

// Channels-last: thread -> 8 consecutive channels (one Philox call) of one pixel column, rows of one parity (canvas rows y0 + odd + 2 i,
// i = 0..7).  The element offset e of a row is the one of the row before + 2 W out_stride, + (gcols HWi - Hv W) out_stride when the row
// leaves its image for the one below (Hv >= 2: at most once per step); the Philox counter stays offset + (e >> 3).
// The replica form (S.replicas > 0: the first conv of an MC-dropout subnet; its output is the same for every run, so the pass writes the
// runs' masked replicas itself, replica r = image r of the output canvas under the mask pod_expand_dropout draws for it) is the same
// loop run S.replicas times over a batch's values, e stepping by one image: four Philox chains in flight there too.
template <bool RELU, bool DROP>
__device__ __forceinline__ float wino_store_channels_last_form(const WinoParams& P, const WinoBlock& B, const WinoStore& S, const float* lds, int ks) {
    const int tid = threadIdx.x;
    float lmax = 0.0f;
    const f32x4 inv = f32x4{S.inv, S.inv, S.inv, S.inv};
    const int k8 = (tid & 7) * 8, kg = ks * 64 + k8, ox = (tid >> 3) & 15, odd = tid >> 7;
    const float sg1 = odd ? -1.0f : 1.0f;
    const f32x4 sg = f32x4{sg1, sg1, sg1, sg1};
    f32x4 bias0 = f32x4{0.f, 0.f, 0.f, 0.f}, bias1 = bias0;
    if (S.bias) {
        bias0 = *reinterpret_cast<const f32x4*>(S.bias + kg);
        bias1 = *reinterpret_cast<const f32x4*>(S.bias + kg + 4);
    }
    const uint64_t drop_key = DROP ? dropout_key(P.seed, P.epoch) : 0ull;
    const int n_rep = S.replicas > 0 ? S.replicas : 1;                           // (0: an ordinary launch; 1: one "replica" under the replicas' mask)
    const uint32_t word = S.replicas > 0 ? 2u : 0u;
    int n, m;
    const int gx = wino_cell(B.x0 + ox, B.Wv, B.rWv, n);
    const bool col_ok = n < B.gcols && gx < B.W;
    int gy = wino_cell(B.y0 + odd, B.Hv, B.rHv, m);                              // grid row m, image row gy (H: the separator)
    int img = m * B.gcols + n;
    const int64_t e_row = (int64_t)(2 * B.W) * P.out_stride, e_wrap = ((int64_t)B.gcols * B.HWi - (int64_t)B.Hv * B.W) * P.out_stride, e_rep = (int64_t)B.HWi * P.out_stride;
    int64_t e = (B.out_px + (int64_t)img * B.HWi + (int64_t)gy * B.W + gx) * P.out_stride + kg - e_row;      // a multiple of 8; one row up: every row steps first
    gy -= 2;
    const float* rbase = lds + (ox >> 2) * WINO_TS + (ox & 3) * 64 + k8 + (odd ? WINO_ZA : 0);      // Z[a][tile][ox & 3][k8] of row a = odd
    // Rows in BATCHES of four: the 24 LDS reads of a batch are issued together (one round trip), then the four rows' arithmetic and
    // Philox calls run as independent, interleaved chains; the values are pinned in front of the stores, so that nothing but the
    // stores sits under a row's exec mask.
#pragma unroll 1
    for (int g = 0; g < 2; ++g) {
        f32x4 z[4][6], v[4][2];
        bool ok[4];
        int64_t er[4];
#pragma unroll
        for (int it = 0; it < 4; ++it) {
            gy += 2;
            const bool wrap = gy >= B.Hv;
            gy -= wrap ? B.Hv : 0;
            img += wrap ? B.gcols : 0;
            e += e_row + (wrap ? e_wrap : 0);
            ok[it] = col_ok && gy < B.H && img < B.n_img;
            er[it] = e;
            const float* r = rbase + (4 * g + it) * 4 * WINO_TS;                          // tile (4 g + it, ox >> 2)
            z[it][0] = *reinterpret_cast<const f32x4*>(r); z[it][1] = *reinterpret_cast<const f32x4*>(r + 4);
            z[it][2] = *reinterpret_cast<const f32x4*>(r + WINO_ZA); z[it][3] = *reinterpret_cast<const f32x4*>(r + WINO_ZA + 4);
            z[it][4] = *reinterpret_cast<const f32x4*>(r + 2 * WINO_ZA); z[it][5] = *reinterpret_cast<const f32x4*>(r + 2 * WINO_ZA + 4);
        }
#pragma unroll
        for (int it = 0; it < 4; ++it) {                                 // even rows (Z0 + Z1) + Z2, odd rows (Z1 - Z2) - Z3
            v[it][0] = __builtin_elementwise_fma(__builtin_elementwise_fma(sg, z[it][4], __builtin_elementwise_fma(sg, z[it][2], z[it][0])), inv, bias0);
            v[it][1] = __builtin_elementwise_fma(__builtin_elementwise_fma(sg, z[it][5], __builtin_elementwise_fma(sg, z[it][3], z[it][1])), inv, bias1);
            if (RELU) {
                wino_relu4(v[it][0]);
                wino_relu4(v[it][1]);
            }
            // (a masked value is 0 or v * scale: v * scale bounds both, whatever the masks)
            // (computed whether or not the launch keeps a record -- a dozen instructions per row, no form of its own: K11, which has no
            // record, never uses the result and the compiler drops it there; K12 publishes it only when S.out_amax is set)
            const float mx = wino_absmax4(wino_absmax4(0.0f, v[it][0]), v[it][1]);
            lmax = fmaxf(lmax, ok[it] ? (DROP ? mx * P.scale : mx) : 0.0f);
        }
#pragma unroll 1
        for (int rep = 0; rep < n_rep; ++rep) {
            f32x4 w[4][2];
#pragma unroll
            for (int it = 0; it < 4; ++it) {
                w[it][0] = v[it][0];
                w[it][1] = v[it][1];
                if (DROP && !(POD_WINO_ELIM & 64)) wino_dropout8(w[it][0], w[it][1], er[it], S.offset, word, drop_key, P.thresh, P.scale);
            }
#pragma unroll
            for (int it = 0; it < 4; ++it) wino_pin(w[it][0], w[it][1]);
#pragma unroll
            for (int it = 0; it < 4; ++it) {
                if (ok[it]) {
                    *reinterpret_cast<f32x4*>(S.out + er[it]) = w[it][0];
                    *reinterpret_cast<f32x4*>(S.out + er[it] + 4) = w[it][1];
                }
                er[it] += e_rep;
            }
        }
    }
    return lmax;
}
__device__ __forceinline__ float wino_store_channels_last(const WinoParams& P, const WinoBlock& B, const WinoStore& S, const float* lds, int ks) {
    switch ((P.relu ? 1 : 0) | (P.thresh ? 2 : 0)) {
        case 0: return wino_store_channels_last_form<false, false>(P, B, S, lds, ks);
        case 1: return wino_store_channels_last_form<true, false>(P, B, S, lds, ks);
        case 2: return wino_store_channels_last_form<false, true>(P, B, S, lds, ks);
        default: return wino_store_channels_last_form<true, true>(P, B, S, lds, ks);
    }
}

}  // namespace pod
