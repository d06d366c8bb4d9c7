// Implicit-GEMM convolution on gfx950 fp32 MFMA (see gemm_conv.h).
//
// Workgroup = 256 threads = 4 waves; block tile BM x 128 (BM = 32, 64, 96 or 128), K step 16,
// LDS double buffer, global->register prefetch of tile k+1 while tile k feeds the matrix cores.
// Both operands sit in LDS k-major ([16][BM], [16][128]) so that a 32x32x2 MFMA fragment
// (lane l: row/col l&31, k = l>>5) is one conflict-free ds_read_b32 per operand.
// Arithmetic is exact fp32 (v_mfma_f32_32x32x2_f32 == k-ordered fmaf chain): the <=1e-4 parity
// target against the fp32 CPU reference leaves no room for bf16 operands.
#include "gemm_tile.h"

namespace mi {

// LFLAGS: the MI_FLAG_GELU/SCALE/RES bits of a LINEAR epilogue as compile-time constants (runtime flag branches
// inside the unrolled epilogue made hipcc copy all 64 accumulators to VGPRs at once: 204 registers, 2 waves/SIMD)
template <int WM, int WN, int TM, int TN, int EPI, int LFLAGS, bool PLAIN>
__global__ __launch_bounds__(256, (TM * TN == 4 ? 3 : 4)) void conv_gemm_kernel(const mi_conv_desc d, const int N, const int MT, const int Gm) {
    constexpr int BM = WM * TM * 32;
    static_assert(WN * TN * 32 == BN, "block N tile is 128");
    static_assert(WM * WN == 4, "4 waves");
    __shared__ float As[2][BK][BM];
    __shared__ float Bs[2][BK][BN];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WN, wn = wave % WN;
    int mt, nt;
    if (!tile_of_block(MT, Gm, N, mt, nt)) return;      // grid padding (whole workgroup, before any barrier)
    const int m0 = mt * BM, n0 = nt * BN;
    const int P = d.O1 * d.O2;

    // ---- A loader: BK x BM floats as float4, thread-linear ---------------------------------------
    constexpr int A_F4 = BK * BM / 4, A_FULL = A_F4 / 256, A_REM = A_F4 % 256;
    constexpr int A_SLOTS = A_FULL + (A_REM ? 1 : 0);
    static_assert(A_SLOTS <= 2, "A tile fits two float4 per thread");
    const int aidx0 = tid < A_F4 ? tid : 0, aidx1 = (tid + 256 < A_F4) ? tid + 256 : 0;
    const int ar0 = aidx0 / (BM / 4), ac0 = (aidx0 % (BM / 4)) * 4;
    const int ar1 = aidx1 / (BM / 4), ac1 = (aidx1 % (BM / 4)) * 4;
    const bool a_on0 = tid < A_F4, a_on1 = tid + 256 < A_F4;
    const float *ap0 = d.wt + (size_t)ar0 * d.Mpad + m0 + ac0;
    const float *ap1 = d.wt + (size_t)ar1 * d.Mpad + m0 + ac1;
    const size_t a_step = (size_t)BK * d.Mpad;

    // ---- B loader ----------------------------------------------------------------------------------
    // generic: this thread owns column (tid & 127), rows khalf + 2*j;  plain: 4 columns x rows r, r + 8
    const int khalf = wave >> 1;
    const int o2v = d.o2_valid ? d.o2_valid : d.O2;
    const ColInfo lc = decompose(n0 + (PLAIN ? (tid & 31) * 4 : (tid & 127)), N, P, d.O2, PLAIN ? d.O2 : o2v);
    const int i1b = lc.o1 * d.S1, i2b = lc.o2 * d.S2;
    const float *xcol = d.x + (size_t)lc.b * d.x_bstride + (PLAIN ? (size_t)lc.p : (size_t)i1b * (d.x_ld ? d.x_ld : d.D2) + i2b);
    const int prow = tid >> 5;                                   // plain: first row of this thread
    const float *bp0 = lc.valid ? xcol + (size_t)prow * P : d.x; // plain row pointers (channel stride = P)
    const float *bp1 = lc.valid ? xcol + (size_t)(prow + 8) * P : d.x;
    const size_t b_step = lc.valid ? (size_t)BK * P : 0;

    float4 areg0 = make_float4(0.f, 0.f, 0.f, 0.f), areg1 = areg0, bq0 = areg0, bq1 = areg0;
    float breg[8];
    bool bok[8];

#define MI_LOAD_TILE(kt)                                                                              \
    do {                                                                                              \
        if (PLAIN) {                                                                                  \
            bq0 = *reinterpret_cast<const float4 *>(bp0 + (size_t)(kt) * b_step);                     \
            bq1 = *reinterpret_cast<const float4 *>(bp1 + (size_t)(kt) * b_step);                     \
        } else {                                                                                      \
            mi_ktab_entry ke[8];                                                                      \
            _Pragma("unroll") for (int j = 0; j < 8; ++j) ke[j] = d.ktab[(kt) * BK + khalf + 2 * j];   \
            _Pragma("unroll") for (int j = 0; j < 8; ++j)                                              \
                breg[j] = gather_b(d, ke[j], xcol, i1b, i2b, lc.valid, bok[j]);                        \
        }                                                                                             \
        if (A_SLOTS >= 1) areg0 = *reinterpret_cast<const float4 *>(ap0 + (size_t)(kt) * a_step);     \
        if (A_SLOTS >= 2) areg1 = *reinterpret_cast<const float4 *>(ap1 + (size_t)(kt) * a_step);     \
    } while (0)

#define MI_STORE_TILE(buf)                                                                            \
    do {                                                                                              \
        if (PLAIN) {                                                                                  \
            if (!lc.valid) { bq0 = make_float4(0.f, 0.f, 0.f, 0.f); bq1 = bq0; }                      \
            *reinterpret_cast<float4 *>(&Bs[buf][prow][(tid & 31) * 4]) = bq0;                        \
            *reinterpret_cast<float4 *>(&Bs[buf][prow + 8][(tid & 31) * 4]) = bq1;                    \
        } else {                                                                                      \
            _Pragma("unroll") for (int j = 0; j < 8; ++j)                                              \
                Bs[buf][khalf + 2 * j][tid & 127] = bok[j] ? breg[j] : 0.f;                            \
        }                                                                                             \
        if (A_SLOTS >= 1 && a_on0) *reinterpret_cast<float4 *>(&As[buf][ar0][ac0]) = areg0;           \
        if (A_SLOTS >= 2 && a_on1) *reinterpret_cast<float4 *>(&As[buf][ar1][ac1]) = areg1;           \
    } while (0)

    f32x16 acc[TM][TN];
#pragma unroll
    for (int a = 0; a < TM; ++a)
#pragma unroll
        for (int b = 0; b < TN; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;

    const int nk = d.Kpad / BK;
    const int li = lane & 31, lh = lane >> 5;
    MI_LOAD_TILE(0);
    MI_STORE_TILE(0);
    __syncthreads();
    int cur = 0;
    for (int kt = 0; kt < nk; ++kt) {
        if (kt + 1 < nk) MI_LOAD_TILE(kt + 1);
        // fragments double-buffered in registers: the reads of step s+1 are in flight under the MFMAs of step s
        float af[2][TM], bf[2][TN];
#pragma unroll
        for (int a = 0; a < TM; ++a) af[0][a] = As[cur][lh][(wm * TM + a) * 32 + li];
#pragma unroll
        for (int b = 0; b < TN; ++b) bf[0][b] = Bs[cur][lh][(wn * TN + b) * 32 + li];
#pragma unroll
        for (int s = 0; s < BK / 2; ++s) {
            if (s + 1 < BK / 2) {
#pragma unroll
                for (int a = 0; a < TM; ++a) af[(s + 1) & 1][a] = As[cur][2 * (s + 1) + lh][(wm * TM + a) * 32 + li];
#pragma unroll
                for (int b = 0; b < TN; ++b) bf[(s + 1) & 1][b] = Bs[cur][2 * (s + 1) + lh][(wn * TN + b) * 32 + li];
            }
#pragma unroll
            for (int a = 0; a < TM; ++a)
#pragma unroll
                for (int b = 0; b < TN; ++b)
                    acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[s & 1][a], bf[s & 1][b], acc[a][b], 0, 0, 0);
        }
        // pin the software pipeline: the LDS reads of step s+1 issue BEFORE the MFMAs of step s, so their
        // latency hides under the matrix pipe (hipcc otherwise sinks each read next to its use and waits)
        constexpr int kReads = (TM == 2 ? 1 : TM) + (TN == 2 ? 1 : TN);    // ds_read2_b32 pairs two 32-apart tiles
        __builtin_amdgcn_sched_group_barrier(0x100, kReads, 0);
#pragma unroll
        for (int s = 0; s < BK / 2; ++s) {
            if (s + 1 < BK / 2) __builtin_amdgcn_sched_group_barrier(0x100, kReads, 0);
            __builtin_amdgcn_sched_group_barrier(0x008, TM * TN, 0);
        }
        if (kt + 1 < nk) MI_STORE_TILE(cur ^ 1);
        __syncthreads();
        cur ^= 1;
    }
#undef MI_LOAD_TILE
#undef MI_STORE_TILE

    conv_epilogue<TM, TN, EPI, LFLAGS>(d, acc, m0, n0, wm, wn, N, P, o2v);
}

// ---------------------------------------------------------------------------------------------
// LDS-DMA main loop for the plain (1x1 / linear) 128 x 128 tile: both operand tiles go global -> LDS with
// global_load_lds_dwordx4 (no staging registers, no ds_write), a 3-stage LDS ring keeps TWO K tiles in flight
// behind a counted s_waitcnt vmcnt(4) and ONE raw s_barrier per K tile (cdna_hip_programming.md: "Pipelining
// across barriers").  Each wave-instruction lands 1 KiB = two 128-float rows of a [16][128] tile image.
typedef __attribute__((address_space(1))) const void gvoid_t;
typedef __attribute__((address_space(3))) void lvoid_t;

template <int EPI, int LFLAGS>
__global__ __launch_bounds__(256, 3) void conv_gemm_dma_kernel(const mi_conv_desc d, const int N, const int MT, const int Gm) {
    constexpr int TM = 2, TN = 2, WN = 2, BM = 128;
    constexpr int SS = BK * (BM + BN);                       // floats per stage: A image then B image
    __shared__ __attribute__((aligned(16))) float smem[3 * SS];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WN, wn = wave % WN;
    int mt, nt;
    if (!tile_of_block(MT, Gm, N, mt, nt)) return;
    const int m0 = mt * BM, n0 = nt * BN;
    const int P = d.O1 * d.O2;
    const int o2v = d.o2_valid ? d.o2_valid : d.O2;

    // this lane's share of every tile: rows 4*wave + 2*j + (lane >> 5), j = 0, 1; 16 bytes at column 4*(lane & 31)
    const int r0 = 4 * wave + (lane >> 5), c4 = (lane & 31) * 4;
    const float *asrc = d.wt + (size_t)r0 * d.Mpad + m0 + c4;
    const size_t a_row2 = (size_t)2 * d.Mpad, a_step = (size_t)BK * d.Mpad;
    const ColInfo lc = decompose(n0 + c4, N, P, d.O2, d.O2);
    const float *bsrc = lc.valid ? d.x + (size_t)lc.b * d.x_bstride + lc.p + (size_t)r0 * P : d.sink + MI_SINK_FLOATS;
    const size_t b_row2 = lc.valid ? (size_t)2 * P : 0, b_step = lc.valid ? (size_t)BK * P : 0;

#define MI_DMA_TILE(kt, stage)                                                                                  \
    do {                                                                                                        \
        float *sa = smem + (stage) * SS + (4 * wave) * BM, *sb = smem + (stage) * SS + BK * BM + (4 * wave) * BN; \
        const float *ga = asrc + (size_t)(kt) * a_step, *gb = bsrc + (size_t)(kt) * b_step;                      \
        __builtin_amdgcn_global_load_lds((gvoid_t *)ga, (lvoid_t *)sa, 16, 0, 0);                                \
        __builtin_amdgcn_global_load_lds((gvoid_t *)(ga + a_row2), (lvoid_t *)(sa + 2 * BM), 16, 0, 0);          \
        __builtin_amdgcn_global_load_lds((gvoid_t *)gb, (lvoid_t *)sb, 16, 0, 0);                                \
        __builtin_amdgcn_global_load_lds((gvoid_t *)(gb + b_row2), (lvoid_t *)(sb + 2 * BN), 16, 0, 0);          \
    } while (0)

    f32x16 acc[TM][TN];
#pragma unroll
    for (int a = 0; a < TM; ++a)
#pragma unroll
        for (int b = 0; b < TN; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;

    const int nk = d.Kpad / BK;
    const int li = lane & 31, lh = lane >> 5;
    MI_DMA_TILE(0, 0);
    if (nk > 1) MI_DMA_TILE(1, 1);
    int stage = 0;
    for (int kt = 0; kt < nk; ++kt) {
        // tile kt has landed once all but this wave's newest tile (4 instructions) are done -- for every wave
        if (kt + 1 < nk) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        // stage (kt+2)%3 == (kt-1)%3 was last read in the previous iteration, which every wave has finished
        if (kt + 2 < nk) MI_DMA_TILE(kt + 2, stage == 0 ? 2 : stage - 1);
        const float *As = smem + stage * SS, *Bs = As + BK * BM;
        float af[2][TM], bf[2][TN];
#pragma unroll
        for (int a = 0; a < TM; ++a) af[0][a] = As[lh * BM + (wm * TM + a) * 32 + li];
#pragma unroll
        for (int b = 0; b < TN; ++b) bf[0][b] = Bs[lh * BN + (wn * TN + b) * 32 + li];
#pragma unroll
        for (int s = 0; s < BK / 2; ++s) {
            if (s + 1 < BK / 2) {
#pragma unroll
                for (int a = 0; a < TM; ++a) af[(s + 1) & 1][a] = As[(2 * (s + 1) + lh) * BM + (wm * TM + a) * 32 + li];
#pragma unroll
                for (int b = 0; b < TN; ++b) bf[(s + 1) & 1][b] = Bs[(2 * (s + 1) + lh) * BN + (wn * TN + b) * 32 + li];
            }
#pragma unroll
            for (int a = 0; a < TM; ++a)
#pragma unroll
                for (int b = 0; b < TN; ++b)
                    acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[s & 1][a], bf[s & 1][b], acc[a][b], 0, 0, 0);
        }
        __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);
#pragma unroll
        for (int s = 0; s < BK / 2; ++s) {
            if (s + 1 < BK / 2) __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);
            __builtin_amdgcn_sched_group_barrier(0x008, TM * TN, 0);
        }
        stage = stage == 2 ? 0 : stage + 1;
    }
#undef MI_DMA_TILE
    conv_epilogue<TM, TN, EPI, LFLAGS>(d, acc, m0, n0, wm, wn, N, P, o2v);
}

// ---------------------------------------------------------------------------------------------
// LDS-DMA main loop for STRIDE-1 k x k convolutions in float32 (the decoders' 3 x 3 / k = 3 "rewrite" convs, reference
// demucs/hdemucs.py:304-314): round 3 ran them on the table-driven gather of conv_gemm_kernel (8 dword gathers + bounds tests
// + ds_writes per thread and K step) at 0.64-0.70 of the fp32 MFMA peak against 0.74 for the DMA loop above.  Row k = (ci, tap)
// of a K step's B tile is, for 128 consecutive output positions, a run of the input row shifted by the tap's offset
// d1 * pitch + d2 -- and global_load_lds_dwordx4 takes a source that is only 4-byte aligned (tools/micro/dma_unaligned.hip), so
// the run goes global -> LDS by DMA like a plain layer's: no staging registers, no table.  What the shift drags in at the two
// ends of an input row (the neighbouring row's sample, or a pitch-padding column) is overwritten with the conv's zero padding
// in LDS by the lane that issued the transfer, after its counted wait and before the barrier: at most two ds_write_b32 per
// lane and K step.  Taps whose input ROW lies outside the frame read the zero page.  K2 = 3 (|d2| <= 1).
// Tiles: 128 x 128 (2 x 2 waves) and 96 x 128 (1 x 4 waves; the A image [16][96] is six 1-KiB transfers: waves 0, 1 issue two
// of them, waves 2, 3 one, so the counted waits are per wave).  Same 3-stage ring, one raw s_barrier per K step.
// DIL (round 4, later): step between the K2 = 3 taps of a k = 3 conv -- the DConv blocks' dilated convs C -> C / 8 (demucs.py:138: dilation
// 1 / 2, padding = dilation) with the row-statistics epilogue, on 32- and 64-row tiles (M = 24 / 48: two / four A transfers per K step).
// With DIL > 1 up to DIL samples at either end of a row come from outside it: the lanes that own the first chunk of a row and the
// chunks within eight columns of its valid end re-test their four elements per tap (a rare branch) instead of the single fix_l / fix_r.
template <int BMT, int EPI, int NT, int DIL = 1>
__global__ __launch_bounds__(256, 3) void conv_gemm_dmatap_kernel(const mi_conv_desc d, const int N, const int MT, const int Gm) {
    constexpr int BM = BMT, WM = BM == 128 ? 2 : 1, WN = 4 / WM, TM = BM / (32 * WM), TN = BN / (32 * WN);
    constexpr int SS = BK * (BM + BN);                       // floats per stage: A image then B image
    __shared__ __attribute__((aligned(16))) float smem[3 * SS];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WN, wn = wave % WN;
    int mt, nt;
    if (!tile_of_block(MT, Gm, N, mt, nt)) return;
    const int m0 = mt * BM, n0 = nt * BN;
    const int P = d.O1 * d.O2;
    const int o2v = d.o2_valid ? d.o2_valid : d.O2;
    constexpr int K2 = 3;                                    // NT = 9 (3 x 3) or 3 (k = 3): divisions by constants
    const int x_ld = d.x_ld ? d.x_ld : d.D2;
    const int64_t chan = (int64_t)d.D1 * x_ld;               // input channel stride
    const float *zero = d.sink + MI_SINK_FLOATS;

    // ---- A: this wave's transfers of every K step ------------------------------------------------------------------------------
    // BM = 128: two transfers of two 128-float rows each (rows 4 wave + 2 j + (lane >> 5)); BM = 96: transfer q moves floats
    // [256 q, 256 q + 256) of the [16][96] image, q = wave and, for waves 0 and 1, q = 4 + wave
    // BM = 64: transfer q = wave (one each); BM = 32: two transfers in all, waves 0 and 1
    constexpr int NA = BM >= 96 ? 2 : 1;                     // slots (the second one of waves 2, 3 is idle at BM = 96)
    const bool a1 = BM != 32 || wave < 2, a2 = BM == 128 || (BM == 96 && wave < 2);
    int a_row[NA], a_col[NA], a_lds[NA];
#pragma unroll
    for (int j = 0; j < NA; ++j) {
        if (BM == 128) { a_row[j] = 4 * wave + 2 * j + (lane >> 5); a_col[j] = (lane & 31) * 4; a_lds[j] = (4 * wave + 2 * j) * BM; }
        else { const int q = j ? 4 + wave : wave, f = 256 * q + 4 * lane; a_row[j] = f / BM; a_col[j] = f % BM; a_lds[j] = 256 * q; }
    }
    // ---- B: rows 4 wave + 2 j + (lane >> 5), 16 bytes at column 4 (lane & 31) ---------------------------------------------------
    const int c4 = (lane & 31) * 4, rb0 = 4 * wave + (lane >> 5);
    const ColInfo lc = decompose(n0 + c4, N, P, d.O2, o2v);
    const float *xcol = d.x + (size_t)lc.b * d.x_bstride + (size_t)lc.o1 * x_ld + lc.o2;
    // elements of this lane's 4-column chunk that a tap with d2 = -1 / +1 reads from outside the input row [0, D2)
    const int fix_l = (lc.valid && lc.o2 == 0) ? 0 : -1;
    const int fr = d.D2 - 1 - lc.o2;
    const int fix_r = (lc.valid && fr >= 0 && fr < 4) ? fr : -1;
    const bool edge = lc.valid && (lc.o2 < 4 || lc.o2 + 8 > d.D2);       // DIL > 1: chunks that can hold an element from outside [0, D2)

#define MI_TAPDMA_TILE(kt, stage)                                                                                   \
    do {                                                                                                            \
        float *sa = smem + (stage) * SS, *sb = sa + BK * BM + (4 * wave) * BN;                                      \
        _Pragma("unroll") for (int j = 0; j < NA; ++j)                                                              \
            if (j == 0 ? a1 : a2) {                                                                                 \
                const float *ga = d.wt + (size_t)((kt) * BK + a_row[j]) * d.Mpad + m0 + a_col[j];                   \
                __builtin_amdgcn_global_load_lds((gvoid_t *)ga, (lvoid_t *)(sa + a_lds[j]), 16, 0, 0);              \
            }                                                                                                       \
        _Pragma("unroll") for (int j = 0; j < 2; ++j) {                                                             \
            const int k = (kt) * BK + rb0 + 2 * j, ci = k / NT, tap = k - ci * NT, t1 = tap / K2, t2 = tap - t1 * K2; \
            const int i1 = lc.o1 + t1 - d.tap_pad1;                                                                 \
            const bool ok = lc.valid && k < d.K && (unsigned)i1 < (unsigned)d.D1;                                   \
            const float *gb = xcol + (int64_t)ci * chan + (int64_t)(t1 - d.tap_pad1) * x_ld + (t2 * DIL - d.tap_pad2); \
            __builtin_amdgcn_global_load_lds((gvoid_t *)(ok ? gb : zero), (lvoid_t *)(sb + 2 * j * BN), 16, 0, 0);  \
        }                                                                                                           \
    } while (0)

    f32x16 acc[TM][TN];
#pragma unroll
    for (int a = 0; a < TM; ++a)
#pragma unroll
        for (int b = 0; b < TN; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;

    const int nk = d.Kpad / BK;
    const int li = lane & 31, lh = lane >> 5;
    MI_TAPDMA_TILE(0, 0);
    if (nk > 1) MI_TAPDMA_TILE(1, 1);
    int stage = 0;
    for (int kt = 0; kt < nk; ++kt) {
        // tile kt has landed once all but this wave's newest tile (2 B transfers + its A transfers: 4, 3 or 2) are done
        if (kt + 1 < nk) {
            if (a2) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
            else if (a1) asm volatile("s_waitcnt vmcnt(3)" ::: "memory");
            else asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
        } else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        {   // the conv's zero padding at the ends of the input rows, in the rows this lane transferred
            float *sb = smem + stage * SS + BK * BM + (4 * wave) * BN + (lane >> 5) * BN + c4;
            if constexpr (DIL == 1) {
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    const int k = kt * BK + rb0 + 2 * j, tap = k % NT, dd2 = tap % K2 - d.tap_pad2;
                    if (dd2 < 0 && fix_l >= 0) sb[2 * j * BN + fix_l] = 0.f;
                    if (dd2 > 0 && fix_r >= 0) sb[2 * j * BN + fix_r] = 0.f;
                }
            } else if (edge) {
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    const int k = kt * BK + rb0 + 2 * j, tap = k % NT, dd2 = (tap % K2) * DIL - d.tap_pad2;
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if ((unsigned)(lc.o2 + e + dd2) >= (unsigned)d.D2) sb[2 * j * BN + e] = 0.f;
                }
            }
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        // stage (kt+2)%3 == (kt-1)%3 was last read in the previous iteration, which every wave has finished
        if (kt + 2 < nk) MI_TAPDMA_TILE(kt + 2, stage == 0 ? 2 : stage - 1);
        const float *As = smem + stage * SS, *Bs = As + BK * BM;
        float af[2][TM], bf[2][TN];
#pragma unroll
        for (int a = 0; a < TM; ++a) af[0][a] = As[lh * BM + (wm * TM + a) * 32 + li];
#pragma unroll
        for (int b = 0; b < TN; ++b) bf[0][b] = Bs[lh * BN + (wn * TN + b) * 32 + li];
#pragma unroll
        for (int s = 0; s < BK / 2; ++s) {
            if (s + 1 < BK / 2) {
#pragma unroll
                for (int a = 0; a < TM; ++a) af[(s + 1) & 1][a] = As[(2 * (s + 1) + lh) * BM + (wm * TM + a) * 32 + li];
#pragma unroll
                for (int b = 0; b < TN; ++b) bf[(s + 1) & 1][b] = Bs[(2 * (s + 1) + lh) * BN + (wn * TN + b) * 32 + li];
            }
#pragma unroll
            for (int a = 0; a < TM; ++a)
#pragma unroll
                for (int b = 0; b < TN; ++b)
                    acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[s & 1][a], bf[s & 1][b], acc[a][b], 0, 0, 0);
        }
        constexpr int kReads = (TM == 2 ? 1 : TM) + (TN == 2 ? 1 : TN);
        __builtin_amdgcn_sched_group_barrier(0x100, kReads, 0);
#pragma unroll
        for (int s = 0; s < BK / 2; ++s) {
            if (s + 1 < BK / 2) __builtin_amdgcn_sched_group_barrier(0x100, kReads, 0);
            __builtin_amdgcn_sched_group_barrier(0x008, TM * TN, 0);
        }
        stage = stage == 2 ? 0 : stage + 1;
    }
#undef MI_TAPDMA_TILE
    conv_epilogue<TM, TN, EPI, 0>(d, acc, m0, n0, wm, wn, N, P, o2v);
}

template <int EPI>
static int launch_dmatap(const mi_conv_desc &d, int tile, hipStream_t st) {
    const int64_t N64 = (int64_t)d.B * d.O1 * d.O2;
    MI_REQUIRE(N64 < (1ll << 31) - 256 && d.Mpad % tile == 0, "conv: DMA tap route: %lld positions, Mpad %d", (long long)N64, d.Mpad);
    const int N = (int)N64, MT = d.Mpad / tile, NT = ceil_div(N, BN);
    const unsigned grid = grouped_grid(MT, NT, 1);
    if constexpr (EPI == MI_EPI_BIAS_STATS) {
        const bool d2 = d.tap_dil2 == 2;
        if (tile == 64 && d2) hipLaunchKernelGGL((conv_gemm_dmatap_kernel<64, EPI, 3, 2>), dim3(grid), dim3(256), 0, st, d, N, MT, 1);
        else if (tile == 64) hipLaunchKernelGGL((conv_gemm_dmatap_kernel<64, EPI, 3, 1>), dim3(grid), dim3(256), 0, st, d, N, MT, 1);
        else if (d2) hipLaunchKernelGGL((conv_gemm_dmatap_kernel<32, EPI, 3, 2>), dim3(grid), dim3(256), 0, st, d, N, MT, 1);
        else hipLaunchKernelGGL((conv_gemm_dmatap_kernel<32, EPI, 3, 1>), dim3(grid), dim3(256), 0, st, d, N, MT, 1);
    } else if (tile == 128 && d.ntaps == 9) hipLaunchKernelGGL((conv_gemm_dmatap_kernel<128, EPI, 9>), dim3(grid), dim3(256), 0, st, d, N, MT, 1);
    else if (tile == 128) hipLaunchKernelGGL((conv_gemm_dmatap_kernel<128, EPI, 3>), dim3(grid), dim3(256), 0, st, d, N, MT, 1);
    else if (d.ntaps == 9) hipLaunchKernelGGL((conv_gemm_dmatap_kernel<96, EPI, 9>), dim3(grid), dim3(256), 0, st, d, N, MT, 1);
    else hipLaunchKernelGGL((conv_gemm_dmatap_kernel<96, EPI, 3>), dim3(grid), dim3(256), 0, st, d, N, MT, 1);
    MI_CHECK_LAUNCH();
    return MI_OK;
}

// ---------------------------------------------------------------------------------------------
// LDS-DMA main loop for float32 layers whose taps move along ROWS only (every table entry has d2 == 0, S2 == 1): the frequency
// branch's strided encoder convs (k = 8, s = 4 along the frequency axis: row 4 o1 + j - 2), its transposed convs as two-tap GEMMs
// (rows q, q - 1) and every 1x1 layer that does not run conv_gemm_dma_kernel (GLU / GroupNorm-GLU epilogues, 96- and 64-row
// tiles).  Row k of a K step's B tile is then a run of an input row at the SAME columns as the output tile, 16-byte chunks at
// aligned positions: no shifted runs, no zero-padding fix-up, never an address outside the tensor (a tap whose row lies outside
// [0, D1), a column past the end and the K padding read the zero page).  The row offsets come from the gather table -- one
// SCALAR 64-byte load per wave and K step (its four rows' entries; lgkmcnt, so the counted vmcnt waits of the transfer ring stay
// exact) -- which keeps ONE kernel per (tile, epilogue) for all of these layers.  Summation order = conv_gemm_kernel's: results
// are bit-identical to the table-driven route (tests/test_gpu_kernels.py).  Round 3 ran these classes at 0.5-0.6 of the fp32 MFMA
// peak (8 dword gathers + bounds tests + ds_writes per thread and K step, or float4 loads staged through registers).
template <int BMT, int EPI, int LFLAGS>
__global__ __launch_bounds__(256, 3) void conv_gemm_dmarow_kernel(const mi_conv_desc d, const int N, const int MT, const int Gm) {
    constexpr int BM = BMT, WM = BM == 128 ? 2 : 1, WN = 4 / WM, TM = BM / (32 * WM), TN = BN / (32 * WN);
    constexpr int SS = BK * (BM + BN);                       // floats per stage: A image then B image
    __shared__ __attribute__((aligned(16))) float smem[3 * SS];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WN, wn = wave % WN;
    int mt, nt;
    if (!tile_of_block(MT, Gm, N, mt, nt)) return;
    const int m0 = mt * BM, n0 = nt * BN;
    const int P = d.O1 * d.O2;
    const int o2v = d.o2_valid ? d.o2_valid : d.O2;
    const int x_ld = d.x_ld ? d.x_ld : d.D2;
    const float *zero = d.sink + MI_SINK_FLOATS;

    // ---- A: the [16][BM] image of a K step is BM / 16 transfers of 1 KiB: BM = 128: two per wave (two 128-float rows each);
    //      BM = 96: six (waves 0, 1 two, waves 2, 3 one); BM = 64: one per wave.  Transfer q moves floats [256 q, 256 q + 256)
    constexpr int NA = BM == 64 ? 1 : 2;
    const bool a2 = BM == 128 || (BM == 96 && wave < 2);
    int a_row[NA], a_col[NA], a_lds[NA];
#pragma unroll
    for (int j = 0; j < NA; ++j) {
        const int q = j ? 4 + wave : wave, f = 256 * q + 4 * lane;
        a_row[j] = f / BM; a_col[j] = f % BM; a_lds[j] = 256 * q;
    }
    // ---- B: rows 4 wave + 2 j + (lane >> 5), 16 bytes at column 4 (lane & 31) ---------------------------------------------------
    const int c4 = (lane & 31) * 4, lh = lane >> 5;
    const ColInfo lc = decompose(n0 + c4, N, P, d.O2, o2v);
    const int i1b = lc.o1 * d.S1;
    const float *xcol = d.x + (size_t)lc.b * d.x_bstride + (size_t)i1b * x_ld + lc.o2;
    const int4 *ktab4 = reinterpret_cast<const int4 *>(d.ktab) + 4 * wave;       // (off, d1, d2, ci) of this wave's four rows
    // (off, d1) of rows 4 wave .. 4 wave + 3 of K step kt into SGPRs.  Inline asm: hipcc turns these uniform loads into VMEM loads
    // inside the loop (the DMA builtins count as stores that might alias the table) and then waits vmcnt(0) for them -- which
    // drains the transfer ring every K step
    typedef int v2i __attribute__((ext_vector_type(2)));
    v2i e0, e1, e2, e3;
#define MI_ROW_ENTRIES(kt)                                                                                           \
    asm volatile("s_load_dwordx2 %0, %4, 0x0\n\ts_load_dwordx2 %1, %4, 0x10\n\ts_load_dwordx2 %2, %4, 0x20\n\t"          \
                 "s_load_dwordx2 %3, %4, 0x30\n\ts_waitcnt lgkmcnt(0)"                                               \
                 : "=&s"(e0), "=&s"(e1), "=&s"(e2), "=&s"(e3) : "s"(ktab4 + (kt) * BK) : "memory")

#define MI_ROWDMA_TILE(kt, stage)                                                                                   \
    do {                                                                                                            \
        float *sa = smem + (stage) * SS, *sb = sa + BK * BM + (4 * wave) * BN;                                      \
        _Pragma("unroll") for (int j = 0; j < NA; ++j)                                                              \
            if (j == 0 || a2) {                                                                                     \
                const float *ga = d.wt + (size_t)((kt) * BK + a_row[j]) * d.Mpad + m0 + a_col[j];                   \
                __builtin_amdgcn_global_load_lds((gvoid_t *)ga, (lvoid_t *)(sa + a_lds[j]), 16, 0, 0);              \
            }                                                                                                       \
        _Pragma("unroll") for (int j = 0; j < 2; ++j) {                                                             \
            const int off = j ? (lh ? e3.x : e2.x) : (lh ? e1.x : e0.x), dd1 = j ? (lh ? e3.y : e2.y) : (lh ? e1.y : e0.y); \
            const bool ok = lc.valid && (unsigned)(i1b + dd1) < (unsigned)d.D1;                                     \
            __builtin_amdgcn_global_load_lds((gvoid_t *)(ok ? xcol + off : zero), (lvoid_t *)(sb + 2 * j * BN), 16, 0, 0); \
        }                                                                                                           \
    } while (0)

    f32x16 acc[TM][TN];
#pragma unroll
    for (int a = 0; a < TM; ++a)
#pragma unroll
        for (int b = 0; b < TN; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;

    const int nk = d.Kpad / BK;
    const int li = lane & 31;
    MI_ROW_ENTRIES(0);
    MI_ROWDMA_TILE(0, 0);
    if (nk > 1) { MI_ROW_ENTRIES(1); MI_ROWDMA_TILE(1, 1); }
    int stage = 0;
    for (int kt = 0; kt < nk; ++kt) {
        // the table rows of K step kt + 2: their latency passes under the wait for tile kt and the barrier
        if (kt + 2 < nk) MI_ROW_ENTRIES(kt + 2);
        // tile kt has landed once all but this wave's newest tile (3 or 4 transfers) are done -- for every wave
        if (kt + 1 < nk) {
            if (BM == 64 || (BM == 96 && !a2)) asm volatile("s_waitcnt vmcnt(3)" ::: "memory");
            else asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
        } else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        // stage (kt+2)%3 == (kt-1)%3 was last read in the previous iteration, which every wave has finished
        if (kt + 2 < nk) MI_ROWDMA_TILE(kt + 2, stage == 0 ? 2 : stage - 1);
        const float *As = smem + stage * SS, *Bs = As + BK * BM;
        float af[2][TM], bf[2][TN];
#pragma unroll
        for (int a = 0; a < TM; ++a) af[0][a] = As[lh * BM + (wm * TM + a) * 32 + li];
#pragma unroll
        for (int b = 0; b < TN; ++b) bf[0][b] = Bs[lh * BN + (wn * TN + b) * 32 + li];
#pragma unroll
        for (int s = 0; s < BK / 2; ++s) {
            if (s + 1 < BK / 2) {
#pragma unroll
                for (int a = 0; a < TM; ++a) af[(s + 1) & 1][a] = As[(2 * (s + 1) + lh) * BM + (wm * TM + a) * 32 + li];
#pragma unroll
                for (int b = 0; b < TN; ++b) bf[(s + 1) & 1][b] = Bs[(2 * (s + 1) + lh) * BN + (wn * TN + b) * 32 + li];
            }
#pragma unroll
            for (int a = 0; a < TM; ++a)
#pragma unroll
                for (int b = 0; b < TN; ++b)
                    acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[s & 1][a], bf[s & 1][b], acc[a][b], 0, 0, 0);
        }
        constexpr int kReads = (TM == 2 ? 1 : TM) + (TN == 2 ? 1 : TN);
        __builtin_amdgcn_sched_group_barrier(0x100, kReads, 0);
#pragma unroll
        for (int s = 0; s < BK / 2; ++s) {
            if (s + 1 < BK / 2) __builtin_amdgcn_sched_group_barrier(0x100, kReads, 0);
            __builtin_amdgcn_sched_group_barrier(0x008, TM * TN, 0);
        }
        stage = stage == 2 ? 0 : stage + 1;
    }
#undef MI_ROWDMA_TILE
#undef MI_ROW_ENTRIES
    conv_epilogue<TM, TN, EPI, LFLAGS>(d, acc, m0, n0, wm, wn, N, P, o2v);
}

template <int EPI, int LFLAGS>
static int launch_dmarow(const mi_conv_desc &d, int tile, hipStream_t st) {
    const int64_t N64 = (int64_t)d.B * d.O1 * d.O2;
    MI_REQUIRE(N64 < (1ll << 31) - 256 && d.Mpad % tile == 0, "conv: DMA row route: %lld positions, Mpad %d", (long long)N64, d.Mpad);
    const int N = (int)N64, MT = d.Mpad / tile, NT = ceil_div(N, BN);
    const unsigned grid = grouped_grid(MT, NT, 1);
    if (tile == 128) hipLaunchKernelGGL((conv_gemm_dmarow_kernel<128, EPI, LFLAGS>), dim3(grid), dim3(256), 0, st, d, N, MT, 1);
    else if constexpr (EPI == MI_EPI_LINEAR || EPI == MI_EPI_CONVTR) {
        if (tile == 96) hipLaunchKernelGGL((conv_gemm_dmarow_kernel<96, EPI, LFLAGS>), dim3(grid), dim3(256), 0, st, d, N, MT, 1);
        else hipLaunchKernelGGL((conv_gemm_dmarow_kernel<64, EPI, LFLAGS>), dim3(grid), dim3(256), 0, st, d, N, MT, 1);
    } else return set_error(MI_EINVAL, "conv: DMA row route has no %d-row tile for epilogue %d", tile, EPI);
    MI_CHECK_LAUNCH();
    return MI_OK;
}

// ---------------------------------------------------------------------------------------------
// The native kernels, `r` as conv_route decided.  Route MI_ROUTE_DMA: the LDS-DMA linear tile instead of the register-staged
// loader -- a plain LINEAR layer on the 128-row tile
template <int WM, int WN, int TM, int TN, int EPI, int LFLAGS, bool PLAIN>
static int launch_cfg(const mi_conv_desc &d, const ConvRoute &r, hipStream_t st) {
    constexpr int BM = WM * TM * 32;
    const bool dma = r.route == MI_ROUTE_DMA;
    const int64_t N64 = (int64_t)d.B * d.O1 * d.O2;
    MI_REQUIRE(N64 < (1ll << 31) - 256, "conv: too many output positions (%lld)", (long long)N64);
    MI_REQUIRE(d.Mpad % BM == 0, "conv: Mpad %d not a multiple of the %d-row tile", d.Mpad, BM);
    const int N = (int)N64, MT = d.Mpad / BM, NT = ceil_div(N, BN);
    const int Gm = r.mgroups ? pick_m_groups(MT, (size_t)d.Kpad * d.Mpad * 4) : 1;
    const unsigned grid = grouped_grid(MT, NT, Gm);
    if constexpr (PLAIN && BM == 128 && EPI == MI_EPI_LINEAR) {
        if (dma) {
            hipLaunchKernelGGL((conv_gemm_dma_kernel<EPI, LFLAGS>), dim3(grid), dim3(256), 0, st, d, N, MT, Gm);
            MI_CHECK_LAUNCH();
            return MI_OK;
        }
    }
    MI_REQUIRE(!dma, "conv: the LDS-DMA linear tile takes a plain LINEAR layer on the 128-row tile");
    hipLaunchKernelGGL((conv_gemm_kernel<WM, WN, TM, TN, EPI, LFLAGS, PLAIN>), dim3(grid), dim3(256), 0, st, d, N, MT, Gm);
    MI_CHECK_LAUNCH();
    return MI_OK;
}

template <int EPI, int LFLAGS, bool PLAIN>
static int launch_tile(const mi_conv_desc &d, const ConvRoute &r, hipStream_t st) {
    switch (r.tile) {
        case 128: return launch_cfg<2, 2, 2, 2, EPI, LFLAGS, PLAIN>(d, r, st);
        case 96: return launch_cfg<1, 4, 3, 1, EPI, LFLAGS, PLAIN>(d, r, st);
        case 64: return launch_cfg<1, 4, 2, 1, EPI, LFLAGS, PLAIN>(d, r, st);
        case 32: return launch_cfg<1, 4, 1, 1, EPI, LFLAGS, PLAIN>(d, r, st);
    }
    return set_error(MI_EINVAL, "conv: unsupported tile_m %d", r.tile);
}

// MI_SINK_FLOATS-float dump for the epilogue's out-of-range stores (thread tid writes word tid % MI_SINK_FLOATS), shared by all
// launches, followed by MI_ZERO_PAGE_FLOATS floats that stay zero (source of the LDS-DMA loader for out-of-range columns)
static float *conv_sink() {
    static float *p = nullptr;
    if (!p) {
        if (hipMalloc((void **)&p, (MI_SINK_FLOATS + MI_ZERO_PAGE_FLOATS) * sizeof(float)) != hipSuccess) { p = nullptr; return nullptr; }
        (void)hipMemset(p, 0, (MI_SINK_FLOATS + MI_ZERO_PAGE_FLOATS) * sizeof(float));
    }
    return p;
}

// 256 bytes of zeros in device memory (the tail of the sink): source of LDS-DMA loads that fall outside a tensor
const void *conv_zero_page() {
    float *p = conv_sink();
    return p ? p + MI_SINK_FLOATS : nullptr;
}

// fill the sink, validate and decide (conv_route.hip), launch
int launch_conv(const mi_conv_desc &din, hipStream_t st) {
    mi_conv_desc d = din;
    if (!d.sink) d.sink = conv_sink();
    MI_REQUIRE(d.sink && ((uintptr_t)d.sink & 15) == 0, "conv: the store sink could not be allocated or is not 16-byte aligned");
    MI_TRY(conv_validate(d));
    const ConvRoute r = conv_route(d);
    // the tile the layer's split image was packed for: a 192-row layer's is a run of 96-row images
    const int image_tile = d.tile_m == 192 ? 96 : d.tile_m ? d.tile_m : conv_pick_tile(d.M);
    g_last_conv_route = r.route;
    g_last_conv_tile = r.tile;
    switch (r.route) {
        case MI_ROUTE_TAP_HALF: return launch_conv_tap(d, r.tile, st);
        case MI_ROUTE_HALF:
        case MI_ROUTE_HALF_IMG:
        case MI_ROUTE_HALF_IMG256: return launch_conv_half(d, r, st);
        case MI_ROUTE_TAP_X6: return launch_conv_tap_x6(d, r.tile, image_tile, st);
        case MI_ROUTE_ROWS_X6: return launch_conv_rows_x6(d, r.tile, image_tile, st);
        case MI_ROUTE_X6: return launch_conv_x6(d, r.tile, image_tile, r.plain, st);
        case MI_ROUTE_DMATAP:
            return d.epi == MI_EPI_GLU ? launch_dmatap<MI_EPI_GLU>(d, r.tile, st) : launch_dmatap<MI_EPI_BIAS_STATS>(d, r.tile, st);
        case MI_ROUTE_DMAROW:
            switch (d.epi) {
                case MI_EPI_LINEAR: return launch_dmarow<MI_EPI_LINEAR, MI_FLAG_GELU>(d, r.tile, st);
                case MI_EPI_CONVTR: return launch_dmarow<MI_EPI_CONVTR, 0>(d, r.tile, st);
                case MI_EPI_GLU: return launch_dmarow<MI_EPI_GLU, 0>(d, r.tile, st);
                case MI_EPI_GN_GLU: return launch_dmarow<MI_EPI_GN_GLU, 0>(d, r.tile, st);
            }
            return set_error(MI_EINVAL, "conv: DMA row route has no epilogue %d", d.epi);
    }
    // MI_ROUTE_TABLE, MI_ROUTE_DMA: the native fp32 kernels
    return dispatch_epilogue(d, [&](auto epi, auto lflags) {
        constexpr int E = decltype(epi)::value, F = decltype(lflags)::value;
        return r.plain ? launch_tile<E, F, true>(d, r, st) : launch_tile<E, F, false>(d, r, st);
    });
}

}  // namespace mi
