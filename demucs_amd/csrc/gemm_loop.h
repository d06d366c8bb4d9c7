// The pieces the implicit-GEMM main loops share, each spelled once (gemm_conv.hip: fp32 MFMA; gemm_x6.hip: split-bf16 MFMA;
// gemm_half.hip, gemm_tap.hip: 16-bit MFMA): workgroup prologue, accumulators, the K steps, the three-stage LDS-DMA ring, the plan
// of a wave's A-image transfers, the loaders of a raw float32 activation tile, and the host's launch geometry.
// Built both ways (-amdgpu-mfma-vgpr-form=1 for gemm_conv.hip, =0 for the others): nothing here depends on the form.
#pragma once
#include "gemm_tile.h"

namespace mi {

// ---- workgroup prologue ------------------------------------------------------------------------------------------------------
struct Wg {
    int tid, lane, li, lh;      // thread; lane, and its place in a 32x32 MFMA fragment: row / column li = lane & 31, k half lh = lane >> 5
    int wave, wm, wn;           // wave (wave-uniform) and its place in the WM x WN grid of waves
    int mt, nt, m0, n0;         // the workgroup's tile and its first row / column
    int P, o2v;                 // output positions per batch item; valid width of an output row (O2 is a padded pitch)
};
template <int WN>
__device__ __forceinline__ Wg wg_lanes(const mi_conv_desc &d) {
    Wg w;
    w.tid = threadIdx.x; w.lane = w.tid & 63; w.li = w.lane & 31; w.lh = w.lane >> 5;
    w.wave = __builtin_amdgcn_readfirstlane(w.tid >> 6);
    w.wm = w.wave / WN; w.wn = w.wave % WN;
    w.mt = w.nt = w.m0 = w.n0 = 0;
    w.P = d.O1 * d.O2;
    w.o2v = d.o2_valid ? d.o2_valid : d.O2;
    return w;
}
// false for the grid's padding workgroups: the whole workgroup returns, before any barrier
template <int WN, int BM>
__device__ __forceinline__ bool wg_tile(const mi_conv_desc &d, int MT, int Gm, int N, Wg &w) {
    w = wg_lanes<WN>(d);
    if (!tile_of_block(MT, Gm, N, w.mt, w.nt)) return false;
    w.m0 = w.mt * BM; w.n0 = w.nt * BN;
    return true;
}

template <int TM, int TN>
__device__ __forceinline__ void zero_acc(f32x16 (&acc)[TM][TN]) {
#pragma unroll
    for (int a = 0; a < TM; ++a)
#pragma unroll
        for (int b = 0; b < TN; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;
}

// ACCUMULATORS IN AGPRs.  On this platform a stream of v_mfma_f32_32x32x16_bf16 / 16x16x32_bf16 whose destination is in
// ARCHITECTURAL VGPRs corrupts kernels of OTHER processes that run on the same CUs (tools/micro/mfma_neighbour.hip:
// a bare MFMA loop with no memory traffic is enough; fp32 MFMAs and bf16 MFMAs with AGPR accumulators -- what the
// vendor GEMMs use -- are clean).  hipcc picks the VGPR form whenever the registers fit; one inline-asm AGPR operand in
// the kernel makes it allocate AGPRs and place every MFMA accumulator there (the Makefile builds the files of the 16-bit MFMA
// kernels with -amdgpu-mfma-vgpr-form=0).
__device__ __forceinline__ void agpr_anchor() {
    float anchor = 0.f;
    asm volatile("; accumulators in AGPRs %0" : "+a"(anchor));
}

// ---- K steps -----------------------------------------------------------------------------------------------------------------
// One fp32 K step of BK on the k-major tile images As [BK][APITCH], Bs [BK][BN].  The fragments are double-buffered in registers:
// the reads of step s + 1 are in flight under the MFMAs of step s
template <int TM, int TN, int APITCH>
__device__ __forceinline__ void fp32_kstep(const float *As, const float *Bs, const Wg &w, f32x16 (&acc)[TM][TN]) {
    float af[2][TM], bf[2][TN];
#pragma unroll
    for (int a = 0; a < TM; ++a) af[0][a] = As[w.lh * APITCH + (w.wm * TM + a) * 32 + w.li];
#pragma unroll
    for (int b = 0; b < TN; ++b) bf[0][b] = Bs[w.lh * BN + (w.wn * TN + b) * 32 + w.li];
#pragma unroll
    for (int s = 0; s < BK / 2; ++s) {
        if (s + 1 < BK / 2) {
#pragma unroll
            for (int a = 0; a < TM; ++a) af[(s + 1) & 1][a] = As[(2 * (s + 1) + w.lh) * APITCH + (w.wm * TM + a) * 32 + w.li];
#pragma unroll
            for (int b = 0; b < TN; ++b) bf[(s + 1) & 1][b] = Bs[(2 * (s + 1) + w.lh) * BN + (w.wn * TN + b) * 32 + w.li];
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
}

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

template <int HT>
__device__ __forceinline__ f32x16 mfma16(const uint4 a, const uint4 b, const f32x16 c) {
    if (HT == MI_DTYPE_BF16)
        return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
    else
        return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
}

// One 16-bit K step of 32 on the operand images As [4 octets][APITCH], Bs [4][BPITCH] of 16-byte words
template <int HT, int TM, int TN, int APITCH, int BPITCH>
__device__ __forceinline__ void half_kstep(const uint4 *As, const uint4 *Bs, const Wg &w, f32x16 (&acc)[TM][TN]) {
    uint4 af[2][TM], bf[2][TN];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
#pragma unroll
        for (int a = 0; a < TM; ++a) af[s][a] = As[(2 * s + w.lh) * APITCH + (w.wm * TM + a) * 32 + w.li];
#pragma unroll
        for (int b = 0; b < TN; ++b) bf[s][b] = Bs[(2 * s + w.lh) * BPITCH + (w.wn * TN + b) * 32 + w.li];
    }
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int a = 0; a < TM; ++a)
#pragma unroll
            for (int b = 0; b < TN; ++b) acc[a][b] = mfma16<HT>(af[s][a], bf[s][b], acc[a][b]);
}

// ---- the three-stage LDS-DMA ring ----------------------------------------------------------------------------------------------
// the counts the rings use; n is a compile-time constant or wave-uniform
__device__ __forceinline__ void wait_vmcnt(int n) {
    if (n == 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    else if (n == 2) asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
    else if (n == 3) asm volatile("s_waitcnt vmcnt(3)" ::: "memory");
    else if (n == 4) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
    else if (n == 6) asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
    else __builtin_trap();                                   // a count no ring uses: a looser wait would be a race
}
struct RingNop {
    template <class... A>
    __device__ __forceinline__ void operator()(A...) const {}
};
// TWO K tiles in flight behind a counted s_waitcnt vmcnt and ONE raw s_barrier per K tile (cdna_hip_programming.md: "Pipelining
// across barriers").  `in_flight` is the number of transfers the calling wave issues per tile: vmcnt retires in order, so tile kt
// has landed once all but this wave's newest tile are done -- and, after the barrier, every wave's share of it.  The tile
// kt + 2 goes into stage (kt + 2) % 3 == (kt - 1) % 3, which was last read in the previous iteration: every wave has finished
// that one when it passes the barrier.
//   prefetch(kt)      wave state that issue(kt, .) needs, fetched ahead of the wait so that its latency passes under it
//   issue(kt, stage)  this wave's transfers of tile kt
//   landed(kt, stage) after the wave's own wait, before the barrier: what the issuing lane mends in its own rows
//   step(stage)       the K step on a landed stage
template <class Prefetch, class Issue, class Landed, class Step>
__device__ __forceinline__ void dma_ring3(int nk, int in_flight, Prefetch prefetch, Issue issue, Landed landed, Step step) {
    prefetch(0);
    issue(0, 0);
    if (nk > 1) { prefetch(1); issue(1, 1); }
    int stage = 0;
    for (int kt = 0; kt < nk; ++kt) {
        if (kt + 2 < nk) prefetch(kt + 2);
        if (kt + 1 < nk) wait_vmcnt(in_flight);
        else wait_vmcnt(0);
        landed(kt, stage);
        __builtin_amdgcn_s_barrier();
        if (kt + 2 < nk) issue(kt + 2, stage == 0 ? 2 : stage - 1);
        step(stage);
        stage = stage == 2 ? 0 : stage + 1;
    }
}

// ---- A: a wave's transfers of the [BK][BM] float32 weight image of a K step ---------------------------------------------------
// The image is BM / 16 transfers of 1 KiB.  Transfer q moves floats [256 q, 256 q + 256); a wave issues q = wave and q = 4 + wave:
// BM = 128: two per wave; BM = 96: six in all (waves 0, 1 two, waves 2, 3 one); BM = 64: one per wave; BM = 32: waves 0, 1 one.
// ROWPAIRS (BM = 128): transfer j of a wave moves the two 128-float rows 4 wave + 2 j, + 1 instead -- the same image.
template <int BM, bool ROWPAIRS>
struct AImagePlan {
    static constexpr int NA = BM >= 96 ? 2 : 1;              // slots (the second one of waves 2, 3 is idle at BM = 96)
    const float *src[NA];                                    // this lane's 16 bytes of slot j in K step 0
    size_t step;                                             // floats between K steps: wave-uniform, so kt * step is scalar arithmetic
    int lds[NA];
    bool a1, a2;
    __device__ __forceinline__ AImagePlan(const mi_conv_desc &d, const Wg &w) {
        a1 = BM != 32 || w.wave < 2; a2 = BM == 128 || (BM == 96 && w.wave < 2);
        step = (size_t)BK * d.Mpad;
#pragma unroll
        for (int j = 0; j < NA; ++j) {
            int row, col;
            if (ROWPAIRS && BM == 128) { row = 4 * w.wave + 2 * j + w.lh; col = w.li * 4; lds[j] = (4 * w.wave + 2 * j) * BM; }
            else { const int q = j ? 4 + w.wave : w.wave, f = 256 * q + 4 * w.lane; row = f / BM; col = f % BM; lds[j] = 256 * q; }
            src[j] = d.wt + (size_t)row * d.Mpad + w.m0 + col;
        }
    }
    // transfers the calling wave has in flight per tile: the counted wait of the ring follows from it
    __device__ __forceinline__ int in_flight() const { return a2 ? 2 : a1 ? 1 : 0; }
    __device__ __forceinline__ void issue(int kt, float *sa) const {
#pragma unroll
        for (int j = 0; j < NA; ++j)
            if (j == 0 ? a1 : a2) lds_dma16_tracked(src[j] + (size_t)kt * step, sa + lds[j]);
    }
};

// ---- B: the loaders of a raw float32 activation tile [BK][BN] ----------------------------------------------------------------
// Each wave moves rows 4 wave + 2 j + lh (j = 0, 1) of every K step, 16 bytes per lane at column 4 li: two transfers per wave and
// tile (kBInFlight).  `brows` is row 4 wave of the tile image in LDS.  A loader is constructed with (d, w, N, chan), chan being the
// input channel stride (the tap loader's; the others ignore it), and offers prefetch(kt), issue(d, kt, brows), fix(d, kt, brows).
constexpr int kBInFlight = 2;

// plain (1 x 1 / linear) layers: row k is channel k, stride P; columns outside the tensor read the zero page
struct PlainRows {
    const float *src;
    size_t row2, step;
    __device__ __forceinline__ PlainRows(const mi_conv_desc &d, const Wg &w, int N, int64_t) {
        const ColInfo lc = decompose(w.n0 + w.li * 4, N, w.P, d.O2, d.O2);
        src = lc.valid ? d.x + (size_t)lc.b * d.x_bstride + lc.p + (size_t)(4 * w.wave + w.lh) * w.P : d.sink + MI_SINK_FLOATS;
        row2 = lc.valid ? (size_t)2 * w.P : 0; step = lc.valid ? (size_t)BK * w.P : 0;
    }
    __device__ __forceinline__ void prefetch(int) {}
    __device__ __forceinline__ void issue(const mi_conv_desc &, int kt, float *brows) const {
        const float *g = src + (size_t)kt * step;
        lds_dma16_tracked(g, brows);
        lds_dma16_tracked(g + row2, brows + 2 * BN);
    }
    __device__ __forceinline__ void fix(const mi_conv_desc &, int, float *) const {}
};

// Shifted-run taps: stride-1 k x k convs with K2 = 3 taps along a row, step DIL between them (NT = 9: 3 x 3, NT = 3: k = 3).
// Row k = ci * NT + tap of the tile is, for 128 consecutive output positions, a run of input row ci shifted by the tap's offset
// (t1 - pad1) * pitch + (t2 * DIL - pad2) -- and global_load_lds_dwordx4 takes a source that is only 4-byte aligned
// (tools/micro/dma_unaligned.hip), so the run goes global -> LDS by DMA like a plain layer's: no staging registers, no table.
// A tap whose input ROW lies outside [0, D1), the K padding and columns past the valid width read the zero page.
// READ SLACK: a lane's 16 bytes start at its column chunk shifted by the tap, so the first chunk of the tensor's first row and
// the last chunk of its last row reach outside it: up to 8 bytes BEFORE and 20 bytes AFTER the tensor at d.x must be readable.
// The caller owns that slack (gemm_conv.h beside `ntaps`, demucs_amd.h mi_conv_forward).
// What the shift drags in at the two ends of an input row (the neighbouring row's sample, a pitch-padding column or that slack)
// is OVERWRITTEN with the conv's zero padding in LDS by fix(): by the lane that issued the transfer, after its own wait for it
// and BEFORE the barrier that publishes the tile -- at most two ds_write_b32 per lane and K step.  A zero weight would not do:
// NaN * 0 is NaN.  With DIL > 1 up to DIL samples at either end come from outside the row: the lanes that own the first chunk of
// a row and the chunks within eight columns of its valid end re-test their four elements per tap (a rare branch) instead.
template <int NT, int DIL>
struct TapRows {
    static constexpr int K2 = 3;                             // NT = 9 or 3: divisions by constants
    ColInfo lc;
    const float *xcol;
    int64_t chan;
    int x_ld, rb0, lofs, fix_l, fix_r;
    bool edge;
    __device__ __forceinline__ TapRows(const mi_conv_desc &d, const Wg &w, int N, int64_t chan_stride) {
        lc = decompose(w.n0 + w.li * 4, N, w.P, d.O2, w.o2v);
        x_ld = d.x_ld ? d.x_ld : d.D2;
        chan = chan_stride;
        rb0 = 4 * w.wave + w.lh; lofs = w.lh * BN + w.li * 4;
        xcol = d.x + (size_t)lc.b * d.x_bstride + (size_t)lc.o1 * x_ld + lc.o2;
        // elements of this lane's 4-column chunk that a tap with d2 = -1 / +1 reads from outside the input row [0, D2)
        fix_l = (lc.valid && lc.o2 == 0) ? 0 : -1;
        const int fr = d.D2 - 1 - lc.o2;
        fix_r = (lc.valid && fr >= 0 && fr < 4) ? fr : -1;
        edge = lc.valid && (lc.o2 < 4 || lc.o2 + 8 > d.D2);   // DIL > 1: chunks that can hold an element from outside [0, D2)
    }
    __device__ __forceinline__ void prefetch(int) {}
    // row k of this lane's transfer j of K step kt; stated non-negative, so that the divisions by NT and K2 stay unsigned multiplies
    __device__ __forceinline__ int row_k(int kt, int j) const {
        const int k = kt * BK + rb0 + 2 * j;
        __builtin_assume(k >= 0);
        return k;
    }
    __device__ __forceinline__ void issue(const mi_conv_desc &d, int kt, float *brows) const {
        // both arms of the source select are plain locals: hipcc then emits a select; around a member or an expression it emits a
        // branch, sinks the address arithmetic into it and keeps the branch (2 % slower on the 3 x 3 convs)
        const float *const zero = d.sink + MI_SINK_FLOATS;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int k = row_k(kt, j), ci = k / NT, tap = k - ci * NT, t1 = tap / K2, t2 = tap - t1 * K2;
            const int i1 = lc.o1 + t1 - d.tap_pad1;
            const bool ok = lc.valid && k < d.K && (unsigned)i1 < (unsigned)d.D1;
            const float *g = xcol + (int64_t)ci * chan + (int64_t)(t1 - d.tap_pad1) * x_ld + (t2 * DIL - d.tap_pad2);
            lds_dma16_tracked(ok ? g : zero, brows + 2 * j * BN);
        }
    }
    __device__ __forceinline__ void fix(const mi_conv_desc &d, int kt, float *brows) const {
        float *sb = brows + lofs;
        if constexpr (DIL == 1) {
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int k = row_k(kt, j), tap = k % NT, dd2 = tap % K2 - d.tap_pad2;
                if (dd2 < 0 && fix_l >= 0) sb[2 * j * BN + fix_l] = 0.f;
                if (dd2 > 0 && fix_r >= 0) sb[2 * j * BN + fix_r] = 0.f;
            }
        } else if (edge) {
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int k = row_k(kt, j), tap = k % NT, dd2 = (tap % K2) * DIL - d.tap_pad2;
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if ((unsigned)(lc.o2 + e + dd2) >= (unsigned)d.D2) sb[2 * j * BN + e] = 0.f;
            }
        }
    }
};

// Row taps: layers whose taps move along ROWS only (every table entry has d2 == 0, S2 == 1).  Row k of the tile is a run of input
// row i1 = o1 * S1 + d1 at the SAME columns as the output tile, 16-byte chunks at aligned positions: no shifted runs, no fix-up,
// never an address outside the tensor (a tap whose row lies outside [0, D1), a column past the end and the K padding, d1 = -2^29,
// read the zero page).  (off, d1) of this wave's four rows come from the gather table into SGPRs by SCALAR loads in inline asm:
// hipcc turns uniform loads into VMEM loads inside the loop (the DMA builtins count as stores that might alias the table) and
// then waits vmcnt(0) for them, which drains the transfer ring every K step; as compiler-visible scalar loads its lgkmcnt
// bookkeeping would not know of the ring.  In asm they count with lgkmcnt, so the counted vmcnt waits of the ring stay exact.
#define MI_ROW_LOADS "s_load_dwordx2 %0, %4, 0x0\n\ts_load_dwordx2 %1, %4, 0x10\n\ts_load_dwordx2 %2, %4, 0x20\n\t" \
                     "s_load_dwordx2 %3, %4, 0x30\n\t"
struct RowTaps {
    typedef int v2i __attribute__((ext_vector_type(2)));
    const float *xcol;
    const int4 *ktab4;                                       // (off, d1, d2, ci) of this wave's four rows of K step 0
    int i1b, lh;
    bool valid;
    v2i e0, e1, e2, e3;
    __device__ __forceinline__ RowTaps(const mi_conv_desc &d, const Wg &w, int N, int64_t) {
        const ColInfo lc = decompose(w.n0 + w.li * 4, N, w.P, d.O2, w.o2v);
        valid = lc.valid; lh = w.lh;
        i1b = lc.o1 * d.S1;                                  // the input row of tap d1 = 0
        xcol = d.x + (size_t)lc.b * d.x_bstride + (size_t)i1b * (d.x_ld ? d.x_ld : d.D2) + lc.o2;
        ktab4 = reinterpret_cast<const int4 *>(d.ktab) + 4 * w.wave;
    }
    // the entries of K step kt; DRAIN: the same statement also waits for every transfer of the wave (gemm_x6.hip's end of step)
    template <bool DRAIN = false>
    __device__ __forceinline__ void prefetch(int kt) {
        if constexpr (DRAIN)
            asm volatile(MI_ROW_LOADS "s_waitcnt vmcnt(0) lgkmcnt(0)" : "=&s"(e0), "=&s"(e1), "=&s"(e2), "=&s"(e3) : "s"(ktab4 + kt * BK) : "memory");
        else
            asm volatile(MI_ROW_LOADS "s_waitcnt lgkmcnt(0)" : "=&s"(e0), "=&s"(e1), "=&s"(e2), "=&s"(e3) : "s"(ktab4 + kt * BK) : "memory");
    }
    __device__ __forceinline__ void issue(const mi_conv_desc &d, int, float *brows) const {
        const float *const zero = d.sink + MI_SINK_FLOATS;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int off = j ? (lh ? e3.x : e2.x) : (lh ? e1.x : e0.x), dd1 = j ? (lh ? e3.y : e2.y) : (lh ? e1.y : e0.y);
            const bool ok = valid && (unsigned)(i1b + dd1) < (unsigned)d.D1;
            lds_dma16_tracked(ok ? xcol + off : zero, brows + 2 * j * BN);
        }
    }
    __device__ __forceinline__ void fix(const mi_conv_desc &, int, float *) const {}
};
#undef MI_ROW_LOADS

// Time-axis transposed conv (ConvTranspose1d k = 8, s = 4 as a two-tap GEMM; the caller vouches with `dma_time`): D1 = O1 = 1, the
// columns are q = 0 .. D2 on a row pitch O2 % 4 == 0 (o2_valid = D2 + 1, so a lane's 4-column chunk never straddles two items), and
// row k = 2 ci + j of the tile is the run of channel ci at the tile's columns shifted by -j: TapRows with two taps at offsets 0 and
// -1.  The parity of a lane's rows 4 wave + 2 j + lh is lh, so a lane serves ONE tap: lh = 0 the run at q, lh = 1 the run at q - 1.
// READ SLACK: the chunk at q = 0 of tap 1 starts 4 bytes BEFORE its channel, and the chunk that holds q = D2 ends up to 16 bytes
// AFTER it (pitch == D2): that much must be readable around the tensor at d.x (gemm_conv.h beside `dma_time`).
// fix() writes the conv's zeros over what the runs drag in (a zero weight would not do: NaN * 0 is NaN): sample -1 (tap 1 of q = 0:
// the previous channel's last element or the slack) and samples >= D2 (tap 0 of q = D2, both taps of the padded columns: the pitch
// padding, the next channel's first samples or the slack) -- only the lanes of the first chunk of an item and of the chunk
// around its valid end take the branch.  The K padding and columns past N read the zero page.
struct TimeTrTaps {
    const float *xcol;                                       // this lane's 16 bytes of channel 0, shifted by its tap
    int64_t chan;
    int ci0, q0, tap, lofs;
    bool valid, edge;
    __device__ __forceinline__ TimeTrTaps(const mi_conv_desc &d, const Wg &w, int N, int64_t) {
        const ColInfo lc = decompose(w.n0 + w.li * 4, N, w.P, d.O2, w.o2v);
        valid = lc.valid; q0 = lc.o2; tap = w.lh;
        chan = d.x_ld ? d.x_ld : d.D2;
        ci0 = 2 * w.wave; lofs = w.lh * BN + w.li * 4;
        xcol = d.x + (size_t)lc.b * d.x_bstride + lc.o2 - w.lh;
        edge = valid && (q0 == 0 || q0 + 4 > d.D2);
    }
    __device__ __forceinline__ void prefetch(int) {}
    __device__ __forceinline__ void issue(const mi_conv_desc &d, int kt, float *brows) const {
        const float *const zero = d.sink + MI_SINK_FLOATS;   // both arms plain locals: a select, not a branch (TapRows::issue)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int ci = kt * (BK / 2) + ci0 + j;
            const bool ok = valid && 2 * ci < d.K;
            const float *g = xcol + (int64_t)ci * chan;
            lds_dma16_tracked(ok ? g : zero, brows + 2 * j * BN);
        }
    }
    __device__ __forceinline__ void fix(const mi_conv_desc &d, int, float *brows) const {
        if (!edge) return;
        float *sb = brows + lofs;
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if ((unsigned)(q0 + e - tap) >= (unsigned)d.D2) sb[2 * j * BN + e] = 0.f;
    }
};

// Time-axis strided conv (Conv1d k = 8, s = 4, pad 2; the caller vouches with `dma_time`): D1 = O1 = 1, K ordered (ci, t), column o
// reads samples 4 o - 2 .. 4 o + 5 of channel ci -- eight CONSECUTIVE floats, so a K step of 16 (two channels) is, per column, two
// runs of 32 bytes, each landed as two 16-byte chunks from a source that is 8 bytes off 16-byte alignment (the DMA takes 4-byte-aligned
// sources).  Every column owns its eight floats: taps 4 .. 7 are landed again for the next column (from the caches), so nothing is
// shared with a neighbour and the last column of a row, of an item or of the tile needs no special case.
// The raw stage is not the [16][128] image of the other loaders but [channel 2][chunk 2][column 128][4 floats]: one transfer of a
// wave lands one chunk of 64 consecutive columns (16 bytes per lane, LDS addresses consecutive), and the thread that owns (column,
// k-half = channel) reads its taps as two conflict-free 16-byte reads (read()).  Wave w moves chunk w >> 1 of columns
// [64 (w & 1), + 64) for both channels: two transfers per wave and tile, as every loader.
// READ SLACK: column 0 starts at sample -2 and the last valid column ends at sample 4 o2_valid + 1 <= D2 + 4: up to 8 bytes BEFORE
// the tensor at d.x and up to 20 bytes AFTER it (8 with a row pitch of 4 o2_valid floats) must be readable (gemm_conv.h beside
// `dma_time`).
// fix(): the lane that issued a chunk overwrites, after its own wait, the samples outside [0, D2) with the conv's zero padding
// (samples -2, -1: the previous channel's end or the slack; samples >= D2: the pitch padding, the next channel's start or the
// slack).  Channels past Cin (the K padding of an odd Cin), columns past o2_valid and past N read the zero page.
struct TimeEncTaps {
    const float *xcol;                                       // sample 4 o - 2 + 4 chunk of channel 0 at this lane's column
    int64_t chan;
    int s0, lofs, wbase;
    bool valid, edge;
    __device__ __forceinline__ TimeEncTaps(const mi_conv_desc &d, const Wg &w, int N, int64_t) {
        const int half = w.wave & 1, chunk = w.wave >> 1, col = 64 * half + w.lane;
        const ColInfo lc = decompose(w.n0 + col, N, w.P, d.O2, w.o2v);
        valid = lc.valid;
        s0 = 4 * lc.o2 - 2 + 4 * chunk;
        chan = d.x_ld ? d.x_ld : d.D2;
        xcol = d.x + (size_t)lc.b * d.x_bstride + s0;
        wbase = (chunk * BN + 64 * half) * 4; lofs = wbase + 4 * w.lane;
        edge = valid && (s0 < 0 || s0 + 3 >= d.D2);
    }
    __device__ __forceinline__ void prefetch(int) {}
    // `stage`: the raw stage itself (not a wave's rows of it)
    __device__ __forceinline__ void issue(const mi_conv_desc &d, int kt, float *stage) const {
        const float *const zero = d.sink + MI_SINK_FLOATS;   // both arms plain locals: a select, not a branch (TapRows::issue)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int ci = 2 * kt + j;
            const bool ok = valid && 8 * ci < d.K;
            const float *g = xcol + (int64_t)ci * chan;
            lds_dma16_tracked(ok ? g : zero, stage + j * (2 * BN * 4) + wbase);
        }
    }
    __device__ __forceinline__ void fix(const mi_conv_desc &d, int, float *stage) const {
        if (!edge) return;
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if ((unsigned)(s0 + e) >= (unsigned)d.D2) stage[j * (2 * BN * 4) + lofs + e] = 0.f;
    }
    // the eight taps of column bn, channel bh of the K step
    static __device__ __forceinline__ void read(const float *stage, int bn, int bh, float (&v)[8]) {
        const float4 a = *reinterpret_cast<const float4 *>(stage + ((2 * bh) * BN + bn) * 4);
        const float4 b = *reinterpret_cast<const float4 *>(stage + ((2 * bh + 1) * BN + bn) * 4);
        v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
    }
};

// NT: 0 plain, kRowTaps row taps, kTimeTr / kTimeEnc the time-axis transposed / strided conv, 9 or 3 shifted-run taps
template <int NT, int DIL = 1>
using BLoader = std::conditional_t<NT == 0, PlainRows, std::conditional_t<NT == kRowTaps, RowTaps, std::conditional_t<NT == kTimeTr, TimeTrTaps,
                                   std::conditional_t<NT == kTimeEnc, TimeEncTaps, TapRows<(NT > 0 ? NT : 3), DIL>>>>>;

// ---- host: launch geometry -----------------------------------------------------------------------------------------------------
// N output columns in NT tiles of `bn`, MT row tiles of `tile`; Mpad must be a multiple of `image_rows` (the tile, or the rows of the
// weight image it reads).  `what` names the kernel family in the messages.  The bound keeps every column index n0 + 255 in an int.
struct ConvGeom { int N, MT, NT; };
static inline int conv_geom(const mi_conv_desc &d, const char *what, int tile, int image_rows, ConvGeom &g, int bn = BN) {
    const int64_t N64 = (int64_t)d.B * d.O1 * d.O2;
    MI_REQUIRE(N64 < (1ll << 31) - 256, "%s: too many output positions (%lld)", what, (long long)N64);
    MI_REQUIRE(d.Mpad % image_rows == 0, "%s: Mpad %d not a multiple of the %d-row tile", what, d.Mpad, tile);
    g.N = (int)N64; g.MT = d.Mpad / tile; g.NT = ceil_div(g.N, bn);
    return MI_OK;
}
// launch on the XCD-grouped grid (tile_of_block) with 256 threads
#define MI_LAUNCH_TILES(kernel, d, g, Gm, st)                                                                          \
    do {                                                                                                          \
        hipLaunchKernelGGL(kernel, dim3(grouped_grid((g).MT, (g).NT, (Gm))), dim3(256), 0, (st), (d), (g).N, (g).MT, (Gm)); \
        MI_CHECK_LAUNCH();                                                                                        \
    } while (0)

}  // namespace mi
