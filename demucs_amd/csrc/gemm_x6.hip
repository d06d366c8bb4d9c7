// Implicit-GEMM convolution with fp32 operands carried as THREE bf16 terms each (x = hi + mid + lo, exact: 3 x 8
// mantissa bits = the 24 of fp32) and SIX bf16 MFMA products accumulated in fp32:
//
//     a*b  ~=  ah*bh + ah*bm + am*bh + am*bm + ah*bl + al*bh          (dropped terms <= 2^-24 |a b|)
//
// Every product of two bf16 values is exact in fp32 and v_mfma_f32_32x32x16_bf16 accumulates in fp32, so the
// result carries the same ~2^-24 relative rounding per term as the native fp32 MFMA path of gemm_conv.hip
// (measured against the fp64 oracle: tests/test_gpu_kernels.py::test_conv_x6_*), while the matrix pipe runs
// bf16 at 16x the fp32 rate: 6 products = 2.67x fewer matrix-pipe cycles per fp32-equivalent FLOP.
//
// Tile image in LDS, per operand and K step of 16: [part 3][k-half 2][row or column][8 bf16] -- a 32x32x16
// fragment (lane l: row l&31, k = 8*(l>>5) .. +7) is ONE conflict-free ds_read_b128 per part.
//   A (weights): split once at load time into exactly this image per (M tile, K step) (pack_split_kernel),
//                so the loader is pure LDS-DMA (global_load_lds_dwordx4, no registers, no ds_write).  Tiles: 128, 96 and 64 rows
//                on an image of their own, 64 rows on the halves of a 128-row image (HALF_IMG: under-filled 128-row layers) and
//                192 rows (WM 2, TM 3: 36 MFMAs per wave and K step behind the same split, waits and barrier) on PAIRS of
//                96-row images, for layers with M % 192 == 0 (mi_conv_desc.tile_m = 192; under-filled: the 96-row tile).
//   B (activations): thread (column n = tid & 127, k-half = tid >> 7) takes its 8 k values, splits them in registers
//                (v_cvt_pk_bf16_f32, round-to-nearest residuals) and writes three 16-byte words.  The values come from
//                the raw fp32 tile that LDS-DMA lands two K steps ahead (plain layers: channel runs; the decoders' 3 x 3 /
//                k = 3 convs, conv_tap_x6_kernel: tap-shifted runs; the frequency branch's strided and transposed convs,
//                conv_rows_x6_kernel: row taps at the output's own columns; the time branch's transposed convs,
//                conv_time_tr_x6_kernel: two runs shifted along the time axis, and strided encoder convs,
//                conv_time_enc_x6_kernel: the 8-sample run of each column), or else through the gather table of the fp32 kernel.
// Epilogues are the shared ones of gemm_tile.h (the accumulator layout of all 32x32 MFMAs is the same).
#include "gemm_loop.h"
#include "split_bf16.h"

namespace mi {

// Wt[Kpad][Mpad] fp32 -> Wx[mt][kt][part][k-half][BM rows][8] bf16
__global__ void pack_split_kernel(const float *__restrict__ wt, int Kpad, int Mpad, int BM, __bf16 *__restrict__ wx) {
    const size_t idx = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (idx >= (size_t)Kpad * Mpad) return;
    const int k = (int)(idx / Mpad), m = (int)(idx % Mpad);
    const int mt = m / BM, mi = m % BM, kt = k / BK, h = (k % BK) / 8, j = k % 8, nk = Kpad / BK;
    const float x = wt[idx];
    const __bf16 a = (__bf16)x;
    const float r = x - (float)a;
    const __bf16 b = (__bf16)r;
    const __bf16 c = (__bf16)(r - (float)b);
    __bf16 *img = wx + ((size_t)mt * nk + kt) * ((size_t)BM * 48);
    img[((0 * 2 + h) * BM + mi) * 8 + j] = a;
    img[((1 * 2 + h) * BM + mi) * 8 + j] = b;
    img[((2 * 2 + h) * BM + mi) * 8 + j] = c;
}

int launch_pack_split(const float *wt, int Kpad, int Mpad, int tile_m, void *wx, hipStream_t st) {
    MI_REQUIRE(Kpad % BK == 0 && Mpad % tile_m == 0, "pack_split: Kpad %d / Mpad %d do not fit tile %d", Kpad, Mpad, tile_m);
    const size_t n = (size_t)Kpad * Mpad;
    hipLaunchKernelGGL(pack_split_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, wt, Kpad, Mpad, tile_m, (__bf16 *)wx);
    MI_CHECK_LAUNCH();
    return MI_OK;
}

// The accumulators stay in AGPRs (gemm_loop.h agpr_anchor).
// HALF_IMG: a 64-row tile that reads its rows out of the 128-row weight image (the small-batch tile of the plain linear
// layers, of the tap and of the row-tap convs: conv_route): the same fragments, products and k order as the 128-row tile, so both give
// bit-identical results.
// NT: the loader of the raw activation tile (gemm_loop.h BLoader), which lands in the braw ring two K steps ahead and is split from
// LDS by the same code whatever the loader.  0 with PLAIN: channel runs.  9 or 3 (conv_tap_x6_kernel): the shifted-run taps of the
// float32 decoders' stride-1 3 x 3 / k = 3 rewrite convs, dilation 1, channel stride P; the k order is the packed weights' one, so
// the split image is pack_split's as for any layer.  kRowTaps (conv_rows_x6_kernel): the frequency branch's encoder convs k = 8,
// s = 4 and transposed convs as two-tap GEMMs, rows q and q - 1, and the encoders' 1 x 1 + GLU rewrites, whose table is the
// identity.  Their table entries of K step kt + 3 are loaded in the same asm statement as the end-of-step vmcnt(0) wait and
// counted with lgkmcnt(0) there: their latency passes under the wait for the ring.  kTimeTr (conv_time_tr_x6_kernel): the time
// branch's transposed convs as two-tap GEMMs along the contiguous axis, columns q and q - 1 (gemm_loop.h TimeTrTaps).  kTimeEnc
// (conv_time_enc_x6_kernel): its strided encoder convs k = 8, s = 4, + GELU (gemm_loop.h TimeEncTaps: a stage layout of its own).
template <int WM, int WN, int TM, int TN, int EPI, int LFLAGS, bool PLAIN, bool HALF_IMG, int NT>
__device__ __forceinline__ void conv_x6_body(const mi_conv_desc &d, const int N, const int MT, const int Gm) {
    constexpr int BM = WM * TM * 32;
    constexpr bool RAW = PLAIN || NT != 0;                   // the activation tile goes through the braw ring
    constexpr bool ROWS = NT == kRowTaps;
    static_assert(NT <= 0 || (!PLAIN && EPI == MI_EPI_GLU), "tap loader: GLU rewrite convs");
    static_assert(!ROWS || (!PLAIN && (EPI == MI_EPI_LINEAR || EPI == MI_EPI_CONVTR || EPI == MI_EPI_GLU)),
                  "row-tap loader: encoder / transposed convs, 1 x 1 + GLU rewrites");
    static_assert(NT != kTimeTr || (!PLAIN && EPI == MI_EPI_CONVTR), "time-axis two-tap loader: transposed convs");
    static_assert(NT != kTimeEnc || (!PLAIN && EPI == MI_EPI_LINEAR && LFLAGS == MI_FLAG_GELU), "time-axis strided loader: encoder convs");
    static_assert(NT >= kTimeEnc, "NT: taps, 0, kRowTaps, kTimeTr or kTimeEnc");
    static_assert(WN * TN * 32 == BN, "block N tile is 128");
    static_assert(WM * WN == 4, "4 waves");
    constexpr int A_BYTES = BM * 96, B_BYTES = BN * 96, STAGE = A_BYTES + B_BYTES;
    constexpr int A_CHUNKS = A_BYTES / 1024;                 // 1 KiB per wave-wide DMA instruction
    static_assert(!HALF_IMG || BM == 64, "HALF_IMG: 64-row tile of a 128-row image");
    // PAIR: the 192-row tile (WM 2, TM 3).  Wave row wm owns rows [96 wm, 96 wm + 96), so the tile reads the two consecutive
    // 96-row images 2 mt and 2 mt + 1 of pack_split_kernel's layout (nine 1 KiB chunks each per K step) and keeps them one after the
    // other in LDS: the same fragments, products and k order as the 96-row tile on that image, so both give bit-identical results
    constexpr bool PAIR = BM == 192;
    static_assert(!PAIR || (WM == 2 && TM == 3), "192-row tile: two wave rows of 96 rows");
    constexpr int IMG_ROWS = PAIR ? 96 : BM, IMG_BYTES = IMG_ROWS * 96, IMG_CHUNKS = IMG_BYTES / 1024;
    // one K step of the image: [part 3][k-half 2][image rows][16 bytes]; the 64-row half of a 128-row image is the first or the
    // second KiB of each 2 KiB (part, k-half) block
    constexpr int A_KSTEP = HALF_IMG ? 2 * A_BYTES : IMG_BYTES, A_CHUNK_STRIDE = HALF_IMG ? 2048 : 1024;
    __shared__ __attribute__((aligned(16))) unsigned char smem[2 * STAGE];
    // plain layers: the fp32 activation tile [16][128] lands here by LDS-DMA two K steps ahead and is split from LDS
    // (a VMEM wave-instruction costs ~12-16 cycles whatever its width: 2 x 1 KiB DMA per wave replace 8 dword loads)
    __shared__ __attribute__((aligned(16))) float braw[RAW ? 2 * BK * BN : 4];

    agpr_anchor();
    Wg w;
    if (!wg_tile<WN, BM>(d, MT, Gm, N, w)) return;
    const int nk = d.Kpad / BK;

    // ---- A: LDS-DMA of the pre-split image; wave w moves chunks w, w + 4, ... -------------------------
    const unsigned char *aimg = reinterpret_cast<const unsigned char *>(d.wx) + (size_t)(HALF_IMG ? w.mt >> 1 : PAIR ? 2 * w.mt : w.mt) * nk * A_KSTEP +
                                (HALF_IMG ? (w.mt & 1) * 1024 : 0) + w.lane * 16;
#define MI_A_DMA(kt, stage)                                                                                         \
    do {                                                                                                            \
        _Pragma("unroll") for (int c = 0; c < (A_CHUNKS + 3) / 4; ++c) {                                             \
            const int chunk = c * 4 + w.wave, img = PAIR ? chunk / IMG_CHUNKS : 0, ic = chunk - img * IMG_CHUNKS;      \
            if (chunk < A_CHUNKS)                                                                                   \
                lds_dma16_tracked(aimg + ((size_t)img * nk + (kt)) * A_KSTEP + ic * A_CHUNK_STRIDE,                    \
                                  smem + (stage) * STAGE + chunk * 1024);                                          \
        }                                                                                                           \
    } while (0)

    // ---- B: this thread owns column bn and the 8 k values of k-half bh ----------------------------------
    const int bn = w.tid & 127;
    const int bh = __builtin_amdgcn_readfirstlane(w.tid >> 7);
    const ColInfo lc = decompose(w.n0 + bn, N, w.P, d.O2, PLAIN ? d.O2 : w.o2v);
    const int i1b = lc.o1 * d.S1, i2b = lc.o2 * d.S2;
    const float *xcol = d.x + (size_t)lc.b * d.x_bstride + (PLAIN ? (size_t)lc.p : (size_t)i1b * (d.x_ld ? d.x_ld : d.D2) + i2b);
    const float *bp = lc.valid ? xcol + (size_t)(8 * bh) * w.P : d.sink + MI_SINK_FLOATS;     // plain: channel stride = P
    const size_t b_row = lc.valid ? (size_t)w.P : 0, b_step = lc.valid ? (size_t)BK * w.P : 0;
    float breg[8];
    // RAW: this wave's rows 4 wave .. 4 wave + 3 of the raw tile, by the loader NT selects; raw stage rs
    BLoader<NT> L(d, w, N, w.P);
    // (the time-axis strided loader lays the stage out itself and takes the stage, not the wave's rows: gemm_loop.h TimeEncTaps)
    constexpr bool OWN_STAGE = NT == kTimeEnc;
#define MI_BRAW_DMA(kt, rs) L.issue(d, (kt), braw + (rs) * (BK * BN) + (OWN_STAGE ? 0 : 4 * w.wave) * BN)
// taps: after this wave's wait for its transfers of tile kt, before the barrier (gemm_loop.h TapRows)
#define MI_BRAW_FIX(kt, rs) L.fix(d, (kt), braw + (rs) * (BK * BN) + (OWN_STAGE ? 0 : 4 * w.wave) * BN)
#define MI_BRAW_READ(rs)                                                                                            \
    do {                                                                                                            \
        if constexpr (OWN_STAGE) {                                                                                  \
            L.read(braw + (rs) * (BK * BN), bn, bh, breg);                                                          \
        } else {                                                                                                    \
            _Pragma("unroll") for (int j = 0; j < 8; ++j) breg[j] = braw[(rs) * (BK * BN) + (8 * bh + j) * BN + bn]; \
        }                                                                                                           \
    } while (0)

#define MI_B_LOAD(kt)                                                                                               \
    do {                                                                                                            \
        if (PLAIN) {                                                                                                \
            _Pragma("unroll") for (int j = 0; j < 8; ++j) breg[j] = bp[(size_t)(kt) * b_step + j * b_row];           \
        } else {                                                                                                    \
            mi_ktab_entry ke[8];                                                                                    \
            _Pragma("unroll") for (int j = 0; j < 8; ++j) ke[j] = d.ktab[(kt) * BK + 8 * bh + j];                    \
            _Pragma("unroll") for (int j = 0; j < 8; ++j) {                                                          \
                bool ok;                                                                                            \
                const float v = gather_b(d, ke[j], xcol, i1b, i2b, lc.valid, ok);                                   \
                breg[j] = ok ? v : 0.f;                                                                             \
            }                                                                                                       \
        }                                                                                                           \
    } while (0)

#define MI_B_STORE(stage)                                                                                           \
    do {                                                                                                            \
        unsigned ph[4], pm[4], pl[4];                                                                               \
        _Pragma("unroll") for (int j = 0; j < 4; ++j) split3(breg[2 * j], breg[2 * j + 1], ph[j], pm[j], pl[j]);    \
        unsigned char *bs = smem + (stage) * STAGE + A_BYTES + (bh * BN + bn) * 16;                                 \
        *reinterpret_cast<uint4 *>(bs) = make_uint4(ph[0], ph[1], ph[2], ph[3]);                                    \
        *reinterpret_cast<uint4 *>(bs + 2 * BN * 16) = make_uint4(pm[0], pm[1], pm[2], pm[3]);                      \
        *reinterpret_cast<uint4 *>(bs + 4 * BN * 16) = make_uint4(pl[0], pl[1], pl[2], pl[3]);                      \
    } while (0)

    f32x16 acc[TM][TN];
    zero_acc(acc);

    // the six products, smallest terms first
    constexpr int PA[6] = {2, 0, 1, 1, 0, 0}, PB[6] = {0, 2, 1, 0, 1, 0};
    MI_A_DMA(0, 0);
    if constexpr (RAW) {
        L.prefetch(0);
        MI_BRAW_DMA(0, 0);
        if (nk > 1) {
            L.prefetch(1);
            MI_BRAW_DMA(1, 1);
        }
        if (nk > 2) L.prefetch(2);                                    // row taps: for the transfer of tile 2 in step 0
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        MI_BRAW_FIX(0, 0);
        if (nk > 1) MI_BRAW_FIX(1, 1);
        __syncthreads();
        MI_BRAW_READ(0);
    } else {
        MI_B_LOAD(0);
    }
    MI_B_STORE(0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    int cur = 0;
    for (int kt = 0; kt < nk; ++kt) {
        // All fragment reads of this K step are ISSUED before the loads of the next one: hipcc orders every ds_read
        // behind pending LDS-DMA with s_waitcnt vmcnt(0) (it cannot tell the ring stages apart), which would
        // otherwise make each step wait for the loads it has just issued.
        const unsigned char *As = smem + cur * STAGE, *Bs = As + A_BYTES;
        bf16x8 af[TM][3], bf[TN][3];
#pragma unroll
        for (int p = 0; p < 3; ++p) {
#pragma unroll
            for (int a = 0; a < TM; ++a)
                af[a][p] = *reinterpret_cast<const bf16x8 *>(As + (PAIR ? w.wm * IMG_BYTES : 0) +
                                                             (((p * 2 + w.lh) * IMG_ROWS) + ((PAIR ? 0 : w.wm * TM) + a) * 32 + w.li) * 16);
#pragma unroll
            for (int b = 0; b < TN; ++b)
                bf[b][p] = *reinterpret_cast<const bf16x8 *>(Bs + (((p * 2 + w.lh) * BN) + (w.wn * TN + b) * 32 + w.li) * 16);
        }
        __builtin_amdgcn_sched_barrier(0);
        if (kt + 1 < nk) {
            MI_A_DMA(kt + 1, cur ^ 1);
            if constexpr (RAW) {
                if (kt + 2 < nk) MI_BRAW_DMA(kt + 2, kt & 1);   // raw stage kt & 1 was consumed during step kt - 1
            } else {
                MI_B_LOAD(kt + 1);
            }
        }
        if constexpr (RAW) {
            // landed and fenced by the barrier that ended step kt - 1.  Unconditional (the last step re-splits a stale
            // tile into the unused stage) so that split and MFMAs share one basic block and can be interleaved.
            MI_BRAW_READ((kt + 1) & 1);
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int q = 0; q < 6; ++q)
#pragma unroll
            for (int a = 0; a < TM; ++a)
#pragma unroll
                for (int b = 0; b < TN; ++b)
                    acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[a][PA[q]], bf[b][PB[q]], acc[a][b], 0, 0, 0);
        if (RAW || kt + 1 < nk) MI_B_STORE(cur ^ 1);
        if constexpr (RAW) {
            // the split of the next activation tile (~70 VALU) issues in the shadow of this step's MFMAs
#pragma unroll
            for (int i = 0; i < 6 * TM * TN; ++i) {
                __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                __builtin_amdgcn_sched_group_barrier(0x002, (72 + 6 * TM * TN - 1) / (6 * TM * TN), 0);
            }
        }
        // this wave's share of the next A image / raw tile has landed (row taps: and the table entries of tile kt + 3, which
        // step kt + 1 transfers, are in SGPRs)
        if constexpr (ROWS) {
            if (kt + 3 < nk) L.template prefetch<true>(kt + 3);
            else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        } else {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        if (kt + 2 < nk) MI_BRAW_FIX(kt + 2, kt & 1);
        __syncthreads();
        cur ^= 1;
    }
#undef MI_A_DMA
#undef MI_B_LOAD
#undef MI_BRAW_DMA
#undef MI_BRAW_FIX
#undef MI_BRAW_READ
#undef MI_B_STORE

    conv_epilogue<TM, TN, EPI, LFLAGS>(d, acc, w.m0, w.n0, w.wm, w.wn, N, w.P, w.o2v);
}

template <int WM, int WN, int TM, int TN, int EPI, int LFLAGS, bool PLAIN, bool HALF_IMG = false>
__global__ __launch_bounds__(256, 2) void conv_gemm_x6_kernel(const mi_conv_desc d, const int N, const int MT, const int Gm) {
    conv_x6_body<WM, WN, TM, TN, EPI, LFLAGS, PLAIN, HALF_IMG, 0>(d, N, MT, Gm);
}

// the float32 decoders' rewrite convs: a symbol of their own, so that profiles keep them apart from the linears
template <int WM, int WN, int TM, int TN, bool HALF_IMG, int NT>
__global__ __launch_bounds__(256, 2) void conv_tap_x6_kernel(const mi_conv_desc d, const int N, const int MT, const int Gm) {
    conv_x6_body<WM, WN, TM, TN, MI_EPI_GLU, 0, false, HALF_IMG, NT>(d, N, MT, Gm);
}

// the float32 row-tap layers (frequency encoder / transposed convs, 1 x 1 + GLU rewrites): a symbol of their own, as the tap convs
template <int WM, int WN, int TM, int TN, int EPI, int LFLAGS, bool HALF_IMG>
__global__ __launch_bounds__(256, 2) void conv_rows_x6_kernel(const mi_conv_desc d, const int N, const int MT, const int Gm) {
    conv_x6_body<WM, WN, TM, TN, EPI, LFLAGS, false, HALF_IMG, kRowTaps>(d, N, MT, Gm);
}

// the float32 time-branch transposed convs (two shifted runs along the time axis): a symbol of their own, as the tap convs
template <int WM, int WN, int TM, int TN, bool HALF_IMG>
__global__ __launch_bounds__(256, 2) void conv_time_tr_x6_kernel(const mi_conv_desc d, const int N, const int MT, const int Gm) {
    conv_x6_body<WM, WN, TM, TN, MI_EPI_CONVTR, 0, false, HALF_IMG, kTimeTr>(d, N, MT, Gm);
}

// ... and its strided encoder convs (k = 8, s = 4, + GELU: 8-sample runs per column)
template <int WM, int WN, int TM, int TN, bool HALF_IMG>
__global__ __launch_bounds__(256, 2) void conv_time_enc_x6_kernel(const mi_conv_desc d, const int N, const int MT, const int Gm) {
    conv_x6_body<WM, WN, TM, TN, MI_EPI_LINEAR, MI_FLAG_GELU, false, HALF_IMG, kTimeEnc>(d, N, MT, Gm);
}

template <int WM, int WN, int TM, int TN, int EPI, int LFLAGS, bool PLAIN, bool HALF_IMG = false, int NTAPS = 0>
static int launch_cfg_x6(const mi_conv_desc &d, hipStream_t st) {
    constexpr int BM = WM * TM * 32;
    ConvGeom g;
    MI_TRY(conv_geom(d, "conv", BM, HALF_IMG ? 2 * BM : BM, g));
    const int Gm = pick_m_groups(g.MT, (size_t)d.Kpad * d.Mpad * 6);
    if constexpr (NTAPS > 0) MI_LAUNCH_TILES((conv_tap_x6_kernel<WM, WN, TM, TN, HALF_IMG, NTAPS>), d, g, Gm, st);
    else if constexpr (NTAPS == kRowTaps) MI_LAUNCH_TILES((conv_rows_x6_kernel<WM, WN, TM, TN, EPI, LFLAGS, HALF_IMG>), d, g, Gm, st);
    else if constexpr (NTAPS == kTimeTr) MI_LAUNCH_TILES((conv_time_tr_x6_kernel<WM, WN, TM, TN, HALF_IMG>), d, g, Gm, st);
    else if constexpr (NTAPS == kTimeEnc) MI_LAUNCH_TILES((conv_time_enc_x6_kernel<WM, WN, TM, TN, HALF_IMG>), d, g, Gm, st);
    else MI_LAUNCH_TILES((conv_gemm_x6_kernel<WM, WN, TM, TN, EPI, LFLAGS, PLAIN, HALF_IMG>), d, g, Gm, st);
    return MI_OK;
}

// `tile` is the tile conv_route decided, `image_tile` the one the split image was packed for: they differ for the
// under-filled 128-row layers, which run 64-row tiles that read the 128-row image (bit-identical to the 128-row tile, no second
// image), and for the 192-row layers (image_tile 96), which run the 192-row tile on pairs of their 96-row images or, under-filled,
// the 96-row tile.  NTAPS: the loader (0: plain / gather table, 9 or 3: shifted-run taps, kRowTaps: row taps, kTimeTr / kTimeEnc:
// time-axis transposed / strided conv)
template <int EPI, int LFLAGS, bool PLAIN, int NTAPS>
static int launch_tile_x6(const mi_conv_desc &d, int tile, int image_tile, hipStream_t st) {
    if (tile != image_tile) {
        if constexpr (NTAPS != 0 || (PLAIN && EPI == MI_EPI_LINEAR)) {
            if (tile == 64 && image_tile == 128) return launch_cfg_x6<1, 4, 2, 1, EPI, LFLAGS, PLAIN, true, NTAPS>(d, st);
        }
        // the 192-row tile on a pair of 96-row images: the loaders' own epilogues, and the plain LINEAR layer on LayerNorm-ed tokens
        if constexpr (conv_x6_tile192(EPI, LFLAGS, PLAIN, NTAPS)) {
            if (tile == 192 && image_tile == 96) return launch_cfg_x6<2, 2, 3, 2, EPI, LFLAGS, PLAIN, false, NTAPS>(d, st);
        }
        return set_error(MI_EINVAL, "conv x6: no %d-row tile on a %d-row image for epilogue %d", tile, image_tile, EPI);
    }
    switch (tile) {
        case 128: return launch_cfg_x6<2, 2, 2, 2, EPI, LFLAGS, PLAIN, false, NTAPS>(d, st);
        case 96: return launch_cfg_x6<1, 4, 3, 1, EPI, LFLAGS, PLAIN, false, NTAPS>(d, st);
        case 64:
            if constexpr (NTAPS == 0) return launch_cfg_x6<1, 4, 2, 1, EPI, LFLAGS, PLAIN>(d, st);
    }
    return set_error(MI_EINVAL, "conv x6: unsupported tile_m %d", tile);
}

// d has been validated by launch_conv (gemm_conv.hip): a stride-1 GLU conv with K2 = 3, dilation 1, NT = 9 or 3 taps, its row
// pitch a multiple of 4 and equal to O2, image tile 96 or 128 (dmatap_eligible)
int launch_conv_tap_x6(const mi_conv_desc &d, int tile, int image_tile, hipStream_t st) {
    MI_REQUIRE(d.wx && ((uintptr_t)d.wx & 15) == 0, "conv tap x6: split weight image missing or misaligned");
    MI_REQUIRE(d.epi == MI_EPI_GLU && (image_tile == 96 || image_tile == 128) && (d.ntaps == 9 || d.ntaps == 3),
               "conv tap x6: GLU layer with 9 or 3 taps on a 96- or 128-row tile (epi %d, tile %d, ntaps %d)", d.epi, image_tile, d.ntaps);
    return d.ntaps == 9 ? launch_tile_x6<MI_EPI_GLU, 0, false, 9>(d, tile, image_tile, st) : launch_tile_x6<MI_EPI_GLU, 0, false, 3>(d, tile, image_tile, st);
}

// d has been validated by launch_conv (gemm_conv.hip): a float32 layer whose table moves its taps along rows only (dma_rows, or a
// plain layer's identity table), row pitch a multiple of 4 and equal to O2, S2 = 1, a 64-byte-aligned table (dmarow_eligible):
// LINEAR + GELU (the encoder convs) or CONVTR (the transposed convs; the epilogue reads its flag set at run time) on 96 or 128
// rows, 1 x 1 + GLU (the encoders' rewrites) on 128 rows -- the epilogue instantiations of conv_gemm_dmarow_kernel
int launch_conv_rows_x6(const mi_conv_desc &d, int tile, int image_tile, hipStream_t st) {
    MI_REQUIRE(d.wx && ((uintptr_t)d.wx & 15) == 0, "conv rows x6: split weight image missing or misaligned");
    MI_REQUIRE(d.ktab && ((uintptr_t)d.ktab & 63) == 0, "conv rows x6: gather table missing or misaligned");
    MI_REQUIRE(image_tile == 96 || image_tile == 128, "conv rows x6: 96- or 128-row tile (tile %d)", image_tile);
    if (d.epi == MI_EPI_CONVTR) return launch_tile_x6<MI_EPI_CONVTR, 0, false, kRowTaps>(d, tile, image_tile, st);
    if (d.epi == MI_EPI_GLU) {
        MI_REQUIRE(image_tile == 128 || d.tile_m == 192, "conv rows x6: GLU on a 128-row tile or a 192-row layer (tile %d)", image_tile);
        return launch_tile_x6<MI_EPI_GLU, 0, false, kRowTaps>(d, tile, image_tile, st);
    }
    MI_REQUIRE(d.epi == MI_EPI_LINEAR && (d.flags & (MI_FLAG_GELU | MI_FLAG_SCALE | MI_FLAG_RES | MI_FLAG_LN | MI_FLAG_STATS)) == MI_FLAG_GELU,
               "conv rows x6: LINEAR + GELU, CONVTR or GLU (epi %d, flags %d)", d.epi, d.flags);
    return launch_tile_x6<MI_EPI_LINEAR, MI_FLAG_GELU, false, kRowTaps>(d, tile, image_tile, st);
}

// d has been validated by launch_conv (gemm_conv.hip): a float32 1-D layer along the time axis (dma_time: D1 = O1 = 1), image tile 96
// or 128 (conv_route.hip dmatime_eligible): a transposed conv as a two-tap GEMM (columns 0 .. D2 on a pitch O2 % 4 == 0, o2_valid =
// D2 + 1; the epilogue reads its flag set at run time), or a strided conv k = 8, s = 4 + GELU
int launch_conv_time_x6(const mi_conv_desc &d, int tile, int image_tile, hipStream_t st) {
    MI_REQUIRE(d.wx && ((uintptr_t)d.wx & 15) == 0, "conv time x6: split weight image missing or misaligned");
    MI_REQUIRE((image_tile == 96 || image_tile == 128) && d.D1 == 1 && d.O1 == 1, "conv time x6: a 1-D layer on a 96- or 128-row tile (tile %d)", image_tile);
    if (d.epi == MI_EPI_CONVTR) {
        MI_REQUIRE(d.O2 % 4 == 0 && d.o2_valid == d.D2 + 1 && d.o2_valid <= d.O2 && d.K % 2 == 0,
                   "conv time x6: columns 0 .. D2 on a pitch that is a multiple of 4 (D2 %d, O2 %d, o2_valid %d)", d.D2, d.O2, d.o2_valid);
        return launch_tile_x6<MI_EPI_CONVTR, 0, false, kTimeTr>(d, tile, image_tile, st);
    }
    MI_REQUIRE(d.epi == MI_EPI_LINEAR && (d.flags & (MI_FLAG_GELU | MI_FLAG_SCALE | MI_FLAG_RES | MI_FLAG_LN | MI_FLAG_STATS)) == MI_FLAG_GELU &&
               d.S2 == 4 && d.K % 8 == 0, "conv time x6: CONVTR, or LINEAR + GELU with k = 8, s = 4 (epi %d, flags %d, S2 %d)", d.epi, d.flags, d.S2);
    return launch_tile_x6<MI_EPI_LINEAR, MI_FLAG_GELU, false, kTimeEnc>(d, tile, image_tile, st);
}

// d has been validated by launch_conv (gemm_conv.hip); `plain` is conv_route's
int launch_conv_x6(const mi_conv_desc &d, int tile, int image_tile, bool plain, hipStream_t st) {
    MI_REQUIRE(d.wx && ((uintptr_t)d.wx & 15) == 0, "conv x6: split weight image missing or misaligned");
    return dispatch_epilogue(d, [&](auto epi, auto lflags) {
        constexpr int E = decltype(epi)::value, F = decltype(lflags)::value;
        return plain ? launch_tile_x6<E, F, true, 0>(d, tile, image_tile, st) : launch_tile_x6<E, F, false, 0>(d, tile, image_tile, st);
    });
}

}  // namespace mi
