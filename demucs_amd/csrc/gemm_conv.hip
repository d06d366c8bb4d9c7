// Implicit-GEMM convolution on gfx950 fp32 MFMA (see gemm_conv.h).
//
// Workgroup = 256 threads = 4 waves; block tile BM x 128 (BM = 32, 64, 96 or 128), K step 16,
// LDS double buffer, global->register prefetch of tile k+1 while tile k feeds the matrix cores.
// Both operands sit in LDS k-major ([16][BM], [16][128]) so that a 32x32x2 MFMA fragment
// (lane l: row/col l&31, k = l>>5) is one conflict-free ds_read_b32 per operand.
// Arithmetic is exact fp32 (v_mfma_f32_32x32x2_f32 == k-ordered fmaf chain): the <=1e-4 parity
// target against the fp32 CPU reference leaves no room for bf16 operands.
#include "gemm_loop.h"

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
    Wg w;
    if (!wg_tile<WN, BM>(d, MT, Gm, N, w)) return;
    const int tid = w.tid;

    // ---- A loader: BK x BM floats as float4, thread-linear ---------------------------------------
    constexpr int A_F4 = BK * BM / 4, A_FULL = A_F4 / 256, A_REM = A_F4 % 256;
    constexpr int A_SLOTS = A_FULL + (A_REM ? 1 : 0);
    static_assert(A_SLOTS <= 2, "A tile fits two float4 per thread");
    const int aidx0 = tid < A_F4 ? tid : 0, aidx1 = (tid + 256 < A_F4) ? tid + 256 : 0;
    const int ar0 = aidx0 / (BM / 4), ac0 = (aidx0 % (BM / 4)) * 4;
    const int ar1 = aidx1 / (BM / 4), ac1 = (aidx1 % (BM / 4)) * 4;
    const bool a_on0 = tid < A_F4, a_on1 = tid + 256 < A_F4;
    const float *ap0 = d.wt + (size_t)ar0 * d.Mpad + w.m0 + ac0;
    const float *ap1 = d.wt + (size_t)ar1 * d.Mpad + w.m0 + ac1;
    const size_t a_step = (size_t)BK * d.Mpad;

    // ---- B loader ----------------------------------------------------------------------------------
    // generic: this thread owns column (tid & 127), rows khalf + 2*j;  plain: 4 columns x rows r, r + 8
    const int khalf = w.wave >> 1;
    const ColInfo lc = decompose(w.n0 + (PLAIN ? (tid & 31) * 4 : (tid & 127)), N, w.P, d.O2, PLAIN ? d.O2 : w.o2v);
    const int i1b = lc.o1 * d.S1, i2b = lc.o2 * d.S2;
    const float *xcol = d.x + (size_t)lc.b * d.x_bstride + (PLAIN ? (size_t)lc.p : (size_t)i1b * (d.x_ld ? d.x_ld : d.D2) + i2b);
    const int prow = tid >> 5;                                   // plain: first row of this thread
    const float *bp0 = lc.valid ? xcol + (size_t)prow * w.P : d.x; // plain row pointers (channel stride = P)
    const float *bp1 = lc.valid ? xcol + (size_t)(prow + 8) * w.P : d.x;
    const size_t b_step = lc.valid ? (size_t)BK * w.P : 0;

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
    zero_acc(acc);

    const int nk = d.Kpad / BK;
    MI_LOAD_TILE(0);
    MI_STORE_TILE(0);
    __syncthreads();
    int cur = 0;
    for (int kt = 0; kt < nk; ++kt) {
        if (kt + 1 < nk) MI_LOAD_TILE(kt + 1);
        fp32_kstep<TM, TN, BM>(&As[cur][0][0], &Bs[cur][0][0], w, acc);
        if (kt + 1 < nk) MI_STORE_TILE(cur ^ 1);
        __syncthreads();
        cur ^= 1;
    }
#undef MI_LOAD_TILE
#undef MI_STORE_TILE

    conv_epilogue<TM, TN, EPI, LFLAGS>(d, acc, w.m0, w.n0, w.wm, w.wn, N, w.P, w.o2v);
}

// ---------------------------------------------------------------------------------------------
// The LDS-DMA main loop of the native float32 kernels: both operand tiles go global -> LDS with global_load_lds_dwordx4 (no
// staging registers, no ds_write) through the three-stage ring of gemm_loop.h; each wave instruction lands 1 KiB.  A stage holds
// the A image [16][BM], then the B image [16][128].  The A transfers follow AImagePlan, the B rows come from the loader NT
// selects (gemm_loop.h: PlainRows, TapRows, RowTaps): each wave waits for its own 2 B + 2, 1 or 0 A transfers per tile.
// Tiles: 128 x 128 (2 x 2 waves) and 96 / 64 / 32 x 128 (1 x 4 waves).
template <int BM, int EPI, int LFLAGS, int NT, int DIL, bool ROWPAIRS>
__device__ __forceinline__ void conv_dma_body(const mi_conv_desc &d, const int N, const int MT, const int Gm) {
    constexpr int WM = BM == 128 ? 2 : 1, WN = 4 / WM, TM = BM / (32 * WM), TN = BN / (32 * WN);
    constexpr int SS = BK * (BM + BN);                       // floats per stage: A image then B image
    __shared__ __attribute__((aligned(16))) float smem[3 * SS];
    Wg w;
    if (!wg_tile<WN, BM>(d, MT, Gm, N, w)) return;
    const AImagePlan<BM, ROWPAIRS> A(d, w);
    BLoader<NT, DIL> B(d, w, N, (int64_t)d.D1 * (d.x_ld ? d.x_ld : d.D2));
    const auto brows = [&](int stage) { return smem + stage * SS + BK * BM + (4 * w.wave) * BN; };
    f32x16 acc[TM][TN];
    zero_acc(acc);
    dma_ring3(
        d.Kpad / BK, kBInFlight + A.in_flight(), [&](int kt) { B.prefetch(kt); },
        [&](int kt, int stage) {
            A.issue(kt, smem + stage * SS);
            B.issue(d, kt, brows(stage));
        },
        [&](int kt, int stage) {
            if constexpr (NT > 0) {
                B.fix(d, kt, brows(stage));
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");      // the fix-up's ds_writes, ahead of the raw barrier
            }
        },
        [&](int stage) { fp32_kstep<TM, TN, BM>(smem + stage * SS, smem + stage * SS + BK * BM, w, acc); });
    conv_epilogue<TM, TN, EPI, LFLAGS>(d, acc, w.m0, w.n0, w.wm, w.wn, N, w.P, w.o2v);
}

// the plain (1x1 / linear) 128 x 128 tile
template <int EPI, int LFLAGS>
__global__ __launch_bounds__(256, 3) void conv_gemm_dma_kernel(const mi_conv_desc d, const int N, const int MT, const int Gm) {
    conv_dma_body<128, EPI, LFLAGS, 0, 1, true>(d, N, MT, Gm);
}

// STRIDE-1 k x k convolutions (the decoders' 3 x 3 / k = 3 "rewrite" convs, reference demucs/hdemucs.py:304-314, on 128- and 96-row
// tiles; DIL: the DConv blocks' dilated k = 3 convs C -> C / 8, demucs.py:138: dilation 1 / 2, padding = dilation, with the
// row-statistics epilogue on 32- and 64-row tiles, M = 24 / 48).  The table-driven gather of conv_gemm_kernel (8 dword gathers +
// bounds tests + ds_writes per thread and K step) ran them at 0.64-0.70 of the fp32 MFMA peak against 0.74 for the plain DMA loop.
template <int BMT, int EPI, int NT, int DIL = 1>
__global__ __launch_bounds__(256, 3) void conv_gemm_dmatap_kernel(const mi_conv_desc d, const int N, const int MT, const int Gm) {
    conv_dma_body<BMT, EPI, 0, NT, DIL, true>(d, N, MT, Gm);
}

template <int EPI>
static int launch_dmatap(const mi_conv_desc &d, int tile, hipStream_t st) {
    ConvGeom g;
    MI_TRY(conv_geom(d, "conv: DMA tap route", tile, tile, g));
    if constexpr (EPI == MI_EPI_BIAS_STATS) {
        const bool d2 = d.tap_dil2 == 2;
        if (tile == 64 && d2) MI_LAUNCH_TILES((conv_gemm_dmatap_kernel<64, EPI, 3, 2>), d, g, 1, st);
        else if (tile == 64) MI_LAUNCH_TILES((conv_gemm_dmatap_kernel<64, EPI, 3, 1>), d, g, 1, st);
        else if (d2) MI_LAUNCH_TILES((conv_gemm_dmatap_kernel<32, EPI, 3, 2>), d, g, 1, st);
        else MI_LAUNCH_TILES((conv_gemm_dmatap_kernel<32, EPI, 3, 1>), d, g, 1, st);
    } else if (tile == 128 && d.ntaps == 9) MI_LAUNCH_TILES((conv_gemm_dmatap_kernel<128, EPI, 9>), d, g, 1, st);
    else if (tile == 128) MI_LAUNCH_TILES((conv_gemm_dmatap_kernel<128, EPI, 3>), d, g, 1, st);
    else if (d.ntaps == 9) MI_LAUNCH_TILES((conv_gemm_dmatap_kernel<96, EPI, 9>), d, g, 1, st);
    else MI_LAUNCH_TILES((conv_gemm_dmatap_kernel<96, EPI, 3>), d, g, 1, st);
    return MI_OK;
}

// Layers whose taps move along ROWS only: the frequency branch's strided encoder convs (k = 8, s = 4 along the frequency axis: row
// 4 o1 + j - 2), its transposed convs as two-tap GEMMs (rows q, q - 1) and every 1x1 layer that does not run conv_gemm_dma_kernel
// (GLU / GroupNorm-GLU epilogues, 96- and 64-row tiles).  The row offsets come from the gather table, which keeps ONE kernel per
// (tile, epilogue) for all of these layers.  Summation order = conv_gemm_kernel's: results are bit-identical to the table-driven
// route (tests/test_gpu_kernels.py), which ran these classes at 0.5-0.6 of the fp32 MFMA peak.
template <int BMT, int EPI, int LFLAGS>
__global__ __launch_bounds__(256, 3) void conv_gemm_dmarow_kernel(const mi_conv_desc d, const int N, const int MT, const int Gm) {
    conv_dma_body<BMT, EPI, LFLAGS, kRowTaps, 1, false>(d, N, MT, Gm);
}

template <int EPI, int LFLAGS>
static int launch_dmarow(const mi_conv_desc &d, int tile, hipStream_t st) {
    ConvGeom g;
    MI_TRY(conv_geom(d, "conv: DMA row route", tile, tile, g));
    if (tile == 128) MI_LAUNCH_TILES((conv_gemm_dmarow_kernel<128, EPI, LFLAGS>), d, g, 1, st);
    else if constexpr (EPI == MI_EPI_LINEAR || EPI == MI_EPI_CONVTR) {
        if (tile == 96) MI_LAUNCH_TILES((conv_gemm_dmarow_kernel<96, EPI, LFLAGS>), d, g, 1, st);
        else MI_LAUNCH_TILES((conv_gemm_dmarow_kernel<64, EPI, LFLAGS>), d, g, 1, st);
    } else return set_error(MI_EINVAL, "conv: DMA row route has no %d-row tile for epilogue %d", tile, EPI);
    return MI_OK;
}

// ---------------------------------------------------------------------------------------------
// The native kernels, `r` as conv_route decided.  Route MI_ROUTE_DMA: the LDS-DMA linear tile instead of the register-staged
// loader -- a plain LINEAR layer on the 128-row tile
template <int WM, int WN, int TM, int TN, int EPI, int LFLAGS, bool PLAIN>
static int launch_cfg(const mi_conv_desc &d, const ConvRoute &r, hipStream_t st) {
    constexpr int BM = WM * TM * 32;
    const bool dma = r.route == MI_ROUTE_DMA;
    ConvGeom g;
    MI_TRY(conv_geom(d, "conv", BM, BM, g));
    const int Gm = r.mgroups ? pick_m_groups(g.MT, (size_t)d.Kpad * d.Mpad * 4) : 1;
    if constexpr (PLAIN && BM == 128 && EPI == MI_EPI_LINEAR) {
        if (dma) {
            MI_LAUNCH_TILES((conv_gemm_dma_kernel<EPI, LFLAGS>), d, g, Gm, st);
            return MI_OK;
        }
    }
    MI_REQUIRE(!dma, "conv: the LDS-DMA linear tile takes a plain LINEAR layer on the 128-row tile");
    MI_LAUNCH_TILES((conv_gemm_kernel<WM, WN, TM, TN, EPI, LFLAGS, PLAIN>), d, g, Gm, st);
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

// decide (conv_route.hip) and launch a validated descriptor whose sink is set
static int launch_routed(const mi_conv_desc &d, hipStream_t st) {
    const ConvRoute r = conv_route(d);
    // the tile the layer's split image was packed for: a 192-row layer's is a run of 96-row images
    const int image_tile = d.tile_m == 192 ? 96 : d.tile_m ? d.tile_m : conv_pick_tile(d.M);
    g_last_conv_route = r.route;
    g_last_conv_tile = r.tile;
    if ((unsigned)r.route < 16u && (unsigned)d.epi < 8u) ++g_conv_route_launches[r.route][d.epi];
    switch (r.route) {
        case MI_ROUTE_TAP_HALF: return launch_conv_tap(d, r.tile, st);
        case MI_ROUTE_HALF:
        case MI_ROUTE_HALF_IMG:
        case MI_ROUTE_HALF_IMG256: return launch_conv_half(d, r, st);
        case MI_ROUTE_TAP_X6: return launch_conv_tap_x6(d, r.tile, image_tile, st);
        case MI_ROUTE_ROWS_X6: return launch_conv_rows_x6(d, r.tile, image_tile, st);
        case MI_ROUTE_TIME_X6: return launch_conv_time_x6(d, r.tile, image_tile, st);
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

// fill the sink, validate, launch -- a statistics layer whose rows the epilogue cannot tell apart (conv_route.hip
// conv_stats_per_item) item by item: tiny tensors, B launches, each with one statistics row
int launch_conv(const mi_conv_desc &din, hipStream_t st) {
    mi_conv_desc d = din;
    if (!d.sink) d.sink = conv_sink();
    MI_REQUIRE(d.sink && ((uintptr_t)d.sink & 15) == 0, "conv: the store sink could not be allocated or is not 16-byte aligned");
    MI_TRY(conv_validate(d));
    if (!conv_stats_per_item(d)) return launch_routed(d, st);
    mi_conv_desc e = d;
    e.B = 1;
    for (int b = 0; b < d.B; ++b) {
        e.x = d.x + (size_t)b * d.x_bstride;
        e.y = d.y ? d.y + (size_t)b * d.y_bstride : nullptr;
        e.res = d.res ? d.res + (size_t)b * d.y_bstride : nullptr;
        e.stats = d.stats ? d.stats + (size_t)b * kStatSlots * 2 : nullptr;
        MI_TRY(launch_routed(e, st));
    }
    return MI_OK;
}

}  // namespace mi
