// Which kernel a conv / linear layer runs: the eligibility of the loaders, the validation of a descriptor and conv_route, which
// turns descriptor and environment switches into one value.  Host code only: no kernel, no HIP call, no pointer followed -- so the
// whole decision table runs in a process without a GPU (tools/conv_route_table.hip, tests/test_conv_route_host.py).
#include "common.h"
#include "kernels.h"

namespace mi {

// process-wide switch of the split-bf16 main loops (mi_set_split_bf16): 0 ignores every split weight image
int g_split_bf16 = 1;

int conv_pick_tile(int M) {
    if (M <= 32) return 32;
    if (M <= 64) return 64;
    if (M % 128 == 0) return 128;
    if (M % 96 == 0) return 96;
    if (M <= 96) return 96;
    return 128;
}

// Small batches: a layer whose 128-row tiles give fewer workgroups than the chip has CUs (B = 1: M = 512 and 2 688 tokens -> 84;
// a k x k GLU conv: 6 x 21) runs on a smaller tile instead -- more workgroups at a lower per-workgroup rate.  Which tile that is
// depends on the route (conv_route).  MI_SMALL_TILE=0: off
static bool under_filled(const mi_conv_desc &d, int tile = 128) {
    return (int64_t)(d.Mpad / tile) * ceil_div((int64_t)d.B * d.O1 * d.O2, BN) < 200;
}

// float32, stride-1 k x k conv with K2 = 3 whose geometry the descriptor states (ntaps, tap_k2, tap_pad*): the DMA loop of
// conv_gemm_dmatap_kernel (gemm_conv.hip), or, for a layer with a usable split weight image (`has_image`) when asked for it
// (`split`), the same shifted-run loader in front of the split-bf16 main loop (gemm_x6.hip conv_tap_x6_kernel; GLU only)
static bool dmatap_eligible(const mi_conv_desc &d, int tile, bool has_image, bool split = false) {
    const bool off = switches().no_dma_tap;
    const int ld = d.x_ld ? d.x_ld : d.D2;
    if (switches().no_dma_dconv && d.epi == MI_EPI_BIAS_STATS) return false;      // A/B switch for the BIAS_STATS kind alone
    const int dil = d.tap_dil2 ? d.tap_dil2 : 1;
    // GLU: the decoders' 3 x 3 / k = 3 rewrite convs (96- / 128-row tiles); BIAS_STATS: the DConv blocks' dilated k = 3 convs (32- / 64-row)
    const bool kind = (d.epi == MI_EPI_GLU && (tile == 96 || tile == 128) && (d.ntaps == 9 || d.ntaps == 3) && dil == 1) ||
                      (d.epi == MI_EPI_BIAS_STATS && (tile == 32 || tile == 64) && d.ntaps == 3 && (dil == 1 || dil == 2) && d.flags == 0);
    return !off && !d.half && (split ? has_image && d.epi == MI_EPI_GLU : !has_image) && kind && d.tap_k2 == 3 && d.Mpad % tile == 0 &&
           d.K % d.ntaps == 0 && d.S1 == 1 && d.S2 == 1 && d.O1 == d.D1 && d.O2 == ld && ld % 4 == 0 && d.tap_pad2 == dil &&
           d.tap_pad1 == (d.ntaps / 3 - 1) / 2 && !(d.flags & (MI_FLAG_IMG | MI_FLAG_IMG4)) && d.x_bstride == (int64_t)(d.K / d.ntaps) * d.D1 * ld;
}
// float32 layer with row taps only (the caller vouches for the table: `dma_rows`; a plain layer's table is the identity): the DMA
// loop of conv_gemm_dmarow_kernel (gemm_conv.hip).
// `split`: such a layer with a split weight image -- a strided encoder conv (LINEAR + GELU) or transposed conv on a 96- / 128-row
// tile, a 1 x 1 + GLU layer on a 128-row tile -- takes the same row loader in front of the split-bf16 main loop (gemm_x6.hip
// conv_rows_x6_kernel); MI_NO_DMA_ROWS=1 turns both off
static bool dmarow_eligible(const mi_conv_desc &d, int tile, bool plain, bool has_image, bool split = false) {
    const bool off = switches().no_dma_rows;
    const int ld = d.x_ld ? d.x_ld : d.D2;
    const int lf = d.flags & (MI_FLAG_GELU | MI_FLAG_SCALE | MI_FLAG_RES | MI_FLAG_LN | MI_FLAG_STATS | MI_FLAG_IMG | MI_FLAG_IMG4 | MI_FLAG_HEADS);
    // 1x1 + GLU / GroupNorm-GLU: 128-row tiles only -- the 96-row ones are the level-0 / 1 rewrites (K = 48 / 96: three or six K steps,
    // bound by their output), where the register-staged kernel's four workgroups per CU measured 3 % faster (476 vs 490 us)
    const bool epi_ok = (d.epi == MI_EPI_LINEAR && lf == MI_FLAG_GELU && !plain) || d.epi == MI_EPI_CONVTR ||
                        ((d.epi == MI_EPI_GLU || d.epi == MI_EPI_GN_GLU) && plain && tile == 128 && !(d.flags & (MI_FLAG_IMG | MI_FLAG_IMG4)));
    if (split && (d.epi == MI_EPI_GN_GLU || tile == 64)) return false;
    return !off && !d.half && (split ? has_image : !has_image) && d.ktab && epi_ok && (plain || d.dma_rows) && (tile == 64 || tile == 96 || tile == 128) &&
           d.Mpad % tile == 0 && d.S2 == 1 && d.O2 == ld && ld % 4 == 0 && ((uintptr_t)d.x & 3) == 0 && ((uintptr_t)d.ktab & 63) == 0 &&
           (d.epi == MI_EPI_CONVTR || tile != 64 || d.epi == MI_EPI_LINEAR);
}

// float32 1-D layer along the TIME axis with a split weight image (the caller vouches for the table and the layout: `dma_time`;
// one row per channel, D1 = O1 = 1).  Its runs go global -> LDS by DMA in front of the split-bf16 main loop (gemm_x6.hip):
//   * a transposed conv as a two-tap GEMM (conv_time_tr_x6_kernel): K ordered (ci, j) with tap j at column q - j, columns q = 0 .. D2
//     on a pitch O2 % 4 == 0 with o2_valid = D2 + 1, so that a lane's 16-byte chunk never straddles two items;
//   * a strided conv k = 8, s = 4, pad 2, + GELU (conv_time_enc_x6_kernel): K ordered (ci, t), column o reads samples 4 o - 2 + t.
// MI_X6=0 / mi_set_split_bf16(0) leave the layer on the table-driven gather
static bool dmatime_eligible(const mi_conv_desc &d, int tile, bool plain, bool has_image) {
    const int ld = d.x_ld ? d.x_ld : d.D2, o2v = d.o2_valid ? d.o2_valid : d.O2;
    const int lf = d.flags & (MI_FLAG_GELU | MI_FLAG_SCALE | MI_FLAG_RES | MI_FLAG_LN | MI_FLAG_STATS | MI_FLAG_IMG | MI_FLAG_IMG4 | MI_FLAG_HEADS);
    const bool tr = d.epi == MI_EPI_CONVTR && !(d.flags & (MI_FLAG_TR_FREQ | MI_FLAG_IMG)) && d.K % 2 == 0 && d.S2 == 1 && d.O2 % 4 == 0 &&
                    d.o2_valid == d.D2 + 1 && d.o2_valid <= d.O2 && d.x_bstride == (int64_t)(d.K / 2) * ld;
    const bool enc = d.epi == MI_EPI_LINEAR && lf == MI_FLAG_GELU && d.K % 8 == 0 && d.S2 == 4 && 4 * (int64_t)o2v <= (int64_t)d.D2 + 3 &&
                     d.x_bstride == (int64_t)(d.K / 8) * ld;
    return d.dma_time && !d.half && has_image && !plain && (tr || enc) && (tile == 96 || tile == 128) && d.Mpad % tile == 0 && d.D1 == 1 &&
           d.O1 == 1 && d.S1 == 1 && ld >= d.D2 && ((uintptr_t)d.x & 3) == 0;
}

int conv_check_tile_m(const mi_conv_desc &d) {
    MI_REQUIRE(d.tile_m != 192 || (d.M > 0 && d.M % 192 == 0 && d.Mpad == d.M), "conv: tile_m 192 needs M %% 192 == 0 and no M padding (M %d, Mpad %d)", d.M, d.Mpad);
    return MI_OK;
}

// plain fast path: a 1x1 / linear layer whose gather is the identity
// (an operand-image input is never read through x: the float4 loader's conditions on K, P and x do not apply to it)
static bool conv_plain(const mi_conv_desc &d) {
    const int64_t P = (int64_t)d.O1 * d.O2;
    return d.plain && (d.xh || (d.K == d.Kpad && P % 4 == 0 && d.x_bstride % 4 == 0 && ((uintptr_t)d.x & 15) == 0)) &&
           d.S1 == 1 && d.S2 == 1 && d.D1 == d.O1 && (d.x_ld ? d.x_ld : d.D2) == d.O2;
}

// the LINEAR flag sets conv_gemm_half_img256_kernel (gemm_half.hip) alone is compiled for
static bool half_img256_only(int f) { return f == (MI_FLAG_LN | MI_FLAG_HEADS) || f == (MI_FLAG_LN | MI_FLAG_GELU | MI_FLAG_IMG); }
static int half_linear_flags(const mi_conv_desc &d) {
    return d.flags & (MI_FLAG_GELU | MI_FLAG_SCALE | MI_FLAG_RES | MI_FLAG_LN | MI_FLAG_IMG | MI_FLAG_HEADS | MI_FLAG_STATS);
}

// What no kernel takes.  The launchers add the checks of their own operands (weight images, table lengths, tile multiples)
int conv_validate(const mi_conv_desc &d) {
    MI_TRY(conv_check_tile_m(d));
    MI_REQUIRE((int64_t)d.Mpad * d.y_cstride < (1ll << 31), "conv: output channel stride too large for 32-bit row offsets");
    MI_REQUIRE(d.Kpad % BK == 0 && d.Kpad >= BK, "conv: Kpad %d must be a positive multiple of %d", d.Kpad, BK);
    MI_REQUIRE(d.Mpad % 4 == 0, "conv: Mpad %d must be a multiple of 4", d.Mpad);
    MI_REQUIRE(d.O2 >= 32 || d.row_mode == 0 || (d.epi != MI_EPI_BIAS_STATS && d.epi != MI_EPI_STATS_ONLY),
               "conv: statistics epilogue with rows (b, o1) (row_mode 1) needs O2 >= 32");      // row_mode 0: any width (conv_stats_per_item)
    MI_REQUIRE(d.pro == 0, "conv: the fused GroupNorm+GELU prologue was replaced by launch_gn_gelu");
    MI_REQUIRE(!(d.flags & MI_FLAG_IMG4) || (d.epi == MI_EPI_GLU && d.half && d.yh && d.yh_pq > 0 && d.yh_n >= (int64_t)d.B * d.yh_pq && d.M % 32 == 0 &&
                                             ((uintptr_t)d.yh & 15) == 0),
               "conv: MI_FLAG_IMG4 needs a half-mode GLU layer with M %% 32 == 0 and an aligned phase image of >= B * yh_pq positions per plane");
    MI_REQUIRE(!(d.flags & MI_FLAG_STATS) || (d.epi == MI_EPI_LINEAR && d.stats && d.O2 >= 32 && d.row_mode == 0),
               "conv: MI_FLAG_STATS needs a LINEAR layer, a statistics buffer and O2 >= 32");
    MI_REQUIRE(!(d.flags & MI_FLAG_LN) || (d.pro_stats && d.scale && d.epi == MI_EPI_LINEAR), "conv: MI_FLAG_LN needs pro_stats and scale");
    const int64_t P = (int64_t)d.O1 * d.O2;
    MI_REQUIRE(!(d.flags & MI_FLAG_IMG) || d.epi == MI_EPI_CONVTR ||
               (d.half && d.yh && d.epi == MI_EPI_LINEAR && d.M % 8 == 0 && d.yh_n >= (int64_t)d.B * P && ((uintptr_t)d.yh & 15) == 0) ||
               (d.half && d.yh && d.epi == MI_EPI_GLU && d.M % 32 == 0 && !(d.flags & (MI_FLAG_IMG4 | MI_FLAG_EMB)) && d.yh_n >= (int64_t)d.B * P &&
                ((uintptr_t)d.yh & 15) == 0),
               "conv: MI_FLAG_IMG needs a half-precision LINEAR layer with M %% 8 == 0 (or GLU layer with M %% 32 == 0) and an aligned "
               "output image of >= B * P columns");
    MI_REQUIRE(d.epi != MI_EPI_CONVTR || ((int64_t)d.Mpad * d.y_cstride < (1ll << 30) && (d.tr_stride == 0 || d.tr_stride == 2 || d.tr_stride == 4) &&
                                          d.M % (d.tr_stride == 2 ? 2 : 4) == 0),
               "conv: transposed conv needs stride 2 or 4, M a multiple of it and 30-bit output offsets per item");
    {   // the scatter epilogue is compiled for these flag sets (gemm_tile.h convtr_tile)
        const int f = d.flags & (MI_FLAG_GELU | MI_FLAG_RES | MI_FLAG_IMG);
        MI_REQUIRE(d.epi != MI_EPI_CONVTR || f == 0 || (d.tr_stride != 2 && (f == (MI_FLAG_GELU | MI_FLAG_RES) || f == (MI_FLAG_GELU | MI_FLAG_RES | MI_FLAG_IMG))),
                   "conv: transposed conv epilogue supports no flags, GELU|RES or GELU|RES|IMG (stride 2: no flags), got %d", d.flags);
    }
    MI_REQUIRE(!(d.flags & MI_FLAG_IMG) || d.epi != MI_EPI_CONVTR ||
               (d.half && d.yh && d.yh_n >= (int64_t)d.B * d.y_cstride && ((uintptr_t)d.yh & 15) == 0),
               "conv: MI_FLAG_IMG on a transposed conv needs a half mode and an output image of >= B * y_cstride positions");
    MI_REQUIRE(!d.wtap || (d.half && d.xh), "conv: tap-ordered weights need a half mode and an operand-image input");
    // (a layer with tap-ordered weights answers to the check above alone)
    MI_REQUIRE(d.wtap || !(d.flags & MI_FLAG_HEADS) || (d.half && d.yh && d.epi == MI_EPI_LINEAR && d.M % 512 == 0 && d.O1 == 1 && d.yh_n >= d.O2 &&
                                                        ((uintptr_t)d.yh & 15) == 0 && !(d.flags & MI_FLAG_IMG)),
               "conv: MI_FLAG_HEADS needs a half-precision LINEAR layer on tokens (O1 = 1) with M %% 512 == 0 and an aligned output");
    MI_REQUIRE(!d.xh || d.half, "conv: an operand-image input needs a half-precision layer");
    if (d.xh && !d.wtap) {      // routes 9 and 10: lin2 / out_proj, and (256-row tile) the in-projections and lin1
        const int f = half_linear_flags(d);
        MI_REQUIRE(d.epi == MI_EPI_LINEAR && conv_plain(d), "conv: an operand-image input needs a plain LINEAR layer");
        MI_REQUIRE(f == (MI_FLAG_SCALE | MI_FLAG_RES) || f == (MI_FLAG_SCALE | MI_FLAG_RES | MI_FLAG_STATS) || half_img256_only(f),
                   "conv: an operand-image input is not instantiated for LINEAR flags %d", d.flags);
    }
    return MI_OK;
}

// The statistics epilogues (gemm_tile.h conv_epilogue) reduce a wave's 32 consecutive columns into the row of its first column and
// ONE other row.  Rows (b, o1) are 32 columns and more (checked above); a per-item row (row_mode 0) of P = O1 * O2 < 32 columns lets
// three or more items share a wave -- time-branch DConv of the hdemucs engine on a batch of short chunks -- and the middle ones would
// be credited to the last.  launch_conv then runs the layer once per item: one row per launch.  Two items never need it; P = 16, 24,
// 28 never put three rows into an aligned 32-column window either, but the tensors are tiny and one rule is easier to hold
bool conv_stats_per_item(const mi_conv_desc &d) {
    return (d.epi == MI_EPI_BIAS_STATS || d.epi == MI_EPI_STATS_ONLY) && d.row_mode == 0 && d.B > 2 && (int64_t)d.O1 * d.O2 < 32;
}

// The decision, top to bottom; the first test that holds wins (kernels.h ConvRoute).  It never fails: what conv_validate refuses
// gets an answer too, which launch_conv never acts on
ConvRoute conv_route(const mi_conv_desc &d) {
    const bool image = d.wx && g_split_bf16;                // mi_set_split_bf16(0): native fp32 MFMA kernels only
    const Switches &sw = switches();
    // tile_m = 192 (a layer with M % 192 == 0 whose split image is a run of 96-row images): the float32 weights, and so every
    // native and half-mode kernel, keep the tile conv_pick_tile gives
    const int tile = d.tile_m && d.tile_m != 192 ? d.tile_m : conv_pick_tile(d.M);
    const bool plain = conv_plain(d);
    if (d.wtap) return {MI_ROUTE_TAP_HALF, tile, plain};
    if (d.half && d.xh) {
        // Input given as a 16-bit operand image.  The in-projections and lin1 (LN|HEADS, LN|GELU|IMG): the 512-thread 256 x 256
        // tile.  The residual epilogues (out_proj, lin2: 340 MB of float32 residual read + output write per launch) keep the
        // 3-stage kernel, 256 x 128 where Mpad allows, at two workgroups per CU, whose epilogues overlap each other's main loops:
        // measured 9.63 ms against 9.79 for the linear class with the 256 x 256 tile here (MI_IMG256=1: A/B switch, SCALE|RES only)
        const int f = half_linear_flags(d);
        const bool wide = d.Mpad % 256 == 0;
        if (half_img256_only(f) || (f == (MI_FLAG_SCALE | MI_FLAG_RES) && sw.img256 && wide)) return {MI_ROUTE_HALF_IMG256, 256, plain};
        return {MI_ROUTE_HALF_IMG, wide ? 256 : 128, plain};
    }
    // the register-staged half kernel; 256 x 128 for the transformer's linear layers: the 128 x 128 tile is bound by cache bandwidth
    // (43 FLOP per byte of float32 activations + 16-bit weights); twice the rows per activation tile brings that to 64
    if (d.half) return {MI_ROUTE_HALF, sw.half_tile256 && plain && tile == 128 && d.epi == MI_EPI_LINEAR && d.Mpad % 256 == 0 ? 256 : tile, plain};
    const bool t192 = d.tile_m == 192 && image;
    const bool small = sw.small_tile && tile == 128 && !t192 && under_filled(d), small_linear = small && plain && d.epi == MI_EPI_LINEAR;
    // The 192-row layers: the 192-row tile where the loader family has it for the layer's epilogue and its workgroups fill the
    // chip, else the 96-row tile on the same image (bit-identical to it); never the 64-row tile, which needs a 128-row image
    const int lf = d.flags & (MI_FLAG_GELU | MI_FLAG_SCALE | MI_FLAG_RES | MI_FLAG_LN | MI_FLAG_STATS);
    auto split_tile = [&](int ntaps) {
        if (!t192) return small ? 64 : tile;
        const bool filled = !(sw.small_tile && under_filled(d, 192));
        return filled && conv_x6_tile192(d.epi, d.epi == MI_EPI_LINEAR ? lf : 0, plain, ntaps) ? 192 : 96;
    };
    // Split weight image.  An under-filled layer takes the 64-row tile that reads the 128-row image: bit-identical to the 128-row
    // tile, no second image.  The decoders' 3 x 3 / k = 3 rewrite convs: shifted-run DMA taps in front of the split-bf16 main loop
    if (!plain && !sw.x6_plain_only && dmatap_eligible(d, tile, image, true)) return {MI_ROUTE_TAP_X6, split_tile(d.ntaps), plain};
    // the frequency branch's encoder / transposed convs and the 1 x 1 + GLU rewrites: the DMA row loader in front of it
    if (!sw.x6_plain_only && dmarow_eligible(d, tile, plain, image, true)) return {MI_ROUTE_ROWS_X6, split_tile(kRowTaps), plain};
    // the time branch's transposed and strided convs: runs along the time axis by DMA in front of it
    if (!sw.x6_plain_only && dmatime_eligible(d, tile, plain, image))
        return {MI_ROUTE_TIME_X6, split_tile(d.epi == MI_EPI_CONVTR ? kTimeTr : kTimeEnc), plain};
    // native DMA taps: an under-filled k x k GLU conv takes 96-row tiles
    const int ktile = small && !plain && d.epi == MI_EPI_GLU && d.Mpad % 96 == 0 ? 96 : tile;
    if (!plain && dmatap_eligible(d, ktile, image)) return {MI_ROUTE_DMATAP, ktile, plain};
    if (dmarow_eligible(d, tile, plain, image)) return {MI_ROUTE_DMAROW, tile, plain};
    // the split-bf16 main loop behind the plain loader or the gather table (MI_X6_MODE=1: plain layers only)
    if (image && conv_x6_supported(tile) && (!sw.x6_plain_only || plain)) return {MI_ROUTE_X6, t192 ? split_tile(0) : small_linear ? 64 : tile, plain};
    // native fp32 kernels: an under-filled plain linear layer takes 64-row tiles.  M groups (gemm_tile.h) halve these kernels' L2
    // misses on the 4 MiB weight matrices (TCC hit rate 48 % -> 74 %) but the misses were Infinity-Cache hits: no time is gained
    // and every activation tile is then fetched from HBM by several XCDs (+10 % HBM bytes), so they keep one group unless MI_MGROUPS=1
    const int ntile = small_linear && d.Mpad % 64 == 0 ? 64 : tile;
    const bool dma = plain && ntile == 128 && d.epi == MI_EPI_LINEAR && !sw.no_dma;
    return {dma ? MI_ROUTE_DMA : MI_ROUTE_TABLE, ntile, plain, sw.mgroups};
}

}  // namespace mi
