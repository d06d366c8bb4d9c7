// The conv route table on the CPU: links demucs_amd/csrc/conv_route.hip and switches.hip, nothing else of the library, and
// prints for each descriptor below one line `name route tile plain`, or `name invalid: <message>` where conv_validate refuses
// it.  No GPU, no HIP call, no pointer followed: small aligned numbers stand in for the descriptors' pointers.  The MI_*
// environment decides as in the library; the argument `nosplit` is mi_set_split_bf16(0).  tests/test_conv_route_host.py
// builds and runs it and holds the expectations.  The argument `time` prints, INSTEAD of those rows, the time branch's transposed
// and strided convs of route 11 (tests/test_conv_route_time_host.py); the argument `stats`, instead of them, the statistics epilogues
// on narrow rows (tests/test_gpu_conv_stats_rows.py).
//   hipcc --offload-arch=gfx950 -std=c++17 tools/conv_route_table.hip demucs_amd/csrc/conv_route.hip demucs_amd/csrc/switches.hip -o conv_route_table
#include "../demucs_amd/csrc/common.h"
#include "../demucs_amd/csrc/kernels.h"

namespace mi {
char *last_error_buf() {
    static char buf[1024] = "";
    return buf;
}
int set_error(int code, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(last_error_buf(), 1024, fmt, ap);
    va_end(ap);
    return code;
}
}  // namespace mi

using namespace mi;

static const float *const kX = (const float *)4096;
static const mi_ktab_entry *const kTab = (const mi_ktab_entry *)8192;
static void *const kPtr = (void *)16384;
static int rup(int v, int m) { return (v + m - 1) / m * m; }

static mi_conv_desc base(int M, int K, int tile, bool image) {
    mi_conv_desc d{};
    d.M = M, d.Mpad = rup(M, tile), d.K = K, d.Kpad = rup(K, 16), d.tile_m = tile;
    d.wt = kX, d.x = kX, d.ktab = kTab, d.y = (float *)kPtr, d.wx = image ? kPtr : nullptr;
    d.B = 1, d.S1 = d.S2 = 1;
    return d;
}
// tests/test_gpu_conv_route.py: plain LINEAR, M = 512, K = 64, B = 2 on O2 tokens
static mi_conv_desc linear(bool image, int O2, int M = 512, int B = 2, int tile = 128) {
    mi_conv_desc d = base(M, 64, tile, image);
    d.B = B, d.D1 = d.O1 = 1, d.D2 = d.O2 = O2, d.x_bstride = 64 * O2, d.plain = 1, d.epi = MI_EPI_LINEAR, d.y_cstride = O2;
    return d;
}
// 3 x 3 conv Cc -> 2 Cc + GLU on 8 rows of 48
static mi_conv_desc glu3x3(bool image, int Cc, int B, bool geometry = true) {
    mi_conv_desc d = base(2 * Cc, 9 * Cc, conv_pick_tile(2 * Cc), image);
    d.B = B, d.D1 = d.O1 = 8, d.D2 = d.O2 = 48, d.x_bstride = Cc * 384, d.row_mode = 1, d.epi = MI_EPI_GLU, d.y_cstride = 384;
    if (geometry) d.ntaps = 9, d.tap_k2 = 3, d.tap_pad1 = d.tap_pad2 = 1;
    return d;
}
// Conv2d k = (8, 1), s = (4, 1) + GELU on rows of `pitch` >= T floats
static mi_conv_desc encoder(bool image, int Cin, int Cout, int B, int Fr, int T, int pitch, int dma_rows) {
    mi_conv_desc d = base(Cout, 8 * Cin, conv_pick_tile(Cout), image);
    d.B = B, d.D1 = Fr, d.D2 = T, d.O1 = Fr / 4, d.O2 = pitch, d.S1 = 4, d.x_bstride = Cin * Fr * pitch, d.row_mode = 1;
    d.epi = MI_EPI_LINEAR, d.flags = MI_FLAG_GELU, d.y_cstride = Fr / 4 * pitch, d.o2_valid = T, d.x_ld = pitch, d.dma_rows = dma_rows;
    return d;
}
// tests/test_gpu_x6_tile192.py _desc: kind 0 linear on N tokens, 1 the 3 x 3 + GLU conv on 8 rows of N / 8, 2 the encoder conv on 16 rows
static mi_conv_desc t192(int M, int N, int tile_m, bool image, int kind = 0, int flags = MI_FLAG_LN, int Mpad = 0) {
    mi_conv_desc d = base(M, 64, conv_pick_tile(M), image);
    d.Mpad = Mpad ? Mpad : d.Mpad, d.tile_m = tile_m;
    if (kind == 0) d.D1 = d.O1 = 1, d.D2 = d.O2 = N, d.x_bstride = 64 * N, d.plain = 1, d.epi = MI_EPI_LINEAR, d.flags = flags, d.pro_stats = d.scale = kX;
    if (kind == 1) d.K = 72, d.Kpad = 80, d.D1 = d.O1 = 8, d.D2 = d.O2 = N / 8, d.x_bstride = 8 * N, d.epi = MI_EPI_GLU, d.ntaps = 9, d.tap_k2 = 3, d.tap_pad1 = d.tap_pad2 = 1;
    if (kind == 2) d.D1 = 16, d.D2 = d.O2 = N / 4, d.O1 = 4, d.S1 = 4, d.x_bstride = 8 * 16 * (N / 4), d.epi = MI_EPI_LINEAR, d.flags = MI_FLAG_GELU, d.dma_rows = 1;
    return d;
}
// tests/test_gpu_half_linear.py describe(): bf16 plain LINEAR, K = 64, B = 2, T = 40, packed for 128-row tiles
static mi_conv_desc half(int M, int flags, bool xh = true, int K = 64) {
    mi_conv_desc d = linear(false, 40, M);
    d.K = K, d.Kpad = rup(K, 16), d.half = MI_DTYPE_BF16, d.wh = kPtr, d.flags = flags, d.ktab_len = rup(d.Kpad, 32);
    if (xh) d.xh = kPtr, d.xh_n = 80, d.x = nullptr, d.ktab = nullptr;
    if (flags & MI_FLAG_LN) d.scale = d.pro_stats = kX;
    if (flags & MI_FLAG_STATS) d.stats = (double *)kPtr;
    if (flags & MI_FLAG_HEADS) d.yh = kPtr, d.yh_n = 40;
    if (flags & MI_FLAG_IMG) d.yh = kPtr, d.yh_n = 80;
    return d;
}

static void row(const char *name, const mi_conv_desc &d);
// the time branch's transposed conv C -> M / 4 on Lv samples per item (row pitch Lp) as the engine describes it: columns 0 .. Lv on
// a pitch that is a multiple of 4; `dma_time` 0: the same layer without the caller's promise
static mi_conv_desc time_tr(bool image, int C, int M, int B, int Lv, int Lp, int dma_time = 1) {
    mi_conv_desc d = base(M, 2 * C, conv_pick_tile(M), image);
    if (image && M % 192 == 0) d.tile_m = 192;
    d.B = B, d.D1 = d.O1 = 1, d.D2 = Lv, d.O2 = rup(Lv + 1, 4), d.o2_valid = Lv + 1, d.x_ld = Lp != Lv ? Lp : 0, d.x_bstride = (int64_t)C * Lp;
    d.epi = MI_EPI_CONVTR, d.out_len = 4 * Lv, d.y_cstride = 4 * Lp, d.dma_time = dma_time;
    return d;
}
// the time branch's strided conv Cin -> M, k = 8, s = 4, pad 2, + GELU on L samples per item (row pitch L rounded up to 4)
static mi_conv_desc time_enc(bool image, int Cin, int M, int B, int L, int dma_time = 1) {
    mi_conv_desc d = base(M, 8 * Cin, conv_pick_tile(M), image);
    if (image && M % 192 == 0) d.tile_m = 192;
    const int Lp = rup(L, 4), Lo = (L + 3) / 4;
    d.B = B, d.D1 = d.O1 = 1, d.D2 = L, d.O2 = rup(Lo, 4), d.o2_valid = Lo, d.S2 = 4, d.x_ld = Lp != L ? Lp : 0, d.x_bstride = (int64_t)Cin * Lp;
    d.epi = MI_EPI_LINEAR, d.flags = MI_FLAG_GELU, d.y_cstride = d.O2, d.dma_time = dma_time;
    return d;
}
static void time_rows() {
    char name[64];
    // tenc[1 .. 3].conv of a 7.8 s segment, under-filled (B = 1) and filled; a 128-row layer (M = 128) for the small-batch tile
    const int E[4][5] = {{48, 96, 85995, 1, 8}, {96, 192, 21499, 1, 5}, {192, 384, 5375, 1, 16}, {24, 128, 149, 3, 640}};
    for (int image = 1; image >= 0; --image)
        for (auto &l : E)
            for (int f = 0; f < 2; ++f) {
                snprintf(name, sizeof(name), "time_enc_M%d_%s%s", l[1], f ? "filled" : "under", image ? "+x6" : "");
                row(name, time_enc(image, l[0], l[1], l[3 + f], l[2]));
            }
    row("time_enc_M384_nopromise+x6", time_enc(true, 192, 384, 16, 5375, 0));
    // tdec[0 .. 2].convtr of a 7.8 s segment, under-filled (B = 1) and filled; a 128-row layer (M = 128) for the small-batch tile
    const int L[4][6] = {{384, 768, 1344, 1344, 1, 8}, {192, 384, 5375, 5376, 1, 4}, {96, 192, 21499, 21500, 1, 2}, {36, 128, 5375, 5376, 1, 8}};
    for (int image = 1; image >= 0; --image)
        for (auto &l : L)
            for (int f = 0; f < 2; ++f) {
                snprintf(name, sizeof(name), "time_tr_M%d_%s%s", l[1], f ? "filled" : "under", image ? "+x6" : "");
                row(name, time_tr(image, l[0], l[1], l[4 + f], l[2], l[3]));
            }
    row("time_tr_M768_nopromise+x6", time_tr(true, 384, 768, 8, 1344, 1344, 0));
    { mi_conv_desc d = time_tr(true, 384, 768, 8, 1344, 1344); d.O2 = 1345, d.o2_valid = 0; row("time_tr_M768_pitch1345+x6", d); }
    { mi_conv_desc d = time_tr(true, 384, 768, 8, 1344, 1344); d.flags = MI_FLAG_GELU | MI_FLAG_RES; d.res = kX; row("time_tr_M768_skip+x6", d); }
}

// the statistics epilogues on narrow rows: a DConv block's k = 3 conv 48 -> 12 (BIAS_STATS) and the statistics-only form, B items of
// O1 x O2 columns; after the three numbers a fourth, 1 where launch_conv runs the layer item by item (conv_stats_per_item)
static void stats_rows() {
    char name[64];
    for (int epi : {MI_EPI_BIAS_STATS, MI_EPI_STATS_ONLY})
        for (int row_mode = 0; row_mode < 2; ++row_mode)
            for (int B = 1; B <= 13; ++B)
                for (int O1 : {1, 3})
                    for (int O2 = 1; O2 <= 40; ++O2) {
                        mi_conv_desc c = base(12, 144, 32, false);
                        c.B = B, c.D1 = c.O1 = O1, c.D2 = c.O2 = O2, c.x_bstride = 48 * O1 * O2, c.epi = epi, c.row_mode = row_mode, c.y_cstride = O1 * O2;
                        c.stats = (double *)kPtr;
                        snprintf(name, sizeof(name), "stats_e%d_r%d_B%d_%dx%d", epi, row_mode, B, O1, O2);
                        if (conv_validate(c) != MI_OK) { printf("%s invalid: %s\n", name, last_error_buf()); continue; }
                        const ConvRoute r = conv_route(c);
                        printf("%s %d %d %d %d\n", name, r.route, r.tile, (int)r.plain, (int)conv_stats_per_item(c));
                    }
}

static void row(const char *name, const mi_conv_desc &d) {
    if (conv_validate(d) != MI_OK) { printf("%s invalid: %s\n", name, last_error_buf()); return; }
    const ConvRoute r = conv_route(d);
    printf("%s %d %d %d\n", name, r.route, r.tile, (int)r.plain);
}

int main(int argc, char **argv) {
    bool time_only = false, stats_only = false;
    for (int i = 1; i < argc; ++i) {
        if (!strcmp(argv[i], "nosplit")) g_split_bf16 = 0;
        if (!strcmp(argv[i], "time")) time_only = true;
        if (!strcmp(argv[i], "stats")) stats_only = true;
    }
    if (time_only) { time_rows(); return 0; }
    if (stats_only) { stats_rows(); return 0; }
    char name[64];
    for (int image = 1; image >= 0; --image) {       // rows A - I of tests/test_gpu_conv_route.py, with and without a split image
        const mi_conv_desc rows[9] = {linear(image, 3136), linear(image, 3200), glu3x3(image, 48, 2), glu3x3(image, 48, 2, false), glu3x3(image, 64, 1),
                                      glu3x3(image, 192, 1), encoder(image, 24, 128, 3, 16, 37, 40, 1), encoder(image, 20, 96, 2, 8, 61, 64, 1),
                                      encoder(image, 24, 128, 3, 16, 37, 40, 0)};
        for (int i = 0; i < 9; ++i) { snprintf(name, sizeof(name), "%c%s", 'A' + i, image ? "+x6" : ""); row(name, rows[i]); }
    }
    static const char *const kinds[3] = {"linear", "tap", "enc"};
    for (int kind = 0; kind < 3; ++kind) {           // the tile_m = 192 rows of tests/test_gpu_x6_tile192.py
        const int MN[4][2] = {{192, 200 * 128}, {192, 199 * 128}, {384, 100 * 128}, {384, 99 * 128}};
        for (auto &mn : MN) { snprintf(name, sizeof(name), "t192_%s_M%d_N%d", kinds[kind], mn[0], mn[1]); row(name, t192(mn[0], mn[1], 192, true, kind)); }
    }
    row("t192_linear_M1536_N3000", t192(1536, 3000, 192, true));
    row("t192_linear_M1536_N3200", t192(1536, 3200, 192, true));
    row("t192_linear_M384_flags0", t192(384, 200 * 128, 192, true, 0, 0));
    const int noimage[6][3] = {{384, 200 * 128, 0}, {192, 200 * 128, 0}, {384, 60 * 128, 0}, {384, 200 * 128, 1}, {384, 60 * 128, 1}, {192, 200 * 128, 2}};
    for (auto &c : noimage) { snprintf(name, sizeof(name), "t192_%s_M%d_N%d_noimage", kinds[c[2]], c[0], c[1]); row(name, t192(c[0], c[1], 192, false, c[2])); }
    row("t192_M256", t192(256, 200 * 128, 192, true, 0, MI_FLAG_LN, 256));
    row("t192_M96", t192(96, 200 * 128, 192, true, 0, MI_FLAG_LN, 96));
    row("t192_M192_Mpad384", t192(192, 200 * 128, 192, true, 0, MI_FLAG_LN, 384));
    // the half rules, one per flag set, at every M
    const int SR = MI_FLAG_SCALE | MI_FLAG_RES, LNH = MI_FLAG_LN | MI_FLAG_HEADS, LGI = MI_FLAG_LN | MI_FLAG_GELU | MI_FLAG_IMG;
    for (int M : {120, 128, 256, 384, 512}) {
        snprintf(name, sizeof(name), "half_xh_sr_M%d", M); row(name, half(M, SR));
        snprintf(name, sizeof(name), "half_xh_srs_M%d", M); row(name, half(M, SR | MI_FLAG_STATS));
        snprintf(name, sizeof(name), "half_xh_heads_M%d", M); row(name, half(M, LNH));
        snprintf(name, sizeof(name), "half_xh_ffn_M%d", M); row(name, half(M, LGI));
        snprintf(name, sizeof(name), "half_reg_M%d", M); row(name, half(M, 0, false));
    }
    {   // a DConv block's k = 3 conv 48 -> 24 with row statistics (what MI_NO_DMA_DCONV moves)
        mi_conv_desc c = base(24, 144, 32, false);
        c.B = 2, c.D1 = c.O1 = 1, c.D2 = c.O2 = 64, c.x_bstride = 48 * 64, c.epi = MI_EPI_BIAS_STATS, c.y_cstride = 64, c.ntaps = 3, c.tap_k2 = 3, c.tap_pad2 = 1;
        row("dconv_k3", c);
    }
    {   // a non-plain half layer, and one with tap-ordered weights
        mi_conv_desc e = encoder(false, 24, 256, 3, 16, 37, 40, 0);
        e.half = MI_DTYPE_BF16, e.wh = kPtr;
        row("half_encoder_M256", e);
        mi_conv_desc t = glu3x3(false, 64, 1);
        t.half = MI_DTYPE_BF16, t.xh = t.wtap = kPtr, t.xh_n = 384;
        row("half_wtap_M128", t);
    }
    // the nine descriptors tests/test_gpu_half_linear.py::test_refusals_launch_nothing refuses: five here, four in the launchers
    row("refuse_xh_gelu", half(512, MI_FLAG_GELU));
    row("refuse_ffn_M128", half(128, LGI));
    row("refuse_ffn_K36", half(256, LGI, true, 36));
    { mi_conv_desc d = half(512, LNH); d.xh_n = 79; row("refuse_heads_narrow_image", d); }
    row("refuse_heads_M256", half(256, LNH));
    { mi_conv_desc d = half(512, LNH); d.O1 = d.D1 = 2, d.O2 = d.D2 = 20; row("refuse_heads_frame", d); }
    { mi_conv_desc d = half(512, LNH); d.xh = (char *)kPtr + 8; row("refuse_heads_xh_off", d); }
    { mi_conv_desc d = half(512, LNH); d.yh = (char *)kPtr + 8; row("refuse_heads_yh_off", d); }
    { mi_conv_desc d = half(256, LGI); d.yh = (char *)kPtr + 8; row("refuse_ffn_yh_off", d); }
    return 0;
}
