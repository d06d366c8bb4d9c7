// The conv route table on the CPU: links demucs_amd/csrc/conv_route.hip and switches.hip, nothing else of the library, and
// prints for each descriptor below one line `name route tile plain`, or `name invalid: <message>` where conv_validate refuses
// it.  No GPU, no HIP call, no pointer followed: small aligned numbers stand in for the descriptors' pointers.  The MI_*
// environment decides as in the library; the argument `nosplit` is mi_set_split_bf16(0).  tests/test_conv_route_host.py
// builds and runs it and holds the expectations.
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

static void row(const char *name, const mi_conv_desc &d) {
    if (conv_validate(d) != MI_OK) { printf("%s invalid: %s\n", name, last_error_buf()); return; }
    const ConvRoute r = conv_route(d);
    printf("%s %d %d %d\n", name, r.route, r.tile, (int)r.plain);
}

int main(int argc, char **argv) {
    if (argc > 1 && !strcmp(argv[1], "nosplit")) g_split_bf16 = 0;
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
