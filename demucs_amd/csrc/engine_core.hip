// Host code both engines run: device memory, the profiler and the conv launcher, the side stream, weight packing and the DConv
// block.  No kernel lives here.
#include <cmath>
#include <string>
#include <vector>

#include "engine_core.h"

namespace mi {

// ------------------------------------------------------------------------------------------------
// device memory helpers
// ------------------------------------------------------------------------------------------------
int DeviceArena::alloc(void **p, size_t n) {
    n = (n + 255) & ~(size_t)255;
    hipError_t e = hipMalloc(p, n);
    if (e != hipSuccess) return set_error(MI_ENOMEM, "hipMalloc(%zu) failed: %s", n, hipGetErrorString(e));
    sizes[*p] = n;
    bytes += (int64_t)n;
    return MI_OK;
}
void DeviceArena::release(void *p) {
    auto it = sizes.find(p);
    if (it == sizes.end()) return;
    (void)hipFree(p);
    bytes -= (int64_t)it->second;
    sizes.erase(it);
}
DeviceArena::~DeviceArena() {
    for (auto &a : sizes) (void)hipFree(a.first);
}

int EngineCore::upload_fft_tables() {
    const FftHostTables h = fft_host_tables();
    float *dw, *de; float2 *dt;
    MI_TRY(upload(h.window, &dw)); MI_TRY(upload(h.twiddle, &dt)); MI_TRY(upload(h.envelope, &de));
    fft = FftTables{dw, dt, de};
    return MI_OK;
}

EngineCore::~EngineCore() {
    if (side_st) (void)hipStreamDestroy(side_st);
    if (ev_main) (void)hipEventDestroy(ev_main);
    if (ev_side) (void)hipEventDestroy(ev_side);
}

// run-time switch of the two-branch schedule (mi_set_two_streams: bench.py times its per-kernel roofline pass with one kernel
// on the GPU at a time)
int g_two_streams = 1;

// side stream and the two fork / join events of the two-branch schedule (created on first use)
int EngineCore::side_streams() {
    if (side_st) return MI_OK;
    // MI_SIDE_PRIO=low / high: the side stream at the device's least / greatest priority (A/B switch; default: normal priority)
    const int prio = switches().side_prio;
    if (prio) {
        int least = 0, greatest = 0;
        MI_HIP(hipDeviceGetStreamPriorityRange(&least, &greatest));
        MI_HIP(hipStreamCreateWithPriority(&side_st, hipStreamNonBlocking, prio < 0 ? least : greatest));
    } else
        MI_HIP(hipStreamCreateWithFlags(&side_st, hipStreamNonBlocking));
    MI_HIP(hipEventCreateWithFlags(&ev_main, hipEventDisableTiming));
    MI_HIP(hipEventCreateWithFlags(&ev_side, hipEventDisableTiming));
    return MI_OK;
}

// ------------------------------------------------------------------------------------------------
// profiler: one HIP event pair per launch of the instrumented kernel classes, on the launch stream
// ------------------------------------------------------------------------------------------------
hipEvent_t Profiler::get() {
    if (!pool.empty()) { hipEvent_t e = pool.back(); pool.pop_back(); return e; }
    hipEvent_t e;
    (void)hipEventCreate(&e);
    return e;
}
void Profiler::begin() {
    for (auto &r : rows) r = ProfRow();
    on = true;
}
int Profiler::end(hipStream_t st) {
    on = false;
    MI_HIP(hipStreamSynchronize(st));
    for (auto &p : pending) {
        float ms = 0.f;
        MI_HIP(hipEventElapsedTime(&ms, p.a, p.b));
        ProfRow &r = rows[p.cls];
        r.cls = p.cls; r.launches += p.launches; r.ms += ms; r.flops += p.flops; r.bytes += p.bytes;
        pool.push_back(p.a); pool.push_back(p.b);
    }
    pending.clear();
    return MI_OK;
}
Profiler::~Profiler() {
    for (auto &p : pending) { (void)hipEventDestroy(p.a); (void)hipEventDestroy(p.b); }
    for (auto e : pool) (void)hipEventDestroy(e);
}

static const char *kEpiNames[6] = {"linear", "glu", "bias_stats", "stats_only", "gn_glu", "convtr"};

int EngineCore::conv(const mi_conv_desc &d, hipStream_t st) {
    if (!prof.on) return launch_conv(d, st);
    // The row of this launch: which main loop runs is conv_route's answer, asked before the launch.  Rows stay keyed by the layer's
    // own tile (the one its float32 weights are packed for: conv_pick_tile(M) for a 192-row layer) and the descriptor's `plain`,
    // not by the small-batch or the 192-row tile the kernel runs
    const int route = conv_route(d).route;
    const int tile = d.tile_m && d.tile_m != 192 ? d.tile_m : conv_pick_tile(d.M), ti = tile == 32 ? 0 : tile == 64 ? 1 : tile == 96 ? 2 : 3;
    // bf16 / fp16 operand or split-bf16 main loops: classes of their own.  The split-bf16 tap convs (conv_tap_x6_kernel) and row-tap
    // convs (conv_rows_x6_kernel: the frequency branch's encoder / transposed convs, the encoders' 1 x 1 + GLU rewrites): rows of
    // their own, named after the kernel -- the conv_gemm_x6 rows stay the linears' ones.  The time branch's strided and transposed
    // convs of route 11 (conv_time_enc_x6_kernel, conv_time_tr_x6_kernel) stay on the rows the layers had on the table route,
    // conv_gemm<linear / convtr,tile>: the recorded launch census (tests/golden/launch_census.json) lists every row of a forward.
    // Kernel profiles keep them apart by symbol, and mi_debug_conv_route_launches counts the launches of a route
    const bool tap_x6 = route == MI_ROUTE_TAP_X6, rows_x6 = route == MI_ROUTE_ROWS_X6, time_x6 = route == MI_ROUTE_TIME_X6;
    const int cls = tap_x6    ? 105 + (d.ntaps == 9 ? 2 : 0) + (tile == 128 ? 1 : 0)
                    : rows_x6 ? 109 + (d.epi == MI_EPI_CONVTR ? 4 : d.epi == MI_EPI_GLU ? 2 : 0) + (tile == 128 ? 1 : 0)
                              : (route >= MI_ROUTE_X6 && !time_x6 ? 48 : 0) + d.epi * 8 + ti * 2 + (d.plain ? 1 : 0);
    const double N = (double)d.B * d.O1 * d.O2;
    // algorithmic work: 2*M*K flops per output column; bytes = input tensor + output tensor + weights, once each
    const double in_bytes = 4.0 * (double)d.B * (double)d.x_bstride;
    double out_rows = d.M;
    if (d.epi == MI_EPI_GLU || d.epi == MI_EPI_GN_GLU) out_rows = d.M / 2;
    if (d.epi == MI_EPI_CONVTR) out_rows = d.M;                     // 4 phases x Cout rows, each column scattered once
    if (d.epi == MI_EPI_STATS_ONLY) out_rows = 0;
    double bytes = in_bytes + 4.0 * out_rows * N + 4.0 * (double)d.M * d.K;
    if (d.flags & MI_FLAG_RES || d.epi == MI_EPI_GN_GLU) bytes += 4.0 * out_rows * N;
    char name[sizeof(ProfRow::name)];
    const bool unnamed = !prof.rows[cls].name[0];        // a row keeps the name its first launch gave it
    if (unnamed && tap_x6)
        snprintf(name, sizeof(name), "conv_tap_x6<%s,tile%d,taps%d>", kEpiNames[d.epi], tile, d.ntaps);
    else if (unnamed && rows_x6)
        snprintf(name, sizeof(name), "conv_rows_x6<%s,tile%d>", kEpiNames[d.epi], tile);
    else if (unnamed)
        snprintf(name, sizeof(name), "conv_gemm%s<%s,tile%d%s>", d.half == MI_DTYPE_BF16 ? "_bf16" : d.half == MI_DTYPE_F16 ? "_f16" : cls >= 48 ? "_x6" : "",
                 kEpiNames[d.epi], tile, d.plain ? ",1x1" : "");
    return prof.timed(cls, unnamed ? name : nullptr, 2.0 * d.M * (double)d.K * N, bytes, st, [&] { return launch_conv(d, st); });
}

// ------------------------------------------------------------------------------------------------
// weight lookup and packing
// ------------------------------------------------------------------------------------------------
// Second copy of the packed weights as exact 3-term bf16 tile images: selects the 6-product bf16 MFMA main loop
// (gemm_x6.hip).  Scope (stated by the call that packs the layer, engine_core.h SplitScope): by default the float32 engine's 44
// transformer linears (SPLIT_DEFAULT), where the split loop is
// ~1.4x faster than the native fp32 MFMA kernels, and its eight decoder rewrite convs (SPLIT_DEFAULT: dec[j] 3 x 3, tdec[j] k = 3,
// + GLU), which the shifted-run DMA tap loader feeds (conv_tap_x6_kernel; the table-driven gather in front of the split loop had
// measured slower than the native DMA tap loop), and the row-tap layers of the DMA row route (SPLIT_ROWS: enc[1..3].conv, k = 8,
// s = 4, + GELU; dec[0..2].convtr; the 128-row 1 x 1 + GLU rewrites of enc / tenc[2..3]), which the DMA row loader feeds
// (conv_rows_x6_kernel; not with MI_NO_DMA_ROWS=1, whose layers keep the native table routes), and the time branch's inner
// strided and transposed convs (SPLIT_TIME: tenc[1..3].conv, tdec[0..2].convtr), which the time-axis DMA loaders feed
// (conv_time_enc_x6_kernel, conv_time_tr_x6_kernel); MI_X6=0 packs none (A/B runs), MI_X6=1 every layer whose tile has the split
// loop.  When several PROCESSES share one GPU, split-loop results were
// intermittently corrupted (tests/test_gpu_distributed.py, tools/micro/det3.py; cause not found), so such a process
// selects the native kernels at run time (mi_set_split_bf16(0): demucs_amd/distributed.py does it for ranks that share
// a device); one process per GPU is the supported deployment.
int EngineCore::pack_split(PackedConv *pc, SplitScope scope) {
    const Switches &sw = switches();
    const bool in_default = scope == SPLIT_DEFAULT || scope == SPLIT_TIME || (scope == SPLIT_ROWS && !sw.no_dma_rows);
    const bool want = sw.x6_scope == 2 || (sw.x6_scope == 1 && in_default && cfg.dtype == MI_DTYPE_F32);
    if (!want || !conv_x6_supported(pc->tile)) return MI_OK;
    // M % 192 == 0 (decoders 0 .. 2 and their time twins, the self-attention in_proj, the deeper frequency-branch layers): 96-row
    // images, which the 192-row tile reads in pairs and the 96-row tile singly (gemm_conv.h tile_m = 192).  The float32 weights
    // and the bias keep conv_pick_tile's Mpad, which is M for these layers; the image costs the same 6 Kpad Mpad bytes as before
    const bool t192 = pc->M % 192 == 0 && pc->Mpad == pc->M;
    MI_TRY(weights.alloc(&pc->wx, (size_t)6 * pc->Kpad * pc->Mpad));
    MI_TRY(launch_pack_split(pc->wt, pc->Kpad, pc->Mpad, t192 ? 96 : pc->tile, pc->wx, nullptr));
    MI_HIP(hipStreamSynchronize(nullptr));
    if (t192) pc->tile = 192;
    return MI_OK;
}

// Reduced-precision compute modes: the weights a second time as the bf16 / fp16 operand image of gemm_half.hip
int EngineCore::pack_half(PackedConv *pc) {
    if (cfg.dtype == MI_DTYPE_F32) return MI_OK;
    const int Kh = round_up(pc->Kpad, 32);
    MI_TRY(weights.alloc(&pc->wh, (size_t)2 * Kh * pc->Mpad));
    pc->half = cfg.dtype;
    MI_TRY(launch_pack_half(pc->wt, pc->Kpad, pc->Mpad, cfg.dtype, pc->wh, nullptr));
    MI_HIP(hipStreamSynchronize(nullptr));
    return MI_OK;
}

// Conv / Linear weights W[M][K] (K = Cin*K1*K2 flattened) -> Wt[Kpad][Mpad]; `glu` interleaves the
// two GLU halves: packed row 2c = W[c], 2c+1 = W[c + M/2].
// half modes, k x k stride-1 convs whose input is written as an operand image: third copy of the weights, tap-ordered
int EngineCore::pack_tap(PackedConv *pc, int ntaps) {
    if (cfg.dtype == MI_DTYPE_F32 || switches().no_tap_image || ntaps < 2 || pc->K % ntaps || (pc->K / ntaps) % 8) return MI_OK;
    const int Cin = pc->K / ntaps;
    MI_TRY(weights.alloc(&pc->wtap, (size_t)16 * conv_tap_pairs_pad(Cin, ntaps) * pc->Mpad));
    pc->ntaps = ntaps;
    MI_TRY(launch_pack_tap(pc->wt, pc->Mpad, Cin, ntaps, cfg.dtype, pc->wtap, nullptr));
    MI_HIP(hipStreamSynchronize(nullptr));
    return MI_OK;
}

// half modes, encoder convs (k = 8, s = 4, pad 2) fed by a phase-split image (gemm_conv.h MI_FLAG_IMG4): the same weights as a stride-1
// two-tap conv over 4 Cin channels -- channel (octet, plane rho, ci % 8), tap j <-> original tap 4 (j - (rho >= 2)) + rho + 2
int EngineCore::pack_enc_tap(const float *W /* (M, Cin, 8) */, int Cin, PackedConv *pc) {
    if (cfg.dtype == MI_DTYPE_F32 || switches().no_enc_image || switches().no_tap_image || Cin % 8) return MI_OK;
    const int M = pc->M, K = 8 * Cin;
    std::vector<float> wt((size_t)K * pc->Mpad, 0.f);
    for (int m = 0; m < M; ++m)
        for (int ci = 0; ci < Cin; ++ci)
            for (int rho = 0; rho < 4; ++rho)
                for (int j = 0; j < 2; ++j) {
                    const int tau = 4 * (j - (rho >= 2)) + rho + 2, ce = ((ci >> 3) * 4 + rho) * 8 + (ci & 7);
                    wt[(size_t)(ce * 2 + j) * pc->Mpad + m] = W[((size_t)m * Cin + ci) * 8 + tau];
                }
    float *tmp = nullptr;
    MI_HIP(hipMalloc((void **)&tmp, wt.size() * sizeof(float)));
    MI_HIP(hipMemcpy(tmp, wt.data(), wt.size() * sizeof(float), hipMemcpyHostToDevice));
    int r = weights.alloc(&pc->wtap, (size_t)16 * conv_tap_pairs_pad(4 * Cin, 2) * pc->Mpad);
    if (r == MI_OK) r = launch_pack_tap(tmp, pc->Mpad, 4 * Cin, 2, cfg.dtype, pc->wtap, nullptr);
    (void)hipStreamSynchronize(nullptr);
    (void)hipFree(tmp);
    if (r == MI_OK) pc->ntaps = 2;
    return r;
}

int EngineCore::pack_conv(const float *W, const float *bias, int M, int K, bool glu, PackedConv *pc, int ntaps, SplitScope scope) {
    const int tile = conv_pick_tile(M);
    pc->M = M; pc->K = K; pc->Mpad = round_up(M, tile); pc->Kpad = round_up(K, 16); pc->tile = tile;
    std::vector<float> wt((size_t)pc->Kpad * pc->Mpad, 0.f), b(pc->Mpad, 0.f);
    for (int m = 0; m < M; ++m) {
        const int src = glu ? ((m & 1) ? (m >> 1) + M / 2 : (m >> 1)) : m;
        for (int k = 0; k < K; ++k) wt[(size_t)k * pc->Mpad + m] = W[(size_t)src * K + k];
        b[m] = bias ? bias[src] : 0.f;
    }
    MI_TRY(upload(wt, &pc->wt));
    MI_TRY(upload(b, &pc->bias));
    MI_TRY(pack_half(pc));
    MI_TRY(pack_tap(pc, ntaps));
    return pack_split(pc, scope);
}

// ConvTranspose(k = 2s, stride s) weights W[Cin][Cout][2s] -> s-phase GEMM (s = 4: k = 8; s = 2: k = 4): row m = s*co + r,
// k = 2*ci + j, tap = r + s*j (output index s*q + r - pad receives input q - j through tap r + s*j).
int EngineCore::pack_convtr(const float *W, const float *bias, int Cin, int Cout, PackedConv *pc, int stride, SplitScope scope) {
    const int M = stride * Cout, K = 2 * Cin, ks = 2 * stride;
    const int tile = conv_pick_tile(M);
    pc->M = M; pc->K = K; pc->Mpad = round_up(M, tile); pc->Kpad = round_up(K, 16); pc->tile = tile;
    std::vector<float> wt((size_t)pc->Kpad * pc->Mpad, 0.f), b(pc->Mpad, 0.f);
    for (int ci = 0; ci < Cin; ++ci)
        for (int co = 0; co < Cout; ++co)
            for (int r = 0; r < stride; ++r)
                for (int j = 0; j < 2; ++j)
                    wt[(size_t)(2 * ci + j) * pc->Mpad + stride * co + r] = W[((size_t)ci * Cout + co) * ks + r + stride * j];
    for (int co = 0; co < Cout; ++co)
        for (int r = 0; r < stride; ++r) b[stride * co + r] = bias[co];
    MI_TRY(upload(wt, &pc->wt));
    MI_TRY(upload(b, &pc->bias));
    MI_TRY(pack_half(pc));
    MI_TRY(pack_tap(pc, 2));             // k = 2 ci + j is already (channel, tap) order
    return pack_split(pc, scope);
}

// Linear layer applied to LayerNorm(x): fold the LayerNorm affine into the weights (MI_FLAG_LN in gemm_conv.h)
int EngineCore::pack_linear_ln(const float *W, const float *bias, const float *ln_w, const float *ln_b, int M, int K, PackedConv *pc,
                               float **c1, SplitScope scope) {
    std::vector<float> wf((size_t)M * K), c2(M), c1h(M);
    for (int m = 0; m < M; ++m) {
        double s1 = 0.0, s2 = bias ? (double)bias[m] : 0.0;
        for (int k = 0; k < K; ++k) {
            const float wp = W[(size_t)m * K + k] * ln_w[k];
            wf[(size_t)m * K + k] = wp;
            s1 += (double)wp;
            s2 += (double)W[(size_t)m * K + k] * (double)ln_b[k];
        }
        c1h[m] = (float)s1; c2[m] = (float)s2;
    }
    MI_TRY(pack_conv(wf.data(), c2.data(), M, K, false, pc, 0, scope));
    return pack_vec(c1h.data(), M, pc->Mpad, false, c1);
}

int EngineCore::pack_vec(const float *v, int n, int npad, bool glu, float **out) {
    std::vector<float> h(npad, 0.f);
    for (int m = 0; m < n; ++m) h[m] = v[glu ? ((m & 1) ? (m >> 1) + n / 2 : (m >> 1)) : m];
    return upload(h, out);
}

int EngineCore::make_ktab(const Gather &g, int Kpad, mi_ktab_entry **out) {
    return upload(build_ktab(g, round_up(Kpad, 32)), out);     // entries past Kpad are "never valid": the K step of 32 of gemm_half.hip
}

int EngineCore::load_dconv(const WeightTable &wt, const std::string &prefix, int C, int64_t chan_stride, int D2, bool freq, DConvW *dw, int comp) {
    const int h = C / comp;
    dw->h = h;
    dw->has_row = comp == 8 && freq && dconv_row_supported(C, D2);
    // MI_NO_DCONV_TIME (A/B switch): fall back to the implicit-GEMM route
    dw->has_time = comp == 8 && !freq && !switches().no_dconv_time && dconv_time_supported(C, D2);
    for (int d = 0; d < 2; ++d) {
        DConvLayerW &l = dw->l[d];
        const std::string p = prefix + ".dconv.layers." + std::to_string(d);
        const float *w0, *b0, *g1w, *g1b, *w3, *b3, *g2w, *g2b, *ls;
        MI_TRY(wt.get(p + ".0.weight", (int64_t)h * C * 3, &w0));
        MI_TRY(wt.get(p + ".0.bias", h, &b0));
        MI_TRY(wt.get(p + ".1.weight", h, &g1w));
        MI_TRY(wt.get(p + ".1.bias", h, &g1b));
        MI_TRY(wt.get(p + ".3.weight", (int64_t)2 * C * h, &w3));
        MI_TRY(wt.get(p + ".3.bias", 2 * C, &b3));
        MI_TRY(wt.get(p + ".4.weight", 2 * C, &g2w));
        MI_TRY(wt.get(p + ".4.bias", 2 * C, &g2b));
        MI_TRY(wt.get(p + ".6.scale", C, &ls));
        MI_TRY(pack_conv(w0, b0, h, 3 * C, false, &l.conv3));
        const int dil = 1 << d;
        MI_TRY(make_ktab(Gather{C, 1, 3, 1, dil, 0, dil, chan_stride, D2}, l.conv3.Kpad, &l.ktab3));
        // the hidden tensor is stored with hp = round_up(h, 16) channels (extra channels stay zero), so the
        // 1x1 conv sees K == Kpad and can take the table-free float4 loader
        const int hp = round_up(h, 16);
        std::vector<float> w3p((size_t)2 * C * hp, 0.f);
        for (int m = 0; m < 2 * C; ++m)
            for (int k = 0; k < h; ++k) w3p[(size_t)m * hp + k] = w3[(size_t)m * h + k];
        MI_TRY(pack_conv(w3p.data(), b3, 2 * C, hp, true, &l.conv1));
        MI_TRY(make_ktab(Gather{hp, 1, 1, 1, 1, 0, 0, chan_stride, D2}, l.conv1.Kpad, &l.ktab1));
        MI_TRY(pack_vec(g1w, h, h, false, &l.gn1_w));
        MI_TRY(pack_vec(g1b, h, h, false, &l.gn1_b));
        MI_TRY(pack_vec(g2w, 2 * C, l.conv1.Mpad, true, &l.gn2_w));
        MI_TRY(pack_vec(g2b, 2 * C, l.conv1.Mpad, true, &l.gn2_b));
        MI_TRY(pack_vec(ls, C, C, false, &l.ls));
        {   // implicit-GEMM route: sum z^2 = <wt, G>, sum z = ct . G[:, h] over the accumulators of gn_gelu_gram_kernel (entries of
            // the upper block triangle; blocks above the diagonal count twice; column h of G holds sum g)
            const int HP = gram_hp(h);
            std::vector<double> gw((size_t)HP * HP, 0.0), gc(HP, 0.0);
            double sb = 0.0, sbq = 0.0;
            for (int m = 0; m < 2 * C; ++m) { sb += (double)b3[m]; sbq += (double)b3[m] * (double)b3[m]; }
            for (int i = 0; i < h; ++i) {
                for (int k = 0; k < h; ++k) {
                    if ((k >> 5) < (i >> 5)) continue;
                    double a = 0.0;
                    for (int m = 0; m < 2 * C; ++m) a += (double)w3[(size_t)m * h + i] * (double)w3[(size_t)m * h + k];
                    gw[(size_t)i * HP + k] = (k >> 5) > (i >> 5) ? 2.0 * a : a;
                }
                double v = 0.0, c1 = 0.0;
                for (int m = 0; m < 2 * C; ++m) { v += 2.0 * (double)w3[(size_t)m * h + i] * (double)b3[m]; c1 += (double)w3[(size_t)m * h + i]; }
                gw[(size_t)i * HP + h] = v;
                gc[i] = c1;
            }
            MI_TRY(upload(gw, &l.gram_wt)); MI_TRY(upload(gc, &l.gram_ct));
            l.sum_b = sb; l.sum_bsq = sbq;
        }
        if (dw->has_row || dw->has_time) {          // packing of dconv_row.hip / dconv_time.hip (dconv_pack_host: the test entries pack with it too)
            const DConvHostPack pk = dconv_pack_host(C, h, w0, b0, g1w, g1b, w3, b3);
            float *p0, *p1, *p2, *p3, *p4, *p5, *p6, *p7;
            MI_TRY(upload(pk.w0, &p0)); MI_TRY(upload(pk.b0, &p1)); MI_TRY(upload(pk.g1w, &p2)); MI_TRY(upload(pk.g1b, &p3));
            MI_TRY(upload(pk.w3, &p4));
            MI_TRY(pack_vec(b3, 2 * C, 2 * C, false, &p5)); MI_TRY(pack_vec(g2w, 2 * C, 2 * C, false, &p6));
            MI_TRY(pack_vec(g2b, 2 * C, 2 * C, false, &p7));
            dw->row[d] = DConvRowLayer{p0, p1, p2, p3, p4, p5, p6, p7, l.ls};
            double *da, *dv, *dc, *de1, *de2;
            MI_TRY(upload(pk.gram_a, &da)); MI_TRY(upload(pk.gram_v, &dv)); MI_TRY(upload(pk.gram_c, &dc));
            MI_TRY(upload(pk.gram_e1, &de1)); MI_TRY(upload(pk.gram_e2, &de2));
            dw->tl[d] = DConvTimeLayer{dw->row[d], da, dv, dc, de1, de2, pk.sum_b3, pk.sum_b3sq};
        }
    }
    return MI_OK;
}

// ------------------------------------------------------------------------------------------------
// layer helpers
// ------------------------------------------------------------------------------------------------
// DConv residual branch, in place on x[b][C][D1][D2] (uses tmp of the same size and hidden of size/8)
int EngineCore::run_dconv(const DConvW &w, int C, const Geo &g, float *x, float *tmp, float *hidden, double *stats, float2 *st1,
                          float2 *st2, hipStream_t st, double *gram2, size_t gram2_cap) {
    if (!gram2) { gram2 = dconv_gram2; gram2_cap = dconv_gram2_bytes; }
    const int h = w.h, hp = round_up(h, 16);
    const int64_t P = (int64_t)g.D1 * g.pitch();
    const int rows = g.row_mode ? g.B * g.D1 : g.B;
    if (w.has_row && g.row_mode == 1) {      // both layers in one LDS-resident pass, in place
        DConvRowArgs a{{w.tl[0], w.tl[1]}, x, x, g.D1, g.D2};
        return prof.timed(101, "dconv_row_kernel", 2.0 * 2.0 * (3.0 * C * h + 2.0 * 2 * C * h) * (double)rows * g.D2,
                          2.0 * 4.0 * C * (double)rows * g.D2, st, [&] { return launch_dconv_row(a, C, rows, switches().dconv_row_lds, st); });
    }
    if (w.has_time && g.row_mode == 0 && g.D1 == 1) {     // time branch, C = 48 / 96: three streaming VALU passes per layer
        MI_REQUIRE(dconv_gram, "dconv: the engine set no Gram buffer for the time kernels");
        return prof.timed(102, "dconv_time_kernels", 2.0 * 2.0 * (3.0 * C * h + 2.0 * C * h) * (double)g.B * g.D2, 2.0 * 4.0 * C * (double)g.B * g.D2, st, [&] {
            float *s = x, *dd = tmp;
            for (int dlayer = 0; dlayer < 2; ++dlayer) {
                MI_TRY(launch_dconv_time_layer(w.tl[dlayer], C, 1 << dlayer, g.B, g.D2, g.pitch(), s, dd, hidden, stats, dconv_gram, st1, st2, st));
                std::swap(s, dd);
            }
            return (int)MI_OK;   // two layers: result is back in x
        });
    }
    const double cnt_row = g.row_mode ? (double)g.D2 : (double)g.D1 * g.D2;
    float *src = x, *dst = tmp;
    for (int dlayer = 0; dlayer < 2; ++dlayer) {
        const DConvLayerW &l = w.l[dlayer];
        mi_conv_desc d = base_desc(l.conv3, l.ktab3, src, (int64_t)C * P, g);
        d.epi = MI_EPI_BIAS_STATS; d.y = hidden; d.y_bstride = (int64_t)hp * P; d.y_cstride = P; d.stats = stats;
        if (dconv_tap_dma) {     // the conv's geometry (k = 3, dilation 2^dlayer = padding): float32 runs it on the DMA tap loop; x / tmp carry slack
            d.ntaps = 3; d.tap_k2 = 3; d.tap_pad1 = 0; d.tap_pad2 = 1 << dlayer; d.tap_dil2 = 1 << dlayer;
        }
        MI_TRY(conv(d, st));
        MI_TRY(launch_finalize_stats(stats, rows, cnt_row * h, 1e-5f, 0, st1, nullptr, st));
        // GroupNorm + GELU of the hidden tensor in place, and in the same pass the Gram sums from which the second GroupNorm's
        // statistics follow (no statistics-only evaluation of the 2C x h GEMM)
        const int gslots = g.row_mode ? 1 : 8, HP = gram_hp(h);
        MI_REQUIRE((size_t)rows * gslots * HP * HP * sizeof(double) <= gram2_cap, "dconv: Gram accumulators need %zu bytes, workspace has %zu",
                   (size_t)rows * gslots * HP * HP * sizeof(double), gram2_cap);
        MI_TRY(launch_gn_gelu_gram(hidden, g.B, h, hp, g.D1, g.D2, g.pitch(), g.row_mode, st1, l.gn1_w, l.gn1_b, gram2, gslots, true, st));
        MI_TRY(launch_gram_finalize(gram2, rows, h, gslots, l.gram_wt, l.gram_ct, l.sum_b, l.sum_bsq, cnt_row, cnt_row * 2 * C, 1e-5f, st2, st));
        mi_conv_desc e = base_desc(l.conv1, l.ktab1, hidden, (int64_t)hp * P, g);
        e.plain = 1;
        e.epi = MI_EPI_GN_GLU; e.stats = nullptr; e.gn_stats = (const float *)st2; e.gn_w = l.gn2_w; e.gn_b = l.gn2_b;
        e.scale = l.ls; e.res = src; e.y = dst; e.y_bstride = (int64_t)C * P; e.y_cstride = P;
        MI_TRY(conv(e, st));
        std::swap(src, dst);
    }
    return MI_OK;   // two layers: result is back in x
}

}  // namespace mi
