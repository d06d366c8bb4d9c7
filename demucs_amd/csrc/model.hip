// HTDemucs segment forward on gfx950: weight packing + kernel orchestration.
//
// Mirrors HTDemucs.forward in eval mode (reference: demucs/htdemucs.py:527-660) for the released
// htdemucs family (depth 4, channels 48, nfft 4096, dconv_mode 3, bottom_channels 512, 5
// transformer layers, 8 heads).  Every activation is channel-first with the position axis
// contiguous: frequency branch x[b][C][Fr][T], time branch xt[b][C][L], transformer tokens
// x[b][512][tokens] (token order irrelevant to attention, so the reference's "(t1 fr)" rearrange
// of transformer.py:653-654 is never materialised; the positional table is stored in our order).
#include <cmath>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "common.h"
#include "gemm_conv.h"
#include "kernels.h"
#include "model.h"
#include "model_internal.h"

namespace mi {

// ------------------------------------------------------------------------------------------------
// device memory helpers
// ------------------------------------------------------------------------------------------------
int Model::dev_alloc(void **p, size_t bytes) {
    bytes = (bytes + 255) & ~(size_t)255;
    hipError_t e = hipMalloc(p, bytes);
    if (e != hipSuccess) return set_error(MI_ENOMEM, "hipMalloc(%zu) failed: %s", bytes, hipGetErrorString(e));
    allocs.push_back(*p);
    device_bytes += (int64_t)bytes;
    return MI_OK;
}

template <typename T>
int Model::upload(const std::vector<T> &h, T **dptr) {
    void *p = nullptr;
    MI_TRY(dev_alloc(&p, std::max<size_t>(h.size(), 1) * sizeof(T)));
    MI_HIP(hipMemcpy(p, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice));
    *dptr = (T *)p;
    return MI_OK;
}

int Model::upload_fft_tables() {
    const FftHostTables h = fft_host_tables();
    float *dw, *de; float2 *dt;
    MI_TRY(upload(h.window, &dw)); MI_TRY(upload(h.twiddle, &dt)); MI_TRY(upload(h.envelope, &de));
    fft = FftTables{dw, dt, de};
    return MI_OK;
}

Model::~Model() {
    for (void *p : allocs) (void)hipFree(p);
    if (side_st) (void)hipStreamDestroy(side_st);
    if (ev_main) (void)hipEventDestroy(ev_main);
    if (ev_side) (void)hipEventDestroy(ev_side);
}

// run-time switch of the two-branch schedule (mi_set_two_streams: bench.py times its per-kernel roofline pass with one kernel
// on the GPU at a time)
int g_two_streams = 1;

// side stream and the two fork / join events of the two-branch schedule (created on first use)
int Model::side_streams() {
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

int Model::conv(const mi_conv_desc &d, hipStream_t st) {
    if (!prof.on) return launch_conv(d, st);
    // The row of this launch: which main loop runs is conv_route's answer, asked before the launch.  Rows stay keyed by the layer's
    // own tile (the one its float32 weights are packed for: conv_pick_tile(M) for a 192-row layer) and the descriptor's `plain`,
    // not by the small-batch or the 192-row tile the kernel runs
    const int route = conv_route(d).route;
    const int tile = d.tile_m && d.tile_m != 192 ? d.tile_m : conv_pick_tile(d.M), ti = tile == 32 ? 0 : tile == 64 ? 1 : tile == 96 ? 2 : 3;
    // bf16 / fp16 operand or split-bf16 main loops: classes of their own.  The split-bf16 tap convs (conv_tap_x6_kernel) and row-tap
    // convs (conv_rows_x6_kernel: the frequency branch's encoder / transposed convs, the encoders' 1 x 1 + GLU rewrites): rows of
    // their own, named after the kernel -- the conv_gemm_x6 rows stay the linears' ones
    const bool tap_x6 = route == MI_ROUTE_TAP_X6, rows_x6 = route == MI_ROUTE_ROWS_X6;
    const int cls = tap_x6    ? 105 + (d.ntaps == 9 ? 2 : 0) + (tile == 128 ? 1 : 0)
                    : rows_x6 ? 109 + (d.epi == MI_EPI_CONVTR ? 4 : d.epi == MI_EPI_GLU ? 2 : 0) + (tile == 128 ? 1 : 0)
                              : (route >= MI_ROUTE_X6 ? 48 : 0) + d.epi * 8 + ti * 2 + (d.plain ? 1 : 0);
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

// The float32 engine's attention core runs on the split-bf16 kernel (attention_x6.hip) in the scope of the split linears:
// unless MI_X6=0, and while the process-wide switch is on (read here, at every launch, as launch_conv does).
int Model::attn(const float *q, const float *k, const float *v, float *o, int B, int Tq, int Tk, int64_t q_bs, int64_t kv_bs,
                int64_t o_bs, hipStream_t st, bool image) {
    void *oh = image ? (void *)o : nullptr;               // the image takes the place (half the bytes) of the float32 tensor
    const int64_t oh_n = (int64_t)B * Tq;
    const bool x6 = cfg.dtype == MI_DTYPE_F32 && !image && g_split_bf16 && switches().x6_scope != 0;
    auto launch = [&]() {
        return x6 ? launch_attention_x6(q, k, v, o, B, 8, Tq, Tk, q_bs, kv_bs, o_bs, st)
                  : launch_attention(q, k, v, o, B, 8, Tq, Tk, q_bs, kv_bs, o_bs, cfg.dtype, st, oh, oh_n);
    };
    const int cls = x6 ? 104 : 100;          // 101-103 are the DConv and LSTM rows
    const char *name = x6 ? "attention_x6_kernel" : cfg.dtype == MI_DTYPE_BF16 ? "attention_bf16_kernel" : cfg.dtype == MI_DTYPE_F16 ? "attention_f16_kernel" : "attention_kernel";
    // QK^T and PV: 2 * 2 * Tq * Tk * 64 flops per head (fp32-equivalent on the split kernel); bytes = q, k, v read once + o written
    return prof.timed(cls, name, 4.0 * B * 8 * (double)Tq * Tk * 64.0, 4.0 * B * 512.0 * (2.0 * Tq + 2.0 * Tk), st, launch);
}

// half modes: per-head 16-bit operands [B][8][T][64] (written by the projections' MI_FLAG_HEADS epilogue); the output is always
// out_proj's operand image
int Model::attn_heads(const void *q, const void *k, const void *v, float *o, int B, int Tq, int Tk, hipStream_t st) {
    const int64_t oh_n = (int64_t)B * Tq;
    const void *zero = conv_zero_page();
    MI_REQUIRE(zero, "attention: could not allocate the zero page");
    return prof.timed(100, cfg.dtype == MI_DTYPE_BF16 ? "attention_heads_bf16_kernel" : "attention_heads_f16_kernel",
                      4.0 * B * 8 * (double)Tq * Tk * 64.0, 2.0 * B * 512.0 * (2.0 * Tq + 2.0 * Tk), st,
                      [&] { return launch_attention_heads(q, k, v, zero, B, 8, Tq, Tk, Tq, Tk, cfg.dtype, o, oh_n, nullptr, 0, st); });
}

// ------------------------------------------------------------------------------------------------
// weight lookup and packing
// ------------------------------------------------------------------------------------------------
// Second copy of the packed weights as exact 3-term bf16 tile images: selects the 6-product bf16 MFMA main loop
// (gemm_x6.hip).  Scope (stated by the call that packs the layer, model.h SplitScope): by default the float32 engine's 44
// transformer linears (SPLIT_DEFAULT), where the split loop is
// ~1.4x faster than the native fp32 MFMA kernels, and its eight decoder rewrite convs (SPLIT_DEFAULT: dec[j] 3 x 3, tdec[j] k = 3,
// + GLU), which the shifted-run DMA tap loader feeds (conv_tap_x6_kernel; the table-driven gather in front of the split loop had
// measured slower than the native DMA tap loop), and the row-tap layers of the DMA row route (SPLIT_ROWS: enc[1..3].conv, k = 8,
// s = 4, + GELU; dec[0..2].convtr; the 128-row 1 x 1 + GLU rewrites of enc / tenc[2..3]), which the DMA row loader feeds
// (conv_rows_x6_kernel; not with MI_NO_DMA_ROWS=1, whose layers keep the native table routes); MI_X6=0 packs none (A/B runs), MI_X6=1 every layer whose tile has the split
// loop.  When several PROCESSES share one GPU, split-loop results were
// intermittently corrupted (tests/test_gpu_distributed.py, tools/micro/det3.py; cause not found), so such a process
// selects the native kernels at run time (mi_set_split_bf16(0): demucs_amd/distributed.py does it for ranks that share
// a device); one process per GPU is the supported deployment.
int Model::pack_split(PackedConv *pc, SplitScope scope) {
    const Switches &sw = switches();
    const bool in_default = scope == SPLIT_DEFAULT || (scope == SPLIT_ROWS && !sw.no_dma_rows);
    const bool want = sw.x6_scope == 2 || (sw.x6_scope == 1 && in_default && cfg.dtype == MI_DTYPE_F32);
    if (!want || !conv_x6_supported(pc->tile)) return MI_OK;
    // M % 192 == 0 (decoders 0 .. 2 and their time twins, the self-attention in_proj, the deeper frequency-branch layers): 96-row
    // images, which the 192-row tile reads in pairs and the 96-row tile singly (gemm_conv.h tile_m = 192).  The float32 weights
    // and the bias keep conv_pick_tile's Mpad, which is M for these layers; the image costs the same 6 Kpad Mpad bytes as before
    const bool t192 = pc->M % 192 == 0 && pc->Mpad == pc->M;
    MI_TRY(dev_alloc(&pc->wx, (size_t)6 * pc->Kpad * pc->Mpad));
    MI_TRY(launch_pack_split(pc->wt, pc->Kpad, pc->Mpad, t192 ? 96 : pc->tile, pc->wx, nullptr));
    MI_HIP(hipStreamSynchronize(nullptr));
    if (t192) pc->tile = 192;
    return MI_OK;
}

// Reduced-precision compute modes: the weights a second time as the bf16 / fp16 operand image of gemm_half.hip
int Model::pack_half(PackedConv *pc) {
    if (cfg.dtype == MI_DTYPE_F32) return MI_OK;
    const int Kh = round_up(pc->Kpad, 32);
    MI_TRY(dev_alloc(&pc->wh, (size_t)2 * Kh * pc->Mpad));
    pc->half = cfg.dtype;
    MI_TRY(launch_pack_half(pc->wt, pc->Kpad, pc->Mpad, cfg.dtype, pc->wh, nullptr));
    MI_HIP(hipStreamSynchronize(nullptr));
    return MI_OK;
}

// Conv / Linear weights W[M][K] (K = Cin*K1*K2 flattened) -> Wt[Kpad][Mpad]; `glu` interleaves the
// two GLU halves: packed row 2c = W[c], 2c+1 = W[c + M/2].
// half modes, k x k stride-1 convs whose input is written as an operand image: third copy of the weights, tap-ordered
int Model::pack_tap(PackedConv *pc, int ntaps) {
    if (cfg.dtype == MI_DTYPE_F32 || switches().no_tap_image || ntaps < 2 || pc->K % ntaps || (pc->K / ntaps) % 8) return MI_OK;
    const int Cin = pc->K / ntaps;
    MI_TRY(dev_alloc(&pc->wtap, (size_t)16 * conv_tap_pairs_pad(Cin, ntaps) * pc->Mpad));
    pc->ntaps = ntaps;
    MI_TRY(launch_pack_tap(pc->wt, pc->Mpad, Cin, ntaps, cfg.dtype, pc->wtap, nullptr));
    MI_HIP(hipStreamSynchronize(nullptr));
    return MI_OK;
}

// half modes, encoder convs (k = 8, s = 4, pad 2) fed by a phase-split image (gemm_conv.h MI_FLAG_IMG4): the same weights as a stride-1
// two-tap conv over 4 Cin channels -- channel (octet, plane rho, ci % 8), tap j <-> original tap 4 (j - (rho >= 2)) + rho + 2
int Model::pack_enc_tap(const float *W /* (M, Cin, 8) */, int Cin, PackedConv *pc) {
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
    int r = dev_alloc(&pc->wtap, (size_t)16 * conv_tap_pairs_pad(4 * Cin, 2) * pc->Mpad);
    if (r == MI_OK) r = launch_pack_tap(tmp, pc->Mpad, 4 * Cin, 2, cfg.dtype, pc->wtap, nullptr);
    (void)hipStreamSynchronize(nullptr);
    (void)hipFree(tmp);
    if (r == MI_OK) pc->ntaps = 2;
    return r;
}

int Model::pack_conv(const float *W, const float *bias, int M, int K, bool glu, PackedConv *pc, int ntaps, SplitScope scope) {
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
int Model::pack_convtr(const float *W, const float *bias, int Cin, int Cout, PackedConv *pc, int stride, SplitScope scope) {
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
int Model::pack_linear_ln(const float *W, const float *bias, const float *ln_w, const float *ln_b, int M, int K, PackedConv *pc,
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

int Model::pack_vec(const float *v, int n, int npad, bool glu, float **out) {
    std::vector<float> h(npad, 0.f);
    for (int m = 0; m < n; ++m) h[m] = v[glu ? ((m & 1) ? (m >> 1) + n / 2 : (m >> 1)) : m];
    return upload(h, out);
}

int Model::make_ktab(const Gather &g, int Kpad, mi_ktab_entry **out) {
    return upload(build_ktab(g, round_up(Kpad, 32)), out);     // entries past Kpad are "never valid": the K step of 32 of gemm_half.hip
}

int Model::load_dconv(const WeightTable &wt, const std::string &prefix, int C, int64_t chan_stride, int D2, bool freq, DConvW *dw, int comp) {
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

static const int kFr[5] = {2048, 512, 128, 32, 8};
static const int kCh[4] = {48, 96, 192, 384};

int Model::init(const mi_config &c, const mi_tensor_desc *weights, size_t n) {
    cfg = c;
    MI_REQUIRE(c.n_sources >= 1 && c.n_sources <= 8, "n_sources %d unsupported", c.n_sources);
    MI_REQUIRE(c.max_batch >= 1 && c.max_batch <= 64, "max_batch %d out of range [1, 64]", c.max_batch);
    MI_REQUIRE(c.dtype == MI_DTYPE_F32 || c.dtype == MI_DTYPE_BF16 || c.dtype == MI_DTYPE_F16, "unknown compute dtype %d", c.dtype);
    MI_REQUIRE(c.segment_length > 4096 && c.segment_length % 4 == 0, "segment_length %d unsupported", c.segment_length);
    S = c.n_sources; SL = c.segment_length; T = (SL + 1023) / 1024;
    MI_REQUIRE(T % 4 == 0, "segment_length %d gives %d STFT frames; the engine needs a multiple of 4", SL, T);
    Lt[0] = SL;
    for (int i = 0; i < 4; ++i) Lt[i + 1] = (Lt[i] + 3) / 4;
    for (int i = 0; i < 5; ++i) Lp[i] = round_up(Lt[i], 4);
    MI_REQUIRE(Lt[4] % 4 == 0, "time branch bottleneck length %d must be a multiple of 4", Lt[4]);
    WeightTable wt;
    for (size_t i = 0; i < n; ++i) wt.t[weights[i].name] = {weights[i].data, weights[i].numel};

    // ---- FFT tables (window in float32 arithmetic like th.hann_window, spec.py:19,41) ------------
    MI_TRY(upload_fft_tables());

    // ---- encoders ---------------------------------------------------------------------------------
    for (int i = 0; i < 4; ++i) {
        const int Cin = i ? kCh[i - 1] : 4, C = kCh[i];
        const std::string p = "encoder." + std::to_string(i);
        const float *w, *b, *rw, *rb;
        MI_TRY(wt.get(p + ".conv.weight", (int64_t)C * Cin * 8, &w));
        MI_TRY(wt.get(p + ".conv.bias", C, &b));
        MI_TRY(wt.get(p + ".rewrite.weight", (int64_t)2 * C * C, &rw));
        MI_TRY(wt.get(p + ".rewrite.bias", 2 * C, &rb));
        EncW &e = enc[i];
        // level 0 (K = 32) is bound by its output: native
        MI_TRY(pack_conv(w, b, C, Cin * 8, false, &e.conv, 0, i > 0 ? SPLIT_ROWS : SPLIT_OPT_IN));
        if (i) MI_TRY(pack_enc_tap(w, Cin, &e.conv));
        MI_TRY(make_ktab(Gather{Cin, 8, 1, 1, 1, 2, 0, (int64_t)kFr[i] * T, T}, e.conv.Kpad, &e.ktab_conv));
        // 128-row rewrites; levels 0 / 1 (96 rows, K = 48 / 96) are bound by their output
        MI_TRY(pack_conv(rw, rb, 2 * C, C, true, &e.rewrite, 0, i >= 2 ? SPLIT_ROWS : SPLIT_OPT_IN));
        MI_TRY(make_ktab(Gather{C, 1, 1, 1, 1, 0, 0, (int64_t)kFr[i + 1] * T, T}, e.rewrite.Kpad, &e.ktab_rw));
        MI_TRY(load_dconv(wt, p, C, (int64_t)kFr[i + 1] * T, T, true, &e.dconv));

        const int Cint = i ? kCh[i - 1] : 2;
        const std::string pt = "tencoder." + std::to_string(i);
        MI_TRY(wt.get(pt + ".conv.weight", (int64_t)C * Cint * 8, &w));
        MI_TRY(wt.get(pt + ".conv.bias", C, &b));
        MI_TRY(wt.get(pt + ".rewrite.weight", (int64_t)2 * C * C, &rw));
        MI_TRY(wt.get(pt + ".rewrite.bias", 2 * C, &rb));
        EncW &te = tenc[i];
        MI_TRY(pack_conv(w, b, C, Cint * 8, false, &te.conv));
        if (i) MI_TRY(pack_enc_tap(w, Cint, &te.conv));
        MI_TRY(make_ktab(Gather{Cint, 1, 8, 1, 1, 0, 2, (int64_t)Lp[i], Lp[i]}, te.conv.Kpad, &te.ktab_conv));
        MI_TRY(pack_conv(rw, rb, 2 * C, C, true, &te.rewrite, 0, i >= 2 ? SPLIT_ROWS : SPLIT_OPT_IN));
        MI_TRY(make_ktab(Gather{C, 1, 1, 1, 1, 0, 0, (int64_t)Lp[i + 1], Lp[i + 1]}, te.rewrite.Kpad, &te.ktab_rw));
        MI_TRY(load_dconv(wt, pt, C, (int64_t)Lp[i + 1], Lp[i + 1], false, &te.dconv));
    }
    {   // freq embedding table: 0.2 * (10 * weight).t()  -> [48][512]   (htdemucs.py:577-582, hdemucs.py:60-66)
        const float *ew;
        MI_TRY(wt.get("freq_emb.embedding.weight", 512 * 48, &ew));
        std::vector<float> emb(48 * 512);
        for (int f = 0; f < 512; ++f)
            for (int ch = 0; ch < 48; ++ch) emb[ch * 512 + f] = 0.2f * (ew[f * 48 + ch] * 10.0f);
        MI_TRY(upload(emb, &freq_emb));
    }
    // ---- decoders ---------------------------------------------------------------------------------
    for (int j = 0; j < 4; ++j) {
        const int C = kCh[3 - j], Fr = kFr[4 - j];
        const int Cout = j < 3 ? kCh[2 - j] : 4 * S, Coutt = j < 3 ? kCh[2 - j] : 2 * S;
        const std::string p = "decoder." + std::to_string(j);
        const float *w, *b, *rw, *rb;
        MI_TRY(wt.get(p + ".conv_tr.weight", (int64_t)C * Cout * 8, &w));
        MI_TRY(wt.get(p + ".conv_tr.bias", Cout, &b));
        MI_TRY(wt.get(p + ".rewrite.weight", (int64_t)2 * C * C * 9, &rw));
        MI_TRY(wt.get(p + ".rewrite.bias", 2 * C, &rb));
        DecW &dd = dec[j];
        MI_TRY(pack_conv(rw, rb, 2 * C, C * 9, true, &dd.rewrite, 9, SPLIT_DEFAULT));
        MI_TRY(make_ktab(Gather{C, 3, 3, 1, 1, 1, 1, (int64_t)Fr * T, T}, dd.rewrite.Kpad, &dd.ktab_rw));
        MI_TRY(load_dconv(wt, p, C, (int64_t)Fr * T, T, true, &dd.dconv));
        // the outermost one (K = 96, 64-row tile) is bound by its output: native
        MI_TRY(pack_convtr(w, b, C, Cout, &dd.convtr, 4, j < 3 ? SPLIT_ROWS : SPLIT_OPT_IN));
        MI_TRY(make_ktab(Gather{C, 2, 1, -1, 1, 0, 0, (int64_t)Fr * T, T}, dd.convtr.Kpad, &dd.ktab_tr));

        const int L = Lp[4 - j];          // row pitch of this level's time-branch tensors
        const std::string pt = "tdecoder." + std::to_string(j);
        MI_TRY(wt.get(pt + ".conv_tr.weight", (int64_t)C * Coutt * 8, &w));
        MI_TRY(wt.get(pt + ".conv_tr.bias", Coutt, &b));
        MI_TRY(wt.get(pt + ".rewrite.weight", (int64_t)2 * C * C * 3, &rw));
        MI_TRY(wt.get(pt + ".rewrite.bias", 2 * C, &rb));
        DecW &td = tdec[j];
        MI_TRY(pack_conv(rw, rb, 2 * C, C * 3, true, &td.rewrite, 3, SPLIT_DEFAULT));
        MI_TRY(make_ktab(Gather{C, 1, 3, 1, 1, 0, 1, (int64_t)L, L}, td.rewrite.Kpad, &td.ktab_rw));
        MI_TRY(load_dconv(wt, pt, C, (int64_t)L, L, false, &td.dconv));
        MI_TRY(pack_convtr(w, b, C, Coutt, &td.convtr));
        MI_TRY(make_ktab(Gather{C, 1, 2, 1, -1, 0, 0, (int64_t)L, L}, td.convtr.Kpad, &td.ktab_tr));
    }
    // ---- bottleneck 1x1 and transformer ------------------------------------------------------------
    const int Tf = 8 * T, Tt = Lt[4];
    {
        const char *names[4] = {"channel_upsampler", "channel_upsampler_t", "channel_downsampler", "channel_downsampler_t"};
        for (int i = 0; i < 4; ++i) {
            const int M = i < 2 ? 512 : 384, K = i < 2 ? 384 : 512, P = (i & 1) ? Tt : Tf;
            const float *w, *b;
            MI_TRY(wt.get(std::string(names[i]) + ".weight", (int64_t)M * K, &w));
            MI_TRY(wt.get(std::string(names[i]) + ".bias", M, &b));
            MI_TRY(pack_conv(w, b, M, K, false, &chan[i]));
            MI_TRY(make_ktab(Gather{K, 1, 1, 1, 1, 0, 0, (int64_t)P, P}, chan[i].Kpad, &chan_ktab[i]));
        }
        // plain [512 or 2048 channel] gathers for the transformer linears, per branch
        for (int br = 0; br < 2; ++br) {
            const int P = br ? Tt : Tf;
            MI_TRY(make_ktab(Gather{512, 1, 1, 1, 1, 0, 0, (int64_t)P, P}, 512, &tr_ktab512[br]));
            MI_TRY(make_ktab(Gather{2048, 1, 1, 1, 1, 0, 0, (int64_t)P, P}, 2048, &tr_ktab2048[br]));
        }
    }
    for (int br = 0; br < 2; ++br) {
        const std::string ni = br ? "crosstransformer.norm_in_t" : "crosstransformer.norm_in";
        const float *w, *b;
        MI_TRY(wt.get(ni + ".weight", 512, &w)); MI_TRY(wt.get(ni + ".bias", 512, &b));
        MI_TRY(pack_vec(w, 512, 512, false, &norm_in_w[br])); MI_TRY(pack_vec(b, 512, 512, false, &norm_in_b[br]));
        for (int k = 0; k < 5; ++k) {
            const std::string p = std::string("crosstransformer.") + (br ? "layers_t." : "layers.") + std::to_string(k);
            const bool cross = k & 1;
            const std::string at = p + (cross ? ".cross_attn" : ".self_attn");
            TrLayerW &l = tr[br][k];
            const float *ipw, *ipb, *ow, *ob, *w1, *b1, *w2, *b2;
            MI_TRY(wt.get(at + ".in_proj_weight", 1536 * 512, &ipw));
            MI_TRY(wt.get(at + ".in_proj_bias", 1536, &ipb));
            MI_TRY(wt.get(at + ".out_proj.weight", 512 * 512, &ow));
            MI_TRY(wt.get(at + ".out_proj.bias", 512, &ob));
            MI_TRY(wt.get(p + ".linear1.weight", 2048 * 512, &w1)); MI_TRY(wt.get(p + ".linear1.bias", 2048, &b1));
            MI_TRY(wt.get(p + ".linear2.weight", 512 * 2048, &w2)); MI_TRY(wt.get(p + ".linear2.bias", 512, &b2));
            const float *nw[4] = {}, *nb[4] = {};
            const char *nn[4] = {".norm1", ".norm2", ".norm3", ".norm_out"};
            for (int q = 0; q < 4; ++q) {
                if (q == 2 && !cross) continue;
                MI_TRY(wt.get(p + nn[q] + ".weight", 512, &nw[q])); MI_TRY(wt.get(p + nn[q] + ".bias", 512, &nb[q]));
            }
            MI_TRY(pack_vec(nw[3], 512, 512, false, &l.norm_w[3])); MI_TRY(pack_vec(nb[3], 512, 512, false, &l.norm_b[3]));
            if (cross) {     // q from norm1(own branch), k/v from norm2(other branch), FFN from norm3
                MI_TRY(pack_linear_ln(ipw, ipb, nw[0], nb[0], 512, 512, &l.q_proj, &l.q_c1, SPLIT_DEFAULT));
                MI_TRY(pack_linear_ln(ipw + 512 * 512, ipb + 512, nw[1], nb[1], 1024, 512, &l.kv_proj, &l.kv_c1, SPLIT_DEFAULT));
                MI_TRY(pack_linear_ln(w1, b1, nw[2], nb[2], 2048, 512, &l.lin1, &l.lin1_c1, SPLIT_DEFAULT));
            } else {
                MI_TRY(pack_linear_ln(ipw, ipb, nw[0], nb[0], 1536, 512, &l.qkv_proj, &l.qkv_c1, SPLIT_DEFAULT));
                MI_TRY(pack_linear_ln(w1, b1, nw[1], nb[1], 2048, 512, &l.lin1, &l.lin1_c1, SPLIT_DEFAULT));
            }
            MI_TRY(pack_conv(ow, ob, 512, 512, false, &l.out_proj, 0, SPLIT_DEFAULT));
            MI_TRY(pack_conv(w2, b2, 512, 2048, false, &l.lin2, 0, SPLIT_DEFAULT));
            MI_TRY(wt.get(p + ".gamma_1.scale", 512, &w)); MI_TRY(pack_vec(w, 512, 512, false, &l.gamma1));
            MI_TRY(wt.get(p + ".gamma_2.scale", 512, &w)); MI_TRY(pack_vec(w, 512, 512, false, &l.gamma2));
        }
    }
    {   // positional tables, float32 arithmetic like the reference (transformer.py:19-70), stored [512][tokens]
        std::vector<float> pe2((size_t)512 * Tf), pe1((size_t)512 * Tt);
        // 2-D: channels [0,256) encode width = time frame t1, [256,512) height = fr; our token = fr*T + t1
        for (int i = 0; i < 128; ++i) {
            const float div = expf((float)(2 * i) * (float)(-(log(10000.0) / 256.0)));
            for (int fr = 0; fr < 8; ++fr)
                for (int t1 = 0; t1 < T; ++t1) {
                    const size_t tok = (size_t)fr * T + t1;
                    pe2[(size_t)(2 * i) * Tf + tok] = sinf((float)t1 * div);
                    pe2[(size_t)(2 * i + 1) * Tf + tok] = cosf((float)t1 * div);
                    pe2[(size_t)(256 + 2 * i) * Tf + tok] = sinf((float)fr * div);
                    pe2[(size_t)(256 + 2 * i + 1) * Tf + tok] = cosf((float)fr * div);
                }
        }
        // 1-D: phase = pos / 10000^(i/255), [cos | sin]
        for (int i = 0; i < 256; ++i) {
            const float den = powf(10000.0f, (float)i / 255.0f);
            for (int t2 = 0; t2 < Tt; ++t2) {
                const float ph = (float)t2 / den;
                pe1[(size_t)i * Tt + t2] = cosf(ph);
                pe1[(size_t)(256 + i) * Tt + t2] = sinf(ph);
            }
        }
        MI_TRY(upload(pe2, &pos_emb[0])); MI_TRY(upload(pe1, &pos_emb[1]));
    }
    MI_TRY(alloc_workspace());
    {   // the forward's plan: every fact below is decided here and only read afterwards
        const Switches &sw = switches();
        const bool half = cfg.dtype != MI_DTYPE_F32;
        plan.ffn_img = half && !sw.no_ffn_image;
        plan.qkv_heads = plan.ffn_img && !sw.no_qkv_heads;
        plan.in_img = plan.qkv_heads && !sw.no_input_image;
        plan.lin2_stats = !sw.no_lin2_stats;
        plan.tap_img = half && dec[0].rewrite.wtap && tdec[0].rewrite.wtap;
        for (int i = 1; i < 4; ++i) {
            plan.enc_img[0][i] = enc[i].conv.wtap && w_eimg[0][i - 1];
            plan.enc_img[1][i] = tenc[i].conv.wtap && w_eimg[1][i - 1];
        }
    }
    MI_HIP(hipDeviceSynchronize());
    return MI_OK;
}

// ------------------------------------------------------------------------------------------------
// workspace
// ------------------------------------------------------------------------------------------------
int Workspace::alloc(void **p, size_t n) {
    n = (n + 255) & ~(size_t)255;
    hipError_t e = hipMalloc(p, n);
    if (e != hipSuccess) return set_error(MI_ENOMEM, "hipMalloc(%zu) failed: %s", n, hipGetErrorString(e));
    allocs.push_back(*p);
    bytes += (int64_t)n;
    return MI_OK;
}
Workspace::~Workspace() {
    for (void *p : allocs) (void)hipFree(p);
}

// process-wide registry: key -> live workspace (weak: freed with its last handle)
static std::mutex g_ws_mutex;
static std::map<std::string, std::weak_ptr<Workspace>> g_ws;

int Model::alloc_workspace() {
    int dev = 0;
    MI_HIP(hipGetDevice(&dev));
    char key[128];
    // half-mode workspaces carry the phase-split encoder images (fill_workspace): float32 and half models do not share one
    snprintf(key, sizeof(key), "htdemucs dev%d S%d SL%d B%d %s", dev, S, SL, cfg.max_batch, cfg.dtype == MI_DTYPE_F32 ? "f32" : "half");
    std::lock_guard<std::mutex> lock(g_ws_mutex);
    auto it = g_ws.find(key);
    if (it != g_ws.end()) ws = it->second.lock();
    if (!ws) {
        auto w = std::make_shared<Workspace>();
        w->key = key;
        MI_TRY(fill_workspace(*w));
        g_ws[key] = w;
        ws = w;
    }
    static_cast<WorkspacePtrs &>(*this) = *ws;
    dconv_tap_dma = true;        // fill_workspace gave w_a / w_b / w_ta / w_tb the slack the shifted DMA runs need
    return MI_OK;
}

int Model::fill_workspace(Workspace &w) {
    const size_t B = cfg.max_batch;
    auto A = [&](float **p, size_t per_item) { return w.alloc((void **)p, per_item * B * sizeof(float)); };
    auto dev_alloc = [&](void **p, size_t n) { return w.alloc(p, n); };
    MI_TRY(A(&w.w_xt0, (size_t)2 * SL));
    MI_TRY(A(&w.w_zt, (size_t)4 * 2048 * T));
    MI_TRY(A(&w.w_x0, (size_t)4 * 2048 * T));
    size_t big = 0;
    for (int i = 0; i < 4; ++i) {
        const size_t nf = (size_t)kCh[i] * kFr[i + 1] * T, nt = (size_t)kCh[i] * Lp[i + 1];
        MI_TRY(A(&w.w_skip[i], nf)); MI_TRY(A(&w.w_skip_t[i], nt));
        big = std::max(big, std::max(nf, nt));
    }
    if (cfg.dtype != MI_DTYPE_F32)
        for (int i = 0; i < 3; ++i) {        // phase-split images of the encoder outputs; the never-written slots are the convs' zero padding
            const size_t pqf = (size_t)(kFr[i + 1] / 4 + 1) * T, pqt = round_up(ceil_div(Lt[i + 1], 4) + 1, 4);
            float *pf = nullptr, *pt = nullptr;
            MI_TRY(A(&pf, 2 * kCh[i] * pqf)); MI_TRY(A(&pt, 2 * kCh[i] * pqt));
            MI_HIP(hipMemset(pf, 0, 2 * kCh[i] * pqf * B * sizeof(float)));
            MI_HIP(hipMemset(pt, 0, 2 * kCh[i] * pqt * B * sizeof(float)));
            w.w_eimg[0][i] = pf; w.w_eimg[1][i] = pt;
        }
    // scratch shared by all U-Net layers (largest layer: 48 x 512 x T)
    MI_TRY(A(&w.w_h, big / 2)); MI_TRY(A(&w.w_th, big / 2));
    // the decoder inputs and the DConv blocks' input / output pair: the float32 k x k convs read them by LDS-DMA in runs shifted by
    // one or two samples (gemm_conv.hip conv_gemm_dmatap_kernel), i.e. up to 8 bytes before the first and 20 after the last
    // element: 128 bytes of slack on both sides
    for (float **p : {&w.w_a, &w.w_b, &w.w_ta, &w.w_tb, &w.w_c, &w.w_tc}) {
        MI_TRY(w.alloc((void **)p, (big * B + 64) * sizeof(float)));
        *p += 32;
    }
    // DConv hidden tensors carry round_up(C/8, 16) channels; the padding channels must read as zero: every layer shares this buffer
    // at its own item stride, so gn_gelu_gram_kernel re-zeroes them in each use (zero_pad) (a NaN another item left there would survive 0 * x)
    MI_HIP(hipMemset(w.w_h, 0, (big / 2) * B * sizeof(float)));
    MI_HIP(hipMemset(w.w_th, 0, (big / 2) * B * sizeof(float)));
    const size_t Tf = 8 * (size_t)T, Tt = Lt[4];
    for (int br = 0; br < 2; ++br) {
        const size_t P = br ? Tt : Tf;
        MI_TRY(A(&w.w_tr_x[br][0], 512 * P)); MI_TRY(A(&w.w_tr_x[br][1], 512 * P));
        if (cfg.dtype != MI_DTYPE_F32) {       // half modes only: operand images of the layer inputs and of x1 (never read in f32)
            MI_TRY(A(&w.w_tr_ximg[br][0], 256 * P)); MI_TRY(A(&w.w_tr_ximg[br][1], 256 * P)); MI_TRY(A(&w.w_tr_x1img[br], 256 * P));
        }
        for (int q = 0; q < 2; ++q) MI_TRY(dev_alloc((void **)&w.w_tr_stat[br][q], B * P * sizeof(float2)));
        MI_TRY(dev_alloc((void **)&w.w_tr_stat1[br], B * P * sizeof(float2)));
        MI_TRY(A(&w.w_tr_qkv[br], 1536 * Tf)) /* cross layers: Q (512 x Tq) + KV (1024 x Tk) */; MI_TRY(A(&w.w_tr_att[br], 512 * P));
        MI_TRY(A(&w.w_tr_x1[br], 512 * P)); MI_TRY(A(&w.w_tr_x2[br], 512 * P)); MI_TRY(A(&w.w_tr_ffh[br], 2048 * P));
    }
    MI_TRY(A(&w.w_yspec, (size_t)4 * S * 2048 * T));
    MI_TRY(A(&w.w_ytime, (size_t)2 * S * SL));
    MI_TRY(A(&w.w_yt, (size_t)4 * S * 2048 * T));
    MI_TRY(A(&w.w_fr, (size_t)S * T * 2 * 4096));
    const size_t max_rows = B * 512;
    w.stats_bytes = max_rows * kStatSlots * 2 * sizeof(double);
    MI_TRY(dev_alloc((void **)&w.w_stats, w.stats_bytes));
    MI_TRY(dev_alloc((void **)&w.w_stats_t, w.stats_bytes));
    w.gram_bytes = B * kStatSlots * 96 * sizeof(double);          // dconv_time.hip: kGramMax doubles per slot
    MI_TRY(dev_alloc((void **)&w.w_gram, w.gram_bytes));
    MI_HIP(hipMemset(w.w_gram, 0, w.gram_bytes));
    w.gram2_bytes = B * ((size_t)4 << 20);                         // B x 512 rows x 32 x 32 float64 is the largest user
    MI_TRY(dev_alloc((void **)&w.w_gram2, w.gram2_bytes));
    MI_HIP(hipMemset(w.w_gram2, 0, w.gram2_bytes));
    w.gram2t_bytes = B * ((size_t)1 << 20);                        // the waveform branch's own accumulators (it runs on a side stream)
    MI_TRY(dev_alloc((void **)&w.w_gram2_t, w.gram2t_bytes));
    MI_HIP(hipMemset(w.w_gram2_t, 0, w.gram2t_bytes));
    MI_HIP(hipMemset(w.w_stats, 0, w.stats_bytes));      // finalize_stats re-zeroes after each use
    MI_HIP(hipMemset(w.w_stats_t, 0, w.stats_bytes));
    MI_TRY(dev_alloc((void **)&w.w_st1, max_rows * sizeof(float2)));
    MI_TRY(dev_alloc((void **)&w.w_st2, max_rows * sizeof(float2)));
    MI_TRY(dev_alloc((void **)&w.w_st1_t, max_rows * sizeof(float2)));
    MI_TRY(dev_alloc((void **)&w.w_st2_t, max_rows * sizeof(float2)));
    MI_TRY(dev_alloc((void **)&w.w_norm_f, B * sizeof(float2))); MI_TRY(dev_alloc((void **)&w.w_denorm_f, B * sizeof(float2)));
    MI_TRY(dev_alloc((void **)&w.w_norm_t, B * sizeof(float2))); MI_TRY(dev_alloc((void **)&w.w_denorm_t, B * sizeof(float2)));
    return MI_OK;
}

// MI_DEBUG_SYNC=1: synchronise after every stage and name it on stderr (locates a faulting kernel)
#define MI_STAGE(name)                                                                        \
    do {                                                                                      \
        if (switches().debug_sync) {                                                          \
            hipError_t _e = hipStreamSynchronize(st);                                         \
            fprintf(stderr, "[mi] reached %s (%s)\n", name, hipGetErrorString(_e));          \
            fflush(stderr);                                                                   \
            if (_e != hipSuccess) return set_error(MI_EHIP, "stage before %s failed: %s", name, hipGetErrorString(_e)); \
        }                                                                                     \
    } while (0)

// ------------------------------------------------------------------------------------------------
// layer helpers
// ------------------------------------------------------------------------------------------------
// DConv residual branch, in place on x[b][C][D1][D2] (uses tmp of the same size and hidden of size/8)
int Model::run_dconv(const DConvW &w, int C, const Geo &g, float *x, float *tmp, float *hidden, double *stats, float2 *st1,
                     float2 *st2, hipStream_t st, double *gram2, size_t gram2_cap) {
    if (!gram2) { gram2 = w_gram2; gram2_cap = gram2_bytes; }
    const int h = w.h, hp = round_up(h, 16);
    const int64_t P = (int64_t)g.D1 * g.pitch();
    const int rows = g.row_mode ? g.B * g.D1 : g.B;
    if (w.has_row && g.row_mode == 1) {      // both layers in one LDS-resident pass, in place
        DConvRowArgs a{{w.tl[0], w.tl[1]}, x, x, g.D1, g.D2};
        return prof.timed(101, "dconv_row_kernel", 2.0 * 2.0 * (3.0 * C * h + 2.0 * 2 * C * h) * (double)rows * g.D2,
                          2.0 * 4.0 * C * (double)rows * g.D2, st, [&] { return launch_dconv_row(a, C, rows, switches().dconv_row_lds, st); });
    }
    if (w.has_time && g.row_mode == 0 && g.D1 == 1) {     // time branch, C = 48 / 96: three streaming VALU passes per layer
        return prof.timed(102, "dconv_time_kernels", 2.0 * 2.0 * (3.0 * C * h + 2.0 * C * h) * (double)g.B * g.D2, 2.0 * 4.0 * C * (double)g.B * g.D2, st, [&] {
            float *s = x, *dd = tmp;
            for (int dlayer = 0; dlayer < 2; ++dlayer) {
                MI_TRY(launch_dconv_time_layer(w.tl[dlayer], C, 1 << dlayer, g.B, g.D2, g.pitch(), s, dd, hidden, stats, w_gram, st1, st2, st));
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

// one transformer layer for branch br: x (B,512,Tq) [+ other (B,512,Tk) for cross] -> out, with the per-token
// LayerNorm statistics of every tensor that feeds a LayerNorm travelling beside it (xstat / ostat -> outstat):
// the LayerNorms themselves are folded into the projections that consume them (MI_FLAG_LN).
int Model::run_tr_layer(int br, int k, int B, const float *x, const float2 *xstat, const float *other, const float2 *ostat,
                        float *out, float2 *outstat, hipStream_t st, const void *ximg, const void *oimg, void *outimg) {
    const TrLayerW &l = tr[br][k];
    const bool cross = k & 1;
    const int Tf = 8 * T, Tt = Lt[4];
    const int Tq = br ? Tt : Tf, Tk = cross ? (br ? Tf : Tt) : Tq;
    const Geo gq{B, 1, Tq, 0}, gk{B, 1, Tk, 0};
    float *qkv = w_tr_qkv[br], *att = w_tr_att[br], *x1 = w_tr_x1[br], *x2 = w_tr_x2[br], *ffh = w_tr_ffh[br];
    double *stats = br ? w_stats_t : w_stats;
    float2 *st1 = br ? w_st1_t : w_st1;
    // half modes: tensors that only feed the next matrix product (attention output, FFN hidden) are written as that product's
    // 16-bit operand image, in place of the float32 tensor, and consumed by the LDS-DMA main loop of gemm_half.hip
    // norm_out's statistics come from lin2's epilogue (MI_FLAG_STATS): ten launches and 1.7 GB of reads fewer per batched forward;
    // time-neutral on the two-stream schedule, where the separate pass was hidden (MI_NO_LIN2_STATS=1 restores it for A/B runs)
    // half modes: Q, K, V feed nothing but the attention kernel, so the projections write them ONLY as 16-bit per-head token-major
    // tensors (MI_FLAG_HEADS, no float32 copy) and attention_heads.hip moves K / V tiles global -> LDS by DMA (MI_NO_QKV_HEADS=1,
    // MI_NO_FFN_IMAGE=1: float32 tensors); with plan.in_img the layer inputs (ximg / oimg -> outimg) and x1 exist as operand images too
    const bool img = plan.ffn_img, heads = plan.qkv_heads, in_img = plan.in_img, lin2_stats = plan.lin2_stats;
    unsigned short *qh = reinterpret_cast<unsigned short *>(qkv);
    const size_t plane_q = (size_t)B * 512 * Tq, plane_k = (size_t)B * 512 * Tk;        // 16-bit elements of one of Q / K / V
    if (!cross) {
        mi_conv_desc d = base_desc(l.qkv_proj, tr_ktab512[br], x, (int64_t)512 * Tq, gq);
        d.plain = 1; d.epi = MI_EPI_LINEAR; d.flags = MI_FLAG_LN; d.scale = l.qkv_c1; d.pro_stats = (const float *)xstat;
        d.y = qkv; d.y_bstride = (int64_t)1536 * Tq; d.y_cstride = Tq;
        if (heads) { d.flags |= MI_FLAG_HEADS; d.yh = qh; d.yh_n = Tq; }
        if (in_img) { d.xh = ximg; d.xh_n = (int64_t)B * Tq; }
        MI_TRY(conv(d, st));
        if (heads) MI_TRY(attn_heads(qh, qh + plane_q, qh + 2 * plane_q, att, B, Tq, Tq, st));
        else MI_TRY(attn(qkv, qkv + (size_t)512 * Tq, qkv + (size_t)1024 * Tq, att, B, Tq, Tq, (int64_t)1536 * Tq, (int64_t)1536 * Tq,
                         (int64_t)512 * Tq, st, img));
    } else {
        mi_conv_desc d = base_desc(l.q_proj, tr_ktab512[br], x, (int64_t)512 * Tq, gq);
        d.plain = 1; d.epi = MI_EPI_LINEAR; d.flags = MI_FLAG_LN; d.scale = l.q_c1; d.pro_stats = (const float *)xstat;
        d.y = qkv; d.y_bstride = (int64_t)512 * Tq; d.y_cstride = Tq;
        if (heads) { d.flags |= MI_FLAG_HEADS; d.yh = qh; d.yh_n = Tq; }
        if (in_img) { d.xh = ximg; d.xh_n = (int64_t)B * Tq; }
        MI_TRY(conv(d, st));
        float *kv = qkv + (size_t)B * 512 * Tq;
        unsigned short *kvh = qh + plane_q;
        mi_conv_desc e = base_desc(l.kv_proj, tr_ktab512[1 - br], other, (int64_t)512 * Tk, gk);
        e.plain = 1; e.epi = MI_EPI_LINEAR; e.flags = MI_FLAG_LN; e.scale = l.kv_c1; e.pro_stats = (const float *)ostat;
        e.y = kv; e.y_bstride = (int64_t)1024 * Tk; e.y_cstride = Tk;
        if (heads) { e.flags |= MI_FLAG_HEADS; e.yh = kvh; e.yh_n = Tk; }
        if (in_img) { e.xh = oimg; e.xh_n = (int64_t)B * Tk; }
        MI_TRY(conv(e, st));
        if (heads) MI_TRY(attn_heads(qh, kvh, kvh + plane_k, att, B, Tq, Tk, st));
        else MI_TRY(attn(qkv, kv, kv + (size_t)512 * Tk, att, B, Tq, Tk, (int64_t)512 * Tq, (int64_t)1024 * Tk, (int64_t)512 * Tq, st, img));
    }
    {   // x1 = x + gamma_1 * (out_proj(att) + b)
        mi_conv_desc d = base_desc(l.out_proj, tr_ktab512[br], att, (int64_t)512 * Tq, gq);
        d.plain = 1; d.epi = MI_EPI_LINEAR; d.flags = MI_FLAG_SCALE | MI_FLAG_RES; d.scale = l.gamma1; d.res = x;
        d.y = x1; d.y_bstride = (int64_t)512 * Tq; d.y_cstride = Tq;
        if (img) { d.xh = att; d.xh_n = (int64_t)B * Tq; }
        MI_TRY(conv(d, st));
    }
    MI_TRY(launch_token_stats(x1, B, 512, Tq, w_tr_stat1[br], st, in_img ? w_tr_x1img[br] : nullptr, (int64_t)B * Tq, cfg.dtype));
    {
        mi_conv_desc d = base_desc(l.lin1, tr_ktab512[br], x1, (int64_t)512 * Tq, gq);
        d.plain = 1; d.epi = MI_EPI_LINEAR; d.flags = MI_FLAG_LN | MI_FLAG_GELU; d.scale = l.lin1_c1;
        d.pro_stats = (const float *)w_tr_stat1[br];
        d.y = ffh; d.y_bstride = (int64_t)2048 * Tq; d.y_cstride = Tq;
        if (img) { d.flags |= MI_FLAG_IMG; d.yh = ffh; d.yh_n = (int64_t)B * Tq; }
        if (in_img) { d.xh = w_tr_x1img[br]; d.xh_n = (int64_t)B * Tq; }
        MI_TRY(conv(d, st));
        mi_conv_desc e = base_desc(l.lin2, tr_ktab2048[br], ffh, (int64_t)2048 * Tq, gq);
        if (img) { e.xh = ffh; e.xh_n = (int64_t)B * Tq; }
        // norm_out's statistics (GroupNorm(1, 512) over (tokens, channels) per item) are accumulated by this epilogue
        e.plain = 1; e.epi = MI_EPI_LINEAR; e.flags = MI_FLAG_SCALE | MI_FLAG_RES; e.scale = l.gamma2; e.res = x1;
        if (lin2_stats) { e.flags |= MI_FLAG_STATS; e.stats = stats; }
        e.y = x2; e.y_bstride = (int64_t)512 * Tq; e.y_cstride = Tq;
        MI_TRY(conv(e, st));
    }
    // norm_out: GroupNorm(1, 512) over (tokens, channels) per item (transformer.py:258-268); the apply also
    // emits the per-token statistics the next layer's LayerNorms need
    if (!lin2_stats) MI_TRY(launch_row_stats(x2, B, (int64_t)512 * Tq, (int64_t)512 * Tq, stats, st));
    MI_TRY(launch_finalize_stats(stats, B, (double)512 * Tq, 1e-5f, 0, st1, nullptr, st));
    MI_TRY(launch_gn_apply_tokstats(x2, B, 512, Tq, st1, l.norm_w[3], l.norm_b[3], out, outstat, st, in_img ? outimg : nullptr,
                                    (int64_t)B * Tq, cfg.dtype));
    return MI_OK;
}

// ------------------------------------------------------------------------------------------------
// forward
// ------------------------------------------------------------------------------------------------
// run_core with the "statistics slots may be dirty" bookkeeping of the (possibly shared) workspace
int Model::run_core(const float *mix, const float *mag, int B, hipStream_t st) {
    if (ws->dirty) {
        MI_HIP(hipMemsetAsync(w_stats, 0, ws->stats_bytes, st));
        MI_HIP(hipMemsetAsync(w_stats_t, 0, ws->stats_bytes, st));
        MI_HIP(hipMemsetAsync(w_gram, 0, ws->gram_bytes, st));
        MI_HIP(hipMemsetAsync(w_gram2, 0, gram2_bytes, st));
        MI_HIP(hipMemsetAsync(w_gram2_t, 0, gram2t_bytes, st));
        ws->dirty = false;
    }
    const int r = run_core_impl(mix, mag, B, st);
    if (r != MI_OK) {
        ws->dirty = true;
        // a failure between fork() and the final join() leaves the side stream running kernels on the shared workspace that
        // the caller's stream never waits for: drain it here, so that the next forward's re-zeroing (and any other handle of
        // this workspace) cannot race with them
        if (side_st) (void)hipStreamSynchronize(side_st);
    }
    return r;
}

int Model::forward(const float *mix, float *out, int B, hipStream_t st) {
    MI_REQUIRE(mix && out, "forward: null buffer");
    MI_TRY(run_core(mix, nullptr, B, st));
    // ---- de-normalise, iSTFT, add the time branch (htdemucs.py:624-657) -----------------------------
    MI_TRY(launch_istft(w_yspec, B, S, SL, w_denorm_f, w_ytime, w_denorm_t, fft, w_yt, w_fr, out, st));
    MI_STAGE("istft done");
    return MI_OK;
}

// HTDemucs.forward_core (htdemucs.py:662-759): the network without iSTFT / branch sum.
// spec_out (B, S, 4, 2048, T) = decoder output * std + mean; time_out (B, S, 2, L) = time decoder * stdt + meant.
int Model::forward_core(const float *mix, const float *mag, float *spec_out, float *time_out, int B, hipStream_t st) {
    MI_REQUIRE(mix && spec_out && time_out, "forward_core: null buffer");
    MI_TRY(run_core(mix, mag, B, st));
    MI_TRY(launch_row_denorm(w_yspec, B, (int64_t)4 * S * 2048 * T, w_denorm_f, spec_out, st));
    MI_TRY(launch_row_denorm(w_ytime, B, (int64_t)2 * S * SL, w_denorm_t, time_out, st));
    return MI_OK;
}

// everything up to the decoder outputs: leaves w_yspec / w_ytime and the (mean, std) pairs in the workspace
int Model::run_core_impl(const float *mix, const float *mag, int B, hipStream_t st) {
    MI_REQUIRE(B >= 1 && B <= cfg.max_batch, "forward: batch %d outside [1, %d]", B, cfg.max_batch);
    const int Tf = 8 * T, Tt = Lt[4];
    // The waveform branch runs on a SIDE stream beside the spectral branch on the caller's stream: the two U-Net halves only
    // meet in the cross-transformer (once per layer: cross-attention reads the other branch's layer input) and in the final sum,
    // and their kernels -- a third of the spectral branch's size, many of them one or two waves of workgroups -- fill the tails
    // of each other's launches.  Every buffer the branches write is per branch (statistics slots, Gram accumulators, scratch).
    const bool two = !switches().one_stream && g_two_streams && !switches().debug_sync && side_streams() == MI_OK;
    hipStream_t stt = two ? side_st : st;
    auto fork = [&]() -> int {              // the side stream waits for everything enqueued on the caller's stream so far
        if (!two) return MI_OK;
        MI_HIP(hipEventRecord(ev_main, st));
        MI_HIP(hipStreamWaitEvent(side_st, ev_main, 0));
        return MI_OK;
    };
    auto join = [&]() -> int {              // the caller's stream waits for everything enqueued on the side stream so far
        if (!two) return MI_OK;
        MI_HIP(hipEventRecord(ev_side, side_st));
        MI_HIP(hipStreamWaitEvent(st, ev_side, 0));
        return MI_OK;
    };
    MI_TRY(fork());
    // ---- input statistics and normalisation (htdemucs.py:545-554) --------------------------------
    MI_TRY(launch_row_stats(mix, B, (int64_t)2 * SL, (int64_t)2 * SL, w_stats_t, stt));
    MI_TRY(launch_finalize_stats(w_stats_t, B, 2.0 * SL, 1e-5f, 1, w_norm_t, w_denorm_t, stt));
    MI_TRY(launch_row_affine(mix, B, (int64_t)2 * SL, w_norm_t, w_xt0, stt));
    MI_STAGE("time normalisation done");
    if (mag) {      // forward_core with a caller-computed spectrogram (htdemucs.py:662-690: `mag` is an INPUT there)
        const int64_t cnt = (int64_t)4 * 2048 * T;
        MI_TRY(launch_row_stats(mag, B, cnt, cnt, w_stats, st));
        MI_TRY(launch_finalize_stats(w_stats, B, (double)cnt, 1e-5f, 1, w_norm_f, w_denorm_f, st));
        MI_TRY(launch_row_affine(mag, B, cnt, w_norm_f, w_x0, st));
    } else {
        MI_TRY(launch_stft_frames(mix, B, SL, fft, w_zt, w_stats, st));
        MI_TRY(launch_finalize_stats(w_stats, B, 4.0 * 2048 * T, 1e-5f, 1, w_norm_f, w_denorm_f, st));
        MI_TRY(launch_cac_transpose(w_zt, B, T, w_norm_f, w_x0, st));
    }
    MI_STAGE("stft done");

    // ---- encoders ----------------------------------------------------------------------------------
    const float *xf = w_x0, *xt = w_xt0;
    for (int i = 0; i < 4; ++i) {
        const int Cin = i ? kCh[i - 1] : 4, Cint = i ? kCh[i - 1] : 2, C = kCh[i];
        {   // frequency branch
            const Geo gin{B, kFr[i], T, 1}, go{B, kFr[i + 1], T, 1};
            const int64_t Pin = (int64_t)kFr[i] * T, P = (int64_t)kFr[i + 1] * T;
            mi_conv_desc d = base_desc(enc[i].conv, enc[i].ktab_conv, xf, Cin * Pin, gin);
            d.O1 = kFr[i + 1]; d.S1 = 4; d.epi = MI_EPI_LINEAR; d.flags = MI_FLAG_GELU;
            d.y = w_a; d.y_bstride = C * P; d.y_cstride = P;
            d.dma_rows = 1;                  // taps along the frequency axis only (float32: LDS-DMA main loop, gemm_conv.hip)
            if (plan.enc_img[0][i]) {
                // the previous level's output as a phase-split image: a stride-1 two-tap conv over its slots (rows o1, o1 + 1)
                const int Q = kFr[i] / 4 + 1;
                d.xh = w_eimg[0][i - 1]; d.xh_n = (int64_t)cfg.max_batch * Q * T; d.wtap = enc[i].conv.wtap; d.ntaps = 2; d.tap_k2 = 1;
                d.D1 = Q; d.S1 = 1;
            }
            MI_TRY(conv(d, st));
            MI_STAGE("enc conv done");
            MI_TRY(run_dconv(enc[i].dconv, C, go, w_a, w_b, w_h, w_stats, w_st1, w_st2, st));
            MI_STAGE("enc dconv done");
            mi_conv_desc r = base_desc(enc[i].rewrite, enc[i].ktab_rw, w_a, C * P, go);
            r.plain = 1; r.epi = MI_EPI_GLU; r.y = w_skip[i]; r.y_bstride = C * P; r.y_cstride = P;
            if (i == 0) { r.flags = MI_FLAG_EMB; r.emb = freq_emb; }
            if (i < 3 && plan.enc_img[0][i + 1]) {
                const int64_t pq = (int64_t)(kFr[i + 1] / 4 + 1) * T;
                r.flags |= MI_FLAG_IMG4 | MI_FLAG_TR_FREQ; r.yh = w_eimg[0][i]; r.yh_pq = pq; r.yh_n = (int64_t)cfg.max_batch * pq;
            }
            MI_TRY(conv(r, st));
            xf = w_skip[i];
            MI_STAGE("enc rewrite done");
        }
        {   // time branch
            const Geo gin{B, 1, Lt[i], 0, Lp[i]}, go{B, 1, Lt[i + 1], 0, Lp[i + 1]};
            const int64_t P = Lp[i + 1];
            mi_conv_desc d = base_desc(tenc[i].conv, tenc[i].ktab_conv, xt, (int64_t)Cint * Lp[i], gin);
            d.O2 = Lp[i + 1]; d.o2_valid = Lt[i + 1]; d.S2 = 4; d.epi = MI_EPI_LINEAR; d.flags = MI_FLAG_GELU;
            d.y = w_ta; d.y_bstride = C * P; d.y_cstride = P;
            if (plan.enc_img[1][i]) {
                const int Qp = round_up(ceil_div(Lt[i], 4) + 1, 4);
                d.xh = w_eimg[1][i - 1]; d.xh_n = (int64_t)cfg.max_batch * Qp; d.wtap = tenc[i].conv.wtap; d.ntaps = 2; d.tap_k2 = 2;
                d.D2 = Qp; d.x_ld = Qp; d.S2 = 1;
            }
            MI_TRY(conv(d, stt));
            MI_TRY(run_dconv(tenc[i].dconv, C, go, w_ta, w_tb, w_th, w_stats_t, w_st1_t, w_st2_t, stt, w_gram2_t, gram2t_bytes));
            mi_conv_desc r = base_desc(tenc[i].rewrite, tenc[i].ktab_rw, w_ta, C * P, go);
            r.plain = 1; r.epi = MI_EPI_GLU; r.y = w_skip_t[i]; r.y_bstride = C * P; r.y_cstride = P;
            if (i < 3 && plan.enc_img[1][i + 1]) {
                const int64_t pq = round_up(ceil_div(Lt[i + 1], 4) + 1, 4);
                r.flags |= MI_FLAG_IMG4; r.yh = w_eimg[1][i]; r.yh_pq = pq; r.yh_n = (int64_t)cfg.max_batch * pq;
            }
            MI_TRY(conv(r, stt));
            xt = w_skip_t[i];
            MI_STAGE("tenc layer done");
        }
    }
    // ---- bottleneck: channel upsamplers, cross transformer, channel downsamplers -------------------
    int cur[2] = {0, 0};
    // half modes: the transformer's projections read 16-bit operand images of their inputs (written by the token kernels)
    const bool in_img = plan.in_img;
    for (int br = 0; br < 2; ++br) {
        const int P = br ? Tt : Tf;
        const Geo g{B, 1, P, 0};
        hipStream_t sb = br ? stt : st;
        mi_conv_desc d = base_desc(chan[br], chan_ktab[br], br ? xt : xf, (int64_t)384 * P, g);
        d.plain = 1; d.epi = MI_EPI_LINEAR; d.y = w_tr_x1[br]; d.y_bstride = (int64_t)512 * P; d.y_cstride = P;
        MI_TRY(conv(d, sb));
        MI_TRY(launch_layernorm_cf(w_tr_x1[br], B, 512, P, norm_in_w[br], norm_in_b[br], pos_emb[br], w_tr_x[br][0],
                                   w_tr_stat[br][0], sb, in_img ? w_tr_ximg[br][0] : nullptr, (int64_t)B * P, cfg.dtype));
    }
    MI_STAGE("upsample + norm_in done");
    for (int k = 0; k < 5; ++k) {
        const float *f_in = w_tr_x[0][cur[0]], *t_in = w_tr_x[1][cur[1]];
        const float2 *f_st = w_tr_stat[0][cur[0]], *t_st = w_tr_stat[1][cur[1]];
        const void *f_img = in_img ? w_tr_ximg[0][cur[0]] : nullptr, *t_img = in_img ? w_tr_ximg[1][cur[1]] : nullptr;
        // both branches' layer inputs are complete on BOTH streams (a cross layer reads the other branch's input, and a layer
        // overwrites the buffer the other branch read two layers ago)
        MI_TRY(join());
        MI_TRY(fork());
        MI_TRY(run_tr_layer(0, k, B, f_in, f_st, t_in, t_st, w_tr_x[0][cur[0] ^ 1], w_tr_stat[0][cur[0] ^ 1], st, f_img, t_img,
                            w_tr_ximg[0][cur[0] ^ 1]));
        MI_TRY(run_tr_layer(1, k, B, t_in, t_st, f_in, f_st, w_tr_x[1][cur[1] ^ 1], w_tr_stat[1][cur[1] ^ 1], stt, t_img, f_img,
                            w_tr_ximg[1][cur[1] ^ 1]));
        cur[0] ^= 1; cur[1] ^= 1;
        MI_STAGE("transformer layer done");
    }
    float *din = w_c, *dtin = w_tc;     // decoder inputs (previous output + skip)
    // half modes: a decoder layer's input feeds nothing but its k x k rewrite conv, so its producer (the channel down-sampler,
    // then each transposed conv + GELU + skip) writes it ONLY as that conv's 16-bit operand image, into the same buffers, and
    // the conv gathers its taps by LDS-DMA (gemm_tap.hip)
    const bool tapimg = plan.tap_img;
    for (int br = 0; br < 2; ++br) {
        const int P = br ? Tt : Tf;
        const Geo g{B, 1, P, 0};
        mi_conv_desc d = base_desc(chan[2 + br], chan_ktab[2 + br], w_tr_x[br][cur[br]], (int64_t)512 * P, g);
        d.plain = 1; d.epi = MI_EPI_LINEAR; d.flags = MI_FLAG_RES; d.res = br ? w_skip_t[3] : w_skip[3];
        d.y = br ? dtin : din; d.y_bstride = (int64_t)384 * P; d.y_cstride = P;
        if (tapimg) { d.flags |= MI_FLAG_IMG; d.yh = br ? dtin : din; d.yh_n = (int64_t)B * P; }
        MI_TRY(conv(d, br ? stt : st));
    }
    // ---- decoders ----------------------------------------------------------------------------------
    for (int j = 0; j < 4; ++j) {
        const int C = kCh[3 - j], Fr = kFr[4 - j];
        const bool last = j == 3;
        {   // frequency branch: rewrite 3x3 + GLU -> DConv -> ConvTranspose (+GELU, + next skip)
            const Geo g{B, Fr, T, 1};
            const int64_t P = (int64_t)Fr * T;
            mi_conv_desc r = base_desc(dec[j].rewrite, dec[j].ktab_rw, din, C * P, g);
            r.epi = MI_EPI_GLU; r.y = w_a; r.y_bstride = C * P; r.y_cstride = P;
            r.ntaps = 9; r.tap_k2 = 3; r.tap_pad1 = 1; r.tap_pad2 = 1;       // the conv's geometry: the DMA routes need no table
            if (tapimg) { r.xh = din; r.xh_n = (int64_t)B * P; r.wtap = dec[j].rewrite.wtap; }
            MI_TRY(conv(r, st));
            MI_TRY(run_dconv(dec[j].dconv, C, g, w_a, w_b, w_h, w_stats, w_st1, w_st2, st));
            const int Cout = last ? 4 * S : kCh[2 - j];
            mi_conv_desc t = base_desc(dec[j].convtr, dec[j].ktab_tr, w_a, C * P, g);
            t.O1 = Fr + 1; t.epi = MI_EPI_CONVTR; t.flags = MI_FLAG_TR_FREQ; t.out_len = 4 * Fr;
            t.y_cstride = (int64_t)4 * Fr * T; t.y_bstride = Cout * t.y_cstride;
            t.dma_rows = 1;                  // rows q and q - 1
            if (last) t.y = w_yspec;
            else { t.flags |= MI_FLAG_GELU | MI_FLAG_RES; t.res = w_skip[2 - j]; t.y = din; }
            if (!last && tapimg) { t.flags |= MI_FLAG_IMG; t.yh = din; t.yh_n = (int64_t)B * t.y_cstride; }
            if (tapimg && dec[j].convtr.wtap && !last) {    // the outermost layer (K = 96) is bound by its output either way
                // the DConv branch's float32 output as the transposed conv's operand image (w_b is free again), then the two taps
                // (input rows q and q - 1) by LDS-DMA
                MI_TRY(launch_f32_to_image(w_a, B, C, P, cfg.dtype, w_b, st));
                t.xh = w_b; t.xh_n = (int64_t)B * P; t.wtap = dec[j].convtr.wtap; t.ntaps = 2; t.tap_k2 = 1; t.tap_dil1 = -1;
            }
            // din is free to overwrite: the rewrite conv that read it has completed (same stream)
            MI_TRY(conv(t, st));
            MI_STAGE("dec freq layer done");
        }
        {   // time branch
            const int Lv = Lt[4 - j], L = Lp[4 - j], Lout = Lt[3 - j], Lpo = Lp[3 - j];   // valid lengths and row pitches
            const Geo g{B, 1, Lv, 0, L};
            mi_conv_desc r = base_desc(tdec[j].rewrite, tdec[j].ktab_rw, dtin, (int64_t)C * L, g);
            r.epi = MI_EPI_GLU; r.y = w_ta; r.y_bstride = (int64_t)C * L; r.y_cstride = L;
            r.ntaps = 3; r.tap_k2 = 3; r.tap_pad1 = 0; r.tap_pad2 = 1;
            if (tapimg) { r.xh = dtin; r.xh_n = (int64_t)B * L; r.wtap = tdec[j].rewrite.wtap; }
            MI_TRY(conv(r, stt));
            MI_TRY(run_dconv(tdec[j].dconv, C, g, w_ta, w_tb, w_th, w_stats_t, w_st1_t, w_st2_t, stt, w_gram2_t, gram2t_bytes));
            const int Cout = last ? 2 * S : kCh[2 - j];
            mi_conv_desc t = base_desc(tdec[j].convtr, tdec[j].ktab_tr, w_ta, (int64_t)C * L, g);
            t.O2 = Lv + 1; t.o2_valid = 0; t.epi = MI_EPI_CONVTR; t.out_len = Lout;     // q = 0 .. Lv, scattered to 4q + r - 2
            t.y_cstride = Lpo; t.y_bstride = (int64_t)Cout * Lpo;
            if (last) t.y = w_ytime;
            else { t.flags |= MI_FLAG_GELU | MI_FLAG_RES; t.res = w_skip_t[2 - j]; t.y = dtin; }
            if (!last && tapimg) { t.flags |= MI_FLAG_IMG; t.yh = dtin; t.yh_n = (int64_t)B * t.y_cstride; }
            if (tapimg && tdec[j].convtr.wtap && !last) {
                MI_TRY(launch_f32_to_image(w_ta, B, C, L, cfg.dtype, w_tb, stt));
                t.xh = w_tb; t.xh_n = (int64_t)B * L; t.wtap = tdec[j].convtr.wtap; t.ntaps = 2; t.tap_k2 = 2; t.tap_dil2 = -1;
            }
            MI_TRY(conv(t, stt));
        }
    }
    MI_TRY(join());                         // the waveform decoder's output is complete on the caller's stream
    MI_STAGE("decoders done");
    return MI_OK;
}

}  // namespace mi
