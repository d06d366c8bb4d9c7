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

#include "model.h"

namespace mi {

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
        // level 0 (K = 16) is bound by its output: native
        MI_TRY(pack_conv(w, b, C, Cint * 8, false, &te.conv, 0, i > 0 ? SPLIT_TIME : SPLIT_OPT_IN));
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
        // the outermost one (K = 96, 32-row tile) is bound by its output: native
        MI_TRY(pack_convtr(w, b, C, Coutt, &td.convtr, 4, j < 3 ? SPLIT_TIME : SPLIT_OPT_IN));
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
    dconv_gram = w_gram; dconv_gram2 = w_gram2; dconv_gram2_bytes = gram2_bytes;     // EngineCore::run_dconv's scratch
    dconv_tap_dma = true;        // fill_workspace gave w_a / w_b / w_ta / w_tb the slack the shifted DMA runs need
    return MI_OK;
}

int Model::fill_workspace(Workspace &w) {
    const size_t B = cfg.max_batch;
    auto A = [&](float **p, size_t per_item) { return w.mem.alloc((void **)p, per_item * B * sizeof(float)); };
    auto dev_alloc = [&](void **p, size_t n) { return w.mem.alloc(p, n); };
    MI_TRY(A(&w.w_xt0, (size_t)2 * SL));
    MI_TRY(A(&w.w_zt, (size_t)4 * 2048 * T));
    MI_TRY(A(&w.w_x0, (size_t)4 * 2048 * T));
    size_t big = 0;
    for (int i = 0; i < 4; ++i) {
        const size_t nf = (size_t)kCh[i] * kFr[i + 1] * T, nt = (size_t)kCh[i] * Lp[i + 1];
        MI_TRY(A(&w.w_skip[i], nf));
        // the time encoder's strided convs read their input by LDS-DMA from sample -2 to past the row's end (gemm_loop.h
        // TimeEncTaps: up to 8 bytes before and 20 after the tensor): 128 bytes of slack on both sides
        // (only the float32 route reads it; the half modes get the same layout, which keeps one allocation rule and 16-byte alignment)
        MI_TRY(w.mem.alloc((void **)&w.w_skip_t[i], (nt * B + 64) * sizeof(float)));
        w.w_skip_t[i] += 32;
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
        MI_TRY(w.mem.alloc((void **)p, (big * B + 64) * sizeof(float)));
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
            // a split image: each column's 8-sample run by LDS-DMA (gemm_loop.h TimeEncTaps); w_skip_t carries the read slack
            if (d.wx && !d.half) d.dma_time = 1;
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
            if (t.wx && !t.half) {
                // a split image: the two taps by LDS-DMA (gemm_loop.h TimeTrTaps).  The columns lie on a pitch that is a multiple of
                // 4, so no 16-byte chunk straddles two items; the padded columns are computed and never stored.  w_ta carries the
                // read slack (fill_workspace)
                t.O2 = round_up(Lv + 1, 4); t.o2_valid = Lv + 1; t.dma_time = 1;
            }
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
