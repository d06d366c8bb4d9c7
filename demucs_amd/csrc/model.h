// HTDemucs engine state: packed weights, gather tables, workspace.  One Model per (weights, device).
#pragma once
#include <memory>
#include <string>

#include "engine_core.h"

namespace mi {

struct EncW {
    PackedConv conv, rewrite;
    mi_ktab_entry *ktab_conv = nullptr, *ktab_rw = nullptr;
    DConvW dconv;
};
struct DecW {
    PackedConv rewrite, convtr;
    mi_ktab_entry *ktab_rw = nullptr, *ktab_tr = nullptr;
    DConvW dconv;
};
struct TrLayerW {
    PackedConv qkv_proj, q_proj, kv_proj, out_proj, lin1, lin2;
    // LayerNorm folded into the projection that consumes it: c1[m] = sum_k (W diag(ln_w))[m][k] (see MI_FLAG_LN)
    float *qkv_c1 = nullptr, *q_c1 = nullptr, *kv_c1 = nullptr, *lin1_c1 = nullptr;
    float *norm_w[4] = {}, *norm_b[4] = {};   // norm1, norm2, norm3 (cross only), norm_out
    float *gamma1 = nullptr, *gamma2 = nullptr;
};

// Activation workspace of one forward (sized for max_batch segments).  Handles created on the same device with the
// same geometry SHARE one workspace (a bag of four fine-tuned models holds the ~0.57 GB per batched segment once,
// not four times): such handles must not run concurrently -- they are used from one stream, one after the other,
// which is what the bag loop of apply_model does.
struct WorkspacePtrs {
    float *w_xt0 = nullptr, *w_zt = nullptr, *w_x0 = nullptr;
    float *w_skip[4] = {}, *w_skip_t[4] = {};
    void *w_eimg[2][3] = {};     // half modes: phase-split operand images of the encoder outputs 0..2 ([branch][level], gemm_conv.h MI_FLAG_IMG4)
    float *w_a = nullptr, *w_b = nullptr, *w_c = nullptr, *w_h = nullptr;
    float *w_ta = nullptr, *w_tb = nullptr, *w_tc = nullptr, *w_th = nullptr;
    float2 *w_tr_stat[2][2] = {}, *w_tr_stat1[2] = {};   // per-token (mean, rstd) of the layer inputs / of x1
    float *w_tr_x[2][2] = {}, *w_tr_qkv[2] = {}, *w_tr_att[2] = {}, *w_tr_x1[2] = {},
          *w_tr_x2[2] = {}, *w_tr_ffh[2] = {};
    // half modes: 16-bit operand images [512 / 8][B tokens][8] of the layer inputs (beside w_tr_x) and of x1: what the
    // in-projections and lin1 move global -> LDS by DMA
    float *w_tr_ximg[2][2] = {}, *w_tr_x1img[2] = {};
    float *w_yspec = nullptr, *w_ytime = nullptr, *w_yt = nullptr, *w_fr = nullptr;
    double *w_stats = nullptr, *w_stats_t = nullptr, *w_gram = nullptr, *w_gram2 = nullptr, *w_gram2_t = nullptr;
    size_t gram2t_bytes = 0;
    size_t gram2_bytes = 0;      // w_gram2: Gram accumulators of the implicit-GEMM DConv route (rows x slots x HP x HP float64)
    float2 *w_st1 = nullptr, *w_st2 = nullptr, *w_st1_t = nullptr, *w_st2_t = nullptr;
    float2 *w_norm_f = nullptr, *w_denorm_f = nullptr, *w_norm_t = nullptr, *w_denorm_t = nullptr;
};
struct Workspace : WorkspacePtrs {
    std::string key;
    DeviceArena mem;
    size_t stats_bytes = 0, gram_bytes = 0;
    // a forward that failed half-way may leave the self-cleaning statistics slots (norms.hip) non-zero: the next
    // forward re-zeroes them first instead of silently mis-normalising every later call
    bool dirty = false;
};

struct Model : EngineCore, WorkspacePtrs {
    Model() : EngineCore(ENGINE_HTDEMUCS) {}
    // What a forward of this handle writes as 16-bit images and which statistics route it takes: decided once, at the end of init,
    // from cfg.dtype, switches() and what was packed and allocated; the forward only reads it.  All false in the float32 mode
    // except lin2_stats.
    struct Plan {
        bool ffn_img = false;      // attention output and FFN hidden tensor exist only as the next product's operand image
        bool qkv_heads = false;    // Q / K / V exist only as per-head 16-bit tensors (attention_heads.hip)
        bool in_img = false;       // the layer inputs and x1 exist as operand images too: the in-projections and lin1 read those
        bool lin2_stats = false;   // norm_out's statistics come from lin2's epilogue
        bool tap_img = false;      // the decoder inputs exist only as their rewrite conv's operand image
        bool enc_img[2][4] = {};   // [branch][level i]: encoder conv i reads the phase-split image of level i - 1's output
    } plan;
    int attn(const float *q, const float *k, const float *v, float *o, int B, int Tq, int Tk, int64_t q_bs, int64_t kv_bs,
             int64_t o_bs, hipStream_t st, bool image = false);
    int attn_heads(const void *q, const void *k, const void *v, float *o, int B, int Tq, int Tk, hipStream_t st);
    int S = 0, SL = 0, T = 0, Lt[5] = {};   // time-branch lengths per level
    int Lp[5] = {};                         // ... and their row pitches (rounded up to 4 floats: 16-byte aligned rows)

    EncW enc[4], tenc[4];
    DecW dec[4], tdec[4];
    float *freq_emb = nullptr;
    PackedConv chan[4];
    mi_ktab_entry *chan_ktab[4] = {};
    mi_ktab_entry *tr_ktab512[2] = {}, *tr_ktab2048[2] = {};
    float *norm_in_w[2] = {}, *norm_in_b[2] = {}, *pos_emb[2] = {};
    TrLayerW tr[2][5];

    std::shared_ptr<Workspace> ws;   // activation workspace, shared by every handle with the same (device, geometry, max_batch)

    int init(const mi_config &c, const mi_tensor_desc *weights, size_t n);
    int forward(const float *mix, float *out, int B, hipStream_t st);
    int forward_core(const float *mix, const float *mag, float *spec_out, float *time_out, int B, hipStream_t st);
    int run_core(const float *mix, const float *mag, int B, hipStream_t st);
    int run_core_impl(const float *mix, const float *mag, int B, hipStream_t st);

   protected:
    int alloc_workspace();
    int fill_workspace(Workspace &w);
    int run_tr_layer(int br, int k, int B, const float *x, const float2 *xstat, const float *other, const float2 *ostat, float *out,
                     float2 *outstat, hipStream_t st, const void *ximg, const void *oimg, void *outimg);
};

}  // namespace mi
