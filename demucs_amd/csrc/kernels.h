// Internal launcher declarations shared by the engine's translation units.
#pragma once
#include <cmath>
#include <vector>
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gemm_conv.h"

namespace mi {

struct FftTables {
    const float *window;    // [4096] periodic Hann, float32 like th.hann_window
    const float2 *twiddle;  // [2048] exp(-2 pi i n / 4096)
    const float *envelope;  // [1024] sum_j window^2[r + 1024 j]
};
// The three tables on the host, one builder for both engines and the handle-free entry points (each uploads with its own
// allocator): the window and its overlap envelope in float32 arithmetic like th.hann_window (spec.py:19,41), the envelope summed in
// ascending frame order; W^n = exp(-2 pi i n / 4096) for n < 2048 (W^(n + 2048) = -W^n) as the float32 of the float64 value
struct FftHostTables {
    std::vector<float> window, envelope;
    std::vector<float2> twiddle;
};
static inline FftHostTables fft_host_tables() {
    FftHostTables t{std::vector<float>(4096), std::vector<float>(1024), std::vector<float2>(2048)};
    for (int i = 0; i < 4096; ++i) t.window[i] = 0.5f - 0.5f * cosf((float)i * (float)(2.0 * M_PI / 4096.0));
    for (int r = 0; r < 1024; ++r) {
        float e = 0.f;
        for (int j = 3; j >= 0; --j) e += t.window[r + 1024 * j] * t.window[r + 1024 * j];
        t.envelope[r] = e;
    }
    for (int i = 0; i < 2048; ++i) { const double a = -2.0 * M_PI * i / 4096.0; t.twiddle[i] = make_float2((float)cos(a), (float)sin(a)); }
    return t;
}

// fft.hip
int launch_stft_frames(const float *mix, int B, int L, const FftTables &tb, float *zt, double *stats, hipStream_t st);
int launch_cac_transpose(const float *zt, int B, int T, const float2 *norm, float *x, hipStream_t st, int x_pitch = 0 /* 0 = T */);
int launch_istft(const float *y, int B, int S, int L, const float2 *denorm, const float *xt, const float2 *denorm_t,
                 const FftTables &tb, float *yt, float *fr, float *out, hipStream_t st, int xt_pitch = 0 /* row pitch of xt, 0 = L */,
                 int y_pitch = 0 /* row pitch of y along T, 0 = T */);

extern int g_transpose_tiles;  // fft.hip: round-3 kernels around the transforms; bit 0: one STFT frame per workgroup, bit 1: tile cac_transpose, bit 2: tile spec_transpose
extern int g_istft_fused;      // fft.hip: 1 = fused inverse-transform + overlap-add kernel (default), 0 = the two separate kernels

// norms.hip
int launch_row_stats(const float *x, int rows, int64_t count, int64_t row_stride, double *stats, hipStream_t st);
int launch_finalize_stats(double *stats, int rows, double count, float eps, int mode, float2 *out_a, float2 *out_b,
                          hipStream_t st);
int launch_row_affine(const float *x, int rows, int64_t count, const float2 *norm, float *y, hipStream_t st);
int launch_row_denorm(const float *x, int rows, int64_t count, const float2 *denorm, float *y, hipStream_t st);
// img (optional, half modes): the tensor the next matrix product reads, as its 16-bit operand image [C / 8][img_n][8]
int launch_layernorm_cf(const float *x, int B, int C, int T, const float *w, const float *b, const float *pe, float *y,
                        float2 *ostat, hipStream_t st, void *img = nullptr, int64_t img_n = 0, int img_dtype = 0);
int launch_token_stats(const float *x, int B, int C, int T, float2 *ostat, hipStream_t st, void *img = nullptr, int64_t img_n = 0,
                       int img_dtype = 0);
int launch_gn_apply_tokstats(const float *x, int B, int C, int T, const float2 *gstat, const float *w, const float *b, float *y,
                             float2 *ostat, hipStream_t st, void *img = nullptr, int64_t img_n = 0, int img_dtype = 0);

// GroupNorm(1) + GELU in place plus the Gram accumulators that give the NEXT GroupNorm's statistics (norms.hip)
int gram_hp(int h);          // accumulator matrix order for h hidden channels: h + 1 rounded up to 32
int launch_gn_gelu_gram(float *x, int B, int h, int Cs, int D1, int D2 /* valid */, int pitch, int row_mode, const float2 *stats, const float *w,
                        const float *b, double *gram /* rows x slots x HP x HP, zero */, int slots, bool zero_pad, hipStream_t st);
int launch_gram_finalize(double *gram, int rows, int h, int slots, const double *wt /* HP x HP */, const double *ct /* HP */, double sum_b,
                         double sum_bsq, double cols, double count, float eps, float2 *out, hipStream_t st);
int launch_gn_gelu(float *x, int B, int C, int Cs, int D1, int D2, int row_mode, const float2 *stats, const float *w, const float *b,
                   hipStream_t st);

// dconv_row.hip: both DConv layers of one frequency-branch row fused in LDS
struct DConvRowLayer {
    const float *w0;    // [C][3][HA]   conv3 weights, hidden index fastest (HA = C/8 rounded up to 4)
    const float *b0;    // [HA]
    const float *g1w, *g1b;   // [HA]  GroupNorm(1, C/8) affine
    const float *w3;    // [2C][HA]    1x1 weights, natural row order (value rows then gate rows)
    const float *b3, *g2w, *g2b;   // [2C]
    const float *ls;    // [C]         LayerScale
};
// a DConv layer's weights plus the constants that give the second GroupNorm's statistics from the Gram matrix of the
// hidden activations (dconv_time.hip, dconv_row.hip)
struct DConvTimeLayer {
    DConvRowLayer w;             // same packing as dconv_row.hip
    const double *gram_a;        // [H (H + 1) / 2]  (W3^T W3)_ii, then 2 (W3^T W3)_ik for k > i, row-major upper triangle
    const double *gram_v;        // [H]              2 W3^T b3
    const double *gram_c;        // [H]              column sums of W3
    const double *gram_e1, *gram_e2;   // [H (H + 1) / 2 + H] the same constants in the ENTRY order of dconv_row.hip's reduction
                                 //   (i, k = i .. H): weight of the entry in sum z^2 / in sum z
    double sum_b3, sum_b3sq;
};
struct DConvRowArgs {
    DConvTimeLayer l[2];
    const float *x;     // [B][C][Fr][T]
    float *y;           // same shape (may alias x)
    int Fr, T;
};
// The host-side packing of one DConv layer (C channels, h = C / 8 hidden) from the checkpoint's natural-layout tensors -- the one
// builder for Model::load_dconv and the handle-free test entries (each uploads with its own allocator): w0 (h, C, 3) -> [C][3][HA],
// b0 / g1w / g1b -> [HA], w3 (2C, h) -> [2C][HA] (HA = h rounded up to 4, padding zero) and the float64 Gram constants of DConvTimeLayer
struct DConvHostPack {
    std::vector<float> w0, b0, g1w, g1b, w3;
    std::vector<double> gram_a, gram_v, gram_c, gram_e1, gram_e2;
    double sum_b3, sum_b3sq;
};
DConvHostPack dconv_pack_host(int C, int h, const float *w0, const float *b0, const float *g1w, const float *g1b, const float *w3,
                              const float *b3);
bool dconv_row_supported(int C, int T);
bool dconv_row_lds_supported(int C, int T);     // what the LDS-resident kernel takes (C = 48)
// lds_row: the LDS-resident kernel where dconv_row_lds_supported(C, T) (Model passes switches().dconv_row_lds), else the per-wave one
int launch_dconv_row(const DConvRowArgs &a, int C, int rows, bool lds_row, hipStream_t st);

// dconv_time.hip: fused DConv layer of the time branch (C = 48 / 96), three streaming passes
bool dconv_time_supported(int C, int Lp);
int launch_dconv_time_layer(const DConvTimeLayer &l, int C, int dil, int B, int Lv, int Lp, const float *x, float *y, float *hbuf,
                            double *stats, double *gram, float2 *st1, float2 *st2, hipStream_t st);

// gemm_conv.hip: fill the sink, validate (conv_validate), decide (conv_route), launch
int launch_conv(const mi_conv_desc &d, hipStream_t st);

// conv_route.hip: which kernel a conv / linear layer runs -- host code only, no kernel and no HIP call
constexpr int BK = 16;       // K step of the float32 main loops
constexpr int BN = 128;      // columns of a block tile
int conv_pick_tile(int M);
int conv_check_tile_m(const mi_conv_desc &d);     // MI_OK, or MI_EINVAL with the error set: tile_m = 192 on a layer that cannot take it
int conv_validate(const mi_conv_desc &d);         // MI_OK, or MI_EINVAL with the error set: a descriptor no kernel takes (d.sink is not looked at)
// true: launch_conv runs a statistics layer item by item (a per-item row of fewer than 32 columns, more than two items: the epilogue's
// wave reduction tells at most two rows apart in a wave's 32 columns)
bool conv_stats_per_item(const mi_conv_desc &d);
extern int g_split_bf16;     // 0 (mi_set_split_bf16): native fp32 MFMA kernels even where a split weight image exists
// Which kernel launch_conv runs for a descriptor, decided from the descriptor alone (no HIP call, no pointer followed):
// route: mi_conv_route (include/demucs_amd.h); tile: the rows of the tile that kernel runs, after every substitution
// (routes 4, 7, 8, 11: 64 under a 128-row layer = the 64-row tile that reads the 128-row image; 192 or 96 under a tile_m = 192
// layer = the 192-row tile on pairs of its 96-row images, or the 96-row tile on them; routes 5, 9, 10: 256 = the half modes'
// 256-row tiles); plain: the 1x1 / linear fast path; mgroups: MI_MGROUPS, the M-grouped tile order of routes 0 and 1
struct ConvRoute { int route; int tile; bool plain; bool mgroups; };
ConvRoute conv_route(const mi_conv_desc &d);
// Every environment switch of the engine (INTEGRATION.md has the table), parsed once, when the library is loaded (switches.hip:
// the only file that looks at the environment).  The values are the parsed meanings, not the strings.
struct Switches {
    // ---- the conv kernels (conv_route) ----
    bool no_dma;            // MI_NO_DMA: plain linear layers on the register-staged loader
    bool no_dma_tap;        // MI_NO_DMA_TAP: no shifted-run DMA taps (routes 2 and 7)
    bool no_dma_rows;       // MI_NO_DMA_ROWS: no DMA row taps (routes 3 and 8)
    bool no_dma_dconv;      // MI_NO_DMA_DCONV: the DConv blocks' k = 3 convs off route 2
    bool small_tile;        // MI_SMALL_TILE (default 1): smaller tiles for under-filled 128-row layers
    bool mgroups;           // MI_MGROUPS: M-grouped tile order in the native fp32 kernels
    bool x6_plain_only;     // MI_X6_MODE=1: the split-bf16 loop for plain layers only
    bool img256;            // MI_IMG256 (a non-zero number): the 256 x 256 tile (route 10) for the half modes' residual epilogues on image inputs
    bool half_tile256;      // MI_HALF_TILE256 (default 1): the half modes' 256-row tile for plain linear layers (route 5)
    // ---- packing and schedule of both engines ----
    int x6_scope;           // MI_X6: which layers get a split-bf16 weight image: unset 1 = the default scope (Model::pack_split), 0 = none, anything else 2 = every layer
    bool no_tap_image;      // MI_NO_TAP_IMAGE: half modes, no tap-ordered weight images: the k x k convs walk gather tables over float32 tensors
    bool no_enc_image;      // MI_NO_ENC_IMAGE: half modes, no phase-split images in front of the strided encoder convs
    bool no_dconv_time;     // MI_NO_DCONV_TIME: the time branch's DConv blocks on the implicit-GEMM route, not dconv_time.hip
    bool no_lin2_stats;     // MI_NO_LIN2_STATS: norm_out's statistics by a separate pass, not by lin2's epilogue
    bool no_ffn_image;      // MI_NO_FFN_IMAGE: half modes, attention output and FFN hidden tensor as float32, not as operand images
    bool no_qkv_heads;      // MI_NO_QKV_HEADS: half modes, Q / K / V as float32 tensors, not as per-head 16-bit ones
    bool no_input_image;    // MI_NO_INPUT_IMAGE: half modes, the projections read their float32 inputs, not operand images of them
    bool one_stream;        // MI_ONE_STREAM: HTDemucs, both branches on the caller's stream
    bool debug_sync;        // MI_DEBUG_SYNC: HTDemucs synchronises after every stage and names it on stderr (one stream)
    int side_prio;          // MI_SIDE_PRIO: the side stream's priority: unset 0 = normal, first letter l -1 = the device's least, else 1 = its greatest
    bool h_no_deep_tap;     // MI_H_NO_DEEP_TAP: HDemucs half modes, the k = 3 convs of layers 4 / 5 and decoders 0 / 1 on table-driven gathers
    bool h_no_last_tap;     // MI_H_NO_LAST_TAP: HDemucs half modes, the outermost transposed conv on the table-driven gather over float32
    bool h_one_stream;      // MI_H_ONE_STREAM: HDemucs, both branches on the caller's stream
    bool lstm_steps;        // MI_LSTM_STEPS (a non-zero number): one launch per LSTM time step, not the persistent kernel
    // ---- single kernels ----
    bool lstm_write_through;    // MI_LSTM_WRITE_THROUGH: the persistent LSTM kernel never uses the same-XCD plain-store path
    bool lstm_debug;        // MI_LSTM_DEBUG: mi_lstm_seq prints the persistent kernel's cycle counters
    int transpose_tiles;    // MI_TRANSPOSE_TILES: initial g_transpose_tiles mask (bit 0 STFT frames, 1 cac_transpose, 2 spec_transpose): unset 0, a number above 1 its low three bits, anything else 7
    bool istft_split;       // MI_ISTFT_SPLIT: g_istft_fused starts at 0 (inverse transform and overlap-add as two kernels)
    bool dconv_row_lds;     // MI_DCONV_ROW (first letter l): the LDS-resident DConv row kernel for C = 48
};
const Switches &switches();
// gemm_x6.hip: `tile` as decided by conv_route, `image_tile` the tile the split image was packed for
constexpr bool conv_x6_supported(int tile) { return tile == 128 || tile == 96 || tile == 64; }
// Which (epilogue, LINEAR flag set, loader) combinations the 192-row tile is compiled for: the layers of the float32 engine with
// M % 192 == 0 -- the tap convs (GLU), the row-tap layers (LINEAR + GELU, CONVTR, 1 x 1 + GLU) and the self-attention in_proj
// (plain LINEAR with MI_FLAG_LN).  Anything else with such an M runs the 96-row tile on the same image.  lflags: the GELU / SCALE /
// RES / LN / STATS bits (0 for other epilogues); ntaps: the loader -- 9 or 3 shifted-run taps, kRowTaps row taps, 0 plain or
// gather table, kTimeTr the time-axis transposed conv's two shifted runs (CONVTR), kTimeEnc the time-axis strided conv's 8-sample runs
// (LINEAR + GELU).  conv_route asks with the descriptor's epilogue
// and flags, launch_tile_x6 with its template arguments
constexpr int kRowTaps = -1;
constexpr int kTimeTr = -2;
constexpr int kTimeEnc = -3;
constexpr bool conv_x6_tile192(int epi, int lflags, bool plain, int ntaps) {
    if (ntaps > 0) return epi == MI_EPI_GLU;
    if (ntaps == kTimeTr) return epi == MI_EPI_CONVTR;
    if (ntaps == kTimeEnc) return epi == MI_EPI_LINEAR && lflags == MI_FLAG_GELU;
    if (ntaps == kRowTaps) return (epi == MI_EPI_LINEAR && lflags == MI_FLAG_GELU) || epi == MI_EPI_CONVTR || epi == MI_EPI_GLU;
    return plain && epi == MI_EPI_LINEAR && lflags == MI_FLAG_LN;
}
int launch_conv_x6(const mi_conv_desc &d, int tile, int image_tile, bool plain, hipStream_t st);
int launch_conv_tap_x6(const mi_conv_desc &d, int tile, int image_tile, hipStream_t st);      // stride-1 3 x 3 / k = 3 GLU convs (route 7)
int launch_conv_rows_x6(const mi_conv_desc &d, int tile, int image_tile, hipStream_t st);     // row-tap encoder / transposed convs (route 8)
int launch_conv_time_x6(const mi_conv_desc &d, int tile, int image_tile, hipStream_t st);     // time-axis transposed / strided convs (route 11)
int launch_pack_split(const float *wt, int Kpad, int Mpad, int tile_m, void *wx, hipStream_t st);

// gemm_half.hip: bf16 / fp16 operand main loops (mi_config.dtype); `r` as decided by conv_route (routes 5, 9, 10)
int launch_conv_half(const mi_conv_desc &d, const ConvRoute &r, hipStream_t st);
int launch_pack_half(const float *wt, int Kpad, int Mpad, int dtype, void *wh, hipStream_t st);
// gemm_tap.hip: k x k stride-1 convs on operand-image inputs (tap-minor K order), half modes
int conv_tap_pairs_pad(int Cin, int ntaps);
int launch_pack_tap(const float *wt, int Mpad, int Cin, int ntaps, int dtype, void *out, hipStream_t st);
int launch_conv_tap(const mi_conv_desc &d, int tile, hipStream_t st);
int launch_f32_to_image(const float *x, int B, int C, int64_t P, int dtype, void *img, hipStream_t st);

// hkernels.hip: the Hybrid Demucs v3 (hdemucs_mmi) path's own kernels
int launch_row_affine_pitch(const float *x, int B, int C, int L, int out_pitch, const float2 *norm, float *y, hipStream_t st);
int launch_gn_apply(const float *x, int B, int Cin, int G, int in_pitch, int off, const float2 *stats, const float *w, const float *bias,
                    int glu, int gelu, const float *scale, const float *res, int res_pitch, float *y, int Cout, int out_len,
                    int out_pitch, hipStream_t st, int chan_div = 1);
int launch_unfold_frames(const float *x, int B, int C, int T, int F, int W, int S, float *fr, hipStream_t st);
int launch_restitch_frames(const float *fr, int B, int C, int T, int F, int W, int S, const float *skip, float *y, hipStream_t st);
void pack_lstm_whh(const float *whh /* (2, 4H, H) */, int H, float *packed);     // host side: the step kernel's operand order
int launch_lstm_seq(const float *gx, const float *whh /* packed */, int N, int H, int W, float *out, float *state /* 6 N H floats */, hipStream_t st);
// lstm.hip: the same recurrence as ONE persistent launch per batch of sequence tiles (hidden state exchanged between workgroups
// as tagged 8-byte granules); scratch: lstm_persist_scratch_bytes() device bytes; ctl_host: pinned host word set on a time-out
size_t lstm_persist_scratch_bytes();
size_t lstm_persist_ctl_offset();      // byte offset of the control / debug words inside the scratch block
int launch_lstm_persist(const float *gx, const float *whh /* packed */, int N, int H, int W, float *out, void *scratch, unsigned *ctl_host,
                        hipStream_t st);
int launch_lstm_small(const float *gx, const float *whh_natural /* (2, 4H, H) */, int N, int H, int W, float *out, hipStream_t st);   // H <= 64
int launch_local_attn(const float *qkc, int B, int C, int T, int ld /* row pitch of qkc, % 4 == 0 */, float *out, int ld_o, hipStream_t st);

// attention.hip
// oh != NULL (half modes): the output goes to a 16-bit operand image [512 / 8][oh_n][8] (column b * Tq + query) instead of o
int launch_attention(const float *q, const float *k, const float *v, float *o, int B, int heads, int Tq, int Tk, int64_t q_bs,
                     int64_t kv_bs, int64_t o_bs, int dtype, hipStream_t st, void *oh = nullptr, int64_t oh_n = 0);
// attention_x6.hip: the float32 attention core on the split-bf16 matrix pipe (same arguments and layout, float32 only)
int launch_attention_x6(const float *q, const float *k, const float *v, float *o, int B, int heads, int Tq, int Tk, int64_t q_bs,
                        int64_t kv_bs, int64_t o_bs, hipStream_t st);

// ola.hip
int launch_segments_gather(const float *track, int64_t track_len, int channels, const int64_t *starts_dev, int B, int valid,
                           float *seg, hipStream_t st);
int launch_ola_accumulate(float *acc, int64_t acc_len, int rows, const float *model_out, int valid, const int64_t *offs_dev,
                          const int32_t *lens_dev, const int32_t *trim_dev, int B, int64_t span_lo, int64_t span_hi,
                          const float *weight, int weight_len, hipStream_t st);
int launch_ola_finish(float *acc, int64_t acc_len, int rows, int64_t acc_off0, const int64_t *offs_dev, const int32_t *lens_dev,
                      int n_segments, int max_len, const float *weight, hipStream_t st);

int launch_segments_gather_packed(const float *tracks, int64_t tracks_cap, int channels, const int64_t *items_dev, int B, int valid,
                                  float *seg, hipStream_t st);
int launch_ola_accumulate_packed(float *acc, int64_t acc_cap, int rows, const float *model_out, int valid, const int64_t *items_dev,
                                 int B, const int64_t *tiles_dev, int n_tiles, const float *weights, int64_t weights_cap,
                                 hipStream_t st);
int launch_ola_finish_packed(float *acc, int64_t acc_cap, int rows, const int64_t *tiles_dev, int n_tiles, const int64_t *segs_dev,
                             int n_segs, const float *weights, int64_t weights_cap, hipStream_t st);

// resample.hip
int launch_resample_frac(const float *x, int rows, int64_t L, const float *table, int old_sr, int new_sr, int width, float *y,
                         int64_t Lout, hipStream_t st);

// convert_stream.hip: the streaming convert_audio fused with the append (mi_streams_convert_append)
int launch_streams_convert_append(float *win, int64_t win_cap, int channels, const int64_t *table, int n_streams, int64_t max_groups,
                                  const float *bank, int64_t bank_cap, float *hist, int64_t hist_cap, const float *stats, int n_stats,
                                  int lds_floats, hipStream_t st);
int launch_streams_convert_append_pcm(float *win, int64_t win_cap, int channels, const int64_t *table, int n_streams,
                                      int64_t max_groups, const float *bank, int64_t bank_cap, float *hist, int64_t hist_cap,
                                      const float *stats, int n_stats, int lds_floats, hipStream_t st);

// ingest.hip: wire PCM (interleaved int16 / int24 / float32 frames) to planar float32, alone and as the streams' append
int launch_pcm_planar(const unsigned char *src, int fmt, int src_ch, int64_t n, int channels, const float *stats, float *dst,
                      hipStream_t st);
int launch_streams_append_pcm(float *win, int64_t win_cap, int channels, const int64_t *table, int n_streams, int64_t max_bytes,
                              const float *stats, int n_stats, hipStream_t st);

// stats_stream.hip: mi_mono_stats block by block, the per-thread sums carried in device memory
int mono_stats_state_bytes();
int launch_mono_stats_update(const unsigned char *src, int fmt, int src_ch, int64_t n, int channels, int64_t before, double *state,
                             hipStream_t st);
int launch_mono_stats_finish(const double *state, int64_t length, double *scratch, float *stats, hipStream_t st);

// score.hip: the nSDR sums of stems against reference stems, whole or block by block (sdr_sums.h)
int64_t sdr_state_bytes(int n_sources);
int64_t sdr_scratch_bytes(int n_sources);
int launch_sdr_update(const void *const *refs, int fmt, int src_ch, int64_t ref_stride, const float *est, int64_t est_stride, int n_sources,
                      int channels, int64_t n, int64_t before, double *state, hipStream_t st);
int launch_sdr_finish(const double *state, int n_sources, double *scratch, double *sums, hipStream_t st);
int launch_sdr(const float *ref, const float *est, int B, int n_sources, int channels, int64_t length, double *state, double *scratch,
               double *sums, hipStream_t st);

const void *conv_zero_page();      // gemm_conv.hip: 256 bytes of device zeros
// attention_heads.hip: half modes, per-head token-major 16-bit operands (MI_FLAG_HEADS), LDS-DMA ring
int launch_attention_heads(const void *q, const void *k, const void *v, const void *zero_page, int B, int heads, int Tq, int Tk, int Tq_pitch,
                           int Tk_pitch, int dtype, void *oh, int64_t oh_n, float *o, int64_t o_bs, hipStream_t st);

// post.hip: Separator normalisation, clip prevention, two-stems sums
int post_stats_scratch_bytes();
int launch_mono_stats(const float *wav, int channels, int64_t length, double *scratch, float *stats, hipStream_t st);
int launch_mono_stats_final(const double *scratch, int64_t length, float *stats, hipStream_t st);
int launch_stream_emit(const float *acc, int64_t acc_cap, int n_sources, int channels, const int64_t *passes, int n_passes,
                       const int64_t *segs, int n_segs, const float *weights, int64_t weights_cap, const float *scales, int n_members,
                       int shifts, int bag, const float *stats, int64_t n, float *out, hipStream_t st);
int launch_streams_emit(const float *acc, int64_t acc_cap, int n_sources, int channels, const int64_t *streams, int n_streams, int64_t max_n,
                        const int64_t *passes, int n_passes, const int64_t *segs, int n_segs, const float *weights, int64_t weights_cap,
                        const float *scales, int n_members, int shifts, int bag, const float *stats, int n_stats, float *out,
                        int64_t out_cap, hipStream_t st);
int launch_streams_append(float *win, int64_t win_cap, int channels, const int64_t *table, int n_streams, int64_t max_n,
                          const float *stats, int n_stats, hipStream_t st);
int launch_streams_compact(float *dst, int64_t dst_cap, const float *src, int64_t src_cap, const int64_t *table, int n_rows, int64_t max_len,
                           hipStream_t st);
int launch_track_affine(float *x, int64_t n, const float *stats, int mode, hipStream_t st);
int launch_prevent_clip(const float *x, int64_t n, int mode, unsigned *peak, float *y, hipStream_t st);
int launch_two_stems(const float *const *stems, int S, int sel, const float *origin, int mode, int64_t n, float *y, hipStream_t st);

// deliver.hip: two-stems value, clip prevention, PCM conversion and interleaving of every output of a call in one launch
int launch_deliver_peaks(const int64_t *table, int n_rows, int64_t max_n, int n_sources, int channels, unsigned *peaks, int n_peaks,
                         int64_t dst_cap, hipStream_t st);
int launch_deliver_pcm(const int64_t *table, int n_rows, int64_t max_n, int n_sources, int channels, const unsigned *peaks, int n_peaks,
                       unsigned char *dst, int64_t dst_cap, hipStream_t st);

// deliver_mix.hip: gain-weighted remixes of the stems and the mix, clipped, converted and interleaved, every remix of a call in one launch
int launch_deliver_mix_pcm(const int64_t *table, int n_rows, int64_t max_n, int n_sources, int channels, const unsigned *peaks,
                           int n_peaks, unsigned char *dst, int64_t dst_cap, hipStream_t st);
int launch_deliver_mix_peaks(const int64_t *table, int n_rows, int64_t max_n, int n_sources, int channels, unsigned *peaks, int n_peaks,
                             int64_t dst_cap, hipStream_t st);
int launch_deliver_mix_peaks_update(const int64_t *table, int n_rows, int64_t max_n, int n_sources, int channels, unsigned *peaks,
                                    int n_peaks, hipStream_t st);

// deliver_mix_auto.hip: the same for remixes whose gains change along the track (steps and linear ramps at track positions)
int launch_deliver_mix_auto_pcm(const int64_t *table, int64_t table_len, int n_rows, int64_t max_n, int n_sources, int channels,
                                const unsigned *peaks, int n_peaks, unsigned char *dst, int64_t dst_cap, hipStream_t st);
int launch_deliver_mix_auto_peaks(const int64_t *table, int64_t table_len, int n_rows, int64_t max_n, int n_sources, int channels,
                                  unsigned *peaks, int n_peaks, int64_t dst_cap, hipStream_t st);

// deliver_resample.hip: a stream's outputs at another sample rate -- value, streaming resample_frac, clip, PCM -- in one launch
int launch_deliver_resample_pcm(const int64_t *table, int n_rows, int64_t max_groups, int n_sources, int channels, const float *bank,
                                int64_t bank_cap, float *hist, int64_t hist_cap, int lds_floats, unsigned char *dst, int64_t dst_cap,
                                hipStream_t st);

// "rescale" on a stream: the running per-output peaks of a measuring pass (deliver.hip at the model's rate, deliver_resample.hip
// at another), and the resampling delivery that divides by peaks measured before
int launch_deliver_peaks_update(const int64_t *table, int n_rows, int64_t max_n, int n_sources, int channels, unsigned *peaks,
                                int n_peaks, hipStream_t st);
int launch_deliver_resample_peaks(const int64_t *table, int n_rows, int64_t max_groups, int n_sources, int channels, const float *bank,
                                  int64_t bank_cap, float *hist, int64_t hist_cap, int lds_floats, const int32_t *slots, unsigned *peaks,
                                  int n_peaks, hipStream_t st);
int launch_deliver_resample_pcm_peaks(const int64_t *table, int n_rows, int64_t max_groups, int n_sources, int channels,
                                      const float *bank, int64_t bank_cap, float *hist, int64_t hist_cap, int lds_floats, unsigned char *dst,
                                      int64_t dst_cap, const int32_t *slots, const unsigned *peaks, int n_peaks, hipStream_t st);

// loudness.hip: K-weighted sub-block energies of gain-weighted remixes (ITU-R BS.1770-4), whole or streamed; coef is a HOST array
int launch_loudness_update(const int64_t *table, int n_rows, int64_t max_n, int64_t max_blocks, int n_sources, int channels,
                           const double *coef, int64_t hop, int64_t warm, float *hist, int64_t hist_cap, double *energies, int64_t e_cap,
                           float *work, int64_t work_cap, hipStream_t st);

// true_peak.hip: oversampled (BS.1770-4 Annex 2) and sample peaks of gain-weighted remixes, whole or streamed; bank is (phases, taps)
int launch_true_peak_update(const int64_t *table, int n_rows, int64_t max_n, int n_sources, int channels, const float *bank, int phases,
                            int taps, float *hist, int64_t hist_cap, unsigned *peaks, int n_peaks, hipStream_t st);

}  // namespace mi
