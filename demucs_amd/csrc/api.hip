// extern "C" surface of libdemucs_amd.so (declared in include/demucs_amd.h).
#include <new>

#include "hmodel.h"
#include "model.h"

namespace mi {

post_launch_hook_t g_post_launch_hook = nullptr;
int g_last_conv_route = -1;
long long g_conv_route_launches[16][8] = {};
int g_last_conv_tile = -1;

char *last_error_buf() {
    static thread_local char buf[1024] = "";
    return buf;
}

int set_error(int code, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(last_error_buf(), 1024, fmt, ap);
    va_end(ap);
    return code;
}

// small cache of FFT tables for the handle-free kernel-level entry points
struct Tables {
    FftTables t{};
    bool ready = false;
};
static int get_tables(FftTables *out) {
    static Tables tb;
    if (!tb.ready) {
        const FftHostTables h = fft_host_tables();
        float *dw, *de; float2 *dt;
        MI_HIP(hipMalloc((void **)&dw, 4096 * 4)); MI_HIP(hipMalloc((void **)&dt, h.twiddle.size() * 8)); MI_HIP(hipMalloc((void **)&de, 1024 * 4));
        MI_HIP(hipMemcpy(dw, h.window.data(), 4096 * 4, hipMemcpyHostToDevice));
        MI_HIP(hipMemcpy(dt, h.twiddle.data(), h.twiddle.size() * 8, hipMemcpyHostToDevice));
        MI_HIP(hipMemcpy(de, h.envelope.data(), 1024 * 4, hipMemcpyHostToDevice));
        tb.t = FftTables{dw, dt, de};
        tb.ready = true;
    }
    *out = tb.t;
    return MI_OK;
}

// One DConv layer of a handle-free test entry on the device: the nine natural-layout tensors as the checkpoint stores them
// (layers.{d}.0.weight (h, C, 3), .0.bias (h), .1.weight / .1.bias (h), .3.weight (2C, h), .3.bias, .4.weight, .4.bias (2C),
// .6.scale (C); h = C / 8), packed by dconv_pack_host like EngineCore::load_dconv and uploaded with hipMalloc
static size_t dconv_layer_floats(int C) { const size_t h = C / 8; return h * C * 3 + 3 * h + 2 * C * h + 6 * (size_t)C + C; }
struct DConvTestLayer {
    std::vector<void *> bufs;
    DConvTimeLayer l{};
    ~DConvTestLayer() { for (void *p : bufs) (void)hipFree(p); }
    template <typename T> int up(const T *h, size_t n, const T **out) {
        void *p = nullptr;
        MI_HIP(hipMalloc(&p, n * sizeof(T)));
        bufs.push_back(p);
        MI_HIP(hipMemcpy(p, h, n * sizeof(T), hipMemcpyHostToDevice));
        *out = (const T *)p;
        return MI_OK;
    }
    int init(int C, const float *w) {
        const int h = C / 8;
        const float *w0 = w, *b0 = w0 + (size_t)h * C * 3, *g1w = b0 + h, *g1b = g1w + h, *w3 = g1b + h, *b3 = w3 + (size_t)2 * C * h,
                    *g2w = b3 + 2 * C, *g2b = g2w + 2 * C, *ls = g2b + 2 * C;
        const DConvHostPack p = dconv_pack_host(C, h, w0, b0, g1w, g1b, w3, b3);
        MI_TRY(up(p.w0.data(), p.w0.size(), &l.w.w0)); MI_TRY(up(p.b0.data(), p.b0.size(), &l.w.b0));
        MI_TRY(up(p.g1w.data(), p.g1w.size(), &l.w.g1w)); MI_TRY(up(p.g1b.data(), p.g1b.size(), &l.w.g1b));
        MI_TRY(up(p.w3.data(), p.w3.size(), &l.w.w3));
        MI_TRY(up(b3, (size_t)2 * C, &l.w.b3)); MI_TRY(up(g2w, (size_t)2 * C, &l.w.g2w)); MI_TRY(up(g2b, (size_t)2 * C, &l.w.g2b));
        MI_TRY(up(ls, (size_t)C, &l.w.ls));
        MI_TRY(up(p.gram_a.data(), p.gram_a.size(), &l.gram_a)); MI_TRY(up(p.gram_v.data(), p.gram_v.size(), &l.gram_v));
        MI_TRY(up(p.gram_c.data(), p.gram_c.size(), &l.gram_c)); MI_TRY(up(p.gram_e1.data(), p.gram_e1.size(), &l.gram_e1));
        MI_TRY(up(p.gram_e2.data(), p.gram_e2.size(), &l.gram_e2));
        l.sum_b3 = p.sum_b3; l.sum_b3sq = p.sum_b3sq;
        return MI_OK;
    }
};

// Scratch of the handle-free transform / normalisation entries: freed on return, after the stream has been waited for
struct TestScratch {
    std::vector<void *> bufs;
    ~TestScratch() { for (void *p : bufs) (void)hipFree(p); }
    template <typename T> int get(size_t n, T **out) {
        void *p = nullptr;
        MI_HIP(hipMalloc(&p, std::max<size_t>(n, 1) * sizeof(T)));
        bufs.push_back(p);
        *out = (T *)p;
        return MI_OK;
    }
};
// the stream is waited for before the scratch goes: a failure of the wait is the call's failure
static int finish_entry(int r, hipStream_t st, const char *who) {
    const hipError_t e = hipStreamSynchronize(st);
    if (e != hipSuccess && r == MI_OK) r = set_error(MI_EHIP, "%s: hipStreamSynchronize: %s", who, hipGetErrorString(e));
    return r;
}

// STFT frames (+ float64 statistics) -> [finalize mode 1 -> (norm, denorm)] -> transpose to the conv layout, normalised when norm_dev
// is given: the sequence of Model::forward / HModel::forward
static int stft_entry(const char *who, const float *mix_dev, int B, int L, float *x_dev, int x_pitch, float *norm_dev, float *denorm_dev,
                      hipStream_t st) {
    FftTables tb;
    MI_TRY(get_tables(&tb));
    const int T = (L + 1023) / 1024;
    TestScratch ws;
    float *zt = nullptr; double *stats = nullptr;
    MI_TRY(ws.get((size_t)B * T * 4 * 2048, &zt));
    MI_TRY(ws.get((size_t)2 * kStatSlots * B, &stats));
    MI_HIP(hipMemsetAsync(stats, 0, sizeof(double) * 2 * kStatSlots * B, st));
    int r = launch_stft_frames(mix_dev, B, L, tb, zt, stats, st);
    if (r == MI_OK && norm_dev) r = launch_finalize_stats(stats, B, 4.0 * 2048 * T, 1e-5f, 1, (float2 *)norm_dev, (float2 *)denorm_dev, st);
    if (r == MI_OK) r = launch_cac_transpose(zt, B, T, (const float2 *)norm_dev, x_dev, st, x_pitch);
    return finish_entry(r, st, who);
}

// A handle of the C interface is the EngineCore part of an engine.  An entry that needs one engine gets it here: a handle of
// the other kind is refused (MI_EINVAL, nullptr) before anything else reads it.
static const char *const kKindNames[2] = {"htdemucs", "hdemucs"};
template <typename Engine>
static Engine *engine_of(void *handle, EngineKind want, const char *entry) {
    EngineCore *core = static_cast<EngineCore *>(handle);
    if (core->kind != want) {
        set_error(MI_EINVAL, "%s: the handle belongs to the %s engine, this entry takes one of the %s engine", entry, kKindNames[core->kind], kKindNames[want]);
        return nullptr;
    }
    return static_cast<Engine *>(core);
}
// mi_conv_forward and the read slack of the shifted-run loaders (routes 2, 7 and 11: up to 8 bytes before and 20 bytes after the
// tensor at x, gemm_loop.h TapRows / TimeTrTaps / TimeEncTaps).  The engines give their buffers that slack; a caller of the C entry
// may hand in a tensor that begins or ends with its device allocation, and the transfer would then touch an address that is not
// mapped.  True when the allocation that holds x reaches kConvSlack bytes past both ends of the tensor
constexpr size_t kConvSlack = 128;
int g_conv_staged = 0;                 // mi_debug_conv_staged
static bool conv_reads_slack(int route) { return route == MI_ROUTE_DMATAP || route == MI_ROUTE_TAP_X6 || route == MI_ROUTE_TIME_X6; }
static bool conv_owns_slack(const float *x, size_t bytes) {
    hipDeviceptr_t base = nullptr;
    size_t size = 0;
    if (hipMemGetAddressRange(&base, &size, (hipDeviceptr_t)x) != hipSuccess) {
        (void)hipGetLastError();       // not an allocation the runtime knows: nothing to rely on
        return false;
    }
    const uintptr_t lo = (uintptr_t)base, hi = lo + size, p = (uintptr_t)x;
    return p >= lo + kConvSlack && p + bytes + kConvSlack <= hi;
}
// ... else the layer runs on a copy of x that has the slack: the same kernel on the same values.  The copy is scratch of the
// call, freed after the stream has been waited for
static int conv_forward_staged(const mi_conv_desc &din, size_t bytes, hipStream_t st) {
    TestScratch ws;
    unsigned char *buf = nullptr;
    MI_TRY(ws.get(bytes + 2 * kConvSlack, &buf));
    MI_HIP(hipMemsetAsync(buf, 0, bytes + 2 * kConvSlack, st));
    MI_HIP(hipMemcpyAsync(buf + kConvSlack, din.x, bytes, hipMemcpyDeviceToDevice, st));
    mi_conv_desc d = din;
    d.x = reinterpret_cast<const float *>(buf + kConvSlack);
    ++g_conv_staged;
    return finish_entry(launch_conv(d, st), st, "mi_conv_forward");
}

static Model *as_model(void *handle, const char *entry) { return engine_of<Model>(handle, ENGINE_HTDEMUCS, entry); }
static HModel *as_hmodel(void *handle, const char *entry) { return engine_of<HModel>(handle, ENGINE_HDEMUCS, entry); }

}  // namespace mi

using namespace mi;

extern "C" {

const char *mi_last_error(void) { return last_error_buf(); }
void mi_debug_set_post_launch_hook(void (*hook)(void *stream)) { g_post_launch_hook = hook; }
int mi_debug_last_conv_route(void) { return g_last_conv_route; }
int mi_debug_last_conv_tile(void) { return g_last_conv_tile; }
int mi_debug_conv_staged(void) { return g_conv_staged; }
int64_t mi_debug_conv_route_launches(int32_t route, int32_t epi) {
    if (route < 0 || route >= 16 || epi >= 8) return -1;
    int64_t n = 0;
    for (int e = 0; e < 8; ++e)
        if (epi < 0 || e == epi) n += mi::g_conv_route_launches[route][e];
    return n;
}
int mi_debug_conv_route(const struct mi_conv_desc *desc, int *tile) {
    if (!desc) return -1;
    if (conv_check_tile_m(*desc) != MI_OK) return -1;
    const ConvRoute r = conv_route(*desc);
    if (tile) *tile = r.tile;
    return r.route;
}
const char *mi_version(void) { return "demucs_amd 0.1 gfx950"; }

int mi_model_create(const mi_config *cfg, const mi_tensor_desc *weights, size_t n_weights, void **handle) {
    if (!cfg || !weights || !handle) return set_error(MI_EINVAL, "mi_model_create: null argument");
    *handle = nullptr;
    Model *m = new (std::nothrow) Model();
    if (!m) return set_error(MI_ENOMEM, "mi_model_create: host allocation failed");
    const int r = m->init(*cfg, weights, n_weights);
    if (r != MI_OK) { delete m; return r; }
    *handle = static_cast<EngineCore *>(m);
    return MI_OK;
}

void mi_model_destroy(void *handle) {
    if (!handle) return;
    Model *m = as_model(handle, "mi_model_destroy");
    if (!m) return;
    (void)hipDeviceSynchronize();
    delete m;
}

int mi_model_forward(void *handle, const float *mix_dev, float *out_dev, int32_t B, void *stream) {
    if (!handle) return set_error(MI_EINVAL, "mi_model_forward: null handle");
    Model *m = as_model(handle, "mi_model_forward");
    return m ? m->forward(mix_dev, out_dev, B, (hipStream_t)stream) : MI_EINVAL;
}

int mi_model_tap(void *handle, const char *name, float *dst_dev, int32_t B, int64_t *numel_per_item, void *stream) {
    if (!handle || !name || !numel_per_item) return set_error(MI_EINVAL, "mi_model_tap: null argument");
    Model *m = as_model(handle, "mi_model_tap");
    if (!m) return MI_EINVAL;
    const float *src = nullptr;
    const float **ptr_dev = &src;
    const std::string n(name);
    const int64_t T = m->T, Tf = 8 * T, Tt = m->Lt[4];
    static const int ch[4] = {48, 96, 192, 384}, fr[4] = {512, 128, 32, 8};
    *ptr_dev = nullptr;
    if (n == "x0") { *ptr_dev = m->w_x0; *numel_per_item = 4 * 2048 * T; }
    else if (n == "xt0") { *ptr_dev = m->w_xt0; *numel_per_item = 2 * (int64_t)m->SL; }
    else if (n == "yspec") { *ptr_dev = m->w_yspec; *numel_per_item = 4 * (int64_t)m->S * 2048 * T; }
    else if (n == "ytime") { *ptr_dev = m->w_ytime; *numel_per_item = 2 * (int64_t)m->S * m->SL; }
    else if (n == "tr_f") { *ptr_dev = m->w_tr_x[0][1]; *numel_per_item = 512 * Tf; }   // 5 layers: ends in buffer 1
    else if (n == "tr_t") { *ptr_dev = m->w_tr_x[1][1]; *numel_per_item = 512 * Tt; }
    else if (n.size() == 4 && n.compare(0, 3, "enc") == 0 && n[3] >= '0' && n[3] <= '3') {
        const int i = n[3] - '0'; *ptr_dev = m->w_skip[i]; *numel_per_item = (int64_t)ch[i] * fr[i] * T;
    } else if (n.size() == 5 && n.compare(0, 4, "tenc") == 0 && n[4] >= '0' && n[4] <= '3') {
        const int i = n[4] - '0'; *ptr_dev = m->w_skip_t[i]; *numel_per_item = (int64_t)ch[i] * m->Lp[i + 1];   // rows padded to a multiple of 4
    }
    if (!*ptr_dev) return set_error(MI_EINVAL, "mi_model_tap: unknown tap '%s'", name);
    if (dst_dev) {
        MI_REQUIRE(B >= 1 && B <= m->cfg.max_batch, "mi_model_tap: batch %d out of range", B);
        MI_HIP(hipMemcpyAsync(dst_dev, src, sizeof(float) * (size_t)B * *numel_per_item, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    }
    return MI_OK;
}

int mi_model_forward_core(void *handle, const float *mix_dev, const float *mag_dev, float *spec_out_dev, float *time_out_dev,
                          int32_t B, void *stream) {
    if (!handle) return set_error(MI_EINVAL, "mi_model_forward_core: null handle");
    Model *m = as_model(handle, "mi_model_forward_core");
    return m ? m->forward_core(mix_dev, mag_dev, spec_out_dev, time_out_dev, B, (hipStream_t)stream) : MI_EINVAL;
}

// ---- Hybrid Demucs v3 (hdemucs_mmi) handles ------------------------------------------------------------------------
int mi_hmodel_create(const mi_config *cfg, const mi_tensor_desc *weights, size_t n_weights, void **handle) {
    if (!cfg || !weights || !handle) return set_error(MI_EINVAL, "mi_hmodel_create: null argument");
    *handle = nullptr;
    HModel *m = new (std::nothrow) HModel();
    if (!m) return set_error(MI_ENOMEM, "mi_hmodel_create: host allocation failed");
    const int r = m->hinit(*cfg, weights, n_weights);
    if (r != MI_OK) { delete m; return r; }
    *handle = static_cast<EngineCore *>(m);
    return MI_OK;
}

void mi_hmodel_destroy(void *handle) {
    if (!handle) return;
    HModel *m = as_hmodel(handle, "mi_hmodel_destroy");
    if (!m) return;
    (void)hipDeviceSynchronize();
    delete m;
}

int mi_hmodel_forward(void *handle, const float *mix_dev, float *out_dev, int32_t B, int32_t length, void *stream) {
    if (!handle) return set_error(MI_EINVAL, "mi_hmodel_forward: null handle");
    HModel *m = as_hmodel(handle, "mi_hmodel_forward");
    return m ? m->hforward(mix_dev, out_dev, B, length, (hipStream_t)stream) : MI_EINVAL;
}

int mi_hmodel_tap(void *handle, const char *name, float *dst_dev, int32_t B, int64_t *numel_per_item, void *stream) {
    if (!handle || !name || !numel_per_item) return set_error(MI_EINVAL, "mi_hmodel_tap: null argument");
    HModel *m = as_hmodel(handle, "mi_hmodel_tap");
    if (!m) return MI_EINVAL;
    auto it = m->taps.find(name);
    if (it == m->taps.end()) return set_error(MI_EINVAL, "mi_hmodel_tap: unknown tap '%s'", name);
    *numel_per_item = it->second.second;
    if (dst_dev) {
        MI_REQUIRE(B >= 1 && B <= m->cfg.max_batch, "mi_hmodel_tap: batch %d out of range", B);
        MI_HIP(hipMemcpyAsync(dst_dev, it->second.first, sizeof(float) * (size_t)B * it->second.second, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    }
    return MI_OK;
}

int mi_hmodel_status(void *handle, void *stream) {
    if (!handle) return set_error(MI_EINVAL, "mi_hmodel_status: null handle");
    HModel *m = as_hmodel(handle, "mi_hmodel_status");
    if (!m) return MI_EINVAL;
    MI_HIP(hipStreamSynchronize((hipStream_t)stream));
    MI_REQUIRE(!m->lstm_timeout || *(volatile unsigned *)m->lstm_timeout == 0,
               "a forward's persistent LSTM kernel timed out waiting for its hidden-state exchange (GPU shared with another process's "
               "persistent kernels?): its output and every later one are invalid; MI_LSTM_STEPS=1 selects the one-launch-per-step recurrence");
    return MI_OK;
}

int64_t mi_hmodel_device_bytes(void *handle) {
    HModel *m = handle ? as_hmodel(handle, "mi_hmodel_device_bytes") : nullptr;
    return m ? m->weights.bytes + m->work.bytes : 0;
}

int mi_set_two_streams(int32_t enabled) {
    const int old = g_two_streams;
    g_two_streams = enabled ? 1 : 0;
    return old;
}

int mi_set_istft_fused(int32_t enabled) {
    const int old = g_istft_fused;
    g_istft_fused = enabled ? 1 : 0;
    return old;
}

int mi_set_split_bf16(int32_t enabled) {
    const int old = g_split_bf16;
    g_split_bf16 = enabled ? 1 : 0;
    return old;
}

int mi_set_transpose_tiles(int32_t enabled) {
    const int old = g_transpose_tiles == 7 ? 1 : g_transpose_tiles;
    g_transpose_tiles = enabled == 1 ? 7 : (enabled & 7);      // 1 = all three round-3 kernels; 2 / 4 / 6: see kernels.h
    return old;
}

int mi_profile_begin(void *handle) {
    if (!handle) return set_error(MI_EINVAL, "mi_profile_begin: null handle");
    static_cast<EngineCore *>(handle)->prof.begin();
    return MI_OK;
}

int mi_profile_end(void *handle, mi_profile_row *rows, int32_t max_rows, int32_t *n_rows, void *stream) {
    if (!handle || !rows || !n_rows) return set_error(MI_EINVAL, "mi_profile_end: null argument");
    EngineCore *m = static_cast<EngineCore *>(handle);
    MI_TRY(m->prof.end((hipStream_t)stream));
    int n = 0;
    for (const ProfRow &r : m->prof.rows) {
        if (!r.launches || n >= max_rows) continue;
        mi_profile_row &o = rows[n++];
        memset(&o, 0, sizeof(o));
        strncpy(o.name, r.name, sizeof(o.name) - 1);
        o.launches = r.launches; o.ms = r.ms; o.flops = r.flops; o.bytes = r.bytes;
    }
    *n_rows = n;
    return MI_OK;
}

int64_t mi_model_device_bytes(void *handle) {
    Model *m = handle ? as_model(handle, "mi_model_device_bytes") : nullptr;
    return m ? m->weights.bytes + (m->ws ? m->ws->mem.bytes : 0) : 0;       // weights + the (possibly shared) workspace
}

int mi_segments_gather(const float *track_dev, int64_t track_len, int32_t channels, const int64_t *starts_dev, int32_t B,
                       int32_t valid, float *seg_dev, int64_t seg_capacity, void *stream) {
    MI_REQUIRE(track_dev && starts_dev && seg_dev && B > 0 && B <= 65535 && valid > 0 && channels > 0 && channels <= 65535,
               "mi_segments_gather: bad argument");
    MI_REQUIRE((int64_t)B * channels * valid <= seg_capacity, "mi_segments_gather: %d x %d x %d floats do not fit seg_dev (%lld)", B,
               channels, valid, (long long)seg_capacity);
    return launch_segments_gather(track_dev, track_len, channels, starts_dev, B, valid, seg_dev, (hipStream_t)stream);
}

int mi_ola_accumulate(float *acc_dev, int64_t acc_len, int32_t rows, const float *model_out_dev, int32_t valid,
                      int64_t out_capacity, const int64_t *offs_dev, const int32_t *lens_dev, const int32_t *trim_dev, int32_t B,
                      int64_t span_lo, int64_t span_hi, const float *weight_dev, int32_t weight_len, void *stream) {
    MI_REQUIRE(acc_dev && model_out_dev && offs_dev && lens_dev && trim_dev && weight_dev && B > 0 && rows > 0 && rows <= 65535 &&
               valid > 0 && weight_len > 0, "mi_ola_accumulate: bad argument");
    MI_REQUIRE((int64_t)B * rows * valid <= out_capacity, "mi_ola_accumulate: %d x %d x %d floats exceed model_out_dev (%lld)", B, rows,
               valid, (long long)out_capacity);
    MI_REQUIRE(span_hi <= acc_len, "mi_ola_accumulate: span end %lld past the accumulator (%lld)", (long long)span_hi, (long long)acc_len);
    return launch_ola_accumulate(acc_dev, acc_len, rows, model_out_dev, valid, offs_dev, lens_dev, trim_dev, B, span_lo, span_hi,
                                 weight_dev, weight_len, (hipStream_t)stream);
}

int mi_ola_finish(float *acc_dev, int64_t acc_len, int32_t rows, int64_t acc_off0, const int64_t *offs_dev,
                  const int32_t *lens_dev, int32_t n_segments, int32_t max_len, const float *weight_dev, void *stream) {
    MI_REQUIRE(acc_dev && offs_dev && lens_dev && weight_dev && n_segments > 0 && rows > 0 && rows <= 65535,
               "mi_ola_finish: bad argument");
    return launch_ola_finish(acc_dev, acc_len, rows, acc_off0, offs_dev, lens_dev, n_segments, max_len, weight_dev,
                             (hipStream_t)stream);
}

int mi_segments_gather_packed(const float *tracks_dev, int64_t tracks_capacity, int32_t channels, const int64_t *items_dev, int32_t B,
                              int32_t valid, float *seg_dev, int64_t seg_capacity, void *stream) {
    MI_REQUIRE(tracks_dev && items_dev && seg_dev && B > 0 && B <= 65535 && valid > 0 && channels > 0 && channels <= 65535 &&
               tracks_capacity > 0, "mi_segments_gather_packed: bad argument");
    MI_REQUIRE((int64_t)B * channels * valid <= seg_capacity, "mi_segments_gather_packed: %d x %d x %d floats do not fit seg_dev (%lld)",
               B, channels, valid, (long long)seg_capacity);
    return launch_segments_gather_packed(tracks_dev, tracks_capacity, channels, items_dev, B, valid, seg_dev, (hipStream_t)stream);
}

int mi_ola_accumulate_packed(float *acc_dev, int64_t acc_capacity, int32_t rows, const float *model_out_dev, int32_t valid,
                             int64_t out_capacity, const int64_t *items_dev, int32_t B, const int64_t *tiles_dev, int32_t n_tiles,
                             const float *weights_dev, int64_t weights_capacity, void *stream) {
    MI_REQUIRE(acc_dev && model_out_dev && items_dev && tiles_dev && weights_dev && B > 0 && rows > 0 && rows <= 65535 && valid > 0 &&
               n_tiles > 0 && acc_capacity > 0 && weights_capacity > 0, "mi_ola_accumulate_packed: bad argument");
    MI_REQUIRE((int64_t)B * rows * valid <= out_capacity, "mi_ola_accumulate_packed: %d x %d x %d floats exceed model_out_dev (%lld)", B,
               rows, valid, (long long)out_capacity);
    return launch_ola_accumulate_packed(acc_dev, acc_capacity, rows, model_out_dev, valid, items_dev, B, tiles_dev, n_tiles, weights_dev,
                                        weights_capacity, (hipStream_t)stream);
}

int mi_ola_finish_packed(float *acc_dev, int64_t acc_capacity, int32_t rows, const int64_t *tiles_dev, int32_t n_tiles,
                         const int64_t *segs_dev, int32_t n_segs, const float *weights_dev, int64_t weights_capacity, void *stream) {
    MI_REQUIRE(acc_dev && tiles_dev && segs_dev && weights_dev && rows > 0 && rows <= 65535 && n_tiles > 0 && n_segs > 0 &&
               acc_capacity > 0 && weights_capacity > 0, "mi_ola_finish_packed: bad argument");
    return launch_ola_finish_packed(acc_dev, acc_capacity, rows, tiles_dev, n_tiles, segs_dev, n_segs, weights_dev, weights_capacity,
                                    (hipStream_t)stream);
}

int mi_stream_emit(const float *acc_dev, int64_t acc_capacity, int32_t n_sources, int32_t channels, const int64_t *passes_dev,
                   int32_t n_passes, const int64_t *segs_dev, int32_t n_segs, const float *weights_dev, int64_t weights_capacity,
                   const float *scales_dev, int32_t n_members, int32_t shifts, int32_t bag, const float *stats_dev, int64_t n,
                   float *out_dev, int64_t out_capacity, void *stream) {
    MI_REQUIRE(acc_dev && passes_dev && segs_dev && weights_dev && scales_dev && out_dev && n_sources > 0 && channels > 0 &&
               (int64_t)n_sources * channels <= 65535 && n_passes > 0 && n_segs >= 0 && n_members > 0 && shifts >= 0 && n >= 1 &&
               acc_capacity >= 0 && weights_capacity > 0, "mi_stream_emit: bad argument");
    MI_REQUIRE((int64_t)n_sources * channels * n <= out_capacity, "mi_stream_emit: %d x %d x %lld floats exceed out_dev (%lld)",
               n_sources, channels, (long long)n, (long long)out_capacity);
    return launch_stream_emit(acc_dev, acc_capacity, n_sources, channels, passes_dev, n_passes, segs_dev, n_segs, weights_dev,
                              weights_capacity, scales_dev, n_members, shifts, bag, stats_dev, n, out_dev, (hipStream_t)stream);
}

int mi_streams_emit(const float *acc_dev, int64_t acc_capacity, int32_t n_sources, int32_t channels, const int64_t *streams_dev,
                    int32_t n_streams, int64_t max_n, const int64_t *passes_dev, int32_t n_passes, const int64_t *segs_dev, int32_t n_segs,
                    const float *weights_dev, int64_t weights_capacity, const float *scales_dev, int32_t n_members, int32_t shifts,
                    int32_t bag, const float *stats_dev, int32_t n_stats, float *out_dev, int64_t out_capacity, void *stream) {
    MI_REQUIRE(acc_dev && streams_dev && passes_dev && segs_dev && weights_dev && scales_dev && out_dev && n_sources > 0 && channels > 0 &&
               (int64_t)n_sources * channels <= 65535 && n_streams > 0 && n_streams <= 65535 && max_n >= 1 &&
               max_n <= (int64_t)INT32_MAX * 256 && n_passes > 0 && n_segs >= 0 && n_members > 0 && shifts >= 0 && n_stats >= 0 &&
               (n_stats == 0 || stats_dev) && acc_capacity >= 0 && weights_capacity > 0 && out_capacity >= 0,
               "mi_streams_emit: bad argument");
    return launch_streams_emit(acc_dev, acc_capacity, n_sources, channels, streams_dev, n_streams, max_n, passes_dev, n_passes, segs_dev,
                               n_segs, weights_dev, weights_capacity, scales_dev, n_members, shifts, bag, stats_dev, n_stats, out_dev,
                               out_capacity, (hipStream_t)stream);
}

int mi_streams_append(float *win_dev, int64_t win_capacity, int32_t channels, const int64_t *table_dev, int32_t n_streams, int64_t max_n,
                      const float *stats_dev, int32_t n_stats, void *stream) {
    MI_REQUIRE(win_dev && table_dev && channels > 0 && n_streams > 0 && (int64_t)n_streams * channels <= 65535 && max_n >= 1 &&
               max_n <= (int64_t)INT32_MAX * 1024 && win_capacity > 0 && n_stats >= 0 && (n_stats == 0 || stats_dev),
               "mi_streams_append: bad argument");
    return launch_streams_append(win_dev, win_capacity, channels, table_dev, n_streams, max_n, stats_dev, n_stats, (hipStream_t)stream);
}

int mi_streams_convert_append(float *win_dev, int64_t win_capacity, int32_t channels, const int64_t *table_dev, int32_t n_streams,
                              int64_t max_groups, const float *bank_dev, int64_t bank_capacity, float *hist_dev, int64_t hist_capacity,
                              const float *stats_dev, int32_t n_stats, int32_t lds_floats, void *stream) {
    MI_REQUIRE(win_dev && table_dev && channels > 0 && n_streams > 0 && (int64_t)n_streams * channels <= 65535 && max_groups >= 1 &&
               max_groups <= INT32_MAX && win_capacity > 0 && bank_capacity >= 0 && (bank_capacity == 0 || bank_dev) &&
               hist_capacity >= 0 && (hist_capacity == 0 || hist_dev) && n_stats >= 0 && (n_stats == 0 || stats_dev) &&
               lds_floats >= 1 && lds_floats <= MI_CVT_LDS_FLOATS, "mi_streams_convert_append: bad argument");
    return launch_streams_convert_append(win_dev, win_capacity, channels, table_dev, n_streams, max_groups, bank_dev, bank_capacity,
                                         hist_dev, hist_capacity, stats_dev, n_stats, lds_floats, (hipStream_t)stream);
}

int mi_pcm_planar(const void *src_dev, int32_t fmt, int32_t src_ch, int64_t n, int32_t channels, const float *stats_dev, float *dst_dev,
                  void *stream) {
    MI_REQUIRE(fmt == MI_PCM_I16 || fmt == MI_PCM_I24 || fmt == MI_PCM_F32, "mi_pcm_planar: unknown format %d", fmt);
    MI_REQUIRE(src_ch >= 1 && channels >= 1 && (src_ch == 1 || src_ch >= channels) && n >= 0 && n <= INT64_MAX / 4 / src_ch,
               "mi_pcm_planar: bad argument");
    if (n == 0) return MI_OK;
    const int width = fmt == MI_PCM_I16 ? 2 : fmt == MI_PCM_I24 ? 3 : 4;
    MI_REQUIRE(src_dev && dst_dev && n * src_ch * width / 16 + 24 <= (int64_t)INT32_MAX * 256, "mi_pcm_planar: bad argument");
    MI_REQUIRE(width == 3 || (uintptr_t)src_dev % width == 0, "mi_pcm_planar: the source is not aligned to its %d-byte samples", width);
    return launch_pcm_planar((const unsigned char *)src_dev, fmt, src_ch, n, channels, stats_dev, dst_dev, (hipStream_t)stream);
}

int mi_streams_append_pcm(float *win_dev, int64_t win_capacity, int32_t channels, const int64_t *table_dev, int32_t n_streams,
                          int64_t max_bytes, const float *stats_dev, int32_t n_stats, void *stream) {
    MI_REQUIRE(win_dev && table_dev && channels > 0 && n_streams > 0 && n_streams <= 65535 && max_bytes >= 1 &&
               max_bytes <= (int64_t)INT32_MAX * 1024 && win_capacity > 0 && n_stats >= 0 && (n_stats == 0 || stats_dev),
               "mi_streams_append_pcm: bad argument");
    return launch_streams_append_pcm(win_dev, win_capacity, channels, table_dev, n_streams, max_bytes, stats_dev, n_stats,
                                     (hipStream_t)stream);
}

int mi_streams_convert_append_pcm(float *win_dev, int64_t win_capacity, int32_t channels, const int64_t *table_dev, int32_t n_streams,
                                  int64_t max_groups, const float *bank_dev, int64_t bank_capacity, float *hist_dev,
                                  int64_t hist_capacity, const float *stats_dev, int32_t n_stats, int32_t lds_floats, void *stream) {
    MI_REQUIRE(win_dev && table_dev && channels > 0 && n_streams > 0 && (int64_t)n_streams * channels <= 65535 && max_groups >= 1 &&
               max_groups <= INT32_MAX && win_capacity > 0 && bank_capacity >= 0 && (bank_capacity == 0 || bank_dev) &&
               hist_capacity >= 0 && (hist_capacity == 0 || hist_dev) && n_stats >= 0 && (n_stats == 0 || stats_dev) &&
               lds_floats >= 1 && lds_floats <= MI_CVT_LDS_FLOATS, "mi_streams_convert_append_pcm: bad argument");
    return launch_streams_convert_append_pcm(win_dev, win_capacity, channels, table_dev, n_streams, max_groups, bank_dev, bank_capacity,
                                             hist_dev, hist_capacity, stats_dev, n_stats, lds_floats, (hipStream_t)stream);
}

int mi_streams_compact(float *dst_dev, int64_t dst_capacity, const float *src_dev, int64_t src_capacity, const int64_t *table_dev,
                       int32_t n_rows, int64_t max_len, void *stream) {
    MI_REQUIRE(dst_dev && src_dev && table_dev && dst_dev != src_dev && n_rows > 0 && n_rows <= 65535 && max_len >= 1 && dst_capacity > 0 &&
               src_capacity >= 0, "mi_streams_compact: bad argument");
    return launch_streams_compact(dst_dev, dst_capacity, src_dev, src_capacity, table_dev, n_rows, max_len, (hipStream_t)stream);
}

int32_t mi_mono_stats_scratch_bytes(void) { return post_stats_scratch_bytes(); }

int mi_mono_stats(const float *wav_dev, int32_t channels, int64_t length, void *scratch_dev, float *stats_dev, void *stream) {
    MI_REQUIRE(wav_dev && scratch_dev && stats_dev && channels >= 1 && length >= 1, "mi_mono_stats: bad argument");
    return launch_mono_stats(wav_dev, channels, length, (double *)scratch_dev, stats_dev, (hipStream_t)stream);
}

int32_t mi_mono_stats_state_bytes(void) { return mono_stats_state_bytes(); }

int mi_mono_stats_update(const void *src_dev, int32_t fmt, int32_t src_ch, int64_t n, int32_t channels, int64_t before, void *state_dev,
                         void *stream) {
    MI_REQUIRE(fmt == MI_PCM_PLANAR || fmt == MI_PCM_I16 || fmt == MI_PCM_I24 || fmt == MI_PCM_F32,
               "mi_mono_stats_update: unknown format %d", fmt);
    const bool planar = fmt == MI_PCM_PLANAR;
    const int64_t per = planar ? channels : src_ch;        // samples per position in the block
    MI_REQUIRE(channels >= 1 && (planar || (src_ch >= 1 && (src_ch == 1 || src_ch >= channels))) && n >= 0 && n <= INT64_MAX / 4 / per &&
                   before >= 0 && before <= INT64_MAX - n,
               "mi_mono_stats_update: bad argument");
    MI_REQUIRE(state_dev && (uintptr_t)state_dev % 8 == 0, "mi_mono_stats_update: the state is null or not aligned to its doubles");
    if (n == 0) return MI_OK;
    const int width = fmt == MI_PCM_I16 ? 2 : fmt == MI_PCM_I24 ? 3 : 4;
    MI_REQUIRE(src_dev, "mi_mono_stats_update: bad argument");
    MI_REQUIRE(width == 3 || (uintptr_t)src_dev % width == 0, "mi_mono_stats_update: the source is not aligned to its %d-byte samples",
               width);
    return launch_mono_stats_update((const unsigned char *)src_dev, fmt, src_ch, n, channels, before, (double *)state_dev,
                                    (hipStream_t)stream);
}

int mi_mono_stats_finish(const void *state_dev, int64_t length, void *scratch_dev, float *stats_dev, void *stream) {
    MI_REQUIRE(state_dev && (uintptr_t)state_dev % 8 == 0 && scratch_dev && stats_dev && length >= 1, "mi_mono_stats_finish: bad argument");
    return launch_mono_stats_finish((const double *)state_dev, length, (double *)scratch_dev, stats_dev, (hipStream_t)stream);
}

int64_t mi_sdr_state_bytes(int32_t n_sources) { return n_sources >= 1 && n_sources <= 8 ? sdr_state_bytes(n_sources) : 0; }
int64_t mi_sdr_scratch_bytes(int32_t n_sources) { return n_sources >= 1 && n_sources <= 8 ? sdr_scratch_bytes(n_sources) : 0; }

int mi_sdr_update(const void *const *refs, int32_t fmt, int32_t src_ch, int64_t ref_stride, const float *est_dev, int64_t est_stride,
                  int32_t n_sources, int32_t channels, int64_t n, int64_t before, void *state_dev, void *stream) {
    MI_REQUIRE(fmt == MI_PCM_PLANAR || fmt == MI_PCM_I16 || fmt == MI_PCM_I24 || fmt == MI_PCM_F32, "mi_sdr_update: unknown format %d", fmt);
    MI_REQUIRE(n_sources >= 1 && n_sources <= 8, "mi_sdr_update: %d sources (1 to 8)", n_sources);
    const bool planar = fmt == MI_PCM_PLANAR;
    const int64_t rows = (int64_t)n_sources * channels, most = INT64_MAX / 4 / std::max<int64_t>(rows, 1);
    MI_REQUIRE(channels >= 1 && channels <= 65535 && n >= 0 && before >= 0 && before <= INT64_MAX - n && est_stride >= n && est_stride <= most,
               "mi_sdr_update: bad argument");
    MI_REQUIRE(planar ? (ref_stride >= n && ref_stride <= most)
                      : (src_ch >= 1 && (src_ch == 1 || src_ch >= channels) && n <= INT64_MAX / 4 / src_ch),
               "mi_sdr_update: bad argument");
    MI_REQUIRE(state_dev && (uintptr_t)state_dev % 8 == 0, "mi_sdr_update: the state is null or not aligned to its doubles");
    if (n == 0) return MI_OK;
    MI_REQUIRE(refs && est_dev && (uintptr_t)est_dev % 4 == 0, "mi_sdr_update: bad argument");
    const int width = fmt == MI_PCM_I16 ? 2 : fmt == MI_PCM_I24 ? 3 : 4;
    for (int s = 0; s < (planar ? 1 : n_sources); ++s) {
        MI_REQUIRE(refs[s], "mi_sdr_update: null reference %d", s);
        MI_REQUIRE(width == 3 || (uintptr_t)refs[s] % width == 0, "mi_sdr_update: reference %d is not aligned to its %d-byte samples", s,
                   width);
    }
    return launch_sdr_update(refs, fmt, src_ch, ref_stride, est_dev, est_stride, n_sources, channels, n, before, (double *)state_dev,
                             (hipStream_t)stream);
}

int mi_sdr_finish(const void *state_dev, int32_t n_sources, void *scratch_dev, double *sums_dev, void *stream) {
    MI_REQUIRE(n_sources >= 1 && n_sources <= 8, "mi_sdr_finish: %d sources (1 to 8)", n_sources);
    MI_REQUIRE(state_dev && (uintptr_t)state_dev % 8 == 0 && scratch_dev && (uintptr_t)scratch_dev % 8 == 0 && sums_dev &&
                   (uintptr_t)sums_dev % 8 == 0, "mi_sdr_finish: bad argument");
    return launch_sdr_finish((const double *)state_dev, n_sources, (double *)scratch_dev, sums_dev, (hipStream_t)stream);
}

int mi_sdr(const float *ref_dev, const float *est_dev, int32_t B, int32_t n_sources, int32_t channels, int64_t length, void *state_dev,
           void *scratch_dev, double *sums_dev, void *stream) {
    MI_REQUIRE(n_sources >= 1 && n_sources <= 8, "mi_sdr: %d sources (1 to 8)", n_sources);
    MI_REQUIRE(B >= 1 && channels >= 1 && channels <= 65535 && length >= 0 && length <= INT64_MAX / 4 / ((int64_t)n_sources * channels) / B,
               "mi_sdr: bad argument");
    MI_REQUIRE(state_dev && (uintptr_t)state_dev % 8 == 0 && scratch_dev && (uintptr_t)scratch_dev % 8 == 0 && sums_dev &&
                   (uintptr_t)sums_dev % 8 == 0, "mi_sdr: bad argument");
    MI_REQUIRE(length == 0 || (ref_dev && est_dev && (uintptr_t)ref_dev % 4 == 0 && (uintptr_t)est_dev % 4 == 0), "mi_sdr: bad argument");
    return launch_sdr(ref_dev, est_dev, B, n_sources, channels, length, (double *)state_dev, (double *)scratch_dev, sums_dev,
                      (hipStream_t)stream);
}

int mi_track_affine(float *x_dev, int64_t numel, const float *stats_dev, int32_t inverse, void *stream) {
    MI_REQUIRE(x_dev && stats_dev && numel >= 1 && (inverse == 0 || inverse == 1), "mi_track_affine: bad argument");
    return launch_track_affine(x_dev, numel, stats_dev, inverse, (hipStream_t)stream);
}

int mi_prevent_clip(const float *x_dev, int64_t numel, int32_t mode, void *peak_dev, float *y_dev, void *stream) {
    MI_REQUIRE(x_dev && y_dev && peak_dev && numel >= 1, "mi_prevent_clip: bad argument");
    MI_REQUIRE(mode >= MI_CLIP_RESCALE && mode <= MI_CLIP_TANH, "mi_prevent_clip: unknown mode %d", mode);
    return launch_prevent_clip(x_dev, numel, mode, (unsigned *)peak_dev, y_dev, (hipStream_t)stream);
}

int mi_two_stems(const float *const *stems_dev, int32_t n_stems, int32_t selected, const float *origin_dev, int32_t minus, int64_t numel,
                 float *y_dev, void *stream) {
    MI_REQUIRE(stems_dev && y_dev && n_stems >= 1 && n_stems <= 8 && selected >= 0 && selected < n_stems && numel >= 1,
               "mi_two_stems: bad argument");
    MI_REQUIRE(!minus || origin_dev, "mi_two_stems: the \"minus\" method needs the original mix");
    for (int k = 0; k < n_stems; ++k) MI_REQUIRE(stems_dev[k], "mi_two_stems: null stem %d", k);
    return launch_two_stems(stems_dev, n_stems, selected, origin_dev, minus ? 1 : 0, numel, y_dev, (hipStream_t)stream);
}

int mi_deliver_peaks(const int64_t *table_dev, int32_t n_rows, int64_t max_n, int32_t n_sources, int32_t channels, void *peaks_dev,
                     int32_t n_peaks, int64_t dst_capacity, void *stream) {
    MI_REQUIRE(table_dev && peaks_dev && n_rows > 0 && n_rows <= 65535 && max_n >= 1 && max_n <= (int64_t)INT32_MAX * 1024 &&
               n_sources > 0 && channels > 0 && n_peaks > 0 && dst_capacity >= 0, "mi_deliver_peaks: bad argument");
    return launch_deliver_peaks(table_dev, n_rows, max_n, n_sources, channels, (unsigned *)peaks_dev, n_peaks, dst_capacity,
                                (hipStream_t)stream);
}

int mi_deliver_pcm(const int64_t *table_dev, int32_t n_rows, int64_t max_n, int32_t n_sources, int32_t channels, const void *peaks_dev,
                   int32_t n_peaks, void *dst_dev, int64_t dst_capacity, void *stream) {
    MI_REQUIRE(table_dev && dst_dev && n_rows > 0 && n_rows <= 65535 && max_n >= 1 && max_n <= (int64_t)INT32_MAX * 1024 &&
               n_sources > 0 && channels > 0 && n_peaks >= 0 && (n_peaks == 0 || peaks_dev) && dst_capacity >= 0,
               "mi_deliver_pcm: bad argument");
    MI_REQUIRE(((uintptr_t)dst_dev & 3) == 0, "mi_deliver_pcm: dst_dev must be 4-byte aligned");
    return launch_deliver_pcm(table_dev, n_rows, max_n, n_sources, channels, (const unsigned *)peaks_dev, n_peaks,
                              (unsigned char *)dst_dev, dst_capacity, (hipStream_t)stream);
}

int mi_deliver_resample_pcm(const int64_t *table_dev, int32_t n_rows, int64_t max_groups, int32_t n_sources, int32_t channels,
                            const float *bank_dev, int64_t bank_capacity, float *hist_dev, int64_t hist_capacity, int32_t lds_floats,
                            void *dst_dev, int64_t dst_capacity, void *stream) {
    MI_REQUIRE(table_dev && dst_dev && n_rows > 0 && n_rows <= 65535 && max_groups >= 1 && max_groups <= INT32_MAX && n_sources > 0 &&
               channels > 0 && bank_capacity >= 0 && (bank_capacity == 0 || bank_dev) && hist_capacity >= 0 &&
               (hist_capacity == 0 || hist_dev) && lds_floats >= 1 && lds_floats <= MI_RATE_LDS_FLOATS && dst_capacity >= 0,
               "mi_deliver_resample_pcm: bad argument");
    MI_REQUIRE(((uintptr_t)dst_dev & 3) == 0, "mi_deliver_resample_pcm: dst_dev must be 4-byte aligned");
    return launch_deliver_resample_pcm(table_dev, n_rows, max_groups, n_sources, channels, bank_dev, bank_capacity, hist_dev,
                                       hist_capacity, lds_floats, (unsigned char *)dst_dev, dst_capacity, (hipStream_t)stream);
}

int mi_deliver_peaks_update(const int64_t *table_dev, int32_t n_rows, int64_t max_n, int32_t n_sources, int32_t channels, void *peaks_dev,
                            int32_t n_peaks, void *stream) {
    MI_REQUIRE(table_dev && peaks_dev && n_rows > 0 && n_rows <= 65535 && max_n >= 1 && max_n <= (int64_t)INT32_MAX * 1024 &&
               n_sources > 0 && channels > 0 && n_peaks > 0, "mi_deliver_peaks_update: bad argument");
    return launch_deliver_peaks_update(table_dev, n_rows, max_n, n_sources, channels, (unsigned *)peaks_dev, n_peaks, (hipStream_t)stream);
}

int mi_deliver_resample_peaks(const int64_t *table_dev, int32_t n_rows, int64_t max_groups, int32_t n_sources, int32_t channels,
                              const float *bank_dev, int64_t bank_capacity, float *hist_dev, int64_t hist_capacity, int32_t lds_floats,
                              const int32_t *slots_dev, void *peaks_dev, int32_t n_peaks, void *stream) {
    MI_REQUIRE(table_dev && slots_dev && peaks_dev && n_peaks > 0 && n_rows > 0 && n_rows <= 65535 && max_groups >= 1 &&
               max_groups <= INT32_MAX && n_sources > 0 && channels > 0 && bank_capacity >= 0 && (bank_capacity == 0 || bank_dev) &&
               hist_capacity >= 0 && (hist_capacity == 0 || hist_dev) && lds_floats >= 1 && lds_floats <= MI_RATE_LDS_FLOATS,
               "mi_deliver_resample_peaks: bad argument");
    return launch_deliver_resample_peaks(table_dev, n_rows, max_groups, n_sources, channels, bank_dev, bank_capacity, hist_dev,
                                         hist_capacity, lds_floats, slots_dev, (unsigned *)peaks_dev, n_peaks, (hipStream_t)stream);
}

int mi_deliver_resample_pcm_peaks(const int64_t *table_dev, int32_t n_rows, int64_t max_groups, int32_t n_sources, int32_t channels,
                                  const float *bank_dev, int64_t bank_capacity, float *hist_dev, int64_t hist_capacity, int32_t lds_floats,
                                  void *dst_dev, int64_t dst_capacity, const int32_t *slots_dev, const void *peaks_dev, int32_t n_peaks,
                                  void *stream) {
    MI_REQUIRE(table_dev && dst_dev && n_rows > 0 && n_rows <= 65535 && max_groups >= 1 && max_groups <= INT32_MAX && n_sources > 0 &&
               channels > 0 && bank_capacity >= 0 && (bank_capacity == 0 || bank_dev) && hist_capacity >= 0 &&
               (hist_capacity == 0 || hist_dev) && lds_floats >= 1 && lds_floats <= MI_RATE_LDS_FLOATS && dst_capacity >= 0 &&
               slots_dev && n_peaks >= 0 && (n_peaks == 0 || peaks_dev), "mi_deliver_resample_pcm_peaks: bad argument");
    MI_REQUIRE(((uintptr_t)dst_dev & 3) == 0, "mi_deliver_resample_pcm_peaks: dst_dev must be 4-byte aligned");
    return launch_deliver_resample_pcm_peaks(table_dev, n_rows, max_groups, n_sources, channels, bank_dev, bank_capacity, hist_dev,
                                             hist_capacity, lds_floats, (unsigned char *)dst_dev, dst_capacity, slots_dev,
                                             (const unsigned *)peaks_dev, n_peaks, (hipStream_t)stream);
}

int mi_deliver_mix_pcm(const int64_t *table_dev, int32_t n_rows, int64_t max_n, int32_t n_sources, int32_t channels,
                       const void *peaks_dev, int32_t n_peaks, void *dst_dev, int64_t dst_capacity, void *stream) {
    MI_REQUIRE(table_dev && dst_dev && n_rows > 0 && n_rows <= 65535 && max_n >= 1 && max_n <= (int64_t)INT32_MAX * 1024 &&
               n_sources > 0 && n_sources <= MI_MIX_MAX_SOURCES && channels > 0 && n_peaks >= 0 && (n_peaks == 0 || peaks_dev) &&
               dst_capacity >= 0, "mi_deliver_mix_pcm: bad argument");
    MI_REQUIRE(((uintptr_t)dst_dev & 3) == 0, "mi_deliver_mix_pcm: dst_dev must be 4-byte aligned");
    return launch_deliver_mix_pcm(table_dev, n_rows, max_n, n_sources, channels, (const unsigned *)peaks_dev, n_peaks,
                                  (unsigned char *)dst_dev, dst_capacity, (hipStream_t)stream);
}

int mi_deliver_mix_peaks(const int64_t *table_dev, int32_t n_rows, int64_t max_n, int32_t n_sources, int32_t channels, void *peaks_dev,
                         int32_t n_peaks, int64_t dst_capacity, void *stream) {
    MI_REQUIRE(table_dev && peaks_dev && n_rows > 0 && n_rows <= 65535 && max_n >= 1 && max_n <= (int64_t)INT32_MAX * 1024 &&
               n_sources > 0 && n_sources <= MI_MIX_MAX_SOURCES && channels > 0 && n_peaks > 0 && dst_capacity >= 0,
               "mi_deliver_mix_peaks: bad argument");
    return launch_deliver_mix_peaks(table_dev, n_rows, max_n, n_sources, channels, (unsigned *)peaks_dev, n_peaks, dst_capacity,
                                    (hipStream_t)stream);
}

int mi_deliver_mix_peaks_update(const int64_t *table_dev, int32_t n_rows, int64_t max_n, int32_t n_sources, int32_t channels,
                                void *peaks_dev, int32_t n_peaks, void *stream) {
    MI_REQUIRE(table_dev && peaks_dev && n_rows > 0 && n_rows <= 65535 && max_n >= 1 && max_n <= (int64_t)INT32_MAX * 1024 &&
               n_sources > 0 && n_sources <= MI_MIX_MAX_SOURCES && channels > 0 && n_peaks > 0, "mi_deliver_mix_peaks_update: bad argument");
    return launch_deliver_mix_peaks_update(table_dev, n_rows, max_n, n_sources, channels, (unsigned *)peaks_dev, n_peaks,
                                           (hipStream_t)stream);
}

int mi_deliver_mix_auto_pcm(const int64_t *table_dev, int64_t table_len, int32_t n_rows, int64_t max_n, int32_t n_sources,
                            int32_t channels, const void *peaks_dev, int32_t n_peaks, void *dst_dev, int64_t dst_capacity, void *stream) {
    MI_REQUIRE(table_dev && dst_dev && n_rows > 0 && n_rows <= 65535 && table_len <= INT32_MAX &&
               table_len >= (int64_t)n_rows * MI_AUTO_COLS && max_n >= 1 && max_n <= (int64_t)INT32_MAX * 1024 && n_sources > 0 &&
               n_sources <= MI_MIX_MAX_SOURCES && channels > 0 && n_peaks >= 0 && (n_peaks == 0 || peaks_dev) && dst_capacity >= 0,
               "mi_deliver_mix_auto_pcm: bad argument");
    MI_REQUIRE(((uintptr_t)dst_dev & 3) == 0, "mi_deliver_mix_auto_pcm: dst_dev must be 4-byte aligned");
    return launch_deliver_mix_auto_pcm(table_dev, table_len, n_rows, max_n, n_sources, channels, (const unsigned *)peaks_dev, n_peaks,
                                       (unsigned char *)dst_dev, dst_capacity, (hipStream_t)stream);
}

int mi_deliver_mix_auto_peaks(const int64_t *table_dev, int64_t table_len, int32_t n_rows, int64_t max_n, int32_t n_sources,
                              int32_t channels, void *peaks_dev, int32_t n_peaks, int64_t dst_capacity, void *stream) {
    MI_REQUIRE(table_dev && peaks_dev && n_rows > 0 && n_rows <= 65535 && table_len <= INT32_MAX &&
               table_len >= (int64_t)n_rows * MI_AUTO_COLS && max_n >= 1 && max_n <= (int64_t)INT32_MAX * 1024 && n_sources > 0 &&
               n_sources <= MI_MIX_MAX_SOURCES && channels > 0 && n_peaks > 0 && dst_capacity >= 0,
               "mi_deliver_mix_auto_peaks: bad argument");
    return launch_deliver_mix_auto_peaks(table_dev, table_len, n_rows, max_n, n_sources, channels, (unsigned *)peaks_dev, n_peaks,
                                         dst_capacity, (hipStream_t)stream);
}

int mi_loudness_update(const int64_t *table_dev, int32_t n_rows, int64_t max_n, int64_t max_blocks, int32_t n_sources, int32_t channels,
                       const double *coef, int64_t hop, int64_t warm, float *hist_dev, int64_t hist_capacity, double *energies_dev,
                       int64_t energies_capacity, float *work_dev, int64_t work_capacity, void *stream) {
    MI_REQUIRE(table_dev && coef && energies_dev && work_dev && n_rows > 0 && n_rows <= 65535 && max_n >= 1 &&
               max_n <= (int64_t)INT32_MAX * 256 && max_blocks >= 0 && max_blocks <= (int64_t)INT32_MAX * 64 && n_sources > 0 &&
               n_sources <= MI_MIX_MAX_SOURCES && channels > 0 && channels <= 65535 && hist_capacity >= 0 &&
               (hist_dev || hist_capacity == 0) && energies_capacity >= 0 && work_capacity >= 0,
               "mi_loudness_update: bad argument");
    if (hop < 1 || warm < 0) return MI_OK;                         // every row is skipped whole
    return launch_loudness_update(table_dev, n_rows, max_n, max_blocks, n_sources, channels, coef, hop, warm, hist_dev, hist_capacity,
                                  energies_dev, energies_capacity, work_dev, work_capacity, (hipStream_t)stream);
}

int mi_true_peak_update(const int64_t *table_dev, int32_t n_rows, int64_t max_n, int32_t n_sources, int32_t channels,
                        const float *bank_dev, int32_t phases, int32_t taps, float *hist_dev, int64_t hist_capacity, void *peaks_dev,
                        int32_t n_peaks, void *stream) {
    MI_REQUIRE(table_dev && bank_dev && peaks_dev && n_rows > 0 && n_rows <= 65535 && max_n >= 1 &&
               max_n <= (int64_t)INT32_MAX * 1024 && n_sources > 0 && n_sources <= MI_MIX_MAX_SOURCES && channels > 0 &&
               channels <= 65535 && phases >= 1 && phases <= MI_TP_MAX_PHASES && taps >= 1 && taps <= MI_TP_MAX_TAPS &&
               hist_capacity >= 0 && (hist_dev || hist_capacity == 0) && n_peaks > 0 && n_peaks <= INT32_MAX / 2,
               "mi_true_peak_update: bad argument");
    return launch_true_peak_update(table_dev, n_rows, max_n, n_sources, channels, bank_dev, phases, taps, hist_dev, hist_capacity,
                                   (unsigned *)peaks_dev, n_peaks, (hipStream_t)stream);
}

// Kernel-level entry points.  They allocate their scratch with hipMalloc and free it after a
// stream synchronise: convenient for parity tests, not meant for the hot loop.
int mi_stft_cac(const float *mix_dev, int32_t B, int32_t L, float *cac_dev, void *stream) {
    MI_REQUIRE(mix_dev && cac_dev && B > 0 && B <= 16383 && L >= 1, "mi_stft_cac: bad argument");
    return stft_entry("mi_stft_cac", mix_dev, B, L, cac_dev, 0, nullptr, nullptr, (hipStream_t)stream);
}

int mi_stft_norm(const float *mix_dev, int32_t B, int32_t L, float *x_dev, int32_t x_pitch, float *norm_dev, float *denorm_dev, void *stream) {
    MI_REQUIRE(mix_dev && x_dev && norm_dev && denorm_dev, "mi_stft_norm: null argument");
    MI_REQUIRE(B >= 1 && B <= 16383, "mi_stft_norm: B = %d outside [1, 16383] (the transpose's grid holds 4 B planes)", B);
    MI_REQUIRE(L >= 1, "mi_stft_norm: L = %d, at least one sample", L);
    const int T = (L + 1023) / 1024;
    MI_REQUIRE(x_pitch == 0 || x_pitch >= T, "mi_stft_norm: row pitch %d below T = %d", x_pitch, T);
    return stft_entry("mi_stft_norm", mix_dev, B, L, x_dev, x_pitch, norm_dev, denorm_dev, (hipStream_t)stream);
}

int mi_istft_full(const float *y_dev, int32_t B, int32_t S, int32_t L, int32_t y_pitch, const float *denorm_f_dev, const float *xt_dev,
                  int32_t xt_pitch, const float *denorm_t_dev, float *wav_dev, void *stream) {
    MI_REQUIRE(y_dev && wav_dev, "mi_istft_full: null argument");
    MI_REQUIRE(B >= 1 && S >= 1 && (int64_t)B * S <= 16383, "mi_istft_full: B = %d, S = %d: 1 <= B S <= 16383 (the transpose's grid holds 4 B S planes)",
               B, S);
    MI_REQUIRE(L >= 1, "mi_istft_full: L = %d, at least one sample", L);
    const int T = (L + 1023) / 1024;
    MI_REQUIRE(y_pitch == 0 || y_pitch >= T, "mi_istft_full: spectrogram row pitch %d below T = %d", y_pitch, T);
    MI_REQUIRE((xt_dev != nullptr) == (denorm_t_dev != nullptr), "mi_istft_full: xt_dev and denorm_t_dev go together");
    MI_REQUIRE(xt_pitch == 0 || xt_pitch >= L, "mi_istft_full: time-branch row pitch %d below L = %d", xt_pitch, L);
    FftTables tb;
    MI_TRY(get_tables(&tb));
    TestScratch ws;
    float *yt = nullptr, *fr = nullptr;
    MI_TRY(ws.get((size_t)B * S * T * 4 * 2048, &yt));
    MI_TRY(ws.get((size_t)B * S * T * 2 * 4096, &fr));
    hipStream_t st = (hipStream_t)stream;
    const int r = launch_istft(y_dev, B, S, L, (const float2 *)denorm_f_dev, xt_dev, (const float2 *)denorm_t_dev, tb, yt, fr, wav_dev, st,
                               xt_pitch, y_pitch);
    return finish_entry(r, st, "mi_istft_full");
}

int mi_istft_cac(const float *x_dev, int32_t B, int32_t S, int32_t L, float *wav_dev, void *stream) {
    MI_REQUIRE(x_dev && wav_dev && B > 0 && S > 0 && (int64_t)B * S <= 16383 && L >= 1, "mi_istft_cac: bad argument");
    return mi_istft_full(x_dev, B, S, L, 0, nullptr, nullptr, 0, nullptr, wav_dev, stream);
}

// the per-item normalisation of the waveform (Model::forward): row_stats -> finalize mode 1 -> row_affine
int mi_item_norm(const float *x_dev, int32_t rows, int64_t count, float *y_dev, float *norm_dev, float *denorm_dev, void *stream) {
    MI_REQUIRE(x_dev && y_dev && norm_dev && denorm_dev, "mi_item_norm: null argument");
    MI_REQUIRE(rows >= 1 && rows <= 65535, "mi_item_norm: rows = %d outside [1, 65535] (the grid's y range)", rows);
    MI_REQUIRE(count >= 2, "mi_item_norm: count = %lld: the unbiased std divides by count - 1", (long long)count);
    TestScratch ws;
    double *stats = nullptr;
    MI_TRY(ws.get((size_t)2 * kStatSlots * rows, &stats));
    hipStream_t st = (hipStream_t)stream;
    MI_HIP(hipMemsetAsync(stats, 0, sizeof(double) * 2 * kStatSlots * rows, st));
    int r = launch_row_stats(x_dev, rows, count, count, stats, st);
    if (r == MI_OK) r = launch_finalize_stats(stats, rows, (double)count, 1e-5f, 1, (float2 *)norm_dev, (float2 *)denorm_dev, st);
    if (r == MI_OK) r = launch_row_affine(x_dev, rows, count, (const float2 *)norm_dev, y_dev, st);
    return finish_entry(r, st, "mi_item_norm");
}

int mi_item_denorm(const float *x_dev, int32_t rows, int64_t count, const float *denorm_dev, float *y_dev, void *stream) {
    MI_REQUIRE(x_dev && denorm_dev && y_dev, "mi_item_denorm: null argument");
    MI_REQUIRE(rows >= 1 && rows <= 65535 && count >= 1, "mi_item_denorm: rows = %d outside [1, 65535] or count = %lld < 1", rows, (long long)count);
    return launch_row_denorm(x_dev, rows, count, (const float2 *)denorm_dev, y_dev, (hipStream_t)stream);
}

int mi_conv_forward(const struct mi_conv_desc *desc, void *stream) {
    MI_REQUIRE(desc, "mi_conv_forward: null descriptor");
    // a loader that reads past the ends of x gets a copy with slack when the caller's allocation has none (conv_owns_slack)
    if (desc->x && desc->B > 0 && desc->x_bstride > 0 && conv_check_tile_m(*desc) == MI_OK && conv_reads_slack(conv_route(*desc).route)) {
        const size_t bytes = (size_t)desc->B * (size_t)desc->x_bstride * sizeof(float);
        if (!conv_owns_slack(desc->x, bytes)) return conv_forward_staged(*desc, bytes, (hipStream_t)stream);
    }
    return launch_conv(*desc, (hipStream_t)stream);
}

int mi_resample_frac(const float *x_dev, int32_t rows, int64_t length, const float *table_dev, int32_t old_sr, int32_t new_sr,
                     int32_t width, float *y_dev, int64_t out_length, void *stream) {
    MI_REQUIRE(x_dev && table_dev && y_dev && old_sr > 0 && new_sr > 0 && width > 0, "mi_resample_frac: bad argument");
    return launch_resample_frac(x_dev, rows, length, table_dev, old_sr, new_sr, width, y_dev, out_length, (hipStream_t)stream);
}

int mi_conv_pack_split(const float *wt_dev, int32_t Kpad, int32_t Mpad, int32_t tile_m, void *wx_dev, void *stream) {
    MI_REQUIRE(wt_dev && wx_dev && Kpad > 0 && Mpad > 0 && (conv_x6_supported(tile_m) || tile_m == 192), "mi_conv_pack_split: bad argument");
    MI_REQUIRE(tile_m != 192 || Mpad % 192 == 0, "mi_conv_pack_split: tile_m 192 needs Mpad %% 192 == 0 (Mpad %d)", Mpad);
    // a 192-row layer's image is the 96-row layout: the 192-row tile reads the images of M tiles 2 mt and 2 mt + 1
    return launch_pack_split(wt_dev, Kpad, Mpad, tile_m == 192 ? 96 : tile_m, wx_dev, (hipStream_t)stream);
}

int mi_conv_pack_tap(const float *wt_dev, int32_t Mpad, int32_t Cin, int32_t ntaps, int32_t dtype, void *wtap_dev, void *stream) {
    MI_REQUIRE(wt_dev && wtap_dev && Mpad > 0 && Cin > 0 && ntaps > 0, "mi_conv_pack_tap: bad argument");
    return launch_pack_tap(wt_dev, Mpad, Cin, ntaps, dtype, wtap_dev, (hipStream_t)stream);
}

int mi_f32_to_image(const float *x_dev, int32_t B, int32_t C, int64_t P, int32_t dtype, void *img_dev, void *stream) {
    MI_REQUIRE(x_dev && img_dev && B > 0 && C > 0 && P > 0, "mi_f32_to_image: bad argument");
    return launch_f32_to_image(x_dev, B, C, P, dtype, img_dev, (hipStream_t)stream);
}

int mi_conv_pack_half(const float *wt_dev, int32_t Kpad, int32_t Mpad, int32_t dtype, void *wh_dev, void *stream) {
    MI_REQUIRE(wt_dev && wh_dev && Kpad > 0 && Mpad > 0, "mi_conv_pack_half: bad argument");
    return launch_pack_half(wt_dev, Kpad, Mpad, dtype, wh_dev, (hipStream_t)stream);
}

int mi_attention(const float *q_dev, const float *k_dev, const float *v_dev, float *o_dev, int32_t B, int32_t heads, int32_t Tq,
                 int32_t Tk, int64_t q_batch_stride, int64_t kv_batch_stride, int64_t o_batch_stride, int32_t dtype, void *stream) {
    MI_REQUIRE(q_dev && k_dev && v_dev && o_dev && B > 0 && heads > 0 && Tq > 0 && Tk > 0, "mi_attention: bad argument");
    return launch_attention(q_dev, k_dev, v_dev, o_dev, B, heads, Tq, Tk, q_batch_stride, kv_batch_stride, o_batch_stride, dtype,
                            (hipStream_t)stream);
}

int mi_attention_split(const float *q_dev, const float *k_dev, const float *v_dev, float *o_dev, int32_t B, int32_t heads, int32_t Tq,
                       int32_t Tk, int64_t q_batch_stride, int64_t kv_batch_stride, int64_t o_batch_stride, void *stream) {
    MI_REQUIRE(q_dev && k_dev && v_dev && o_dev && B > 0 && heads > 0 && Tq > 0 && Tk > 0, "mi_attention_split: bad argument");
    return launch_attention_x6(q_dev, k_dev, v_dev, o_dev, B, heads, Tq, Tk, q_batch_stride, kv_batch_stride, o_batch_stride,
                               (hipStream_t)stream);
}

int mi_attention_heads(const void *q_dev, const void *k_dev, const void *v_dev, float *o_dev, int32_t B, int32_t heads, int32_t Tq, int32_t Tk,
                       int32_t Tq_pitch, int32_t Tk_pitch, int32_t dtype, void *stream) {
    MI_REQUIRE(q_dev && k_dev && v_dev && o_dev && B > 0 && heads > 0 && Tq > 0 && Tk > 0, "mi_attention_heads: bad argument");
    const void *zero = conv_zero_page();
    MI_REQUIRE(zero, "mi_attention_heads: could not allocate the zero page");
    return launch_attention_heads(q_dev, k_dev, v_dev, zero, B, heads, Tq, Tk, Tq_pitch, Tk_pitch, dtype, nullptr, 0, o_dev,
                                  (int64_t)heads * 64 * Tq, (hipStream_t)stream);
}

int mi_attention_heads_image(const void *q_dev, const void *k_dev, const void *v_dev, void *img_dev, int64_t n_img, int32_t B, int32_t heads,
                             int32_t Tq, int32_t Tk, int32_t Tq_pitch, int32_t Tk_pitch, int32_t dtype, void *stream) {
    MI_REQUIRE(q_dev && k_dev && v_dev && img_dev && B > 0 && heads > 0 && Tq > 0 && Tk > 0, "mi_attention_heads_image: bad argument");
    const void *zero = conv_zero_page();
    MI_REQUIRE(zero, "mi_attention_heads_image: could not allocate the zero page");
    return launch_attention_heads(q_dev, k_dev, v_dev, zero, B, heads, Tq, Tk, Tq_pitch, Tk_pitch, dtype, img_dev, n_img, nullptr, 0,
                                  (hipStream_t)stream);
}

int mi_attention_image(const float *q_dev, const float *k_dev, const float *v_dev, void *img_dev, int64_t n_img, int32_t B,
                       int32_t heads, int32_t Tq, int32_t Tk, int64_t q_batch_stride, int64_t kv_batch_stride, int32_t dtype,
                       void *stream) {
    MI_REQUIRE(q_dev && k_dev && v_dev && img_dev && B > 0 && heads > 0 && Tq > 0 && Tk > 0, "mi_attention_image: bad argument");
    MI_REQUIRE(dtype == MI_DTYPE_BF16 || dtype == MI_DTYPE_F16, "mi_attention_image: dtype %d is not a half mode", dtype);
    return launch_attention(q_dev, k_dev, v_dev, nullptr, B, heads, Tq, Tk, q_batch_stride, kv_batch_stride, 0, dtype,
                            (hipStream_t)stream, img_dev, n_img);
}

int mi_gn_gelu(float *x_dev, int32_t B, int32_t C, int32_t C_alloc, int32_t D1, int32_t D2, int32_t row_mode, const float *stats_dev,
               const float *w_dev, const float *b_dev, void *stream) {
    MI_REQUIRE(x_dev && stats_dev && w_dev && b_dev && B > 0 && C > 0 && D1 > 0 && D2 > 0, "mi_gn_gelu: bad argument");
    MI_REQUIRE(C_alloc >= C, "mi_gn_gelu: C_alloc < C");
    return launch_gn_gelu(x_dev, B, C, C_alloc, D1, D2, row_mode, (const float2 *)stats_dev, w_dev, b_dev, (hipStream_t)stream);
}

int32_t mi_gram_order(int32_t h) { return gram_hp(h); }

int mi_lstm_seq(const float *gx_dev, const float *whh_host, int32_t N, int32_t H, int32_t W, float *out_dev, int32_t mode, void *stream) {
    MI_REQUIRE(mode == 0 || mode == 1 || mode == 2, "mi_lstm_seq: mode 0 (one launch per step), 1 (persistent kernel) or 2 (generic small kernel)");
    hipStream_t st = (hipStream_t)stream;
    if (mode == 2) {                 // the generic kernel reads W_hh in its natural order: upload, launch, wait
        MI_REQUIRE(gx_dev && whh_host && out_dev && N > 0 && N <= 65535 && W > 0 && H >= 1 && H <= 64,
                   "mi_lstm_seq: bad argument (mode 2 needs 1 <= H <= 64)");
        const size_t bytes = (size_t)2 * 4 * H * H * sizeof(float);
        float *wn = nullptr;
        MI_HIP(hipMalloc((void **)&wn, bytes));
        int rs = MI_OK;
        if (hipMemcpyAsync(wn, whh_host, bytes, hipMemcpyHostToDevice, st) != hipSuccess) rs = set_error(MI_EHIP, "mi_lstm_seq: hipMemcpyAsync failed");
        if (rs == MI_OK) rs = launch_lstm_small(gx_dev, wn, N, H, W, out_dev, st);
        const hipError_t es = hipStreamSynchronize(st);
        if (es != hipSuccess && rs == MI_OK) rs = set_error(MI_EHIP, "mi_lstm_seq: hipStreamSynchronize: %s", hipGetErrorString(es));
        (void)hipFree(wn);
        return rs;
    }
    MI_REQUIRE(gx_dev && whh_host && out_dev && N > 0 && W > 0 && (H == 192 || H == 384), "mi_lstm_seq: bad argument (H must be 192 or 384)");
    std::vector<float> packed((size_t)2 * 4 * H * H);
    pack_lstm_whh(whh_host, H, packed.data());
    float *wd = nullptr, *state = nullptr;
    void *scratch = nullptr;
    unsigned *flag = nullptr;
    int r = MI_OK;
    auto fail = [&](hipError_t e, const char *what) { if (e != hipSuccess && r == MI_OK) r = set_error(MI_EHIP, "mi_lstm_seq: %s: %s", what, hipGetErrorString(e)); };
    fail(hipMalloc((void **)&wd, packed.size() * sizeof(float)), "hipMalloc");
    fail(hipMalloc((void **)&state, (size_t)6 * N * H * sizeof(float)), "hipMalloc");
    fail(hipMalloc(&scratch, lstm_persist_scratch_bytes()), "hipMalloc");
    fail(hipHostMalloc((void **)&flag, 64, hipHostMallocMapped), "hipHostMalloc");
    if (r == MI_OK) {
        *flag = 0;
        fail(hipMemcpyAsync(wd, packed.data(), packed.size() * sizeof(float), hipMemcpyHostToDevice, st), "hipMemcpyAsync");
        if (r == MI_OK) r = mode ? launch_lstm_persist(gx_dev, wd, N, H, W, out_dev, scratch, flag, st) : launch_lstm_seq(gx_dev, wd, N, H, W, out_dev, state, st);
        fail(hipStreamSynchronize(st), "hipStreamSynchronize");
        if (r == MI_OK && *(volatile unsigned *)flag) r = set_error(MI_EHIP, "mi_lstm_seq: the persistent kernel timed out waiting for its hidden-state exchange");
        if (r == MI_OK && mode && switches().lstm_debug) {
                        unsigned dbg[16] = {};
            (void)hipMemcpy(dbg, (char *)scratch + lstm_persist_ctl_offset(), sizeof(dbg), hipMemcpyDeviceToHost);
            fprintf(stderr, "[lstm] H %d N %d W %d: block 0 / wave 1 spent %.1f us gathering h in %u poll passes (%.2f us, %.2f passes per step); "
                    "%s stores\n", H, N, W, dbg[2] * 0.01, dbg[3], dbg[2] * 0.01 / std::max(1, W - 1), (double)dbg[3] / std::max(1, W - 1),
                    dbg[4] ? "same-XCD plain" : "write-through");
            fprintf(stderr, "[lstm]   shader cycles per step: gather %.0f, issue + products %.0f, LDS write + barrier %.0f, gate stage %.0f; whole step %.0f\n",
                    (double)dbg[8] / W, (double)dbg[9] / W, (double)dbg[10] / W, (double)dbg[11] / W, (double)dbg[12] / W);
        }
    }
    if (wd) (void)hipFree(wd);
    if (state) (void)hipFree(state);
    if (scratch) (void)hipFree(scratch);
    if (flag) (void)hipHostFree(flag);
    return r;
}

int mi_gn_gelu_gram(float *x_dev, int32_t B, int32_t h, int32_t C_alloc, int32_t D1, int32_t D2, int32_t pitch, int32_t row_mode,
                    const float *stats_dev, const float *w_dev, const float *b_dev, double *gram_dev, int32_t slots, void *stream) {
    MI_REQUIRE(x_dev && stats_dev && w_dev && b_dev && gram_dev && B > 0 && h > 0 && D1 > 0 && D2 > 0 && slots > 0, "mi_gn_gelu_gram: bad argument");
    MI_REQUIRE(C_alloc >= h && pitch >= D2, "mi_gn_gelu_gram: C_alloc < h or pitch < D2");
    return launch_gn_gelu_gram(x_dev, B, h, C_alloc, D1, D2, pitch, row_mode, (const float2 *)stats_dev, w_dev, b_dev, gram_dev, slots,
                               false, (hipStream_t)stream);
}

int mi_dconv_gn_gelu_gram(float *x_dev, int32_t B, int32_t h, int32_t C_alloc, int32_t D1, int32_t D2, int32_t pitch, int32_t row_mode,
                          const float *stats_dev, const float *w_dev, const float *b_dev, double *gram_dev, int32_t slots, void *stream) {
    MI_REQUIRE(x_dev && stats_dev && w_dev && b_dev && gram_dev && B > 0 && h > 0 && D1 > 0 && D2 > 0 && slots > 0, "mi_dconv_gn_gelu_gram: bad argument");
    MI_REQUIRE(C_alloc >= h && C_alloc <= gram_hp(h) && pitch >= D2, "mi_dconv_gn_gelu_gram: C_alloc outside [h, mi_gram_order(h)] or pitch < D2");
    return launch_gn_gelu_gram(x_dev, B, h, C_alloc, D1, D2, pitch, row_mode, (const float2 *)stats_dev, w_dev, b_dev, gram_dev, slots,
                               true, (hipStream_t)stream);
}

int mi_gram_finalize(double *gram_dev, int32_t rows, int32_t h, int32_t slots, const double *wt_dev, const double *ct_dev, double sum_b,
                     double sum_bsq, double cols, double count, float eps, float *stats_out_dev, void *stream) {
    MI_REQUIRE(gram_dev && wt_dev && ct_dev && stats_out_dev && rows > 0 && h > 0 && slots > 0 && count > 0.0, "mi_gram_finalize: bad argument");
    return launch_gram_finalize(gram_dev, rows, h, slots, wt_dev, ct_dev, sum_b, sum_bsq, cols, count, eps, (float2 *)stats_out_dev,
                                (hipStream_t)stream);
}

int mi_layernorm_cf(const float *x_dev, int32_t B, int32_t C, int32_t T, const float *w_dev, const float *b_dev,
                    const float *add_dev, float *y_dev, void *stream) {
    MI_REQUIRE(x_dev && w_dev && b_dev && y_dev, "mi_layernorm_cf: null argument");
    return launch_layernorm_cf(x_dev, B, C, T, w_dev, b_dev, add_dev, y_dev, nullptr, (hipStream_t)stream);
}

// ---- test entries of the hdemucs_mmi kernels (hkernels.hip) and of the token kernel (norms.hip): argument checks + the launcher
int mi_token_norm(int32_t mode, const float *x_dev, int32_t B, int32_t C, int32_t T, const float *w_dev, const float *b_dev,
                  const float *pe_dev, const float *gstat_dev, float *y_dev, float *ostat_dev, void *img_dev, int64_t img_n,
                  int32_t img_dtype, void *stream) {
    MI_REQUIRE(mode >= 0 && mode <= 2, "mi_token_norm: mode %d (0 LayerNorm, 1 statistics, 2 GroupNorm(1) apply)", mode);
    MI_REQUIRE(x_dev && B > 0 && B <= 65535 && C > 0 && T > 0, "mi_token_norm: bad argument");
    hipStream_t st = (hipStream_t)stream;
    if (mode == 1) {
        MI_REQUIRE(ostat_dev, "mi_token_norm: mode 1 writes only the statistics, ostat_dev is NULL");
        return launch_token_stats(x_dev, B, C, T, (float2 *)ostat_dev, st, img_dev, img_n, img_dtype);
    }
    MI_REQUIRE(w_dev && b_dev && y_dev, "mi_token_norm: mode %d needs w_dev, b_dev and y_dev", mode);
    if (mode == 0) return launch_layernorm_cf(x_dev, B, C, T, w_dev, b_dev, pe_dev, y_dev, (float2 *)ostat_dev, st, img_dev, img_n, img_dtype);
    MI_REQUIRE(gstat_dev, "mi_token_norm: mode 2 needs gstat_dev");
    return launch_gn_apply_tokstats(x_dev, B, C, T, (const float2 *)gstat_dev, w_dev, b_dev, y_dev, (float2 *)ostat_dev, st, img_dev, img_n,
                                    img_dtype);
}

int mi_local_attn(const float *qkc_dev, int32_t B, int32_t C, int32_t T, int32_t ld, float *out_dev, int32_t ld_o, void *stream) {
    MI_REQUIRE(qkc_dev && out_dev && B > 0 && B <= 65535 && C > 0 && T > 0, "mi_local_attn: bad argument");
    MI_REQUIRE(ld_o >= T, "mi_local_attn: output pitch %d < T = %d", ld_o, T);
    return launch_local_attn(qkc_dev, B, C, T, ld, out_dev, ld_o, (hipStream_t)stream);
}

int mi_group_norm_apply(const float *x_dev, int32_t B, int32_t Cin, int32_t G, int32_t in_pitch, int32_t in_len, int32_t off,
                        const float *w_dev, const float *b_dev, int32_t glu, int32_t gelu, const float *scale_dev, const float *res_dev,
                        int32_t res_pitch, float *y_dev, int32_t Cout, int32_t out_len, int32_t out_pitch, int32_t chan_div,
                        double *stats_ws_dev, float *stats_out_dev, void *stream) {
    MI_REQUIRE(x_dev && w_dev && b_dev && y_dev && stats_ws_dev && stats_out_dev, "mi_group_norm_apply: null argument");
    MI_REQUIRE(B > 0 && B <= 65535 && Cin > 0 && G > 0 && (int64_t)B * G <= 65535 && Cin % G == 0 && Cout > 0 && Cout <= 65535 && in_len > 0 && out_len > 0 &&
               chan_div >= 1 && Cin % chan_div == 0, "mi_group_norm_apply: bad sizes");
    MI_REQUIRE(in_pitch == in_len, "mi_group_norm_apply: statistics need contiguous channel rows (in_pitch %d != in_len %d)", in_pitch, in_len);
    MI_REQUIRE(off >= 0 && (int64_t)off + out_len <= in_len, "mi_group_norm_apply: window [%d, %d + %d) outside the %d input columns", off, off,
               out_len, in_len);
    MI_REQUIRE(out_pitch >= out_len && (!res_dev || res_pitch >= out_len), "mi_group_norm_apply: a row pitch below out_len = %d", out_len);
    hipStream_t st = (hipStream_t)stream;
    const int64_t cnt = (int64_t)(Cin / G) * in_len;
    MI_TRY(launch_row_stats(x_dev, B * G, cnt, cnt, stats_ws_dev, st));
    MI_TRY(launch_finalize_stats(stats_ws_dev, B * G, (double)cnt, 1e-5f, 0, (float2 *)stats_out_dev, nullptr, st));
    return launch_gn_apply(x_dev, B, Cin, G, in_pitch, off, (const float2 *)stats_out_dev, w_dev, b_dev, glu ? 1 : 0, gelu ? 1 : 0, scale_dev,
                           res_dev, res_pitch, y_dev, Cout, out_len, out_pitch, st, chan_div);
}

int mi_blstm_unfold(const float *x_dev, int32_t B, int32_t C, int32_t T, int32_t F, int32_t W, int32_t S, float *frames_dev, void *stream) {
    MI_REQUIRE(x_dev && frames_dev && B > 0 && C > 0 && C <= 65535 && T > 0 && F > 0 && (int64_t)B * F <= 65535 && W > 0 && S > 0,
               "mi_blstm_unfold: bad argument");
    return launch_unfold_frames(x_dev, B, C, T, F, W, S, frames_dev, (hipStream_t)stream);
}

int mi_blstm_restitch(const float *frames_dev, int32_t B, int32_t C, int32_t T, int32_t F, int32_t W, int32_t S, const float *skip_dev,
                      float *y_dev, void *stream) {
    MI_REQUIRE(frames_dev && y_dev && B > 0 && B <= 65535 && C > 0 && C <= 65535 && T > 0 && F > 0 && W > 0 && S > 0,
               "mi_blstm_restitch: bad argument");
    const int64_t per = (int64_t)W - 2 * (S / 2);
    MI_REQUIRE(per > 0 && T <= W + (F - 1) * per, "mi_blstm_restitch: %d frames of %d columns every %d do not cover T = %d", F, W, S, T);
    return launch_restitch_frames(frames_dev, B, C, T, F, W, S, skip_dev, y_dev, (hipStream_t)stream);
}

int mi_row_affine_pitch(const float *x_dev, int32_t B, int32_t C, int32_t L, int32_t out_pitch, const float *norm_dev, float *y_dev,
                        void *stream) {
    MI_REQUIRE(x_dev && norm_dev && y_dev && B > 0 && C > 0 && (int64_t)B * C <= 65535 && L > 0 && out_pitch >= L,
               "mi_row_affine_pitch: bad argument");
    return launch_row_affine_pitch(x_dev, B, C, L, out_pitch, (const float2 *)norm_dev, y_dev, (hipStream_t)stream);
}

// ---- test entries of the fused DConv kernels (dconv_row.hip, dconv_time.hip): argument checks, the engine's packing, the launcher
int mi_dconv_row(const float *x_dev, float *y_dev, int32_t B, int32_t C, int32_t Fr, int32_t T, const float *weights_host, int32_t variant,
                 void *stream) {
    MI_REQUIRE(x_dev && y_dev && weights_host && B > 0 && Fr > 0 && (int64_t)B * Fr <= (1 << 24), "mi_dconv_row: bad argument");
    MI_REQUIRE(((uintptr_t)x_dev & 7) == 0 && ((uintptr_t)y_dev & 7) == 0, "mi_dconv_row: tensors must be 8-byte aligned");
    MI_REQUIRE(dconv_row_supported(C, T), "mi_dconv_row: C = %d must be 48 or 96, T = %d a multiple of 6 up to 384", C, T);
    MI_REQUIRE(variant == 0 || variant == 1, "mi_dconv_row: variant 0 (one wave per row) or 1 (LDS-resident row)");
    MI_REQUIRE(variant == 0 || dconv_row_lds_supported(C, T), "mi_dconv_row: the LDS-resident kernel does not take C = %d, T = %d", C, T);
    const int64_t n = (int64_t)B * C * Fr * T;
    MI_REQUIRE(x_dev == y_dev || x_dev + n <= y_dev || y_dev + n <= x_dev, "mi_dconv_row: y must be x itself or not overlap it");
    DConvTestLayer l0, l1;
    MI_TRY(l0.init(C, weights_host));
    MI_TRY(l1.init(C, weights_host + dconv_layer_floats(C)));
    hipStream_t st = (hipStream_t)stream;
    const DConvRowArgs a{{l0.l, l1.l}, x_dev, y_dev, Fr, T};
    int r = launch_dconv_row(a, C, B * Fr, variant == 1, st);
    const hipError_t e = hipStreamSynchronize(st);           // the weights are freed on return
    if (e != hipSuccess && r == MI_OK) r = set_error(MI_EHIP, "mi_dconv_row: hipStreamSynchronize: %s", hipGetErrorString(e));
    return r;
}

int mi_dconv_time_layer(const float *x_dev, float *y_dev, int32_t B, int32_t C, int32_t Lv, int32_t Lp, int32_t dil,
                        const float *weights_host, float *hbuf_dev, double *stats_dev, double *gram_dev, float *st_dev, void *stream) {
    MI_REQUIRE(x_dev && y_dev && weights_host && hbuf_dev && stats_dev && gram_dev && st_dev, "mi_dconv_time_layer: null argument");
    MI_REQUIRE(B >= 1 && B <= 65535, "mi_dconv_time_layer: B = %d outside [1, 65535] (the grid's y range)", B);
    MI_REQUIRE(dconv_time_supported(C, Lp) && Lv >= 1 && Lp >= Lv, "mi_dconv_time_layer: C = %d must be 48 or 96, Lp = %d even and >= Lv = %d >= 1",
               C, Lp, Lv);
    MI_REQUIRE(dil == 1 || dil == 2, "mi_dconv_time_layer: dilation %d (1 or 2)", dil);
    MI_REQUIRE((((uintptr_t)x_dev | (uintptr_t)y_dev | (uintptr_t)hbuf_dev | (uintptr_t)stats_dev | (uintptr_t)gram_dev | (uintptr_t)st_dev) & 7) == 0,
               "mi_dconv_time_layer: buffers must be 8-byte aligned");
    const int64_t n = (int64_t)B * C * Lp;
    MI_REQUIRE(x_dev + n <= y_dev || y_dev + n <= x_dev, "mi_dconv_time_layer: y must not overlap x");
    DConvTestLayer l;
    MI_TRY(l.init(C, weights_host));
    hipStream_t st = (hipStream_t)stream;
    float2 *st1 = (float2 *)st_dev;
    int r = launch_dconv_time_layer(l.l, C, dil, B, Lv, Lp, x_dev, y_dev, hbuf_dev, stats_dev, gram_dev, st1, st1 + B, st);
    const hipError_t e = hipStreamSynchronize(st);           // the weights are freed on return
    if (e != hipSuccess && r == MI_OK) r = set_error(MI_EHIP, "mi_dconv_time_layer: hipStreamSynchronize: %s", hipGetErrorString(e));
    return r;
}

}  // extern "C"
