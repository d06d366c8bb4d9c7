// What the two engines (model.hip: htdemucs family; hmodel.hip: Hybrid Demucs v3) share: device memory, the profiler and the
// conv launcher, the side stream, weight lookup and packing, gather tables, activation-tensor geometry and the DConv block.
#pragma once
#include <algorithm>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "common.h"
#include "gemm_conv.h"
#include "kernels.h"

namespace mi {

extern int g_two_streams;      // engine_core.hip: 1 = waveform branch on a side stream (default), 0 = everything on the caller's stream

// Device allocations of one owner (an engine's weights and tables, a workspace): freed one by one or with the owner
struct DeviceArena {
    int64_t bytes = 0;                       // device bytes held, each allocation rounded up to 256
    DeviceArena() = default;
    DeviceArena(const DeviceArena &) = delete;
    DeviceArena &operator=(const DeviceArena &) = delete;
    int alloc(void **p, size_t n);
    void release(void *p);                   // p: a pointer alloc() returned (hipFree waits for the device)
    ~DeviceArena();

   private:
    std::map<void *, size_t> sizes;
};

struct PackedConv {
    float *wt = nullptr, *bias = nullptr;
    void *wx = nullptr;            // split-bf16 tile image of wt (gemm_x6.hip) when the tile has that main loop; tile == 192: 96-row images
    void *wh = nullptr;            // bf16 / fp16 operand image of wt (gemm_half.hip) in the reduced-precision modes
    void *wtap = nullptr;          // ... and, for k x k convs fed by an operand image, the tap-ordered image (gemm_tap.hip)
    int ntaps = 0;
    int M = 0, Mpad = 0, K = 0, Kpad = 0, tile = 0, half = 0;
};

struct DConvLayerW {
    PackedConv conv3, conv1;
    mi_ktab_entry *ktab3 = nullptr, *ktab1 = nullptr;
    float *gn1_w = nullptr, *gn1_b = nullptr, *gn2_w = nullptr, *gn2_b = nullptr, *ls = nullptr;
    // implicit-GEMM route: weights that turn the Gram accumulators of the hidden activations into the second GroupNorm's
    // statistics (norms.hip: gram_finalize_kernel)
    double *gram_wt = nullptr, *gram_ct = nullptr, sum_b = 0.0, sum_bsq = 0.0;
};
struct DConvW {
    DConvLayerW l[2];
    int h = 0;                     // hidden channels: C / 8 (htdemucs, dconv_comp 8) or C / 4 (hdemucs, dconv_comp 4)
    bool has_row = false;          // frequency-branch C = 48 / 96: fused LDS-resident row kernel
    DConvRowLayer row[2];
    bool has_time = false;         // time-branch C = 48 / 96: fused three-pass VALU kernels (dconv_time.hip)
    DConvTimeLayer tl[2];
};

// Per-kernel-class device timing with HIP events on the launch stream (bench.py's roofline leg).
struct ProfRow {
    int cls = 0;
    char name[48] = "";
    long long launches = 0;
    double ms = 0.0, flops = 0.0, bytes = 0.0;
};
struct Profiler {
    bool on = false;
    struct Pending { int cls; hipEvent_t a, b; double flops, bytes; long long launches = 1; };
    std::vector<Pending> pending;
    std::vector<hipEvent_t> pool;
    ProfRow rows[128];
    hipEvent_t get();
    // Runs fn (one launch, or `launches` of them timed as one span) between two events on its stream and books the span under
    // row `cls`; `name`, when given, names the row.  While the profiler is off: fn alone.
    template <typename Fn>
    int timed(int cls, const char *name, double flops, double bytes, hipStream_t st, Fn &&fn, long long launches = 1) {
        if (!on) return fn();
        Pending p{cls, get(), get(), flops, bytes, launches};
        MI_HIP(hipEventRecord(p.a, st));
        const int r = fn();
        MI_HIP(hipEventRecord(p.b, st));
        pending.push_back(p);
        if (name) snprintf(rows[cls].name, sizeof(rows[cls].name), "%s", name);
        return r;
    }
    void begin();
    int end(hipStream_t st);
    ~Profiler();
};

// Which layers get a split-bf16 weight image (pack_split), stated by the call that packs the layer.  MI_X6=0 gives none of them
// one, MI_X6=1 all of them; in between (the default) the float32 engine gives one to:
enum SplitScope {
    SPLIT_OPT_IN,      // no layer of this kind
    SPLIT_DEFAULT,     // the transformer linears and the decoders' 3 x 3 / k = 3 rewrite convs
    SPLIT_ROWS,        // the row-tap layers of the DMA row route: like SPLIT_DEFAULT, unless MI_NO_DMA_ROWS keeps them on the table routes
    SPLIT_TIME,        // the time branch's inner strided and transposed convs (route 11): like SPLIT_DEFAULT
};

struct WeightTable {
    std::map<std::string, std::pair<const float *, int64_t>> t;
    int get(const std::string &name, int64_t numel, const float **out) const {
        auto it = t.find(name);
        if (it == t.end()) return set_error(MI_EWEIGHT, "missing tensor '%s'", name.c_str());
        if (it->second.second != numel)
            return set_error(MI_EWEIGHT, "tensor '%s' has %lld elements, expected %lld", name.c_str(),
                             (long long)it->second.second, (long long)numel);
        *out = it->second.first;
        return MI_OK;
    }
};

static inline int round_up(int v, int m) { return (v + m - 1) / m * m; }

// geometry of one gather table
struct Gather {
    int Cin, K1, K2, dil1, dil2, pad1, pad2;
    int64_t chan_stride;
    int D2;
};

static inline std::vector<mi_ktab_entry> build_ktab(const Gather &g, int Kpad) {
    std::vector<mi_ktab_entry> tab(Kpad);
    const int K = g.Cin * g.K1 * g.K2;
    for (int k = 0; k < Kpad; ++k) {
        mi_ktab_entry e;
        if (k < K) {
            const int ci = k / (g.K1 * g.K2), r = k % (g.K1 * g.K2), k1 = r / g.K2, k2 = r % g.K2;
            e.d1 = k1 * g.dil1 - g.pad1;
            e.d2 = k2 * g.dil2 - g.pad2;
            e.off = (int32_t)(ci * g.chan_stride + (int64_t)e.d1 * g.D2 + e.d2);
            e.ci = ci;
        } else {                       // K padding: never valid (weights are zero there as well)
            e.d1 = -(1 << 29); e.d2 = -(1 << 29); e.off = 0; e.ci = 0;
        }
        tab[k] = e;
    }
    return tab;
}

struct Geo {          // geometry of one activation tensor family
    int B, D1, D2;    // batch, rows (freq bins or 1), columns (frames / samples)
    int row_mode;     // 1: DConv / GroupNorm rows are (b, d1) (frequency branch), 0: b
    int ld;           // row pitch in floats (>= D2, multiple of 4 when it differs): time-branch rows are padded
    int pitch() const { return ld ? ld : D2; }
};

static inline mi_conv_desc base_desc(const PackedConv &pc, const mi_ktab_entry *ktab, const float *x, int64_t x_bs, const Geo &g) {
    mi_conv_desc d;
    memset(&d, 0, sizeof(d));
    d.wt = pc.wt; d.M = pc.M; d.Mpad = pc.Mpad; d.K = pc.K; d.Kpad = pc.Kpad; d.ktab = ktab; d.bias = pc.bias; d.tile_m = pc.tile; d.wx = pc.wx;
    d.wh = pc.wh; d.half = pc.wh ? pc.half : 0; d.ktab_len = round_up(pc.Kpad, 32);
    d.x = x; d.x_bstride = x_bs; d.B = g.B; d.D1 = g.D1; d.D2 = g.D2; d.O1 = g.D1; d.O2 = g.pitch(); d.S1 = 1; d.S2 = 1;
    d.o2_valid = g.pitch() != g.D2 ? g.D2 : 0;       // enumerate the padded row, mask the padding columns
    d.x_ld = g.pitch() != g.D2 ? g.pitch() : 0;        // ... and the gather / plain loaders step rows by the pitch
    d.row_mode = g.row_mode;
    return d;
}

enum EngineKind { ENGINE_HTDEMUCS, ENGINE_HDEMUCS };

// The handle of the C interface points at this part of an engine: `kind` says which engine (Model, HModel) it belongs to
struct EngineCore {
    const EngineKind kind;
    mi_config cfg{};
    Profiler prof;
    int conv(const mi_conv_desc &d, hipStream_t st);
    DeviceArena weights;                    // packed weights, gather tables, FFT tables
    FftTables fft{};

    hipStream_t side_st = nullptr;          // the waveform branch's stream
    hipEvent_t ev_main = nullptr, ev_side = nullptr;
    int side_streams();

   protected:
    explicit EngineCore(EngineKind k) : kind(k) {}
    ~EngineCore();                           // engines are deleted as what they are (api.hip), never through this base
    template <typename T> int upload(const std::vector<T> &h, T **dptr) {
        void *p = nullptr;
        MI_TRY(weights.alloc(&p, std::max<size_t>(h.size(), 1) * sizeof(T)));
        MI_HIP(hipMemcpy(p, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice));
        *dptr = (T *)p;
        return MI_OK;
    }
    int upload_fft_tables();         // fills `fft`
    int pack_split(PackedConv *pc, SplitScope scope);
    int pack_half(PackedConv *pc);
    int pack_conv(const float *W, const float *bias, int M, int K, bool glu, PackedConv *pc, int ntaps = 0, SplitScope scope = SPLIT_OPT_IN);
    int pack_tap(PackedConv *pc, int ntaps);
    int pack_enc_tap(const float *W, int Cin, PackedConv *pc);
    int pack_convtr(const float *W, const float *bias, int Cin, int Cout, PackedConv *pc, int stride = 4, SplitScope scope = SPLIT_OPT_IN);
    int pack_vec(const float *v, int n, int npad, bool glu, float **out);
    int pack_linear_ln(const float *W, const float *bias, const float *ln_w, const float *ln_b, int M, int K, PackedConv *pc,
                       float **c1, SplitScope scope);
    int make_ktab(const Gather &g, int Kpad, mi_ktab_entry **out);
    int load_dconv(const WeightTable &wt, const std::string &prefix, int C, int64_t chan_stride, int D2, bool freq, DConvW *dw, int comp = 8);
    // run_dconv's scratch, set by the engine where it allocates it (zeroed; the kernels that use it leave it zeroed)
    double *dconv_gram = nullptr;            // time kernels (dconv_time.hip): needed when a layer has_time
    double *dconv_gram2 = nullptr;           // implicit-GEMM route: Gram accumulators (rows x slots x HP x HP float64) ...
    size_t dconv_gram2_bytes = 0;            // ... and their size
    bool dconv_tap_dma = false;  // run_dconv may state the k = 3 convs' geometry (DMA tap route): only when x / tmp carry 128 bytes of slack
    // (gram2, gram2_cap): the accumulators of a branch that runs beside the other one, in place of dconv_gram2
    int run_dconv(const DConvW &w, int C, const Geo &g, float *x, float *tmp, float *hidden, double *stats, float2 *st1, float2 *st2,
                  hipStream_t st, double *gram2 = nullptr, size_t gram2_cap = 0);
};

}  // namespace mi
