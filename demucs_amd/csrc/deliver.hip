// Delivery of the stems as the reference saves them (demucs/separate.py:178-218 through save_audio, demucs/audio.py:236-265):
// per output the `--two-stems` value, prevent_clip, i16_pcm (or float32) and the interleaving of channels per frame, for EVERY
// output of a call in one table-driven launch (include/demucs_amd.h, MI_DELIVER_*).  Both kernels are memory-bound elementwise
// passes; the arithmetic is post_ops.h's, shared with mi_prevent_clip / mi_two_stems, each step a separately rounded float32
// operation in the reference's order.  Nothing here synchronises with the host and there is no scratch.
#include "common.h"
#include "kernels.h"
#include "post_ops.h"
#include "deliver_io.h"

namespace mi {

struct DeliverRow {
    const float *src, *origin;
    int64_t n, dst_off;
    int kind, sel, clip, fmt, peak;
    bool ok, vec;
};

// One row of the table, with every rule under which it is skipped; every kernel reads a row through this, so they agree on it.
// DST = false is a row that writes no frames (mi_deliver_peaks_update): FMT and DST_OFF are not read, and dst_cap is not used
template <bool DST = true>
__device__ __forceinline__ DeliverRow deliver_row(const int64_t *__restrict__ t, int n_sources, int channels, int n_peaks, int64_t dst_cap) {
    DeliverRow r;
    r.src = reinterpret_cast<const float *>(static_cast<uintptr_t>(t[MI_DELIVER_SRC]));
    r.origin = reinterpret_cast<const float *>(static_cast<uintptr_t>(t[MI_DELIVER_ORIGIN]));
    r.n = t[MI_DELIVER_N];
    r.dst_off = DST ? t[MI_DELIVER_DST_OFF] : 0;
    const int64_t kind = t[MI_DELIVER_KIND], sel = t[MI_DELIVER_SEL], clip = t[MI_DELIVER_CLIP];
    const int64_t fmt = DST ? t[MI_DELIVER_FMT] : MI_DELIVER_I16;
    const int64_t peak = t[MI_DELIVER_PEAK];
    r.ok = r.src && r.n > 0 && kind >= MI_DELIVER_STEM && kind <= MI_DELIVER_MINUS && sel >= 0 && sel < n_sources && clip >= 0 &&
           clip <= MI_CLIP_TANH && fmt >= MI_DELIVER_I16 && fmt <= MI_DELIVER_F32 && (clip != MI_CLIP_RESCALE || (peak >= 0 && peak < n_peaks)) &&
           (kind != MI_DELIVER_MINUS || r.origin) && r.dst_off >= 0 && (r.dst_off & 3) == 0;
    r.kind = (int)kind; r.sel = (int)sel; r.clip = (int)clip; r.fmt = (int)fmt; r.peak = (int)peak;
    if (DST && r.ok) {
        const int64_t frame = (int64_t)channels * (r.fmt == MI_DELIVER_F32 ? 4 : 2);        // bytes
        r.ok = r.n <= dst_cap / frame && r.dst_off <= dst_cap - r.n * frame;
    }
    // 16-byte loads: every (source, channel) row starts at a multiple of 4 floats from an aligned base
    r.vec = (r.n & 3) == 0 && (reinterpret_cast<uintptr_t>(r.src) & 15) == 0 &&
            (r.kind != MI_DELIVER_MINUS || (reinterpret_cast<uintptr_t>(r.origin) & 15) == 0);
    return r;
}

// step 1, the value: frames j0 .. j0 + 3 of channel c of the row's output, before clipping
__device__ __forceinline__ void row_values(const DeliverRow &r, int n_sources, int channels, int c, int64_t j0, float (&v)[4]) {
    const int64_t stem_stride = (int64_t)channels * r.n;
    const float *base = r.src + (int64_t)c * r.n;                  // stem k's channel c at base + k * stem_stride
    if (r.kind == MI_DELIVER_STEM) {
        load4(base + r.sel * stem_stride, j0, r.n, r.vec, v);
    } else if (r.kind == MI_DELIVER_MINUS) {
        float o[4], s[4];
        load4(r.origin + (int64_t)c * r.n, j0, r.n, r.vec, o);
        load4(base + r.sel * stem_stride, j0, r.n, r.vec, s);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = two_stems_minus(o[e], s[e]);
    } else {
        two_stems_add<4>(n_sources, r.sel, [&](int k, float (&s)[4]) { load4(base + k * stem_stride, j0, r.n, r.vec, s); }, v);
    }
}

// mi_deliver_peaks (DST: the rows are those mi_deliver_pcm will write) and mi_deliver_peaks_update (no destination; the slots
// carry the running maximum): grid (ceil(max_n / 1024), n_rows); a thread takes four consecutive frames of every channel of its row
template <bool DST>
__global__ __launch_bounds__(256) void deliver_peaks_kernel(const int64_t *__restrict__ table, int n_sources, int channels,
                                                            unsigned *__restrict__ peaks, int n_peaks, int64_t dst_cap) {
    const DeliverRow r = deliver_row<DST>(table + (size_t)blockIdx.y * MI_DELIVER_COLS, n_sources, channels, n_peaks, dst_cap);
    if (!r.ok || r.clip != MI_CLIP_RESCALE) return;                // the same for the whole block
    const int64_t j0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
    deliver_peak4([&](int c, float (&v)[4]) { row_values(r, n_sources, channels, c, j0, v); }, channels, j0, r.n, peaks + r.peak);
}

// mi_deliver_pcm: the same grid and thread assignment; the stores are deliver_store4's
__global__ __launch_bounds__(256) void deliver_pcm_kernel(const int64_t *__restrict__ table, int n_sources, int channels,
                                                          const unsigned *__restrict__ peaks, int n_peaks, unsigned char *__restrict__ dst,
                                                          int64_t dst_cap) {
    const DeliverRow r = deliver_row(table + (size_t)blockIdx.y * MI_DELIVER_COLS, n_sources, channels, n_peaks, dst_cap);
    if (!r.ok) return;
    const int64_t j0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
    if (j0 >= r.n) return;
    const float d = r.clip == MI_CLIP_RESCALE ? clip_divisor(peaks[r.peak]) : 0.f;
    unsigned char *out = dst + r.dst_off;                          // frames [0, n) of the row: inside dst_cap by deliver_row
    deliver_store4([&](int c, float (&v)[4]) { row_values(r, n_sources, channels, c, j0, v); }, channels, j0, r.n, r.clip, d,
                   r.fmt == MI_DELIVER_I16, out);
}

int launch_deliver_peaks(const int64_t *table, int n_rows, int64_t max_n, int n_sources, int channels, unsigned *peaks, int n_peaks,
                         int64_t dst_cap, hipStream_t st) {
    MI_HIP(hipMemsetAsync(peaks, 0, sizeof(unsigned) * (size_t)n_peaks, st));
    hipLaunchKernelGGL(deliver_peaks_kernel<true>, dim3(ceil_div(max_n, 1024), n_rows), dim3(256), 0, st, table, n_sources, channels,
                       peaks, n_peaks, dst_cap);
    MI_CHECK_LAUNCH();
    return MI_OK;
}

int launch_deliver_peaks_update(const int64_t *table, int n_rows, int64_t max_n, int n_sources, int channels, unsigned *peaks,
                                int n_peaks, hipStream_t st) {
    hipLaunchKernelGGL(deliver_peaks_kernel<false>, dim3(ceil_div(max_n, 1024), n_rows), dim3(256), 0, st, table, n_sources, channels,
                       peaks, n_peaks, (int64_t)0);
    MI_CHECK_LAUNCH();
    return MI_OK;
}

int launch_deliver_pcm(const int64_t *table, int n_rows, int64_t max_n, int n_sources, int channels, const unsigned *peaks, int n_peaks,
                       unsigned char *dst, int64_t dst_cap, hipStream_t st) {
    hipLaunchKernelGGL(deliver_pcm_kernel, dim3(ceil_div(max_n, 1024), n_rows), dim3(256), 0, st, table, n_sources, channels, peaks,
                       n_peaks, dst, dst_cap);
    MI_CHECK_LAUNCH();
    return MI_OK;
}

}  // namespace mi
