// Delivery of gain-weighted remixes of the stems and of the input mix (include/demucs_amd.h, MI_MIX_*): per output row
// post_ops.h's mix_values -- acc = 0, then + g_mix * mix and + g_k * stem k in index order, a term with a zero gain not read --
// followed by deliver.hip's prevent_clip, i16_pcm (or float32) and interleaving, for EVERY remix of a call in one launch.  The
// mix is read where a stream keeps it: a window whose row pitch is not N, holding the Separator's normalised samples, which are
// restored (w * s, then + mean) on the way in.  Memory-bound elementwise passes on deliver.hip's grid; nothing here synchronises
// with the host and no kernel uses scratch: the gains stay in the table and are read by uniform loads, never indexed in registers.
#include "common.h"
#include "kernels.h"
#include "post_ops.h"
#include "deliver_io.h"

namespace mi {

struct MixRow {
    const int64_t *t;                  // the row: the gains are read from it where they are used
    const float *src, *origin;
    int64_t n, pitch, dst_off;
    float mean, s;
    int clip, fmt, peak;
    bool ok, affine, vec, vec_origin;
};

// float32 i of the nine gains (0: the mix's, 1 + k: stem k's), two to an int64 from MI_MIX_GAINS, little-endian
__device__ __forceinline__ float mix_gain(const int64_t *__restrict__ t, int i) {
    return __uint_as_float((unsigned)((uint64_t)t[MI_MIX_GAINS + (i >> 1)] >> ((i & 1) * 32)));
}

// One row of the table, with every rule under which it is skipped; every kernel reads a row through this, so they agree on it.
// DST = false is a row that writes no frames (mi_deliver_mix_peaks_update): FMT and DST_OFF are not read, and dst_cap is not used
template <bool DST = true>
__device__ __forceinline__ MixRow mix_row(const int64_t *__restrict__ t, int n_sources, int channels, int n_peaks, int64_t dst_cap) {
    MixRow r;
    r.t = t;
    r.src = reinterpret_cast<const float *>(static_cast<uintptr_t>(t[MI_MIX_SRC]));
    r.origin = reinterpret_cast<const float *>(static_cast<uintptr_t>(t[MI_MIX_ORIGIN]));
    r.n = t[MI_MIX_N];
    r.pitch = t[MI_MIX_ORIGIN_PITCH];
    r.dst_off = DST ? t[MI_MIX_DST_OFF] : 0;
    const uint64_t aff = (uint64_t)t[MI_MIX_ORIGIN_AFFINE];
    r.mean = __uint_as_float((unsigned)aff);
    r.s = __uint_as_float((unsigned)(aff >> 32));
    r.affine = t[MI_MIX_AFFINE_ON] != 0;
    const int64_t clip = t[MI_MIX_CLIP], fmt = DST ? t[MI_MIX_FMT] : MI_DELIVER_I16, peak = t[MI_MIX_PEAK];
    bool finite = true, any = false;
    for (int i = 0; i <= n_sources; ++i) {
        const float g = mix_gain(t, i);
        finite = finite && fabsf(g) <= 3.402823466e+38f;           // false for an Inf and for a NaN
        any = any || g != 0.f;
    }
    const bool mixed = mix_gain(t, 0) != 0.f;
    r.ok = r.src && r.n > 0 && finite && any && (!mixed || (r.origin && r.pitch >= r.n)) && clip >= 0 && clip <= MI_CLIP_TANH &&
           fmt >= MI_DELIVER_I16 && fmt <= MI_DELIVER_F32 && (clip != MI_CLIP_RESCALE || (peak >= 0 && peak < n_peaks)) &&
           r.dst_off >= 0 && (r.dst_off & 3) == 0;
    r.clip = (int)clip; r.fmt = (int)fmt; r.peak = (int)peak;
    if (DST && r.ok) {
        const int64_t frame = (int64_t)channels * (r.fmt == MI_DELIVER_F32 ? 4 : 2);        // bytes
        r.ok = r.n <= dst_cap / frame && r.dst_off <= dst_cap - r.n * frame;
    }
    // 16-byte loads: every (source, channel) row starts at a multiple of 4 floats from an aligned base; the mix's rows do when its
    // pitch is a multiple of 4 too
    r.vec = (r.n & 3) == 0 && (reinterpret_cast<uintptr_t>(r.src) & 15) == 0;
    r.vec_origin = (r.n & 3) == 0 && (r.pitch & 3) == 0 && (reinterpret_cast<uintptr_t>(r.origin) & 15) == 0;
    return r;
}

// the value: frames j0 .. j0 + 3 of channel c of the row's remix, before clipping
__device__ __forceinline__ void mix_row_values(const MixRow &r, int n_sources, int channels, int c, int64_t j0, float (&v)[4]) {
    const int64_t stem_stride = (int64_t)channels * r.n;
    const float *base = r.src + (int64_t)c * r.n;                  // stem k's channel c at base + k * stem_stride
    mix_values<4>(
        n_sources, [&](int i) { return mix_gain(r.t, i); },
        [&](float (&o)[4]) {
            load4(r.origin + (int64_t)c * r.pitch, j0, r.n, r.vec_origin, o);
            if (r.affine) {
#pragma unroll
                for (int e = 0; e < 4; ++e) o[e] = restore_sample(o[e], r.mean, r.s);
            }
        },
        [&](int k, float (&s)[4]) { load4(base + k * stem_stride, j0, r.n, r.vec, s); }, v);
}

// mi_deliver_mix_peaks (DST) and mi_deliver_mix_peaks_update: deliver_peaks_kernel's grid, (ceil(max_n / 1024), n_rows)
template <bool DST>
__global__ __launch_bounds__(256) void deliver_mix_peaks_kernel(const int64_t *__restrict__ table, int n_sources, int channels,
                                                                unsigned *__restrict__ peaks, int n_peaks, int64_t dst_cap) {
    const MixRow r = mix_row<DST>(table + (size_t)blockIdx.y * MI_MIX_COLS, n_sources, channels, n_peaks, dst_cap);
    if (!r.ok || r.clip != MI_CLIP_RESCALE) return;                // the same for the whole block
    const int64_t j0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
    deliver_peak4([&](int c, float (&v)[4]) { mix_row_values(r, n_sources, channels, c, j0, v); }, channels, j0, r.n, peaks + r.peak);
}

// mi_deliver_mix_pcm: deliver_pcm_kernel's grid and thread assignment (four frames per thread) and its stores
__global__ __launch_bounds__(256) void deliver_mix_pcm_kernel(const int64_t *__restrict__ table, int n_sources, int channels,
                                                              const unsigned *__restrict__ peaks, int n_peaks,
                                                              unsigned char *__restrict__ dst, int64_t dst_cap) {
    const MixRow r = mix_row(table + (size_t)blockIdx.y * MI_MIX_COLS, n_sources, channels, n_peaks, dst_cap);
    if (!r.ok) return;
    const int64_t j0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
    if (j0 >= r.n) return;
    const float d = r.clip == MI_CLIP_RESCALE ? clip_divisor(peaks[r.peak]) : 0.f;
    unsigned char *out = dst + r.dst_off;                          // frames [0, n) of the row: inside dst_cap by mix_row
    deliver_store4([&](int c, float (&v)[4]) { mix_row_values(r, n_sources, channels, c, j0, v); }, channels, j0, r.n, r.clip, d,
                   r.fmt == MI_DELIVER_I16, out);
}

int launch_deliver_mix_peaks(const int64_t *table, int n_rows, int64_t max_n, int n_sources, int channels, unsigned *peaks, int n_peaks,
                             int64_t dst_cap, hipStream_t st) {
    MI_HIP(hipMemsetAsync(peaks, 0, sizeof(unsigned) * (size_t)n_peaks, st));
    hipLaunchKernelGGL(deliver_mix_peaks_kernel<true>, dim3(ceil_div(max_n, 1024), n_rows), dim3(256), 0, st, table, n_sources, channels,
                       peaks, n_peaks, dst_cap);
    MI_CHECK_LAUNCH();
    return MI_OK;
}

int launch_deliver_mix_peaks_update(const int64_t *table, int n_rows, int64_t max_n, int n_sources, int channels, unsigned *peaks,
                                    int n_peaks, hipStream_t st) {
    hipLaunchKernelGGL(deliver_mix_peaks_kernel<false>, dim3(ceil_div(max_n, 1024), n_rows), dim3(256), 0, st, table, n_sources,
                       channels, peaks, n_peaks, (int64_t)0);
    MI_CHECK_LAUNCH();
    return MI_OK;
}

int launch_deliver_mix_pcm(const int64_t *table, int n_rows, int64_t max_n, int n_sources, int channels, const unsigned *peaks,
                           int n_peaks, unsigned char *dst, int64_t dst_cap, hipStream_t st) {
    hipLaunchKernelGGL(deliver_mix_pcm_kernel, dim3(ceil_div(max_n, 1024), n_rows), dim3(256), 0, st, table, n_sources, channels, peaks,
                       n_peaks, dst, dst_cap);
    MI_CHECK_LAUNCH();
    return MI_OK;
}

}  // namespace mi
