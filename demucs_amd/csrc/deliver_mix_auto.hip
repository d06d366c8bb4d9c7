// Delivery of remixes whose gains CHANGE along the track (include/demucs_amd.h, MI_AUTO_*): deliver_mix.hip's rows with a track
// position, base gains and a list of changes (at, ramp, target gains).  Term j at track position p has the gain
//     k = p - at < 0: unchanged;   k >= ramp: G_j exactly;   else P_j + (G_j - P_j) * (float(k) / float(ramp))
// of the last change with at <= p (P: the gains before it), every operation a separately rounded float32 one; the value is then
// post_ops.h's mix_values_each -- a term is added only at the samples where its gain is not 0 -- and deliver_io.h's clip, convert and
// interleave, on deliver_mix_pcm_kernel's grid (four frames a thread).
//
// A wave's 256 frames lie inside ONE settled stretch nearly always (no change at all, or the last one fully reached); the pass over
// the change list that checks the row's rules finds that out, and the wave then runs mix_values on uniform gains, exactly as
// deliver_mix.hip does.  Only a wave that a change or a ramp reaches takes the per-frame path, each thread bisecting `at` between
// the wave's two bounds.
// The gains of a ramp are read from the table where they are used and those of a settled wave are picked by compares from the
// registers the row check left them in; no register array is indexed by a variable, so no kernel uses scratch.
#include "common.h"
#include "kernels.h"
#include "post_ops.h"
#include "deliver_io.h"

namespace mi {

// |at|, ramp and |T0| up to this: a position, a difference of two and at + ramp then stay inside int64
static constexpr int64_t AUTO_POS_MAX = (int64_t)1 << 61;

struct AutoRow {
    const int64_t *t;                  // the row: the base gains are read from it where they are used
    const int64_t *chg;                // its changes, MI_AUTO_CHG_COLS words each
    int cnt;
    int64_t t0;                        // track position of frame 0
    const float *src, *origin;
    int64_t n, pitch, dst_off;
    float mean, s;
    int clip, fmt, peak;
    bool ok, affine, vec, vec_origin;
    int w_lo, w_hi;                    // the changes in force at the wave's first and last position (-1: none, the base gains)
    bool settled;                      // every frame of the wave has the gains of change w_lo, fully reached
    unsigned g_lo[10];                 // the bits of those gains, handed over by the lane that checked change w_lo
};

// float32 i of nine gains (0: the mix's, 1 + k: stem k's) packed two to an int64 from w, little-endian (as MI_MIX_GAINS)
__device__ __forceinline__ float packed_gain(const int64_t *__restrict__ w, int i) {
    return __uint_as_float((unsigned)((uint64_t)w[i >> 1] >> ((i & 1) * 32)));
}

// the five words of the gains that change `idx` reaches; -1: the row's base gains
__device__ __forceinline__ const int64_t *auto_gains(const AutoRow &r, int idx) {
    return idx < 0 ? r.t + MI_AUTO_GAINS : r.chg + (int64_t)idx * MI_AUTO_CHG_COLS + MI_AUTO_CHG_GAINS;
}

// the last change among [lo, hi) whose AT <= p, lo - 1 when there is none: a bisection, AT being ascending
__device__ __forceinline__ int change_at(const AutoRow &r, int64_t p, int lo, int hi) {
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (r.chg[(int64_t)mid * MI_AUTO_CHG_COLS + MI_AUTO_CHG_AT] <= p) lo = mid + 1;
        else hi = mid;
    }
    return lo - 1;
}

// One row of the table with every rule under which it is skipped: deliver_mix.hip's mix_row rules (all but "every gain is 0": a
// fade to silence is a legitimate stretch of a track) and those of the change list.  Every WAVE checks the whole list for itself,
// its lanes side by side, 64 changes a pass -- no LDS and no barrier, and all waves of a row reach the same verdict.  The same pass
// counts the changes that begin at or before the wave's first and last position (pw = T0 + jw and pw + 255): the list being
// ordered, those counts bound the change in force at any of the wave's frames (w_lo .. w_hi), and `settled` says that every one
// of them has the gains of change w_lo fully reached.  Every lane of the wave calls this.
__device__ __forceinline__ AutoRow auto_row(const int64_t *__restrict__ table, int64_t table_len, int row, int64_t jw, int n_sources,
                                            int channels, int n_peaks, int64_t dst_cap) {
    const int64_t *t = table + (int64_t)row * MI_AUTO_COLS;
    AutoRow r;
    r.t = t;
    r.src = reinterpret_cast<const float *>(static_cast<uintptr_t>(t[MI_AUTO_SRC]));
    r.origin = reinterpret_cast<const float *>(static_cast<uintptr_t>(t[MI_AUTO_ORIGIN]));
    r.n = t[MI_AUTO_N];
    r.pitch = t[MI_AUTO_ORIGIN_PITCH];
    r.dst_off = t[MI_AUTO_DST_OFF];
    r.t0 = t[MI_AUTO_T0];
    const uint64_t aff = (uint64_t)t[MI_AUTO_ORIGIN_AFFINE];
    r.mean = __uint_as_float((unsigned)aff);
    r.s = __uint_as_float((unsigned)(aff >> 32));
    r.affine = t[MI_AUTO_AFFINE_ON] != 0;
    const int64_t clip = t[MI_AUTO_CLIP], fmt = t[MI_AUTO_FMT], peak = t[MI_AUTO_PEAK];
    const int64_t off = t[MI_AUTO_CHG_OFF], cnt = t[MI_AUTO_CHG_N];
    // the list lies inside the table (table_len <= INT32_MAX words, so cnt fits an int)
    const bool inside = off >= 0 && cnt >= 0 && off <= table_len && cnt <= (table_len - off) / MI_AUTO_CHG_COLS;
    r.chg = table + (inside ? off : 0);
    r.cnt = inside ? (int)cnt : 0;
    const bool t0_ok = r.t0 >= -AUTO_POS_MAX && r.t0 <= AUTO_POS_MAX;
    const int64_t pw = (t0_ok ? r.t0 : 0) + jw, pe = pw + 255;

    bool good = inside && t0_ok, mixed = packed_gain(t + MI_AUTO_GAINS, 0) != 0.f, moving = false;
    for (int i = 0; i <= n_sources; ++i) good = good && fabsf(packed_gain(t + MI_AUTO_GAINS, i)) <= 3.402823466e+38f;   // false for Inf and NaN
    int n_lo = 0, n_hi = 0;
#pragma unroll
    for (int j = 0; j < 5; ++j) {
        r.g_lo[2 * j] = (unsigned)(uint64_t)t[MI_AUTO_GAINS + j];
        r.g_lo[2 * j + 1] = (unsigned)((uint64_t)t[MI_AUTO_GAINS + j] >> 32);
    }
    for (int c0 = 0; c0 < r.cnt; c0 += 64) {                       // the same trips for every lane
        const int c = c0 + (threadIdx.x & 63);
        bool ok = true, mix = false, lo = false, hi = false, mov = false;
        unsigned g[10] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
        if (c < r.cnt) {
            const int64_t *w = r.chg + (int64_t)c * MI_AUTO_CHG_COLS;
            const int64_t at = w[MI_AUTO_CHG_AT], ramp = w[MI_AUTO_CHG_RAMP];
#pragma unroll
            for (int j = 0; j < 5; ++j) {
                g[2 * j] = (unsigned)(uint64_t)w[MI_AUTO_CHG_GAINS + j];
                g[2 * j + 1] = (unsigned)((uint64_t)w[MI_AUTO_CHG_GAINS + j] >> 32);
            }
            ok = at >= -AUTO_POS_MAX && at <= AUTO_POS_MAX && ramp >= 0 && ramp <= AUTO_POS_MAX;
            if (c > 0) {               // ordered, and not before the end of the ramp in front of it
                const int64_t pa = w[MI_AUTO_CHG_AT - MI_AUTO_CHG_COLS], pr = w[MI_AUTO_CHG_RAMP - MI_AUTO_CHG_COLS];
                ok = ok && pa >= -AUTO_POS_MAX && pa <= AUTO_POS_MAX && pr >= 0 && pr <= AUTO_POS_MAX && at >= pa + pr;
            }
#pragma unroll
            for (int i = 0; i < 9; ++i)                             // 2^64: G - P cannot overflow; false for Inf and NaN
                ok = ok && (i > n_sources || fabsf(__uint_as_float(g[i])) <= 18446744073709551616.f);
            mix = __uint_as_float(g[0]) != 0.f;
            if (ok) {
                lo = at <= pw;
                hi = at <= pe;
                mov = hi && pw - at < ramp;                         // it begins in the wave's frames, or its ramp reaches into them
            }
        }
        good = good && __all(ok);
        mixed = mixed || __any(mix);                               // some stretch of the row reads the mix
        moving = moving || __any(mov);
        const int c_lo = __popcll(__ballot(lo));                  // ordered: the pass's changes behind pw are its first c_lo
        n_lo += c_lo;
        n_hi += __popcll(__ballot(hi));
        if (c_lo) {                                                // the last of them so far: its gains come over from its lane
#pragma unroll
            for (int j = 0; j < 10; ++j) r.g_lo[j] = (unsigned)__builtin_amdgcn_readlane((int)g[j], c_lo - 1);
        }
    }
    r.w_lo = n_lo - 1;
    r.w_hi = n_hi - 1;
    r.settled = !moving;               // then w_lo == w_hi: a change that begins behind pw has at + ramp > pw

    r.ok = good && r.src && r.n > 0 && (!mixed || (r.origin && r.pitch >= r.n)) && clip >= 0 && clip <= MI_CLIP_TANH &&
           fmt >= MI_DELIVER_I16 && fmt <= MI_DELIVER_F32 && (clip != MI_CLIP_RESCALE || (peak >= 0 && peak < n_peaks)) &&
           r.dst_off >= 0 && (r.dst_off & 3) == 0;
    r.clip = (int)clip; r.fmt = (int)fmt; r.peak = (int)peak;
    if (r.ok) {
        const int64_t frame = (int64_t)channels * (r.fmt == MI_DELIVER_F32 ? 4 : 2);        // bytes
        r.ok = r.n <= dst_cap / frame && r.dst_off <= dst_cap - r.n * frame;
    }
    r.vec = (r.n & 3) == 0 && (reinterpret_cast<uintptr_t>(r.src) & 15) == 0;
    r.vec_origin = (r.n & 3) == 0 && (r.pitch & 3) == 0 && (reinterpret_cast<uintptr_t>(r.origin) & 15) == 0;
    return r;
}

// What a thread knows of its four frames j0 .. j0 + 3: for each the change in force, whether its ramp is still running, and t
struct AutoFrames {
    int idx[4];
    bool ramping[4];
    float t[4];
};

__device__ __forceinline__ AutoFrames auto_frames(const AutoRow &r, int64_t j0) {
    AutoFrames f;
#pragma unroll
    for (int e = 0; e < 4; ++e) { f.idx[e] = r.w_lo; f.ramping[e] = false; f.t[e] = 0.f; }
    if (r.settled) return f;
    const int64_t p0 = r.t0 + j0;
    // bisections between the wave's bounds: at[w_lo] <= pw <= p0, and no change past w_hi begins in the wave's frames
    f.idx[0] = change_at(r, p0, r.w_lo + 1, r.w_hi + 1);
    f.idx[3] = change_at(r, p0 + 3, f.idx[0] + 1, r.w_hi + 1);
    f.idx[1] = f.idx[0] == f.idx[3] ? f.idx[0] : change_at(r, p0 + 1, f.idx[0] + 1, f.idx[3] + 1);
    f.idx[2] = f.idx[1] == f.idx[3] ? f.idx[1] : change_at(r, p0 + 2, f.idx[1] + 1, f.idx[3] + 1);
    int64_t at = 0, ramp = 0;
    float ramp_f = 0.f;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        if (f.idx[e] < 0) continue;
        if (e == 0 || f.idx[e] != f.idx[e - 1]) {
            const int64_t *w = r.chg + (int64_t)f.idx[e] * MI_AUTO_CHG_COLS;
            at = w[MI_AUTO_CHG_AT];
            ramp = w[MI_AUTO_CHG_RAMP];
            ramp_f = __ll2float_rn(ramp);
        }
        const int64_t k = p0 + e - at;
        if (k < ramp) {
            f.ramping[e] = true;
            f.t[e] = __fdiv_rn(__ll2float_rn(k), ramp_f);
        }
    }
    return f;
}

// the value: frames j0 .. j0 + 3 of channel c of the row's remix, before clipping
__device__ __forceinline__ void auto_row_values(const AutoRow &r, const AutoFrames &f, int n_sources, int channels, int c, int64_t j0,
                                                float (&v)[4]) {
    const int64_t stem_stride = (int64_t)channels * r.n;
    const float *base = r.src + (int64_t)c * r.n;                  // stem k's channel c at base + k * stem_stride
    auto origin = [&](float (&o)[4]) {
        load4(r.origin + (int64_t)c * r.pitch, j0, r.n, r.vec_origin, o);
        if (r.affine) {
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = restore_sample(o[e], r.mean, r.s);
        }
    };
    auto stem = [&](int k, float (&s)[4]) { load4(base + k * stem_stride, j0, r.n, r.vec, s); };
    if (r.settled) {                   // uniform gains that the row check left in registers: picked by compares, never indexed
        mix_values<4>(
            n_sources,
            [&](int i) {
                unsigned bits = r.g_lo[0];
#pragma unroll
                for (int j = 1; j < 9; ++j) bits = i == j ? r.g_lo[j] : bits;
                return __uint_as_float(bits);
            },
            origin, stem, v);
        return;
    }
    mix_values_each<4>(
        n_sources,
        [&](int i, float (&g)[4]) {
            float P = 0.f, G = 0.f;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                // along a thread's frames the change index only grows and a ramp only ends, so what was loaded for e - 1 serves e
                // whenever the index is the same
                if (e == 0 || f.idx[e] != f.idx[e - 1]) {
                    G = packed_gain(auto_gains(r, f.idx[e]), i);
                    if (f.ramping[e]) P = packed_gain(auto_gains(r, f.idx[e] - 1), i);
                }
                g[e] = f.ramping[e] ? __fadd_rn(P, __fmul_rn(__fsub_rn(G, P), f.t[e])) : G;
            }
        },
        origin, stem, v);
}

// mi_deliver_mix_auto_peaks: deliver_mix_peaks_kernel's grid, (ceil(max_n / 1024), n_rows)
__global__ __launch_bounds__(256) void deliver_mix_auto_peaks_kernel(const int64_t *__restrict__ table, int64_t table_len, int n_sources,
                                                                     int channels, unsigned *__restrict__ peaks, int n_peaks,
                                                                     int64_t dst_cap) {
    const int64_t j0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
    const AutoRow r = auto_row(table, table_len, blockIdx.y, j0 - (threadIdx.x & 63) * 4, n_sources, channels, n_peaks, dst_cap);
    if (!r.ok || r.clip != MI_CLIP_RESCALE) return;                // the same for the whole block
    const AutoFrames f = auto_frames(r, j0);
    deliver_peak4([&](int c, float (&v)[4]) { auto_row_values(r, f, n_sources, channels, c, j0, v); }, channels, j0, r.n, peaks + r.peak);
}

// mi_deliver_mix_auto_pcm: deliver_mix_pcm_kernel's grid and thread assignment (four frames per thread) and its stores
__global__ __launch_bounds__(256) void deliver_mix_auto_pcm_kernel(const int64_t *__restrict__ table, int64_t table_len, int n_sources,
                                                                   int channels, const unsigned *__restrict__ peaks, int n_peaks,
                                                                   unsigned char *__restrict__ dst, int64_t dst_cap) {
    const int64_t j0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
    const AutoRow r = auto_row(table, table_len, blockIdx.y, j0 - (threadIdx.x & 63) * 4, n_sources, channels, n_peaks, dst_cap);
    if (!r.ok) return;
    if (j0 >= r.n) return;
    const AutoFrames f = auto_frames(r, j0);
    const float d = r.clip == MI_CLIP_RESCALE ? clip_divisor(peaks[r.peak]) : 0.f;
    unsigned char *out = dst + r.dst_off;                          // frames [0, n) of the row: inside dst_cap by auto_row
    deliver_store4([&](int c, float (&v)[4]) { auto_row_values(r, f, n_sources, channels, c, j0, v); }, channels, j0, r.n, r.clip, d,
                   r.fmt == MI_DELIVER_I16, out);
}

int launch_deliver_mix_auto_peaks(const int64_t *table, int64_t table_len, int n_rows, int64_t max_n, int n_sources, int channels,
                                  unsigned *peaks, int n_peaks, int64_t dst_cap, hipStream_t st) {
    MI_HIP(hipMemsetAsync(peaks, 0, sizeof(unsigned) * (size_t)n_peaks, st));
    hipLaunchKernelGGL(deliver_mix_auto_peaks_kernel, dim3(ceil_div(max_n, 1024), n_rows), dim3(256), 0, st, table, table_len, n_sources,
                       channels, peaks, n_peaks, dst_cap);
    MI_CHECK_LAUNCH();
    return MI_OK;
}

int launch_deliver_mix_auto_pcm(const int64_t *table, int64_t table_len, int n_rows, int64_t max_n, int n_sources, int channels,
                                const unsigned *peaks, int n_peaks, unsigned char *dst, int64_t dst_cap, hipStream_t st) {
    hipLaunchKernelGGL(deliver_mix_auto_pcm_kernel, dim3(ceil_div(max_n, 1024), n_rows), dim3(256), 0, st, table, table_len, n_sources,
                       channels, peaks, n_peaks, dst, dst_cap);
    MI_CHECK_LAUNCH();
    return MI_OK;
}

}  // namespace mi
