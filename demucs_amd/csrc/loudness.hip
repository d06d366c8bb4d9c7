// Sub-block energies for ITU-R BS.1770-4 loudness of gain-weighted remixes (include/demucs_amd.h, MI_LOUD_*): per output row the
// value is deliver_mix.hip's before clipping (post_ops.h's mix_values in float32, the mix through ORIGIN / ORIGIN_PITCH /
// ORIGIN_AFFINE), K-weighted by two cascaded biquads in float64 and squared and summed over sub-blocks of `hop` samples that are
// anchored to absolute track positions.  The recursion is sequential in time, so the parallelism is over sub-blocks: the work item
// of (row, channel, sub-block h) runs both biquads from zero state over positions [h * hop - warm, (h + 1) * hop) -- positions
// below 0 read 0, the true zero state -- and adds y * y over the last `hop` of them in ascending order.  e[c][h] is therefore a
// pure function of the values in that window, produced by one instruction sequence wherever and whenever it is computed: a
// stream's energies have the bits of the whole-track call for every partition of the input.
//
// Two launches, nothing synchronises with the host, no atomics:
//   loud_values_kernel    the carried values [HIST_START, BEFORE) from the read side of the history and the call's N new values
//                         side by side into the work area, and positions [HIST_NEXT, BEFORE + N) into the write side;
//   loud_energy_kernel    the recursions of the sub-blocks that became complete, reading the work area alone.
// A wave's 64 lanes walk 64 windows `hop` samples apart: 64 cache lines per load instruction, so a lane takes 16 floats at a time
// by 16-byte loads and asks for the next 16 before it works on these (loud_run); per step and lane there are ten float64 FMAs, of
// which one per biquad is on the recurrence.
#include "common.h"
#include "kernels.h"
#include "post_ops.h"

namespace mi {

struct LoudCoef {                      // the two biquads, y = b0 x + b1 x1 + b2 x2 - a1 y1 - a2 y2
    double b[2][3], a[2][2];
};

struct LoudRow {
    const int64_t *t;
    const float *src, *origin;
    int64_t n, src_pitch, pitch, before, hist_len, hist_rd, hist_wr, hist_start, hist_next, e_off, e_pitch, work_off, work_pitch;
    int64_t kept, h0, h1;              // carried values; the sub-blocks [h0, h1) become complete on this call
    float mean, s;
    bool ok, affine;
};

// float32 i of the nine gains, packed as MI_MIX_GAINS
__device__ __forceinline__ float loud_gain(const int64_t *__restrict__ t, int i) {
    return __uint_as_float((unsigned)((uint64_t)t[MI_LOUD_GAINS + (i >> 1)] >> ((i & 1) * 32)));
}

// whether [off, off + rows * len) lies inside [0, cap), without overflow
__device__ __forceinline__ bool loud_inside(int64_t off, int64_t rows, int64_t len, int64_t cap) {
    return off >= 0 && len >= 0 && off <= cap && len <= (cap - off) / rows;
}

// One row of the table with every rule under which it is skipped; both kernels read a row through this, so they agree on it
__device__ __forceinline__ LoudRow loud_row(const int64_t *__restrict__ t, int n_sources, int channels, int64_t hop, int64_t warm,
                                            int64_t hist_cap, int64_t e_cap, int64_t work_cap) {
    constexpr int64_t kMax = (int64_t)1 << 61;
    LoudRow r;
    r.t = t;
    r.src = reinterpret_cast<const float *>(static_cast<uintptr_t>(t[MI_LOUD_SRC]));
    r.origin = reinterpret_cast<const float *>(static_cast<uintptr_t>(t[MI_LOUD_ORIGIN]));
    r.n = t[MI_LOUD_N];
    r.src_pitch = t[MI_LOUD_SRC_PITCH];
    r.pitch = t[MI_LOUD_ORIGIN_PITCH];
    const uint64_t aff = (uint64_t)t[MI_LOUD_ORIGIN_AFFINE];
    r.mean = __uint_as_float((unsigned)aff);
    r.s = __uint_as_float((unsigned)(aff >> 32));
    r.affine = t[MI_LOUD_AFFINE_ON] != 0;
    r.before = t[MI_LOUD_BEFORE];
    r.hist_len = t[MI_LOUD_HIST_LEN];
    r.hist_rd = t[MI_LOUD_HIST_RD];
    r.hist_wr = t[MI_LOUD_HIST_WR];
    r.hist_start = t[MI_LOUD_HIST_START];
    r.hist_next = t[MI_LOUD_HIST_NEXT];
    r.e_off = t[MI_LOUD_E_OFF];
    r.e_pitch = t[MI_LOUD_E_PITCH];
    r.work_off = t[MI_LOUD_WORK_OFF];
    r.work_pitch = t[MI_LOUD_WORK_PITCH];
    r.kept = r.h0 = r.h1 = 0;
    bool finite = true, any = false;
    for (int i = 0; i <= n_sources; ++i) {
        const float g = loud_gain(t, i);
        finite = finite && fabsf(g) <= 3.402823466e+38f;           // false for an Inf and for a NaN
        any = any || g != 0.f;
    }
    const bool mixed = loud_gain(t, 0) != 0.f;
    r.ok = hop >= 1 && hop <= kMax && warm >= 0 && warm <= kMax && r.src && r.n > 0 && r.n <= kMax && r.src_pitch >= r.n && finite &&
           any && (!mixed || (r.origin && r.pitch >= r.n)) && r.before >= 0 && r.before <= kMax && r.hist_start >= 0 &&
           r.hist_start <= r.before && r.hist_len >= 0;
    if (!r.ok) return r;
    const int64_t end = r.before + r.n;
    r.kept = r.before - r.hist_start;
    r.h0 = r.before / hop;
    r.h1 = end / hop;
    // the history: both sides inside their capacity and apart; what is carried in fits a side, what is carried out does too
    const int64_t side = r.hist_len;
    r.ok = r.kept <= side && loud_inside(r.hist_rd, channels, side, hist_cap) && loud_inside(r.hist_wr, channels, side, hist_cap) &&
           (side == 0 || r.hist_rd - r.hist_wr >= channels * side || r.hist_wr - r.hist_rd >= channels * side) &&
           (r.hist_next < 0 || (r.hist_next >= r.hist_start && r.hist_next <= end && end - r.hist_next <= side)) &&
           // the first window of this call, from max(0, h0 * hop - warm) on, begins inside what is carried
           (r.h1 == r.h0 || (r.h0 * hop - warm > 0 ? r.h0 * hop - warm : 0) >= r.hist_start) &&
           r.e_pitch >= r.h1 && loud_inside(r.e_off, channels, r.e_pitch, e_cap) && r.work_pitch >= r.kept + r.n &&
           loud_inside(r.work_off, channels, r.work_pitch, work_cap);
    return r;
}

// loud_values_kernel: grid (ceil(max_n / 256), channels, n_rows); element i of a (row, channel) is track position HIST_START + i
__global__ __launch_bounds__(256) void loud_values_kernel(const int64_t *__restrict__ table, int n_sources, int channels, int64_t hop,
                                                          int64_t warm, float *__restrict__ hist, int64_t hist_cap, int64_t e_cap,
                                                          float *__restrict__ work, int64_t work_cap) {
    const LoudRow r = loud_row(table + (size_t)blockIdx.z * MI_LOUD_COLS, n_sources, channels, hop, warm, hist_cap, e_cap, work_cap);
    if (!r.ok) return;                                             // the same for the whole block
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= r.kept + r.n) return;
    const int c = blockIdx.y;
    float v;
    if (i < r.kept) {
        v = hist[r.hist_rd + (int64_t)c * r.hist_len + i];
    } else {
        const int64_t j = i - r.kept;
        const float *base = r.src + (int64_t)c * r.src_pitch + j;  // stem k's channel c at + k * channels * src_pitch
        float a[1];
        mix_values<1>(
            n_sources, [&](int g) { return loud_gain(r.t, g); },
            [&](float (&o)[1]) {
                o[0] = r.origin[(int64_t)c * r.pitch + j];
                if (r.affine) o[0] = restore_sample(o[0], r.mean, r.s);
            },
            [&](int k, float (&s)[1]) { s[0] = base[(int64_t)k * channels * r.src_pitch]; }, a);
        v = a[0];
    }
    work[r.work_off + (int64_t)c * r.work_pitch + i] = v;
    const int64_t p = r.hist_start + i;
    if (r.hist_next >= 0 && p >= r.hist_next) hist[r.hist_wr + (int64_t)c * r.hist_len + (p - r.hist_next)] = v;
}

// one step of both biquads: x -> y of the second.  The sum without y[n-1] first, so that one FMA per biquad is on the recurrence
struct LoudState {
    double x1[2], x2[2], y1[2], y2[2];
};
__device__ __forceinline__ double loud_step(const LoudCoef &k, LoudState &s, double x) {
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        const double t = fma(k.b[q][0], x, fma(k.b[q][1], s.x1[q], fma(k.b[q][2], s.x2[q], -(k.a[q][1] * s.y2[q]))));
        const double y = fma(-k.a[q][0], s.y1[q], t);
        s.x2[q] = s.x1[q]; s.x1[q] = x;
        s.y2[q] = s.y1[q]; s.y1[q] = y;
        x = y;
    }
    return x;
}

// Positions [p, end) of one window through both biquads; SUM: y * y is added to e, in ascending order.  The arithmetic is one
// loud_step per position whatever the loads look like: scalar loads up to a 16-byte boundary of the address, then 16 floats a
// lane by four 16-byte loads, the next 16 requested before the current 16 steps run (a step issues about 48 cycles of float64
// FMAs, so the 16 steps cover a load from HBM), then what is left by fours and by ones.  Nothing outside [p, end) is read
template <bool SUM>
__device__ __forceinline__ void loud_run(const LoudCoef &k, LoudState &s, const float *__restrict__ w, int64_t &p, int64_t end, double &e) {
    auto step = [&](float x) {
        const double y = loud_step(k, s, (double)x);
        if (SUM) e = fma(y, y, e);
    };
    auto step4 = [&](const float4 &v) {
        step(v.x); step(v.y); step(v.z); step(v.w);
    };
    for (; p < end && (reinterpret_cast<uintptr_t>(w + p) & 15) != 0; ++p) step(w[p]);
    if (p + 16 <= end) {
        const float4 *v = reinterpret_cast<const float4 *>(w + p);
        float4 a0 = v[0], a1 = v[1], a2 = v[2], a3 = v[3];
        for (;;) {
            p += 16;
            v += 4;
            const bool more = p + 16 <= end;
            float4 b0 = a0, b1 = a1, b2 = a2, b3 = a3;
            if (more) {
                b0 = v[0]; b1 = v[1]; b2 = v[2]; b3 = v[3];
            }
            step4(a0); step4(a1); step4(a2); step4(a3);
            if (!more) break;
            a0 = b0; a1 = b1; a2 = b2; a3 = b3;
        }
    }
    for (; p + 4 <= end; p += 4) step4(*reinterpret_cast<const float4 *>(w + p));
    for (; p < end; ++p) step(w[p]);
}

// loud_energy_kernel: grid (ceil(max_blocks / 64), channels, n_rows), one wave a workgroup; lane -> sub-block
__global__ __launch_bounds__(64) void loud_energy_kernel(const int64_t *__restrict__ table, int n_sources, int channels, int64_t hop,
                                                         int64_t warm, LoudCoef k, int64_t hist_cap, double *__restrict__ energies,
                                                         int64_t e_cap, const float *__restrict__ work, int64_t work_cap) {
    const LoudRow r = loud_row(table + (size_t)blockIdx.z * MI_LOUD_COLS, n_sources, channels, hop, warm, hist_cap, e_cap, work_cap);
    if (!r.ok) return;
    const int64_t h = r.h0 + (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (h >= r.h1) return;
    const int c = blockIdx.y;
    // position p at w[p]: inside the work area from max(0, h * hop - warm) >= HIST_START on, by loud_row
    const float *__restrict__ w = work + r.work_off + (int64_t)c * r.work_pitch - r.hist_start;
    const int64_t lo = h * hop;
    int64_t p = lo - warm > 0 ? lo - warm : 0;
    LoudState s = {};
    double e = 0.0;
    loud_run<false>(k, s, w, p, lo, e);                            // the warm-up
    loud_run<true>(k, s, w, p, lo + hop, e);
    energies[r.e_off + (int64_t)c * r.e_pitch + h] = e;
}

int launch_loudness_update(const int64_t *table, int n_rows, int64_t max_n, int64_t max_blocks, int n_sources, int channels,
                           const double *coef, int64_t hop, int64_t warm, float *hist, int64_t hist_cap, double *energies, int64_t e_cap,
                           float *work, int64_t work_cap, hipStream_t st) {
    LoudCoef k;
    for (int q = 0; q < 2; ++q) {
        for (int i = 0; i < 3; ++i) k.b[q][i] = coef[5 * q + i];
        for (int i = 0; i < 2; ++i) k.a[q][i] = coef[5 * q + 3 + i];
    }
    hipLaunchKernelGGL(loud_values_kernel, dim3(ceil_div(max_n, 256), channels, n_rows), dim3(256), 0, st, table, n_sources, channels, hop,
                       warm, hist, hist_cap, e_cap, work, work_cap);
    MI_CHECK_LAUNCH();
    if (max_blocks > 0) {
        hipLaunchKernelGGL(loud_energy_kernel, dim3(ceil_div(max_blocks, 64), channels, n_rows), dim3(64), 0, st, table, n_sources,
                           channels, hop, warm, k, hist_cap, energies, e_cap, work, work_cap);
        MI_CHECK_LAUNCH();
    }
    return MI_OK;
}

}  // namespace mi
