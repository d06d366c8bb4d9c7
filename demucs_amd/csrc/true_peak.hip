// True peak of gain-weighted remixes (ITU-R BS.1770-4 Annex 2; include/demucs_amd.h, MI_TP_*): per output row the value is
// deliver_mix.hip's before clipping (post_ops.h's mix_values in float32, the mix through ORIGIN / ORIGIN_PITCH / ORIGIN_AFFINE),
// v = 0 outside the track.  With a bank h[p][k] of P phases x T taps, every phase p, channel c and position n has
//     acc = 0;  for k = 0 .. T-1 ascending:  acc = acc + h[p][k] * v[c][n - k]        (product and sum rounded separately)
// and the row keeps two uint32 bit patterns: `over`, max |acc| over p, c, n, and `sample`, max |v| over c and the track.  Both are
// pure functions of the values and max is order-free, so a stream's slots have the bits of the whole-track call for every
// partition of the input; the T - 1 values before a call's first position come from a two-sided history as deliver_resample.hip's.
//
// One launch, grid (ceil(max_n / 1024), n_rows), 256 threads, nothing synchronises with the host.  A workgroup takes 1024
// consecutive positions of its row, channel after channel: it stages them and the T - 1 before them in LDS once -- history, zeros
// below position 0 and past BEFORE + N, the mix's affine and the 16-byte loads are resolved there, thread t holding positions
// 4 t .. 4 t + 3 at a 16-byte boundary -- and runs the chains from LDS.  The Annex 2 bank (4 x 12) has its own instance whose
// window of 15 values sits in registers by four 16-byte LDS reads, every index a constant; any other bank reads LDS per tap.  The
// coefficients come by uniform loads from the bank.  The two maxima are reduced over the workgroup; per workgroup and slot there is
// at most one atomicMax, none when the maximum is 0 or the slot already holds as much (atomics of every wave on a row's one word
// were what bound the pass: DESIGN.md section 1, "True peak").
#include "common.h"
#include "kernels.h"
#include "post_ops.h"

namespace mi {

constexpr int kTpHead = 32;            // LDS floats before a workgroup's first position: >= MI_TP_MAX_TAPS - 1, a multiple of 4
constexpr int kTpSpan = 1024;          // positions of a workgroup

struct TpRow {
    const int64_t *t;
    const float *src, *origin;
    int64_t n, src_pitch, pitch, before, tail, hist_len, hist_rd, hist_wr, hist_start, hist_next;
    float mean, s;
    int peak;
    bool ok, affine, vec, vec_origin;
};

// float32 i of the nine gains, packed as MI_MIX_GAINS
__device__ __forceinline__ float tp_gain(const int64_t *__restrict__ t, int i) {
    return __uint_as_float((unsigned)((uint64_t)t[MI_TP_GAINS + (i >> 1)] >> ((i & 1) * 32)));
}

// whether [off, off + rows * len) lies inside [0, cap), without overflow
__device__ __forceinline__ bool tp_inside(int64_t off, int64_t rows, int64_t len, int64_t cap) {
    return off >= 0 && len >= 0 && off <= cap && len <= (cap - off) / rows;
}

// One row of the table with every rule under which it is skipped
__device__ __forceinline__ TpRow tp_row(const int64_t *__restrict__ t, int n_sources, int channels, int taps, int64_t hist_cap, int n_peaks) {
    constexpr int64_t kMax = (int64_t)1 << 61;
    TpRow r;
    r.t = t;
    r.src = reinterpret_cast<const float *>(static_cast<uintptr_t>(t[MI_TP_SRC]));
    r.origin = reinterpret_cast<const float *>(static_cast<uintptr_t>(t[MI_TP_ORIGIN]));
    r.n = t[MI_TP_N];
    r.src_pitch = t[MI_TP_SRC_PITCH];
    r.pitch = t[MI_TP_ORIGIN_PITCH];
    const uint64_t aff = (uint64_t)t[MI_TP_ORIGIN_AFFINE];
    r.mean = __uint_as_float((unsigned)aff);
    r.s = __uint_as_float((unsigned)(aff >> 32));
    r.affine = t[MI_TP_AFFINE_ON] != 0;
    r.before = t[MI_TP_BEFORE];
    r.tail = t[MI_TP_TAIL];
    r.hist_len = t[MI_TP_HIST_LEN];
    r.hist_rd = t[MI_TP_HIST_RD];
    r.hist_wr = t[MI_TP_HIST_WR];
    r.hist_start = t[MI_TP_HIST_START];
    r.hist_next = t[MI_TP_HIST_NEXT];
    const int64_t peak = t[MI_TP_PEAK];
    r.peak = (int)peak;
    bool finite = true, any = false;
    for (int i = 0; i <= n_sources; ++i) {
        const float g = tp_gain(t, i);
        finite = finite && fabsf(g) <= 3.402823466e+38f;           // false for an Inf and for a NaN
        any = any || g != 0.f;
    }
    const bool mixed = tp_gain(t, 0) != 0.f;
    r.ok = r.n >= 0 && r.n <= kMax && r.tail >= 0 && r.tail < taps && (r.n > 0 || r.tail > 0) && (r.n == 0 || r.src) &&
           r.src_pitch >= r.n && finite && any && (!mixed || r.n == 0 || (r.origin && r.pitch >= r.n)) && r.before >= 0 &&
           r.before <= kMax && r.hist_start >= 0 && r.hist_start <= r.before && r.hist_len >= 0 && peak >= 0 && peak < n_peaks;
    r.vec = r.vec_origin = false;
    if (!r.ok) return r;
    const int64_t end = r.before + r.n, kept = r.before - r.hist_start, side = r.hist_len;
    // the history: what is carried in fits a side and reaches T - 1 positions back (or to position 0); both sides inside their
    // capacity and apart; what is carried out fits a side
    r.ok = kept <= side && (r.hist_start == 0 || kept >= taps - 1) && tp_inside(r.hist_rd, channels, side, hist_cap) &&
           tp_inside(r.hist_wr, channels, side, hist_cap) &&
           (side == 0 || r.hist_rd - r.hist_wr >= channels * side || r.hist_wr - r.hist_rd >= channels * side) &&
           (r.hist_next < 0 || (r.hist_next >= r.hist_start && r.hist_next <= end && end - r.hist_next <= side));
    // 16-byte loads of frames j0 .. j0 + 3 (j0 a multiple of 4, all four inside N): every (source, channel) row starts at a multiple
    // of 4 floats from an aligned base; the mix's rows do when its pitch is a multiple of 4 too
    r.vec = (r.src_pitch & 3) == 0 && (reinterpret_cast<uintptr_t>(r.src) & 15) == 0;
    r.vec_origin = (r.pitch & 3) == 0 && (reinterpret_cast<uintptr_t>(r.origin) & 15) == 0;
    return r;
}

// W consecutive frames from j0 of a row; VEC: one 16-byte load (W == 4)
template <int W>
__device__ __forceinline__ void tp_load(const float *__restrict__ p, int64_t j0, bool vec, float (&v)[W]) {
    if constexpr (W == 4) {
        if (vec) {
            const float4 q = *reinterpret_cast<const float4 *>(p + j0);
            v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
            return;
        }
    }
#pragma unroll
    for (int e = 0; e < W; ++e) v[e] = p[j0 + e];
}

// the value: frames j0 .. j0 + W - 1 (all inside [0, N)) of channel c of the row's remix, before clipping
template <int W>
__device__ __forceinline__ void tp_values(const TpRow &r, int n_sources, int channels, int c, int64_t j0, bool vec, float (&v)[W]) {
    const float *base = r.src + (int64_t)c * r.src_pitch;          // stem k's channel c at + k * channels * src_pitch
    mix_values<W>(
        n_sources, [&](int g) { return tp_gain(r.t, g); },
        [&](float (&o)[W]) {
            tp_load<W>(r.origin + (int64_t)c * r.pitch, j0, vec && r.vec_origin, o);
            if (r.affine) {
#pragma unroll
                for (int e = 0; e < W; ++e) o[e] = restore_sample(o[e], r.mean, r.s);
            }
        },
        [&](int k, float (&s)[W]) { tp_load<W>(base + (int64_t)k * channels * r.src_pitch, j0, vec && r.vec, s); }, v);
}

// the value at track position p: 0 outside [0, BEFORE + N), the history below BEFORE, else the remix
__device__ __forceinline__ float tp_value_at(const TpRow &r, int n_sources, int channels, int c, int64_t p,
                                             const float *__restrict__ hist) {
    if (p < 0 || p >= r.before + r.n) return 0.f;
    if (p < r.before) return hist[r.hist_rd + (int64_t)c * r.hist_len + (p - r.hist_start)];   // p >= HIST_START by tp_row
    float v[1];
    tp_values<1>(r, n_sources, channels, c, p - r.before, false, v);
    return v[0];
}

// The chains of the thread's four positions from LDS; at(i) is the value i positions after the thread's first (i may be negative).
// FIXED: P x T are constants and the window of 4 + T - 1 values sits in registers, read by 16-byte LDS loads, every index a constant
template <int P, int T>
__device__ __forceinline__ unsigned tp_chains_fixed(const float *__restrict__ lds4, const float *__restrict__ bank, int live) {
    constexpr int A = (T - 1 + 3) / 4 * 4;                         // the window from a 16-byte boundary: w[i] is position i - A
    float w[A + 4];
#pragma unroll
    for (int q = 0; q < A / 4 + 1; ++q) {
        const float4 x = *reinterpret_cast<const float4 *>(lds4 - A + 4 * q);
        w[4 * q] = x.x; w[4 * q + 1] = x.y; w[4 * q + 2] = x.z; w[4 * q + 3] = x.w;
    }
    unsigned m = 0u;
#pragma unroll
    for (int p = 0; p < P; ++p) {
        float h[T];
#pragma unroll
        for (int k = 0; k < T; ++k) h[k] = bank[p * T + k];        // uniform
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float acc = 0.f;
#pragma unroll
            for (int k = 0; k < T; ++k) acc = __fadd_rn(acc, __fmul_rn(h[k], w[A + e - k]));
            if (e < live) m = max(m, abs_bits(acc));
        }
    }
    return m;
}

__device__ __forceinline__ unsigned tp_chains(const float *__restrict__ lds4, const float *__restrict__ bank, int phases, int taps,
                                              int live) {
    unsigned m = 0u;
    for (int e = 0; e < live; ++e) {
        for (int p = 0; p < phases; ++p) {
            const float *__restrict__ h = bank + p * taps;
            float acc = 0.f;
            for (int k = 0; k < taps; ++k) acc = __fadd_rn(acc, __fmul_rn(h[k], lds4[e - k]));
            m = max(m, abs_bits(acc));
        }
    }
    return m;
}

// FIXED: the bank is 4 x 12 (Annex 2)
template <bool FIXED>
__global__ __launch_bounds__(256) void true_peak_kernel(const int64_t *__restrict__ table, int n_sources, int channels,
                                                        const float *__restrict__ bank, int phases, int taps, float *__restrict__ hist,
                                                        int64_t hist_cap, unsigned *__restrict__ peaks, int n_peaks) {
    __shared__ __attribute__((aligned(16))) float lds[kTpHead + kTpSpan];
    __shared__ unsigned red[2][4];
    const TpRow r = tp_row(table + (size_t)blockIdx.y * MI_TP_COLS, n_sources, channels, taps, hist_cap, n_peaks);
    if (!r.ok) return;                                             // the same for the whole block
    const int64_t j_blk = (int64_t)blockIdx.x * kTpSpan;           // relative to BEFORE
    const int64_t count = r.n + r.tail;                            // positions the call evaluates
    if (j_blk >= count) return;
    const int tid = threadIdx.x;
    const int64_t j0 = j_blk + 4 * tid;
    const int live = (int)(count - j0 < 0 ? 0 : count - j0 > 4 ? 4 : count - j0);          // positions of the thread that are evaluated
    const int fresh = (int)(r.n - j0 < 0 ? 0 : r.n - j0 > 4 ? 4 : r.n - j0);               // ... that are samples of this call
    unsigned m_over = 0u, m_sample = 0u;
    for (int c = 0; c < channels; ++c) {
        if (c) __syncthreads();                                    // the chains of the channel before are done with the LDS
        float v[4] = {0.f, 0.f, 0.f, 0.f};
        if (fresh == 4) {
            tp_values<4>(r, n_sources, channels, c, j0, true, v);
        } else {
            for (int e = 0; e < fresh; ++e) {
                float one[1];
                tp_values<1>(r, n_sources, channels, c, j0 + e, false, one);
                v[e] = one[0];
            }
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) m_sample = max(m_sample, abs_bits(v[e]));               // positions past N hold 0
        *reinterpret_cast<float4 *>(lds + kTpHead + 4 * tid) = make_float4(v[0], v[1], v[2], v[3]);
        if (tid < taps - 1) lds[kTpHead - 1 - tid] = tp_value_at(r, n_sources, channels, c, r.before + j_blk - 1 - tid, hist);
        __syncthreads();
        if (live) {
            const float *lds4 = lds + kTpHead + 4 * tid;
            m_over = max(m_over, FIXED ? tp_chains_fixed<4, 12>(lds4, bank, live) : tp_chains(lds4, bank, phases, taps, live));
        }
    }
    for (int o = 32; o > 0; o >>= 1) {
        m_over = max(m_over, (unsigned)__shfl_xor((int)m_over, o));
        m_sample = max(m_sample, (unsigned)__shfl_xor((int)m_sample, o));
    }
    if ((tid & 63) == 0) {
        red[0][tid >> 6] = m_over;
        red[1][tid >> 6] = m_sample;
    }
    __syncthreads();
    if (tid < 2) {                                                 // thread 0: `over`, thread 1: `sample`
        const unsigned m = max(max(red[tid][0], red[tid][1]), max(red[tid][2], red[tid][3]));
        unsigned *slot = peaks + 2 * r.peak + tid;
        // a slot only grows, so a stale read can only be too small: the atomic is skipped only where it would change nothing
        if (m && __atomic_load_n(slot, __ATOMIC_RELAXED) < m) atomicMax(slot, m);
    }
    // block 0 of the row rewrites the other side of the history: positions [HIST_NEXT, BEFORE + N), from the read side below BEFORE
    if (blockIdx.x == 0 && r.hist_next >= 0) {
        const int64_t cnt = r.before + r.n - r.hist_next;
        for (int64_t i = tid; i < cnt * channels; i += 256) {
            const int c = (int)(i / cnt);
            const int64_t o = i - c * cnt;
            hist[r.hist_wr + (int64_t)c * r.hist_len + o] = tp_value_at(r, n_sources, channels, c, r.hist_next + o, hist);
        }
    }
}

int launch_true_peak_update(const int64_t *table, int n_rows, int64_t max_n, int n_sources, int channels, const float *bank, int phases,
                            int taps, float *hist, int64_t hist_cap, unsigned *peaks, int n_peaks, hipStream_t st) {
    const dim3 grid(ceil_div(max_n, kTpSpan), n_rows);
    if (phases == 4 && taps == 12)
        hipLaunchKernelGGL(true_peak_kernel<true>, grid, dim3(256), 0, st, table, n_sources, channels, bank, phases, taps, hist, hist_cap,
                           peaks, n_peaks);
    else
        hipLaunchKernelGGL(true_peak_kernel<false>, grid, dim3(256), 0, st, table, n_sources, channels, bank, phases, taps, hist, hist_cap,
                           peaks, n_peaks);
    MI_CHECK_LAUNCH();
    return MI_OK;
}

}  // namespace mi
