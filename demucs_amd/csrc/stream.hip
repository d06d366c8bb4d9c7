// Device side of the streaming scheduler (demucs_amd/stream.py): the emit step that turns the finished spans of every
// (bag member, shift pass) accumulator into final stems (reference: demucs/apply.py:201-256,297-299, demucs/api.py:285-288).
//
// The reference computes these stems over the whole track with separate torch operations: per pass `out /= sum_weight`
// (ola.hip's finish), the shift average, the bag average, the Separator's inverse affine.  Each is elementwise, so the emitted
// span can be computed on its own, and one thread runs the whole chain for one (row, sample) in the reference's order with
// every step a separately rounded float32 operation (__fadd_rn / __fmul_rn / __fdiv_rn; the library builds with
// -ffp-contract=off).  The host-scalar factors are the float32 values torch's CUDA kernels use (include/demucs_amd.h).
//
// A stream group (StreamGroup in demucs_amd/stream.py) keeps every stream's input window and accumulators in one state buffer and
// treats its streams as one unit of work per push: one streams_append launch writes every stream's new samples into its window,
// one streams_emit launch turns every stream's finished spans into stems, and streams_compact re-lays the state buffer out when a
// stream outgrows its room.  All three are table-driven, memory-bound scatter / elementwise kernels.
#include "common.h"
#include "kernels.h"

namespace mi {

// The whole chain for output sample i of row `row` (source k = row / channels) from the pass rows [p_lo, p_hi) of `passes`,
// whose segment ranges are clamped to [s_lo, s_hi) of `segs`.  stream_emit_kernel (one stream) and streams_emit_kernel (a table of
// streams) both call it, so one stream's stems are the same float32 sequence whichever entry computes them.
__device__ __forceinline__ float emit_sample(const float *__restrict__ acc, int64_t acc_cap, int n_sources, int channels, int row,
                                             int64_t i, const int64_t *__restrict__ passes, int p_lo, int p_hi,
                                             const int64_t *__restrict__ segs, int64_t s_lo, int64_t s_hi,
                                             const float *__restrict__ weights, int64_t weights_cap, const float *__restrict__ scales,
                                             int n_members, int shifts, int bag, const float *__restrict__ stats) {
    const int rows = n_sources * channels, k = row / channels;
    const int stride = n_sources + 1;                     // per member: [1 / shifts, w[m][0 .. S-1]]
    float est = 0.f, mem = 0.f;
    bool have_est = false, have_mem = false;
    int cur = -1;
    auto close_member = [&]() {
        if (!have_mem) return;
        float v = mem;
        if (shifts > 0) v = __fmul_rn(v, scales[(size_t)cur * stride]);            // out /= shifts
        if (bag) {
            v = __fmul_rn(v, scales[(size_t)cur * stride + 1 + k]);                   // out[:, k] *= w[m][k]
            est = have_est ? __fadd_rn(est, v) : v;                                   // estimates.add_(out)
        } else {
            est = v;
        }
        have_est = true;
        have_mem = false;
    };
    for (int p = p_lo; p < p_hi; ++p) {
        const int64_t *t = passes + (size_t)p * MI_EMIT_PASS_COLS;
        int64_t member = t[MI_EMIT_MEMBER];
        member = member < 0 ? 0 : member >= n_members ? n_members - 1 : member;
        if ((int)member != cur) {
            close_member();
            cur = (int)member;
        }
        const int64_t base = t[MI_EMIT_ACC_BASE], len = t[MI_EMIT_ACC_LEN], q = t[MI_EMIT_Q0] + i;
        const int64_t w_off = t[MI_EMIT_W_OFF];
        const bool acc_ok = base >= 0 && len >= 0 && len <= acc_cap && base <= acc_cap - (int64_t)rows * len && q >= 0 && q < len;
        float v = acc_ok ? acc[base + (int64_t)row * len + q] : 0.f;
        // sum_weight at q in ascending segment order (ola.hip's finish): the first segment that can reach q by binary search
        const bool w_ok = w_off >= 0 && w_off <= weights_cap;
        const int64_t w_room = w_ok ? weights_cap - w_off : 0;
        const int64_t w_len = t[MI_EMIT_W_LEN] < 0 ? 0 : t[MI_EMIT_W_LEN] < w_room ? t[MI_EMIT_W_LEN] : w_room;
        int64_t lo = t[MI_EMIT_SEG_LO], hi = t[MI_EMIT_SEG_HI];
        lo = lo < s_lo ? s_lo : lo > s_hi ? s_hi : lo;
        hi = hi < lo ? lo : hi > s_hi ? s_hi : hi;
        int64_t a = lo, b = hi;
        while (a < b) { const int64_t mid = (a + b) >> 1; if (segs[2 * mid] > q - w_len) b = mid; else a = mid + 1; }
        float sw = 0.f;
        for (int64_t s = a; s < hi && segs[2 * s] <= q; ++s) {
            const int64_t j = q - segs[2 * s];
            if (j >= 0 && j < segs[2 * s + 1] && j < w_len) sw = __fadd_rn(sw, weights[w_off + j]);
        }
        v = __fdiv_rn(v, sw);                                                         // out /= sum_weight
        mem = have_mem ? __fadd_rn(mem, v) : v;                                       // out.add_(piece)
        have_mem = true;
    }
    close_member();
    if (bag) est = __fmul_rn(est, scales[(size_t)n_members * stride + k]);           // estimates[:, k] /= totals[k]
    if (stats) est = __fadd_rn(__fmul_rn(est, stats[1]), stats[0]);                   // x *= std; x += mean
    return est;
}

// grid (ceil(n / 256), n_sources * channels); thread: output sample i = blockIdx.x * 256 + threadIdx.x of row blockIdx.y
__global__ __launch_bounds__(256) void stream_emit_kernel(const float *__restrict__ acc, int64_t acc_cap, int n_sources, int channels,
                                                          const int64_t *__restrict__ passes, int n_passes,
                                                          const int64_t *__restrict__ segs, int n_segs,
                                                          const float *__restrict__ weights, int64_t weights_cap,
                                                          const float *__restrict__ scales, int n_members, int shifts, int bag,
                                                          const float *__restrict__ stats, int64_t n, float *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int row = blockIdx.y;
    out[(size_t)row * n + i] = emit_sample(acc, acc_cap, n_sources, channels, row, i, passes, 0, n_passes, segs, 0, n_segs, weights,
                                           weights_cap, scales, n_members, shifts, bag, stats);
}

// mi_streams_emit: stream_emit_kernel over a table of streams.  grid (ceil(max_n / 256), n_sources * channels, n_streams); a stream's
// row, pass range, segment range, stats pair and output span are clamped to the declared table sizes and capacities.
__global__ __launch_bounds__(256) void streams_emit_kernel(const float *__restrict__ acc, int64_t acc_cap, int n_sources, int channels,
                                                           const int64_t *__restrict__ streams, const int64_t *__restrict__ passes,
                                                           int n_passes, const int64_t *__restrict__ segs, int n_segs,
                                                           const float *__restrict__ weights, int64_t weights_cap,
                                                           const float *__restrict__ scales, int n_members, int shifts, int bag,
                                                           const float *__restrict__ stats, int n_stats, float *__restrict__ out,
                                                           int64_t out_cap) {
    const int64_t *t = streams + (size_t)blockIdx.z * MI_STREAMS_EMIT_COLS;
    const int64_t n = t[MI_STREAMS_EMIT_N], off = t[MI_STREAMS_EMIT_OUT_OFF];
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int row = blockIdx.y, rows = n_sources * channels;
    if (i >= n || n > out_cap || off < 0 || off > out_cap - (int64_t)rows * n) return;
    auto clamp = [](int64_t v, int64_t lo, int64_t hi) { return v < lo ? lo : v > hi ? hi : v; };
    const int p_lo = (int)clamp(t[MI_STREAMS_EMIT_PASS_LO], 0, n_passes);
    const int p_hi = (int)clamp(t[MI_STREAMS_EMIT_PASS_HI], p_lo, n_passes);
    const int64_t s_lo = clamp(t[MI_STREAMS_EMIT_SEG_LO], 0, n_segs);
    const int64_t s_hi = clamp(t[MI_STREAMS_EMIT_SEG_HI], s_lo, n_segs);
    const int64_t si = t[MI_STREAMS_EMIT_STATS];
    const float *st = stats && si >= 0 && si < n_stats ? stats + 2 * si : nullptr;
    out[off + (int64_t)row * n + i] = emit_sample(acc, acc_cap, n_sources, channels, row, i, passes, p_lo, p_hi, segs, s_lo, s_hi,
                                                  weights, weights_cap, scales, n_members, shifts, bag, st);
}

// mi_streams_append: row (stream, channel) of the table; four consecutive new samples per thread.  Sample j of the block's channel c
// (at src + c * n + j) goes to window column col + j of row c of the (channels, dst_len) window at float offset dst_off, through
// `(x - mean) / s` (track_affine_kernel mode 0) when the stream has a stats pair.  grid (ceil(max_n / 1024), n_streams * channels)
__global__ __launch_bounds__(256) void streams_append_kernel(float *__restrict__ win, int64_t win_cap, int channels,
                                                             const int64_t *__restrict__ table, const float *__restrict__ stats,
                                                             int n_stats) {
    const int s = blockIdx.y / channels, c = blockIdx.y % channels;
    const int64_t *t = table + (size_t)s * MI_APPEND_COLS;
    const int64_t n = t[MI_APPEND_N], dst_off = t[MI_APPEND_DST_OFF], dst_len = t[MI_APPEND_DST_LEN], col = t[MI_APPEND_COL];
    if (n <= 0 || dst_len < 0 || dst_len > win_cap || dst_off < 0 || dst_off > win_cap - (int64_t)channels * dst_len || col < 0 ||
        col > dst_len)
        return;
    const float *src = reinterpret_cast<const float *>(static_cast<uintptr_t>(t[MI_APPEND_SRC])) + (int64_t)c * n;
    const int64_t si = t[MI_APPEND_STATS];
    const bool aff = stats && si >= 0 && si < n_stats;
    const float mean = aff ? stats[2 * si] : 0.f, sd = aff ? stats[2 * si + 1] : 1.f;
    float *dst = win + dst_off + (int64_t)c * dst_len + col;
    const int64_t room = dst_len - col;
    const int64_t j0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int64_t j = j0 + e;
        if (j < n && j < room) {
            const float v = src[j];
            dst[j] = aff ? __fdiv_rn(__fsub_rn(v, mean), sd) : v;
        }
    }
}

// mi_streams_compact: row r of the table copies n floats from src_off of `src` to dst_off of `dst`, then writes zeros up to len floats.
// grid (min(ceil(max_len / 1024), 1024), n_rows), grid-stride over a row's floats
__global__ __launch_bounds__(256) void streams_compact_kernel(float *__restrict__ dst, int64_t dst_cap, const float *__restrict__ src,
                                                              int64_t src_cap, const int64_t *__restrict__ table) {
    const int64_t *t = table + (size_t)blockIdx.y * MI_COMPACT_COLS;
    const int64_t src_off = t[MI_COMPACT_SRC_OFF], dst_off = t[MI_COMPACT_DST_OFF];
    int64_t n = t[MI_COMPACT_N], len = t[MI_COMPACT_LEN];
    if (dst_off < 0 || dst_off > dst_cap || len <= 0) return;
    len = len < dst_cap - dst_off ? len : dst_cap - dst_off;
    const bool src_ok = src_off >= 0 && src_off <= src_cap;
    n = !src_ok || n < 0 ? 0 : n < src_cap - src_off ? n : src_cap - src_off;
    for (int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x; j < len; j += (int64_t)gridDim.x * 256)
        dst[dst_off + j] = j < n ? src[src_off + j] : 0.f;
}

int launch_stream_emit(const float *acc, int64_t acc_cap, int n_sources, int channels, const int64_t *passes, int n_passes,
                       const int64_t *segs, int n_segs, const float *weights, int64_t weights_cap, const float *scales, int n_members,
                       int shifts, int bag, const float *stats, int64_t n, float *out, hipStream_t st) {
    hipLaunchKernelGGL(stream_emit_kernel, dim3(ceil_div(n, 256), n_sources * channels), dim3(256), 0, st, acc, acc_cap, n_sources,
                       channels, passes, n_passes, segs, n_segs, weights, weights_cap, scales, n_members, shifts, bag, stats, n, out);
    MI_CHECK_LAUNCH();
    return MI_OK;
}

int launch_streams_emit(const float *acc, int64_t acc_cap, int n_sources, int channels, const int64_t *streams, int n_streams, int64_t max_n,
                        const int64_t *passes, int n_passes, const int64_t *segs, int n_segs, const float *weights, int64_t weights_cap,
                        const float *scales, int n_members, int shifts, int bag, const float *stats, int n_stats, float *out,
                        int64_t out_cap, hipStream_t st) {
    hipLaunchKernelGGL(streams_emit_kernel, dim3(ceil_div(max_n, 256), n_sources * channels, n_streams), dim3(256), 0, st, acc, acc_cap,
                       n_sources, channels, streams, passes, n_passes, segs, n_segs, weights, weights_cap, scales, n_members, shifts, bag,
                       stats, n_stats, out, out_cap);
    MI_CHECK_LAUNCH();
    return MI_OK;
}

int launch_streams_append(float *win, int64_t win_cap, int channels, const int64_t *table, int n_streams, int64_t max_n,
                          const float *stats, int n_stats, hipStream_t st) {
    hipLaunchKernelGGL(streams_append_kernel, dim3(ceil_div(max_n, 1024), n_streams * channels), dim3(256), 0, st, win, win_cap, channels,
                       table, stats, n_stats);
    MI_CHECK_LAUNCH();
    return MI_OK;
}

int launch_streams_compact(float *dst, int64_t dst_cap, const float *src, int64_t src_cap, const int64_t *table, int n_rows, int64_t max_len,
                           hipStream_t st) {
    hipLaunchKernelGGL(streams_compact_kernel, dim3(std::min(ceil_div(max_len, 1024), 1024), n_rows), dim3(256), 0, st, dst, dst_cap, src,
                       src_cap, table);
    MI_CHECK_LAUNCH();
    return MI_OK;
}

}  // namespace mi
