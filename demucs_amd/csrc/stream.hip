// Device side of the streaming scheduler (demucs_amd/stream.py): the emit step that turns the finished spans of every
// (bag member, shift pass) accumulator into final stems (reference: demucs/apply.py:201-256,297-299, demucs/api.py:285-288).
//
// The reference computes these stems over the whole track with separate torch operations: per pass `out /= sum_weight`
// (ola.hip's finish), the shift average, the bag average, the Separator's inverse affine.  Each is elementwise, so the emitted
// span can be computed on its own, and one thread runs the whole chain for one (row, sample) in the reference's order with
// every step a separately rounded float32 operation (__fadd_rn / __fmul_rn / __fdiv_rn; the library builds with
// -ffp-contract=off).  The host-scalar factors are the float32 values torch's CUDA kernels use (include/demucs_amd.h).
#include "common.h"
#include "kernels.h"

namespace mi {

// grid (ceil(n / 256), n_sources * channels); thread: output sample i = blockIdx.x * 256 + threadIdx.x of row blockIdx.y
__global__ __launch_bounds__(256) void stream_emit_kernel(const float *__restrict__ acc, int64_t acc_cap, int n_sources, int channels,
                                                          const int64_t *__restrict__ passes, int n_passes,
                                                          const int64_t *__restrict__ segs, int n_segs,
                                                          const float *__restrict__ weights, int64_t weights_cap,
                                                          const float *__restrict__ scales, int n_members, int shifts, int bag,
                                                          const float *__restrict__ stats, int64_t n, float *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int row = blockIdx.y, rows = n_sources * channels, k = row / channels;
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
    for (int p = 0; p < n_passes; ++p) {
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
        lo = lo < 0 ? 0 : lo > n_segs ? n_segs : lo;
        hi = hi < lo ? lo : hi > n_segs ? n_segs : hi;
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
    out[(size_t)row * n + i] = est;
}

int launch_stream_emit(const float *acc, int64_t acc_cap, int n_sources, int channels, const int64_t *passes, int n_passes,
                       const int64_t *segs, int n_segs, const float *weights, int64_t weights_cap, const float *scales, int n_members,
                       int shifts, int bag, const float *stats, int64_t n, float *out, hipStream_t st) {
    hipLaunchKernelGGL(stream_emit_kernel, dim3(ceil_div(n, 256), n_sources * channels), dim3(256), 0, st, acc, acc_cap, n_sources,
                       channels, passes, n_passes, segs, n_segs, weights, weights_cap, scales, n_members, shifts, bag, stats, n, out);
    MI_CHECK_LAUNCH();
    return MI_OK;
}

}  // namespace mi
