// Streaming `convert_audio` (demucs/audio.py:169-172) fused with a stream's append: the device side of
// `demucs_amd.audio.ConvertStream` and of the converting streams of a StreamGroup (demucs_amd/stream.py).
//
// resample.hip computes, for a whole row x of length L,
//     y[n * new + i] = fmaf chain over k = 0 .. klen - 1 ascending, acc = 0:  acc = fmaf(kernel[i][k], x[clamp(n * old - width + k, 0, L - 1)], acc)
// This kernel evaluates the same chain (every tap, ascending k, one fmaf each, the same clamped sample) for the frames n whose
// operands are known after a push (n * old + width + old <= pushed), and at the final call for the rest with the right taps
// clamped to x[L - 1]; the input a later frame still needs is carried in a small history that one launch reads on one side and
// rewrites on the other.  So the concatenation of a stream's outputs is resample.hip's result bit for bit for every partition.
//
// Shape: a workgroup takes one (stream, channel) row and a run of 8 * G consecutive frames.  It stages the run's
// `frames * old + 2 * width` input samples in LDS once, resolving history / block / clamps there, so the tap loop has no branch.
// A work item is (sub-run g of 8 frames, phase i): with the bank transposed ([klen][new]) a coefficient load is coalesced over
// the phases and feeds the item's 8 accumulators, the input reads are LDS broadcasts, and the output stores are coalesced.
// Memory bound on paper (4 B in / 4 B out per sample, the bank stays in L2); the tap loop is LDS-issue bound.
#include "common.h"
#include "kernels.h"
#include "pcm_ingest.h"

namespace mi {

constexpr int CVT_F = 8;            // frames (accumulators) per work item
constexpr int CVT_G = 4;            // at most this many sub-runs per workgroup
constexpr int CVT_COPY_SPAN = 1024; // equal rates: samples per workgroup

// sub-runs per workgroup for a rate entry: as many as the LDS staging area holds (demucs_amd/audio.py computes the same)
__host__ __device__ inline int cvt_subruns(int64_t old_sr, int64_t width, int lds_floats) {
    const int64_t g = (lds_floats - 2 * width) / (CVT_F * old_sr);
    return (int)(g > CVT_G ? CVT_G : g);
}

// One body for both entries: PCM = false is mi_streams_convert_append (rows of MI_CVT_COLS, every block planar float32), PCM = true
// mi_streams_convert_append_pcm (rows of MI_CVT_PCM_COLS, whose FMT column names the block's format).  Only `block(i)`, the read of
// input sample P0 + i of this row, depends on the format; the history (float32), the tap loop, `ready` and the staging are the same code.
template <bool PCM>
__global__ __launch_bounds__(256) void streams_convert_append_kernel(float *__restrict__ win, int64_t win_cap, int channels,
                                                                     const int64_t *__restrict__ table,
                                                                     const float *__restrict__ bank, int64_t bank_cap,
                                                                     float *__restrict__ hist, int64_t hist_cap,
                                                                     const float *__restrict__ stats, int n_stats, int lds_floats) {
    extern __shared__ float xs[];
    const int s = blockIdx.y / channels, c = blockIdx.y % channels;
    const int64_t *t = table + (size_t)s * (PCM ? MI_CVT_PCM_COLS : MI_CVT_COLS);
    const int64_t n_in = t[MI_CVT_N_IN], src_ch = t[MI_CVT_SRC_CH], P0 = t[MI_CVT_BEFORE];
    const int64_t h_len = t[MI_CVT_HIST_LEN], h_rd = t[MI_CVT_HIST_RD], h_wr = t[MI_CVT_HIST_WR];
    const int64_t h0 = t[MI_CVT_HIST_START], h1 = t[MI_CVT_HIST_NEXT];
    const int64_t out0 = t[MI_CVT_OUT0], n_out = t[MI_CVT_N_OUT], total = t[MI_CVT_TOTAL];
    const int64_t old_sr = t[MI_CVT_OLD], new_sr = t[MI_CVT_NEW], width = t[MI_CVT_WIDTH], bank_off = t[MI_CVT_BANK_OFF];
    const int64_t dst_off = t[MI_CVT_DST_OFF], dst_len = t[MI_CVT_DST_LEN], col = t[MI_CVT_COL];
    if (n_in < 0 || src_ch < 1 || P0 < 0 || out0 < 0 || old_sr < 1 || new_sr < 1 || width < 0 || old_sr > lds_floats ||
        width > lds_floats || new_sr > (1 << 24))
        return;
    const bool copy = width == 0;                            // equal rates: the channel map alone
    const bool h_ok = h_len > 0 && h_len <= hist_cap;
    const bool rd_ok = h_ok && h_rd >= 0 && h_rd <= hist_cap - (int64_t)channels * h_len;
    const bool wr_ok = h_ok && h_wr >= 0 && h_wr <= hist_cap - (int64_t)channels * h_len;
    const int64_t srow = src_ch == 1 ? 0 : (c < src_ch ? c : src_ch - 1);      // mono feeds every row; else the first `channels` rows
    const uintptr_t addr = static_cast<uintptr_t>(t[MI_CVT_SRC]);
    const float *src = reinterpret_cast<const float *>(addr) + srow * n_in;
    const int fmt = PCM ? (int)t[MI_CVT_PCM_FMT] : MI_PCM_PLANAR;
    const bool wire = PCM && fmt != MI_PCM_PLANAR;          // interleaved wire frames: pcm_ingest.h reads them
    if (wire && (t[MI_CVT_PCM_FMT] != fmt || !pcm_source_ok(fmt, src_ch, addr))) return;
    auto block = [&](int64_t i) -> float {
        return wire ? pcm_sample(reinterpret_cast<const unsigned char *>(addr), fmt, src_ch, i, srow) : src[i];
    };
    const float *hr = hist + (rd_ok ? h_rd + (int64_t)c * h_len : 0);
    // input sample j of this row: from the block when it starts at or after P0, else from the read side of the history
    auto sample = [&](int64_t j) -> float {
        if (j >= P0) return j - P0 < n_in ? block(j - P0) : 0.f;
        const int64_t r = j - h0;
        return rd_ok && r >= 0 && r < h_len ? hr[r] : 0.f;
    };
    // the write side of the history: inputs [h1, P0 + n_in), what the next frame still needs
    if (blockIdx.x == 0 && wr_ok && h1 >= 0) {
        float *hw = hist + h_wr + (int64_t)c * h_len;
        int64_t n = P0 + n_in - h1;
        n = n < h_len ? n : h_len;
        for (int64_t r = threadIdx.x; r < n; r += 256) hw[r] = sample(h1 + r);
    }
    if (n_out <= 0 || dst_len < 0 || dst_len > win_cap || dst_off < 0 || dst_off > win_cap - (int64_t)channels * dst_len || col < 0 ||
        col > dst_len)
        return;
    const int64_t si = t[MI_CVT_STATS];
    const bool aff = stats && si >= 0 && si < n_stats;
    const float mean = aff ? stats[2 * si] : 0.f, sd = aff ? stats[2 * si + 1] : 1.f;
    float *dst = win + dst_off + (int64_t)c * dst_len + col;
    const int64_t room = dst_len - col;
    if (copy) {
        const int64_t r0 = (int64_t)blockIdx.x * CVT_COPY_SPAN + threadIdx.x;
#pragma unroll
        for (int e = 0; e < CVT_COPY_SPAN / 256; ++e) {
            const int64_t r = r0 + e * 256;
            if (r < n_out && r < room) {
                const float v = sample(out0 + r);
                dst[r] = aff ? __fdiv_rn(__fsub_rn(v, mean), sd) : v;
            }
        }
        return;
    }
    const int G = cvt_subruns(old_sr, width, lds_floats);
    const int klen = (int)(2 * width + old_sr), nsr = (int)new_sr, osr = (int)old_sr;
    if (G < 1 || bank_off < 0 || bank_off > bank_cap - (int64_t)klen * nsr) return;
    const int64_t frames = (n_out + new_sr - 1) / new_sr;
    const int64_t fA = (int64_t)blockIdx.x * (CVT_F * G);     // first frame of this workgroup, counted from the call's first
    if (fA >= frames) return;
    const int nf = (int)(frames - fA < CVT_F * G ? frames - fA : CVT_F * G);
    const int64_t nA = out0 / new_sr + fA;
    const int64_t base_in = nA * old_sr - width;              // xpad[j] = x[clamp(j - width)]
    const int span = nf * osr + (int)(2 * width);
    for (int idx = threadIdx.x; idx < span; idx += 256) {
        int64_t j = base_in + idx;
        j = j < 0 ? 0 : j;
        if (total >= 0 && j > total - 1) j = total - 1;
        xs[idx] = sample(j);
    }
    __syncthreads();
    const float *bk = bank + bank_off;
    for (int w = threadIdx.x; w < G * nsr; w += 256) {
        const int g = w / nsr, i = w - g * nsr;
        const int f0 = g * CVT_F;
        if (f0 >= nf) continue;
        // frames past nf read staged-area floats no frame owns (inside the allocation: G comes from lds_floats); never stored
        const float *xb = xs + f0 * osr;
        const float *kb = bk + i;
        float acc[CVT_F];
#pragma unroll
        for (int f = 0; f < CVT_F; ++f) acc[f] = 0.f;
        for (int k = 0; k < klen; ++k) {
            const float cf = kb[(size_t)k * nsr];
#pragma unroll
            for (int f = 0; f < CVT_F; ++f) acc[f] = fmaf(cf, xb[f * osr + k], acc[f]);
        }
#pragma unroll
        for (int f = 0; f < CVT_F; ++f) {
            const int64_t r = (fA + f0 + f) * new_sr + i + (out0 / new_sr) * new_sr - out0;
            if (f0 + f < nf && r >= 0 && r < n_out && r < room) dst[r] = aff ? __fdiv_rn(__fsub_rn(acc[f], mean), sd) : acc[f];
        }
    }
}

int launch_streams_convert_append(float *win, int64_t win_cap, int channels, const int64_t *table, int n_streams, int64_t max_groups,
                                  const float *bank, int64_t bank_cap, float *hist, int64_t hist_cap, const float *stats, int n_stats,
                                  int lds_floats, hipStream_t st) {
    hipLaunchKernelGGL(streams_convert_append_kernel<false>, dim3((unsigned)max_groups, n_streams * channels), dim3(256),
                       (size_t)lds_floats * sizeof(float), st, win, win_cap, channels, table, bank, bank_cap, hist, hist_cap, stats,
                       n_stats, lds_floats);
    MI_CHECK_LAUNCH();
    return MI_OK;
}

int launch_streams_convert_append_pcm(float *win, int64_t win_cap, int channels, const int64_t *table, int n_streams,
                                      int64_t max_groups, const float *bank, int64_t bank_cap, float *hist, int64_t hist_cap,
                                      const float *stats, int n_stats, int lds_floats, hipStream_t st) {
    hipLaunchKernelGGL(streams_convert_append_kernel<true>, dim3((unsigned)max_groups, n_streams * channels), dim3(256),
                       (size_t)lds_floats * sizeof(float), st, win, win_cap, channels, table, bank, bank_cap, hist, hist_cap, stats,
                       n_stats, lds_floats);
    MI_CHECK_LAUNCH();
    return MI_OK;
}

}  // namespace mi
