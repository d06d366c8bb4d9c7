// Delivery of a stream's stems at another sample rate: what a user of the reference writes to save a stem at rate R,
// `save_audio(julius.resample_frac(v, M, R), path, samplerate=R, clip=...)` (demucs/audio.py:169-172,175-181,218-265 on the
// outputs of demucs/separate.py:178-218), for EVERY resampling output of a call in one table-driven launch
// (include/demucs_amd.h, MI_RATE_*).
//
// Per output the value v at the model's rate is deliver.hip's (a stem, or 0 + the other stems in index order: post_ops.h), and
// every resampled sample is convert_stream.hip's chain on it,
//     y[n * new + i] = fmaf chain over k = 0 .. klen - 1 ascending, acc = 0:  acc = fmaf(kernel[i][k], v[clamp(n * old - width + k, 0, L - 1)], acc)
// for the frames n whose last tap the stream has emitted (n * old + width + old <= emitted), and at the final call for the rest
// with the right taps clamped to v[L - 1]; then post_ops.h's clip_sample and pcm_i16 (or the float), channels interleaved.  The
// VALUES a later frame still needs are carried in a small two-sided history per output, read on one side and rewritten on the
// other by one launch, so the concatenation of a stream's frames is the whole-track chain bit for bit for every partition.
//
// Shape: a workgroup takes one row (one output) and a run of 8 * G consecutive frames, for all channels.  It stages the run's
// `frames * old + 2 * width` values per channel in LDS once, resolving history / stems / two-stems / clamps there, so the tap
// loop has no branch.  A work item is (sub-run g of 8 frames, phase i): with the bank transposed ([klen][new]) a coefficient load
// is coalesced over the phases and feeds the item's 8 accumulators of each channel, the value reads are LDS broadcasts, and an
// int16 stereo frame is one 4-byte store, coalesced over the phases.  Memory bound on paper; the tap loop is LDS-issue bound.
//
// "rescale" (v / max(1.01 * peak, 1), the peak that of the whole resampled output) takes two passes over a stream: the same body
// instantiated to MEASURE keeps the running max |frame| per output in a slot of peaks (mi_deliver_resample_peaks), and
// instantiated to deliver with peaks divides by what an earlier pass measured (mi_deliver_resample_pcm_peaks).
#include "common.h"
#include "kernels.h"
#include "post_ops.h"

namespace mi {

constexpr int RATE_F = 8;            // frames (accumulators per channel) per work item
constexpr int RATE_G = 4;            // at most this many sub-runs per workgroup

// sub-runs per workgroup for a rate entry: as many as the LDS staging area holds for all channels (demucs_amd/audio.py computes
// the same)
__host__ __device__ inline int rate_subruns(int64_t old_sr, int64_t width, int channels, int lds_floats) {
    const int64_t g = (lds_floats / channels - 2 * width) / (RATE_F * old_sr);
    return (int)(g > RATE_G ? RATE_G : g);
}

// the tap chains of NC channels of one work item: coefficient k of phase i at kb[k * nsr], channel c's staged values at xb + c * cs
template <int NC>
__device__ __forceinline__ void rate_taps(const float *__restrict__ kb, int nsr, int klen, const float *xb, int cs, int osr,
                                          float (&acc)[NC][RATE_F]) {
#pragma unroll
    for (int c = 0; c < NC; ++c)
#pragma unroll
        for (int f = 0; f < RATE_F; ++f) acc[c][f] = 0.f;
    for (int k = 0; k < klen; ++k) {
        const float cf = kb[(size_t)k * nsr];
#pragma unroll
        for (int c = 0; c < NC; ++c)
#pragma unroll
            for (int f = 0; f < RATE_F; ++f) acc[c][f] = fmaf(cf, xb[c * cs + f * osr + k], acc[c][f]);
    }
}

// The three entries are this one body.  RATE_PCM is mi_deliver_resample_pcm (no "rescale": slots / peaks are not read);
// RATE_PCM_PEAKS is mi_deliver_resample_pcm_peaks, which also takes MI_CLIP_RESCALE rows and divides by the peak in the row's slot;
// RATE_MEASURE is mi_deliver_resample_peaks: the same history and the same tap chains, but the frames go into the running maximum
// of the row's slot instead of a destination (FMT and DST_OFF are not read, dst is not used)
enum { RATE_PCM = 0, RATE_PCM_PEAKS = 1, RATE_MEASURE = 2 };

template <int MODE>
__global__ __launch_bounds__(256) void deliver_resample_pcm_kernel(const int64_t *__restrict__ table, int n_sources, int channels,
                                                                   const float *__restrict__ bank, int64_t bank_cap,
                                                                   float *__restrict__ hist, int64_t hist_cap, int lds_floats,
                                                                   unsigned char *__restrict__ dst, int64_t dst_cap,
                                                                   const int32_t *__restrict__ slots, unsigned *__restrict__ peaks,
                                                                   int n_peaks) {
    extern __shared__ float xs[];
    const int64_t *t = table + (size_t)blockIdx.y * MI_RATE_COLS;
    const int64_t n_in = t[MI_RATE_N_IN], P0 = t[MI_RATE_BEFORE];
    const int64_t kind = t[MI_RATE_KIND], sel = t[MI_RATE_SEL], clip = t[MI_RATE_CLIP];
    const int64_t fmt = MODE == RATE_MEASURE ? MI_DELIVER_I16 : t[MI_RATE_FMT];
    const int64_t old_sr = t[MI_RATE_OLD], new_sr = t[MI_RATE_NEW], width = t[MI_RATE_WIDTH], bank_off = t[MI_RATE_BANK_OFF];
    const int64_t out0 = t[MI_RATE_OUT0], n_out = t[MI_RATE_N_OUT], total = t[MI_RATE_TOTAL];
    const int64_t h_len = t[MI_RATE_HIST_LEN], h_rd = t[MI_RATE_HIST_RD], h_wr = t[MI_RATE_HIST_WR];
    const int64_t h0 = t[MI_RATE_HIST_START], h1 = t[MI_RATE_HIST_NEXT];
    const int64_t dst_off = MODE == RATE_MEASURE ? 0 : t[MI_RATE_DST_OFF];
    const float *src = reinterpret_cast<const float *>(static_cast<uintptr_t>(t[MI_RATE_SRC]));
    // every rule under which a row is skipped whole (nothing of it is read or written); the same for the whole workgroup
    const bool clip_ok = MODE == RATE_MEASURE ? clip == MI_CLIP_RESCALE
                                              : clip == 0 || clip == MI_CLIP_CLAMP || clip == MI_CLIP_TANH ||
                                                    (MODE == RATE_PCM_PEAKS && clip == MI_CLIP_RESCALE);
    if (n_in < 0 || (n_in > 0 && !src) || P0 < 0 || kind < MI_DELIVER_STEM || kind > MI_DELIVER_ADD || sel < 0 || sel >= n_sources ||
        !clip_ok || fmt < MI_DELIVER_I16 || fmt > MI_DELIVER_F32)
        return;
    // a row that measures or rescales names its slot of peaks; one outside [0, n_peaks) skips the row, history included
    int slot = 0;
    if (MODE != RATE_PCM && clip == MI_CLIP_RESCALE) {
        slot = slots[blockIdx.y];
        if (slot < 0 || slot >= n_peaks) return;
    }
    if (old_sr < 1 || new_sr < 1 || new_sr > (1 << 24) || width < 1 || old_sr > lds_floats || width > lds_floats) return;
    const int G = rate_subruns(old_sr, width, channels, lds_floats);
    const int klen = (int)(2 * width + old_sr), nsr = (int)new_sr, osr = (int)old_sr;
    if (G < 1 || bank_off < 0 || bank_off > bank_cap - (int64_t)klen * nsr) return;
    if (out0 < 0 || out0 % new_sr != 0 || n_out < 0 || h0 < 0 || (total >= 0 && total != P0 + n_in)) return;
    // the history: none (a stream's only call), or both sides inside hist_cap and apart
    const int64_t side = (int64_t)channels * h_len;
    if (h_len < 0 || h_len > hist_cap) return;
    if (h_len == 0) {
        if (P0 != 0 || h1 >= 0) return;
    } else if (h_rd < 0 || h_wr < 0 || h_rd > hist_cap - side || h_wr > hist_cap - side || (h_rd < h_wr + side && h_wr < h_rd + side)) {
        return;
    }
    const int64_t frame = (int64_t)channels * (fmt == MI_DELIVER_F32 ? 4 : 2);      // bytes
    if (MODE != RATE_MEASURE && n_out > 0 &&
        (dst_off < 0 || (dst_off & 3) != 0 || n_out > dst_cap / frame || dst_off > dst_cap - n_out * frame))
        return;

    const int64_t stem_stride = (int64_t)channels * n_in;
    const float *hr = hist + h_rd;
    // the output's value at model-rate position j of channel c: from the emitted block when j >= P0, else from the history
    auto value = [&](int64_t j, int c) -> float {
        if (j >= P0) {
            const int64_t r = j - P0;
            if (r >= n_in) return 0.f;
            const float *base = src + (int64_t)c * n_in + r;
            if (kind == MI_DELIVER_STEM) return base[sel * stem_stride];
            float a[1];
            two_stems_add<1>(n_sources, (int)sel, [&](int k, float (&s)[1]) { s[0] = base[k * stem_stride]; }, a);
            return a[0];
        }
        const int64_t r = j - h0;
        return h_len > 0 && r >= 0 && r < h_len ? hr[(int64_t)c * h_len + r] : 0.f;
    };
    // the write side of the history: values [h1, P0 + n_in), what the next frame still needs
    if (blockIdx.x == 0 && h_len > 0 && h1 >= 0) {
        float *hw = hist + h_wr;
        int64_t n = P0 + n_in - h1;
        n = n < h_len ? n : h_len;
        for (int c = 0; c < channels; ++c)
            for (int64_t r = threadIdx.x; r < n; r += 256) hw[(int64_t)c * h_len + r] = value(h1 + r, c);
    }
    if (n_out <= 0) return;
    const int64_t frames = (n_out + new_sr - 1) / new_sr;
    const int64_t fA = (int64_t)blockIdx.x * (RATE_F * G);    // first frame of this workgroup, counted from the call's first
    if (fA >= frames) return;
    const int nf = (int)(frames - fA < RATE_F * G ? frames - fA : RATE_F * G);
    const int64_t base_in = (out0 / new_sr + fA) * old_sr - width;          // staged[idx] = v[clamp(base_in + idx)]
    const int span = nf * osr + (int)(2 * width);
    const int cs = RATE_F * G * osr + (int)(2 * width);                     // a channel's staging area; channels * cs <= lds_floats
    for (int c = 0; c < channels; ++c) {
        for (int idx = threadIdx.x; idx < span; idx += 256) {
            int64_t j = base_in + idx;
            j = j < 0 ? 0 : j;
            if (total >= 0 && j > total - 1) j = total - 1;
            xs[c * cs + idx] = value(j, c);
        }
    }
    __syncthreads();
    const float *bk = bank + bank_off;
    unsigned char *out = dst + dst_off;                                      // frames [0, n_out) of the row: inside dst_cap, above
    const int mode = (int)clip;
    // the divisor of a rescaling row, read once per workgroup; every other mode ignores it
    const float d = (MODE == RATE_PCM_PEAKS && clip == MI_CLIP_RESCALE) ? clip_divisor(peaks[slot]) : 0.f;
    unsigned m = 0u;                                                         // RATE_MEASURE: max |frame| over this item's frames
    for (int w = threadIdx.x; w < G * nsr; w += 256) {
        const int g = w / nsr, i = w - g * nsr;
        const int f0 = g * RATE_F;
        if (f0 >= nf) continue;
        // frames past nf read staged-area floats no frame owns (inside the channel's area: cs covers 8 * G frames); never stored
        const float *xb = xs + f0 * osr;
        const float *kb = bk + i;
        if (channels == 2) {
            float acc[2][RATE_F];
            rate_taps<2>(kb, nsr, klen, xb, cs, osr, acc);
#pragma unroll
            for (int f = 0; f < RATE_F; ++f) {
                const int64_t r = (fA + f0 + f) * new_sr + i;
                if (f0 + f >= nf || r >= n_out) continue;
                if (MODE == RATE_MEASURE) {       // only frames of this call: a lane past n_out holds taps of no data
                    m = max(m, max(abs_bits(acc[0][f]), abs_bits(acc[1][f])));
                    continue;
                }
                const float a = clip_sample(acc[0][f], mode, d), b = clip_sample(acc[1][f], mode, d);
                if (fmt == MI_DELIVER_I16) {
                    const unsigned lo = (unsigned short)pcm_i16(a), hi = (unsigned short)pcm_i16(b);
                    reinterpret_cast<unsigned *>(out)[r] = lo | (hi << 16);     // 4-byte aligned: dst is, and DST_OFF is a multiple of 4
                } else {
                    reinterpret_cast<float *>(out)[2 * r] = a;                  // DST_OFF need not be a multiple of 8
                    reinterpret_cast<float *>(out)[2 * r + 1] = b;
                }
            }
            continue;
        }
        for (int c = 0; c < channels; ++c) {
            float acc[1][RATE_F];
            rate_taps<1>(kb, nsr, klen, xb + c * cs, cs, osr, acc);
#pragma unroll
            for (int f = 0; f < RATE_F; ++f) {
                const int64_t r = (fA + f0 + f) * new_sr + i;
                if (f0 + f >= nf || r >= n_out) continue;
                if (MODE == RATE_MEASURE) {
                    m = max(m, abs_bits(acc[0][f]));
                    continue;
                }
                const float y = clip_sample(acc[0][f], mode, d);
                const int64_t at = r * channels + c;
                if (fmt == MI_DELIVER_I16) reinterpret_cast<short *>(out)[at] = pcm_i16(y);
                else reinterpret_cast<float *>(out)[at] = y;
            }
        }
    }
    if (MODE == RATE_MEASURE) {          // every work item of the workgroup arrives here: the returns above are per workgroup
        for (int o = 32; o > 0; o >>= 1) m = max(m, (unsigned)__shfl_xor((int)m, o));
        if ((threadIdx.x & 63) == 0 && m) atomicMax(peaks + slot, m);
    }
}

template <int MODE>
static int launch_rate(const int64_t *table, int n_rows, int64_t max_groups, int n_sources, int channels, const float *bank,
                       int64_t bank_cap, float *hist, int64_t hist_cap, int lds_floats, unsigned char *dst, int64_t dst_cap,
                       const int32_t *slots, unsigned *peaks, int n_peaks, hipStream_t st) {
    hipLaunchKernelGGL(deliver_resample_pcm_kernel<MODE>, dim3((unsigned)max_groups, n_rows), dim3(256),
                       (size_t)lds_floats * sizeof(float), st, table, n_sources, channels, bank, bank_cap, hist, hist_cap, lds_floats, dst,
                       dst_cap, slots, peaks, n_peaks);
    MI_CHECK_LAUNCH();
    return MI_OK;
}

int launch_deliver_resample_pcm(const int64_t *table, int n_rows, int64_t max_groups, int n_sources, int channels, const float *bank,
                                int64_t bank_cap, float *hist, int64_t hist_cap, int lds_floats, unsigned char *dst, int64_t dst_cap,
                                hipStream_t st) {
    return launch_rate<RATE_PCM>(table, n_rows, max_groups, n_sources, channels, bank, bank_cap, hist, hist_cap, lds_floats, dst, dst_cap,
                                 nullptr, nullptr, 0, st);
}

int launch_deliver_resample_pcm_peaks(const int64_t *table, int n_rows, int64_t max_groups, int n_sources, int channels,
                                      const float *bank, int64_t bank_cap, float *hist, int64_t hist_cap, int lds_floats, unsigned char *dst,
                                      int64_t dst_cap, const int32_t *slots, const unsigned *peaks, int n_peaks, hipStream_t st) {
    return launch_rate<RATE_PCM_PEAKS>(table, n_rows, max_groups, n_sources, channels, bank, bank_cap, hist, hist_cap, lds_floats, dst,
                                       dst_cap, slots, const_cast<unsigned *>(peaks), n_peaks, st);       // only read in this mode
}

int launch_deliver_resample_peaks(const int64_t *table, int n_rows, int64_t max_groups, int n_sources, int channels, const float *bank,
                                  int64_t bank_cap, float *hist, int64_t hist_cap, int lds_floats, const int32_t *slots, unsigned *peaks,
                                  int n_peaks, hipStream_t st) {
    return launch_rate<RATE_MEASURE>(table, n_rows, max_groups, n_sources, channels, bank, bank_cap, hist, hist_cap, lds_floats, nullptr,
                                     0, slots, peaks, n_peaks, st);
}

}  // namespace mi
