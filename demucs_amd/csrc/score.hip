// nSDR scoring of separated stems against reference stems (demucs/evaluate.py:30-43, `new_sdr`): the two float64 sums per source,
// for a whole track or block by block with the same bits (sdr_sums.h has the arithmetic and the order of summation).
//
// sdr_update_kernel runs on at most kSdrSlots threads: thread g of a block of n positions takes the block's positions g,
// g + kSdrSlots, ... -- all of one slot, and no other thread's -- so a slot has one owner per launch and its (num, den) pairs
// travel through the thread's registers with plain float64 adds, no atomics.  The estimates are planar float32 rows with an
// explicit stride, read where they lie (the span a stream has just emitted, a slice of a longer tensor); the references are
// the same, or one block of interleaved wire PCM frames per source (pcm_ingest.h), MusDB's stems being separate files.
// sdr_slots_kernel and sdr_final_kernel reduce the slots on fixed grids; they only read the state.  mi_sdr is a memset, one
// update and the finish per track.  HBM bound: every sample is read once, and a block touches the state of the slots it reaches.
#include <algorithm>

#include "common.h"
#include "kernels.h"
#include "pcm_ingest.h"
#include "sdr_sums.h"

namespace mi {

struct SdrRefs { const unsigned char *p[kSdrMaxSources]; };     // planar: p[0] is the (S, C) rows' base; PCM: one block per source

// grid (ceil(min(n, kSdrSlots) / 256)).  state: [S][2][kSdrSlots] doubles
template <int S>
__global__ __launch_bounds__(256) void sdr_update_kernel(SdrRefs refs, int fmt, int src_ch, int64_t ref_stride, const float *__restrict__ est,
                                                         int64_t est_stride, int channels, int64_t n, int64_t before,
                                                         double *__restrict__ state) {
    const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (g >= n || g >= kSdrSlots) return;
    const int64_t slot = (before % kSdrSlots + g) % kSdrSlots;
    double num[S], den[S];
#pragma unroll
    for (int s = 0; s < S; ++s) {
        num[s] = state[(int64_t)(2 * s) * kSdrSlots + slot];
        den[s] = state[(int64_t)(2 * s + 1) * kSdrSlots + slot];
    }
    if (fmt == MI_PCM_PLANAR) {
        const float *__restrict__ ref = reinterpret_cast<const float *>(refs.p[0]);
        for (int64_t j = g; j < n; j += kSdrSlots)
            for (int c = 0; c < channels; ++c) {
#pragma unroll
                for (int s = 0; s < S; ++s) {
                    const int64_t row = (int64_t)s * channels + c;
                    sdr_step(ref[row * ref_stride + j], est[row * est_stride + j], num[s], den[s]);
                }
            }
    } else {
        const int spread = src_ch == 1 ? 0 : 1;            // a mono source feeds every channel; else channel c reads channel c
        for (int64_t j = g; j < n; j += kSdrSlots)
            for (int c = 0; c < channels; ++c) {
#pragma unroll
                for (int s = 0; s < S; ++s)
                    sdr_step(pcm_sample(refs.p[s], fmt, src_ch, j, spread * c), est[((int64_t)s * channels + c) * est_stride + j], num[s],
                             den[s]);
            }
    }
#pragma unroll
    for (int s = 0; s < S; ++s) {
        state[(int64_t)(2 * s) * kSdrSlots + slot] = num[s];
        state[(int64_t)(2 * s + 1) * kSdrSlots + slot] = den[s];
    }
}

// grid (kSdrBlocks, 2 S): block (b, q) sums the 256 slots of quantity q = 2 s + {num: 0, den: 1} that start at 256 b
__global__ __launch_bounds__(256) void sdr_slots_kernel(const double *__restrict__ state, double *__restrict__ part) {
    __shared__ double sh[256];
    sdr_tree(state[(int64_t)blockIdx.y * kSdrSlots + blockIdx.x * 256 + threadIdx.x], sh);
    if (threadIdx.x == 0) part[blockIdx.y * kSdrBlocks + blockIdx.x] = sh[0];
}

// grid (2 S): the kSdrBlocks partial sums of quantity q, t + (t + 256) first, then the tree; sums[s][2] = (num, den)
__global__ __launch_bounds__(256) void sdr_final_kernel(const double *__restrict__ part, double *__restrict__ sums) {
    static_assert(kSdrBlocks == 512, "two partial sums per thread");
    __shared__ double sh[256];
    const double *p = part + blockIdx.x * kSdrBlocks;
    sdr_tree(p[threadIdx.x] + p[threadIdx.x + 256], sh);
    if (threadIdx.x == 0) sums[blockIdx.x] = sh[0];
}

int64_t sdr_state_bytes(int n_sources) { return (int64_t)n_sources * 2 * kSdrSlots * (int64_t)sizeof(double); }
int64_t sdr_scratch_bytes(int n_sources) { return (int64_t)n_sources * 2 * kSdrBlocks * (int64_t)sizeof(double); }

template <int S>
static void sdr_update_launch(const SdrRefs &refs, int fmt, int src_ch, int64_t ref_stride, const float *est, int64_t est_stride, int channels,
                              int64_t n, int64_t before, double *state, hipStream_t st) {
    const int64_t slots = std::min<int64_t>(n, kSdrSlots);
    hipLaunchKernelGGL(sdr_update_kernel<S>, dim3(ceil_div(slots, 256)), dim3(256), 0, st, refs, fmt, src_ch, ref_stride, est, est_stride,
                       channels, n, before, state);
}

int launch_sdr_update(const void *const *refs, int fmt, int src_ch, int64_t ref_stride, const float *est, int64_t est_stride, int n_sources,
                      int channels, int64_t n, int64_t before, double *state, hipStream_t st) {
    SdrRefs r{};
    for (int s = 0; s < (fmt == MI_PCM_PLANAR ? 1 : n_sources); ++s) r.p[s] = (const unsigned char *)refs[s];
    switch (n_sources) {
#define MI_SDR_CASE(S) case S: sdr_update_launch<S>(r, fmt, src_ch, ref_stride, est, est_stride, channels, n, before, state, st); break;
        MI_SDR_CASE(1) MI_SDR_CASE(2) MI_SDR_CASE(3) MI_SDR_CASE(4) MI_SDR_CASE(5) MI_SDR_CASE(6) MI_SDR_CASE(7) MI_SDR_CASE(8)
#undef MI_SDR_CASE
        default: return set_error(MI_EINVAL, "mi_sdr_update: %d sources", n_sources);
    }
    MI_CHECK_LAUNCH();
    return MI_OK;
}

int launch_sdr_finish(const double *state, int n_sources, double *scratch, double *sums, hipStream_t st) {
    hipLaunchKernelGGL(sdr_slots_kernel, dim3(kSdrBlocks, 2 * n_sources), dim3(256), 0, st, state, scratch);
    MI_CHECK_LAUNCH();
    hipLaunchKernelGGL(sdr_final_kernel, dim3(2 * n_sources), dim3(256), 0, st, scratch, sums);
    MI_CHECK_LAUNCH();
    return MI_OK;
}

int launch_sdr(const float *ref, const float *est, int B, int n_sources, int channels, int64_t length, double *state, double *scratch,
               double *sums, hipStream_t st) {
    const int64_t track = (int64_t)n_sources * channels * length;
    for (int b = 0; b < B; ++b) {
        MI_HIP(hipMemsetAsync(state, 0, (size_t)sdr_state_bytes(n_sources), st));
        if (length > 0) {
            const void *base = ref + b * track;
            MI_TRY(launch_sdr_update(&base, MI_PCM_PLANAR, 1, length, est + b * track, length, n_sources, channels, length, 0, state, st));
        }
        MI_TRY(launch_sdr_finish(state, n_sources, scratch, sums + (int64_t)b * 2 * n_sources, st));
    }
    return MI_OK;
}

}  // namespace mi
