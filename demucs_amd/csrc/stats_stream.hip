// Track statistics for a track that arrives block by block: mi_mono_stats' sums, carried between the blocks.
//
// mono_stats_partial_kernel (post.hip) runs on a fixed grid of kStatsSlots = kPostBlocks x 256 threads: position p of the track
// always belongs to thread p % kStatsSlots, and a thread adds its positions in ascending order in float64.  So the only state a
// block-by-block evaluation has to carry is one (s, q) pair of doubles per thread ("slot"), 4 MiB in all: the update kernel adds
// a block's positions to their slots in the order the one-shot kernel would, and the finish kernel reduces the slots of block b
// with that kernel's shared-memory tree before mono_stats_final_kernel runs as it is.  The arithmetic is mono_stats.h's in both
// files, so the result has the one-shot kernel's bits for every partition of the track.
//
// A block is planar float32 (channels, n) or n interleaved wire PCM frames (pcm_ingest.h), read where they lie: the analysis
// pass of a PCM feed needs no planar copy.  HBM bound and small: a 1 s stereo int16 block is 176 KB in, and the slots it touches
// (16 B each) are read and written once.
#include <algorithm>

#include "common.h"
#include "kernels.h"
#include "mono_stats.h"
#include "pcm_ingest.h"

namespace mi {

// mi_mono_stats_update: grid (ceil(min(n, kStatsSlots) / 256)).  Thread g takes the block's positions g, g + kStatsSlots, ...
// (track positions before + g, ...): all of one slot, and no other thread's.  state: kStatsSlots x (s, q)
__global__ __launch_bounds__(256) void mono_stats_update_kernel(const unsigned char *__restrict__ src, int fmt, int src_ch, int64_t n,
                                                                int channels, int64_t before, double *__restrict__ state) {
    const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (g >= n || g >= kStatsSlots) return;
    const int64_t slot = (before % kStatsSlots + g) % kStatsSlots;
    double s = state[2 * slot], q = state[2 * slot + 1];
    if (fmt == MI_PCM_PLANAR) {
        const float *wav = reinterpret_cast<const float *>(src);
        for (int64_t j = g; j < n; j += kStatsSlots)
            mono_stats_step([&](int c) { return wav[(int64_t)c * n + j]; }, channels, s, q);
    } else {
        const int spread = src_ch == 1 ? 0 : 1;            // a mono source feeds every row; else row c reads channel c
        for (int64_t j = g; j < n; j += kStatsSlots)
            mono_stats_step([&](int c) { return pcm_sample(src, fmt, src_ch, j, spread * c); }, channels, s, q);
    }
    state[2 * slot] = s;
    state[2 * slot + 1] = q;
}

// mi_mono_stats_finish, first kernel: grid kPostBlocks x 256; block b sums its threads' slots as mono_stats_partial_kernel does
__global__ __launch_bounds__(256) void mono_stats_slots_kernel(const double *__restrict__ state, double *__restrict__ part) {
    const int slot = blockIdx.x * 256 + threadIdx.x;
    __shared__ double sh[2][256];
    mono_stats_tree(state[2 * slot], state[2 * slot + 1], sh);
    if (threadIdx.x == 0) { part[2 * blockIdx.x] = sh[0][0]; part[2 * blockIdx.x + 1] = sh[1][0]; }
}

int mono_stats_state_bytes() { return kStatsSlots * 2 * (int)sizeof(double); }

int launch_mono_stats_update(const unsigned char *src, int fmt, int src_ch, int64_t n, int channels, int64_t before, double *state,
                             hipStream_t st) {
    const int64_t slots = std::min<int64_t>(n, kStatsSlots);
    hipLaunchKernelGGL(mono_stats_update_kernel, dim3(ceil_div(slots, 256)), dim3(256), 0, st, src, fmt, src_ch, n, channels, before,
                       state);
    MI_CHECK_LAUNCH();
    return MI_OK;
}

int launch_mono_stats_finish(const double *state, int64_t length, double *scratch, float *stats, hipStream_t st) {
    hipLaunchKernelGGL(mono_stats_slots_kernel, dim3(kPostBlocks), dim3(256), 0, st, state, scratch);
    MI_CHECK_LAUNCH();
    return launch_mono_stats_final(scratch, length, stats, st);
}

}  // namespace mi
