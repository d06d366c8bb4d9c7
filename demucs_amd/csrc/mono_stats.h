// The arithmetic of the track statistics, spelled once for post.hip (mi_mono_stats: the whole track in one launch) and
// stats_stream.hip (mi_mono_stats_update / _finish: the same sums block by block), so both give the same bits.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mi {

constexpr int kPostBlocks = 1024;                   // partial-sum slots of the statistics pass (fixed: the result does not depend on the grid)
constexpr int kStatsSlots = kPostBlocks * 256;      // threads of that pass: position p always belongs to thread p % kStatsSlots

// One position into a thread's (s, q): ref = wav.mean(0) (float32, channel sum in ascending order then / channels, api.py:267),
// the sums of ref and ref^2 in float64.  row(c) is the position's sample of channel c.
template <class Row>
__device__ __forceinline__ void mono_stats_step(Row row, int channels, double &s, double &q) {
    float a = row(0);
    for (int c = 1; c < channels; ++c) a = __fadd_rn(a, row(c));
    const float m = __fdiv_rn(a, (float)channels);
    s += (double)m;
    q += (double)m * (double)m;
}

// The (s, q) of a block's 256 threads summed by a shared-memory tree; the sums end in sh[0][0] and sh[1][0].
__device__ __forceinline__ void mono_stats_tree(double s, double q, double (&sh)[2][256]) {
    sh[0][threadIdx.x] = s; sh[1][threadIdx.x] = q;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) { sh[0][threadIdx.x] += sh[0][threadIdx.x + w]; sh[1][threadIdx.x] += sh[1][threadIdx.x + w]; }
        __syncthreads();
    }
}

}  // namespace mi
