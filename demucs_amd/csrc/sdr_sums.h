// The arithmetic of the nSDR sums (demucs/evaluate.py:30-43, `new_sdr`), spelled once for score.hip's kernels:
//   num[s] = sum r * r,  den[s] = sum (r - e) * (r - e),  r = (double)ref[s, c, p], e = (double)est[s, c, p]
// over channels c and positions p, both in float64.
//
// Order of summation.  Position p of the track belongs to slot p % kSdrSlots; a slot adds its positions in ascending order and,
// within a position, its channels in ascending order; the sources are independent sums.  kSdrSlots is a constant of the build:
// it depends neither on the grid, nor on the block size, nor on the length of a block, so the carried (num, den) of a slot is
// the same whatever partition of the track reached it.  The finish step reduces the slots with a fixed tree (256 consecutive
// slots by sdr_tree, the 512 partial sums t + (t + 256) and sdr_tree again).
//
// kSdrSlots = 131 072 = 512 blocks x 256 threads: two blocks (eight waves, two per SIMD) on each of the MI355X's 256 CUs.  One
// position of a 4-stem stereo pair is 16 independent 4-byte loads per thread, so the resident grid has 512 x 64 B = 32 KiB of
// loads in flight per CU -- the level at which a CU streams from HBM -- without unrolling over positions, and the 16 (8 sources:
// 32) float64 accumulators of a thread stay in registers.  More slots would buy nothing but a larger state: it is
// n_sources x 2 x kSdrSlots doubles (2 MiB per source), laid out [source][num, den][slot] so that a wave reads and writes whole
// 512-byte lines.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mi {

constexpr int kSdrBlocks = 512;                     // blocks of the slot reduction (fixed: the result does not depend on a grid)
constexpr int kSdrSlots = kSdrBlocks * 256;         // position p always belongs to slot p % kSdrSlots
constexpr int kSdrMaxSources = 8;

// One (reference, estimate) sample pair into its source's sums
__device__ __forceinline__ void sdr_step(float ref, float est, double &num, double &den) {
    const double r = (double)ref, d = r - (double)est;
    num += r * r;
    den += d * d;
}

// The values of a block's 256 threads summed by a shared-memory tree; the sum ends in sh[0].
__device__ __forceinline__ void sdr_tree(double v, double (&sh)[256]) {
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) sh[threadIdx.x] += sh[threadIdx.x + w];
        __syncthreads();
    }
}

}  // namespace mi
