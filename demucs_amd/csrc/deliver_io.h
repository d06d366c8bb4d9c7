// What the delivery kernels of deliver.hip (the reference's save loop) and deliver_mix.hip (gain-weighted remixes) share around
// their row's value: the loads of four consecutive samples, the wave's peak, and the clipped, converted, interleaved stores.
// A thread takes frames j0 .. j0 + 3 of every channel of its row; `values(c, v)` fills channel c's four values before clipping.
#pragma once
#include "common.h"
#include "post_ops.h"

namespace mi {

// four consecutive samples from j0 of a row of n; positions past n read nothing and give 0
__device__ __forceinline__ void load4(const float *__restrict__ p, int64_t j0, int64_t n, bool vec, float (&v)[4]) {
    if (vec) {
        const float4 q = *reinterpret_cast<const float4 *>(p + j0);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = j0 + e < n ? p[j0 + e] : 0.f;
    }
}

// max |value| of the thread's frames (none when j0 >= n), reduced over the wave, then one atomicMax per wave, none when it is 0
template <class Values>
__device__ __forceinline__ void deliver_peak4(Values values, int channels, int64_t j0, int64_t n, unsigned *__restrict__ peak) {
    unsigned m = 0u;
    if (j0 < n) {
        for (int c = 0; c < channels; ++c) {
            float v[4];
            values(c, v);                                          // positions past n give 0, which changes no maximum
#pragma unroll
            for (int e = 0; e < 4; ++e) m = max(m, abs_bits(v[e]));
        }
    }
    for (int o = 32; o > 0; o >>= 1) m = max(m, (unsigned)__shfl_xor((int)m, o));
    if ((threadIdx.x & 63) == 0 && m) atomicMax(peak, m);
}

// Stores of frames j0 .. j0 + 3 (j0 < n) into the row's (n, channels) block `out`: one 16-byte store of four frames for int16
// stereo when all four exist and their address is 16-byte aligned; else one 4-byte store per int16 stereo frame; else element by
// element.  `out` is 4-byte aligned.  i16: MI_DELIVER_I16, else float32
template <class Values>
__device__ __forceinline__ void deliver_store4(Values values, int channels, int64_t j0, int64_t n, int clip, float d, bool i16,
                                               unsigned char *__restrict__ out) {
    if (channels == 2 && i16) {
        float a[4], b[4];
        values(0, a);
        values(1, b);
        unsigned w[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const unsigned lo = (unsigned short)pcm_i16(clip_sample(a[e], clip, d)), hi = (unsigned short)pcm_i16(clip_sample(b[e], clip, d));
            w[e] = lo | (hi << 16);
        }
        unsigned *frames = reinterpret_cast<unsigned *>(out) + j0;
        if (j0 + 4 <= n && (reinterpret_cast<uintptr_t>(frames) & 15) == 0) {
            *reinterpret_cast<uint4 *>(frames) = make_uint4(w[0], w[1], w[2], w[3]);
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (j0 + e < n) frames[e] = w[e];
        }
        return;
    }
    for (int c = 0; c < channels; ++c) {
        float v[4];
        values(c, v);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if (j0 + e >= n) continue;
            const float y = clip_sample(v[e], clip, d);
            const int64_t at = (j0 + e) * channels + c;
            if (i16) reinterpret_cast<short *>(out)[at] = pcm_i16(y);
            else reinterpret_cast<float *>(out)[at] = y;
        }
    }
}

}  // namespace mi
