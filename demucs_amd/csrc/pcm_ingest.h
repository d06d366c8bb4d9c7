// Wire PCM in: the one conversion from little-endian interleaved int16 / packed int24 / float32 frames to the float32 samples the
// streams keep, shared by ingest.hip (mi_pcm_planar, mi_streams_append_pcm) and convert_stream.hip
// (mi_streams_convert_append_pcm), so every route reads a PCM block as the same values.
//   i16: float(v) * 2^-15        exact: |v| <= 2^15 fits a float32 mantissa and the factor is a power of two
//   i24: float(v) * 2^-23        exact: |v| <= 2^23, v sign-extended from bit 23 of the three packed bytes
//   f32: the bits as they are    NaN payloads, infinities, -0 and subnormals included
// So `int16 / 32768` on the host and the device conversion agree bit for bit, and PCM in gives what the float path gives.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/demucs_amd.h"

namespace mi {

__host__ __device__ inline int pcm_width(int64_t fmt) { return fmt == MI_PCM_I16 ? 2 : fmt == MI_PCM_I24 ? 3 : fmt == MI_PCM_F32 ? 4 : 0; }

// A source the entries accept: a known wire format, at least one channel, the address aligned to the sample width (any byte
// address for i24)
__device__ __forceinline__ bool pcm_source_ok(int64_t fmt, int64_t src_ch, uintptr_t addr) {
    const int w = pcm_width(fmt);
    return w != 0 && src_ch >= 1 && (w == 3 || addr % (unsigned)w == 0);
}

__device__ __forceinline__ float pcm_from_i16(int v) { return __fmul_rn((float)v, 0x1p-15f); }
__device__ __forceinline__ float pcm_from_i24(unsigned u) { return __fmul_rn((float)((int)(u << 8) >> 8), 0x1p-23f); }

// Sample (frame j, source channel r) of the block of `src_ch`-channel frames at byte address `src` (aligned to the sample width).
// Reads the sample's own bytes and nothing else: an i24 sample is three byte loads, never a 4-byte load past the block's end.
__device__ __forceinline__ float pcm_sample(const unsigned char *__restrict__ src, int fmt, int64_t src_ch, int64_t j, int64_t r) {
    const int64_t q = j * src_ch + r;
    if (fmt == MI_PCM_I16) return pcm_from_i16(*reinterpret_cast<const short *>(src + 2 * q));
    if (fmt == MI_PCM_F32) return *reinterpret_cast<const float *>(src + 4 * q);
    const unsigned char *p = src + 3 * q;
    return pcm_from_i24((unsigned)p[0] | (unsigned)p[1] << 8 | (unsigned)p[2] << 16);
}

// The aligned middle of a block: a unit is the fewest 16-byte loads that hold a whole number of samples.
template <int FMT> struct pcm_unit;
template <> struct pcm_unit<MI_PCM_I16> { static constexpr int SAMPLES = 8, LOADS = 1, WIDTH = 2; };
template <> struct pcm_unit<MI_PCM_I24> { static constexpr int SAMPLES = 16, LOADS = 3, WIDTH = 3; };
template <> struct pcm_unit<MI_PCM_F32> { static constexpr int SAMPLES = 4, LOADS = 1, WIDTH = 4; };

// SAMPLES consecutive samples whose first byte is `d` bytes (0 <= d < WIDTH; 0 unless i24) after the 16-byte aligned address p:
// LOADS 16-byte loads, and for d > 0 the d bytes after them one by one (they belong to the unit's last sample).
template <int FMT>
__device__ __forceinline__ void pcm_unit_load(const unsigned char *__restrict__ p, int d, float (&v)[pcm_unit<FMT>::SAMPLES]) {
    using U = pcm_unit<FMT>;
    unsigned w[4 * U::LOADS + 1];
#pragma unroll
    for (int l = 0; l < U::LOADS; ++l) {
        const uint4 x = reinterpret_cast<const uint4 *>(p)[l];
        w[4 * l] = x.x, w[4 * l + 1] = x.y, w[4 * l + 2] = x.z, w[4 * l + 3] = x.w;
    }
    w[4 * U::LOADS] = 0;
    if (FMT == MI_PCM_I16) {
#pragma unroll
        for (int k = 0; k < U::SAMPLES; ++k) v[k] = pcm_from_i16((short)(w[k >> 1] >> (16 * (k & 1))));
    } else if (FMT == MI_PCM_F32) {
#pragma unroll
        for (int k = 0; k < U::SAMPLES; ++k) v[k] = __uint_as_float(w[k]);
    } else {
        if (d > 0) {
            unsigned tail = p[16 * U::LOADS];
            if (d > 1) tail |= (unsigned)p[16 * U::LOADS + 1] << 8;
            w[4 * U::LOADS] = tail;
            // drop the d bytes in front, so that sample k starts at byte 3 k whatever d is (no register is indexed by d)
#pragma unroll
            for (int i = 0; i < 4 * U::LOADS; ++i) w[i] = (unsigned)((((uint64_t)w[i + 1] << 32) | w[i]) >> (8 * d));
        }
#pragma unroll
        for (int k = 0; k < U::SAMPLES; ++k) {
            const int o = 3 * k, i = o >> 2, s = 8 * (o & 3);
            const unsigned lo = w[i] >> s;
            const unsigned u = s > 8 ? lo | w[i + 1] << (32 - s) : lo;        // i + 1 <= 4 * LOADS - 1 here: 3 * 15 + 2 = 47
            v[k] = pcm_from_i24(u & 0xffffffu);
        }
    }
}

// One block as work items: item t of `pcm_items(...)` decodes either a unit of the aligned middle or one sample of the
// unaligned head or tail, and hands every sample it decoded to put(j, r, value) (frame, source channel).  Every sample of the
// block is handed over exactly once over t = 0 .. pcm_items - 1; no byte outside [src, src + n * src_ch * width) is read.
struct pcm_split {
    int64_t head;      // samples before the first unit
    int64_t units;     // units of the aligned middle
    int64_t rest;      // samples after the last unit
    int d;             // bytes between the 16-byte boundary and the first unit's first sample (i24 only)
    const unsigned char *mid;   // 16-byte aligned address of the first unit
};

template <int FMT>
__device__ __forceinline__ pcm_split pcm_split_block(const unsigned char *src, int64_t src_ch, int64_t n) {
    using U = pcm_unit<FMT>;
    const int64_t Q = n * src_ch, T = Q * U::WIDTH;
    int64_t hb = (int64_t)((16 - ((uintptr_t)src & 15)) & 15);
    hb = hb < T ? hb : T;
    pcm_split s;
    s.head = (hb + U::WIDTH - 1) / U::WIDTH;
    s.head = s.head < Q ? s.head : Q;
    s.d = (int)(s.head * U::WIDTH - hb);
    s.units = (Q - s.head) / U::SAMPLES;
    s.rest = Q - s.head - s.units * U::SAMPLES;
    s.mid = src + hb;
    return s;
}

// items of a block of `bytes` bytes at most: every unit is at least 16 bytes, the head is under 16 bytes and the rest under a unit
__host__ __device__ inline int64_t pcm_max_items(int64_t bytes) { return bytes / 16 + 8 + 16; }

template <int FMT, class Put>
__device__ __forceinline__ void pcm_item(const unsigned char *__restrict__ src, int64_t src_ch, int64_t n, int64_t t, Put put) {
    using U = pcm_unit<FMT>;
    const pcm_split s = pcm_split_block<FMT>(src, src_ch, n);
    if (t < s.units) {
        float v[U::SAMPLES];
        pcm_unit_load<FMT>(s.mid + t * (16 * U::LOADS), s.d, v);
        const int64_t q = s.head + t * U::SAMPLES;
        int64_t j = q / src_ch, r = q - j * src_ch;
#pragma unroll
        for (int k = 0; k < U::SAMPLES; ++k) {
            put(j, r, v[k]);
            if (++r == src_ch) r = 0, ++j;
        }
        return;
    }
    int64_t q = t - s.units;                               // the head's samples, then the rest's
    if (q >= s.head + s.rest) return;
    if (q >= s.head) q += s.units * U::SAMPLES;
    const int64_t j = q / src_ch, r = q - j * src_ch;
    put(j, r, pcm_sample(src, FMT, src_ch, j, r));
}

// pcm_item for a format known at run time (wave-uniform: one block is one format)
template <class Put>
__device__ __forceinline__ void pcm_item_any(const unsigned char *__restrict__ src, int fmt, int64_t src_ch, int64_t n, int64_t t,
                                             Put put) {
    if (fmt == MI_PCM_I16) pcm_item<MI_PCM_I16>(src, src_ch, n, t, put);
    else if (fmt == MI_PCM_I24) pcm_item<MI_PCM_I24>(src, src_ch, n, t, put);
    else if (fmt == MI_PCM_F32) pcm_item<MI_PCM_F32>(src, src_ch, n, t, put);
}

}  // namespace mi
