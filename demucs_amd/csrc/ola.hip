// Device side of the segment scheduler (reference: demucs/apply.py:108-124,257-301).
//
// The whole track stays resident in HBM: segments are cut out of it with TensorChunk.padded
// semantics, and the weighted overlap-add runs on the device in the reference's summation
// order (ascending segment offset, float32, product and sum rounded separately), so the stitched
// result is bit-identical to `out[..., off:off+SL] += weight[:n] * chunk_out; out /= sum_weight`
// applied to the same per-segment outputs.
#include "common.h"
#include "kernels.h"

namespace mi {

// Every kernel below serves two callers with ONE body: the one-track entries (mi_segments_gather / mi_ola_accumulate /
// mi_ola_finish: one track, one accumulator, flat index arrays) and the packed entries (*_packed: many tracks in one buffer,
// many accumulators in another, one per-batch item table and a host-built tile list).  The one-track case maps onto the
// packed fields uniformly per launch, so both run the same loads, the same compaction and the same float32 sequence.

// seg[b][c][i] = track_b[c][start_b + i] or 0 outside [0, len_b) -- and 0 wherever the read would leave [0, track_cap).
// One-track: track_b = track (len track_len, cap channels * track_len), start_b = starts[b].  Packed: item b of `items`
// (MI_PACK_* columns) names its track by float offset and length inside the packed buffer.  grid (ceil(valid/256), channels, B)
__global__ __launch_bounds__(256) void segments_gather_kernel(const float *__restrict__ track, int64_t track_cap, int channels,
                                                              const int64_t *__restrict__ starts, int64_t track_len,
                                                              const int64_t *__restrict__ items, int valid,
                                                              float *__restrict__ seg) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= valid) return;
    const int c = blockIdx.y, b = blockIdx.z;
    int64_t src_off = 0, src_len = track_len, start;
    if (items) {
        const int64_t *it = items + (size_t)b * MI_PACK_ITEM_COLS;
        src_off = it[MI_PACK_SRC_OFF];
        src_len = it[MI_PACK_SRC_LEN];
        start = it[MI_PACK_START];
    } else {
        start = starts[b];
    }
    const int64_t p = start + i;
    // the whole (channels, src_len) track must lie inside [0, track_cap): src_len <= track_cap and channels <= 65535 keep
    // channels * src_len far from overflow, and src_off is compared against what is left, never added first
    const bool ok = src_len >= 0 && src_len <= track_cap && src_off >= 0 && src_off <= track_cap - (int64_t)channels * src_len &&
                    p >= 0 && p < src_len;
    seg[((size_t)b * channels + c) * valid + i] = ok ? track[src_off + (int64_t)c * src_len + p] : 0.f;
}

// A workgroup of the two overlap-add kernels owns kOlaSpan consecutive positions, thread i the positions i + 256 e: every access
// stays a fully coalesced 4-byte one (segment offsets are odd sample counts: no wider alignment exists on the model-output side),
// the loads of a thread's kOlaE positions are in flight together and the per-workgroup search for the overlapping segments is
// paid once per 1 024 positions (one position per thread, round 1-3: 2.0-2.3 TB/s on plain streaming traffic).
constexpr int kOlaE = 4, kOlaSpan = 256 * kOlaE;
static_assert(kOlaSpan == MI_PACK_TILE_SPAN, "the packed tile span is part of the C ABI");

// One tile: an accumulator (rows, acc_len) at float offset acc_base of `acc`, its positions [pos, pos + kOlaSpan), the item (or
// segment) range [lo, hi) that may touch them, and the weight ramp w_len floats long at float offset w_off of `weight`.  Tiles
// whose fields leave the declared capacities are clamped or dropped on the device, where the host cannot look.
struct OlaTile {
    int64_t acc_base, acc_len, pos, w_off;
    int lo, hi, w_len;
    bool ok;
};

__device__ inline OlaTile load_tile(const int64_t *__restrict__ tiles, int64_t acc_cap, int rows, int n_cap, int64_t weight_cap) {
    const int64_t *t = tiles + (size_t)blockIdx.x * MI_PACK_TILE_COLS;
    OlaTile o;
    o.acc_base = t[MI_PACK_T_ACC_BASE];
    o.acc_len = t[MI_PACK_T_ACC_LEN];
    o.pos = t[MI_PACK_T_POS];
    o.w_off = t[MI_PACK_T_W_OFF];
    const int64_t lo = t[MI_PACK_T_LO], hi = t[MI_PACK_T_HI], wl = t[MI_PACK_T_W_LEN];
    o.ok = o.acc_base >= 0 && o.acc_len >= 0 && o.acc_len <= acc_cap && o.acc_base <= acc_cap - (int64_t)rows * o.acc_len &&
           o.w_off >= 0 && o.w_off <= weight_cap && lo >= 0 && lo <= hi;
    o.lo = (int)(lo < n_cap ? lo : n_cap);
    o.hi = (int)(hi < n_cap ? hi : n_cap);
    const int64_t w_room = weight_cap - o.w_off;
    o.w_len = (int)(wl < 0 ? 0 : wl < w_room ? wl : w_room < INT32_MAX ? w_room : INT32_MAX);
    return o;
}

// acc[row][p] += sum over items (ascending) of weight[p - off] * out[item][row][trim + p - off]
// One-track: grid (ceil(span/kOlaSpan), rows), tile x = positions span_lo + x kOlaSpan of the one accumulator, items [0, B).
// Packed: grid (n_tiles, rows), tile x from `tiles`, items from `items` (at most 256 per tile, and only those whose
// accumulator base is the tile's).
__global__ __launch_bounds__(256) void ola_accumulate_kernel(float *__restrict__ acc, int64_t acc_cap, const float *__restrict__ mo,
                                                             int rows, int valid, int B,
                                                             const int64_t *__restrict__ offs, const int32_t *__restrict__ lens,
                                                             const int32_t *__restrict__ trim, int64_t acc_len1, int64_t span_lo,
                                                             int64_t span_hi, const int64_t *__restrict__ items,
                                                             const int64_t *__restrict__ tiles, const float *__restrict__ weight,
                                                             int64_t weight_cap) {
    OlaTile tl;
    int64_t lim;
    if (tiles) {
        tl = load_tile(tiles, acc_cap, rows, B, weight_cap);
        if (!tl.ok) return;
        if (tl.hi - tl.lo > 256) tl.hi = tl.lo + 256;
        lim = tl.acc_len;
    } else {
        tl.acc_base = 0; tl.acc_len = acc_len1; tl.pos = span_lo + (int64_t)blockIdx.x * kOlaSpan; tl.w_off = 0;
        tl.lo = 0; tl.hi = B; tl.w_len = (int)weight_cap; tl.ok = true;
        lim = span_hi < acc_len1 ? span_hi : acc_len1;
    }
    auto item = [&](int i, int64_t &off, int64_t &len, int64_t &tr) -> bool {
        if (items) {
            const int64_t *it = items + (size_t)i * MI_PACK_ITEM_COLS;
            off = it[MI_PACK_OFF]; len = it[MI_PACK_LEN]; tr = it[MI_PACK_TRIM];
            return it[MI_PACK_ACC_BASE] == tl.acc_base && it[MI_PACK_ACC_LEN] == tl.acc_len;
        }
        off = offs[i]; len = lens[i]; tr = trim[i];
        return true;
    };
    // the items that overlap this workgroup's positions, in ascending item order (= the reference's summation
    // order), found once per workgroup instead of B range checks per sample
    __shared__ int n_hit;
    __shared__ int hit[256];
    const int64_t p0 = tl.pos;
    if (threadIdx.x == 0) n_hit = 0;
    __syncthreads();
    for (int base = tl.lo; base < tl.hi; base += 256) {     // at most 256 items per tile: one round
        const int i = base + threadIdx.x;
        int64_t off_i = 0, len_i = 0, tr_i = 0;
        const bool over = i < tl.hi && item(i, off_i, len_i, tr_i) && off_i < p0 + kOlaSpan && off_i + len_i > p0;
        const unsigned long long m = __ballot(over);
        // wave-ordered compaction keeps ascending item order: waves append in order through the barrier sequence below
        for (int w = 0; w < 4; ++w) {
            if ((threadIdx.x >> 6) == w && over) hit[n_hit + __popcll(m & ((1ull << (threadIdx.x & 63)) - 1))] = i;
            __syncthreads();
            if (threadIdx.x == w * 64) n_hit += __popcll(m);
            __syncthreads();
        }
    }
    const int row = blockIdx.y;
    float *acc_row = acc + tl.acc_base + (size_t)row * tl.acc_len;
    const float *w = weight + tl.w_off;
    float a[kOlaE];
    bool touched[kOlaE];
#pragma unroll
    for (int e = 0; e < kOlaE; ++e) {
        const int64_t p = p0 + e * 256 + threadIdx.x;
        a[e] = (p >= 0 && p < lim) ? acc_row[p] : 0.f;
        touched[e] = false;
    }
    const int nh = n_hit;
    for (int h = 0; h < nh; ++h) {
        const int i = hit[h];
        int64_t off_i, len_i, trim_i;
        item(i, off_i, len_i, trim_i);
        const float *src_row = mo + ((size_t)i * rows + row) * valid;
#pragma unroll
        for (int e = 0; e < kOlaE; ++e) {
            const int64_t p = p0 + e * 256 + threadIdx.x;
            const int64_t j = p - off_i;
            // lens / trim live on the device, where the host cannot validate them without a sync: clamp to the buffers' extents
            const int64_t src = trim_i + j;
            if (p >= 0 && p < lim && j >= 0 && j < len_i && j < tl.w_len && src >= 0 && src < valid) {
                const float v = src_row[src];
                a[e] = __fadd_rn(a[e], __fmul_rn(w[j], v));
                touched[e] = true;
            }
        }
    }
#pragma unroll
    for (int e = 0; e < kOlaE; ++e)
        if (touched[e]) acc_row[p0 + e * 256 + threadIdx.x] = a[e];
}

// acc[row][q] /= sum_weight[acc_off0 + q], sum_weight rebuilt in ascending-offset float32 order from the segment list.
// Segment offsets must be sorted ascending.  One-track: grid (ceil(acc_len/kOlaSpan), rows), segments (offs, lens)[0, n),
// max_len = ramp length.  Packed: grid (n_tiles, rows), tile x from `tiles`, segments [lo, hi) of `segs` ((offset, length)
// int64 pairs in accumulator positions, acc_off0 = 0), ramp of the tile.
__global__ __launch_bounds__(256) void ola_finish_kernel(float *__restrict__ acc, int64_t acc_cap, int rows, int64_t acc_len1,
                                                         int64_t acc_off0, const int64_t *__restrict__ offs,
                                                         const int32_t *__restrict__ lens, int n, const int64_t *__restrict__ segs,
                                                         const int64_t *__restrict__ tiles, const float *__restrict__ weight,
                                                         int64_t weight_cap) {
    OlaTile tl;
    if (tiles) {
        tl = load_tile(tiles, acc_cap, rows, n, weight_cap);
        if (!tl.ok) return;
        acc_off0 = 0;
    } else {
        tl.acc_base = 0; tl.acc_len = acc_len1; tl.pos = (int64_t)blockIdx.x * kOlaSpan; tl.w_off = 0;
        tl.lo = 0; tl.hi = n; tl.w_len = (int)weight_cap; tl.ok = true;
    }
    auto seg_off = [&](int i) -> int64_t { return segs ? segs[2 * (size_t)i] : offs[i]; };
    auto seg_len = [&](int i) -> int64_t { return segs ? segs[2 * (size_t)i + 1] : lens[i]; };
    const int max_len = tl.w_len;
    // one binary search per workgroup (first segment that can still cover the workgroup's first position)
    __shared__ int lo_s;
    if (threadIdx.x == 0) {
        const int64_t pb = acc_off0 + tl.pos;
        int lo = tl.lo, hi = tl.hi;
        while (lo < hi) { const int mid = (lo + hi) >> 1; if (seg_off(mid) > pb - max_len) hi = mid; else lo = mid + 1; }
        lo_s = lo;
    }
    __syncthreads();
    const int lo = lo_s;                                  // segments before lo end at or before pb <= p: they add nothing
    const int64_t q0 = tl.pos + threadIdx.x;
    float *acc_row = acc + tl.acc_base + (size_t)blockIdx.y * tl.acc_len;
    const float *w = weight + tl.w_off;
    float v[kOlaE], sw[kOlaE];
#pragma unroll
    for (int e = 0; e < kOlaE; ++e) {
        const int64_t q = q0 + e * 256;
        v[e] = (q >= 0 && q < tl.acc_len) ? acc_row[q] : 0.f;
        sw[e] = 0.f;
    }
    const int64_t p_last = acc_off0 + tl.pos + kOlaSpan - 1;
    for (int i = lo; i < tl.hi && seg_off(i) <= p_last; ++i) {
        const int64_t off_i = seg_off(i);
        const int64_t len_i = seg_len(i);
#pragma unroll
        for (int e = 0; e < kOlaE; ++e) {
            const int64_t j = acc_off0 + q0 + e * 256 - off_i;
            if (j >= 0 && j < len_i && j < max_len) sw[e] = __fadd_rn(sw[e], w[j]);
        }
    }
#pragma unroll
    for (int e = 0; e < kOlaE; ++e) {
        const int64_t q = q0 + e * 256;
        if (q >= 0 && q < tl.acc_len) acc_row[q] = __fdiv_rn(v[e], sw[e]);
    }
}

int launch_segments_gather(const float *track, int64_t track_len, int channels, const int64_t *starts_dev, int B, int valid,
                           float *seg, hipStream_t st) {
    hipLaunchKernelGGL(segments_gather_kernel, dim3(ceil_div(valid, 256), channels, B), dim3(256), 0, st, track,
                       (int64_t)channels * track_len, channels, starts_dev, track_len, (const int64_t *)nullptr, valid, seg);
    MI_CHECK_LAUNCH();
    return MI_OK;
}

int launch_segments_gather_packed(const float *tracks, int64_t tracks_cap, int channels, const int64_t *items_dev, int B, int valid,
                                  float *seg, hipStream_t st) {
    hipLaunchKernelGGL(segments_gather_kernel, dim3(ceil_div(valid, 256), channels, B), dim3(256), 0, st, tracks, tracks_cap, channels,
                       (const int64_t *)nullptr, (int64_t)0, items_dev, valid, seg);
    MI_CHECK_LAUNCH();
    return MI_OK;
}

int launch_ola_accumulate(float *acc, int64_t acc_len, int rows, const float *model_out, int valid, const int64_t *offs_dev,
                          const int32_t *lens_dev, const int32_t *trim_dev, int B, int64_t span_lo, int64_t span_hi,
                          const float *weight, int weight_len, hipStream_t st) {
    MI_REQUIRE(span_hi > span_lo && span_lo >= 0, "ola: empty span");
    MI_REQUIRE(B >= 1 && B <= 256, "ola: %d segments per call (at most 256)", B);
    hipLaunchKernelGGL(ola_accumulate_kernel, dim3(ceil_div(span_hi - span_lo, kOlaSpan), rows), dim3(256), 0, st, acc,
                       (int64_t)rows * acc_len, model_out, rows, valid, B, offs_dev, lens_dev, trim_dev, acc_len, span_lo, span_hi,
                       (const int64_t *)nullptr, (const int64_t *)nullptr, weight, (int64_t)weight_len);
    MI_CHECK_LAUNCH();
    return MI_OK;
}

int launch_ola_accumulate_packed(float *acc, int64_t acc_cap, int rows, const float *model_out, int valid, const int64_t *items_dev,
                                 int B, const int64_t *tiles_dev, int n_tiles, const float *weights, int64_t weights_cap,
                                 hipStream_t st) {
    hipLaunchKernelGGL(ola_accumulate_kernel, dim3(n_tiles, rows), dim3(256), 0, st, acc, acc_cap, model_out, rows, valid, B,
                       (const int64_t *)nullptr, (const int32_t *)nullptr, (const int32_t *)nullptr, (int64_t)0, (int64_t)0,
                       (int64_t)0, items_dev, tiles_dev, weights, weights_cap);
    MI_CHECK_LAUNCH();
    return MI_OK;
}

int launch_ola_finish(float *acc, int64_t acc_len, int rows, int64_t acc_off0, const int64_t *offs_dev, const int32_t *lens_dev,
                      int n_segments, int max_len, const float *weight, hipStream_t st) {
    hipLaunchKernelGGL(ola_finish_kernel, dim3(ceil_div(acc_len, kOlaSpan), rows), dim3(256), 0, st, acc, (int64_t)rows * acc_len,
                       rows, acc_len, acc_off0, offs_dev, lens_dev, n_segments, (const int64_t *)nullptr, (const int64_t *)nullptr,
                       weight, (int64_t)max_len);
    MI_CHECK_LAUNCH();
    return MI_OK;
}

int launch_ola_finish_packed(float *acc, int64_t acc_cap, int rows, const int64_t *tiles_dev, int n_tiles, const int64_t *segs_dev,
                             int n_segs, const float *weights, int64_t weights_cap, hipStream_t st) {
    hipLaunchKernelGGL(ola_finish_kernel, dim3(n_tiles, rows), dim3(256), 0, st, acc, acc_cap, rows, (int64_t)0, (int64_t)0,
                       (const int64_t *)nullptr, (const int32_t *)nullptr, n_segs, segs_dev, tiles_dev, weights, weights_cap);
    MI_CHECK_LAUNCH();
    return MI_OK;
}

}  // namespace mi
