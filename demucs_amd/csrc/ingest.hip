// Wire PCM into the streams (demucs_amd/stream.py, demucs_amd/audio.py): a live feed delivers little-endian interleaved int16,
// packed int24 or float32 frames, and these kernels de-interleave, convert and normalise them on the device, so the bytes cross
// PCIe as they came off the wire (4 B per stereo int16 frame against 8 B as planar float32) and no host pass touches a sample.
// The conversion is pcm_ingest.h's and exact, so a PCM block gives the bits the float path gives for `int16 / 32768`.
//
// Memory bound and small (a 1 s stereo block is 176 KB in, 353 KB out): one work item takes a unit of the 16-byte aligned middle of a
// block (one or three 16-byte loads, 4 to 16 samples) or one sample of its unaligned head or tail, and writes each sample to its
// destination row; consecutive lanes read consecutive units and write consecutive columns of every row.
#include "common.h"
#include "kernels.h"
#include "pcm_ingest.h"

namespace mi {

// `convert_audio_channels`' per-sample cases, seen from the source: a mono sample feeds every row; else source channel r is row r
// and the channels past the destination's are dropped.  store(c, j, v) writes row c.
template <class Store>
__device__ __forceinline__ void pcm_route(int64_t src_ch, int channels, int64_t j, int64_t r, float v, Store store) {
    if (src_ch == 1) {
        for (int c = 0; c < channels; ++c) store(c, j, v);
    } else if (r < channels) {
        store((int)r, j, v);
    }
}

// mi_pcm_planar: grid (ceil(pcm_max_items(bytes) / 256)); dst (channels, n)
__global__ __launch_bounds__(256) void pcm_planar_kernel(const unsigned char *__restrict__ src, int fmt, int src_ch, int64_t n, int channels,
                                                         const float *__restrict__ stats, float *__restrict__ dst) {
    const bool aff = stats != nullptr;
    const float mean = aff ? stats[0] : 0.f, sd = aff ? stats[1] : 1.f;
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    pcm_item_any(src, fmt, src_ch, n, t, [&](int64_t j, int64_t r, float v) {
        const float y = aff ? __fdiv_rn(__fsub_rn(v, mean), sd) : v;
        pcm_route(src_ch, channels, j, r, y, [&](int c, int64_t jj, float yy) { dst[(int64_t)c * n + jj] = yy; });
    });
}

// mi_streams_append_pcm: streams_append_kernel (stream.hip) with a source format per row.  grid (ceil(max_items / 256), n_streams);
// a planar float32 row copies four consecutive floats of its (channels, n) block per item, as streams_append_kernel does per thread
__global__ __launch_bounds__(256) void streams_append_pcm_kernel(float *__restrict__ win, int64_t win_cap, int channels,
                                                                 const int64_t *__restrict__ table, const float *__restrict__ stats,
                                                                 int n_stats) {
    const int64_t *t = table + (size_t)blockIdx.y * MI_APPEND_PCM_COLS;
    const int64_t n = t[MI_APPEND_PCM_N], dst_off = t[MI_APPEND_PCM_DST_OFF], dst_len = t[MI_APPEND_PCM_DST_LEN];
    const int64_t col = t[MI_APPEND_PCM_COL], fmt = t[MI_APPEND_PCM_FMT], src_ch = t[MI_APPEND_PCM_SRC_CH];
    if (n <= 0 || dst_len < 0 || dst_len > win_cap || dst_off < 0 || dst_off > win_cap - (int64_t)channels * dst_len || col < 0 ||
        col > dst_len)
        return;
    const uintptr_t addr = static_cast<uintptr_t>(t[MI_APPEND_PCM_SRC]);
    const int64_t si = t[MI_APPEND_PCM_STATS];
    const bool aff = stats && si >= 0 && si < n_stats;
    const float mean = aff ? stats[2 * si] : 0.f, sd = aff ? stats[2 * si + 1] : 1.f;
    float *dst = win + dst_off + col;
    const int64_t room = dst_len - col;
    auto store = [&](int c, int64_t j, float v) {
        if (j < room) dst[(int64_t)c * dst_len + j] = aff ? __fdiv_rn(__fsub_rn(v, mean), sd) : v;
    };
    const int64_t item = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (fmt == MI_PCM_PLANAR) {
        const float *src = reinterpret_cast<const float *>(addr);
        const int64_t total = (int64_t)channels * n;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int64_t i = item * 4 + e;
            if (i < total) store((int)(i / n), i % n, src[i]);
        }
        return;
    }
    if (!pcm_source_ok(fmt, src_ch, addr) || (src_ch != 1 && src_ch < channels)) return;
    pcm_item_any(reinterpret_cast<const unsigned char *>(addr), (int)fmt, src_ch, n, item,
                 [&](int64_t j, int64_t r, float v) { pcm_route(src_ch, channels, j, r, v, store); });
}

int launch_pcm_planar(const unsigned char *src, int fmt, int src_ch, int64_t n, int channels, const float *stats, float *dst,
                      hipStream_t st) {
    const int64_t items = pcm_max_items(n * src_ch * pcm_width(fmt));
    hipLaunchKernelGGL(pcm_planar_kernel, dim3(ceil_div(items, 256)), dim3(256), 0, st, src, fmt, src_ch, n, channels, stats, dst);
    MI_CHECK_LAUNCH();
    return MI_OK;
}

int launch_streams_append_pcm(float *win, int64_t win_cap, int channels, const int64_t *table, int n_streams, int64_t max_bytes,
                              const float *stats, int n_stats, hipStream_t st) {
    hipLaunchKernelGGL(streams_append_pcm_kernel, dim3(ceil_div(pcm_max_items(max_bytes), 256), n_streams), dim3(256), 0, st, win, win_cap,
                       channels, table, stats, n_stats);
    MI_CHECK_LAUNCH();
    return MI_OK;
}

}  // namespace mi
