/* demucs_amd.h — C ABI of the MI355X (gfx950) HTDemucs segment-inference engine.
 *
 * The upstream project (DrorT/demucs) is pure Python and has no FFI; its boundary for this
 * path is a Python call + a weight schema.  Each entry point below names the reference
 * interface it stands in for (paths relative to the reference checkout).  A maintainer binds
 * them with ctypes (demucs_amd/_lib.py is that binding).
 *
 * Conventions
 *   - every function returns 0 on success or a negative MI_E* code; nothing throws across the
 *     ABI; `mi_last_error()` returns a thread-local, NUL-terminated description of the last
 *     failure on the calling thread.
 *   - `*_dev` pointers are device (HBM) addresses owned by the caller (e.g. torch tensors'
 *     data_ptr()), contiguous float32 unless stated; `stream` is a hipStream_t (NULL = the
 *     default stream).  All work is enqueued asynchronously on `stream`; no call synchronises
 *     the device except mi_model_create / mi_model_destroy.
 *   - a handle is single-stream: do not use one handle from two streams/threads at once.
 *   - a handle knows its engine: an mi_model_* entry given an hdemucs handle, or an mi_hmodel_* entry given an htdemucs one,
 *     returns MI_EINVAL (the byte counts: 0) before it touches the handle's state or the GPU; mi_profile_begin / _end take both.
 *   - PROCESS-WIDE STATE (one process per GPU is the deployment).  Handles are independent EXCEPT for: (1) the activation
 *     workspace of the htdemucs engine, which every handle created on the same device with the same (n_sources,
 *     segment_length, max_batch, float32 / half) shares -- a bag of four fine-tuned models holds its ~0.57 GB per batched
 *     segment once: such handles must run one after the other on one stream (what apply_model's bag loop does), never
 *     concurrently; hdemucs handles own their workspace; (2) the schedule switches mi_set_two_streams / mi_set_istft_fused / mi_set_transpose_tiles
 *     and the MI_* environment variables (read once); (3) one small device block every launch may use: a 256-float sink for
 *     masked stores followed by 64 floats (256 bytes) that hold zero and stay zero, the source of out-of-frame LDS-DMA transfers
 *     (MI_SINK_FLOATS, MI_ZERO_PAGE_FLOATS in demucs_amd/csrc/gemm_conv.h; a caller-provided mi_conv_desc.sink has the same layout).  A forward also uses a side stream
 *     owned by its handle; it is joined on the caller's stream before the call returns.
 */
#ifndef DEMUCS_AMD_H
#define DEMUCS_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MI_OK 0
#define MI_EINVAL (-1)   /* bad argument / unsupported configuration            */
#define MI_EHIP (-2)     /* a HIP runtime call failed (see mi_last_error)        */
#define MI_ENOMEM (-3)   /* device or host allocation failed                     */
#define MI_EWEIGHT (-4)  /* missing / mis-shaped tensor in the weight table      */

/* One tensor of a reference `state_dict()` (demucs/states.py:83-107 yields these names;
 * schema in SURVEY.md App. B).  `data` is a HOST pointer to float32, row-major, `numel`
 * elements; the library copies what it needs before mi_model_create returns. */
typedef struct mi_tensor_desc {
    const char *name;
    const float *data;
    int64_t numel;
} mi_tensor_desc;

/* Architecture = the released htdemucs family (demucs/htdemucs.py:56-133 with
 * channels=48, depth=4, nfft=4096, dconv_mode=3, bottom_channels=512, t_layers=5, t_heads=8). */
typedef struct mi_config {
    int32_t n_sources;       /* len(model.sources): 4 (htdemucs, htdemucs_ft) or 6 (htdemucs_6s) */
    int32_t segment_length;  /* int(model.segment * model.samplerate) = 343980                   */
    int32_t max_batch;       /* segments per forward the workspace is sized for                  */
    int32_t dtype;           /* MI_DTYPE_*: operand type of the matrix-core GEMMs and attention  */
} mi_config;

/* Compute modes.  F32 is the parity mode (fp32 MFMA, exact fp32 arithmetic, <= 1e-4 of the CPU reference).
 * BF16 / F16 round the OPERANDS of every conv / linear GEMM and of the attention products to bf16 / fp16 and
 * feed them to v_mfma_f32_32x32x16_{bf16,f16}; accumulation, biases, GroupNorm / LayerNorm statistics, softmax,
 * GELU / GLU, the STFT / iSTFT and all activations in HBM stay float32 (BASELINE.json configs[2], configs[4]).
 * One rounding to nearest even moves a value x by at most half an ulp: relative to |x| that is 2^-8 (bf16) / 2^-11 (fp16)
 * at the bottom of x's binade and 2^-9 / 2^-12 at its top; bounds on the half modes (tests/test_gpu_attention.py,
 * tests/test_gpu_half_linear.py) use the half ulp itself or the bottom-of-binade figure, never the smaller one. */
#define MI_DTYPE_F32 0
#define MI_DTYPE_BF16 1
#define MI_DTYPE_F16 2

/* ---- model lifetime: replaces `states.load_model` + `model.to(device)`
 *      (demucs/states.py:50-80, demucs/apply.py:233) ------------------------------------- */
int mi_model_create(const mi_config *cfg, const mi_tensor_desc *weights, size_t n_weights, void **handle);
void mi_model_destroy(void *handle);

/* ---- `model(padded_mix)` under no_grad (demucs/apply.py:316-317 -> HTDemucs.forward,
 *      demucs/htdemucs.py:527-660).  mix_dev: (B, 2, segment_length); out_dev:
 *      (B, n_sources, 2, segment_length).  1 <= B <= max_batch.  Batch items are independent of each other and of
 *      earlier forwards on the handle, non-finite input included: a NaN / Inf in item k makes item k's output NaN and leaves
 *      every other item, and every later forward, bit for bit what it would have been (tests/test_gpu_isolation.py). ------ */
int mi_model_forward(void *handle, const float *mix_dev, float *out_dev, int32_t B, void *stream);

/* ---- `HTDemucs.forward_core(mag, mix)` (demucs/htdemucs.py:662-759; the fork's ONNX "core", docs/onnx.md):
 *      the network without the STFT in front, the iSTFT behind and the branch sum.  mag_dev (B, 4, 2048, T) is the
 *      caller's `_magnitude(_spec(mix))` (the fork's ONNX / web tools compute it with their own STFT) and is what
 *      the frequency branch consumes; NULL = derive it from mix_dev (B, 2, segment_length) with the engine's STFT.
 *      spec_out_dev: (B, S, 4, 2048, T); time_out_dev: (B, S, 2, segment_length). --------------------------- */
int mi_model_forward_core(void *handle, const float *mix_dev, const float *mag_dev, float *spec_out_dev,
                          float *time_out_dev, int32_t B, void *stream);

/* ---- Hybrid Demucs v3 (`hdemucs_mmi`: demucs/hdemucs.py:338-794 with the constructor's defaults; BASELINE.json configs[4]).
 *      mi_config.segment_length is the LONGEST input the handle's workspace is sized for (remote/hdemucs_mmi.yaml: 44 s);
 *      every forward names its own length (the reference's HDemucs has no valid_length: demucs/apply.py:309-310 hands it
 *      each chunk as it is): mix_dev (B, 2, length) -> out_dev (B, n_sources, 2, length), 64 <= length <= segment_length.
 *      Tap names: "enc0".."enc5", "tenc0".."tenc4", "dec0+skip".."dec4+skip", "dec5", "tdec0+skip".."tdec3+skip", "tdec4"
 *      (decoder outputs are stored with the next layer's skip already added); frequency-branch taps carry a frame pitch of
 *      max(32, ceil(T / 4) * 4) floats per row. ------------------------------------------- */
int mi_hmodel_create(const mi_config *cfg, const mi_tensor_desc *weights, size_t n_weights, void **handle);
void mi_hmodel_destroy(void *handle);
/* mi_hmodel_forward: the same independence as mi_model_forward -- between the B items of a call, and between successive calls of
 *   any B and length on one handle, non-finite input included. */
int mi_hmodel_forward(void *handle, const float *mix_dev, float *out_dev, int32_t B, int32_t length, void *stream);
int mi_hmodel_tap(void *handle, const char *name, float *dst_dev, int32_t B, int64_t *numel_per_item, void *stream);
int64_t mi_hmodel_device_bytes(void *handle);
/* mi_hmodel_status: waits for `stream` and reports whether any forward of this handle so far lost its BLSTM recurrence
 *   (demucs/demucs.py:20-67 runs as one persistent kernel per sequence; a hidden-state wait that exceeds 0.3 s -- only when other
 *   persistent kernels keep part of its grid from becoming resident, e.g. two processes on one GPU -- abandons the sequence and sets a
 *   sticky word).  mi_hmodel_forward checks that word when it STARTS, so a time-out in the LAST forward of a job would go unnoticed:
 *   callers that hand results on (demucs_amd.apply.apply_model does) ask here once the work is enqueued.  MI_OK, or MI_EINVAL with the
 *   message of mi_last_error. */
int mi_hmodel_status(void *handle, void *stream);

/* Debug / parity aid: copy an internal activation left behind by the last mi_model_forward
 * (first B items) into dst_dev (may be NULL to query *numel_per_item only).  Names: "x0" (normalised CaC spectrogram),
 * "xt0", "enc0".."enc3", "tenc0".."tenc3" (encoder outputs = skip tensors; time-branch rows are stored with a
 * pitch rounded up to 4 samples), "tr_f", "tr_t"
 * (transformer outputs, channel-first), "yspec", "ytime" (decoder outputs before iSTFT). */
int mi_model_tap(void *handle, const char *name, float *dst_dev, int32_t B, int64_t *numel_per_item, void *stream);

/* Per-kernel-class device timing for the roofline report: between begin and end every launch of
 * the conv-GEMM and attention kernels made by mi_model_forward is bracketed by a HIP event pair
 * on the launch stream; end synchronises the stream and returns one row per kernel class with
 * the summed duration and the ALGORITHMIC flops / bytes of those launches. */
typedef struct mi_profile_row {
    char name[48];
    int64_t launches;
    double ms, flops, bytes;
} mi_profile_row;
/* mi_set_two_streams: the htdemucs engine runs the waveform branch of a forward on a side stream beside the spectral branch
 *   (enabled = 1, the default: results are bit-identical either way); 0 keeps every launch on the caller's stream, one kernel on
 *   the GPU at a time -- what a per-kernel timing wants.  Returns the previous setting.  Process-wide. */
int mi_set_two_streams(int32_t enabled);
/* mi_set_istft_fused: the inverse STFT (demucs/spec.py:30-47) runs its per-frame inverse transforms and the overlap-add in ONE
 *   kernel (hop blocks accumulated in registers; the windowed frames never go to memory).  0 selects the two separate kernels
 *   (frames to memory, then a gather): same summation order, bit-identical output -- kept for A/B runs and as the check of the
 *   fused kernel.  Process-wide; returns the previous setting.  Initial value: 1 unless MI_ISTFT_SPLIT is set. */
int mi_set_istft_fused(int32_t enabled);
/* mi_set_split_bf16: the float32 engine runs its transformer linears, its decoders' 3 x 3 / k = 3 rewrite convs and its frequency
 *   branch's encoder convs (levels 1-3) and transposed convs (decoders 0-2) (and, with
 *   MI_X6=1, every layer with a split image) on the split-bf16 main loop (gemm_x6.hip: fp32 operands as three exact bf16 terms, six bf16 MFMA products, fp32 accumulate), and
 *   its attention core on the split-bf16 attention kernel (mi_attention_split).  0 selects the native fp32 MFMA kernels, the
 *   linears', the conv routes' and mi_attention's, for every later launch, e.g. in a process that shares its GPU with another rank
 *   (demucs_amd/distributed.py does this by itself).  Process-wide; returns the previous setting.  Initial value: 1. */
int mi_set_split_bf16(int32_t enabled);
/* mi_set_transpose_tiles: the kernels either side of the transforms (demucs/htdemucs.py:420-471, demucs/spec.py:11-47).  0, the
 *   default: the STFT walks a run of consecutive frames per workgroup (twiddles and window read once per run, the next frame's samples
 *   prefetched), and the layout changes between the frame-major scratch and the conv layout x[b][c][bin][frame] move 32 bins x all
 *   frames of a plane per workgroup (one contiguous run on the conv-layout side).  1 selects the kernels of rounds 1-3 for all three
 *   (one frame per workgroup, 32 x 32 tile transposes); as a bit mask 2 selects only the tile cac_transpose, 4 only the tile
 *   spec_transpose.  Same values, same arithmetic, bit-identical spectrograms and waveforms (the float64 normalisation sums are
 *   accumulated in another order) -- kept for A/B runs and as the check of the default kernels.  Process-wide; returns the previous
 *   setting.  Initial value: 0 unless MI_TRANSPOSE_TILES is set. */
int mi_set_transpose_tiles(int32_t enabled);
int mi_profile_begin(void *handle);
int mi_profile_end(void *handle, mi_profile_row *rows, int32_t max_rows, int32_t *n_rows, void *stream);

/* Device bytes held by the handle (weights + workspace). */
int64_t mi_model_device_bytes(void *handle);

/* ---- segment scheduler pieces (demucs/apply.py:257-301,108-124) --------------------------
 * Index arrays (`*_idx_dev`) are DEVICE arrays (tiny; e.g. torch int tensors) so that every call
 * stays asynchronous on `stream`.
 *
 * mi_segments_gather: TensorChunk.padded for a batch of segments.  For item i the segment is
 *   the `valid`-long window starting at track sample starts[i] (may be negative / run past the
 *   end: zero filled) of track_dev (channels, track_len); seg_dev is (B, channels, valid) and holds seg_capacity
 *   floats (checked: the call fails instead of writing past the buffer).  1 <= channels, B <= 65535. */
int mi_segments_gather(const float *track_dev, int64_t track_len, int32_t channels, const int64_t *starts_idx_dev,
                       int32_t B, int32_t valid, float *seg_dev, int64_t seg_capacity, void *stream);

/* mi_ola_accumulate: `out[..., off:off+SL] += weight[:n] * chunk_out` for a batch
 *   (demucs/apply.py:295-296) with chunk_out = center_trim(model_out, n) (utils.py:38-54).
 *   model_out_dev: (B, rows, valid), rows = n_sources*channels; item i contributes samples
 *   [trim[i], trim[i]+lens[i]) of its rows, weighted by weight_dev[0:lens[i]], to
 *   acc_dev (rows, acc_len) at acc position offs[i].  [span_lo, span_hi) is the union of the
 *   items' acc ranges.  Items are applied in index order with separately rounded float32
 *   product and sum, i.e. exactly the reference's sequential loop.  model_out_dev holds out_capacity floats and
 *   weight_dev weight_len floats: the host-visible extents are checked, and because lens / trim live on the device
 *   the kernel itself never reads model_out_dev beyond `valid` per row nor weight_dev beyond weight_len.
 *   1 <= rows <= 65535, 1 <= B <= 256. */
int mi_ola_accumulate(float *acc_dev, int64_t acc_len, int32_t rows, const float *model_out_dev, int32_t valid,
                      int64_t out_capacity, const int64_t *offs_idx_dev, const int32_t *lens_idx_dev,
                      const int32_t *trim_idx_dev, int32_t B, int64_t span_lo, int64_t span_hi, const float *weight_dev,
                      int32_t weight_len, void *stream);

/* mi_ola_finish: `out /= sum_weight` (demucs/apply.py:297-299); sum_weight is rebuilt from the
 *   (offs, lens) list of ALL segments of the track (sorted by offset, track coordinates) in the
 *   reference's float32 summation order.  In place on acc_dev (rows, acc_len); acc_off0 is the
 *   track position of acc sample 0; max_len = the segment length.  1 <= rows <= 65535. */
int mi_ola_finish(float *acc_dev, int64_t acc_len, int32_t rows, int64_t acc_off0, const int64_t *offs_idx_dev,
                  const int32_t *lens_idx_dev, int32_t n_segments, int32_t max_len, const float *weight_dev, void *stream);

/* ---- packed scheduler pieces: many tracks / accumulators per launch (demucs_amd/packed.py) -------------------------------
 * The one-track entries above are the single-track case of the same kernels.  All tables are int64 DEVICE arrays.
 *
 * Item table (B rows of MI_PACK_ITEM_COLS): item b is a segment of the track stored (channels, src_len) at float offset src_off
 *   of the packed track buffer; its window starts at track sample `start` (zero fill outside [0, src_len)); its output is
 *   overlap-added into the accumulator (rows, acc_len) at float offset acc_base of the accumulator buffer, at position `off`,
 *   `len` samples from output sample `trim` on (mi_ola_accumulate's offs / lens / trim).
 * Tile table (MI_PACK_TILE_COLS per tile): the accumulator (acc_base, acc_len), its positions [pos, pos + MI_PACK_TILE_SPAN),
 *   the item range [lo, hi) -- or, for the finish, the segment range of `segs` -- that may touch them (at most 256 items per
 *   accumulate tile), and the weight ramp of w_len floats at float offset w_off of the weight buffer.  Within a tile items are
 *   summed in ascending index order; only items whose (acc_base, acc_len) equal the tile's count.
 * Every device-side read or write is clamped to the declared capacities (floats) of the track buffer, the model output, the
 *   accumulator buffer and the weight buffer: a wrong table changes results, never memory outside them. */
#define MI_PACK_SRC_OFF 0
#define MI_PACK_SRC_LEN 1
#define MI_PACK_START 2
#define MI_PACK_ACC_BASE 3
#define MI_PACK_ACC_LEN 4
#define MI_PACK_OFF 5
#define MI_PACK_LEN 6
#define MI_PACK_TRIM 7
#define MI_PACK_ITEM_COLS 8
#define MI_PACK_T_ACC_BASE 0
#define MI_PACK_T_ACC_LEN 1
#define MI_PACK_T_POS 2
#define MI_PACK_T_LO 3
#define MI_PACK_T_HI 4
#define MI_PACK_T_W_OFF 5
#define MI_PACK_T_W_LEN 6
#define MI_PACK_TILE_COLS 7
#define MI_PACK_TILE_SPAN 1024

/* mi_segments_gather_packed: seg_dev (B, channels, valid) from the item table's (src_off, src_len, start) columns. */
int mi_segments_gather_packed(const float *tracks_dev, int64_t tracks_capacity, int32_t channels, const int64_t *items_dev,
                              int32_t B, int32_t valid, float *seg_dev, int64_t seg_capacity, void *stream);

/* mi_ola_accumulate_packed: mi_ola_accumulate for the B items of model_out_dev (B, rows, valid), over n_tiles tiles. */
int mi_ola_accumulate_packed(float *acc_dev, int64_t acc_capacity, int32_t rows, const float *model_out_dev, int32_t valid,
                             int64_t out_capacity, const int64_t *items_dev, int32_t B, const int64_t *tiles_dev, int32_t n_tiles,
                             const float *weights_dev, int64_t weights_capacity, void *stream);

/* mi_ola_finish_packed: mi_ola_finish for every accumulator of a run in one launch.  segs_dev holds n_segs (offset, length)
 *   pairs in accumulator positions, each accumulator's run sorted by offset; a tile's [lo, hi) is its accumulator's run. */
int mi_ola_finish_packed(float *acc_dev, int64_t acc_capacity, int32_t rows, const int64_t *tiles_dev, int32_t n_tiles,
                         const int64_t *segs_dev, int32_t n_segs, const float *weights_dev, int64_t weights_capacity, void *stream);

/* mi_stream_emit: the final stems of the track span [t0, t0 + n) of a stream (demucs_amd/stream.py) from every (member, pass)
 *   accumulator, in ONE launch, as these reference lines compute them on the device path, each step a separately rounded float32
 *   operation in this order:
 *     1. `out /= sum_weight` (demucs/apply.py:297-299), sum_weight rebuilt from the pass's segment list as mi_ola_finish does;
 *     2. the shift average `out = piece.clone(); out.add_(piece) ...; out /= shifts` (apply.py:237-256), when shifts > 0;
 *     3. the bag average `out[:, k] *= w[m][k]; estimates.add_(out) ...; estimates[:, k] /= totals[k]` (apply.py:201-229),
 *        when bag != 0;
 *     4. `x *= std; x += mean` (api.py:285-288, mi_track_affine inverse = 1), when stats_dev is not null.
 *   PyTorch's CUDA kernels apply a host scalar divisor s as a product with float32(1 / s), the reciprocal taken in double:
 *   scales_dev holds those float32 factors, per member [1 / shifts, w[m][0 .. S-1]] and then [1 / totals[k]] (n_members * (S + 1) + S floats).
 *   Pass table (n_passes rows of MI_EMIT_PASS_COLS int64): the accumulator (S * channels, acc_len) at float offset acc_base of
 *   acc_dev, the accumulator position q0 of sample t0, the pass's segments [seg_lo, seg_hi) of segs_dev ((offset, length)
 *   int64 pairs in accumulator positions, ascending), its ramp of w_len floats at float offset w_off of weights_dev, and its
 *   bag member.  Rows are grouped by member (ascending) and listed in pass order within a member.
 *   out_dev (S, channels, n).  Reads are clamped to acc_capacity / weights_capacity / n_segs / n_members: a wrong table
 *   changes results, never memory outside the buffers. */
#define MI_EMIT_ACC_BASE 0
#define MI_EMIT_ACC_LEN 1
#define MI_EMIT_Q0 2
#define MI_EMIT_SEG_LO 3
#define MI_EMIT_SEG_HI 4
#define MI_EMIT_W_OFF 5
#define MI_EMIT_W_LEN 6
#define MI_EMIT_MEMBER 7
#define MI_EMIT_PASS_COLS 8
int mi_stream_emit(const float *acc_dev, int64_t acc_capacity, int32_t n_sources, int32_t channels, const int64_t *passes_dev,
                   int32_t n_passes, const int64_t *segs_dev, int32_t n_segs, const float *weights_dev, int64_t weights_capacity,
                   const float *scales_dev, int32_t n_members, int32_t shifts, int32_t bag, const float *stats_dev, int64_t n,
                   float *out_dev, int64_t out_capacity, void *stream);

/* ---- stream groups: many streams as one unit of work per push (demucs_amd/stream.py, StreamGroup) ---------------------------
 * All tables are int64 DEVICE arrays; every read and write of a buffer is clamped to its declared capacity (floats) or table size.
 * A stream whose input is at another sample rate or channel count is appended by mi_streams_convert_append (below) instead of
 * mi_streams_append: the streaming convert_audio, bit-identical to mi_resample_frac on the whole track.
 *
 * mi_streams_emit: mi_stream_emit for every stream of a table in ONE launch, each stream's (row, sample) the same float32 chain.
 *   Stream table (n_streams rows of MI_STREAMS_EMIT_COLS): the stream's rows [pass_lo, pass_hi) of the pass table (MI_EMIT_*
 *   columns, its accumulators in acc_dev), the range [seg_lo, seg_hi) of segs_dev its pass rows' segment ranges are clamped to,
 *   the index of its (mean, std + 1e-8) pair in stats_dev (n_stats pairs; negative: no affine), and its stems (S, channels, n) at
 *   float offset out_off of out_dev.  max_n >= every n (grid size); rows with n = 0 write nothing.
 * mi_streams_append: row s of the table (MI_APPEND_COLS) writes the stream's new block, (channels, n) float32 at the DEVICE
 *   address `src` (row stride n), into columns [col, col + n) of its window (channels, dst_len) at float offset dst_off of win_dev,
 *   as `(x - mean) / s` (mi_track_affine inverse = 0) when its stats index names a pair of stats_dev.  `src` is trusted: the
 *   caller names live blocks of at least channels * n floats; the writes are clamped to the window.
 * mi_streams_compact: row r of the table (MI_COMPACT_COLS) copies n floats from float offset src_off of src_dev to dst_off of
 *   dst_dev and writes zeros after them up to len floats (src_dev and dst_dev must not overlap); max_len >= every len. */
#define MI_STREAMS_EMIT_PASS_LO 0
#define MI_STREAMS_EMIT_PASS_HI 1
#define MI_STREAMS_EMIT_SEG_LO 2
#define MI_STREAMS_EMIT_SEG_HI 3
#define MI_STREAMS_EMIT_STATS 4
#define MI_STREAMS_EMIT_OUT_OFF 5
#define MI_STREAMS_EMIT_N 6
#define MI_STREAMS_EMIT_COLS 7
#define MI_APPEND_SRC 0
#define MI_APPEND_N 1
#define MI_APPEND_DST_OFF 2
#define MI_APPEND_DST_LEN 3
#define MI_APPEND_COL 4
#define MI_APPEND_STATS 5
#define MI_APPEND_COLS 6
#define MI_COMPACT_SRC_OFF 0
#define MI_COMPACT_DST_OFF 1
#define MI_COMPACT_N 2
#define MI_COMPACT_LEN 3
#define MI_COMPACT_COLS 4
int mi_streams_emit(const float *acc_dev, int64_t acc_capacity, int32_t n_sources, int32_t channels, const int64_t *streams_dev,
                    int32_t n_streams, int64_t max_n, const int64_t *passes_dev, int32_t n_passes, const int64_t *segs_dev, int32_t n_segs,
                    const float *weights_dev, int64_t weights_capacity, const float *scales_dev, int32_t n_members, int32_t shifts,
                    int32_t bag, const float *stats_dev, int32_t n_stats, float *out_dev, int64_t out_capacity, void *stream);
int mi_streams_append(float *win_dev, int64_t win_capacity, int32_t channels, const int64_t *table_dev, int32_t n_streams, int64_t max_n,
                      const float *stats_dev, int32_t n_stats, void *stream);
int mi_streams_compact(float *dst_dev, int64_t dst_capacity, const float *src_dev, int64_t src_capacity, const int64_t *table_dev,
                       int32_t n_rows, int64_t max_len, void *stream);

/* mi_streams_convert_append: `convert_audio` (channel map + julius.resample_frac, demucs/audio.py:169-172) for streams, fused with
 *   mi_streams_append's write: the concatenation of what a stream's calls write equals mi_resample_frac on the whole row bit for
 *   bit, for every partition of the input.  With old / new the rates divided by their gcd, width and klen = 2 * width + old as for
 *   mi_resample_frac, every output y[n * new + i] is the same chain (acc = 0; k ascending; acc = fmaf(kernel[i][k],
 *   x[clamp(n * old - width + k, 0, L - 1)], acc)).  Frame n (outputs n * new .. n * new + new - 1) is final once
 *   n * old + width + old <= pushed, so after P input samples ready(P) = new * max(0, (P - width - old) / old + 1) outputs exist;
 *   the final call (total >= 0) writes the rest up to floor(new * total / old) with the right taps clamped to x[total - 1].
 *   Row s of the table (MI_CVT_COLS int64) is one stream of the call:
 *     SRC, SRC_CH, N_IN   its new block (src_ch, n_in) float32 at the DEVICE address src (row stride n_in; trusted as in
 *                         mi_streams_append).  Output row c reads source row 0 when src_ch == 1, else row min(c, src_ch - 1);
 *     BEFORE              input samples pushed before this block;
 *     HIST_LEN, HIST_RD, HIST_WR, HIST_START, HIST_NEXT
 *                         the carried input: (channels, hist_len) floats at float offset hist_rd of hist_dev hold inputs
 *                         [hist_start, before) of every output row; the call writes inputs [hist_next, before + n_in) (at most
 *                         hist_len of them) at float offset hist_wr.  The two sides must differ: one launch reads one and writes
 *                         the other.  hist_next = max(0, n * old - width) for the first frame n that is not ready, so
 *                         before + n_in - hist_next <= klen - 1; hist_next < 0: nothing is written (the final call);
 *     OUT0, N_OUT         the first output index (a multiple of new) and the number of outputs to write;
 *     TOTAL               the total input length when this is the stream's final call, else negative;
 *     OLD, NEW, WIDTH, BANK_OFF
 *                         its rate entry; the kernel bank TRANSPOSED, (klen, new) float32, at float offset bank_off of bank_dev.
 *                         width == 0 (equal rates): outputs are the inputs OUT0 .. through the channel map, no filter, no history;
 *     DST_OFF, DST_LEN, COL, STATS
 *                         outputs go to columns [col, col + n_out) of the (channels, dst_len) window at float offset dst_off of
 *                         win_dev, as `(y - mean) / s` (mi_track_affine inverse = 0) when stats names a pair of stats_dev.
 *   A workgroup takes 8 * G consecutive frames of one (stream, channel) row, G = min(4, (lds_floats - 2 * width) / (8 * old)) >= 1
 *   (1024 samples when width == 0); max_groups >= every row's number of such runs (grid size); lds_floats <= MI_CVT_LDS_FLOATS is
 *   the staging area, >= 8 * old + 2 * width for every row.  Reads and writes of win_dev / hist_dev / bank_dev are clamped to the
 *   declared capacities (floats): a wrong table changes results, never memory outside the buffers.  A one-row table with a plain
 *   (channels, n_out) output buffer as the window serves a single stream. */
#define MI_CVT_SRC 0
#define MI_CVT_SRC_CH 1
#define MI_CVT_N_IN 2
#define MI_CVT_BEFORE 3
#define MI_CVT_HIST_LEN 4
#define MI_CVT_HIST_RD 5
#define MI_CVT_HIST_WR 6
#define MI_CVT_HIST_START 7
#define MI_CVT_HIST_NEXT 8
#define MI_CVT_OUT0 9
#define MI_CVT_N_OUT 10
#define MI_CVT_TOTAL 11
#define MI_CVT_OLD 12
#define MI_CVT_NEW 13
#define MI_CVT_WIDTH 14
#define MI_CVT_BANK_OFF 15
#define MI_CVT_DST_OFF 16
#define MI_CVT_DST_LEN 17
#define MI_CVT_COL 18
#define MI_CVT_STATS 19
#define MI_CVT_COLS 20
#define MI_CVT_LDS_FLOATS 16384
int mi_streams_convert_append(float *win_dev, int64_t win_capacity, int32_t channels, const int64_t *table_dev, int32_t n_streams,
                              int64_t max_groups, const float *bank_dev, int64_t bank_capacity, float *hist_dev, int64_t hist_capacity,
                              const float *stats_dev, int32_t n_stats, int32_t lds_floats, void *stream);

/* ---- wire PCM in (demucs_amd/csrc/ingest.hip, pcm_ingest.h) ------------------------------------------------------------------
 * A block of a live feed as it comes off the wire: n frames of src_ch channels, little-endian, the channels interleaved per frame.
 *   MI_PCM_I16   2 bytes per sample, value float32(v) * 2^-15;
 *   MI_PCM_I24   3 bytes per sample, packed, sign-extended from bit 23, value float32(v) * 2^-23;
 *   MI_PCM_F32   4 bytes per sample, the bits unchanged (NaN, +-Inf, -0 and subnormals as they are).
 * Both products are exact in float32, so a PCM block gives the bits the float entries give for `v / 32768` (`v / 8388608`).
 * MI_PCM_PLANAR names a planar float32 (channels, n) block in a table of the entries below: the row then behaves exactly as a row
 * of the float entry (mi_streams_append / mi_streams_convert_append), so one launch serves a mix of formats.
 * The source address must be aligned to the sample width (any byte address for MI_PCM_I24); no byte outside
 * [src, src + n * src_ch * width) is read.  The channel map is convert_audio_channels' per-sample one: a mono source feeds every
 * destination row, otherwise row c reads source channel c (src_ch >= channels).
 *
 * mi_pcm_planar: one block at the DEVICE address src_dev -> planar float32 (channels, n) at dst_dev, as `(x - mean) / s`
 *   (mi_track_affine inverse = 0) when stats_dev names a (mean, s) pair; n = 0 does nothing.
 * mi_streams_append_pcm: mi_streams_append with a format per row.  Row s of the table (MI_APPEND_PCM_COLS) is MI_APPEND_*'s six
 *   columns (N in frames), then FMT (MI_PCM_*) and SRC_CH (ignored for MI_PCM_PLANAR, whose source is (channels, n) floats).  The
 *   writes are clamped to the row's window columns as in mi_streams_append; a row with an unknown format, a misaligned source or a
 *   channel count the map does not take writes nothing.  max_bytes >= every row's source size in bytes (grid size).
 * mi_streams_convert_append_pcm: mi_streams_convert_append with a format per row: MI_CVT_*'s twenty columns, then FMT
 *   (MI_CVT_PCM_COLS).  The block is (n_in frames, src_ch) in that format; the carried history stays float32, and the filter chain
 *   is the same code, so the outputs equal mi_streams_convert_append's on the converted planar floats bit for bit. */
#define MI_PCM_PLANAR 0
#define MI_PCM_I16 1
#define MI_PCM_I24 2
#define MI_PCM_F32 3
#define MI_APPEND_PCM_SRC 0
#define MI_APPEND_PCM_N 1
#define MI_APPEND_PCM_DST_OFF 2
#define MI_APPEND_PCM_DST_LEN 3
#define MI_APPEND_PCM_COL 4
#define MI_APPEND_PCM_STATS 5
#define MI_APPEND_PCM_FMT 6
#define MI_APPEND_PCM_SRC_CH 7
#define MI_APPEND_PCM_COLS 8
#define MI_CVT_PCM_FMT 20
#define MI_CVT_PCM_COLS 21
int mi_pcm_planar(const void *src_dev, int32_t fmt, int32_t src_ch, int64_t n, int32_t channels, const float *stats_dev, float *dst_dev,
                  void *stream);
int mi_streams_append_pcm(float *win_dev, int64_t win_capacity, int32_t channels, const int64_t *table_dev, int32_t n_streams,
                          int64_t max_bytes, const float *stats_dev, int32_t n_stats, void *stream);
int mi_streams_convert_append_pcm(float *win_dev, int64_t win_capacity, int32_t channels, const int64_t *table_dev, int32_t n_streams,
                                  int64_t max_groups, const float *bank_dev, int64_t bank_capacity, float *hist_dev,
                                  int64_t hist_capacity, const float *stats_dev, int32_t n_stats, int32_t lds_floats, void *stream);

/* mi_resample_frac: `julius.resample_frac` as called by `demucs.audio.convert_audio` (demucs/audio.py:169-172), the step
 *   `Separator.separate_tensor` runs first when the input sample rate differs from the model's (demucs/api.py:265-266).
 *   old_sr / new_sr already divided by their gcd; table_dev (new_sr, 2*width + old_sr) is julius' windowed-sinc kernel bank
 *   (built by demucs_amd/audio.py); x_dev (rows, length) -> y_dev (rows, out_length), out_length <= new_sr*(length/old_sr + 1). */
int mi_resample_frac(const float *x_dev, int32_t rows, int64_t length, const float *table_dev, int32_t old_sr, int32_t new_sr,
                     int32_t width, float *y_dev, int64_t out_length, void *stream);

/* ---- track-level pre / post processing of `Separator` and the CLI, on the device -------------------------------------------
 * mi_mono_stats: `ref = wav.mean(0)`, then stats_dev[0] = ref.mean(), stats_dev[1] = ref.std() + 1e-8 (unbiased std;
 *   demucs/api.py:267-269), float32 results of float64 accumulation in a fixed order.  wav_dev (channels, length);
 *   scratch_dev: mi_mono_stats_scratch_bytes() bytes of device memory.  The scalars never visit the host.
 * mi_track_affine: in place on x_dev (numel floats): inverse = 0: `x -= mean; x /= std` (api.py:268-269), inverse = 1:
 *   `x *= std; x += mean` (api.py:285-288), each as two separately rounded float32 operations like the reference's. */
int32_t mi_mono_stats_scratch_bytes(void);
int mi_mono_stats(const float *wav_dev, int32_t channels, int64_t length, void *scratch_dev, float *stats_dev, void *stream);
int mi_track_affine(float *x_dev, int64_t numel, const float *stats_dev, int32_t inverse, void *stream);

/* mi_mono_stats for a track that arrives block by block (demucs_amd/csrc/stats_stream.hip): the same (mean, s), bit for bit, for
 * every partition of the track.  mi_mono_stats runs on a fixed grid of 262 144 threads, position p belongs to thread p % 262144
 * and a thread adds its positions in ascending order, so the carried state is one (sum, sum of squares) pair of doubles per
 * thread: state_dev, mi_mono_stats_state_bytes() = 2 x 262 144 x 8 bytes (4 MiB), 8-byte aligned, all-zero bytes at the start.
 * mi_mono_stats_update: adds track positions [before, before + n) to the state.  fmt MI_PCM_PLANAR: src_dev is a contiguous planar
 *   float32 (channels, n) block (src_ch is ignored); MI_PCM_I16 / _I24 / _F32: n interleaved frames of src_ch channels under
 *   mi_pcm_planar's rules (alignment to the sample width, the channel map, no byte outside the block is read).  The caller
 *   passes `before` as the sum of the earlier blocks' n; n = 0 does nothing.  Nothing outside the state is written.
 * mi_mono_stats_finish: stats_dev[0], stats_dev[1] as mi_mono_stats writes them for the `length` positions added so far;
 *   scratch_dev: mi_mono_stats_scratch_bytes() bytes.  The state is only read: a second call gives the same result, and more
 *   blocks may follow. */
int32_t mi_mono_stats_state_bytes(void);
int mi_mono_stats_update(const void *src_dev, int32_t fmt, int32_t src_ch, int64_t n, int32_t channels, int64_t before, void *state_dev,
                         void *stream);
int mi_mono_stats_finish(const void *state_dev, int64_t length, void *scratch_dev, float *stats_dev, void *stream);

/* ---- evaluation: the nSDR of separated stems against reference stems (demucs/evaluate.py:30-43, `new_sdr`) --------------------
 * For source s over channels c and positions p, r = (double)ref[s, c, p], e = (double)est[s, c, p]:
 *   num[s] = sum r * r,  den[s] = sum (r - e) * (r - e),  both in float64; the host takes 10 * log10((num + 1e-7) / (den + 1e-7)).
 * Position p of a track belongs to slot p % 131072 (a constant of the build); a slot adds its positions in ascending order and
 * the channels of a position in ascending order, and a fixed tree reduces the slots, so the sums have the same bits for the whole
 * track in one call and for every partition of it into blocks (demucs_amd/csrc/sdr_sums.h).  NaN and Inf samples reach the sums.
 * state_dev: mi_sdr_state_bytes(n_sources) = n_sources x 2 x 131072 x 8 bytes (2 MiB per source), 8-byte aligned, all-zero bytes at
 *   the start of a track; scratch_dev: mi_sdr_scratch_bytes(n_sources) bytes, 8-byte aligned.  1 <= n_sources <= 8; the byte
 *   counts are 0 outside that range.
 * mi_sdr_update: adds track positions [before, before + n) to the state.  Estimates: planar float32 rows, (source s, channel c)
 *   at est_dev + (s * channels + c) * est_stride, est_stride >= n -- the span a stream has just emitted, or a slice of a longer
 *   (S, C, N) tensor, is read where it lies.  References: refs is a HOST array of device pointers.  fmt MI_PCM_PLANAR: refs[0] is
 *   float32 rows in the same form with ref_stride >= n (src_ch is ignored); MI_PCM_I16 / _I24 / _F32: refs[s] is source s's
 *   block of n interleaved frames of src_ch channels (ref_stride is ignored) under mi_pcm_planar's rules: alignment to the sample
 *   width, a mono source feeds every channel and else src_ch >= channels, no byte outside a block is read.  The caller passes
 *   `before` as the sum of the earlier blocks' n; n = 0 does nothing.  Nothing outside the state is written.
 * mi_sdr_finish: sums_dev[n_sources][2] doubles, the raw (num, den) of the positions added so far.  The state is only read: a
 *   second call gives the same bits, and more blocks may follow.
 * mi_sdr: B independent tracks, ref_dev and est_dev contiguous (B, n_sources, channels, length) float32, sums_dev
 *   [B][n_sources][2]: per track a memset of state_dev, one mi_sdr_update and mi_sdr_finish -- the same device code.  length = 0
 *   gives zeros. */
int64_t mi_sdr_state_bytes(int32_t n_sources);
int64_t mi_sdr_scratch_bytes(int32_t n_sources);
int mi_sdr_update(const void *const *refs, int32_t fmt, int32_t src_ch, int64_t ref_stride, const float *est_dev, int64_t est_stride,
                  int32_t n_sources, int32_t channels, int64_t n, int64_t before, void *state_dev, void *stream);
int mi_sdr_finish(const void *state_dev, int32_t n_sources, void *scratch_dev, double *sums_dev, void *stream);
int mi_sdr(const float *ref_dev, const float *est_dev, int32_t B, int32_t n_sources, int32_t channels, int64_t length, void *state_dev,
           void *scratch_dev, double *sums_dev, void *stream);

/* mi_prevent_clip: `demucs.audio.prevent_clip(wav, mode)` (demucs/audio.py:218-234) on device stems: y = x / max(1.01 * max|x|, 1)
 *   ("rescale"; the peak is reduced on the device into peak_dev, 4 bytes), clamp(x, -0.99, 0.99) or tanh(x).
 * mi_two_stems: the `--two-stems` outputs of demucs/separate.py:189-218: minus = 0: y = 0 + (every stem but `selected`, in
 *   index order) -- the "no_STEM" file; minus = 1: y = origin - stems[selected] -- the "minus_STEM" file.  stems_dev is a
 *   HOST array of n_stems (<= 8) device pointers of numel floats each. */
#define MI_CLIP_RESCALE 1
#define MI_CLIP_CLAMP 2
#define MI_CLIP_TANH 3
int mi_prevent_clip(const float *x_dev, int64_t numel, int32_t mode, void *peak_dev, float *y_dev, void *stream);
int mi_two_stems(const float *const *stems_dev, int32_t n_stems, int32_t selected, const float *origin_dev, int32_t minus, int64_t numel,
                 float *y_dev, void *stream);

/* ---- delivery: the stems as the reference saves them, every output of a call in ONE launch -----------------------------------
 * The reference's save loop (demucs/separate.py:178-218) forms the `--two-stems` outputs and hands each to `save_audio`
 * (demucs/audio.py:236-265): `prevent_clip` (audio.py:218-234), then `i16_pcm` (audio.py:175-181) or float32, channels
 * interleaved per frame.  Row r of the table (MI_DELIVER_COLS int64, a DEVICE array) is ONE such output:
 *     SRC       DEVICE address of the contiguous float32 (n_sources, channels, n) stems (trusted, as MI_APPEND_SRC is);
 *     ORIGIN    DEVICE address of the (channels, n) float32 mix, or 0 (needed by KIND 2 only; trusted);
 *     N         frames;
 *     KIND      MI_DELIVER_STEM: stem SEL; MI_DELIVER_ADD: 0 + every stem but SEL in index order (separate.py:207-210, the
 *               "no_STEM" file); MI_DELIVER_MINUS: origin - stem SEL (separate.py:197, the "minus_STEM" file);
 *     SEL       source index;
 *     CLIP      0 (none) or MI_CLIP_*, as mi_prevent_clip;
 *     PEAK      the row's slot in peaks_dev (n_peaks uint32 bit patterns; read only by MI_CLIP_RESCALE rows);
 *     FMT       MI_DELIVER_I16: clamp to [-1, 1], times 32767.f, truncated toward zero (a NaN becomes 0); MI_DELIVER_F32: the
 *               clipped value as it is;
 *     DST_OFF   byte offset of the row's (n, channels) interleaved frames in dst_dev: channel c of frame j at
 *               DST_OFF + (j * channels + c) * (2 or 4).
 *   Every step is a separately rounded float32 operation in the reference's order, by the device functions mi_prevent_clip and
 *   mi_two_stems are built from.  A row is skipped (nothing of it is read or written) when its frames leave dst_capacity (bytes),
 *   DST_OFF is negative or no multiple of 4, N <= 0, SRC is 0, KIND / SEL / CLIP / FMT is out of range, a MI_CLIP_RESCALE row's PEAK is
 *   not in [0, n_peaks), or a MI_DELIVER_MINUS row has no ORIGIN.  dst_dev is 4-byte aligned; max_n >= every N (grid size).
 * mi_deliver_peaks: zeroes peaks_dev (one memset) and reduces max |value| of every MI_CLIP_RESCALE row into its slot, on the
 *   unsigned bit patterns as mi_prevent_clip does (a NaN sample makes the row's peak NaN, as torch's abs().max()).  The peak is
 *   per row, as the reference calls save_audio per output.  Call it before mi_deliver_pcm on the same stream when a row rescales;
 *   nothing synchronises with the host.
 * mi_deliver_pcm: writes every row's frames.  peaks_dev may be null when n_peaks == 0 (rescaling rows are then skipped). */
#define MI_DELIVER_SRC 0
#define MI_DELIVER_ORIGIN 1
#define MI_DELIVER_N 2
#define MI_DELIVER_KIND 3
#define MI_DELIVER_SEL 4
#define MI_DELIVER_CLIP 5
#define MI_DELIVER_PEAK 6
#define MI_DELIVER_FMT 7
#define MI_DELIVER_DST_OFF 8
#define MI_DELIVER_COLS 9
#define MI_DELIVER_STEM 0
#define MI_DELIVER_ADD 1
#define MI_DELIVER_MINUS 2
#define MI_DELIVER_I16 0
#define MI_DELIVER_F32 1
int mi_deliver_peaks(const int64_t *table_dev, int32_t n_rows, int64_t max_n, int32_t n_sources, int32_t channels, void *peaks_dev,
                     int32_t n_peaks, int64_t dst_capacity, void *stream);
int mi_deliver_pcm(const int64_t *table_dev, int32_t n_rows, int64_t max_n, int32_t n_sources, int32_t channels, const void *peaks_dev,
                   int32_t n_peaks, void *dst_dev, int64_t dst_capacity, void *stream);

/* mi_deliver_resample_pcm: delivery of a STREAM's outputs at another sample rate R than the model's M, what a user of the reference
 *   writes as `save_audio(julius.resample_frac(v, M, R), path, samplerate=R, clip=...)` for each output v of the save loop
 *   (demucs/audio.py:169-172,175-181,218-265 on the outputs of demucs/separate.py:178-218): the `--two-stems` value of
 *   mi_deliver_pcm, then mi_resample_frac's chain on it (old / new = M / R divided by their gcd; acc = 0; k ascending;
 *   acc = fmaf(kernel[i][k], v[clamp(n * old - width + k, 0, L - 1)], acc) for output n * new + i), then prevent_clip and i16_pcm or
 *   float32, channels interleaved.  The concatenation of what a stream's calls write equals that chain on the whole track bit for
 *   bit, for every partition: frame n is written once n * old + width + old <= emitted (mi_streams_convert_append's `ready` rule
 *   with the model-rate samples the stream has emitted as the input), the final call (TOTAL >= 0) writes the rest up to
 *   floor(new * total / old) with the right taps clamped to v[total - 1].
 *   Row r of the table (MI_RATE_COLS int64, a DEVICE array) is ONE output of one stream on one call:
 *     SRC, N_IN           DEVICE address of the stream's newly emitted float32 stems (n_sources, channels, n_in) (trusted, as
 *                         MI_DELIVER_SRC; may be 0 when n_in == 0);
 *     BEFORE              model-rate samples emitted before this call;
 *     KIND, SEL, CLIP, FMT  as MI_DELIVER_*: KIND is MI_DELIVER_STEM or MI_DELIVER_ADD, CLIP 0, MI_CLIP_CLAMP or MI_CLIP_TANH (the
 *                         whole-track modes "minus" and "rescale" do not exist on a stream: this entry skips such a row.  A stream
 *                         rescales in two passes by mi_deliver_resample_peaks and mi_deliver_resample_pcm_peaks, below);
 *     OLD, NEW, WIDTH, BANK_OFF   the rate entry as MI_CVT_*: the kernel bank TRANSPOSED, (klen, new) float32, at float offset bank_off
 *                         of bank_dev; width >= 1 (equal rates are mi_deliver_pcm's);
 *     OUT0, N_OUT         the first output frame (a multiple of new) and the number of frames to write;
 *     TOTAL               before + n_in when this is the stream's final call, else negative;
 *     HIST_LEN, HIST_RD, HIST_WR, HIST_START, HIST_NEXT
 *                         the carried VALUES of this output, as MI_CVT_HIST_*: (channels, hist_len) floats at float offset hist_rd
 *                         of hist_dev hold positions [hist_start, before); the call writes positions [hist_next, before + n_in) (at
 *                         most hist_len, <= klen - 1 by the same rule) at float offset hist_wr, a side apart from the read one;
 *                         hist_next < 0: nothing is written (the final call).  hist_len == 0: no history, for a stream whose only
 *                         call is its final one (before == 0, hist_next < 0);
 *     DST_OFF             byte offset of the row's (n_out, channels) interleaved frames in dst_dev (a multiple of 4).
 *   A workgroup takes 8 * G consecutive frames of one row for all channels, G = min(4, (lds_floats / channels - 2 * width) / (8 * old))
 *   >= 1; max_groups >= every row's number of such runs (grid size); lds_floats <= MI_RATE_LDS_FLOATS is the staging area,
 *   >= channels * (8 * old + 2 * width) for every row.  A row is skipped whole (nothing of it is read or written, its history
 *   included) when its frames leave dst_capacity (bytes), DST_OFF is negative or no multiple of 4, a history side or the bank leaves
 *   its capacity (floats) or the sides overlap, KIND / SEL / CLIP / FMT / OLD / NEW / WIDTH is out of range, OUT0 is no multiple
 *   of NEW, TOTAL >= 0 differs from before + n_in, or the staging area is too small for it.  dst_dev is 4-byte aligned. */
#define MI_RATE_SRC 0
#define MI_RATE_N_IN 1
#define MI_RATE_BEFORE 2
#define MI_RATE_KIND 3
#define MI_RATE_SEL 4
#define MI_RATE_CLIP 5
#define MI_RATE_FMT 6
#define MI_RATE_OLD 7
#define MI_RATE_NEW 8
#define MI_RATE_WIDTH 9
#define MI_RATE_BANK_OFF 10
#define MI_RATE_OUT0 11
#define MI_RATE_N_OUT 12
#define MI_RATE_TOTAL 13
#define MI_RATE_HIST_LEN 14
#define MI_RATE_HIST_RD 15
#define MI_RATE_HIST_WR 16
#define MI_RATE_HIST_START 17
#define MI_RATE_HIST_NEXT 18
#define MI_RATE_DST_OFF 19
#define MI_RATE_COLS 20
#define MI_RATE_LDS_FLOATS 16384
int mi_deliver_resample_pcm(const int64_t *table_dev, int32_t n_rows, int64_t max_groups, int32_t n_sources, int32_t channels,
                            const float *bank_dev, int64_t bank_capacity, float *hist_dev, int64_t hist_capacity, int32_t lds_floats,
                            void *dst_dev, int64_t dst_capacity, void *stream);

/* ---- "rescale" on a stream: peaks measured by one pass over the stream, frames delivered by a second ---------------------------
 * `prevent_clip(wav, "rescale")` divides by max(1.01 * wav.abs().max(), 1) (demucs/audio.py:225-227), the whole output's peak.  A
 * stream's forwards are deterministic, so a first pass that keeps only max |value| per output (4 bytes each, on the device) finds
 * the peaks a second pass of the same stream divides by; the frames are mi_deliver_peaks + mi_deliver_pcm's on the whole track.
 * peaks_dev: n_peaks uint32, the bit patterns of float32 max |value| as mi_deliver_peaks writes them (a NaN sample leaves a NaN
 * pattern, which orders above +inf).  The caller zeroes a slot at the start of a track; nothing here does, and nothing
 * synchronises with the host.
 * mi_deliver_peaks_update: mi_deliver_peaks without the memset: max |value| of every row goes into peaks_dev[PEAK] by atomicMax,
 *   so the slots carry the running maximum over the calls of a track.  Rows are MI_DELIVER_* rows with CLIP == MI_CLIP_RESCALE
 *   (others are skipped); FMT and DST_OFF are not read, and no row is skipped for a destination.  The other skip rules are
 *   mi_deliver_peaks': N <= 0, SRC 0, KIND / SEL out of range, PEAK outside [0, n_peaks), a MI_DELIVER_MINUS row without ORIGIN.
 *   Delivering at the model's rate with peaks measured before needs no entry of its own: mi_deliver_pcm takes peaks_dev.
 * mi_deliver_resample_peaks: mi_deliver_resample_pcm's arguments without dst, on the same MI_RATE_* rows with CLIP ==
 *   MI_CLIP_RESCALE (others are skipped whole); FMT and DST_OFF are not read.  The history is carried exactly as
 *   mi_deliver_resample_pcm carries it, every frame that entry would write on this call is computed by the same fmaf chain, and
 *   max |frame| over frames [OUT0, OUT0 + N_OUT) and channels < channels goes into peaks_dev[slots_dev[r]] for row r: a
 *   reduction over the wave, then one atomicMax per wave, none when the wave's maximum is 0.  slots_dev: n_rows int32, a DEVICE
 *   array.  A row whose slot is outside [0, n_peaks) is skipped whole, its history included.
 * mi_deliver_resample_pcm_peaks: mi_deliver_resample_pcm with slots_dev and peaks_dev (read only).  It also takes rows with CLIP
 *   == MI_CLIP_RESCALE and writes v / max(1.01 * peak, 1) for them (mi_prevent_clip's operations, the divisor formed once per
 *   workgroup from peaks_dev[slots_dev[r]]); such a row with a slot outside [0, n_peaks) is skipped whole.  slots_dev[r] is not
 *   read for a row of another CLIP, whose bytes are mi_deliver_resample_pcm's.  peaks_dev may be null when n_peaks == 0. */
int mi_deliver_peaks_update(const int64_t *table_dev, int32_t n_rows, int64_t max_n, int32_t n_sources, int32_t channels, void *peaks_dev,
                            int32_t n_peaks, void *stream);
int mi_deliver_resample_peaks(const int64_t *table_dev, int32_t n_rows, int64_t max_groups, int32_t n_sources, int32_t channels,
                              const float *bank_dev, int64_t bank_capacity, float *hist_dev, int64_t hist_capacity, int32_t lds_floats,
                              const int32_t *slots_dev, void *peaks_dev, int32_t n_peaks, void *stream);
int mi_deliver_resample_pcm_peaks(const int64_t *table_dev, int32_t n_rows, int64_t max_groups, int32_t n_sources, int32_t channels,
                                  const float *bank_dev, int64_t bank_capacity, float *hist_dev, int64_t hist_capacity, int32_t lds_floats,
                                  void *dst_dev, int64_t dst_capacity, const int32_t *slots_dev, const void *peaks_dev, int32_t n_peaks,
                                  void *stream);

/* ---- delivery of gain-weighted remixes of the stems and of the input mix, every remix of a call in ONE launch -------------------
 * What a user of the reference writes after `separate_tensor` as `save_audio(sum(g * x for ...), path, clip=...)`: vocals lowered
 * instead of removed, drums raised, `mix - vocals`.  For channel c and frame j of a row, with float32 gains g_mix, g_0 .. g_{S-1}:
 *     acc = 0.0f;  if g_mix != 0: acc = acc + g_mix * o(c, j);  for k ascending, if g_k != 0: acc = acc + g_k * s_k(c, j)
 * every product and sum a separately rounded float32 operation; a term whose gain is exactly 0 is NOT READ (a NaN or Inf in a
 * muted stem does not reach the output).  CLIP, FMT and the interleaving follow as in mi_deliver_pcm.  Gains of 1 on every stem
 * but SEL give MI_DELIVER_ADD's bits; {g_mix 1, g_SEL -1} gives MI_DELIVER_MINUS's int16 bytes, and its float32 values as numbers
 * (only a -0.0 can come out as +0.0).  Row r of the table (MI_MIX_COLS int64, a DEVICE array) is ONE remix:
 *     SRC, N         as MI_DELIVER_SRC / _N: the contiguous float32 (n_sources, channels, n) stems (trusted), n_sources <= 8;
 *     ORIGIN         DEVICE address of frame 0 of the mix's channel 0, or 0 (read only when g_mix != 0; trusted);
 *     ORIGIN_PITCH   floats between the mix's channel rows: channel c, frame j at ORIGIN + c * ORIGIN_PITCH + j.  A stream names
 *                    its input window here, whose rows are longer than n;
 *     ORIGIN_AFFINE  two float32 in one int64, mean in the low half and s in the high: when AFFINE_ON is not 0 the mix is stored
 *     AFFINE_ON      normalised, and o = w * s, then + mean (two rounded operations, mi_track_affine's restore);
 *     GAINS          nine float32 in five int64 (two a word, low half first): g_mix, g_0 .. g_7; those past n_sources are not read;
 *     CLIP, PEAK, FMT, DST_OFF   as MI_DELIVER_*.
 *   A row is skipped whole (nothing of it is read or written) under mi_deliver_pcm's rules -- its frames leave dst_capacity, DST_OFF
 *   is negative or no multiple of 4, N <= 0, SRC is 0, CLIP / FMT out of range, a MI_CLIP_RESCALE row's PEAK outside [0, n_peaks) --
 *   and when a gain among g_mix, g_0 .. g_{n_sources-1} is not finite, all of them are 0, g_mix != 0 without ORIGIN, or g_mix != 0
 *   with ORIGIN_PITCH < N.  No kernel uses scratch memory and nothing synchronises with the host.
 * mi_deliver_mix_pcm: writes every row's frames, four frames a thread on mi_deliver_pcm's grid, 16-byte loads where base, pitch
 *   and N allow.  peaks_dev may be null when n_peaks == 0.
 * mi_deliver_mix_peaks: zeroes peaks_dev and reduces max |value| of every MI_CLIP_RESCALE row into its slot, as mi_deliver_peaks.
 * mi_deliver_mix_peaks_update: the same without the memset and without a destination (FMT, DST_OFF not read): the slots carry the
 *   running maximum over the calls of a track, as mi_deliver_peaks_update's. */
#define MI_MIX_SRC 0
#define MI_MIX_N 1
#define MI_MIX_ORIGIN 2
#define MI_MIX_ORIGIN_PITCH 3
#define MI_MIX_ORIGIN_AFFINE 4
#define MI_MIX_AFFINE_ON 5
#define MI_MIX_GAINS 6
#define MI_MIX_CLIP 11
#define MI_MIX_PEAK 12
#define MI_MIX_FMT 13
#define MI_MIX_DST_OFF 14
#define MI_MIX_COLS 15
#define MI_MIX_MAX_SOURCES 8
int mi_deliver_mix_pcm(const int64_t *table_dev, int32_t n_rows, int64_t max_n, int32_t n_sources, int32_t channels,
                       const void *peaks_dev, int32_t n_peaks, void *dst_dev, int64_t dst_capacity, void *stream);
int mi_deliver_mix_peaks(const int64_t *table_dev, int32_t n_rows, int64_t max_n, int32_t n_sources, int32_t channels, void *peaks_dev,
                         int32_t n_peaks, int64_t dst_capacity, void *stream);
int mi_deliver_mix_peaks_update(const int64_t *table_dev, int32_t n_rows, int64_t max_n, int32_t n_sources, int32_t channels,
                                void *peaks_dev, int32_t n_peaks, void *stream);

/* ---- remixes whose gains change along the track (gain automation), every such remix of a call in ONE launch ---------------------
 * What a user of the reference writes after `separate_tensor` as `save_audio(sum(g(p) * x for ...), path, clip=...)` with gain
 * curves g(p) made of steps and linear ramps: vocals brought down for a chorus and back up, a fade written over track time.  A row
 * has base gains and an ordered list of CHANGES (AT, RAMP, target gains G).  At track position p = T0 + j the change in force is
 * the last one with AT <= p (none: the base gains); with P the gains before it (the change before it fully reached, or the base
 * gains) and k = p - AT, term i has the gain
 *     k >= RAMP:  G_i exactly;        else  t = float(k) / float(RAMP),  g_i = P_i + (G_i - P_i) * t
 * every conversion, quotient, difference, product and sum a separately rounded float32 operation (no fused multiply-add).  Frame
 * AT therefore still has the old gains and frame AT + RAMP is the first with the new ones; RAMP = 0 is a step.  The value is
 * mi_deliver_mix_pcm's chain with these per-sample gains: acc = 0, then acc = acc + g_i * x_i for the mix first and the stems in
 * order, a term being added only at the samples where its gain is not 0 (a NaN in a stem stays out of exactly the samples at which
 * the stem is muted; a term none of whose gains is non-zero over a thread's four frames is not loaded).  CLIP, FMT and the
 * interleaving follow as in mi_deliver_pcm.  A row without changes, or whose changes all equal its base gains, gives
 * mi_deliver_mix_pcm's bytes.
 * The table (table_len int64, a DEVICE array, table_len <= INT32_MAX) begins with n_rows rows of MI_AUTO_COLS words; the changes
 * lie anywhere in the same table.  Row r:
 *     SRC .. DST_OFF   MI_MIX_*'s columns at the same indices; GAINS are the BASE gains, in force before the row's first change;
 *     T0               track position of the row's frame 0;
 *     CHG_OFF, CHG_N   the row's changes: CHG_N records of MI_AUTO_CHG_COLS words from word CHG_OFF of the table, each
 *                      AT, RAMP (int64) and nine float32 target gains in five words, packed as MI_MIX_GAINS.
 *   There is no cap on CHG_N; the change in force is found by bisection over AT.  A row is skipped whole (nothing of it is written)
 *   under mi_deliver_mix_pcm's rules, except that all gains may be 0 (a fade to silence), the mix being needed (ORIGIN, ORIGIN_PITCH)
 *   when g_mix is not 0 in the base gains or in any change, and when: the change list reaches outside [0, table_len); changes are
 *   out of order or overlap (AT[i] < AT[i-1] + RAMP[i-1]); RAMP < 0; |AT|, RAMP or |T0| exceed 2^61; a gain of a change is not
 *   finite or exceeds 2^64 in magnitude (so that G - P cannot overflow).  No kernel uses scratch memory, nothing synchronises with
 *   the host.
 * mi_deliver_mix_auto_pcm: writes every row's frames on mi_deliver_mix_pcm's grid (four frames a thread, 16-byte loads and stores
 *   where base, pitch and N allow).  peaks_dev may be null when n_peaks == 0.
 * mi_deliver_mix_auto_peaks: zeroes peaks_dev and reduces max |value| of every MI_CLIP_RESCALE row into its slot, as
 *   mi_deliver_mix_peaks. */
#define MI_AUTO_SRC 0
#define MI_AUTO_N 1
#define MI_AUTO_ORIGIN 2
#define MI_AUTO_ORIGIN_PITCH 3
#define MI_AUTO_ORIGIN_AFFINE 4
#define MI_AUTO_AFFINE_ON 5
#define MI_AUTO_GAINS 6
#define MI_AUTO_CLIP 11
#define MI_AUTO_PEAK 12
#define MI_AUTO_FMT 13
#define MI_AUTO_DST_OFF 14
#define MI_AUTO_T0 15
#define MI_AUTO_CHG_OFF 16
#define MI_AUTO_CHG_N 17
#define MI_AUTO_COLS 18
#define MI_AUTO_CHG_AT 0
#define MI_AUTO_CHG_RAMP 1
#define MI_AUTO_CHG_GAINS 2
#define MI_AUTO_CHG_COLS 7
int mi_deliver_mix_auto_pcm(const int64_t *table_dev, int64_t table_len, int32_t n_rows, int64_t max_n, int32_t n_sources,
                            int32_t channels, const void *peaks_dev, int32_t n_peaks, void *dst_dev, int64_t dst_capacity, void *stream);
int mi_deliver_mix_auto_peaks(const int64_t *table_dev, int64_t table_len, int32_t n_rows, int64_t max_n, int32_t n_sources,
                              int32_t channels, void *peaks_dev, int32_t n_peaks, int64_t dst_capacity, void *stream);

/* ---- loudness of remixes (ITU-R BS.1770-4 / EBU R 128): K-weighted sub-block energies, whole or streamed ------------------------
 * No counterpart in the reference: what a user of it does with a CPU meter on the float stems after `separate_tensor`.  The
 * measured signal of a row is mi_deliver_mix_pcm's value before clipping -- acc = 0, + g_mix * o, + g_k * s_k in index order,
 * float32, a term with gain 0 not read, the mix through ORIGIN / ORIGIN_PITCH / ORIGIN_AFFINE.  It passes two cascaded biquads
 * in float64, each y[n] = b0 x[n] + b1 x[n-1] + b2 x[n-2] - a1 y[n-1] - a2 y[n-2]; coef (a HOST array of 10 doubles, copied
 * into the launch) holds b0, b1, b2, a1, a2 of the first and then of the second.  Sub-block h of a channel is the track positions
 * [h * hop, (h + 1) * hop), and its energy e[c][h] the sum of y * y over them in ascending order, where y comes from running both
 * biquads from zero state over [h * hop - warm, (h + 1) * hop), positions below 0 reading 0.  e[c][h] is a pure function of the
 * values in that window, so the energies of a track have the same bits for every partition of it into calls; against the
 * recursion over the whole track they differ by the filters' response after `warm` samples (below float64 rounding for the
 * BS.1770 filters at warm = 16384 * ceil(fs / 48000)).  Gating and the logarithm are the host's (a few numbers per second).
 * mi_loudness_update: ONE call takes the next N samples of every output of a track (or of a push) in two launches, one that
 *   lays the carried and the new values side by side in work_dev and rewrites the history, one that runs the recursions of the
 *   sub-blocks that became complete, one work item each; nothing synchronises with the host and no atomics are used.
 *   Row r of the table (MI_LOUD_COLS int64, a DEVICE array) is ONE output:
 *     SRC, N, ORIGIN, ORIGIN_PITCH, ORIGIN_AFFINE, AFFINE_ON, GAINS   as MI_MIX_*, at the same indices;
 *     SRC_PITCH           floats between the (source, channel) rows of the stems: source k, channel c, frame j at
 *                         SRC + (k * channels + c) * SRC_PITCH + j (N for a contiguous block; longer for a view of a whole track);
 *     BEFORE              track position of the row's frame 0: the samples of this output taken by earlier calls;
 *     HIST_LEN, HIST_RD, HIST_WR, HIST_START, HIST_NEXT
 *                         the carried VALUES of this output, as MI_RATE_HIST_*: (channels, hist_len) floats at float offset
 *                         hist_rd of hist_dev hold positions [hist_start, before); the call writes positions [hist_next,
 *                         before + n) (at most hist_len) at float offset hist_wr, a side apart from the read one; hist_next < 0:
 *                         nothing is written.  A stream carries from max(0, (before + n) / hop * hop - warm) on: at most
 *                         warm + hop - 1 values;
 *     E_OFF, E_PITCH      the row's energies: (channels, e_pitch) doubles at double offset e_off of energies_dev; the call writes
 *                         e[c][h] for before / hop <= h < (before + n) / hop, every channel;
 *     WORK_OFF, WORK_PITCH  the row's work area: (channels, work_pitch) floats at float offset work_off of work_dev,
 *                         work_pitch >= before - hist_start + n.  Its contents mean nothing after the call.
 *   max_n >= every row's before - hist_start + n, max_blocks >= every row's number of sub-blocks that become complete (grid
 *   sizes; max_blocks == 0: the second launch is left out).  Rows must not share history sides, energies or work areas.
 *   A row is skipped whole (nothing of it is read or written, its history included) under mi_deliver_mix_pcm's rules for SRC, N,
 *   the gains and ORIGIN -- SRC is 0, N <= 0, a gain among g_mix, g_0 .. g_{n_sources-1} is not finite, all of them are 0,
 *   g_mix != 0 without ORIGIN or with ORIGIN_PITCH < N -- and when SRC_PITCH < N; BEFORE or HIST_START is negative, HIST_START >
 *   BEFORE, or before - hist_start > hist_len; a history side leaves hist_capacity (floats) or the sides overlap; HIST_NEXT >= 0
 *   lies outside [hist_start, before + n] or before + n - hist_next > hist_len; a sub-block becomes complete whose window begins
 *   before HIST_START (max(0, before / hop * hop - warm) < hist_start); the energies or the work area leave their capacity
 *   (doubles, floats), E_PITCH < (before + n) / hop or WORK_PITCH is too small; N or BEFORE exceed 2^61.  With hop < 1 or
 *   warm < 0 every row is skipped.  hop and warm are arguments, not constants of the build. */
#define MI_LOUD_SRC 0
#define MI_LOUD_N 1
#define MI_LOUD_ORIGIN 2
#define MI_LOUD_ORIGIN_PITCH 3
#define MI_LOUD_ORIGIN_AFFINE 4
#define MI_LOUD_AFFINE_ON 5
#define MI_LOUD_GAINS 6
#define MI_LOUD_SRC_PITCH 11
#define MI_LOUD_BEFORE 12
#define MI_LOUD_HIST_LEN 13
#define MI_LOUD_HIST_RD 14
#define MI_LOUD_HIST_WR 15
#define MI_LOUD_HIST_START 16
#define MI_LOUD_HIST_NEXT 17
#define MI_LOUD_E_OFF 18
#define MI_LOUD_E_PITCH 19
#define MI_LOUD_WORK_OFF 20
#define MI_LOUD_WORK_PITCH 21
#define MI_LOUD_COLS 22
int mi_loudness_update(const int64_t *table_dev, int32_t n_rows, int64_t max_n, int64_t max_blocks, int32_t n_sources, int32_t channels,
                       const double *coef, int64_t hop, int64_t warm, float *hist_dev, int64_t hist_capacity, double *energies_dev,
                       int64_t energies_capacity, float *work_dev, int64_t work_capacity, void *stream);

/* ---- true peak of remixes (ITU-R BS.1770-4 Annex 2 / EBU R 128): oversampled and sample peaks, whole or streamed -----------------
 * No counterpart in the reference: the other half of a delivery specification (-14 LUFS at no more than -1 dBTP).  The measured
 * signal v[c][j], 0 <= j < L, of a row is mi_deliver_mix_pcm's value before clipping, exactly as mi_loudness_update reads it;
 * v = 0 outside [0, L).  bank_dev is a DEVICE array of (phases, taps) float32, h[p][k] (for Annex 2 the 4 x 12 polyphase table of
 * its 4-times oversampling filter).  For every phase p, channel c and position n in [0, L + taps - 1):
 *     acc = 0.0f;  for k = 0 .. taps-1 ascending:  acc = acc + h[p][k] * v[c][n - k]
 * every product and every sum a separately rounded float32 operation (no fused multiply-add).  Per output two uint32 bit patterns
 * of float32 are kept in peaks_dev (2 * n_peaks uint32): `over` = max |acc| over p, c, n at peaks_dev[2 * PEAK], and `sample` =
 * max |v| over c, j at peaks_dev[2 * PEAK + 1], each reduced over a workgroup and then by at most one atomicMax per workgroup, none
 * when the maximum is 0 or the slot already holds at least as much; a NaN leaves a NaN pattern, which orders above +inf.  The
 * caller zeroes a row's slots at the start of a track.
 * Both are pure functions of the values and max is order-free: the slots have the same bits for every partition of a track into
 * calls.  The oversampled estimate can lie below the sample peak (a tone at fs/4 sampled at its crests), so both are kept.
 * mi_true_peak_update: ONE launch takes the next N samples of every output of a track (or of a push), grid (ceil(max_n / 1024),
 *   n_rows); nothing synchronises with the host.  Row r of the table (MI_TP_COLS int64, a DEVICE array) is ONE output:
 *     SRC, N, ORIGIN, ORIGIN_PITCH, ORIGIN_AFFINE, AFFINE_ON, GAINS   as MI_MIX_*, at the same indices;
 *     SRC_PITCH, BEFORE   as MI_LOUD_*: floats between the (source, channel) rows of the stems, and the track position of frame 0;
 *     TAIL                positions past BEFORE + N that the call also evaluates, reading 0 there: 0 on a push, taps - 1 on the final
 *                         call of a track, after which every position of [0, L + taps - 1) has been evaluated once.  The call
 *                         evaluates the positions [BEFORE, BEFORE + N + TAIL);
 *     HIST_LEN, HIST_RD, HIST_WR, HIST_START, HIST_NEXT
 *                         the carried VALUES of this output, as MI_RATE_HIST_*: (channels, hist_len) floats at float offset
 *                         hist_rd of hist_dev hold positions [hist_start, before); the call (workgroup 0 of the row) writes positions
 *                         [hist_next, before + n) (at most hist_len), taken from the read side below BEFORE, at float offset
 *                         hist_wr, a side apart from the read one; hist_next < 0: nothing is written.  A stream carries from
 *                         max(0, before + n - (taps - 1)) on: taps - 1 values a channel.  hist_len == 0: no history, for a track
 *                         measured in one call (before == 0, hist_next < 0);
 *     PEAK                the row's slot in peaks_dev.
 *   max_n >= every row's N + TAIL (grid size).  Rows must not share history sides; rows that share a slot share its maximum.
 *   A row is skipped whole (nothing of it is read or written, its history and its slots included) under mi_loudness_update's rules
 *   -- SRC is 0 (with N > 0), a gain among g_mix, g_0 .. g_{n_sources-1} is not finite, all of them are 0, g_mix != 0 (with N > 0)
 *   without ORIGIN or with ORIGIN_PITCH < N, SRC_PITCH < N; BEFORE or HIST_START is negative, HIST_START > BEFORE, or before -
 *   hist_start > hist_len; a history side leaves hist_capacity (floats) or the sides overlap; HIST_NEXT >= 0 lies outside
 *   [hist_start, before + n] or before + n - hist_next > hist_len; N or BEFORE exceed 2^61 -- and when N < 0, or N == 0 with
 *   TAIL == 0 (N may be 0 when TAIL > 0: the final call of a stream, which reads only its history; SRC and ORIGIN are then not
 *   read); TAIL is outside [0, taps); PEAK is outside [0, n_peaks); HIST_START > 0 with fewer than taps - 1 values carried
 *   (before - hist_start < taps - 1: the chains of the first positions would miss values).
 *   1 <= phases <= MI_TP_MAX_PHASES and 1 <= taps <= MI_TP_MAX_TAPS are arguments, not constants of the build; the 4 x 12 bank
 *   runs an instance of the kernel with its window in registers, every other bank a generic loop with the same arithmetic. */
#define MI_TP_SRC 0
#define MI_TP_N 1
#define MI_TP_ORIGIN 2
#define MI_TP_ORIGIN_PITCH 3
#define MI_TP_ORIGIN_AFFINE 4
#define MI_TP_AFFINE_ON 5
#define MI_TP_GAINS 6
#define MI_TP_SRC_PITCH 11
#define MI_TP_BEFORE 12
#define MI_TP_TAIL 13
#define MI_TP_HIST_LEN 14
#define MI_TP_HIST_RD 15
#define MI_TP_HIST_WR 16
#define MI_TP_HIST_START 17
#define MI_TP_HIST_NEXT 18
#define MI_TP_PEAK 19
#define MI_TP_COLS 20
#define MI_TP_MAX_PHASES 8
#define MI_TP_MAX_TAPS 32
int mi_true_peak_update(const int64_t *table_dev, int32_t n_rows, int64_t max_n, int32_t n_sources, int32_t channels,
                        const float *bank_dev, int32_t phases, int32_t taps, float *hist_dev, int64_t hist_capacity, void *peaks_dev,
                        int32_t n_peaks, void *stream);

/* ---- kernel-level entry points (parity tests; same kernels the forward uses) --------------
 * mi_stft_cac: `_magnitude(_spec(mix))` (demucs/htdemucs.py:420-461, demucs/spec.py:11-27):
 *   mix_dev (B,2,L) -> cac_dev (B,4,2048,ceil(L/1024)), channel order [c0.re,c0.im,c1.re,c1.im]. */
int mi_stft_cac(const float *mix_dev, int32_t B, int32_t L, float *cac_dev, void *stream);
/* mi_istft_cac: `_ispec(_mask(z, x), length)` (demucs/htdemucs.py:442-471, demucs/spec.py:30-47):
 *   x_dev (B,S,4,2048,T) -> wav_dev (B,S,2,L) with T = ceil(L/1024). */
int mi_istft_cac(const float *x_dev, int32_t B, int32_t S, int32_t L, float *wav_dev, void *stream);

/* The same transforms with everything the forwards pass to them, and the per-item normalisation around them (norms.hip), for
 * kernel-level parity tests: the entries allocate their scratch, call the launchers the engine calls and wait for the stream
 * (synchronous).  Any L >= 1 (mi_stft_cac / mi_istft_cac too): below 2 560 samples pad1d's short-input rule (demucs/hdemucs.py:29-36)
 * zero-pads before it reflects.  T = ceil(L / 1024); 1 <= B (B S) <= 16383.
 *
 * mi_stft_norm: `_magnitude(_spec(mix))`, then `(x - mean) / (1e-5 + std)` over each item (demucs/htdemucs.py:545-548), as the
 *   forwards run it: frames + float64 statistics, finalisation (unbiased std), normalising transpose.
 *   mix_dev (B,2,L) -> x_dev (B,4,2048,x_pitch), columns T .. x_pitch - 1 untouched; x_pitch = 0 means T, otherwise >= T.
 *   norm_dev receives B pairs (mean, 1 / (1e-5 + std)), denorm_dev B pairs (mean, std). */
int mi_stft_norm(const float *mix_dev, int32_t B, int32_t L, float *x_dev, int32_t x_pitch, float *norm_dev, float *denorm_dev, void *stream);
/* mi_istft_full: `_ispec(_mask(z, y * std + mean), length)` + `xt * std_t + mean_t` (demucs/htdemucs.py:625-656):
 *   y_dev (B,S,4,2048,y_pitch) (0 = T, otherwise >= T), denorm_f_dev B pairs (mean, std) or NULL (no de-normalisation),
 *   xt_dev (B,S,2,xt_pitch) (0 = L, otherwise >= L) with denorm_t_dev B pairs (mean_t, std_t): both or neither;
 *   -> wav_dev (B,S,2,L). */
int mi_istft_full(const float *y_dev, int32_t B, int32_t S, int32_t L, int32_t y_pitch, const float *denorm_f_dev, const float *xt_dev,
                  int32_t xt_pitch, const float *denorm_t_dev, float *wav_dev, void *stream);
/* mi_item_norm: `(x - mean) / (1e-5 + std)` over each of `rows` contiguous rows of `count` >= 2 floats (the time branch's input,
 *   demucs/htdemucs.py:551-554; std unbiased): statistics, finalisation, apply.  x_dev -> y_dev (rows, count); norm_dev receives
 *   `rows` pairs (mean, 1 / (1e-5 + std)), denorm_dev (mean, std).  1 <= rows <= 65535.
 * mi_item_denorm: `x * std + mean` per row with denorm_dev = `rows` pairs (mean, std) (htdemucs.py:626,656); not synchronous. */
int mi_item_norm(const float *x_dev, int32_t rows, int64_t count, float *y_dev, float *norm_dev, float *denorm_dev, void *stream);
int mi_item_denorm(const float *x_dev, int32_t rows, int64_t count, const float *denorm_dev, float *y_dev, void *stream);

/* Generic convolution / linear layer evaluated by the implicit-GEMM MFMA kernel (stands in for
 *   F.conv1d / F.conv2d / F.conv_transpose / F.linear as invoked at demucs/hdemucs.py:110,116,
 *   136,153,287,294,313,326, demucs/demucs.py:138,140, demucs/htdemucs.py:589-599).
 *   See demucs_amd/csrc/gemm_conv.h (mi_conv_desc) for the field meanings.
 *   A float32 descriptor that states its kernel geometry (ntaps / tap_*) may run the shifted-run tap loader (routes 2 and 7), which
 *   reads up to 8 bytes before and 20 bytes after the tensor at `x`: the caller owns that slack (gemm_conv.h, beside `ntaps`).
 *   A float32 descriptor with a split image that sets `dma_time` (a 1-D time-axis strided or transposed conv) may run the time-axis
 *   loaders (route 11), which read the same 8 bytes before and 20 bytes after the tensor at `x` (gemm_conv.h, beside `dma_time`).
 *   Where the device allocation that holds `x` does not reach 128 bytes past both ends of the B * x_bstride floats at `x` (a tensor
 *   that begins or ends with its allocation: the read could touch an unmapped address), this entry runs the same kernel on a copy
 *   of `x` that has the slack, waits for the stream and frees the copy: same route, same bits (mi_debug_conv_staged counts these). */
struct mi_conv_desc;
int mi_conv_forward(const struct mi_conv_desc *desc, void *stream);

/* Re-packs fp32 weights Wt[Kpad][Mpad] (the mi_conv_desc.wt layout) into the split-bf16 tile image
 *   [Mpad/tile_m][Kpad/16][3 terms][2 k-halves][tile_m][8] bf16 (6 * Kpad * Mpad bytes) that mi_conv_desc.wx takes:
 *   each weight w = hi + mid + lo exactly, so the 6-product bf16 MFMA loop reproduces the fp32 product sum
 *   (no reference counterpart: it is the load-time half of how F.conv / F.linear run on the matrix cores).
 *   tile_m must be the tile the layer will run with (64, 96 or 128), or 192 for a layer with Mpad % 192 == 0 that sets
 *   mi_conv_desc.tile_m = 192: that writes the 96-row layout, which the 192-row tile reads two images at a time. */
int mi_conv_pack_split(const float *wt_dev, int32_t Kpad, int32_t Mpad, int32_t tile_m, void *wx_dev, void *stream);

/* mi_conv_pack_tap: weights of a k x k stride-1 conv for the operand-image route of the half modes (gemm_tap.hip): from the
 *   packed float32 Wt[Kpad][Mpad] with k = ci * ntaps + tap to the 16-bit image Wtap[pairs][Mpad][8], pair =
 *   (ci / 8) * ntaps + tap, pairs rounded up to a multiple of 4: 16 * pairs * Mpad bytes.  Cin %% 8 == 0. */
int mi_conv_pack_tap(const float *wt_dev, int32_t Mpad, int32_t Cin, int32_t ntaps, int32_t dtype, void *wtap_dev, void *stream);
/* mi_f32_to_image: float32 x (B, C, P) (channel stride P) -> the 16-bit operand image [C / 8][B * P][8] a matrix product reads by
 *   LDS-DMA (half modes; used where the producer of x cannot write the image itself: the DConv branch's output in front of a
 *   decoder's transposed conv).  C %% 8 == 0. */
int mi_f32_to_image(const float *x_dev, int32_t B, int32_t C, int64_t P, int32_t dtype, void *img_dev, void *stream);

/* Converts fp32 weights Wt[Kpad][Mpad] (the mi_conv_desc.wt layout) into the bf16 / fp16 operand image
 *   Wh[ceil(Kpad/32)*4][Mpad][8] (2 * round_up(Kpad, 32) * Mpad bytes) that mi_conv_desc.wh takes when mi_conv_desc.half
 *   = MI_DTYPE_BF16 / MI_DTYPE_F16 (the load-time half of the reduced-precision compute modes; no reference counterpart). */
int mi_conv_pack_half(const float *wt_dev, int32_t Kpad, int32_t Mpad, int32_t dtype, void *wh_dev, void *stream);

/* Multi-head attention core softmax(QK^T/sqrt(64))V on channel-first tensors (stands in for the
 *   attention inside nn.MultiheadAttention, called at demucs/transformer.py:418-419,506):
 *   q_dev (B, heads*64, Tq), k_dev / v_dev (B, heads*64, Tk), tokens contiguous, with the given batch strides; o_dev like
 *   q_dev.  dtype = MI_DTYPE_F32 (fp32 MFMA, parity mode) or MI_DTYPE_BF16 / MI_DTYPE_F16 (operands of both products
 *   rounded to that type, float32 softmax and accumulation). */
int mi_attention(const float *q_dev, const float *k_dev, const float *v_dev, float *o_dev, int32_t B, int32_t heads,
                 int32_t Tq, int32_t Tk, int64_t q_batch_stride, int64_t kv_batch_stride, int64_t o_batch_stride,
                 int32_t dtype, void *stream);

/* mi_attention_split: the float32 attention core of mi_attention (same arguments and layout, no dtype; stands in for the
 *   attention inside nn.MultiheadAttention, called at demucs/transformer.py:418-419,506) on the bf16 matrix pipe: Q / 8, K, V
 *   and the softmax probabilities are each carried as three exact bf16 terms, both products as six bf16 MFMA products
 *   accumulated in float32 (dropped terms <= 2^-24 |ab|); the softmax stays float32.  The float32 engine's default
 *   attention kernel (see mi_set_split_bf16).  Tk % 4 == 0; k_dev / v_dev 16-byte aligned, kv_batch_stride % 4 == 0. */
int mi_attention_split(const float *q_dev, const float *k_dev, const float *v_dev, float *o_dev, int32_t B, int32_t heads,
                       int32_t Tq, int32_t Tk, int64_t q_batch_stride, int64_t kv_batch_stride, int64_t o_batch_stride,
                       void *stream);

/* mi_attention_heads: the attention core of the half modes on the operands the projections really write in those modes:
 *   q / k / v_dev are 16-bit (bf16 / fp16 by `dtype`) per-head token-major tensors [B][heads][T pitch][64] (what the
 *   MI_FLAG_HEADS epilogue of the in-projection produces; K / V tiles reach LDS by DMA); o_dev float32 (B, heads * 64, Tq)
 *   = softmax(q k^T / 8) v per head (demucs/transformer.py:339-377,466-512). */
int mi_attention_heads(const void *q_dev, const void *k_dev, const void *v_dev, float *o_dev, int32_t B, int32_t heads, int32_t Tq, int32_t Tk,
                       int32_t Tq_pitch, int32_t Tk_pitch, int32_t dtype, void *stream);

/* mi_attention_heads with the result written as the 16-bit operand image of the projection that consumes it (out_proj): the only
 *   output form the half-mode engine uses.  img_dev[heads * 64 / 8][n_img][8] bf16 / fp16 (by `dtype`), column b * Tq + query,
 *   n_img >= B * Tq, 16-byte aligned; element [c / 8][b * Tq + query][c % 8] is channel c = head * 64 + d of mi_attention_heads'
 *   float32 result rounded to nearest even; columns past B * Tq are left untouched.  Feeds mi_conv_desc.xh. */
int mi_attention_heads_image(const void *q_dev, const void *k_dev, const void *v_dev, void *img_dev, int64_t n_img, int32_t B, int32_t heads,
                             int32_t Tq, int32_t Tk, int32_t Tq_pitch, int32_t Tk_pitch, int32_t dtype, void *stream);

/* mi_attention in a half mode with the result written as the 16-bit operand image of the projection that consumes it
 *   (out_proj, demucs/transformer.py:418-419 inside nn.MultiheadAttention): img_dev[(heads * 64) / 8][n_img][8] bf16 / fp16,
 *   column b * Tq + query, n_img >= B * Tq; element values are the float32 results of mi_attention rounded to nearest even.
 *   Feeds mi_conv_desc.xh (demucs_amd/csrc/gemm_conv.h). */
int mi_attention_image(const float *q_dev, const float *k_dev, const float *v_dev, void *img_dev, int64_t n_img, int32_t B,
                       int32_t heads, int32_t Tq, int32_t Tk, int64_t q_batch_stride, int64_t kv_batch_stride, int32_t dtype,
                       void *stream);

/* In-place GroupNorm(1, C) + GELU of the first C channels of x (B, C_alloc, D1, D2) given per-row (mean, rstd) float2 statistics
 *   (row = b*D1 + d1 if row_mode else b): the norm/activation pair inside DConv (demucs/demucs.py:139). */
int mi_gn_gelu(float *x_dev, int32_t B, int32_t C, int32_t C_alloc, int32_t D1, int32_t D2, int32_t row_mode, const float *stats_dev,
               const float *w_dev, const float *b_dev, void *stream);

/* The same GroupNorm(1, h) + GELU in place on the valid columns of x (B, C_alloc, D1, pitch >= D2) AND, in the same pass, the
 *   Gram sums of the normalised hidden activations g per statistics row: gram_dev (rows x slots x HP x HP float64, zero on
 *   entry, HP = mi_gram_order(h)) receives G[i][j] += g_i g_j for i, j <= h in the upper 32 x 32 block triangle, with
 *   g_h = 1 (so G[i][h] = sum g_i).  They give the statistics of the GroupNorm(1, 2C) that follows DConv's 1x1 conv
 *   z = W g + b (demucs/demucs.py:141-142) without evaluating it: mi_gram_finalize computes per row
 *   sum z^2 = <wt, G> + cols * sum_bsq and sum z = ct . G[:, h] + cols * sum_b, writes (mean, rstd) float2 and re-zeroes
 *   gram_dev.  wt_dev: HP x HP float64 (W^T W on diagonal blocks, 2 W^T W above them, 2 W^T b in column h); ct_dev: HP
 *   float64 column sums of W. */
int32_t mi_gram_order(int32_t h);
int mi_gn_gelu_gram(float *x_dev, int32_t B, int32_t h, int32_t C_alloc, int32_t D1, int32_t D2, int32_t pitch, int32_t row_mode,
                    const float *stats_dev, const float *w_dev, const float *b_dev, double *gram_dev, int32_t slots, void *stream);
/* mi_dconv_gn_gelu_gram: the form the engine's DConv runs -- mi_gn_gelu_gram, and in the same pass channels h..C_alloc-1 of the valid
 *   columns (the K padding of the 1x1 conv that follows) are set to zero, whatever they held: the engine shares one hidden buffer
 *   between layers of different item strides, so another layer or batch item may have left NaN there.  h <= C_alloc <=
 *   mi_gram_order(h). */
int mi_dconv_gn_gelu_gram(float *x_dev, int32_t B, int32_t h, int32_t C_alloc, int32_t D1, int32_t D2, int32_t pitch, int32_t row_mode,
                          const float *stats_dev, const float *w_dev, const float *b_dev, double *gram_dev, int32_t slots, void *stream);
int mi_gram_finalize(double *gram_dev, int32_t rows, int32_t h, int32_t slots, const double *wt_dev, const double *ct_dev, double sum_b,
                     double sum_bsq, double cols, double count, float eps, float *stats_out_dev, void *stream);

/* The recurrence of one bidirectional nn.LSTM layer as the BLSTM of demucs/demucs.py:20-67 runs it (zero initial state, gate order
 *   i, f, g, o): gx_dev (N, 2 directions, 4H, W) = W_ih x_t + b_ih + b_hh for every step (a GEMM done before), whh_host = the HOST
 *   array (2, 4H, H) of weight_hh_l{k} / weight_hh_l{k}_reverse; out_dev (N, 2H, W): forward hidden states in channels [0, H), backward
 *   ones in [H, 2H).  mode 0: one launch per time step; mode 1: the persistent kernel the engine uses (hidden state exchanged between
 *   workgroups as self-validating 4-byte values whose least significant mantissa bit carries a step tag, bounded waits); both for
 *   H = 192 or 384 (hdemucs_mmi's layers 4 / 5).  mode 2: the generic kernel the engine runs for every other hidden size (one
 *   workgroup per sequence and direction, W_hh in LDS in its natural order), 1 <= H <= 64.  Synchronous (test entry). */
int mi_lstm_seq(const float *gx_dev, const float *whh_host, int32_t N, int32_t H, int32_t W, float *out_dev, int32_t mode, void *stream);

/* LayerNorm over the channel axis of channel-first tokens x (B, C, T), optional additive table
 *   add_dev (C, T) (nn.LayerNorm at demucs/transformer.py:434-436,591-592 + positional
 *   embedding add :655-663). */
int mi_layernorm_cf(const float *x_dev, int32_t B, int32_t C, int32_t T, const float *w_dev, const float *b_dev,
                    const float *add_dev, float *y_dev, void *stream);

/* ---- Kernel-level test entries of the remaining hand-written kernels (hkernels.hip, norms.hip): each validates its arguments and
 * calls the launcher the engine calls, nothing else.  Asynchronous on `stream`. ---- */

/* The token kernel of the transformer (norms.hip token_tile_kernel) on channel-first tokens x (B, C, T), C % 4 == 0:
 *   mode 0  LayerNorm over channels (eps 1e-5) with affine w, b (C) plus the optional additive table pe (C, T) -> y (B, C, T)
 *   mode 1  statistics only: nothing but ostat (and img) is written; w, b, pe, gstat, y are ignored (y_dev may be NULL)
 *   mode 2  GroupNorm(1) apply y = (x - gstat[b].mean) * gstat[b].rstd * w[c] + b[c], gstat_dev = B (mean, rstd) float pairs
 * ostat_dev (B * T (mean, rstd) float pairs, NULL = not wanted in modes 0 / 2, required in mode 1): per token, mean over channels
 * and 1 / sqrt(biased variance + 1e-5) of y (modes 0, 2) or of x (mode 1) -- what the next GEMM's folded LayerNorm consumes.
 * img_dev (may be NULL): the same tensor (y, or x in mode 1) as a 16-bit operand image [C / 8][img_n][8], column b * T + t,
 * img_dtype MI_DTYPE_BF16 / MI_DTYPE_F16, round to nearest even; needs C % 32 == 0, img_n >= B * T and 16-byte alignment. */
int mi_token_norm(int32_t mode, const float *x_dev, int32_t B, int32_t C, int32_t T, const float *w_dev, const float *b_dev,
                  const float *pe_dev, const float *gstat_dev, float *y_dev, float *ostat_dev, void *img_dev, int64_t img_n,
                  int32_t img_dtype, void *stream);

/* LocalState attention core (demucs/demucs.py:182-216; hkernels.hip): qkc_dev (B, 3C + 16, ld) holds per item C query rows, C key
 *   rows, C content rows and 16 decay-logit rows (4 heads x 4), row pitch ld >= T, ld % 4 == 0, 16-byte aligned; out_dev (B, C, ld_o),
 *   ld_o >= T.  C = 192 / 384: the matrix-pipe kernels; any other C % 4 == 0 with C / 4 <= 16: the generic kernel.  Columns past T of
 *   either tensor are neither read nor written. */
int mi_local_attn(const float *qkc_dev, int32_t B, int32_t C, int32_t T, int32_t ld, float *out_dev, int32_t ld_o, void *stream);

/* GroupNorm(G, Cin) (eps 1e-5) of x (B, Cin, in_len) with contiguous rows (in_pitch == in_len) followed by the fused apply of the
 *   hdemucs_mmi layers, as HModel::group_norm runs it (row statistics, their finalisation, the apply kernel):
 *     y[b][co][p] = res[b][co][p] + scale[co'] * act(n(co, p + off) [* sigmoid(n(co + Cout, p + off)) if glu]),  0 <= p < out_len,
 *     n(c, q) = (x[b][c][q] - mean) * rstd * w[c'] + b[c'],  c' = c / chan_div,  act = erf-GELU if gelu,
 *   Cout = Cin / 2 with glu, Cin without; scale_dev / res_dev may be NULL; res rows have pitch res_pitch, y rows pitch out_pitch
 *   (columns past out_len are not written).  chan_div > 1: the Cin rows are (channel, row) pairs of a (Cin / chan_div, chan_div, len)
 *   tensor and w, b, scale hold Cin / chan_div values.
 *   stats_ws_dev: B * G * 64 doubles (32 slots of (sum, sum of squares) per statistics row), ZERO on entry and zero again on return
 *   (the finalisation cleans what it read); stats_out_dev: B * G (mean, rstd) float pairs, written. */
int mi_group_norm_apply(const float *x_dev, int32_t B, int32_t Cin, int32_t G, int32_t in_pitch, int32_t in_len, int32_t off,
                        const float *w_dev, const float *b_dev, int32_t glu, int32_t gelu, const float *scale_dev, const float *res_dev,
                        int32_t res_pitch, float *y_dev, int32_t Cout, int32_t out_len, int32_t out_pitch, int32_t chan_div,
                        double *stats_ws_dev, float *stats_out_dev, void *stream);

/* BLSTM framing (demucs/utils.py:20-35, demucs/demucs.py:38-44,51-64).  unfold: x (B, C, T) -> frames (B * F, C, W), frame f =
 *   columns [f * S, f * S + W) of x, zero past T.  restitch: frames (B * F, C, W) -> y (B, C, T) = skip (B, C, T, may be NULL) + the
 *   kept part of every frame (frame 0 columns [0, W - S / 2), the last one [S / 2, W), the others [S / 2, W - S / 2)) concatenated and
 *   cut to T; needs W > 2 (S / 2) and T <= W + (F - 1) (W - 2 (S / 2)). */
int mi_blstm_unfold(const float *x_dev, int32_t B, int32_t C, int32_t T, int32_t F, int32_t W, int32_t S, float *frames_dev, void *stream);
int mi_blstm_restitch(const float *frames_dev, int32_t B, int32_t C, int32_t T, int32_t F, int32_t W, int32_t S, const float *skip_dev,
                      float *y_dev, void *stream);

/* y (B, C, out_pitch)[.., i] = (x (B, C, L)[.., i] - norm[b].x) * norm[b].y for i < L and exactly 0 for L <= i < out_pitch;
 *   norm_dev = B (mean, 1 / (eps + std)) float pairs: the waveform branch's input normalisation into pitched rows. */
int mi_row_affine_pitch(const float *x_dev, int32_t B, int32_t C, int32_t L, int32_t out_pitch, const float *norm_dev, float *y_dev,
                        void *stream);

/* ---- Kernel-level test entries of the fused DConv kernels (dconv_row.hip, dconv_time.hip).  A DConv residual layer
 * (demucs/demucs.py:133-154) is conv1d(C -> C / 8, k = 3, dilation d, padding d) -> GroupNorm(1) -> GELU -> conv1d(C / 8 -> 2C, k = 1) ->
 * GroupNorm(1) -> GLU -> LayerScale -> + x.  `weights_host` is a HOST array holding, per layer, its nine tensors in the checkpoint's
 * natural layout, concatenated in this order (h = C / 8): 0.weight (h, C, 3), 0.bias (h), 1.weight (h), 1.bias (h), 3.weight (2C, h),
 * 3.bias (2C), 4.weight (2C), 4.bias (2C), 6.scale (C).  The entries pack them with the function Model uses, upload, call the launcher
 * the engine calls and wait for the stream (synchronous).  C = 48 or 96. ---- */

/* Both layers (d = 1, then d = 2) of the frequency branch on every (b, fr) row of x (B, C, Fr, T): weights_host = layer 0 then layer 1.
 *   T a multiple of 6, at most 384; x and y 8-byte aligned; y_dev may be x_dev itself (as the engine runs it) or must not overlap it.
 *   variant 0: one wave per row (the default kernel); variant 1: the LDS-resident kernel (MI_DCONV_ROW=lds), C = 48 only -- what
 *   it does not take is refused, not rerouted. */
int mi_dconv_row(const float *x_dev, float *y_dev, int32_t B, int32_t C, int32_t Fr, int32_t T, const float *weights_host, int32_t variant,
                 void *stream);

/* One layer of dilation dil (1 or 2) of the time branch on x (B, C, Lp): Lv valid columns per row of pitch Lp (Lp even, Lp >= Lv >= 1),
 *   1 <= B <= 65535; y (B, C, Lp) must not overlap x.  Columns Lv .. Lp - 1 of x are never used; those of y are unspecified.
 *   The caller owns the workspace, all of it 8-byte aligned:
 *     hbuf_dev   B * HA * Lp floats (HA = C / 8 rounded up to 4): the hidden tensor, any contents on entry;
 *     stats_dev  B * 32 * 2 doubles and gram_dev B * 32 * 96 doubles: ZERO on entry and zero again on return;
 *     st_dev     2 * B (mean, rstd) float pairs, written: [0, B) the first GroupNorm's statistics, [B, 2B) the second's. */
int mi_dconv_time_layer(const float *x_dev, float *y_dev, int32_t B, int32_t C, int32_t Lv, int32_t Lp, int32_t dil,
                        const float *weights_host, float *hbuf_dev, double *stats_dev, double *gram_dev, float *st_dev, void *stream);

/* Debug aid: `hook(stream)` is called after every kernel launch the library makes (NULL switches it off).  Used by
 * tools/micro/poison_all.py to interleave a register / LDS poisoning kernel between the engine's kernels. */
void mi_debug_set_post_launch_hook(void (*hook)(void *stream));

/* The main loops a conv / linear layer can run on ("routes"): chosen from the descriptor alone, so a test that compares two
 * routes bit for bit also has to see that they WERE two routes. */
enum mi_conv_route {
    MI_ROUTE_TABLE = 0,    /* table-driven gather / register-staged loader (conv_gemm_kernel) */
    MI_ROUTE_DMA = 1,      /* LDS-DMA plain linear tile (conv_gemm_dma_kernel) */
    MI_ROUTE_DMATAP = 2,   /* LDS-DMA shifted-run taps (conv_gemm_dmatap_kernel) */
    MI_ROUTE_DMAROW = 3,   /* LDS-DMA row taps (conv_gemm_dmarow_kernel) */
    MI_ROUTE_X6 = 4,       /* split-bf16 (gemm_x6.hip conv_gemm_x6_kernel) */
    MI_ROUTE_HALF = 5,     /* half modes, register-staged loader (gemm_half.hip conv_gemm_half_kernel); tile 32 / 64 / 96 / 128, or 256 for
                              a plain LINEAR layer of 128-row tiles with Mpad % 256 == 0 (MI_HALF_TILE256=0: 128) */
    MI_ROUTE_TAP_HALF = 6, /* half-mode tap images (gemm_tap.hip) */
    MI_ROUTE_TAP_X6 = 7,   /* split-bf16 with LDS-DMA shifted-run taps (gemm_x6.hip conv_tap_x6_kernel: stride-1 3 x 3 / k = 3 GLU
                              convs with a split image and the geometry of route 2) */
    MI_ROUTE_ROWS_X6 = 8,  /* split-bf16 with LDS-DMA row taps (gemm_x6.hip conv_rows_x6_kernel: the row-tap layers of route 3 --
                              LINEAR + GELU or CONVTR on 96- / 128-row tiles, 1 x 1 + GLU on 128-row tiles -- with a split image) */
    MI_ROUTE_HALF_IMG = 9, /* half modes, operand-image input, 3-stage LDS-DMA ring (gemm_half.hip conv_gemm_half_img_kernel: plain
                              LINEAR with SCALE|RES or SCALE|RES|STATS); tile 256 where Mpad % 256 == 0, else 128 */
    MI_ROUTE_HALF_IMG256 = 10, /* half modes, operand-image input, 512-thread 256 x 256 tile (gemm_half.hip conv_gemm_half_img256_kernel:
                              plain LINEAR with LN|HEADS or LN|GELU|IMG; with SCALE|RES under MI_IMG256=1 where Mpad % 256 == 0); tile 256 */
    MI_ROUTE_TIME_X6 = 11  /* split-bf16 with LDS-DMA shifted-run taps along the time axis (gemm_x6.hip conv_time_tr_x6_kernel,
                              conv_time_enc_x6_kernel: the time branch's transposed convs as two-tap GEMMs and its strided convs k = 8,
                              s = 4 + GELU, `dma_time`, with a split image; 96- / 128-row tiles).  These loaders read up to 8 bytes
                              before and 20 bytes after the tensor at x: the caller owns that slack (gemm_conv.h `dma_time`) */
};

/* Debug aid for the kernel tests: the route the LAST mi_conv_forward of this process took; -1 before any call.  Process-wide,
 * not thread-safe. */
int mi_debug_last_conv_route(void);

/* Debug aid, as mi_debug_last_conv_route: the rows of the tile the LAST mi_conv_forward of this process ran (what
 * mi_debug_conv_route answers in *tile); -1 before any call. */
int mi_debug_last_conv_tile(void);

/* Debug aid: how many calls of mi_conv_forward in this process ran on a copy of `x` with read slack, because the caller's
 * allocation did not reach 128 bytes past both ends of the tensor (see mi_conv_forward).  Process-wide, not thread-safe. */
int mi_debug_conv_staged(void);

/* Debug aid: how many layers this process has launched on `route` (enum mi_conv_route) with epilogue `epi` (enum mi_epilogue of
 * gemm_conv.h; -1: any), through mi_conv_forward and through the engines' forwards alike; -1 for a route or epilogue out of
 * range.  A test takes the difference around a forward.  Process-wide, not thread-safe. */
int64_t mi_debug_conv_route_launches(int32_t route, int32_t epi);

/* Debug aid: the route mi_conv_forward WOULD take for `desc` (under the environment switches and mi_set_split_bf16 as they
 * stand) and, in *tile (may be NULL), the rows of the tile that kernel runs, after every substitution: for the
 * split-bf16 routes 64 under a 128-row layer means the 64-row tile that reads the 128-row image, and a tile_m = 192 layer
 * answers 192 (the 192-row tile on pairs of its 96-row images) or, under-filled, 96.  Host code only: launches nothing, follows
 * no pointer of the descriptor, works in a process that never touches the GPU.  Returns -1 for desc == NULL and for a
 * descriptor whose tile_m is 192 while its M is no multiple of 192 or is padded (mi_last_error names it). */
int mi_debug_conv_route(const struct mi_conv_desc *desc, int *tile);

/* Debug aid: the MI_* environment switches as this process parsed them, when the library was loaded (INTEGRATION.md has the
 * table): one `NAME=value` line per switch, the value being the parsed meaning, not the string -- 0 / 1 for an on / off switch,
 * `MI_X6` none | default | all, `MI_SIDE_PRIO` low | normal | high, `MI_DCONV_ROW` wave | lds, `MI_TRANSPOSE_TILES` the mask.
 * Writes at most n - 1 characters and a terminating NUL into buf (nothing when buf is NULL or n <= 0); returns the length of
 * the whole text, as snprintf does.  Host code only. */
int mi_debug_switches(char *buf, int32_t n);

const char *mi_last_error(void);
/* "demucs_amd <version> gfx950" */
const char *mi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* DEMUCS_AMD_H */
