"""The analysis pass of a stream on the MI355X: `audio.MonoStatsStream`, `Separator.analyse_stream`, the `stats=` keyword of the
streams and `Separator.separate_blocks`.  The statistics are `mi_mono_stats`' bit for bit for every partition of the input, so a
file read twice -- once to analyse, once to separate -- gives `separate_tensor`'s stems exactly (`torch.equal` per stem, `random`
in the same state) without the track ever lying whole on the host or the device."""
import ctypes as C
import functools
import random

import numpy as np
import pytest
import torch

from demucs_amd import _lib, audio
from demucs_amd.api import Delivery, Separator
from demucs_amd.audio import MonoStatsStream, PcmFeed, TrackStats
from test_gpu_ingest import byte_chunks, run_stream, to_i16
from test_gpu_stream import hd, ht, track

pytestmark = pytest.mark.gpu
SR = 44100


def one_shot(wav):
    """(mean, s) of `mi_mono_stats` on the whole (channels, length) track, as float32 scalars."""
    lib = _lib.load()
    dev = wav.cuda().contiguous()
    scratch = torch.empty(lib.mi_mono_stats_scratch_bytes(), dtype=torch.uint8, device="cuda")
    stats = torch.empty(2, dtype=torch.float32, device="cuda")
    _lib.check(lib.mi_mono_stats(dev.data_ptr(), dev.shape[0], dev.shape[1], scratch.data_ptr(), stats.data_ptr(),
                                 C.c_void_p(_lib.current_stream_ptr())), "mi_mono_stats")
    return tuple(np.float32(v) for v in stats.cpu().tolist())


def same_bits(stats: TrackStats, want) -> bool:
    got = np.array([stats.mean, stats.s], np.float32)
    return np.array_equal(got.view(np.uint32), np.array(want, np.float32).view(np.uint32))


def chunks(data: bytes, size: int):
    return [data[i:i + size] for i in range(0, len(data), size)]


@functools.lru_cache(maxsize=None)
def small_model():
    return hd("f32", max_batch=2, channels=4, segment=2)


# ---- 1. MonoStatsStream ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size,frames", [(1, 1500), (5, 5000), (4097, 300001)])
def test_byte_chunks_that_end_inside_a_frame(size, frames):
    """Stereo int16 in chunks of 1, 5 and 4097 bytes: none is a multiple of the 4-byte frame."""
    q, floats = to_i16(track(frames, seed=20 + size) * 0.7)
    data = q.numpy().tobytes() + b"\x7f\x01\x02"             # an incomplete last frame: dropped
    st = MonoStatsStream(2, pcm="i16", src_channels=2)
    tails = set()
    for c in chunks(data, size):
        st.push(c)
        tails.add(st.trailing_bytes)
    assert st.pushed == frames and st.trailing_bytes == 3 and tails == {0, 1, 2, 3}
    assert st.device_bytes() == 2 * 262144 * 8
    stats = st.finish()
    assert st.trailing_bytes == 3
    assert (stats.length, stats.input_length) == (frames, frames)
    decoded = audio.pcm_to_tensor(q.numpy().tobytes(), "i16", 2)
    assert torch.equal(decoded.cpu(), floats)
    assert same_bits(stats, one_shot(decoded)), (stats, one_shot(decoded))
    with pytest.raises(RuntimeError, match="push after finish"):
        st.push(b"\x00" * 8)


def test_every_kind_of_block_counts_the_same():
    """Planar float blocks on the host and the device, typed (n, 2) tensors, 1-D uint8 tensors and `PcmBlock`s in one stream."""
    L = 262144 + 3001
    q, floats = to_i16(track(L, seed=31) * 0.6)
    want = one_shot(floats)
    st = MonoStatsStream(2)
    for blk in (floats[:, :1000], floats[:, 1000:1000], floats[:, 1000:200001].cuda(), floats[:, 200001:]):
        st.push(blk)
    assert st.pushed == L and same_bits(st.finish(), want)
    cuts = [0, 999, 100000, 262145, L - 7, L]
    blocks = [q[a:b] for a, b in zip(cuts[:-1], cuts[1:])]
    st = MonoStatsStream(2, pcm="i16", src_channels=2)
    feed = PcmFeed("i16", 2)
    st.push(blocks[0])                                        # (n, 2) int16 on the host
    st.push(blocks[1].cuda())                                 # ... on the device
    st.push(blocks[2].cuda().view(torch.uint8).reshape(-1))   # 1-D uint8 on the device
    st.push(blocks[3].numpy().tobytes())                      # bytes
    st.push(feed.accept(memoryview(blocks[4].numpy().tobytes())))      # a PcmBlock of a caller's own feed
    assert st.pushed == L and same_bits(st.finish(), want)
    state = torch.cuda.memory_allocated()
    del st
    assert torch.cuda.memory_allocated() < state              # the 4 MiB of sums go with the stream


# ---- 2. Separator.analyse_stream ----------------------------------------------------------------------------------------------------
def test_converting_analysis_equals_the_statistics_of_convert_audio():
    sr = 48000
    L = 3 * sr + 321
    q, floats = to_i16(track(L, seed=43)[:1] * 0.7)           # mono, 48 kHz
    sep = Separator(small_model(), device="cuda", shifts=1)
    state = random.getstate()
    an = sep.analyse_stream(sr=sr, convert=True, pcm="i16", channels=1)
    for c in byte_chunks(q.numpy().tobytes() + b"\x01", seed=3, typical=sr):
        an.push(c)
    assert an.pushed == L and an.trailing_bytes == 1
    stats = an.finish()
    assert random.getstate() == state                         # the analysis draws nothing
    converted = audio.convert_audio(floats.cuda(), sr, SR, 2)
    assert stats.input_length == L and stats.length == converted.shape[1] == 147 * L // 160
    assert same_bits(stats, one_shot(converted)), (stats, one_shot(converted))
    assert an.device_bytes() < 5 << 20
    with pytest.raises(RuntimeError, match="push after finish"):
        an.push(b"")
    # the same input as planar float blocks
    an = sep.analyse_stream(sr=sr, convert=True, channels=1)
    for i in range(0, L, 30011):
        an.push(floats[:, i:i + 30011])
    assert an.finish() == stats


# ---- 3. end to end: analyse, then separate -------------------------------------------------------------------------------------------
def analysed_stems(sep, blocks, seed, **kw):
    """Pass 1 and pass 2 over `blocks`: (stats, {source: stems}, the state of `random` afterwards)."""
    an = sep.analyse_stream(**kw)
    for b in blocks:
        an.push(b)
    stats = an.finish()
    random.seed(seed)
    ss = sep.separate_stream(stats=stats, **kw)
    got = run_stream(ss, blocks)
    return stats, got, random.getstate()


def offline(sep, wav, seed, sr=None):
    random.seed(seed)
    _, want = sep.separate_tensor(wav.clone(), sr)
    return want, random.getstate()


def test_float_blocks_equal_separate_tensor():
    L = 7 * SR + 3
    wav = track(L, seed=12) * 0.3
    sep = Separator(small_model(), device="cuda", shifts=1)
    want, state = offline(sep, wav, 3)
    stats, got, after = analysed_stems(sep, [wav[:, i:i + SR] for i in range(0, L, SR)], 3)
    assert after == state and stats.length == L
    for k in want:
        assert torch.equal(got[k], want[k]), k


def test_converting_i16_feed_equals_separate_tensor():
    sr = 48000
    L = 7 * sr + 3
    q, floats = to_i16(track(L, seed=44)[:1] * 0.7)           # mono, 48 kHz
    sep = Separator(small_model(), device="cuda", shifts=1)
    want, state = offline(sep, floats, 5, sr=sr)
    blocks = byte_chunks(q.numpy().tobytes(), seed=1, typical=2 * sr)
    stats, got, after = analysed_stems(sep, blocks, 5, sr=sr, channels=1, convert=True, pcm="i16")
    assert after == state and stats.input_length == L
    for k in want:
        assert got[k].shape == (2, stats.length) and torch.equal(got[k], want[k]), k


def test_htdemucs_stream_with_analysed_stats_equals_separate_tensor():
    L = 9 * SR + 17
    wav = track(L, seed=13) * 0.3
    sep = Separator(ht("f32"), device="cuda", shifts=1)
    want, state = offline(sep, wav, 3)
    stats, got, after = analysed_stems(sep, [wav[:, i:i + 3 * SR] for i in range(0, L, 3 * SR)], 3)
    assert after == state
    for k in want:
        assert torch.equal(got[k], want[k]), k


def test_a_group_stream_opened_with_stats_returns_what_the_solo_stream_returns():
    L = 5 * SR + 11
    wav = track(L, seed=14) * 0.4
    blocks = [wav[:, i:i + SR] for i in range(0, L, SR)]
    sep = Separator(small_model(), device="cuda", shifts=1)
    an = sep.analyse_stream()
    for b in blocks:
        an.push(b)
    stats = an.finish()
    random.seed(9)
    ss = sep.separate_stream(stats=stats)
    solo = [ss.push(b) for b in blocks] + [ss.finish()]
    state = random.getstate()
    random.seed(9)
    g = sep.separate_stream_group()
    key = g.open(stats=stats)
    grouped = [g.push({key: b})[key] for b in blocks] + [g.finish([key])[key]]
    assert random.getstate() == state
    for a, b in zip(solo, grouped):
        for k in a:
            assert a[k].shape == b[k].shape and torch.equal(a[k], b[k]), k


# ---- 4. separate_blocks -----------------------------------------------------------------------------------------------------------------
def test_separate_blocks_equals_separate_tensor_and_deliver():
    L = 6 * SR + 5
    wav = track(L, seed=15) * 0.9
    sep = Separator(small_model(), device="cuda", shifts=1)
    want, state = offline(sep, wav, 21)
    reads = []

    def source():
        reads.append(0)
        for i in range(0, L, SR + 7):
            yield wav[:, i:i + SR + 7]

    random.seed(21)
    outs = list(sep.separate_blocks(source))
    assert random.getstate() == state and len(reads) == 2     # the file is read twice
    assert len(outs) == -(-L // (SR + 7)) + 1
    for k in want:
        assert torch.equal(torch.cat([o[k] for o in outs], -1), want[k]), k
    frames = audio.deliver(wav, want, stem="vocals", clip="clamp")
    random.seed(21)
    outs = list(sep.separate_blocks(source, deliver=Delivery("vocals", clip="clamp")))
    assert random.getstate() == state
    assert list(outs[0]) == list(frames) == ["vocals", "no_vocals"]
    for k in frames:
        got = torch.cat([o[k] for o in outs], 0)
        assert got.dtype == torch.int16 and got.shape == (L, 2) and torch.equal(got, frames[k]), k
    assert frames["vocals"].abs().max() > 0                   # not silence: the comparison means something
