"""Host logic of the wire-PCM input of the streams (`demucs_amd.audio.PcmFeed`, `wav_info`, the `pcm=` keyword) without a GPU:
the frame carry over byte chunks that end anywhere, `wav_info` as the inverse of `wav_header`, and every refusal before any RNG
call or device work."""
import random
import struct

import numpy as np
import pytest
import torch

from demucs_amd import _lib, audio
from demucs_amd.api import Separator
from demucs_amd.apply import apply_model_stream
from demucs_amd.audio import PCM_FORMATS, PcmFeed, wav_header, wav_info
from demucs_amd.stream import StreamGroup
from test_apply_host import ToyModel
from test_stream_host import Refusing

CASES = [("i16", 2), ("i16", 1), ("i24", 2), ("i24", 3), ("i24", 1), ("f32", 2), ("f32", 3)]


def payload(nbytes, seed):
    return np.random.default_rng(seed).integers(0, 256, nbytes, dtype=np.uint8).tobytes()


def fed(fmt, ch, chunks):
    """The frames a feed hands over for `chunks` (bytes of whole frames, per push), the largest carry, and the feed."""
    feed = PcmFeed(fmt, ch)
    frames, worst, total = [], 0, 0
    for c in chunks:
        blk = feed.accept(c)
        assert feed.trailing_bytes == total % feed.frame_bytes          # accept changes nothing
        feed.commit(blk)
        total += len(c)
        got = b"".join(bytes(p) for p in blk.pieces)
        assert len(got) == blk.nbytes == blk.n * feed.frame_bytes and blk.shape == (ch, blk.n)
        assert blk.device.type == "cpu" and feed.trailing_bytes == total % feed.frame_bytes
        staged = np.zeros(blk.nbytes, dtype=np.uint8)
        blk.stage(staged)
        assert staged.tobytes() == got
        frames.append(got)
        worst = max(worst, feed.trailing_bytes)
    return b"".join(frames), worst, feed


def cut(data, points):
    points = [0] + sorted(points) + [len(data)]
    return [data[a:b] for a, b in zip(points, points[1:])]


@pytest.mark.parametrize("fmt,ch", CASES)
def test_frame_carry_gives_the_frames_of_one_push(fmt, ch):
    frame = ch * PCM_FORMATS[fmt][1]
    for n_frames, extra in [(0, 0), (1, 0), (37, 0), (37, 1), (37, frame - 1), (0, frame - 1)]:
        data = payload(n_frames * frame + extra, seed=n_frames + extra)
        whole = data[:n_frames * frame]
        one, _, feed = fed(fmt, ch, [data])
        assert one == whole and feed.trailing_bytes == extra
        # a byte at a time: every cut inside a sample and inside a frame
        got, worst, feed = fed(fmt, ch, [data[i:i + 1] for i in range(len(data))])
        assert got == whole and feed.trailing_bytes == extra
        assert worst == min(frame - 1, len(data))
        # random cut points, with empty chunks among them
        rng = random.Random(n_frames * 7 + extra)
        for trial in range(6):
            points = [rng.randint(0, len(data)) for _ in range(rng.randint(0, 12))]
            points += points[:2]                                        # equal cut points: empty chunks
            chunks = cut(data, points)
            assert trial == 0 or b"" in chunks or len(points) == 0
            got, worst, feed = fed(fmt, ch, chunks)
            assert got == whole and worst <= frame - 1 and feed.trailing_bytes == extra


def test_cuts_inside_an_i24_sample():
    data = payload(8 * 6 + 4, seed=3)                      # 8 stereo frames and 4 bytes: one sample and a third of the next
    for a in range(1, 3):                                   # the first chunk ends after a bytes of sample 0 of some frame
        chunks = cut(data, [6 * 2 + a, 6 * 5 + 3 + a])
        got, worst, feed = fed("i24", 2, chunks)
        assert got == data[:48] and feed.trailing_bytes == 4 and worst <= 5
    feed = PcmFeed("i24", 2)
    assert feed.accept(data[:5]).n == 0 and feed.accept(data[:6]).n == 1


def test_block_types():
    feed = PcmFeed("i16", 2)
    data = payload(40, 1)
    want = feed.accept(data)
    for block in (bytearray(data), memoryview(data), torch.frombuffer(bytearray(data), dtype=torch.uint8),
                  torch.frombuffer(bytearray(data), dtype=torch.int16).view(10, 2)):
        blk = feed.accept(block)
        assert blk.n == want.n == 10 and b"".join(bytes(p) for p in blk.pieces) == data
    f32 = PcmFeed("f32", 3)
    x = torch.arange(12, dtype=torch.float32).view(4, 3)
    assert b"".join(bytes(p) for p in f32.accept(x).pieces) == x.numpy().tobytes()
    assert f32.accept(x.t().contiguous().t()).n == 4       # a strided (n, channels) tensor is made contiguous
    for bad in (torch.zeros(2, 10), torch.zeros(10, 2, dtype=torch.int32), torch.zeros(10, 3, dtype=torch.int16), 5, None, [1, 2],
                torch.zeros(10, dtype=torch.int16)):
        with pytest.raises(ValueError, match="expected a block of 'i16' PCM"):
            feed.accept(bad)
    with pytest.raises(ValueError, match="i24"):
        PcmFeed("i24", 2).accept(torch.zeros(10, 2, dtype=torch.int32))
    with pytest.raises(ValueError, match="Invalid PCM format"):
        PcmFeed("i32", 2)
    with pytest.raises(ValueError, match="at least one"):
        PcmFeed("i16", 0)


# ---- wav_info ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["i16", "f32"])
@pytest.mark.parametrize("frames", [0, 12345, None])
@pytest.mark.parametrize("channels,rate", [(2, 44100), (1, 48000), (6, 96000)])
def test_wav_info_inverts_wav_header(fmt, frames, channels, rate):
    head = wav_header(frames, rate, channels, fmt)
    assert wav_info(head) == (fmt, channels, rate, frames, len(head))
    assert wav_info(head + b"\x01\x02\x03") == (fmt, channels, rate, frames, len(head))
    for k in range(len(head)):
        assert wav_info(head[:k]) is None, k
    assert wav_info(bytearray(head)) == wav_info(memoryview(head)) == wav_info(head)


def chunk(tag, body):
    return tag + struct.pack("<I", len(body)) + body + (b"\x00" if len(body) & 1 else b"")


def riff(*chunks, form=b"WAVE", magic=b"RIFF"):
    body = form + b"".join(chunks)
    return magic + struct.pack("<I", len(body)) + body


def fmt_chunk(tag, channels, rate, bits, extensible=None):
    align = channels * bits // 8
    body = struct.pack("<HHIIHH", 0xFFFE if extensible is not None else tag, channels, rate, rate * align, align, bits)
    if extensible is not None:
        body += struct.pack("<HHI", 22, bits, 3) + struct.pack("<H", tag) + extensible
    return chunk(b"fmt ", body)


GUID_TAIL = bytes.fromhex("000000001000800000aa00389b71")


def test_wav_info_hand_built_headers():
    data = b"data" + struct.pack("<I", 6 * 100)
    # 24-bit stereo with a LIST chunk of odd size (padded) and a chunk nobody knows before data
    head = riff(fmt_chunk(1, 2, 48000, 24), chunk(b"LIST", b"INFOabc"), chunk(b"junk", b"\x00" * 10)) + data
    assert wav_info(head) == ("i24", 2, 48000, 100, len(head))
    for k in range(len(head)):
        assert wav_info(head[:k]) is None, k
    # WAVE_FORMAT_EXTENSIBLE: PCM 16 and 24 bits, IEEE float
    for tag, bits, name in [(1, 16, "i16"), (1, 24, "i24"), (3, 32, "f32")]:
        head = riff(fmt_chunk(tag, 3, 44100, bits, GUID_TAIL), chunk(b"fact", struct.pack("<I", 7))) + b"data" + struct.pack("<I", 3 * bits // 8 * 7)
        assert wav_info(head) == (name, 3, 44100, 7, len(head))
        for k in range(len(head)):
            assert wav_info(head[:k]) is None, k
    # a fmt chunk longer than 16 bytes (cbSize = 0), the unknown-length sizes
    head = riff(chunk(b"fmt ", struct.pack("<HHIIHHH", 1, 1, 8000, 16000, 2, 16, 0))) + b"data" + struct.pack("<I", 0xFFFFFFFF)
    assert wav_info(head) == ("i16", 1, 8000, None, len(head))


@pytest.mark.parametrize("head", [
    riff(fmt_chunk(1, 2, 44100, 16), magic=b"RIFX") + b"data\x00\x00\x00\x00",
    riff(fmt_chunk(1, 2, 44100, 16), form=b"AVI ") + b"data\x00\x00\x00\x00",
    riff(fmt_chunk(1, 2, 44100, 8)) + b"data\x00\x00\x00\x00",                       # 8-bit
    riff(fmt_chunk(1, 2, 44100, 32)) + b"data\x00\x00\x00\x00",                      # int32
    riff(fmt_chunk(3, 2, 44100, 64)) + b"data\x00\x00\x00\x00",                      # float64
    riff(fmt_chunk(3, 2, 44100, 16)) + b"data\x00\x00\x00\x00",                      # half floats
    riff(fmt_chunk(2, 2, 44100, 4)) + b"data\x00\x00\x00\x00",                       # ADPCM
    riff(fmt_chunk(6, 1, 8000, 8)) + b"data\x00\x00\x00\x00",                        # A-law
    riff(fmt_chunk(1, 2, 44100, 16, bytes(14))) + b"data\x00\x00\x00\x00",           # extensible, another sub-format
    riff(fmt_chunk(2, 2, 44100, 16, GUID_TAIL)) + b"data\x00\x00\x00\x00",           # extensible ADPCM
    riff(chunk(b"fmt ", struct.pack("<HHIIHH", 1, 2, 44100, 176400, 3, 16))) + b"data\x00\x00\x00\x00",   # wrong block align
    riff(chunk(b"fmt ", struct.pack("<HHIIHH", 1, 0, 44100, 0, 0, 16))) + b"data\x00\x00\x00\x00",        # no channels
    riff(chunk(b"fmt ", b"\x01\x00\x02\x00")) + b"data\x00\x00\x00\x00",             # a fmt chunk too short
    riff() + b"data\x00\x00\x00\x00",                                                  # data before fmt
])
def test_wav_info_refusals(head):
    with pytest.raises(ValueError, match="wav_info"):
        wav_info(head)


def test_wav_info_refuses_as_soon_as_the_magic_is_wrong():
    with pytest.raises(ValueError, match="RIFF"):
        wav_info(b"RIFX")
    with pytest.raises(ValueError, match="RIFF"):
        wav_info(b"ID3")
    with pytest.raises(ValueError, match="WAVE"):
        wav_info(b"RIFF\x00\x00\x00\x00AIFF")
    assert wav_info(b"") is None and wav_info(b"RIF") is None and wav_info(b"RIFF\x00\x00\x00\x00WAV") is None


# ---- refusals: before any RNG call or device work -----------------------------------------------------------------------------------
def test_pcm_refusals_draw_nothing():
    state = random.getstate()
    sep = Separator(Refusing(), device="cpu", shifts=1)
    g = sep.separate_stream_group()
    calls = [
        lambda: sep.separate_stream(0.0, 1.0, pcm="i16"),                               # not an engine, not a GPU
        lambda: sep.separate_stream(0.0, 1.0, pcm="i16", sr=48000, channels=1, convert=True),
        lambda: sep.separate_stream(pcm="i24", length=100),
        lambda: sep.separate_stream(pcm="s16"),
        lambda: g.open(0.0, 1.0, pcm="f32"),
        lambda: g.open(pcm="u8"),
        lambda: apply_model_stream(ToyModel(), shifts=1, pcm="i16"),
        lambda: apply_model_stream(ToyModel(), shifts=1, pcm="i16", device="cpu", length=10),
        lambda: apply_model_stream(ToyModel(), shifts=1, pcm="wav"),
        lambda: apply_model_stream(ToyModel(), shifts=1, channels=1),                   # float blocks convert no channel layout
        lambda: StreamGroup(ToyModel(), shifts=1).open(pcm="i16"),
        lambda: StreamGroup(ToyModel(), shifts=1).open(channels=1),
        lambda: audio.ConvertStream(48000, 44100, 2, device="cuda", pcm="i16"),         # no source channel count
        lambda: audio.ConvertStream(48000, 44100, 2, device="cuda", pcm="i16", src_channels=0),
        lambda: audio.ConvertStream(48000, 44100, 4, device="cuda", pcm="i16", src_channels=3),
        lambda: audio.ConvertStream(48000, 44100, 1, device="cuda", pcm="f32", src_channels=2),
        lambda: audio.ConvertStream(48000, 44100, 2, device="cuda", pcm="i8", src_channels=2),
    ]
    for k, call in enumerate(calls):
        with pytest.raises(ValueError):
            call()
        assert random.getstate() == state, k
    assert g.open_keys == []
    with pytest.raises(ValueError, match="GPU engines"):
        sep.separate_stream(pcm="i16")
    with pytest.raises(ValueError, match="Invalid PCM format"):
        sep.separate_stream(pcm="s16")
    with pytest.raises(_lib.EngineError):
        audio.pcm_to_tensor(b"\x00\x00", "i16", 1, device="cpu")


def test_converting_pcm_stream_is_host_state_only_until_the_first_push():
    cs = audio.convert_audio_stream(48000, 44100, 2, pcm="i24", src_channels=1)
    assert cs.src_channels == 1 and cs.trailing_bytes == 0 and cs.device_bytes() == 0 and cs.pushed == 0
