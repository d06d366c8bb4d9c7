"""Wire PCM into the streams on the MI355X (`mi_pcm_planar`, `mi_streams_append_pcm`, `mi_streams_convert_append_pcm`, the `pcm=`
keyword): interleaved int16 / int24 / float32 frames give, bit for bit, what the float path gives for the same values -- the kernels
alone against numpy and against the float entries, then the streams end to end with byte chunks cut anywhere.  The conversion is
exact, so every comparison is of bit patterns."""
import ctypes as C
import gc
import random
from collections import Counter

import numpy as np
import pytest
import torch

from demucs_amd import _lib, audio
from demucs_amd.api import Delivery, Separator
from demucs_amd.audio import APPEND_PCM_COLS, CVT_COLS, CVT_PCM_COLS, PCM_FORMATS, PCM_PLANAR, ConvertPlan
from demucs_amd.stream import APPEND_COLS, ModelStream
from test_gpu_convert_stream import PAIRS
from test_gpu_stream import _stats_for, assert_same_bits, hd, ht, track

pytestmark = pytest.mark.gpu
SR = 44100
CANARY = 0x7B1D2C3E                 # a float bit pattern no conversion below produces


def stream_ptr():
    return C.c_void_p(_lib.current_stream_ptr())


# ---- numpy side: wire bytes and the floats they stand for ---------------------------------------------------------------------------
def wire_values(fmt, count, seed):
    """`count` sample values of a format, the extremes and (f32) the special values among them, as the array `encode` packs."""
    rng = np.random.default_rng(seed)
    if fmt == "f32":
        v = rng.standard_normal(count).astype(np.float32)
        special = np.array([0x7FC00001, 0xFFC12345, 0x7F800000, 0xFF800000, 0x80000000, 0x00000001, 0x807FFFFF, 0x00400000, 0x7F7FFFFF],
                           dtype=np.uint32).view(np.float32)          # NaNs with payloads, +-Inf, -0, subnormals, the largest
    else:
        lo, hi = (-32768, 32767) if fmt == "i16" else (-(1 << 23), (1 << 23) - 1)
        v = rng.integers(lo, hi + 1, count).astype(np.int32)
        special = np.array([lo, hi, 0, -1, 1, lo + 1, hi - 1], dtype=np.int32)
    at = np.arange(0, count, 3)
    v[at] = special[np.arange(len(at)) % len(special)]
    return v


def encode(fmt, v):
    """The little-endian wire bytes of the values."""
    if fmt == "i16":
        return v.astype("<i2").tobytes()
    if fmt == "f32":
        return v.astype("<f4").tobytes()
    u = v.astype(np.int64) & 0xFFFFFF
    return np.stack([u & 255, (u >> 8) & 255, (u >> 16) & 255], -1).astype(np.uint8).tobytes()


def decode(fmt, v):
    """float32 of the values: the contract's `float32(v) * 2^-15` / `* 2^-23` / the bits."""
    if fmt == "f32":
        return v.astype(np.float32)
    return v.astype(np.float32) * np.float32(2.0 ** -15 if fmt == "i16" else 2.0 ** -23)


def planar(fmt, v, src_ch, channels):
    """(channels, n) float32: convert_audio_channels' per-sample map of the decoded (n, src_ch) frames."""
    x = decode(fmt, v).reshape(-1, src_ch).T
    return np.ascontiguousarray(np.repeat(x, channels, 0) if src_ch == 1 else x[:channels])


def affine(x, stats):
    with np.errstate(all="ignore"):
        return ((x - np.float32(stats[0])) / np.float32(stats[1])).astype(np.float32)


def bits(x, canonical_nan=False):
    x = np.ascontiguousarray(x, dtype=np.float32)
    if canonical_nan:
        x = np.where(np.isnan(x), np.float32("nan"), x)
    return x.view(np.int32)


def device_bytes(data: bytes, offset: int = 0, pad: int = 64) -> torch.Tensor:
    """`data` at byte `offset` of a larger device buffer (the allocation is 256-byte aligned)."""
    host = np.full(offset + len(data) + pad, 0xA5, dtype=np.uint8)
    host[offset:offset + len(data)] = np.frombuffer(data, dtype=np.uint8)
    buf = torch.from_numpy(host).cuda()
    assert buf.data_ptr() % 256 == 0
    return buf[offset:offset + len(data)]


# ---- 1. mi_pcm_planar alone ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["i16", "i24", "f32"])
def test_pcm_planar_equals_numpy(fmt):
    lib = _lib.load()
    code, width, _ = PCM_FORMATS[fmt]
    stats_host = (0.25, 1.75)
    stats = torch.tensor(stats_host, dtype=torch.float32).cuda()
    channels, guard = 2, 64
    for src_ch in (1, 2, 3):
        for n in (0, 1, 3, 4, 5, 63, 64, 65, 1023, 1024, 1025, 4099):
            v = wire_values(fmt, n * src_ch, seed=n * 3 + src_ch)
            want = planar(fmt, v, src_ch, channels)
            for shift in (0, 1, 3):
                src = device_bytes(encode(fmt, v), shift * width)
                for st in (None, stats):
                    out = torch.full((guard + channels * n + guard,), 0, dtype=torch.int32, device="cuda").fill_(CANARY)
                    dst = out[guard:guard + channels * n]
                    _lib.check(lib.mi_pcm_planar(src.data_ptr() if n else None, code, src_ch, n, channels,
                                                 st.data_ptr() if st is not None else None, dst.data_ptr() if n else None,
                                                 stream_ptr()), "mi_pcm_planar")
                    got = out.cpu().numpy()
                    what = f"{fmt} src_ch={src_ch} n={n} shift={shift} stats={st is not None}"
                    assert (got[:guard] == CANARY).all() and (got[guard + channels * n:] == CANARY).all(), what
                    ref = want if st is None else affine(want, stats_host)
                    # without stats every bit is the source's, NaN payloads included; a NaN through the affine is any NaN
                    ref_bits = bits(ref, canonical_nan=st is not None).reshape(-1)
                    got_bits = got[guard:guard + channels * n]
                    if st is not None:
                        got_bits = bits(got_bits.view(np.float32), canonical_nan=True)
                    bad = np.nonzero(got_bits != ref_bits)[0]
                    assert len(bad) == 0, f"{what}: {len(bad)} differ, first at {bad[:4]}: {got_bits[bad[:4]]} != {ref_bits[bad[:4]]}"


def test_pcm_planar_refusals():
    lib = _lib.load()
    buf = torch.zeros(64, dtype=torch.uint8, device="cuda")
    out = torch.zeros(64, device="cuda")
    for args in [(buf.data_ptr(), 0, 2, 4, 2), (buf.data_ptr(), 4, 2, 4, 2), (buf.data_ptr(), 1, 0, 4, 2), (buf.data_ptr(), 1, 3, 4, 4),
                 (buf.data_ptr(), 1, 2, -1, 2), (buf.data_ptr() + 1, 1, 2, 4, 2), (buf.data_ptr() + 2, 3, 2, 4, 2), (None, 1, 2, 4, 2)]:
        assert lib.mi_pcm_planar(args[0], args[1], args[2], args[3], args[4], None, out.data_ptr(), stream_ptr()) != 0, args
    assert lib.mi_pcm_planar(buf.data_ptr() + 1, 2, 2, 4, 2, None, out.data_ptr(), stream_ptr()) == 0       # i24: any byte address
    torch.cuda.synchronize()


# ---- 2. mi_streams_append_pcm against mi_streams_append on the converted floats ------------------------------------------------------
def _append(entry, win, table, n_rows, longest, stats, n_stats, win_cap=None):
    lib = _lib.load()
    _lib.check(getattr(lib, entry)(win.data_ptr(), win.numel() if win_cap is None else win_cap, 2, table.data_ptr(), n_rows, longest,
                                   stats.data_ptr(), n_stats, stream_ptr()), entry)


def test_streams_append_pcm_equals_streams_append_on_the_floats():
    """Six rows of mixed formats and channel counts (one of them planar float32, one at an odd byte address) in ONE launch: the whole
    window buffer, untouched columns included, is what mi_streams_append writes from the converted planar floats."""
    stats = torch.tensor([0.25, 1.75, -0.5, 0.125], dtype=torch.float32).cuda()
    spec = [("i16", 2, 4099, 0, 0), ("i24", 1, 1025, 1, -1), ("f32", 3, 777, 0, 1), (None, 2, 2051, 0, 0), ("i24", 2, 64, 2, -1),
            ("i16", 1, 1, 3, 1)]                          # (format or planar, src_ch, n, source shift in samples, stats index)
    keep, rows_pcm, rows_f32 = [], [], []
    off, longest, max_bytes = 37, 1, 1
    for k, (fmt, src_ch, n, shift, si) in enumerate(spec):
        dst_len, col = n + 100 + k, 11 * k + 3
        if fmt is None:
            x = torch.randn(2, n, generator=torch.Generator().manual_seed(k)).cuda()
            keep.append(x)
            rows_pcm += [x.data_ptr(), n, off, dst_len, col, si, PCM_PLANAR, 2]
            max_bytes = max(max_bytes, 4 * 2 * n)
        else:
            v = wire_values(fmt, n * src_ch, seed=50 + k)
            raw = device_bytes(encode(fmt, v), shift * PCM_FORMATS[fmt][1])
            x = torch.from_numpy(planar(fmt, v, src_ch, 2)).cuda()
            keep += [raw, x]
            rows_pcm += [raw.data_ptr(), n, off, dst_len, col, si, PCM_FORMATS[fmt][0], src_ch]
            max_bytes = max(max_bytes, raw.numel())
        rows_f32 += [x.data_ptr(), n, off, dst_len, col, si]
        off += 2 * dst_len + 5
        longest = max(longest, n)
    assert len(rows_pcm) == APPEND_PCM_COLS * len(spec) and len(rows_f32) == APPEND_COLS * len(spec)
    wins = []
    for entry, rows, size in (("mi_streams_append", rows_f32, longest), ("mi_streams_append_pcm", rows_pcm, max_bytes)):
        win = torch.full((off + 50,), 7.0, device="cuda")
        _append(entry, win, torch.tensor(rows, dtype=torch.int64).cuda(), len(spec), size, stats, 2)
        wins.append(win)
    torch.cuda.synchronize()
    assert int((wins[0] != 7.0).sum()) >= sum(2 * s[2] for s in spec) - 8          # the float entry did write the blocks
    a, b = (w.view(torch.int32) for w in wins)
    assert torch.equal(a, b), f"{int((a != b).sum())} floats differ"


def test_streams_append_pcm_malformed_destinations_write_nothing_outside():
    """Destination columns far out of range, and blocks longer than their room: the guard regions and every float outside a row's
    own columns [col, dst_len) stay as they were; the sources are live and as large as the rows say."""
    n, cap, guard = 600, 3000, 4096
    v = wire_values("i16", 2 * n, seed=9)
    raw = device_bytes(encode("i16", v))
    x = torch.randn(2, n).cuda()
    stats = torch.tensor([0.0, 1.0], dtype=torch.float32).cuda()
    whole = torch.full((guard + cap + guard,), 7.0, device="cuda")
    win = whole[guard:guard + cap]
    big = 1 << 40
    rows, allowed = [], torch.zeros(cap, dtype=torch.bool)
    for src, fmt, src_ch in ((raw.data_ptr(), 1, 2), (x.data_ptr(), PCM_PLANAR, 2)):
        for dst_off, dst_len, col in [(0, 500, 501), (0, 500, big), (0, 500, -1), (cap - 999, 500, 0), (big, 500, 0), (-8, 500, 0),
                                      (0, cap, 0), (0, big, 0), (0, -5, 0), (100, 700, 650), (1700, 300, 0)]:
            rows += [src, n, dst_off, dst_len, col, 0, fmt, src_ch]
            if (dst_off, dst_len, col) in [(100, 700, 650), (1700, 300, 0)]:      # n beyond the room: the row's columns only
                for c in range(2):
                    allowed[dst_off + c * dst_len + col:dst_off + (c + 1) * dst_len] = True
        rows += [src, n, 0, 500, 0, 0, 7, src_ch] + [src, n, 0, 500, 0, 0, -1, src_ch]      # unknown formats
    rows += [raw.data_ptr(), n, 0, 500, 0, 0, 1, 0] + [raw.data_ptr() + 1, n, 0, 500, 0, 0, 1, 2]      # no channels; misaligned i16
    rows += [raw.data_ptr(), 200, 0, 500, 0, 0, 1, 3]      # 3 source channels into 2 rows is fine, so this one names room it may use
    allowed[0:200] = allowed[500:700] = True
    n_rows = len(rows) // APPEND_PCM_COLS
    _append("mi_streams_append_pcm", win, torch.tensor(rows, dtype=torch.int64).cuda(), n_rows, 4 * 2 * n, stats, 1, win_cap=cap)
    torch.cuda.synchronize()
    got = whole.cpu()
    assert bool((got[:guard] == 7.0).all()) and bool((got[-guard:] == 7.0).all())
    inner = got[guard:guard + cap]
    assert bool((inner[~allowed] == 7.0).all()), f"{int((inner[~allowed] != 7.0).sum())} floats outside the rows' columns changed"
    assert bool((inner[allowed] != 7.0).any())


# ---- 3. mi_streams_convert_append_pcm against mi_streams_convert_append on the floats ------------------------------------------------
def _blocks(length, seed, big):
    rng = np.random.default_rng(seed)
    out, total = [0, 1], 1
    while total < length:
        b = min(length - total, int(rng.choice([0, 1, int(rng.integers(1, 40)), int(rng.integers(1, big))])))
        out.append(b)
        total += b
    return out


@pytest.mark.parametrize("pair", PAIRS)
def test_convert_append_pcm_equals_convert_append_on_the_floats(pair):
    """One stream through both entries, call by call over random partitions (blocks of 0 and 1 frame among them) and the final
    call: the window and both sides of the history are the same bits after every call."""
    lib = _lib.load()
    plan = ConvertPlan(*pair)
    width, bank = audio.sinc_bank(plan.old, plan.new)
    bank = bank.t().contiguous().reshape(-1).cuda()
    stats = torch.tensor([0.25, 1.75], dtype=torch.float32).cuda()
    L = plan.width + 5 * plan.old + 7
    n_total = plan.final_count(L)
    # every pair takes i16 stereo and i24 mono, and in turn f32 with three channels or i24 stereo
    for k, (fmt, src_ch) in enumerate([("i16", 2), ("i24", 1), [("f32", 3), ("i24", 2)][PAIRS.index(pair) % 2]]):
        v = wire_values(fmt, L * src_ch, seed=L + k)
        if fmt == "f32":
            v = np.where(np.isfinite(v), v, np.float32(0.5))    # the filter spreads a NaN; the stream tests cover that
        frames = np.frombuffer(encode(fmt, v), dtype=np.uint8)
        x = decode(fmt, v).reshape(L, src_ch).T
        fw = src_ch * PCM_FORMATS[fmt][1]
        for seed in range(2):
            wins = [torch.full((2 * (n_total + 9),), 7.0, device="cuda") for _ in range(2)]
            hists = [torch.zeros(2 * 2 * plan.carry + 8, device="cuda") for _ in range(2)]
            P, h0, side, col = 0, 0, 0, 4
            for b in _blocks(L, seed + k, 3 * plan.old) + [None]:
                final = b is None
                n_in = 0 if final else b
                out0, n_out, nxt = plan.step(P, n_in, final)
                raw = device_bytes(frames[P * fw:(P + n_in) * fw].tobytes(), [0, 1, 3][(seed + k) % 3] * PCM_FORMATS[fmt][1])
                blk = torch.from_numpy(np.ascontiguousarray(x[:, P:P + n_in])).cuda()
                side_len = 2 * plan.carry
                row = [0, src_ch, n_in, P, plan.carry, 4 + side * side_len, 4 + (1 - side) * side_len, h0, nxt, out0, n_out,
                       L if final else -1, plan.old, plan.new, plan.width, 0, 0, n_total + 9, col, 0]
                for which, (entry, src, extra) in enumerate([("mi_streams_convert_append", blk, []),
                                                             ("mi_streams_convert_append_pcm", raw, [PCM_FORMATS[fmt][0]])]):
                    row[0] = src.data_ptr() if n_in else 0
                    table = torch.tensor(row + extra, dtype=torch.int64).cuda()
                    assert table.numel() == (CVT_PCM_COLS if extra else CVT_COLS)
                    _lib.check(getattr(lib, entry)(wins[which].data_ptr(), wins[which].numel(), 2, table.data_ptr(), 1,
                                                   plan.groups(n_out), bank.data_ptr(), bank.numel(), hists[which].data_ptr(),
                                                   hists[which].numel(), stats.data_ptr(), 1, plan.lds_floats(), stream_ptr()), entry)
                torch.cuda.synchronize()
                what = f"{pair} {fmt} x{src_ch} partition {seed} at {P}+{n_in}"
                assert torch.equal(wins[0].view(torch.int32), wins[1].view(torch.int32)), what
                assert torch.equal(hists[0].view(torch.int32), hists[1].view(torch.int32)), what
                col += n_out
                P += n_in
                if not final:
                    h0, side = nxt, 1 - side
            assert col - 4 == n_total and P == L
            assert bool((wins[1][4:4 + n_total] != 7.0).all())
    # a planar row of the PCM entry is the float entry's row
    n_in = plan.width + 3 * plan.old
    blk = torch.randn(2, n_in).cuda()
    out0, n_out, nxt = plan.step(0, n_in, False)
    row = [blk.data_ptr(), 2, n_in, 0, plan.carry, 0, 2 * plan.carry, 0, nxt, out0, n_out, -1, plan.old, plan.new, plan.width, 0, 0,
           n_out, 0, -1]
    res = []
    for entry, extra in (("mi_streams_convert_append", []), ("mi_streams_convert_append_pcm", [PCM_PLANAR])):
        win, hist = torch.full((2 * n_out,), 7.0, device="cuda"), torch.zeros(4 * plan.carry, device="cuda")
        table = torch.tensor(row + extra, dtype=torch.int64).cuda()
        _lib.check(getattr(lib, entry)(win.data_ptr(), win.numel(), 2, table.data_ptr(), 1, plan.groups(n_out), bank.data_ptr(),
                                       bank.numel(), hist.data_ptr(), hist.numel(), stats.data_ptr(), 1, plan.lds_floats(),
                                       stream_ptr()), entry)
        res.append((win, hist))
    assert_same_bits(res[1][0], res[0][0], "planar row, window")
    assert_same_bits(res[1][1], res[0][1], "planar row, history")


# ---- 4. the streams, end to end -----------------------------------------------------------------------------------------------------------
def to_i16(wav):
    """(channels, n) float -> ((n, channels) int16 frames, the (channels, n) floats they stand for)."""
    q = (wav * 32767.0).round().clamp(-32768, 32767).to(torch.int16).t().contiguous()
    return q, (q.to(torch.float32) / 32768.0).t().contiguous()


def byte_chunks(data: bytes, seed, typical):
    """`data` cut at random byte positions (inside samples and frames, empty chunks among them)."""
    rng = random.Random(seed)
    out, pos = [], 0
    while pos < len(data):
        b = rng.choice([0, 1, 3, rng.randint(1, 64), rng.randint(1, typical), rng.randint(1, 3 * typical)])
        out.append(data[pos:pos + b])
        pos += b
    return out


def two_segments_and_a_tail(model):
    m = ModelStream(model, shifts=0).members[0]
    return m.SL + m.stride + 1001


def run_stream(ss, blocks):
    outs = [ss.push(b) for b in blocks]
    outs.append(ss.finish())
    return {k: torch.cat([o[k] for o in outs], 0 if outs[0][k].dtype == torch.int16 else -1) for k in outs[0]}


@pytest.mark.parametrize("make,mode", [(ht, "f32"), (ht, "bf16"), (hd, "f16")])
def test_separate_stream_i16_equals_the_float_stream(make, mode):
    model = make(mode) if make is ht else make(mode, segment=3)
    L = two_segments_and_a_tail(model)
    frames, floats = to_i16(track(L, seed=41) * 0.8)
    data = frames.numpy().tobytes() + b"\x12\x34\x56"                  # an incomplete last frame: dropped
    sep = Separator(model, device="cuda", shifts=1)
    for mean, std in [(None, None), _stats_for(floats)]:
        random.seed(11)
        want = run_stream(sep.separate_stream(mean, std), [floats[:, i:i + SR] for i in range(0, L, SR)])
        state = random.getstate()
        random.seed(11)
        ss = sep.separate_stream(mean, std, pcm="i16")
        got = run_stream(ss, byte_chunks(data, seed=len(mode), typical=4 * SR))
        assert random.getstate() == state
        assert ss.trailing_bytes == 3 and ss.stream.pushed == L and ss.emitted == L
        for k in want:
            assert got[k].device.type == "cpu" and got[k].shape == (2, L)
            assert_same_bits(got[k], want[k], f"{mode} {k} stats={mean is not None}")


def test_device_blocks_and_typed_tensors():
    """The same stream fed (n, 2) int16 tensors on the device, 1-D uint8 device tensors and host bytes in turn; malformed device
    blocks are refused with nothing changed."""
    model = hd("f16", segment=3)
    L = 4 * SR + 77
    frames, floats = to_i16(track(L, seed=42) * 0.8)
    sep = Separator(model, device="cuda", shifts=1)
    random.seed(3)
    want = run_stream(sep.separate_stream(0.01, 0.5), [floats.cuda()])
    random.seed(3)
    ss = sep.separate_stream(0.01, 0.5, pcm="i16", length=L)
    dev = frames.cuda()
    state = random.getstate()
    for bad in (dev.view(torch.uint8).reshape(-1)[:4 * 100 + 2], dev.view(torch.uint8).reshape(-1)[1:4 * 100 + 1],
                torch.zeros(100, 2, dtype=torch.int32, device="cuda"), dev[:1].expand(L + 1, 2)):
        with pytest.raises(ValueError):
            ss.push(bad)
        assert random.getstate() == state and ss.stream.pushed == 0 and ss.trailing_bytes == 0
    outs = [ss.push(dev[:SR]), ss.push(dev[SR:2 * SR].view(torch.uint8).reshape(-1))]
    assert all(v.device.type == "cuda" for o in outs for v in o.values())
    outs.append(ss.push(frames[2 * SR:].numpy().tobytes()))
    outs.append(ss.finish())
    for k in want:
        assert_same_bits(torch.cat([o[k].cuda() for o in outs], -1), want[k], k)


def test_converting_i16_stream_equals_separate_tensor_and_delivers_the_same_frames():
    sr = 48000
    L = 9 * sr + 321
    frames, floats = to_i16(track(L, seed=43)[:1] * 0.7)               # mono, 48 kHz
    data = frames.numpy().tobytes()
    sep = Separator(ht("f32"), device="cuda", shifts=1)
    random.seed(5)
    _, want = sep.separate_tensor(floats.clone(), sr=sr)
    state = random.getstate()
    mean, std = _stats_for(audio.convert_audio(floats.cuda(), sr, SR, 2))
    random.seed(5)
    ss = sep.separate_stream(mean, std, sr=sr, channels=1, convert=True, pcm="i16", length=L)
    got = run_stream(ss, byte_chunks(data, seed=1, typical=2 * sr))
    assert random.getstate() == state and ss.pushed_input == L and ss.trailing_bytes == 0
    for k in want:
        assert_same_bits(got[k], want[k], k)
    # wire frames in, wire frames out
    dl = dict(fmt="i16", samplerate=sr)
    random.seed(5)
    want_frames = run_stream(sep.separate_stream(mean, std, sr=sr, channels=1, convert=True, deliver=Delivery(**dl)),
                             [floats[:, i:i + sr] for i in range(0, L, sr)])
    random.seed(5)
    got_frames = run_stream(sep.separate_stream(mean, std, sr=sr, channels=1, convert=True, deliver=Delivery(**dl), pcm="i16"),
                            byte_chunks(data, seed=2, typical=2 * sr))
    for k in want_frames:
        assert got_frames[k].dtype == torch.int16 and got_frames[k].shape == want_frames[k].shape and got_frames[k].shape[0] > 8 * sr
        assert torch.equal(got_frames[k], want_frames[k]), k


# ---- 5. a group of mixed feeds --------------------------------------------------------------------------------------------------------------
def _group_feeds(nan=False):
    """[(open keywords, [blocks])]: a planar-float stream, an i16 stream, a converting mono i24 stream at 48 kHz and an f32 stream."""
    feeds = []
    n = 9 * SR
    plain = track(n + 5, seed=60) * 0.5
    feeds.append((dict(), [plain[:, i:i + SR] for i in range(0, n + 5, SR)]))
    frames, _ = to_i16(track(n + 17, seed=61) * 0.6)
    feeds.append((dict(pcm="i16"), byte_chunks(frames.numpy().tobytes(), seed=6, typical=4 * SR)))
    m = track(9 * 48000 + 3, seed=62)[:1] * 0.6
    v24 = (m[0] * (2 ** 23 - 1)).round().to(torch.int32).numpy()
    feeds.append((dict(pcm="i24", sr=48000, channels=1), byte_chunks(encode("i24", v24), seed=7, typical=3 * 48000)))
    f = (track(n + 29, seed=63) * 0.5).t().contiguous()
    if nan:
        f[3 * SR + 5, 0] = float("nan")
    feeds.append((dict(pcm="f32"), byte_chunks(f.numpy().tobytes(), seed=8, typical=8 * SR)))
    return feeds


def _run_feeds(sep, feeds, grouped):
    """Stream i opens at call i and is finished once its blocks are used up; [{i: result}] per call."""
    g = sep.separate_stream_group() if grouped else None
    handles, calls, pos = {}, [], [0] * len(feeds)
    step = 0
    while len(handles) < len(feeds) or any(h is not None for h in handles.values()):
        if step < len(feeds):
            kw = feeds[step][0]
            handles[step] = g.open(0.0, 1.0, **kw) if grouped else \
                sep.separate_stream(0.0, 1.0, convert="sr" in kw, **kw)
        blocks, done = {}, []
        for i, h in handles.items():
            if h is None:
                continue
            if pos[i] < len(feeds[i][1]):
                blocks[i] = feeds[i][1][pos[i]]
                pos[i] += 1
            else:
                done.append(i)
        if blocks:
            if grouped:
                got = g.push({handles[i]: b for i, b in blocks.items()})
                calls.append({i: got[handles[i]] for i in blocks})
            else:
                calls.append({i: handles[i].push(b) for i, b in blocks.items()})
        if done:
            if grouped:
                got = g.finish([handles[i] for i in done])
                calls.append({i: got[handles[i]] for i in done})
            else:
                calls.append({i: handles[i].finish() for i in done})
            for i in done:
                handles[i] = None
        step += 1
    return calls


def test_group_of_mixed_feeds_equals_the_solo_streams_and_a_nan_stays_in_its_stream():
    sep = Separator(ht("f32", max_batch=4), device="cuda", shifts=0)
    feeds = _group_feeds()
    want = _run_feeds(sep, feeds, grouped=False)
    got = _run_feeds(sep, feeds, grouped=True)
    assert len(got) == len(want)
    total = Counter()
    for call, (g, w) in enumerate(zip(got, want)):
        assert list(g) == list(w)
        for i in w:
            for k in w[i]:
                assert g[i][k].shape == w[i][k].shape and g[i][k].device.type == "cpu", (call, i, k)
                assert_same_bits(g[i][k], w[i][k], f"call {call} stream {i} {k}")
            total[i] += next(iter(w[i].values())).shape[-1]
    assert total[0] == 9 * SR + 5 and total[1] == 9 * SR + 17 and total[3] == 9 * SR + 29
    assert total[2] == ConvertPlan(48000, SR).final_count(9 * 48000 + 3)
    dirty = _run_feeds(sep, _group_feeds(nan=True), grouped=True)
    poisoned = False
    for c, d in zip(got, dirty):
        for i in c:
            for k in c[i]:
                if i == 3:
                    poisoned = poisoned or not bool(torch.isfinite(d[i][k]).all())
                else:
                    assert_same_bits(d[i][k], c[i][k], f"stream {i} {k} beside a NaN")
    assert poisoned


# ---- 6. calls, copies and bytes per push --------------------------------------------------------------------------------------------------
PER_FORWARD = {"mi_segments_gather_packed", "mi_ola_accumulate_packed"}


def _count_pushes(n_pcm, monkeypatch, pushes=10):
    """Pushes of 1 s host blocks into n_pcm int16 streams, a converting int24 stream and a float stream: per push the library
    calls outside the forwards, the host -> device copies, and the pinned upload against its bound."""
    m = ht("f32", max_batch=8)
    lib = _lib.load()
    counts, in_forward, h2d = Counter(), [False], [0]
    for name in _lib.SIGNATURES:
        real = getattr(lib, name)

        def wrapped(*args, _real=real, _name=name):
            if not in_forward[0]:
                counts[_name] += 1
            return _real(*args)

        monkeypatch.setattr(lib, name, wrapped)
    real_fwd = type(m).forward_segments

    def forward(self, *a, **k):
        in_forward[0] = True
        try:
            return real_fwd(self, *a, **k)
        finally:
            in_forward[0] = False

    monkeypatch.setattr(type(m), "forward_segments", forward)
    real_copy, real_to = torch.Tensor.copy_, torch.Tensor.to

    def copy_(self, src, *a, **k):
        if self.is_cuda and not src.is_cuda and not in_forward[0]:
            h2d[0] += 1
        return real_copy(self, src, *a, **k)

    def to(self, *a, **k):
        out = real_to(self, *a, **k)
        if out.is_cuda and not self.is_cuda and not in_forward[0]:
            h2d[0] += 1
        return out

    monkeypatch.setattr(torch.Tensor, "copy_", copy_)
    monkeypatch.setattr(torch.Tensor, "to", to)
    sep = Separator(m, device="cuda", shifts=1)
    g = sep.separate_stream_group()
    frames, _ = to_i16(track(SR, seed=51) * 0.5)
    data16 = frames.numpy().tobytes()
    mono = track(48000, seed=50)[:1] * 0.5
    data24 = encode("i24", (mono[0] * (2 ** 23 - 1)).round().to(torch.int32).numpy())
    blocks = {g.open(0.0, 1.0, pcm="i16"): data16 for _ in range(n_pcm)}
    blocks[g.open(0.0, 1.0, pcm="i24", sr=48000, channels=1)] = data24
    blocks[g.open(0.0, 1.0)] = track(SR, seed=52)
    # the i16 blocks: table plus at most 4 n + 16 bytes each; the int24 mono block 3 n + 16, the float block 8 n + 16
    bound = n_pcm * (4 * SR + 16) + 3 * 48000 + 16 + 8 * SR + 16
    worst = Counter()
    gc.collect()
    gc.disable()                    # an earlier test's model, collected mid-push, would count its mi_model_destroy here
    try:
        for i in range(pushes):
            counts.clear()
            h2d[0] = 0
            g.push(blocks)
            table_bytes, upload = g.group._exec.last_upload
            assert upload <= table_bytes + bound, (upload, table_bytes, bound)
            assert upload >= n_pcm * 4 * SR + 3 * 48000 + 8 * SR
            appends = counts["mi_streams_append"] + counts["mi_streams_append_pcm"]
            converts = counts["mi_streams_convert_append"] + counts["mi_streams_convert_append_pcm"]
            assert appends == 1 and counts["mi_streams_append_pcm"] == 1, counts
            assert converts == 1 and counts["mi_streams_convert_append_pcm"] == 1, counts
            assert counts["mi_pcm_planar"] == 0 and counts["mi_track_affine"] == 0
            # one H2D per call: the table with the blocks behind it; the first call also uploads the streams' stats pairs and,
            # in a fresh process, the resampler's kernel bank
            assert h2d[0] == 1 if i else 1 <= h2d[0] <= 3, (i, h2d[0])
            worst["other"] = max(worst["other"], sum(v for k, v in counts.items() if k not in PER_FORWARD and not k.endswith("_destroy")))
    finally:
        gc.enable()
    g.finish(list(blocks))
    monkeypatch.undo()
    return worst["other"]


def test_calls_copies_and_bytes_per_push_do_not_grow_with_pcm_streams(monkeypatch):
    a = _count_pushes(1, monkeypatch)
    b = _count_pushes(6, monkeypatch)
    assert a <= 4 and b <= 4, (a, b)          # append, convert-append, emit and at most one compaction


# ---- 7. a whole buffer --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt,channels", [("i16", 2), ("i24", 2), ("f32", 2), ("i16", 1), ("i24", 3)])
def test_pcm_to_tensor_equals_numpy(fmt, channels):
    n = 5003
    v = wire_values(fmt, n * channels, seed=n + channels)
    data = encode(fmt, v)
    want = decode(fmt, v).reshape(n, channels).T
    for block in (data, data + b"\x01", bytearray(data), torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()):
        got = audio.pcm_to_tensor(block, fmt, channels)
        assert got.shape == (channels, n) and got.dtype == torch.float32 and got.is_cuda
        assert (got.cpu().numpy().view(np.int32) == bits(want)).all()
    assert audio.pcm_to_tensor(b"", fmt, channels).shape == (channels, 0)


def test_separate_tensor_takes_a_decoded_payload():
    model = hd("f16", segment=3)
    L = 4 * SR + 77
    frames, floats = to_i16(track(L, seed=44) * 0.8)
    head = audio.wav_header(L, SR, 2, "i16")
    file = head + frames.numpy().tobytes()
    fmt, channels, rate, count, at = audio.wav_info(file[:64])
    assert (fmt, channels, rate, count, at) == ("i16", 2, SR, L, 44)
    sep = Separator(model, device="cuda", shifts=1)
    random.seed(9)
    _, want = sep.separate_tensor(floats.cuda(), sr=rate)
    random.seed(9)
    wav = audio.pcm_to_tensor(memoryview(file)[at:], fmt, channels)
    assert_same_bits(wav, floats.cuda(), "payload")
    _, got = sep.separate_tensor(wav, sr=rate)
    for k in want:
        assert_same_bits(got[k], want[k], k)
