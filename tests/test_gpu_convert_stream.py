"""The streaming `convert_audio` on the MI355X (`mi_streams_convert_append`, `audio.ConvertStream`,
`Separator.separate_stream(convert=True)`, `SeparatorStreamGroup.open(sr=...)`): whatever the partition of the input, the
concatenated outputs are the one-piece `convert_audio` / `separate_tensor(wav, sr)` bit for bit (NaN positions included), a push
stays a fixed number of launches, and device state does not grow with the stream.  Every comparison is `assert_same_bits`."""
import ctypes as C
import gc
import random
from collections import Counter

import numpy as np
import pytest
import torch

from demucs_amd import _lib, audio
from demucs_amd.api import Separator
from demucs_amd.audio import CVT_COLS, ConvertPlan, convert_audio_stream
from test_gpu_stream import _stats_for, assert_same_bits, hd, ht, track

pytestmark = pytest.mark.gpu
SR = 44100
PAIRS = [(48000, 44100), (96000, 44100), (32000, 44100), (22050, 44100), (8000, 44100), (44100, 16000)]


def stream_ptr():
    return C.c_void_p(_lib.current_stream_ptr())


def partition(length, seed, big):
    rng = np.random.default_rng(seed)
    out, total = [], 0
    while total < length:
        b = int(rng.choice([0, 1, int(rng.integers(1, 40)), int(rng.integers(1, big))]))
        out.append(b)
        total += b
    return out


def streamed_convert(full, from_sr, to_sr, channels, blocks, affine=None):
    cs = convert_audio_stream(from_sr, to_sr, channels, affine=affine)
    outs, pos = [], 0
    for b in blocks:
        blk = full[:, pos:pos + b]
        pos += blk.shape[1]
        o = cs.push(blk)
        assert o.device == full.device and o.shape == (channels, cs.emitted - sum(x.shape[1] for x in outs))
        assert cs.pushed == pos and cs.plan.final_count(pos) - cs.emitted <= cs.hold
        outs.append(o)
    outs.append(cs.finish())
    assert cs.emitted == cs.plan.final_count(full.shape[1])
    return torch.cat(outs, -1)


def noise(channels, n, seed, device="cpu"):
    return torch.randn(channels, n, generator=torch.Generator().manual_seed(seed)).to(device)


# ---- 1. ConvertStream over random partitions ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("pair", PAIRS)
@pytest.mark.parametrize("where", ["cpu", "cuda"])
def test_convert_stream_equals_convert_audio(pair, where):
    plan = ConvertPlan(*pair)
    w, old = plan.width, plan.old
    lengths = [1, w, w + old - 1, w + old, w + old + 1, w + 3 * old - 1, w + 3 * old, w + 3 * old + 1, 7 * old + 5, pair[0] // 3 + 11]
    if pair[0] == 48000:
        lengths.append(10 * pair[0] + 37)
    for k, L in enumerate(lengths):
        src_channels = [2, 1, 3][k % 3]
        full = noise(src_channels, L, seed=L + k, device=where)
        want = audio.convert_audio(full.cuda(), pair[0], pair[1], 2)
        for seed in range(2):
            got = streamed_convert(full, pair[0], pair[1], 2, partition(L, seed + k, max(2, min(L, 3 * pair[0]))))
            assert got.device == full.device
            assert_same_bits(got.cuda(), want, f"{pair} L={L} partition {seed}")
        assert_same_bits(streamed_convert(full, pair[0], pair[1], 2, [L]).cuda(), want, f"{pair} L={L} one block")
        if L < 700:
            assert_same_bits(streamed_convert(full, pair[0], pair[1], 2, [1] * L).cuda(), want, f"{pair} L={L} single samples")


@pytest.mark.parametrize("src_channels", [1, 3, 2])
def test_equal_rates_convert_the_channels_only(src_channels):
    L = 5000
    full = noise(src_channels, L, seed=src_channels, device="cuda")
    full[0, 17] = -0.0                                  # a copy keeps the sign of zero; a filter would not
    want = audio.convert_audio(full, SR, SR, 2).contiguous()
    got = streamed_convert(full, SR, SR, 2, partition(L, 3, 2000))
    assert_same_bits(got, want, f"{src_channels} -> 2")
    assert convert_audio_stream(SR, SR, 2).hold == 0


def test_refusals_on_the_device():
    with pytest.raises(ValueError, match="mono"):
        convert_audio_stream(48000, SR, 1).push(torch.zeros(2, 10, device="cuda"))
    with pytest.raises(ValueError, match="less channels"):
        convert_audio_stream(48000, SR, 4).push(torch.zeros(3, 10, device="cuda"))
    cs = convert_audio_stream(48000, SR, 2)
    cs.push(torch.zeros(1, 10, device="cuda"))
    with pytest.raises(ValueError, match="block"):
        cs.push(torch.zeros(2, 10, device="cuda"))


# ---- 2. the kernel alone through the C ABI -------------------------------------------------------------------------------------------
def _bank_t(plan):
    width, bank = audio.sinc_bank(plan.old, plan.new)
    return bank.t().contiguous().reshape(-1).cuda()


def _whole(x, plan, stats):
    """mi_resample_frac + mi_track_affine on the whole rows."""
    lib = _lib.load()
    width, bank = audio.sinc_bank(plan.old, plan.new)
    table = bank.cuda()
    y = torch.empty(x.shape[0], plan.final_count(x.shape[1]), device="cuda")
    _lib.check(lib.mi_resample_frac(x.data_ptr(), x.shape[0], x.shape[1], table.data_ptr(), plan.old, plan.new, width, y.data_ptr(),
                                    y.shape[1], stream_ptr()), "mi_resample_frac")
    if stats is not None:
        _lib.check(lib.mi_track_affine(y.data_ptr(), y.numel(), stats.data_ptr(), 0, stream_ptr()), "mi_track_affine")
    return y


def _launch(win, table, n_rows, groups, bank, hist, stats, n_stats, lds_floats, channels=2, win_cap=None, hist_cap=None,
            bank_cap=None):
    lib = _lib.load()
    _lib.check(lib.mi_streams_convert_append(win.data_ptr(), win.numel() if win_cap is None else win_cap, channels, table.data_ptr(),
                                             n_rows, groups, bank.data_ptr(), bank.numel() if bank_cap is None else bank_cap,
                                             hist.data_ptr(), hist.numel() if hist_cap is None else hist_cap,
                                             stats.data_ptr() if stats is not None else None, n_stats, lds_floats, stream_ptr()),
               "mi_streams_convert_append")


def test_kernel_writes_its_own_columns_only():
    """Two streams of different rates in one launch, two calls each (a push, then the final call), into windows pre-filled with
    NaN: the columns [col, col + n_out) hold mi_resample_frac + mi_track_affine's bits, every other float is still NaN."""
    plans = [ConvertPlan(48000, SR), ConvertPlan(8000, SR)]
    banks = [_bank_t(p) for p in plans]
    bank = torch.cat(banks)
    bank_offs = [0, banks[0].numel()]
    stats = torch.tensor([0.25, 1.75, -0.5, 0.125], dtype=torch.float32).cuda()
    xs = [noise(2, 5 * plans[0].old + 91, 1, "cuda"), noise(1, 9 * plans[1].old + 13, 2, "cuda")]
    cuts = [plans[0].width + 3 * plans[0].old + 5, plans[1].width + 6 * plans[1].old]
    wants = [_whole(xs[0], plans[0], stats[:2]), _whole(xs[1].expand(2, -1).contiguous(), plans[1], None)]
    dst_len, cols = [2000, 6000], [100, 7]
    dst_offs = [64, 64 + 2 * dst_len[0] + 32]
    win = torch.full((dst_offs[1] + 2 * dst_len[1] + 50,), float("nan"), device="cuda")
    h_len = max(p.carry for p in plans)
    hist = torch.full((2 * 2 * 2 * h_len + 16,), float("nan"), device="cuda")
    written = torch.zeros_like(win, dtype=torch.bool)
    col = list(cols)
    state = [(0, 0, 0), (0, 0, 0)]                     # (pushed, carried start, side)
    for call in range(2):
        rows, keep = [], []
        for s, (p, x) in enumerate(zip(plans, xs)):
            P, h0, side = state[s]
            final = call == 1
            blk = x[:, P:(x.shape[1] if final else cuts[s])].contiguous()
            keep.append(blk)
            out0, n_out, nxt = p.step(P, blk.shape[1], final)
            base = 8 + s * 4 * h_len
            rows += [blk.data_ptr(), x.shape[0], blk.shape[1], P, h_len, base + side * 2 * h_len, base + (1 - side) * 2 * h_len, h0, nxt,
                     out0, n_out, x.shape[1] if final else -1, p.old, p.new, p.width, bank_offs[s], dst_offs[s], dst_len[s], col[s],
                     0 if s == 0 else -1]
            for c in range(2):
                a = dst_offs[s] + c * dst_len[s] + col[s]
                written[a:a + n_out] = True
            col[s] += n_out
            state[s] = (P + blk.shape[1], nxt, 1 - side)
        table = torch.tensor(rows, dtype=torch.int64).cuda()
        assert len(rows) == 2 * CVT_COLS
        _launch(win, table, 2, max(p.groups(6000) for p in plans), bank, hist, stats, 2, max(p.lds_floats() for p in plans))
    torch.cuda.synchronize()
    assert bool(torch.isnan(win[~written]).all())
    for s in range(2):
        got = win[dst_offs[s]:dst_offs[s] + 2 * dst_len[s]].view(2, dst_len[s])[:, cols[s]:cols[s] + wants[s].shape[1]]
        assert col[s] - cols[s] == wants[s].shape[1]
        assert_same_bits(got.contiguous(), wants[s], f"stream {s}")
    assert bool(torch.isnan(hist[:8]).all()) and bool(torch.isnan(hist[8 + 8 * h_len:]).all())


def test_wrong_tables_write_nothing_outside_the_buffers():
    """Offsets, lengths and counts far out of range: the declared capacities end before the guard regions, which stay intact."""
    plan = ConvertPlan(48000, SR)
    bank = _bank_t(plan)
    x = noise(2, 4000, 5, "cuda")
    guard = 4096
    win_all = torch.full((guard + 10000 + guard,), 7.0, device="cuda")
    hist_all = torch.full((guard + 2 * 2 * plan.carry + guard,), 7.0, device="cuda")
    win, hist = win_all[guard:guard + 10000], hist_all[guard:guard + 4 * plan.carry]
    big = 1 << 40
    good = [x.data_ptr(), 2, 4000, 0, plan.carry, 0, 2 * plan.carry, 0, plan.carry_start(4000), 0, plan.ready(4000), -1, plan.old,
            plan.new, plan.width, 0, 0, 5000, 0, -1]
    bad_values = {4: [big, -1, plan.carry + 1], 5: [big, -big, 3 * plan.carry], 6: [big, -big, 3 * plan.carry + 1],
                  7: [big, -big], 8: [-big, big], 9: [big], 10: [big], 12: [big, 0, -3], 13: [big, 0, -3], 14: [big, -1],
                  15: [big, -big, bank.numel()], 16: [big, -big, 9999], 17: [big, -1, 5001], 18: [big, -1, 4999], 19: [big, -big]}
    rows = []
    for colm, values in bad_values.items():
        for v in values:
            row = list(good)
            row[colm] = v
            rows += row
    n_rows = len(rows) // CVT_COLS
    table = torch.tensor(rows, dtype=torch.int64).cuda()
    stats = torch.tensor([0.0, 1.0], dtype=torch.float32).cuda()
    _launch(win, table, n_rows, 4, bank, hist, stats, 1, plan.lds_floats())
    torch.cuda.synchronize()
    for buf in (win_all, hist_all):
        assert bool((buf[:guard] == 7.0).all()) and bool((buf[-guard:] == 7.0).all())


# ---- 3. non-finite input samples ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pair", [(48000, 44100), (44100, 16000)])
def test_nan_and_inf_spread_as_in_the_whole_track_call(pair):
    plan = ConvertPlan(*pair)
    L = 40 * plan.old + 3
    full = noise(2, L, 9, "cuda")
    full[0, 11 * plan.old + 5] = float("nan")
    full[1, 23 * plan.old] = float("inf")
    full[1, L - 1] = float("nan")                      # the right clamp repeats it
    want = audio.convert_audio(full, pair[0], pair[1], 2)
    for seed in range(3):
        got = streamed_convert(full, pair[0], pair[1], 2, partition(L, seed, 6 * plan.old))
        assert_same_bits(got, want, f"{pair} partition {seed}")
    # the spread of one NaN sample is its klen taps, no more
    row = torch.isnan(want[0]).nonzero().flatten()
    frames = (row // plan.new).unique()
    assert len(frames) <= -(-plan.klen // plan.old) + 1


def _separate_streamed(sep, wav, sr, blocks, mean, std, **kw):
    ss = sep.separate_stream(mean, std, sr=sr, convert=True, channels=wav.shape[0], **kw)
    outs, pos = [], 0
    for b in blocks:
        blk = wav[:, pos:pos + b]
        pos += blk.shape[1]
        o = ss.push(blk)
        assert all(v.device == wav.device for v in o.values())
        assert ss.pushed_input - -(-ss.emitted * ss.plan.old // ss.plan.new) <= ss.input_latency
        outs.append(o)
    outs.append(ss.finish())
    return {k: torch.cat([o[k] for o in outs], -1) for k in outs[0]}, ss


def _converted_stats(wav, sr, channels=2):
    return _stats_for(audio.convert_audio(wav.cuda(), sr, SR, channels))


# ---- 4. Separator.separate_stream(convert=True) -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("make,mode", [(ht, "f32"), (ht, "bf16"), (hd, "f16")])
def test_separate_stream_convert_equals_separate_tensor(make, mode):
    sr = 48000
    L = 11 * sr + 321
    wav = track(L, seed=21)[:1] * 0.4                   # mono, 48 kHz, on the host
    model = make(mode) if make is ht else make(mode, segment=3)
    sep = Separator(model, device="cuda", shifts=1)
    random.seed(5)
    _, want = sep.separate_tensor(wav.clone(), sr=sr)
    state = random.getstate()
    mean, std = _converted_stats(wav, sr)
    for blocks in ([sr] * (L // sr + 1), partition(L, 4, 3 * sr)):
        random.seed(5)
        got, ss = _separate_streamed(sep, wav, sr, blocks, mean, std)
        assert random.getstate() == state
        assert ss.emitted == want["drums"].shape[-1]
        for k in want:
            assert got[k].device.type == "cpu"
            assert_same_bits(got[k], want[k], f"{mode} {k}")


def test_separate_stream_convert_with_shifts_and_length():
    sr = 48000
    L = 9 * sr + 77
    wav = track(L, seed=22, device="cuda")[:1] * 0.4
    sep = Separator(ht("f32"), device="cuda", shifts=2)
    random.seed(8)
    _, want = sep.separate_tensor(wav.clone(), sr=sr)
    state = random.getstate()
    mean, std = _converted_stats(wav, sr)
    random.seed(8)
    got, _ = _separate_streamed(sep, wav, sr, partition(L, 6, 2 * sr), mean, std, length=L)
    assert random.getstate() == state
    for k in want:
        assert_same_bits(got[k], want[k], k)
    with pytest.raises(ValueError, match="sample rate"):
        sep.separate_stream(sr=48000)


# ---- 5. a group of streams at different rates --------------------------------------------------------------------------------------------
SPEC = [(48000, 1, "cpu"), (96000, 2, "cuda"), (22050, 2, "cpu"), (SR, 2, "cuda")]       # (rate, channels, where the blocks live)


def _group_inputs(seconds=(10, 9, 11, 9)):
    wavs = []
    for i, ((sr, ch, where), sec) in enumerate(zip(SPEC, seconds)):
        n = sec * sr + 13 * i + 1
        wavs.append((track(n, seed=30 + i, device=where)[:ch] * 0.5).contiguous())
    return wavs


def _group_script(wavs, seed):
    """[("open", i) | ("push", {i: n}) | ("finish", [i])]: opens and finishes at different pushes, blocks of about a second."""
    rng = random.Random(seed)
    pos, script = [0] * len(wavs), []
    opened, done = [], []
    step = 0
    while len(done) < len(wavs):
        if len(opened) < len(wavs) and step % 2 == 0:
            script.append(("open", len(opened)))
            opened.append(len(opened))
        blocks = {}
        for i in opened:
            if i in done or pos[i] >= wavs[i].shape[1]:
                continue
            sr = SPEC[i][0]
            b = min(wavs[i].shape[1] - pos[i], rng.choice([0, 1, sr, sr, rng.randint(1, 2 * sr)]))
            blocks[i] = b
            pos[i] += b
        if blocks:
            script.append(("push", blocks))
        for i in opened:
            if i not in done and pos[i] >= wavs[i].shape[1]:
                script.append(("finish", [i]))
                done.append(i)
        step += 1
    return script


def _run_group(sep, wavs, stats, script, grouped, poison=None):
    g = sep.separate_stream_group() if grouped else None
    keys, pos, calls = {}, [0] * len(wavs), []
    for op, arg in script:
        if op == "open":
            sr, ch, _ = SPEC[arg]
            mean, std = stats[arg]
            keys[arg] = g.open(mean, std, sr=sr, channels=ch) if grouped else \
                sep.separate_stream(mean, std, sr=sr, channels=ch, convert=True)
            continue
        if op == "push":
            blocks = {}
            for i, b in arg.items():
                blocks[i] = wavs[i][:, pos[i]:pos[i] + b]
                pos[i] += b
            if grouped:
                got = g.push({keys[i]: x for i, x in blocks.items()})
                res = {i: got[keys[i]] for i in blocks}
            else:
                res = {i: keys[i].push(x) for i, x in blocks.items()}
        else:
            if grouped:
                got = g.finish([keys[i] for i in arg])
                res = {i: got[keys[i]] for i in arg}
            else:
                res = {i: keys[i].finish() for i in arg}
        calls.append(res)
    return calls


def test_group_of_converting_streams_equals_solo_streams_and_separate_tensor():
    sep = Separator(ht("f32", max_batch=4), device="cuda", shifts=0)
    wavs = _group_inputs()
    stats = [_converted_stats(w, sr) for w, (sr, _, _) in zip(wavs, SPEC)]
    script = _group_script(wavs, seed=2)
    want = _run_group(sep, wavs, stats, script, grouped=False)
    got = _run_group(sep, wavs, stats, script, grouped=True)
    pieces = [[] for _ in wavs]
    for call, (g, w) in enumerate(zip(got, want)):
        assert list(g) == list(w)
        for i in w:
            for k in w[i]:
                assert g[i][k].device == wavs[i].device and g[i][k].shape == w[i][k].shape, (call, i, k)
                assert_same_bits(g[i][k], w[i][k], f"call {call} stream {i} {k}")
            pieces[i].append(g[i])
    for i, (wav, (sr, _, _)) in enumerate(zip(wavs, SPEC)):
        _, ref = sep.separate_tensor(wav.clone(), sr=sr)
        for k in ref:
            assert_same_bits(torch.cat([p[k] for p in pieces[i]], -1), ref[k].to(wav.device), f"stream {i} {k}")


def test_a_poisoned_stream_leaves_the_others_alone():
    sep = Separator(ht("f32", max_batch=4), device="cuda", shifts=0)
    wavs = _group_inputs(seconds=(9, 9, 9, 9))
    stats = [_converted_stats(w, sr) for w, (sr, _, _) in zip(wavs, SPEC)]
    script = [("open", i) for i in range(4)]
    for sec in range(10):
        script.append(("push", {i: SPEC[i][0] for i in range(4) if sec * SPEC[i][0] < wavs[i].shape[1]}))
    script.append(("finish", [0, 1, 2, 3]))
    clean = _run_group(sep, wavs, stats, script, grouped=True)
    bad = [w.clone() for w in wavs]
    bad[1][0, 3 * SPEC[1][0] + 5] = float("nan")
    bad[1][1, 5 * SPEC[1][0]] = float("inf")
    dirty = _run_group(sep, bad, stats, script, grouped=True)
    poisoned = False
    for c, d in zip(clean, dirty):
        for i in c:
            for k in c[i]:
                if i == 1:
                    poisoned = poisoned or not bool(torch.isfinite(d[i][k]).all())
                else:
                    assert_same_bits(d[i][k], c[i][k], f"stream {i} {k}")
    assert poisoned


# ---- 6. library calls per push ------------------------------------------------------------------------------------------------------------
PER_FORWARD = {"mi_segments_gather_packed", "mi_ola_accumulate_packed"}


def max_calls_per_push(n_converting, n_plain, monkeypatch):
    m = ht("f32", max_batch=8)
    lib = _lib.load()
    counts, in_forward = Counter(), [False]
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
    sep = Separator(m, device="cuda", shifts=1)
    g = sep.separate_stream_group()
    block48, block = track(48000, seed=50)[:1].contiguous(), track(SR, seed=51)
    blocks = {g.open(0.0, 1.0, sr=48000, channels=1): block48 for _ in range(n_converting)}
    blocks.update({g.open(0.0, 1.0): block for _ in range(n_plain)})
    worst, seen = 0, Counter()
    gc.collect()
    gc.disable()                    # an earlier test's model, collected mid-push, would count its mi_model_destroy here
    try:
        for _ in range(24):
            counts.clear()
            g.push(blocks)
            other = sum(v for k, v in counts.items() if k not in PER_FORWARD and not k.endswith("_destroy"))
            assert counts["mi_segments_gather_packed"] == counts["mi_ola_accumulate_packed"]
            assert counts["mi_streams_convert_append"] == 1 and counts["mi_streams_append"] == (1 if n_plain else 0)
            worst = max(worst, other)
            seen.update(counts)
    finally:
        gc.enable()
    counts.clear()
    g.finish(list(blocks))
    monkeypatch.undo()
    return worst


def test_calls_per_push_do_not_grow_with_converting_streams(monkeypatch):
    a = max_calls_per_push(2, 0, monkeypatch)
    b = max_calls_per_push(16, 0, monkeypatch)
    assert a == b and a <= 3, (a, b)          # convert-append, emit and at most one compaction
    c = max_calls_per_push(8, 8, monkeypatch)
    assert c <= 4, c                          # plus the plain streams' append


# ---- 7. bounded device state ----------------------------------------------------------------------------------------------------------------
def test_device_bytes_do_not_grow_with_the_stream():
    """After five minutes of 1 s blocks a converter and a group of converting streams hold exactly what they held after one
    minute.  A solo converting `separate_stream` is its converter plus a plain `ModelStream`, whose window and accumulator spans
    are re-laid every push and so follow the phase of the push within a segment stride (measured on the parent's code path:
    61 852 432 bytes after 60 s, 61 905 352 after 300 s): its converter's share is constant, and the whole stays under a bound
    that does not depend on the duration: the forward buffers (max_batch segments in, max_batch x sources segments out), a
    window of at most two segments and a block, and per pass an accumulator span of at most two segments and a block."""
    sep = Separator(ht("f32", max_batch=4), device="cuda", shifts=1)
    block = (track(48000, seed=60, device="cuda")[:1] * 0.3).contiguous()
    cs = convert_audio_stream(48000, SR, 2)
    ss = sep.separate_stream(0.0, 1.0, sr=48000, channels=1, convert=True)
    g = sep.separate_stream_group()
    keys = [g.open(0.0, 1.0, sr=48000, channels=1), g.open(0.0, 1.0, sr=48000, channels=1)]
    sizes = {}
    for sec in range(5 * 60):
        cs.push(block)
        ss.push(block)
        g.push({k: block for k in keys})
        if sec + 1 in (60, 5 * 60):
            own = ss.device_bytes() - ss.stream.device_bytes()
            sizes[sec + 1] = (cs.device_bytes(), own, g.group.device_bytes())
            print(f"device bytes after {sec + 1} s: converter {sizes[sec + 1][0]}, solo stream {ss.device_bytes()} "
                  f"(converter {own}), group {sizes[sec + 1][2]}")
            SL, B, S, C_ = ss.stream.members[0].SL, 4, len(ss.sources), 2
            assert ss.device_bytes() <= 4 * (B * C_ * SL + B * S * C_ * SL + (1 + S) * C_ * (2 * SL + SR)) + own
    assert sizes[5 * 60] == sizes[60], sizes
    assert sizes[60][0] == sizes[60][1] == 4 * 2 * 2 * cs.plan.carry
    cs.finish()
    ss.finish()
    g.finish(keys)
