"""Delivery at another sample rate on the MI355X (demucs_amd/csrc/deliver_resample.hip, `Delivery(samplerate=R)` on streams and
stream groups, `audio.deliver(..., samplerate=(M, R))`): whatever the partition of the input, the concatenated frames are
`i16_pcm` (or float32) of `prevent_clip(resample_frac(value, M, R), clip)` per output bit for bit -- what a user of the reference
writes as `save_audio(julius.resample_frac(v, M, R), path, samplerate=R, clip=...)`.  The resampler is the project's
(`audio.resample_frac`, `mi_resample_frac`); every comparison with it is `torch.equal`, the value / clip / PCM steps have the exact
CPU restatement of tests/test_gpu_deliver.py (tanh, whose libm differs, through `audio.prevent_clip`, the same compiled function)."""
import ctypes as C
import gc
import random
from collections import Counter

import pytest
import torch

from demucs_amd import _lib, audio
from demucs_amd.api import Delivery, Separator
from oracle import resample_oracle as R
from test_gpu_stream import SR, _stats_for, hd, ht, track

pytestmark = pytest.mark.gpu
STEM, ADD = audio.DELIVER_STEM, audio.DELIVER_ADD


def stream_ptr():
    return C.c_void_p(_lib.current_stream_ptr())


# ---- the CPU restatement (tests/test_gpu_deliver.py) ------------------------------------------------------------------------------
def i16_pcm(v):
    return (v.clone().clamp_(-1, 1) * (2 ** 15 - 1)).short()                # demucs/audio.py:178


def value_of(x, kind, sel):
    """The tensor the reference hands to save_audio: x (S, C, n) on the CPU."""
    if kind == STEM:
        return x[sel].clone()
    other = torch.zeros_like(x[0])                                            # separate.py:208-210
    for k in range(x.shape[0]):
        if k != sel:
            other += x[k]
    return other


def clip_of(v, clip):
    if clip == 2:
        return v.clamp(-0.99, 0.99)                                           # audio.py:228
    if clip == 3:
        return audio.prevent_clip(v.cuda(), "tanh").cpu()                    # the same compiled tanh
    assert clip == 0
    return v


def frames_of(v, clip, fmt):
    w = clip_of(v, clip)
    return (i16_pcm(w) if fmt == 0 else w).t().contiguous()


def same(got, want):
    """torch.equal, with NaN equal to NaN for float frames."""
    if got.dtype.is_floating_point:
        return got.shape == want.shape and torch.equal(torch.nan_to_num(got, nan=12345.0), torch.nan_to_num(want, nan=12345.0)) and \
            torch.equal(torch.isnan(got), torch.isnan(want))
    return torch.equal(got, want)


def rate_frames(value, rate, clip, fmt):
    """The definition: frames of prevent_clip(resample_frac(value, SR, rate), clip), value (C, L) on the CPU."""
    return frames_of(audio.resample_frac(value, SR, rate), clip, fmt)


# ---- 1. the kernel alone ----------------------------------------------------------------------------------------------------------
GUARD = 64           # floats / bytes around every buffer the kernel writes
COMBOS = [(kind, clip, fmt) for kind in (STEM, ADD) for clip in (0, 2, 3) for fmt in (0, 1)]


def kernel_length(plan, channels):
    """Three full workgroup runs, two and a half frames and a few samples."""
    return 3 * audio.RATE_FRAMES * audio.rate_subruns(plan, channels) * plan.old + 5 * plan.old // 2 + 17


def launch(rows, S, C_, groups, lds, hist, hist_cap, dst, dst_cap, bank=None):
    bank = audio._BankArena.get(torch.device("cuda", torch.cuda.current_device())).buf if bank is None else bank
    table = torch.tensor([v for r in rows for v in r], dtype=torch.int64).cuda()
    _lib.check(_lib.load().mi_deliver_resample_pcm(table.data_ptr(), len(rows), groups, S, C_, bank.data_ptr(), bank.numel(),
                                                   hist.data_ptr() if hist is not None else None, hist_cap, lds, dst.data_ptr(),
                                                   dst_cap, stream_ptr()), "mi_deliver_resample_pcm")
    torch.cuda.synchronize()


def run_kernel(x, plan, specs, blocks, final_with_block, history=True):
    """Feed x (S, C, L) block by block as a stream's emitted stems; every spec (kind, sel, clip, fmt) is one row of each launch,
    with its own history and destination.  Returns per spec the concatenated frames, and checks the guards."""
    S, C_, L = x.shape
    dev = torch.device("cuda", torch.cuda.current_device())
    bank_off = audio._BankArena.get(dev).offset(plan)
    side = C_ * plan.carry
    h_len = plan.carry if history else 0
    hist = torch.full((GUARD + len(specs) * 2 * side + GUARD,), 7.5, device="cuda") if history else None
    sides, h0 = [0] * len(specs), 0
    pieces = [[] for _ in specs]
    pos = 0
    calls = [(b, False) for b in blocks]
    if final_with_block:
        calls[-1] = (calls[-1][0], True)
    else:
        calls.append((0, True))
    assert sum(b for b, _ in calls) == L
    for n_in, final in calls:
        out0, n_out, nxt = plan.step(pos, n_in, final)
        src = x[:, :, pos:pos + n_in].contiguous().cuda()
        rows, offs, at = [], [], GUARD
        for i, (kind, sel, clip, fmt) in enumerate(specs):
            at = -(-at // 16) * 16 + (4 if i % 3 == 1 else 0)              # destinations at 16-byte boundaries and at 4 mod 16
            base = GUARD + i * 2 * side
            rows.append([src.data_ptr() if n_in else 0, n_in, pos, kind, sel, clip, fmt, plan.old, plan.new, plan.width, bank_off,
                         out0, n_out, pos + n_in if final else -1, h_len, base + sides[i] * side if history else 0,
                         base + (1 - sides[i]) * side if history else 0, h0, nxt, at])
            offs.append(at)
            at += n_out * C_ * (4 if fmt else 2)
        if n_in or n_out:
            dst = torch.full((at + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
            launch(rows, S, C_, audio.rate_groups(plan, C_, n_out), audio.rate_lds_floats(plan, C_), hist,
                   hist.numel() if history else 0, dst, at)
            host = dst.cpu()
            used = torch.zeros(at + GUARD, dtype=torch.bool)
            for i, (kind, sel, clip, fmt) in enumerate(specs):
                size = n_out * C_ * (4 if fmt else 2)
                used[offs[i]:offs[i] + size] = True
                pieces[i].append(host[offs[i]:offs[i] + size].clone().view(torch.float32 if fmt else torch.int16).view(n_out, C_))
            assert bool((host[~used] == 0xA5).all())                         # nothing outside the rows' frames
            if not final:
                sides, h0 = [1 - s for s in sides], nxt
        pos += n_in
    if history:
        h = hist.cpu()
        assert bool((h[:GUARD] == 7.5).all()) and bool((h[-GUARD:] == 7.5).all())
    return [torch.cat(p, 0) for p in pieces]


def mixed_partition(L, klen):
    """Blocks of 0, 1, fewer than klen and many frames; the rest as one block."""
    head = [0, 1, klen // 3, 0, 1, klen - 1, 1, L // 3, 2, 0, klen + 5]
    assert sum(head) < L
    return head + [L - sum(head)]


@pytest.mark.parametrize("S,C_", [(4, 2), (6, 1)])
@pytest.mark.parametrize("rate", [48000, 16000])                             # 147:160 and 441:160
def test_kernel_equals_the_whole_track_chain_for_every_partition(S, C_, rate):
    plan = audio.delivery_rate_plan(SR, rate, C_)
    assert (plan.old, plan.new) == ((147, 160) if rate == 48000 else (441, 160))
    L = kernel_length(plan, C_)
    g = torch.Generator().manual_seed(1000 * S + rate)
    x = torch.rand(S, C_, L, generator=g) * 3 - 1.5                          # above 1: every clip mode acts
    specs = [(kind, (i % 2) * (S - 1), clip, fmt) for i, (kind, clip, fmt) in enumerate(COMBOS)]
    values = {(kind, sel): audio.resample_frac(value_of(x, kind, sel), SR, rate) for kind, sel, _, _ in specs}
    want = [frames_of(values[kind, sel], clip, fmt) for kind, sel, clip, fmt in specs]
    assert want[0].shape[0] == plan.final_count(L) > 3 * audio.RATE_FRAMES * audio.rate_subruns(plan, C_) * plan.new
    assert any(float(v.abs().max()) > 1.0 for v in values.values())
    runs = {
        "one final call, no history": run_kernel(x, plan, specs, [L], True, history=False),
        "one push, then the tail": run_kernel(x, plan, specs, [L], False),
        "mixed, final with a block": run_kernel(x, plan, specs, mixed_partition(L, plan.klen), True),
        "mixed, final without": run_kernel(x, plan, specs, mixed_partition(L, plan.klen)[::-1], False),
    }
    for tag, got in runs.items():
        for i, spec in enumerate(specs):
            assert got[i].dtype == want[i].dtype and torch.equal(got[i], want[i]), (tag, spec)


def test_kernel_against_the_resampling_oracle():
    """One float32 / no-clip row against oracle/resample_oracle.py at tests/test_gpu_resample.py's tolerances (4e-6 x scale: the
    float32 summation order of a ~200-tap filter; 1e-4 x scale against the float64 table)."""
    plan = audio.delivery_rate_plan(SR, 48000, 2)
    L = kernel_length(plan, 2)
    x = torch.rand(4, 2, L, generator=torch.Generator().manual_seed(3)) * 3 - 1.5
    got = run_kernel(x, plan, [(ADD, 1, 0, 1)], mixed_partition(L, plan.klen), True)[0].t()
    v = value_of(x, ADD, 1)
    want = R.resample_frac(v, SR, 48000, dtype=torch.float32)
    scale = max(1.0, float(want.abs().max()))
    assert got.shape == want.shape
    assert float((got - want).abs().max()) < 4e-6 * scale
    exact = R.resample_frac(v, SR, 48000, dtype=torch.float64)
    assert float((got.double() - exact).abs().max()) < 1e-4 * scale


# ---- 2. NaN and Inf ----------------------------------------------------------------------------------------------------------------
def test_nan_and_inf_stay_in_the_outputs_that_read_them():
    S, C_, rate = 4, 2, 48000
    plan = audio.delivery_rate_plan(SR, rate, C_)
    L = kernel_length(plan, C_)
    clean = torch.rand(S, C_, L, generator=torch.Generator().manual_seed(9)) * 3 - 1.5
    dirty = clean.clone()
    dirty[1, 0, L // 2] = float("nan")
    dirty[1, 1, L // 4] = float("inf")
    # stem 1 is read by its own row and by the sums that leave another stem out
    specs = [(STEM, 1, 2, 0), (ADD, 0, 2, 0), (ADD, 3, 0, 1), (STEM, 1, 3, 1), (STEM, 0, 2, 0), (ADD, 1, 2, 0), (ADD, 1, 3, 1), (STEM, 3, 0, 1)]
    reads = [True, True, True, True, False, False, False, False]
    blocks = mixed_partition(L, plan.klen)
    got = run_kernel(dirty, plan, specs, blocks, True)
    base = run_kernel(clean, plan, specs, blocks, True)
    for i, (kind, sel, clip, fmt) in enumerate(specs):
        v = audio.resample_frac(value_of(dirty, kind, sel), SR, rate)
        want = frames_of(v, clip, fmt)
        assert same(got[i], want), specs[i]
        if reads[i]:
            assert bool(torch.isnan(v).any()) and not same(got[i], base[i])
            if fmt == 0:
                assert bool((got[i][torch.isnan(v.t())] == 0).all())         # a NaN frame is 0 in int16
            else:
                assert bool(torch.isnan(got[i]).any())
        else:
            assert torch.equal(got[i], base[i]), specs[i]


# ---- 3. rows that break a rule write nothing ----------------------------------------------------------------------------------------
def test_rows_that_break_a_rule_write_nothing():
    """Every row here is one the kernel must reject: the destination and both history sides keep their fill."""
    S, C_ = 4, 2
    plan = audio.delivery_rate_plan(SR, 48000, C_)
    dev = torch.device("cuda", torch.cuda.current_device())
    bank_off = audio._BankArena.get(dev).offset(plan)
    bank = audio._BankArena.get(dev).buf
    n_in = 2000
    x = (torch.rand(S, C_, n_in, generator=torch.Generator().manual_seed(4)) * 3 - 1.5).cuda()
    side = C_ * plan.carry
    hist = torch.full((GUARD + 2 * side + GUARD,), 7.5, device="cuda")
    hist_cap = hist.numel()
    out0, n_out, nxt = plan.step(0, n_in, False)
    assert n_out > 0 and nxt >= 0
    size = n_out * C_ * 2
    room = GUARD + size + GUARD
    dst = torch.full((room + 4096,), 0xA5, dtype=torch.uint8, device="cuda")

    def row(**kw):
        r = dict(src=x.data_ptr(), n_in=n_in, before=0, kind=STEM, sel=1, clip=2, fmt=0, old=plan.old, new=plan.new,
                 width=plan.width, bank_off=bank_off, out0=out0, n_out=n_out, total=-1, h_len=plan.carry, h_rd=GUARD,
                 h_wr=GUARD + side, h0=0, h1=nxt, dst_off=GUARD)
        assert set(kw) <= set(r)
        r.update(kw)
        return list(r.values())

    bad = [
        row(dst_off=room - size + 4),                    # the frames leave dst_cap
        row(fmt=1, dst_off=room - 2 * size + 4),         # float frames are twice as long and leave it too
        row(dst_off=room), row(dst_off=-16),
        row(n_out=1 << 60),                              # a count whose bytes overflow
        row(dst_off=GUARD + 2), row(dst_off=GUARD + 6),  # no multiple of 4
        row(h_rd=-1), row(h_rd=hist_cap - side + 1), row(h_wr=-4), row(h_wr=hist_cap - side + 1), row(h_len=hist_cap + 1),
        row(h_wr=GUARD + side - 1),                      # the sides overlap
        row(h_len=0), row(h_len=-1),                     # no history, though the row carries values over
        row(bank_off=-1), row(bank_off=bank.numel() - plan.klen * plan.new + 1), row(bank_off=1 << 61),
        row(kind=2), row(kind=-1), row(kind=3),          # "minus" does not exist here
        row(sel=S), row(sel=-1),
        row(clip=1), row(clip=4), row(clip=-1),          # nor does "rescale"
        row(fmt=2), row(fmt=-1),
        row(new=0), row(new=(1 << 24) + 1), row(new=-160),
        row(width=0), row(width=-26), row(width=1 << 40),
        row(old=0), row(old=1 << 40),
        row(old=1100),                                   # two channels of 8 such frames do not fit the staging area
        row(out0=out0 + 1), row(out0=-plan.new),
        row(n_in=-1), row(before=-1), row(src=0),
        row(total=n_in + 1),                             # a final call whose total is not before + n_in
    ]
    assert audio.RATE_FRAMES * 1100 * C_ > audio.RATE_LDS_FLOATS
    for at in range(0, len(bad), 16):
        launch(bad[at:at + 16], S, C_, 4, audio.RATE_LDS_FLOATS, hist, hist_cap, dst, room, bank=bank)
    assert bool((dst.cpu() == 0xA5).all())
    assert bool((hist.cpu() == 7.5).all())
    # and the row they were derived from is served
    launch([row()], S, C_, audio.rate_groups(plan, C_, n_out), audio.rate_lds_floats(plan, C_), hist, hist_cap, dst, room, bank=bank)
    host, h = dst.cpu(), hist.cpu()
    # a ready frame reads nothing behind the block: the same chain on the block alone
    want = frames_of(audio.resample_frac(x[1].cpu(), SR, 48000)[:, :n_out], 2, 0)
    assert torch.equal(host[GUARD:GUARD + size].clone().view(torch.int16).view(n_out, C_), want)
    assert bool((host[:GUARD] == 0xA5).all()) and bool((host[GUARD + size:] == 0xA5).all())
    kept = h[GUARD + side:GUARD + 2 * side].view(C_, plan.carry)[:, :n_in - nxt]
    assert torch.equal(kept, x[1].cpu()[:, nxt:]) and bool((h[:GUARD + side] == 7.5).all()) and bool((h[-GUARD:] == 7.5).all())


# ---- 4. solo streams -------------------------------------------------------------------------------------------------------------------
def blocks_for(length, seed, max_block):
    g = random.Random(seed)
    out, total = [], 0
    while total < length:
        b = g.choice([0, 1, g.randint(1, SR // 10), g.randint(SR // 2, max_block)])
        out.append(b)
        total += b
    return out


def run_stream(sep, mix, blocks, deliver, seed=7, mean=0.02, std=0.5):
    """Per call the result and (emitted, delivered) after it."""
    random.seed(seed)
    ss = sep.separate_stream(mean, std, deliver=deliver)
    outs, marks, pos = [], [], 0
    for b in blocks:
        blk = mix[:, pos:pos + b]
        pos += blk.shape[1]
        o = ss.push(blk)
        for v in o.values():
            assert v.device == mix.device
        outs.append(o)
        marks.append((ss.emitted, ss.delivered))
    outs.append(ss.finish())
    marks.append((ss.emitted, ss.delivered))
    return outs, marks, random.getstate(), ss


def restated(stems, sources, dl):
    """`dl`'s frames from the float stems (S, C, L) of the same stream run without delivery."""
    x = stems.cpu()
    return {name: rate_frames(value_of(x, kind, sel), dl.samplerate, dl.clip_code, 0 if dl.fmt == "i16" else 1)
            for name, kind, sel in dl.outputs(sources)}


def check_resampling_stream(model, length, where, deliveries, seed):
    mix = track(length, seed=seed, device=where)
    blocks = blocks_for(length, seed, 3 * SR)
    assert 0 in blocks and 1 in blocks
    sep = Separator(model, device="cuda", shifts=1)
    plain, plain_marks, state, _ = run_stream(sep, mix, blocks, None, seed=seed)
    stems = torch.stack([torch.cat([o[k] for o in plain], -1) for k in model.sources])
    for dl in deliveries:
        plan = audio.ConvertPlan(SR, dl.samplerate)
        outs, marks, got_state, ss = run_stream(sep, mix, blocks, dl, seed=seed)
        assert got_state == state
        assert ss.output_hold == plan.hold
        want = restated(stems, model.sources, dl)
        assert all(list(o) == list(want) for o in outs)
        before = (0, 0)
        for o, (emitted, delivered), (p_emitted, _) in zip(outs[:-1], marks, plain_marks):
            assert emitted == p_emitted                                        # the model's stream is the same stream
            m = plan.ready(emitted) - plan.ready(before[0])
            assert all(v.shape == (m, 2) for v in o.values()) and delivered == before[1] + m == plan.ready(emitted)
            assert 0 <= plan.new * emitted // plan.old - delivered <= ss.output_hold
            before = (emitted, delivered)
        assert marks[-1] == (length, plan.final_count(length))
        for k in want:
            got = torch.cat([o[k] for o in outs], 0)
            assert got.device == mix.device and got.dtype == want[k].dtype and got.shape == (plan.final_count(length), 2)
            assert torch.equal(got.cpu(), want[k]), (dl, k)


DELIVERIES = [Delivery("vocals", samplerate=48000), Delivery(samplerate=16000, clip="tanh", fmt="f32"),
              Delivery("drums", "none", samplerate=48000)]


@pytest.mark.parametrize("where", ["cpu", "cuda"])
def test_hdemucs_stream_delivers_the_resampled_frames(where):
    m = hd("f32", max_batch=2, channels=4, segment=3)
    check_resampling_stream(m, 9 * SR + 777, where, DELIVERIES, seed=31 if where == "cpu" else 32)


def test_htdemucs_stream_delivers_the_resampled_frames():
    check_resampling_stream(ht("f32"), 12 * SR + 5, "cpu", DELIVERIES[:1], seed=33)


# ---- 5. the whole track ---------------------------------------------------------------------------------------------------------------
CLIPS = ["rescale", "clamp", "tanh", None]


@pytest.fixture(scope="module")
def separated():
    g = torch.Generator().manual_seed(11)
    block = (torch.randn(4, 2, 3 * SR, generator=g) * 0.45).cuda()       # peaks above 1: every clip mode acts
    origin = (torch.randn(2, 3 * SR, generator=g) * 0.6).cuda()
    names = ["drums", "bass", "other", "vocals"]
    return origin, block, dict(zip(names, block))


def composed(origin, stems, stem, method, clip, fmt, rates):
    """The public functions one at a time: two_stems, resample_frac, prevent_clip, i16_pcm."""
    outs = dict(stems) if stem is None else audio.two_stems(origin, stems, stem, method)
    want = {}
    for name, v in outs.items():
        w = audio.prevent_clip(audio.resample_frac(v, *rates), clip).cpu()
        want[name] = (i16_pcm(w) if fmt == "i16" else w).t().contiguous()
    return want


@pytest.mark.parametrize("fmt", ["i16", "f32"])
@pytest.mark.parametrize("stem,method", [(None, "add"), ("vocals", "add"), ("vocals", "minus"), ("bass", "none")])
def test_deliver_at_another_rate_equals_the_composed_chain(separated, stem, method, fmt):
    origin, block, stems = separated
    rates = (SR, 48000)
    n = audio.ConvertPlan(*rates).final_count(3 * SR)
    host_stems = {k: v.cpu() for k, v in stems.items()}
    for clip in CLIPS:
        want = composed(origin, stems, stem, method, clip, fmt, rates)
        got = audio.deliver(origin, stems, stem=stem, other_method=method, clip=clip, fmt=fmt, samplerate=rates)
        assert list(got) == list(want) == [name for name, _, _ in audio.delivery_outputs(list(stems), stem, method)]
        for k in want:
            assert got[k].is_cuda and got[k].shape == (n, 2) and torch.equal(got[k].cpu(), want[k]), (clip, k)
        on_host = audio.deliver(origin.cpu(), host_stems, stem=stem, other_method=method, clip=clip, fmt=fmt, samplerate=rates)
        assert list(on_host) == list(want)
        for k in want:
            assert on_host[k].device.type == "cpu" and torch.equal(on_host[k], want[k]), (clip, k)
    # equal rates: today's call
    a = audio.deliver(origin, stems, stem=stem, other_method=method, fmt=fmt, samplerate=(SR, SR))
    b = audio.deliver(origin, stems, stem=stem, other_method=method, fmt=fmt)
    assert list(a) == list(b) and all(torch.equal(a[k], b[k]) for k in a)


# ---- 6. the round trip: a 48 kHz feed gets its stems back at 48 kHz ------------------------------------------------------------------
def test_round_trip_of_a_48_khz_feed():
    sr = 48000
    N = 7 * sr + 321
    wav = track(N, seed=41) * 0.4                                             # stereo, 48 kHz, on the host
    sep = Separator(hd("f32", max_batch=2, channels=4, segment=3), device="cuda", shifts=1)
    random.seed(5)
    origin, stems = sep.separate_tensor(wav.clone(), sr=sr)
    state = random.getstate()
    want = audio.deliver(origin, stems, "vocals", "add", clip="clamp", samplerate=(SR, sr))
    mean, std = _stats_for(audio.convert_audio(wav.cuda(), sr, SR, 2))
    down, up = audio.ConvertPlan(sr, SR), audio.ConvertPlan(SR, sr)
    total = up.final_count(down.final_count(N))
    assert total == (up.new * (down.new * N // down.old)) // up.old and 0 <= N - total <= 2
    for length in (N, None):
        random.seed(5)
        ss = sep.separate_stream(mean, std, sr=sr, length=length, convert=True, deliver=Delivery("vocals", samplerate=sr))
        outs = [ss.push(wav[:, i:i + sr + 11]) for i in range(0, N, sr + 11)] + [ss.finish()]
        assert random.getstate() == state
        assert list(outs[0]) == list(want) == ["vocals", "no_vocals"]
        for k in want:
            got = torch.cat([o[k] for o in outs], 0)
            assert got.device.type == "cpu" and got.dtype == torch.int16 and got.shape == (total, 2)
            assert torch.equal(got, want[k]), k
        assert ss.delivered == total


# ---- 7. groups ---------------------------------------------------------------------------------------------------------------------------
def group_script(lengths, seed):
    """[{stream: block length}] until every stream is pushed; blocks of 0 and 1 sample among them.  Stream i joins at call i."""
    g = random.Random(seed)
    pos, script = [0] * len(lengths), []
    while any(p < n for p, n in zip(pos, lengths)):
        call = {}
        for i, n in enumerate(lengths):
            if len(script) >= i and pos[i] < n and g.random() < (1.0 if i == 0 else 0.8):
                b = min(n - pos[i], g.choice([0, 1, g.randint(1, SR // 10), g.randint(SR // 2, 2 * SR)]))
                call[i] = b
                pos[i] += b
        if call:
            script.append(call)
    return script


def run_group(sep, mixes, deliveries, script, grouped, seed=5):
    """[(operation, {stream: result})]: stream i is opened at call i and finished on the call that pushes its last sample (a
    staggered script); solo streams (grouped=False) are opened, pushed and finished in the same order."""
    random.seed(seed)
    g = sep.separate_stream_group() if grouped else None
    keys, pos, calls = {}, [0] * len(mixes), []
    for c, call in enumerate(script):
        if c < len(mixes):
            keys[c] = g.open(0.02, 0.5, deliver=deliveries[c]) if grouped else sep.separate_stream(0.02, 0.5, deliver=deliveries[c])
        blocks = {}
        for i, b in call.items():
            blocks[i] = mixes[i][:, pos[i]:pos[i] + b]
            pos[i] += b
        if grouped:
            got = g.push({keys[i]: x for i, x in blocks.items()})
            res = {i: got[keys[i]] for i in blocks}
        else:
            res = {i: keys[i].push(x) for i, x in blocks.items()}
        calls.append(("push", res))
        done = [i for i in keys if keys[i] is not None and pos[i] >= mixes[i].shape[1]]
        if done:
            if grouped:
                got = g.finish([keys[i] for i in done])
                calls.append(("finish", {i: got[keys[i]] for i in done}))
            else:
                calls.append(("finish", {i: keys[i].finish() for i in done}))
            for i in done:
                keys[i] = None
    assert all(k is None for k in keys.values()) and len(keys) == len(mixes)
    return calls, random.getstate()


def assert_calls_equal(got, want, only=None):
    assert len(got) == len(want)
    for c, ((gop, g), (wop, w)) in enumerate(zip(got, want)):
        assert gop == wop and list(g) == list(w)
        for i in w:
            if only is not None and i not in only:
                continue
            if not isinstance(w[i], dict):
                w_i, g_i = {"stems": w[i]}, {"stems": g[i]}
            else:
                w_i, g_i = w[i], g[i]
            assert list(g_i) == list(w_i)
            for k in w_i:
                assert g_i[k].device == w_i[k].device and g_i[k].dtype == w_i[k].dtype
                assert same(g_i[k], w_i[k]), (c, i, k)


GROUP_DELIVERIES = [Delivery("vocals", samplerate=48000), Delivery(samplerate=16000, clip="tanh", fmt="f32"), Delivery("bass"), None]


def group_mixes(device_of):
    lengths = [9 * SR + 3, 10 * SR + 777, 11 * SR + 1, 9 * SR + 40]
    return [track(n, seed=80 + i, device=w) for i, (n, w) in enumerate(zip(lengths, device_of))], lengths


def test_group_streams_equal_their_solo_streams():
    m = hd("f32", max_batch=3, channels=4, segment=3)
    sep = Separator(m, device="cuda", shifts=1)
    mixes, lengths = group_mixes(["cpu", "cuda", "cpu", "cpu"])
    script = group_script(lengths, 6)
    want, ws = run_group(sep, mixes, GROUP_DELIVERIES, script, grouped=False)
    got, gs = run_group(sep, mixes, GROUP_DELIVERIES, script, grouped=True)
    assert gs == ws
    assert_calls_equal(got, want)
    for i, rate in ((0, 48000), (1, 16000)):
        n = sum(next(iter(res[i].values())).shape[0] for _, res in got if i in res)
        assert n == audio.ConvertPlan(SR, rate).final_count(lengths[i])
    assert [op for op, _ in got].count("finish") >= 2                          # streams ended on different calls


def test_a_nan_block_stays_in_its_stream():
    m = hd("f32", max_batch=3, channels=4, segment=3)
    sep = Separator(m, device="cuda", shifts=1)
    mixes, lengths = group_mixes(["cpu"] * 4)
    script = group_script(lengths, 8)
    clean, _ = run_group(sep, mixes, GROUP_DELIVERIES, script, grouped=True)
    bad = [x.clone() for x in mixes]
    bad[0][:, 2 * SR:3 * SR] = float("nan")
    dirty, _ = run_group(sep, bad, GROUP_DELIVERIES, script, grouped=True)
    assert_calls_equal(dirty, clean, only={1, 2, 3})
    assert any(not same(d[0]["vocals"], c[0]["vocals"]) for (_, d), (_, c) in zip(dirty, clean) if 0 in d)


# ---- 8. work per push ------------------------------------------------------------------------------------------------------------------
PER_FORWARD = {"mi_segments_gather_packed", "mi_ola_accumulate_packed"}


def max_calls_per_push(deliveries, monkeypatch):
    """tests/test_gpu_deliver.py's count: library calls per push outside the forwards, the worst of 24 pushes."""
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
    block = track(SR, seed=50)
    random.seed(9)                  # the same shift offsets, so the same samples become final on the same push in every run
    g = Separator(m, device="cuda", shifts=1).separate_stream_group()
    keys = [g.open(0.0, 1.0, deliver=d) for d in deliveries]
    worst, most = 0, Counter()
    gc.collect()
    gc.disable()                    # an earlier test's model, collected mid-push, would count its mi_model_destroy here
    try:
        for _ in range(24):
            counts.clear()
            g.push({k: block for k in keys})
            worst = max(worst, sum(v for k, v in counts.items() if k not in PER_FORWARD and not k.endswith("_destroy")))
            for k in ("mi_deliver_pcm", "mi_deliver_resample_pcm"):
                most[k] = max(most[k], counts[k])
    finally:
        gc.enable()
    counts.clear()
    g.finish(keys)
    monkeypatch.undo()
    return worst, most


def test_a_push_is_one_more_call_whatever_the_number_of_resampling_streams(monkeypatch):
    """The new launch takes `mi_deliver_pcm`'s place for the streams that resample and plain delivering streams keep theirs, so
    "one more than with samplerate=None" is a group that holds both kinds: n resampling streams beside one plain delivering
    stream, against the same group with `samplerate=None` everywhere.  A group of resampling streams alone has as many calls as
    the plain group."""
    def group(n, rate):
        return [Delivery("vocals", samplerate=rate if i % 2 else (rate and 16000)) for i in range(n)] + [Delivery("vocals")]

    a, ma = max_calls_per_push(group(2, 48000), monkeypatch)
    b, mb = max_calls_per_push(group(8, 48000), monkeypatch)
    c, mc = max_calls_per_push(group(2, None), monkeypatch)
    assert a == b == c + 1, (a, b, c)
    assert ma["mi_deliver_resample_pcm"] == mb["mi_deliver_resample_pcm"] == 1 and ma["mi_deliver_pcm"] == mb["mi_deliver_pcm"] == 1
    assert mc["mi_deliver_resample_pcm"] == 0 and mc["mi_deliver_pcm"] == 1
    d, md = max_calls_per_push(group(2, 48000)[:2], monkeypatch)
    assert d == c and md["mi_deliver_pcm"] == 0 and md["mi_deliver_resample_pcm"] == 1


def test_device_bytes_follow_the_open_streams_not_their_duration():
    """One long stream, solo and in a group, in blocks of a third of the segment stride (0.75 s): after 20.25 s it holds what it held
    after 11.25 s, the same phase of the stride (a solo stream's window and accumulator spans follow that phase, see
    tests/test_gpu_convert_stream.py).  The resampler's share is the two-sided history alone."""
    m = hd("f32", max_batch=2, channels=4, segment=3)
    sep = Separator(m, device="cuda", shifts=1)
    dl = Delivery("vocals", samplerate=48000)
    plan = audio.ConvertPlan(SR, 48000)
    random.seed(2)
    ss = sep.separate_stream(0.0, 1.0, deliver=dl)
    g = sep.separate_stream_group()
    key = g.open(0.0, 1.0, deliver=dl)
    stride = ss.stream.members[0].stride
    assert stride % 3 == 0
    block = track(stride // 3, seed=90)
    sizes = {}
    for push in range(1, 28):
        ss.push(block)
        g.push({key: block})
        if push in (15, 27):
            assert push * block.shape[1] >= (10 if push == 15 else 20) * SR
            sizes[push] = (ss.stream.device_bytes(), g.group.device_bytes())
            print(f"device bytes after {push * block.shape[1] / SR:.2f} s: solo {sizes[push][0]}, group {sizes[push][1]}")
    assert sizes[27] == sizes[15], sizes
    share = 4 * 2 * 2 * 2 * plan.carry                                        # outputs x sides x channels x (klen - 1) floats
    assert ss.stream._exec.rate_hist.numel() * 4 == share and g.group._exec.hist.numel() * 4 >= share
    ss.finish()
    g.finish([key])
    key2 = g.open(0.0, 1.0, deliver=dl)                                       # a finished stream's region is used again
    g.push({key2: block})
    assert g.group._exec.hist.numel() * 4 == max(share, 4 * 4096) and g.group._exec.hist_used * 4 == share
    g.finish([key2])
