"""Delivery on the MI355X (demucs_amd/csrc/deliver.hip, `audio.deliver`, `Delivery` on streams and stream groups): the frames are
bit for bit what the reference's save path computes on the CPU -- the `--two-stems` value (demucs/separate.py:195-210),
`prevent_clip` (demucs/audio.py:218-234), `i16_pcm` (audio.py:178), channels interleaved -- for every output of a call in one
launch.  Every comparison is `torch.equal`: each step is one float32 operation with an exact CPU restatement (tanh, whose libm
differs, is compared with the project's own `audio.prevent_clip`, the same compiled device function)."""
import ctypes as C
import gc
import itertools
import random
from collections import Counter

import pytest
import torch

from demucs_amd import _lib, audio
from demucs_amd.api import Delivery, Separator
from demucs_amd.apply import apply_model_stream
from test_gpu_stream import SR, hd, ht, track

pytestmark = pytest.mark.gpu
COLS = audio.DELIVER_COLS
PLANTED = [1.0, -1.0, 0.99, -0.99, 0.99997, 0.5, -0.5, -0.0, 1e-6, float("inf"), -float("inf")]
PLANTED_I16 = [32767, -32767, 32439, -32439, 32766, 16383, -16383, 0, 0, 32767, -32767]     # i16_pcm of PLANTED on the CPU


def stream_ptr():
    return C.c_void_p(_lib.current_stream_ptr())


# ---- the CPU restatement ------------------------------------------------------------------------------------------------------
def i16_pcm(v):
    return (v.clone().clamp_(-1, 1) * (2 ** 15 - 1)).short()                # demucs/audio.py:178


def value_of(x, origin, kind, sel):
    """The tensor the reference hands to save_audio: x (S, C, n), origin (C, n), on the CPU."""
    if kind == 0:
        return x[sel].clone()
    if kind == 2:
        return origin - x[sel]                                                # separate.py:197
    other = torch.zeros_like(x[0])                                            # separate.py:208-210
    for k in range(x.shape[0]):
        if k != sel:
            other += x[k]
    return other


def clip_of(v, clip):
    if clip == 1:
        return v / max(1.01 * v.abs().max(), 1)                               # audio.py:226
    if clip == 2:
        return v.clamp(-0.99, 0.99)                                           # audio.py:228
    if clip == 3:
        return audio.prevent_clip(v.cuda(), "tanh").cpu()                    # parent code, the same compiled tanh
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


def test_the_restatement_on_the_planted_values():
    assert i16_pcm(torch.tensor(PLANTED)).tolist() == PLANTED_I16
    assert i16_pcm(torch.tensor([float("nan")])).tolist() == [0]


# ---- 1. the kernel alone -------------------------------------------------------------------------------------------------------
NS = [1, 3, 4, 1023, 1025, 4099, 2048, 4100]          # the last two: multiples of 4 over several blocks, the 16-byte load path


def noise(S, C_, n, seed, nan_at=None, planted=PLANTED):
    g = torch.Generator().manual_seed(seed)
    x = (torch.rand(S, C_, n, generator=g) * 3 - 1.5)
    o = (torch.rand(C_, n, generator=g) * 3 - 1.5)
    k = min(n, len(planted))
    x[:, :, :k] = torch.tensor(planted[:k])
    if n > 40:
        o[:, 20:20 + len(planted)] = torch.tensor(planted)
    if nan_at is not None:
        x[nan_at[0], nan_at[1], nan_at[2]] = float("nan")
    return x, o


def launch(rows, S, C_, n_peaks, dst, max_n, dst_cap=None, peaks=None):
    lib = _lib.load()
    table = torch.tensor([v for r in rows for v in r], dtype=torch.int64).cuda()
    cap = dst.numel() if dst_cap is None else dst_cap
    if n_peaks:
        _lib.check(lib.mi_deliver_peaks(table.data_ptr(), len(rows), max_n, S, C_, peaks.data_ptr(), n_peaks, cap, stream_ptr()),
                   "mi_deliver_peaks")
    _lib.check(lib.mi_deliver_pcm(table.data_ptr(), len(rows), max_n, S, C_, peaks.data_ptr() if n_peaks else None, n_peaks,
                                  dst.data_ptr(), cap, stream_ptr()), "mi_deliver_pcm")
    torch.cuda.synchronize()


@pytest.mark.parametrize("S,C_", [(4, 1), (4, 2), (6, 1), (6, 2)])
def test_kernel_equals_the_cpu_restatement(S, C_):
    """Every (n, kind, clip, format) as one row of ONE launch: rows of different n, SEL first and last, destinations at 16-byte
    boundaries and at 4 mod 16, one source offset by a float (no 16-byte loads), a NaN row among clean ones."""
    data = {}
    for i, n in enumerate(NS):
        data[n, "all"] = noise(S, C_, n, seed=100 * S + 10 * C_ + i)
    # the planted infinities make every peak infinite: two sets without them, so that "rescale" divides by a finite peak too
    data[1023, "finite"] = noise(S, C_, 1023, seed=5, planted=PLANTED[:9])
    data[4100, "finite"] = noise(S, C_, 4100, seed=6, planted=PLANTED[:9])
    data[1025, "nan"] = noise(S, C_, 1025, seed=7, nan_at=(0, C_ - 1, 777), planted=PLANTED[:9])
    data[2048, "nan"] = noise(S, C_, 2048, seed=8, nan_at=(S - 1, 0, 2047), planted=PLANTED[:9])
    dev, keep = {}, []
    for key, (x, o) in data.items():
        for shift in (0, 1):                         # shift 1: the block starts one float behind a 16-byte boundary
            bx = torch.zeros(x.numel() + 4, device="cuda")
            bo = torch.zeros(o.numel() + 4, device="cuda")
            bx[shift:shift + x.numel()] = x.reshape(-1).cuda()
            bo[shift:shift + o.numel()] = o.reshape(-1).cuda()
            keep += [bx, bo]
            dev[key, shift] = (bx.data_ptr() + 4 * shift, bo.data_ptr() + 4 * shift)
    specs, rows, at = [], [], 0
    combos = itertools.product(data, (0, 1, 2), (0, 1, 2, 3), (0, 1))
    for i, ((n, tag), kind, clip, fmt) in enumerate(combos):
        sel = 0 if (i % 7) % 2 == 0 else S - 1
        shift = 1 if i % 5 == 3 else 0
        at = -(-at // 16) * 16 + (4 if i % 3 == 1 else 0)
        src, org = dev[(n, tag), shift]
        rows.append([src, org if kind == 2 else 0, n, kind, sel, clip, i, fmt, at])
        specs.append(((n, tag), kind, sel, clip, fmt, at))
        at += n * C_ * (4 if fmt else 2)
    assert any(r[8] % 16 == 4 for r in rows) and any(r[0] % 16 == 4 for r in rows)
    dst = torch.full((at + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    peaks = torch.full((len(rows) + 2,), -1, dtype=torch.int32, device="cuda")
    launch(rows, S, C_, len(rows), dst, max(NS), dst_cap=at, peaks=peaks)
    host, pk = dst.cpu(), peaks.cpu()
    assert pk[-2:].tolist() == [-1, -1] and bool((host[at:] == 0xA5).all())
    values = {}
    nan_rows = 0
    for i, (key, kind, sel, clip, fmt, off) in enumerate(specs):
        n = key[0]
        x, o = data[key]
        if (key, kind, sel) not in values:
            values[key, kind, sel] = value_of(x, o, kind, sel)
        v = values[key, kind, sel]
        want = frames_of(v, clip, fmt)
        size = n * C_ * (4 if fmt else 2)
        got = host[off:off + size].clone().view(torch.float32 if fmt else torch.int16).view(n, C_)
        assert same(got, want), (i, key, kind, sel, clip, fmt, off)
        if fmt == 0 and kind == 0 and clip == 0:
            k = min(n, len(PLANTED) if key[1] == "all" else 9)
            assert got[:k, 0].tolist() == PLANTED_I16[:k]
            assert bool((got[torch.isnan(v.t())] == 0).all())                  # a NaN is 0 in int16
        if clip == 1:                                 # the row's own peak, NaN when the row holds one; other slots stay 0
            peak = v.abs().max()
            got_peak = pk[i:i + 1].view(torch.float32)[0]
            assert same(got_peak.reshape(1), peak.reshape(1)), (i, float(got_peak), float(peak))
            nan_rows += int(torch.isnan(peak))
            if torch.isnan(peak):
                assert bool(torch.isnan(want).all()) if fmt else bool((want == 0).all())
        else:
            assert int(pk[i]) == 0
    assert 0 < nan_rows < sum(1 for s in specs if s[3] == 1) // 2               # only the rows that hold the NaN
    finite = [i for i, s in enumerate(specs) if s[3] == 1 and s[0][1] == "finite"]
    assert finite and all(1.0 <= float(pk[i:i + 1].view(torch.float32)) < 16.0 for i in finite)


def test_rows_that_break_a_rule_write_nothing():
    S, C_, n = 4, 2, 1025
    x, o = noise(S, C_, n, seed=3)
    xd, od = x.cuda(), o.cuda()
    size = n * C_ * 2
    room = 3 * (size + 64)
    dst = torch.full((room + 4096,), 0xA5, dtype=torch.uint8, device="cuda")
    good = [xd.data_ptr(), 0, n, 0, 1, 2, 0, 0, 16]
    bad = [
        [xd.data_ptr(), 0, n, 0, 1, 2, 0, 0, room - size + 4],           # the span leaves dst_cap
        [xd.data_ptr(), 0, n, 0, 1, 2, 0, 1, room - 2 * size + 4],       # float frames: twice as long, leave it too
        [xd.data_ptr(), 0, n, 0, 1, 2, 0, 0, room],                      # starts at the end
        [xd.data_ptr(), 0, n, 0, 1, 2, 0, 0, -16],
        [xd.data_ptr(), 0, 1 << 62, 0, 1, 2, 0, 0, 16],                  # a length whose byte count overflows
        [xd.data_ptr(), 0, n, 0, 1, 2, 0, 0, size + 64 + 2],             # DST_OFF no multiple of 4
        [xd.data_ptr(), 0, n, 0, 1, 2, 0, 0, size + 64 + 6],
        [xd.data_ptr(), 0, n, 0, S, 2, 0, 0, size + 64],                 # SEL
        [xd.data_ptr(), 0, n, 1, -1, 2, 0, 0, size + 64],
        [xd.data_ptr(), 0, n, 0, 1, 1, 3, 0, size + 64],                 # PEAK (three slots)
        [xd.data_ptr(), 0, n, 0, 1, 1, -1, 0, size + 64],
        [xd.data_ptr(), 0, n, 3, 1, 2, 0, 0, size + 64],                 # KIND
        [xd.data_ptr(), 0, n, 0, 1, 4, 0, 0, size + 64],                 # CLIP
        [xd.data_ptr(), 0, n, 0, 1, 2, 0, 2, size + 64],                 # FMT
        [xd.data_ptr(), 0, n, 2, 1, 2, 0, 0, size + 64],                 # "minus" without the mix
        [0, od.data_ptr(), n, 0, 1, 2, 0, 0, size + 64],                 # no stems
        [xd.data_ptr(), 0, 0, 0, 1, 2, 0, 0, size + 64],
    ]
    peaks = torch.full((5,), -1, dtype=torch.int32, device="cuda")
    rows = bad[:8] + [good] + bad[8:]
    launch(rows, S, C_, 3, dst, n, dst_cap=room, peaks=peaks)
    host = dst.cpu()
    want = frames_of(x[1], 2, 0)
    assert torch.equal(host[16:16 + size].clone().view(torch.int16).view(n, C_), want)
    assert bool((host[:16] == 0xA5).all()) and bool((host[16 + size:] == 0xA5).all())
    assert peaks.cpu().tolist() == [0, 0, 0, -1, -1]                     # zeroed, no row reduced into them, none behind them


# ---- 2. audio.deliver ------------------------------------------------------------------------------------------------------------
CLIPS = ["rescale", "clamp", "tanh", None]


@pytest.fixture(scope="module")
def separated():
    g = torch.Generator().manual_seed(11)
    block = (torch.randn(4, 2, 3 * SR, generator=g) * 0.45).cuda()       # peaks above 1: every clip mode acts
    origin = (torch.randn(2, 3 * SR, generator=g) * 0.6).cuda()
    names = ["drums", "bass", "other", "vocals"]
    return origin, block, dict(zip(names, block))


def expected(origin, stems, stem, method, clip, fmt):
    outs = dict(stems) if stem is None else audio.two_stems(origin, stems, stem, method)
    want = {}
    for name, v in outs.items():
        w = audio.prevent_clip(v, clip).cpu()
        want[name] = (i16_pcm(w) if fmt == "i16" else w).t().contiguous()
    return want


@pytest.mark.parametrize("fmt", ["i16", "f32"])
@pytest.mark.parametrize("stem,method", [(None, "add"), ("vocals", "add"), ("vocals", "minus"), ("bass", "none"), ("drums", "add")])
def test_deliver_equals_the_one_call_per_output_chain(separated, stem, method, fmt):
    origin, block, stems = separated
    assert float(block.abs().max()) > 1.0
    host_stems = {k: v.cpu() for k, v in stems.items()}
    for clip in CLIPS:
        want = expected(origin, stems, stem, method, clip, fmt)
        got = audio.deliver(origin, stems, stem=stem, other_method=method, clip=clip, fmt=fmt)
        assert list(got) == list(want) == [n for n, _, _ in audio.delivery_outputs(list(stems), stem, method)]
        for k in want:
            assert got[k].is_cuda and got[k].shape == (3 * SR, 2) and torch.equal(got[k].cpu(), want[k]), (clip, k)
        on_host = audio.deliver(origin.cpu(), host_stems, stem=stem, other_method=method, clip=clip, fmt=fmt)
        assert list(on_host) == list(want)
        for k in want:
            assert on_host[k].device.type == "cpu" and torch.equal(on_host[k], want[k]), (clip, k)


def test_deliver_is_one_launch_per_track_and_reads_the_stems_in_place(separated, monkeypatch):
    origin, block, stems = separated
    assert audio._stems_block(list(stems.values()), block.device).data_ptr() == block.data_ptr()
    apart = [v.clone() for v in stems.values()]
    assert torch.equal(audio._stems_block(apart, block.device), block)
    lib = _lib.load()
    counts = Counter()
    for name in _lib.SIGNATURES:
        real = getattr(lib, name)

        def wrapped(*args, _real=real, _name=name):
            counts[_name] += 1
            return _real(*args)

        monkeypatch.setattr(lib, name, wrapped)
    audio.deliver(origin, stems, stem="vocals", other_method="minus", clip="rescale")
    assert counts["mi_deliver_peaks"] == 1 and counts["mi_deliver_pcm"] == 1
    assert counts["mi_prevent_clip"] == 0 and counts["mi_two_stems"] == 0
    counts.clear()
    audio.deliver(origin, {k: v.cpu() for k, v in stems.items()}, clip="tanh", fmt="f32")
    assert counts["mi_deliver_peaks"] == 0 and counts["mi_deliver_pcm"] == 1 and sum(counts.values()) == 1
    monkeypatch.undo()


# ---- 3. streams ------------------------------------------------------------------------------------------------------------------------
def blocks_for(length, seed, max_block):
    g = random.Random(seed)
    out, total = [], 0
    while total < length:
        b = g.choice([0, 1, g.randint(1, SR // 10), g.randint(SR // 2, max_block)])
        out.append(b)
        total += b
    return out


def run_stream(sep, mix, blocks, deliver, seed=7, mean=0.02, std=0.5):
    random.seed(seed)
    ss = sep.separate_stream(mean, std, deliver=deliver)
    outs, pos = [], 0
    for b in blocks:
        blk = mix[:, pos:pos + b]
        pos += blk.shape[1]
        o = ss.push(blk)
        for v in o.values():
            assert v.device == mix.device
        outs.append(o)
    outs.append(ss.finish())
    return outs, random.getstate()


def restated(stems, sources, dl):
    """`dl`'s frames from the float stems (S, C, L) of the same stream run without delivery, on the CPU."""
    x = stems.cpu()
    return {name: frames_of(value_of(x, None, kind, sel), dl.clip_code, 0 if dl.fmt == "i16" else 1)
            for name, kind, sel in dl.outputs(sources)}


def check_delivering_stream(model, length, where, deliveries, seed):
    mix = track(length, seed=seed, device=where)
    blocks = blocks_for(length, seed, 3 * SR)
    assert 0 in blocks and 1 in blocks
    sep = Separator(model, device="cuda", shifts=1)
    plain, state = run_stream(sep, mix, blocks, None, seed=seed)
    stems = torch.stack([torch.cat([o[k] for o in plain], -1) for k in model.sources])
    for dl in deliveries:
        outs, got_state = run_stream(sep, mix, blocks, dl, seed=seed)
        assert got_state == state
        want = restated(stems, model.sources, dl)
        assert all(list(o) == list(want) for o in outs)
        for o, p in zip(outs, plain):
            m = p[model.sources[0]].shape[-1]
            assert all(v.shape == (m, 2) for v in o.values())              # the same samples become final on the same push
        for k in want:
            got = torch.cat([o[k] for o in outs], 0)
            assert got.device == mix.device and got.dtype == want[k].dtype
            assert torch.equal(got.cpu(), want[k]), (dl, k)


@pytest.mark.parametrize("where", ["cpu", "cuda"])
def test_hdemucs_stream_delivers_the_restated_frames(where):
    m = hd("f32", max_batch=2, channels=4, segment=3)
    check_delivering_stream(m, 9 * SR + 777, where, [Delivery("vocals"), Delivery("drums", "none", clip="tanh", fmt="f32"),
                                                     Delivery(clip=None)], seed=21 if where == "cpu" else 22)


def test_htdemucs_stream_delivers_the_restated_frames():
    check_delivering_stream(ht("f32"), 12 * SR + 5, "cpu", [Delivery("vocals")], seed=23)


def test_apply_model_stream_delivers_without_the_affine():
    m = hd("f32", max_batch=2, channels=4, segment=3)
    mix = track(5 * SR + 3, seed=24, device="cuda")
    dl = Delivery("bass", fmt="f32", clip="clamp")
    random.seed(3)
    st = apply_model_stream(m, shifts=1, device="cuda")
    plain = torch.cat([st.push(mix[:, :2 * SR]), st.push(mix[:, 2 * SR:]), st.finish()], -1)
    random.seed(3)
    st = apply_model_stream(m, shifts=1, device="cuda", deliver=dl)
    outs = [st.push(mix[:, :2 * SR]), st.push(mix[:, 2 * SR:]), st.finish()]
    want = restated(plain, m.sources, dl)
    for k in want:
        assert torch.equal(torch.cat([o[k] for o in outs], 0).cpu(), want[k]), k


# ---- 4. groups ---------------------------------------------------------------------------------------------------------------------------
def group_script(lengths, seed):
    """[{stream: block length}] until every stream is pushed; blocks of 0 and 1 sample among them."""
    g = random.Random(seed)
    pos, script = [0] * len(lengths), []
    while any(p < n for p, n in zip(pos, lengths)):
        call = {}
        for i, n in enumerate(lengths):
            if pos[i] < n and g.random() < 0.8:
                b = min(n - pos[i], g.choice([0, 1, g.randint(1, SR // 10), g.randint(SR // 2, 2 * SR)]))
                call[i] = b
                pos[i] += b
        if call:
            script.append(call)
    return script


def run_group(sep, mixes, deliveries, script, grouped, seed=5):
    """Per call {stream: result}; solo streams (grouped=False) are opened and pushed in the same order."""
    random.seed(seed)
    g = sep.separate_stream_group() if grouped else None
    keys = [g.open(0.02, 0.5, deliver=d) if grouped else sep.separate_stream(0.02, 0.5, deliver=d) for d in deliveries]
    pos, calls = [0] * len(mixes), []
    for call in script:
        blocks = {}
        for i, b in call.items():
            blocks[i] = mixes[i][:, pos[i]:pos[i] + b]
            pos[i] += b
        if grouped:
            got = g.push({keys[i]: x for i, x in blocks.items()})
            calls.append({i: got[keys[i]] for i in blocks})
        else:
            calls.append({i: keys[i].push(x) for i, x in blocks.items()})
    if grouped:
        got = g.finish(keys)
        calls.append({i: got[k] for i, k in enumerate(keys)})
    else:
        calls.append({i: k.finish() for i, k in enumerate(keys)})
    return calls, random.getstate()


def assert_calls_equal(got, want, only=None):
    assert len(got) == len(want)
    for c, (g, w) in enumerate(zip(got, want)):
        assert list(g) == list(w)
        for i in w:
            if only is not None and i not in only:
                continue
            assert list(g[i]) == list(w[i])
            for k in w[i]:
                assert g[i][k].device == w[i][k].device and g[i][k].dtype == w[i][k].dtype
                assert same(g[i][k], w[i][k]), (c, i, k)


def test_group_streams_equal_their_solo_streams():
    m = hd("f32", max_batch=3, channels=4, segment=3)
    sep = Separator(m, device="cuda", shifts=1)
    lengths = [7 * SR + 3, 9 * SR + 777, 5 * SR + 1]
    mixes = [track(n, seed=60 + i, device=w) for i, (n, w) in enumerate(zip(lengths, ["cpu", "cpu", "cuda"]))]
    deliveries = [None, Delivery("vocals"), Delivery(fmt="f32", clip="tanh")]
    script = group_script(lengths, 4)
    want, ws = run_group(sep, mixes, deliveries, script, grouped=False)
    got, gs = run_group(sep, mixes, deliveries, script, grouped=True)
    assert gs == ws
    assert_calls_equal(got, want)
    final = got[-1]
    assert list(final[0]) == m.sources and list(final[1]) == ["vocals", "no_vocals"] and list(final[2]) == m.sources
    assert final[1]["vocals"].dtype == torch.int16 and final[2]["drums"].dtype == torch.float32 and final[2]["drums"].is_cuda


def test_a_nan_block_stays_in_its_stream():
    m = hd("f32", max_batch=3, channels=4, segment=3)
    sep = Separator(m, device="cuda", shifts=1)
    lengths = [6 * SR + 5] * 3
    mixes = [track(n, seed=70 + i) for i, n in enumerate(lengths)]
    deliveries = [Delivery("vocals"), Delivery("vocals"), Delivery("bass", fmt="f32")]
    script = [{0: SR, 1: SR, 2: SR}] * 6 + [{0: 5, 1: 5, 2: 5}]
    clean, _ = run_group(sep, mixes, deliveries, script, grouped=True)
    bad = [x.clone() for x in mixes]
    bad[1][:, 2 * SR:3 * SR] = float("nan")
    dirty, _ = run_group(sep, bad, deliveries, script, grouped=True)
    assert_calls_equal(dirty, clean, only={0, 2})
    assert any(not torch.equal(d[1]["vocals"], c[1]["vocals"]) for d, c in zip(dirty, clean))


PER_FORWARD = {"mi_segments_gather_packed", "mi_ola_accumulate_packed"}


def max_calls_per_push(n_streams, monkeypatch, deliver):
    """tests/test_gpu_stream_group.py's count: library calls per push outside the forwards, the worst of 24 pushes."""
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
    keys = [g.open(0.0, 1.0, deliver=deliver) for _ in range(n_streams)]
    worst, delivered, nbytes = 0, 0, []
    gc.collect()
    gc.disable()                    # an earlier test's model, collected mid-push, would count its mi_model_destroy here
    try:
        for _ in range(24):
            counts.clear()
            out = g.push({k: block for k in keys})
            other = sum(v for k, v in counts.items() if k not in PER_FORWARD and not k.endswith("_destroy"))
            worst = max(worst, other)
            delivered = max(delivered, counts["mi_deliver_pcm"])
            m_new = g.emitted(keys[0]) - sum(n for n, _ in nbytes)
            nbytes.append((m_new, sum(v.nbytes for v in out[keys[0]].values())))
    finally:
        gc.enable()
    counts.clear()
    g.finish(keys)
    monkeypatch.undo()
    return worst, delivered, nbytes


def test_group_delivery_is_one_more_call_per_push_and_a_quarter_of_the_bytes(monkeypatch):
    karaoke = Delivery("vocals")
    a, da, bytes_a = max_calls_per_push(2, monkeypatch, karaoke)
    b, db, _ = max_calls_per_push(16, monkeypatch, karaoke)
    assert a == b and a <= 3 + 1, (a, b)          # the parent's append, emit and compaction, plus the delivery
    assert da == db == 1
    _, d0, bytes_0 = max_calls_per_push(2, monkeypatch, None)
    assert d0 == 0
    S, channels = 4, 2
    assert sum(n for n, _ in bytes_a) > 0
    for (n, got), (n0, plain) in zip(bytes_a, bytes_0):
        assert n == n0 and got == 2 * channels * 2 * n and plain == S * channels * 4 * n


def test_group_device_bytes_stay_flat():
    m = hd("f32", max_batch=3, channels=4, segment=3)
    g = Separator(m, device="cuda", shifts=1).separate_stream_group()
    keys = [g.open(0.0, 1.0, deliver=d) for d in (Delivery("vocals"), Delivery(fmt="f32"), None)]
    block = track(SR // 2, seed=90)
    # a room in the state buffer is sized at a compaction from what is live at that moment and never shrinks; what is live
    # repeats every 9 pushes (stride 2.25 s, blocks of 0.5 s) and a compaction comes about every 13, so the rooms have seen the
    # largest live span after some 9 compactions: warm up well past that, then nothing may change
    for _ in range(200):
        g.push({k: block for k in keys})
    seen = []
    for _ in range(30):
        g.push({k: block for k in keys})
        seen.append(g.group.device_bytes())
    assert len(set(seen)) == 1, seen
    g.finish(keys)
