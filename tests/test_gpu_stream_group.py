"""`apply_model_stream_group` / `Separator.separate_stream_group` on the MI355X: every per-push output of a group of streams equals
a solo `ModelStream`'s bit for bit, with the same use of `random`, while the group pools its streams' segments into shared
forwards and does a fixed number of other library calls per push (demucs_amd/stream.py, StreamGroup); and `mi_streams_emit` /
`mi_streams_append` / `mi_streams_compact` alone against the one-stream kernels."""
import ctypes as C
import gc
import random
from collections import Counter

import pytest
import torch

from demucs_amd import _lib
from demucs_amd.api import Separator
from demucs_amd.apply import BagOfModels, apply_model, apply_model_stream, apply_model_stream_group
from demucs_amd.stream import emit_scales
from test_gpu_stream import BAG_W, SR, _stats_for, assert_same_bits, hd, ht, track

pytestmark = pytest.mark.gpu


def stream_ptr():
    return C.c_void_p(_lib.current_stream_ptr())


def script_for(lengths, seed, max_block=3 * SR, stagger=True):
    """Calls [("open", i) | ("push", {i: n}) | ("finish", [i, ...])]: staggered opens, random blocks (zero-length ones too),
    random finish groupings."""
    g = random.Random(seed)
    n = len(lengths)
    pos, state, script = [0] * n, ["new"] * n, []
    while any(s != "done" for s in state):
        new = [i for i in range(n) if state[i] == "new"]
        if new and (not stagger or g.random() < 0.35 or all(s != "open" for s in state)):
            for i in (new[:1] if stagger else new):
                script.append(("open", i))
                state[i] = "open"
            continue
        live = [i for i in range(n) if state[i] == "open"]
        full = [i for i in live if pos[i] >= lengths[i]]
        if full and g.random() < 0.5:
            g.shuffle(full)
            keys = full[:g.randint(1, len(full))]
            script.append(("finish", keys))
            for i in keys:
                state[i] = "done"
            continue
        pick = [i for i in live if pos[i] < lengths[i] and g.random() < 0.8] or [i for i in live if pos[i] < lengths[i]][:1]
        g.shuffle(pick)
        blocks = {}
        for i in pick:
            b = min(lengths[i] - pos[i], g.choice([0, 1, g.randint(1, SR // 10), g.randint(SR // 2, max_block)]))
            blocks[i] = b
            pos[i] += b
        script.append(("push", blocks))
    return script


def run(model, script, mixes, kw, grouped, seed=7, length_kw=False):
    random.seed(seed)
    group = apply_model_stream_group(model, device="cuda", **kw) if grouped else None
    keys, pos, outs, pieces = {}, [0] * len(mixes), [], [[] for _ in mixes]
    opened = {}
    for op, arg in script:
        if op == "open":
            opened[arg] = random.getstate()             # the stream's shift offsets come from here, as apply_model's would
            length = mixes[arg].shape[1] if length_kw else None
            keys[arg] = group.open(length=length) if grouped else apply_model_stream(model, device="cuda", length=length, **kw)
            continue
        if op == "push":
            blocks = {}
            for i, b in arg.items():
                blocks[i] = mixes[i][:, pos[i]:pos[i] + b]
                pos[i] += b
            if grouped:
                got = group.push({keys[i]: x for i, x in blocks.items()})
                res = {i: got[keys[i]] for i in blocks}
            else:
                res = {i: keys[i].push(x) for i, x in blocks.items()}
            for i in res:
                assert res[i].device == mixes[i].device
        else:
            if grouped:
                got = group.finish([keys[i] for i in arg])
                res = {i: got[keys[i]] for i in arg}
            else:
                res = {i: keys[i].finish() for i in arg}
        outs.append(res)
        for i, o in res.items():
            pieces[i].append(o)
    run.opened = opened
    return outs, [torch.cat(p, -1) for p in pieces], random.getstate()


def check_group(model, lengths, where, seed, length_kw=False, whole=True, **kw):
    mixes = [track(n, seed=seed + i, device=w) for i, (n, w) in enumerate(zip(lengths, where))]
    script = script_for(lengths, seed)
    want, want_cat, want_state = run(model, script, mixes, kw, grouped=False, length_kw=length_kw)
    got, got_cat, got_state = run(model, script, mixes, kw, grouped=True, length_kw=length_kw)
    opened = run.opened
    assert got_state == want_state
    for call, (g, w) in enumerate(zip(got, want)):
        assert list(g) == list(w)
        for i in w:
            assert g[i].shape == w[i].shape and g[i].device == w[i].device
            assert torch.equal(g[i], w[i]), f"call {call} stream {i}: max diff {(g[i] - w[i]).abs().max().item():.3e}"
    if whole:
        for i, mix in enumerate(mixes):
            random.setstate(opened[i])
            ref = apply_model(model, mix[None], device="cuda", **kw)[0]
            assert torch.equal(got_cat[i], ref.to(got_cat[i].device)), i
    return got_cat


# ---- 1. HTDemucs: six streams, staggered, host and device blocks mixed --------------------------------------------------------
@pytest.mark.parametrize("mode", ["f32", "bf16", "f16"])
def test_htdemucs_group_equals_solo_streams(mode):
    lengths = [5 * SR + 7, 9 * SR + 1, 26 * SR + 333, 13 * SR, 17 * SR + 5, 11 * SR + 99]       # one < a segment, one > 3
    where = ["cpu", "cuda", "cpu", "cuda", "cuda", "cpu"]
    check_group(ht(mode, max_batch=4), lengths, where, seed={"f32": 1, "bf16": 2, "f16": 3}[mode], shifts=1)


# ---- 2. a bag of two, two shift passes, length= -------------------------------------------------------------------------------
def test_bag_with_shifts_and_length():
    bag = BagOfModels([ht("f32", seed=0), ht("f32", seed=1)], BAG_W)
    check_group(bag, [12 * SR + 5, 4 * SR, 9 * SR + 77], ["cpu", "cuda", "cpu"], seed=11, length_kw=True, shifts=2)


# ---- 3. HDemucs: tails of equal and of different lengths in one finish ---------------------------------------------------------
@pytest.mark.parametrize("mode", ["f32", "f16"])
def test_hdemucs_group_tails_in_one_finish(mode):
    m = hd(mode, segment=3)
    lengths = [7 * SR + 123, 7 * SR + 123, 5 * SR + 4321, 2 * SR + 10]
    mixes = [track(n, seed=20 + i, device="cuda") for i, n in enumerate(lengths)]
    script = [("open", i) for i in range(4)] + [("push", {i: SR for i in range(4)})] * 2 + \
        [("push", {i: n - 2 * SR for i, n in enumerate(lengths)}), ("finish", [0, 1, 2, 3])]
    want, want_cat, ws = run(m, script, mixes, dict(shifts=0), grouped=False)       # no offsets: equal tracks, equal tails
    lib = _lib.load()
    real, calls = lib.mi_hmodel_forward, []

    def counting(*args):
        calls.append(args[3])
        return real(*args)

    lib.mi_hmodel_forward = counting
    try:
        got, got_cat, gs = run(m, script, mixes, dict(shifts=0), grouped=True)
    finally:
        lib.mi_hmodel_forward = real
    assert gs == ws
    for g, w in zip(got, want):
        for i in w:
            assert torch.equal(g[i], w[i]), i
    assert any(b >= 2 for b in calls)          # the two equal tails share a main-engine forward, where a solo stream's is alone
    for i, mix in enumerate(mixes):
        assert torch.equal(got_cat[i], apply_model(m, mix[None], shifts=0, device="cuda")[0]), i


def test_demucs_unittest_width_group():
    m = hd("f32", max_batch=2, channels=4, segment=2)
    check_group(m, [7 * SR + 3, 3 * SR + 1, 5 * SR], ["cpu", "cuda", "cpu"], seed=31, shifts=0)


# ---- 4. fewer forwards than the solo streams, none above max_batch ---------------------------------------------------------------
def lockstep(n_streams, seconds=20):
    return [("open", i) for i in range(n_streams)] + [("push", {i: SR for i in range(n_streams)})] * seconds + \
        [("finish", list(range(n_streams)))]


def test_group_runs_fewer_forwards(monkeypatch):
    m = ht("f32", max_batch=8)
    mixes = [track(20 * SR, seed=40 + i) for i in range(8)]
    lib = _lib.load()
    real, calls = lib.mi_model_forward, []

    def counting(*args):
        calls.append(args[3])
        return real(*args)

    monkeypatch.setattr(lib, "mi_model_forward", counting)
    _, solo, _ = run(m, lockstep(8), mixes, dict(shifts=1), grouped=False)
    n_solo = len(calls)
    calls.clear()
    _, grp, _ = run(m, lockstep(8), mixes, dict(shifts=1), grouped=True)
    assert len(calls) < n_solo and all(b <= 8 for b in calls), (len(calls), n_solo, calls)
    assert all(torch.equal(a, b) for a, b in zip(grp, solo))


# ---- 5. library calls per push do not grow with the number of streams -------------------------------------------------------------
PER_FORWARD = {"mi_segments_gather_packed", "mi_ola_accumulate_packed"}


def max_calls_per_push(n_streams, monkeypatch):
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
    g = apply_model_stream_group(m, shifts=1, device="cuda")
    keys = [g.open() for _ in range(n_streams)]
    worst = 0
    gc.collect()
    gc.disable()                    # an earlier test's model, collected mid-push, would count its mi_model_destroy here
    try:
        for _ in range(24):
            counts.clear()
            g.push({k: block for k in keys})
            other = sum(v for k, v in counts.items() if k not in PER_FORWARD and not k.endswith("_destroy"))
            assert counts["mi_segments_gather_packed"] == counts["mi_ola_accumulate_packed"]
            worst = max(worst, other)
    finally:
        gc.enable()
    counts.clear()
    g.finish(keys)
    monkeypatch.undo()
    return worst


def test_calls_per_push_do_not_grow_with_streams(monkeypatch):
    a = max_calls_per_push(2, monkeypatch)
    b = max_calls_per_push(16, monkeypatch)
    assert a == b and a <= 3, (a, b)          # append, emit and at most one compaction


# ---- 6. the kernels alone ------------------------------------------------------------------------------------------------------------
S4, CH, SL6 = 4, 2, 3000


def _emit_fixture(members, shifts, g):
    """One stream's accumulators with NaN / Inf, its segment lists and pass table, as test_gpu_stream's emit test builds them."""
    L, stride = 6000, 2250
    rows = S4 * CH
    passes, segs, accs, base = [], [], [], 0
    for e in range(members):
        for _ in range(max(1, shifts)):
            d = int(torch.randint(0, 501, (1,), generator=g)) if shifts else 0
            plen = L + d
            acc = torch.randn(rows, plen, generator=g) * 3
            acc[torch.rand(rows, plen, generator=g) < 0.01] = float("nan")
            acc[torch.rand(rows, plen, generator=g) < 0.01] = float("inf")
            acc[torch.rand(rows, plen, generator=g) < 0.01] = -float("inf")
            s_lo = len(segs) // 2
            for o in range(0, plen, stride):
                segs += [o, min(plen - o, SL6)]
            passes.append([base, plen, d + 1234, s_lo, len(segs) // 2, 0, SL6, e])
            base += rows * plen
            accs.append(acc.reshape(-1))
    return passes, segs, torch.cat(accs)


@pytest.mark.parametrize("members,shifts", [(1, 0), (1, 1), (2, 2), (3, 1)])
def test_streams_emit_equals_stream_emit(members, shifts):
    lib = _lib.load()
    g = torch.Generator().manual_seed(members * 10 + shifts)
    weights = (torch.cat([torch.arange(1, SL6 // 2 + 1), torch.arange(SL6 - SL6 // 2, 0, -1)]) / (SL6 // 2)).float().cuda()
    bag = [[float(x) for x in torch.rand(S4, generator=g) * 2] for _ in range(members)] if members > 1 else None
    scales = torch.tensor(emit_scales(shifts, members, bag, S4), dtype=torch.float32).cuda()
    stats = torch.tensor([0.25, 1.75, -0.5, 0.125], dtype=torch.float32).cuda()
    spec = [(2000, -1), (3111, 0), (0, 0), (1500, 1), (77, -1)]         # (n, stats pair): plain, affine, n = 0, ...
    all_passes, all_segs, accs, rows_t, wants = [], [], [], [], []
    acc_off = out_off = 0
    for n, si in spec:
        passes, segs, acc = _emit_fixture(members, shifts, g)
        acc = acc.cuda()
        if n:
            want = torch.empty(S4, CH, n, device="cuda")
            t_p = torch.tensor(passes, dtype=torch.int64).cuda()
            t_s = torch.tensor(segs, dtype=torch.int64).cuda()
            st = stats[2 * si:2 * si + 2] if si >= 0 else None
            _lib.check(lib.mi_stream_emit(acc.data_ptr(), acc.numel(), S4, CH, t_p.data_ptr(), len(passes), t_s.data_ptr(),
                                          len(segs) // 2, weights.data_ptr(), weights.numel(), scales.data_ptr(), members, shifts,
                                          int(bag is not None), st.data_ptr() if st is not None else None, n, want.data_ptr(),
                                          want.numel(), stream_ptr()), "mi_stream_emit")
            wants.append((out_off, n, want))
        p_lo, s_lo = len(all_passes), len(all_segs) // 2
        all_passes += [[p[0] + acc_off, p[1], p[2], p[3] + s_lo, p[4] + s_lo, p[5], p[6], p[7]] for p in passes]
        all_segs += segs
        rows_t.append([p_lo, len(all_passes), s_lo, len(all_segs) // 2, si, out_off, n])
        accs.append(acc)
        acc_off += acc.numel()
        out_off += S4 * CH * n
    acc_all = torch.cat(accs)
    t_passes = torch.tensor(all_passes, dtype=torch.int64).cuda()
    t_segs = torch.tensor(all_segs, dtype=torch.int64).cuda()

    def emit(rows, out, cap):
        table = torch.tensor(rows, dtype=torch.int64).cuda()
        _lib.check(lib.mi_streams_emit(acc_all.data_ptr(), acc_all.numel(), S4, CH, table.data_ptr(), len(rows), 3111,
                                       t_passes.data_ptr(), len(all_passes), t_segs.data_ptr(), len(all_segs) // 2,
                                       weights.data_ptr(), weights.numel(), scales.data_ptr(), members, shifts, int(bag is not None),
                                       stats.data_ptr(), 2, out.data_ptr(), cap, stream_ptr()), "mi_streams_emit")
        torch.cuda.synchronize()

    canary = 12345.0
    out = torch.full((1024 + out_off + 1024,), canary, device="cuda")
    emit(rows_t, out[1024:], out_off)
    for off, n, want in wants:
        assert_same_bits(out[1024 + off:1024 + off + S4 * CH * n].view(S4, CH, n), want, f"stream at {off}")
    assert (out[:1024] == canary).all() and (out[1024 + out_off:] == canary).all()
    # out-of-range table entries: outputs past the capacity, negative offsets, wild pass / segment / stats indices
    out.fill_(canary)
    bad = [[0, 10 ** 6, -5, 10 ** 9, 7, out_off - 8, 2000], [0, 1, 0, 1, -1, -8, 50], [-3, 2, 0, 1, 99, 0, 10 ** 6],
           [0, 1, 0, 1, -1, 2 ** 62, 5]]
    emit(bad, out[1024:], out_off)
    assert (out[:1024] == canary).all() and (out[1024 + out_off:] == canary).all()


def test_streams_append_equals_track_affine():
    lib = _lib.load()
    g = torch.Generator().manual_seed(3)
    stats = torch.tensor([0.125, 0.75, -0.3, 1.5e-3], dtype=torch.float32).cuda()
    blocks = [torch.randn(2, n, generator=g).cuda() for n in (1, 1029, 4096, 333)]
    blocks[1][0, 7] = float("nan")
    sis = [0, -1, 1, 0]
    cols = [0, 5, 100, 17]
    caps = [b.shape[1] + c + 40 for b, c in zip(blocks, cols)]
    bases = [sum(2 * cp for cp in caps[:i]) + 256 for i in range(len(caps))]
    total = bases[-1] + 2 * caps[-1]
    canary = -777.0
    win = torch.full((total + 256,), canary, device="cuda")
    rows = [[b.data_ptr(), b.shape[1], base, cap, col, si] for b, base, cap, col, si in zip(blocks, bases, caps, cols, sis)]
    rows.append([blocks[2].data_ptr(), 4096, total - 10, 4096, 0, -1])             # a window past the buffer: nothing written
    table = torch.tensor(rows, dtype=torch.int64).cuda()
    _lib.check(lib.mi_streams_append(win.data_ptr(), total, 2, table.data_ptr(), len(rows), 4096, stats.data_ptr(), 2,
                                     stream_ptr()), "mi_streams_append")
    torch.cuda.synchronize()
    for b, base, cap, col, si in zip(blocks, bases, caps, cols, sis):
        want = b.clone()
        if si >= 0:
            _lib.check(lib.mi_track_affine(want.data_ptr(), want.numel(), stats[2 * si:].data_ptr(), 0, stream_ptr()),
                       "mi_track_affine")
        got = win[base:base + 2 * cap].view(2, cap)
        assert_same_bits(got[:, col:col + b.shape[1]], want, f"append at {base}")
        assert (got[:, :col] == canary).all() and (got[:, col + b.shape[1]:] == canary).all()
    assert (win[:256] == canary).all() and (win[total:] == canary).all()


def test_streams_compact_copies_and_zero_fills():
    lib = _lib.load()
    src = torch.randn(5000, device="cuda")
    canary = 3.5
    dst = torch.full((6000,), canary, device="cuda")
    rows = [[100, 10, 300, 400], [0, 500, 0, 50], [4900, 1000, 500, 200], [-5, 2000, 10, 10], [0, 5990, 10, 100]]
    table = torch.tensor(rows, dtype=torch.int64).cuda()
    _lib.check(lib.mi_streams_compact(dst[8:].data_ptr(), 5992 - 8, src.data_ptr(), src.numel(), table.data_ptr(), len(rows), 400,
                                      stream_ptr()), "mi_streams_compact")
    torch.cuda.synchronize()
    d = dst[8:]
    assert torch.equal(d[10:310], src[100:400]) and (d[310:410] == 0).all()
    assert (d[500:550] == 0).all()
    assert torch.equal(d[1000:1100], src[4900:5000]) and (d[1100:1200] == 0).all()        # source clamped to its capacity
    assert (d[2000:2010] == 0).all()                                                      # a negative source reads nothing
    assert (dst[:8] == canary).all() and (dst[5992:] == canary).all()                     # nothing past the declared capacity


# ---- 7. a NaN block stays in its stream --------------------------------------------------------------------------------------------
def test_non_finite_block_stays_in_its_stream():
    m = ht("f32", max_batch=8)
    lengths = [12 * SR + 5, 12 * SR + 5, 10 * SR + 1]
    clean = [track(n, seed=60 + i, device="cuda") for i, n in enumerate(lengths)]
    dirty = [x.clone() for x in clean]
    dirty[1][:, 3 * SR:3 * SR + 100] = float("nan")
    dirty[1][1, 5 * SR] = float("inf")
    script = script_for(lengths, 61)
    _, alone, _ = run(m, script, clean, dict(shifts=1), grouped=False)
    _, mixed, _ = run(m, script, dirty, dict(shifts=1), grouped=True)
    assert torch.equal(mixed[0], alone[0]) and torch.equal(mixed[2], alone[2])
    assert not torch.isfinite(mixed[1]).all()


# ---- 8. Separator.separate_stream_group ------------------------------------------------------------------------------------------
def test_separate_stream_group_equals_separate_tensor():
    sep = Separator(ht("f32", max_batch=8), device="cuda", shifts=1)
    wavs = [track(n, seed=70 + i) * 0.3 for i, n in enumerate([9 * SR + 17, 14 * SR + 3, 6 * SR + 1])]
    wants = []
    for i, w in enumerate(wavs):
        random.seed(70 + i)
        wants.append(sep.separate_tensor(w.clone())[1])
    sg = sep.separate_stream_group()
    keys = []
    for i, w in enumerate(wavs):
        random.seed(70 + i)                   # each stream's shift offset drawn as its own separate_tensor's
        keys.append(sg.open(*_stats_for(w)))
    outs = {k: [] for k in keys}
    for p in range(0, max(w.shape[1] for w in wavs), 2 * SR):
        got = sg.push({k: w[:, p:p + 2 * SR] for k, w in zip(keys, wavs) if p < w.shape[1]})
        for k, v in got.items():
            outs[k].append(v)
    fin = sg.finish(keys)
    for k, want in zip(keys, wants):
        for s in want:
            assert torch.equal(torch.cat([o[s] for o in outs[k]] + [fin[k][s]], -1), want[s]), s


# ---- 9. bounded device memory ------------------------------------------------------------------------------------------------------
def test_device_memory_is_flat_and_freed():
    m = ht("f32", max_batch=8)
    g = apply_model_stream_group(m, shifts=1, device="cuda")
    keys = [g.open() for _ in range(16)]
    block = track(SR, seed=80)
    peaks = {}
    torch.cuda.synchronize()
    for sec in range(8 * 60):
        g.push({k: block for k in keys})
        if sec == 30:
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
        if sec + 1 in (2 * 60, 8 * 60):
            torch.cuda.synchronize()
            peaks[sec + 1] = torch.cuda.max_memory_allocated()
    assert abs(peaks[8 * 60] - peaks[2 * 60]) < 1 << 20, peaks
    full = g.device_bytes()
    g.finish(keys[:8])
    g.push({k: block for k in keys[8:]})
    assert g.device_bytes() < full, (g.device_bytes(), full)
    g.finish(keys[8:])
