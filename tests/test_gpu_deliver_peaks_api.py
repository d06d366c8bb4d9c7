"""`clip="rescale"` on streams through the public interface, on the MI355X: `Separator.separate_blocks` with
`Delivery(clip="rescale", peaks="measure")` reads its source three times and yields the frames of `audio.deliver(..., clip="rescale")`
on `separate_tensor`'s stems bit for bit; a measuring stream returns nothing but its `audio.TrackPeaks`; in a group measuring,
rescaling and clamping streams share a fixed number of launches per push.  Float32 engines throughout."""
import functools
import gc
import random
from collections import Counter

import numpy as np
import pytest
import torch

from demucs_amd import _lib, audio
from demucs_amd.api import Delivery, Separator, TrackPeaks
from test_gpu_deliver_peaks import bits_of, cpu_rescaled_frames, whole_track_peak_bits
from test_gpu_deliver_rate import blocks_for, group_script, same, value_of
from test_gpu_ingest import to_i16
from test_gpu_stream import SR, hd, ht, track

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def small_hd():
    return hd("f32", max_batch=2, channels=4, segment=3)


@functools.lru_cache(maxsize=None)
def small_ht():
    return ht("f32")


def uneven(wav, seed):
    """The track in blocks of uneven length, empty and 1-sample blocks among them."""
    out, pos = [], 0
    for b in blocks_for(wav.shape[1], seed, 2 * SR):
        out.append(wav[:, pos:pos + b])
        pos += b
    assert pos >= wav.shape[1]
    return out


# ---- 1. separate_blocks -------------------------------------------------------------------------------------------------------------
def check_blocks(sep, wav, blocks, pcm, deliveries, seed):
    """`blocks` decode to `wav`: every delivery's frames are audio.deliver's on separate_tensor's stems, the source is read three
    times and `random` ends where separate_tensor leaves it."""
    random.seed(seed)
    origin, stems = sep.separate_tensor(wav.clone())
    state = random.getstate()
    divides = []
    for dl in deliveries:
        rates = None if dl.samplerate is None else (SR, dl.samplerate)
        want = audio.deliver(origin, stems, dl.stem, dl.other_method, clip="rescale", fmt=dl.fmt, samplerate=rates)
        reads = []

        def source():
            reads.append(1)
            return iter(blocks)

        random.seed(seed)
        outs = list(sep.separate_blocks(source, pcm=pcm, deliver=dl))
        assert random.getstate() == state
        assert len(reads) == 3                                               # analysis, measuring, delivering
        assert all(list(o) == list(want) for o in outs) and len(outs) == len(blocks) + 1
        for k in want:
            got = torch.cat([o[k] for o in outs], 0)
            assert got.dtype == want[k].dtype and got.shape == want[k].shape and same(got, want[k]), (dl, k)
        x = torch.stack(list(stems.values()))
        for name, kind, sel in dl.outputs(list(stems)):
            v = value_of(x, kind, sel)
            v = v if rates is None else audio.resample_frac(v, *rates)
            divides.append(float(np.float32(1.01) * np.float32(v.abs().max())) > 1.0)
    return divides


@pytest.mark.parametrize("rate", [None, 48000])
@pytest.mark.parametrize("make", [small_hd, small_ht])
def test_separate_blocks_delivers_rescaled_frames(make, rate):
    model = make()
    sep = Separator(model, device="cuda", shifts=1)
    L = 9 * SR + 777
    base = track(L, seed=61) * 0.5
    random.seed(1)
    _, probe = sep.separate_tensor(base.clone())
    loudest = max(float(v.abs().max()) for v in probe.values())
    assert loudest > 0
    # the stems follow the input's scale (the Separator normalises it and restores them): the loudest stem now peaks near 2
    loud = base * (2.0 / loudest)
    deliveries = [Delivery(clip="rescale", samplerate=rate, peaks="measure"),
                  Delivery("vocals", "add", clip="rescale", fmt="f32", samplerate=rate, peaks="measure")]
    divides = check_blocks(sep, loud, uneven(loud, 3), None, deliveries, seed=11)
    assert any(divides)                                                       # the division happened
    # the same as int16 PCM: typed (n, channels) blocks of uneven length
    q, floats = to_i16(track(L, seed=62) * 0.9)
    cuts = [0, 1, 1, SR // 3, 2 * SR + 5, 2 * SR + 5, 5 * SR, L]
    pcm_blocks = [q[a:b] for a, b in zip(cuts[:-1], cuts[1:])]
    check_blocks(sep, floats, pcm_blocks, "i16", deliveries[1 if rate else 0:][:1], seed=12)


# ---- 2. a measuring stream ------------------------------------------------------------------------------------------------------------
def run_solo(sep, mix, blocks, deliver, seed, mean=0.02, std=0.5):
    random.seed(seed)
    ss = sep.separate_stream(mean, std, deliver=deliver)
    outs, pos = [], 0
    for b in blocks:
        outs.append(ss.push(mix[:, pos:pos + b]))
        pos += b
    outs.append(ss.finish())
    return outs, ss


def plain_stems(sep, mix, blocks, seed):
    outs, _ = run_solo(sep, mix, blocks, None, seed)
    return torch.stack([torch.cat([o[k] for o in outs], -1) for k in sep.model.sources])


@pytest.mark.parametrize("where", ["cpu", "cuda"])
def test_a_measuring_stream_returns_only_its_peaks(where):
    sep = Separator(small_hd(), device="cuda", shifts=1)
    L = 9 * SR + 321
    mix = track(L, seed=71, device=where) * 3.0
    parts = [blocks_for(L, 5, 3 * SR), blocks_for(L, 6, SR)]
    stems = plain_stems(sep, mix, parts[0], seed=9).cpu()
    for rate in (None, 48000):
        for stem in (None, "vocals"):
            dl = Delivery(stem, clip="rescale", samplerate=rate, peaks="measure")
            want = []
            for name, kind, sel in dl.outputs(sep.model.sources):
                v = value_of(stems, kind, sel)
                want.append(whole_track_peak_bits(v if rate is None else audio.resample_frac(v, SR, rate)))
            found = []
            for blocks in parts:
                outs, ss = run_solo(sep, mix, blocks, dl, seed=9)
                assert all(o == {} for o in outs[:-1])
                pk = outs[-1]
                assert isinstance(pk, TrackPeaks) and pk.names == tuple(n for n, _, _ in dl.outputs(sep.model.sources))
                assert (pk.samplerate, pk.stem, pk.other_method, pk.length) == (rate, stem, "add", L)
                assert list(pk.bits) == want, (rate, stem, [hex(b) for b in pk.bits], [hex(b) for b in want])
                found.append(pk)
            assert found[0] == found[1] and all(0 < b < 0x7F800000 for b in found[0].bits)


def test_a_measuring_streams_device_bytes_do_not_grow():
    sep = Separator(small_hd(), device="cuda", shifts=1)
    for rate in (None, 48000):
        random.seed(2)
        ss = sep.separate_stream(0.0, 1.0, deliver=Delivery("vocals", clip="rescale", samplerate=rate, peaks="measure"))
        stride = ss.stream.members[0].stride
        block = track(stride // 3, seed=90)
        sizes = {}
        for push in range(1, 28):
            assert ss.push(block) == {}
            if push in (15, 27):
                sizes[push] = ss.stream.device_bytes()
        assert sizes[27] == sizes[15] > 0, sizes
        pk = ss.finish()
        assert isinstance(pk, TrackPeaks) and pk.length == 27 * block.shape[1]
        # the peaks' share: 4 bytes per output, and as many for the rows' slots
        assert ss.stream._exec.peaks.numel() == 2 and ss.stream._exec.slots.tolist() == [0, 1]


# ---- 3. a hand-made TrackPeaks ---------------------------------------------------------------------------------------------------------
def test_a_hand_made_peak_is_a_fixed_gain():
    sep = Separator(small_hd(), device="cuda", shifts=1)
    L = 7 * SR + 5
    mix = track(L, seed=75) * 3.0
    blocks = blocks_for(L, 8, 2 * SR)
    stems = plain_stems(sep, mix, blocks, seed=4)
    two = bits_of(torch.tensor(2.0))
    pk = TrackPeaks(sep.model.sources, [two] * 4)
    assert pk == TrackPeaks.from_values(sep.model.sources, [2.0, -2.0, 2.0, 2.0]) and pk.divisor("drums") == np.float32(2.0) * np.float32(1.01)
    for fmt in ("i16", "f32"):
        outs, _ = run_solo(sep, mix, blocks, Delivery(clip="rescale", fmt=fmt, peaks=pk), seed=4)
        for i, name in enumerate(sep.model.sources):
            got = torch.cat([o[name] for o in outs], 0)
            want = cpu_rescaled_frames(stems[i], two, 0 if fmt == "i16" else 1)            # i16_pcm(v / 2.02f)
            assert got.dtype == want.dtype and torch.equal(got, want), (fmt, name)
    assert float(stems.abs().max()) > 0


# ---- 4. groups ---------------------------------------------------------------------------------------------------------------------------
def run_mixed(sep, mixes, deliveries, script, grouped, seed=5):
    """tests/test_gpu_deliver_rate.py's `run_group`: stream i is opened at call i and finished on the call that pushes its last
    sample; solo streams (grouped=False) are opened, pushed and finished in the same order."""
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
    return calls, random.getstate(), g


def test_group_streams_equal_their_solo_streams():
    sep = Separator(hd("f32", max_batch=3, channels=4, segment=3), device="cuda", shifts=1)
    lengths = [9 * SR + 3, 8 * SR + 777, 10 * SR + 1, 7 * SR + 40, 9 * SR + 5]
    where = ["cpu", "cuda", "cpu", "cpu", "cuda"]
    mixes = [track(n, seed=80 + i, device=w) * 3.0 for i, (n, w) in enumerate(zip(lengths, where))]
    # the peaks the delivering streams are given: found beforehand by a solo measuring stream over the same mix, and a hand-made
    # peak of 1 at 48 kHz, with which every frame is divided whatever the stems' level
    outs, _ = run_solo(sep, mixes[1], [lengths[1]], Delivery("vocals", clip="rescale", peaks="measure"), seed=3)
    found = {1: outs[-1], 4: TrackPeaks.from_values(["vocals", "no_vocals"], [1.0, 1.0], stem="vocals", samplerate=48000)}
    assert isinstance(found[1], TrackPeaks) and found[1].length == lengths[1]
    deliveries = [Delivery(clip="rescale", samplerate=48000, peaks="measure"),
                  Delivery("vocals", clip="rescale", peaks=found[1]),
                  Delivery("bass", clip="clamp"),
                  Delivery("vocals", clip="rescale", fmt="f32", peaks="measure"),
                  Delivery("vocals", clip="rescale", fmt="f32", samplerate=48000, peaks=found[4])]
    script = group_script(lengths, 6)
    want, ws, _ = run_mixed(sep, mixes, deliveries, script, grouped=False)
    got, gs, g = run_mixed(sep, mixes, deliveries, script, grouped=True)
    assert gs == ws and len(got) == len(want)
    peaks_seen = 0
    for c, ((gop, gr), (wop, wr)) in enumerate(zip(got, want)):
        assert gop == wop and list(gr) == list(wr)
        for i in wr:
            if isinstance(wr[i], TrackPeaks):
                assert gop == "finish" and gr[i] == wr[i], (c, i, gr[i], wr[i])
                peaks_seen += 1
                continue
            assert list(gr[i]) == list(wr[i]) and (deliveries[i].measures) == (wr[i] == {})
            for k in wr[i]:
                assert gr[i][k].device == wr[i][k].device and gr[i][k].dtype == wr[i][k].dtype and same(gr[i][k], wr[i][k]), (c, i, k)
    assert peaks_seen == 2 and [op for op, _ in got].count("finish") >= 2      # streams ended on different calls
    # every finished stream's slots are free again
    ex = g.group._exec
    assert 0 < ex.peaks_used <= 4 + 2 + 2 + 2 and sum(n * len(v) for n, v in ex.peaks_free.items()) == ex.peaks_used


PER_FORWARD = {"mi_segments_gather_packed", "mi_ola_accumulate_packed"}
DELIVERY_CALLS = ("mi_deliver_pcm", "mi_deliver_resample_pcm", "mi_deliver_resample_pcm_peaks", "mi_deliver_peaks_update",
                  "mi_deliver_resample_peaks", "mi_deliver_peaks")


def calls_per_push(deliveries, monkeypatch, pushes=16):
    """tests/test_gpu_stream_group.py's census: library calls per push outside the forwards; the worst push, and per delivery
    entry the most calls a push made."""
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
        for _ in range(pushes):
            counts.clear()
            g.push({k: block for k in keys})
            worst = max(worst, sum(v for k, v in counts.items() if k not in PER_FORWARD and not k.endswith("_destroy")))
            for k in DELIVERY_CALLS:
                most[k] = max(most[k], counts[k])
    finally:
        gc.enable()
    counts.clear()
    g.finish(keys)
    monkeypatch.undo()
    return worst, most


def test_a_push_is_a_fixed_number_of_launches_whatever_the_number_of_streams(monkeypatch):
    pk = TrackPeaks.from_values(["vocals", "no_vocals"], [2.0, 0.5], stem="vocals")
    pk48 = TrackPeaks.from_values(["vocals", "no_vocals"], [2.0, 0.5], stem="vocals", samplerate=48000)

    def group(n):
        one = [Delivery("vocals", clip="rescale", peaks="measure"), Delivery("vocals", clip="rescale", samplerate=48000, peaks="measure"),
               Delivery("vocals", clip="rescale", peaks=pk), Delivery("vocals", clip="rescale", samplerate=48000, peaks=pk48),
               Delivery("vocals"), Delivery("vocals", samplerate=48000)]
        return one * n

    a, ma = calls_per_push(group(1), monkeypatch)
    b, mb = calls_per_push(group(2), monkeypatch)
    assert a == b and ma == mb, (a, b, ma, mb)
    # one launch for all model-rate rows, one for all resampled rows, one measuring launch each for the two kinds of row
    assert ma == Counter({"mi_deliver_pcm": 1, "mi_deliver_resample_pcm_peaks": 1, "mi_deliver_peaks_update": 1,
                          "mi_deliver_resample_peaks": 1, "mi_deliver_resample_pcm": 0, "mi_deliver_peaks": 0}), ma
    # without measuring streams there is no measuring launch, and without a rescaling row the resampled rows take today's entry
    c, mc = calls_per_push([Delivery("vocals"), Delivery("vocals", samplerate=48000)], monkeypatch)
    assert c == a - 2 and mc["mi_deliver_resample_pcm"] == 1 and mc["mi_deliver_pcm"] == 1 and sum(mc.values()) == 2
