"""Gain-weighted remixes through the public interface, on the MI355X: `audio.deliver_mix` on a separated track, and
`Delivery(mix=...)` on solo streams, stream groups, `Separator.separate_stream` and `separate_blocks`.  A stream's frames equal
`audio.deliver_mix(*sep.separate_tensor(wav), mix, ...)` bit for bit, `wav` a device tensor: `separate_tensor` hands a device mix
back normalised and restored (`w * s + mean`), which is what a stream reads from its window.  Float32 engines throughout."""
import gc
import random
from collections import Counter

import pytest
import torch

from demucs_amd import _lib, audio
from demucs_amd.api import Delivery, Separator, TrackPeaks
from demucs_amd.apply import apply_model_stream
from test_gpu_deliver import i16_pcm
from test_gpu_deliver_peaks_api import PER_FORWARD, run_mixed, small_hd, small_ht, uneven
from test_gpu_deliver_rate import group_script, same
from test_gpu_ingest import to_i16
from test_gpu_stream import SR, hd, track

pytestmark = pytest.mark.gpu
MIX = {"practice": {"mix": 1, "vocals": 10 ** -0.6 - 1},                     # vocals lowered by 12 dB
       "drums_up": {"drums": 1.5, "bass": 1, "other": 1, "vocals": 1.0},
       "minus_vocals": {"mix": 1, "vocals": -1},
       "quiet_bass": {"bass": 0.1, "drums": 0}}
MIX_ENTRIES = ("mi_deliver_mix_pcm", "mi_deliver_mix_peaks", "mi_deliver_mix_peaks_update")


def cat(outs, name):
    return torch.cat([o[name] for o in outs], 0)


def analysed(sep, blocks, **kw):
    an = sep.analyse_stream(**kw)
    for b in blocks:
        an.push(b)
    return an.finish()


def stream_frames(sep, blocks, deliver, seed, grouped=False, **kw):
    """Every push's and finish's result of one stream over `blocks`, solo or as a group of one."""
    random.seed(seed)
    if grouped:
        g = sep.separate_stream_group()
        key = g.open(deliver=deliver, **kw)
        outs = [g.push({key: b})[key] for b in blocks]
        outs.append(g.finish([key])[key])
    else:
        ss = sep.separate_stream(deliver=deliver, **kw)
        outs = [ss.push(b) for b in blocks]
        outs.append(ss.finish())
    return outs, random.getstate()


# ---- 1. audio.deliver_mix on a whole track -------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def separated():
    g = torch.Generator().manual_seed(12)
    block = (torch.randn(4, 2, SR + 3, generator=g) * 0.45).cuda()
    origin = (torch.randn(2, SR + 3, generator=g) * 0.6).cuda()
    return origin, dict(zip(["drums", "bass", "other", "vocals"], block))


def restated(origin, stems, mix, clip, fmt):
    """The chain a user of the reference writes: sum(g * x) in float32, prevent_clip, i16_pcm."""
    want = {}
    for name, gains in mix.items():
        acc = torch.zeros_like(origin)
        for key in ["mix"] + list(stems):
            g = gains.get(key, 0)
            if g != 0:
                acc = acc + torch.tensor(g, dtype=torch.float32) * (origin if key == "mix" else stems[key])
        w = audio.prevent_clip(acc, clip).cpu()
        want[name] = (i16_pcm(w) if fmt == "i16" else w).t().contiguous()
    return want


@pytest.mark.parametrize("fmt", ["i16", "f32"])
def test_deliver_mix_equals_the_restated_chain(separated, fmt):
    origin, stems = separated
    host = {k: v.cpu() for k, v in stems.items()}
    for clip in ("rescale", "clamp", "tanh", None):
        want = restated(origin, stems, MIX, clip, fmt)
        got = audio.deliver_mix(origin, stems, MIX, clip=clip, fmt=fmt)
        assert list(got) == list(MIX)
        for k in want:
            assert got[k].is_cuda and got[k].shape == (SR + 3, 2) and torch.equal(got[k].cpu(), want[k]), (clip, k)
        on_host = audio.deliver_mix(origin.cpu(), host, MIX, clip=clip, fmt=fmt)
        for k in want:
            assert on_host[k].device.type == "cpu" and torch.equal(on_host[k], want[k]), (clip, k)
        # the reference's own residuals, by their gains
        minus = audio.deliver(origin, stems, "vocals", "minus", clip=clip, fmt=fmt)["minus_vocals"]
        assert torch.equal(got["minus_vocals"], minus) if fmt == "i16" else bool((got["minus_vocals"] == minus).all())
        add = audio.deliver(origin, stems, "vocals", "add", clip=clip, fmt=fmt)["no_vocals"]
        alone = audio.deliver_mix(None, stems, {"no_vocals": {"drums": 1, "bass": 1, "other": 1}}, clip=clip, fmt=fmt)
        assert torch.equal(alone["no_vocals"], add)


def test_deliver_mix_is_one_launch_pair_per_track(separated, monkeypatch):
    origin, stems = separated
    lib = _lib.load()
    counts = Counter()
    for name in _lib.SIGNATURES:
        real = getattr(lib, name)

        def wrapped(*args, _real=real, _name=name):
            counts[_name] += 1
            return _real(*args)

        monkeypatch.setattr(lib, name, wrapped)
    audio.deliver_mix(origin, stems, MIX, clip="rescale")
    assert counts == Counter({"mi_deliver_mix_peaks": 1, "mi_deliver_mix_pcm": 1})
    counts.clear()
    audio.deliver_mix(origin.cpu(), {k: v.cpu() for k, v in stems.items()}, MIX, clip="tanh", fmt="f32")
    assert counts == Counter({"mi_deliver_mix_pcm": 1})
    monkeypatch.undo()


# ---- 2. streams against separate_tensor ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("make,grouped", [(small_hd, False), (small_hd, True), (small_ht, False)])
def test_stream_frames_equal_deliver_mix_on_separate_tensor(make, grouped):
    sep = Separator(make(), device="cuda", shifts=1)
    L = (12 if make is small_ht else 7) * SR + 777           # longer than a segment: the window is trimmed along the way
    wav = track(L, seed=31, device="cuda") * 0.8
    random.seed(5)
    origin, stems = sep.separate_tensor(wav.clone())
    state = random.getstate()
    blocks = uneven(wav.cpu(), 4)                           # host blocks of uneven length, empty and 1-sample ones among them
    stats = analysed(sep, blocks)
    for clip, fmt in (("clamp", "i16"), ("tanh", "f32")) if make is small_hd else (("clamp", "i16"),):
        want = audio.deliver_mix(origin, stems, MIX, clip=clip, fmt=fmt)
        outs, got_state = stream_frames(sep, blocks, Delivery(mix=MIX, clip=clip, fmt=fmt), 5, grouped, stats=stats)
        assert got_state == state and all(list(o) == list(MIX) for o in outs)
        for k in want:
            got = cat(outs, k)
            assert got.device.type == "cpu" and got.dtype == want[k].dtype and same(got, want[k].cpu()), (clip, fmt, k)
        if fmt == "i16":
            minus = audio.deliver(origin, stems, "vocals", "minus", clip=clip, fmt="i16")["minus_vocals"]
            assert cat(outs, "minus_vocals").numpy().tobytes() == minus.cpu().numpy().tobytes()
    assert sum(o["practice"].shape[0] > 0 for o in outs) >= 2     # the frames came over several calls


def test_int16_feed_and_device_blocks():
    sep = Separator(small_hd(), device="cuda", shifts=1)
    L = 6 * SR + 41
    q, floats = to_i16(track(L, seed=32) * 0.9)
    random.seed(6)
    origin, stems = sep.separate_tensor(floats.cuda())
    want = audio.deliver_mix(origin, stems, MIX, clip="clamp", fmt="i16")
    cuts = [0, 1, 1, SR // 3, 2 * SR + 5, 2 * SR + 5, 5 * SR, L]
    for where in ("cpu", "cuda"):
        blocks = [q[a:b].to(where) for a, b in zip(cuts[:-1], cuts[1:])]
        stats = analysed(sep, blocks, pcm="i16")
        for grouped in (False, True):
            outs, _ = stream_frames(sep, blocks, Delivery(mix=MIX), 6, grouped, stats=stats, pcm="i16")
            for k in want:
                got = cat(outs, k)
                assert got.device.type == where and torch.equal(got.cpu(), want[k].cpu()), (where, grouped, k)


def test_apply_model_stream_reads_the_window_as_it_is():
    """Without the Separator's affine the mix is the pushed input itself."""
    m = small_hd()
    mix = track(5 * SR + 3, seed=24, device="cuda")
    cuts = [0, 2 * SR, 2 * SR + 1, 5 * SR + 3]
    random.seed(3)
    st = apply_model_stream(m, shifts=1, device="cuda")
    plain = torch.cat([st.push(mix[:, a:b]) for a, b in zip(cuts[:-1], cuts[1:])] + [st.finish()], -1)
    want = audio.deliver_mix(mix, dict(zip(m.sources, plain)), MIX, clip="clamp", fmt="f32")
    random.seed(3)
    st = apply_model_stream(m, shifts=1, device="cuda", deliver=Delivery(mix=MIX, fmt="f32"))
    outs = [st.push(mix[:, a:b]) for a, b in zip(cuts[:-1], cuts[1:])] + [st.finish()]
    for k in want:
        assert torch.equal(cat(outs, k), want[k]), k


# ---- 3. rescale: measure, then deliver -------------------------------------------------------------------------------------------------
def test_separate_blocks_rescales_remixes_in_three_passes():
    sep = Separator(small_hd(), device="cuda", shifts=1)
    L = 6 * SR + 5
    wav = track(L, seed=33, device="cuda") * 4.0            # loud: the stems follow the input's scale, so "rescale" divides
    dl = Delivery(mix=MIX, clip="rescale", peaks="measure")
    for sr in (None, 48000):
        random.seed(8)
        origin, stems = sep.separate_tensor(wav.clone(), sr)
        state = random.getstate()
        want = audio.deliver_mix(origin, stems, MIX, clip="rescale")
        blocks = uneven(wav.cpu(), 9)
        reads = []

        def source():
            reads.append(1)
            return iter(blocks)

        random.seed(8)
        outs = list(sep.separate_blocks(source, sr=sr, deliver=dl))
        assert random.getstate() == state and len(reads) == 3
        for k in want:
            assert torch.equal(cat(outs, k), want[k].cpu()), (sr, k)
        loud = audio.deliver_mix(origin, stems, MIX, clip=None, fmt="f32")
        assert any(float(v.abs().max()) * 1.01 > 1 for v in loud.values())


def test_a_measuring_stream_names_its_gains_and_other_gains_are_refused():
    sep = Separator(small_hd(), device="cuda", shifts=1)
    L = 5 * SR + 9
    wav = track(L, seed=35, device="cuda") * 3.0
    blocks = uneven(wav, 2)
    stats = analysed(sep, blocks)
    dl = Delivery(mix=MIX, clip="rescale", fmt="f32", peaks="measure")
    found = []
    for grouped in (False, True):
        outs, _ = stream_frames(sep, blocks, dl, 4, grouped, stats=stats)
        assert all(o == {} for o in outs[:-1]) and isinstance(outs[-1], TrackPeaks)
        found.append(outs[-1])
    pk = found[0]
    assert found[1] == pk and pk.names == tuple(MIX) and pk.length == L
    assert pk.mix == audio.mix_identity(audio.mix_gains(MIX, sep.model.sources))
    random.seed(4)
    origin, stems = sep.separate_tensor(wav.clone())
    values = audio.deliver_mix(origin, stems, MIX, clip=None, fmt="f32")
    assert [int(values[k].abs().max().view(torch.int32)) for k in MIX] == list(pk.bits)
    want = audio.deliver_mix(origin, stems, MIX, clip="rescale", fmt="f32")
    outs, _ = stream_frames(sep, blocks, dl.with_peaks(pk), 4, stats=stats)
    for k in want:
        assert torch.equal(cat(outs, k), want[k]), k
    other = {**MIX, "practice": {"mix": 1, "vocals": -0.5}}
    with pytest.raises(ValueError, match="other gains"):
        sep.separate_stream(stats=stats, deliver=Delivery(mix=other, clip="rescale", peaks=pk))
    with pytest.raises(ValueError, match="other gains"):
        sep.separate_stream(stats=stats, deliver=Delivery(clip="rescale", peaks=pk))


# ---- 4. groups ---------------------------------------------------------------------------------------------------------------------------
def test_mixing_and_plain_group_streams_equal_their_solo_streams():
    sep = Separator(hd("f32", max_batch=3, channels=4, segment=3), device="cuda", shifts=1)
    lengths = [7 * SR + 3, 6 * SR + 777, 8 * SR + 1, 5 * SR + 40, 7 * SR + 5]
    where = ["cpu", "cuda", "cpu", "cuda", "cpu"]
    mixes = [track(n, seed=80 + i, device=w) * 3.0 for i, (n, w) in enumerate(zip(lengths, where))]
    ident = audio.mix_identity(audio.mix_gains(MIX, sep.model.sources))
    pk = TrackPeaks.from_values(list(MIX), [2.0, 3.0, 1.5, 0.25], mix=ident)
    deliveries = [Delivery(mix=MIX), Delivery("vocals"), Delivery(mix=MIX, clip="rescale", fmt="f32", peaks=pk),
                  Delivery(mix={"a": {"mix": -1}, "b": {"other": 1}}, clip="rescale", peaks="measure"), Delivery(mix=MIX, clip="tanh")]
    script = group_script(lengths, 6)
    want, ws, _ = run_mixed(sep, mixes, deliveries, script, grouped=False)
    got, gs, g = run_mixed(sep, mixes, deliveries, script, grouped=True)
    assert gs == ws and len(got) == len(want)
    peaks_seen = 0
    for c, ((gop, gr), (wop, wr)) in enumerate(zip(got, want)):
        assert gop == wop and list(gr) == list(wr)
        for i in wr:
            if isinstance(wr[i], TrackPeaks):
                assert gr[i] == wr[i] and wr[i].mix is not None
                peaks_seen += 1
                continue
            assert list(gr[i]) == list(wr[i])
            for k in wr[i]:
                assert gr[i][k].device == wr[i][k].device and gr[i][k].dtype == wr[i][k].dtype and same(gr[i][k], wr[i][k]), (c, i, k)
    assert peaks_seen == 1


def census(deliveries, monkeypatch, pushes=12):
    """Library calls per push of a group outside the forwards (tests/test_gpu_deliver_peaks_api.py's census): the worst push's
    total, and per delivery entry the most calls a push made."""
    m = small_ht()
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
    random.seed(9)
    g = Separator(m, device="cuda", shifts=1).separate_stream_group()
    keys = [g.open(0.0, 1.0, deliver=d) for d in deliveries]
    worst, most = 0, Counter()
    gc.collect()
    gc.disable()
    try:
        for _ in range(pushes):
            counts.clear()
            g.push({k: block for k in keys})
            worst = max(worst, sum(v for k, v in counts.items() if k not in PER_FORWARD and not k.endswith("_destroy")))
            for k in MIX_ENTRIES + ("mi_deliver_pcm",):
                most[k] = max(most[k], counts[k])
    finally:
        gc.enable()
    counts.clear()
    g.finish(keys)
    monkeypatch.undo()
    return worst, +most


def test_a_push_with_mixing_streams_is_one_more_launch_whatever_their_number(monkeypatch):
    plain, mp = census([Delivery("vocals")] * 2, monkeypatch)
    assert mp == Counter({"mi_deliver_pcm": 1})
    one, m1 = census([Delivery("vocals")] * 2 + [Delivery(mix=MIX)], monkeypatch)
    many, m3 = census([Delivery("vocals")] * 2 + [Delivery(mix=MIX), Delivery(mix={"x": {"mix": 1, "bass": -1}}, fmt="f32"),
                                                   Delivery(mix=MIX, clip="tanh")], monkeypatch)
    assert one == many == plain + 1
    assert m1 == m3 == Counter({"mi_deliver_pcm": 1, "mi_deliver_mix_pcm": 1})
    alone, ma = census([Delivery(mix=MIX)] * 2, monkeypatch)
    assert alone == plain and ma == Counter({"mi_deliver_mix_pcm": 1})
    measuring, mm = census([Delivery(mix=MIX), Delivery(mix=MIX, clip="rescale", peaks="measure")] * 2, monkeypatch)
    assert measuring == plain + 1 and mm == Counter({"mi_deliver_mix_pcm": 1, "mi_deliver_mix_peaks_update": 1})


def test_the_mix_costs_no_device_memory():
    """The mix is read from the window a stream holds anyway: a remixing stream's device bytes are a plain delivering stream's,
    push for push, solo and in a group, and stop growing with the stream."""
    sep = Separator(small_hd(), device="cuda", shifts=1)
    sizes = {}
    for tag, dl in (("mix", Delivery(mix=MIX)), ("plain", Delivery("vocals"))):
        random.seed(2)
        ss = sep.separate_stream(0.0, 1.0, deliver=dl)
        random.seed(2)
        g = sep.separate_stream_group()
        key = g.open(0.0, 1.0, deliver=dl)
        block = track(ss.stream.members[0].stride // 3, seed=90)
        seen = []
        for _ in range(27):
            ss.push(block)
            g.push({key: block})
            seen.append((ss.stream.device_bytes(), g.group.device_bytes()))
        ss.finish()
        g.finish([key])
        sizes[tag] = seen
    assert sizes["mix"] == sizes["plain"]
    assert sizes["mix"][26][0] == sizes["mix"][14][0] > 0
