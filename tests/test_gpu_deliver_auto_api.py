"""Gain automation through the public interface, on the MI355X: `audio.deliver_mix(..., changes=)` on a separated track against
the CPU restatement of tests/test_gpu_deliver_auto.py, and `Delivery(mix=, changes=)` / `change_mix` on solo streams, stream groups,
`Separator.separate_stream` and `separate_blocks` against that whole-track call, bit for bit.  Float32 engines throughout; the small
models and tracks of tests/test_gpu_stream.py."""
import gc
import random
from collections import Counter

import pytest
import torch

from demucs_amd import _lib, audio
from demucs_amd.api import Delivery, Separator
from test_gpu_deliver import frames_of
from test_gpu_deliver_auto import auto_value, gains_along
from test_gpu_deliver_mix_api import analysed, cat
from test_gpu_deliver_peaks_api import PER_FORWARD, small_hd, small_ht, uneven
from test_gpu_deliver_rate import same
from test_gpu_ingest import to_i16
from test_gpu_stream import SR, track

pytestmark = pytest.mark.gpu
SOURCES = ["drums", "bass", "other", "vocals"]
MIX = {"practice": {"mix": 1, "vocals": 10 ** -0.6 - 1},                     # vocals lowered by 12 dB
       "drums_up": {"drums": 1.5, "bass": 1, "other": 1, "vocals": 1.0},
       "quiet_bass": {"bass": 0.1, "drums": 0}}
KARAOKE, SILENCE = {"mix": 1, "vocals": -1}, {}
AUTO_ENTRIES = ("mi_deliver_mix_auto_pcm", "mi_deliver_mix_auto_peaks")
CLIPS = {None: 0, "rescale": 1, "clamp": 2, "tanh": 3}


def changes_for(n, marks=()):
    """A schedule over a track of n frames: vocals out for a chorus and back (ramps), a fade out and in of another output (through
    silence), steps and one-frame ramps at `marks` (emit boundaries, when the caller knows them), and a fade that runs past the
    end.  "quiet_bass" keeps its gains."""
    practice = [(n // 7, n // 16, KARAOKE), (n // 2, n // 16, MIX["practice"]), (n - 1000, 5000, SILENCE)]
    used = 0
    for m in marks:                                         # where the schedule leaves room around the mark
        if all(m - 4 >= a + r for a, r, _ in practice if a <= m) and all(m + 4 <= a for a, _, _ in practice if a > m):
            practice += ([(m, 0, KARAOKE), (m, 2, MIX["practice"])], [(m - 1, 1, KARAOKE), (m, 0, MIX["practice"])],
                         [(m - 3, 7, KARAOKE)])[used % 3]   # at the mark; ending at it; across it
            used += 1
    drums_up = [(0, 0, {"drums": 2}), (3, 1, MIX["drums_up"]), (n // 3, n // 8, SILENCE), (n // 3 + n // 8, 0, SILENCE),
                (n // 3 + n // 4, n // 5, {"mix": 0.5, "drums": 1})]
    return {"practice": practice, "drums_up": drums_up}


def restated(origin, stems, mix, changes, clip, fmt):
    x = torch.stack([stems[k].cpu() for k in SOURCES])
    o = origin.cpu()
    gains = audio.mix_gains(mix, SOURCES)
    sched = audio.mix_changes(changes, gains, SOURCES)
    want = {}
    for name, base in gains:
        g = gains_along(base, sched.get(name, []), 0, x.shape[-1], len(SOURCES))
        want[name] = frames_of(auto_value(x, o, g), CLIPS[clip], int(fmt == "f32"))
    return want


def counting(monkeypatch):
    lib = _lib.load()
    counts = Counter()
    for name in _lib.SIGNATURES:
        real = getattr(lib, name)

        def wrapped(*args, _real=real, _name=name):
            counts[_name] += 1
            return _real(*args)

        monkeypatch.setattr(lib, name, wrapped)
    return counts


# ---- 1. audio.deliver_mix on a whole track -------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def separated():
    g = torch.Generator().manual_seed(13)
    block = (torch.randn(4, 2, SR + 3, generator=g) * 0.45).cuda()
    origin = (torch.randn(2, SR + 3, generator=g) * 0.6).cuda()
    return origin, dict(zip(SOURCES, block))


@pytest.mark.parametrize("fmt", ["i16", "f32"])
def test_deliver_mix_with_changes_equals_the_restatement(separated, fmt):
    origin, stems = separated
    changes = changes_for(SR + 3, marks=(1024, 2048, 30001))
    host = {k: v.cpu() for k, v in stems.items()}
    for clip in ("rescale", "clamp", "tanh", None):
        want = restated(origin, stems, MIX, changes, clip, fmt)
        got = audio.deliver_mix(origin, stems, MIX, clip=clip, fmt=fmt, changes=changes)
        assert list(got) == list(MIX)
        for k in want:
            assert got[k].is_cuda and got[k].shape == (SR + 3, 2) and same(got[k].cpu(), want[k]), (clip, k)
        on_host = audio.deliver_mix(origin.cpu(), host, MIX, clip=clip, fmt=fmt, changes=changes)
        for k in want:
            assert on_host[k].device.type == "cpu" and same(on_host[k], want[k]), (clip, k)
        # the output without a change is the fixed gains', and the others differ from theirs
        fixed = audio.deliver_mix(origin, stems, MIX, clip=clip, fmt=fmt)
        assert torch.equal(got["quiet_bass"], fixed["quiet_bass"]) and not torch.equal(got["practice"], fixed["practice"])
    # only a change reads the mix: it is staged for it
    late = audio.deliver_mix(origin, stems, {"b": {"bass": 1}}, clip=None, fmt=fmt, changes={"b": [(100, 50, {"mix": 1})]})
    assert same(late["b"].cpu(), restated(origin, stems, {"b": {"bass": 1}}, {"b": [(100, 50, {"mix": 1})]}, None, fmt)["b"])


def test_deliver_mix_with_changes_is_one_launch_pair_per_track(separated, monkeypatch):
    origin, stems = separated
    changes = changes_for(SR + 3)
    counts = counting(monkeypatch)
    audio.deliver_mix(origin, stems, MIX, clip="rescale", changes=changes)
    assert counts == Counter({"mi_deliver_mix_auto_peaks": 1, "mi_deliver_mix_auto_pcm": 1})
    counts.clear()
    audio.deliver_mix(origin.cpu(), {k: v.cpu() for k, v in stems.items()}, MIX, clip="tanh", fmt="f32", changes=changes)
    assert counts == Counter({"mi_deliver_mix_auto_pcm": 1})
    for none in (None, {}, {"practice": []}):              # nothing scheduled: today's launches
        counts.clear()
        audio.deliver_mix(origin, stems, MIX, clip="rescale", changes=none)
        assert counts == Counter({"mi_deliver_mix_peaks": 1, "mi_deliver_mix_pcm": 1})
    monkeypatch.undo()


# ---- 2. streams against the whole-track call -----------------------------------------------------------------------------------
def run_stream(sep, blocks, deliver, seed, grouped, live=None, **kw):
    """Every push's and finish's result of one stream over `blocks`, solo or as a group of one, and the frames emitted after each
    call.  `live(call index, emitted, change_mix)` runs before every push and before finish."""
    random.seed(seed)
    if grouped:
        g = sep.separate_stream_group()
        key = g.open(deliver=deliver, **kw)
        push, finish = (lambda b: g.push({key: b})[key]), (lambda: g.finish([key])[key])
        emitted, change = (lambda: g.emitted(key)), (lambda *a, **k: g.change_mix(key, *a, **k))
    else:
        ss = sep.separate_stream(deliver=deliver, **kw)
        push, finish, emitted, change = ss.push, ss.finish, (lambda: ss.emitted), ss.change_mix
    outs, marks = [], []
    for i, b in enumerate(blocks):
        if live is not None:
            live(i, emitted(), change)
        outs.append(push(b))
        marks.append(emitted())
    if live is not None:
        live(len(blocks), emitted(), change)
    outs.append(finish())
    return outs, marks


@pytest.fixture(scope="module")
def hd_track():
    sep = Separator(small_hd(), device="cuda", shifts=1)
    L = 7 * SR + 777                                        # longer than a segment: the window is trimmed along the way
    wav = track(L, seed=31, device="cuda") * 0.8
    random.seed(5)
    origin, stems = sep.separate_tensor(wav.clone())
    return sep, wav, origin, stems, random.getstate()


@pytest.mark.parametrize("grouped", [False, True])
def test_stream_frames_equal_the_whole_track_call_for_any_partition(hd_track, grouped):
    """Changes inside, at and across emit boundaries: the boundaries of each partition are found by a run of the fixed gains, then
    steps, one- and two-frame ramps are put on them, beside ramps of half a second and more that span several calls."""
    sep, wav, origin, stems, state = hd_track
    for seed, clip, fmt in ((4, "clamp", "i16"), (7, "tanh", "f32")):
        blocks = uneven(wav.cpu(), seed)
        stats = analysed(sep, blocks)
        _, marks = run_stream(sep, blocks, Delivery(mix=MIX, clip=clip, fmt=fmt), 5, grouped, stats=stats)
        inner = sorted({m for m in marks if 0 < m < wav.shape[1]})
        assert len(inner) >= 2
        changes = changes_for(wav.shape[1], marks=inner)
        every = [c for rows in changes.values() for c in rows]
        assert any(a == m for m in inner for a, _, _ in every) and any(a < m < a + r for m in inner for a, r, _ in every)
        want = audio.deliver_mix(origin, stems, MIX, clip=clip, fmt=fmt, changes=changes)
        outs, again = run_stream(sep, blocks, Delivery(mix=MIX, clip=clip, fmt=fmt, changes=changes), 5, grouped, stats=stats)
        assert again == marks and random.getstate() == state and all(list(o) == list(MIX) for o in outs)
        for k in want:
            got = cat(outs, k)
            assert got.device.type == "cpu" and got.dtype == want[k].dtype and same(got, want[k].cpu()), (seed, k)
        assert not same(cat(outs, "practice"), audio.deliver_mix(origin, stems, MIX, clip=clip, fmt=fmt)["practice"].cpu())


def test_int16_feed_and_device_blocks():
    sep = Separator(small_hd(), device="cuda", shifts=1)
    L = 6 * SR + 41
    q, floats = to_i16(track(L, seed=32) * 0.9)
    random.seed(6)
    origin, stems = sep.separate_tensor(floats.cuda())
    changes = changes_for(L, marks=(2 * SR, 4 * SR + 1))
    want = audio.deliver_mix(origin, stems, MIX, clip="clamp", fmt="i16", changes=changes)
    cuts = [0, 1, 1, SR // 3, 2 * SR + 5, 2 * SR + 5, 5 * SR, L]
    for where in ("cpu", "cuda"):
        blocks = [q[a:b].to(where) for a, b in zip(cuts[:-1], cuts[1:])]
        stats = analysed(sep, blocks, pcm="i16")
        for grouped in (False, True):
            outs, _ = run_stream(sep, blocks, Delivery(mix=MIX, changes=changes), 6, grouped, stats=stats, pcm="i16")
            for k in want:
                got = cat(outs, k)
                assert got.device.type == where and torch.equal(got.cpu(), want[k].cpu()), (where, grouped, k)


@pytest.mark.parametrize("grouped", [False, True])
def test_live_changes_equal_the_same_changes_given_at_open(hd_track, grouped):
    sep, wav, origin, stems, _ = hd_track
    L = wav.shape[1]
    cuts = [0, 1, SR, SR, 2 * SR + 5, 3 * SR, 3 * SR + 1, 5 * SR, 6 * SR + 100, L]
    blocks = [wav[:, a:b].cpu() for a, b in zip(cuts[:-1], cuts[1:])]
    stats = analysed(sep, blocks)
    made = {"practice": [], "drums_up": []}
    # before the call with this index (9: before finish): the outputs' new gains, the ramp
    plan = {5: ({"practice": KARAOKE}, 0), 6: ({"drums_up": SILENCE, "practice": MIX["practice"]}, SR // 3),
            7: ({"drums_up": MIX["drums_up"]}, 1), 8: ({"practice": SILENCE}, 3 * SR), 9: ({"practice": KARAOKE, "drums_up": {"mix": 0.5}}, 100)}

    def live(i, emitted, change):
        if i not in plan:
            return
        mix, ramp = plan[i]
        ends = {k: max([emitted] + [a + r for a, r, _ in made[k][-1:]]) for k in mix}
        if i == 6:                                          # one change named by its position, ahead of everything delivered
            at = max(ends.values()) + 1234
            change(mix, at=at, ramp=ramp)
            ends = {k: at for k in mix}
        else:                                               # at=None: at `emitted`, or where the output's last ramp ends
            change(mix, ramp=ramp)
        for k, g in mix.items():
            made[k].append((ends[k], ramp, g))

    outs, _ = run_stream(sep, blocks, Delivery(mix=MIX, fmt="f32"), 5, grouped, live=live, stats=stats)
    assert sum(len(v) for v in made.values()) == 7 and 0 < made["practice"][0][0] < made["practice"][1][0] < L
    want = audio.deliver_mix(origin, stems, MIX, clip="clamp", fmt="f32", changes=made)
    at_open, _ = run_stream(sep, blocks, Delivery(mix=MIX, fmt="f32", changes=made), 5, grouped, stats=stats)
    for k in want:
        assert same(cat(outs, k), want[k].cpu()) and same(cat(at_open, k), want[k].cpu()), k
        assert [o[k].shape for o in outs] == [o[k].shape for o in at_open]
    # the first change landed at `emitted`: the frames before it are the fixed gains', the first one after it is not
    fixed = audio.deliver_mix(origin, stems, MIX, clip="clamp", fmt="f32")["practice"].cpu()
    first = made["practice"][0][0]
    assert torch.equal(cat(outs, "practice")[:first], fixed[:first]) and not torch.equal(cat(outs, "practice")[first], fixed[first])


def test_separate_blocks_takes_a_schedule_at_open():
    sep = Separator(small_hd(), device="cuda", shifts=1)
    L = 5 * SR + 5
    wav = track(L, seed=33, device="cuda")
    for sr in (None, 48000):
        random.seed(8)
        origin, stems = sep.separate_tensor(wav.clone(), sr)
        state = random.getstate()
        n = origin.shape[-1]                                # the schedule counts delivered (model-rate) frames
        changes = changes_for(n, marks=(SR, 2 * SR + 7))
        want = audio.deliver_mix(origin, stems, MIX, clip="tanh", changes=changes)
        random.seed(8)
        outs = list(sep.separate_blocks(lambda: iter(uneven(wav.cpu(), 9)), sr=sr, deliver=Delivery(mix=MIX, clip="tanh", changes=changes)))
        assert random.getstate() == state
        for k in want:
            assert torch.equal(cat(outs, k), want[k].cpu()), (sr, k)
    with pytest.raises(ValueError, match="gain changes"):
        next(sep.separate_blocks(lambda: iter([]), deliver=Delivery(mix=MIX, clip="rescale", peaks="measure", changes=changes)))


# ---- 3. launches ---------------------------------------------------------------------------------------------------------------
def census(deliveries, monkeypatch, pushes=12, live=None):
    """Library calls per push of a group outside the forwards (tests/test_gpu_deliver_mix_api.py's census): the worst push's total,
    and per push the calls of the remix entries."""
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
    worst, per_push = 0, []                                 # per push: the streams that emitted, the remix entries' calls
    gc.collect()
    gc.disable()
    try:
        for i in range(pushes):
            if live is not None:
                live(i, g, keys)
            counts.clear()
            out = g.push({k: block for k in keys})
            worst = max(worst, sum(v for k, v in counts.items() if k not in PER_FORWARD and not k.endswith("_destroy")))
            emits = [i for i, k in enumerate(keys) if any(v.shape[0] > 0 for v in out[k].values())]
            per_push.append((emits, {k: counts[k] for k in ("mi_deliver_pcm", "mi_deliver_mix_pcm") + AUTO_ENTRIES if counts[k]}))
    finally:
        gc.enable()
    counts.clear()
    g.finish(keys)
    monkeypatch.undo()
    return worst, per_push


ENTRY = {"pcm": "mi_deliver_pcm", "mix": "mi_deliver_mix_pcm", "auto": "mi_deliver_mix_auto_pcm"}


def launches(kinds, emits):
    """One launch of an entry for all the streams of its kind that emitted on the push, none when none did."""
    return {ENTRY[k]: 1 for k in {kinds[i] for i in emits}}


def test_a_push_with_automated_streams_is_one_more_launch_whatever_their_number(monkeypatch):
    changes = changes_for(12 * SR)
    auto = Delivery(mix=MIX, changes=changes)
    plain, pp = census([Delivery("vocals")] * 2, monkeypatch)
    assert any(e for e, _ in pp) and all(c == launches(["pcm"] * 2, e) for e, c in pp)
    one, p1 = census([Delivery("vocals")] * 2 + [auto], monkeypatch)
    many, p3 = census([Delivery("vocals")] * 2 + [auto, Delivery(mix={"x": {"bass": 1}}, fmt="f32", changes={"x": [(5, 9, {"mix": 1})]}),
                                                   Delivery(mix=MIX, clip="tanh", changes=changes)], monkeypatch)
    assert one == many == plain + 1
    assert all(c == launches(["pcm"] * 2 + ["auto"] * 3, e) for e, c in p1 + p3) and any(len(e) == 5 for e, _ in p3)
    # beside streams of fixed gains: one launch for those, one for the automated
    both, pb = census([Delivery(mix=MIX), auto, Delivery(mix=MIX, fmt="f32"), auto], monkeypatch)
    assert both == plain + 1 and all(c == launches(["mix", "auto"] * 2, e) for e, c in pb) and any(len(e) == 4 for e, _ in pb)


def test_a_stream_without_a_change_never_calls_the_new_entries(monkeypatch):
    _, fixed = census([Delivery(mix=MIX)] * 2, monkeypatch, pushes=18)
    assert any(e for e, _ in fixed) and all(c == launches(["mix"] * 2, e) for e, c in fixed)
    # from its first change on a stream's rows go to the new entry, those of its neighbour stay where they were
    emitting = [i for i, (e, _) in enumerate(fixed) if 0 in e]
    assert len(emitting) >= 2
    first = emitting[0]

    def live(i, g, keys):
        if i == first + 1:
            g.change_mix(keys[0], {"practice": KARAOKE}, ramp=SR)

    _, seen = census([Delivery(mix=MIX)] * 2, monkeypatch, pushes=18, live=live)
    assert [e for e, _ in seen] == [e for e, _ in fixed]
    for i, (e, c) in enumerate(seen):
        assert c == launches(["mix" if i <= first else "auto", "mix"], e), i
    assert any(0 in e for e, _ in seen[first + 1:])
    # a solo stream: the fixed gains' entry until the change, the new one after it, one launch a push either way
    sep = Separator(small_hd(), device="cuda", shifts=1)
    random.seed(2)
    ss = sep.separate_stream(0.0, 1.0, deliver=Delivery(mix=MIX))
    counts = counting(monkeypatch)
    block = track(SR, seed=51)
    before = [ss.push(block)["practice"].shape[0] for _ in range(5)]
    assert sum(n > 0 for n in before) == counts["mi_deliver_mix_pcm"] > 0 and not any(counts[k] for k in AUTO_ENTRIES)
    ss.change_mix({"practice": KARAOKE})
    counts.clear()
    after = [ss.push(block)["practice"].shape[0] for _ in range(3)] + [ss.finish()["practice"].shape[0]]
    assert sum(n > 0 for n in after) == counts["mi_deliver_mix_auto_pcm"] > 0 and counts["mi_deliver_mix_pcm"] == 0
    monkeypatch.undo()
