"""Host side of gain-weighted remixes (`audio.mix_gains`, `audio.mix_rows`, `audio.deliver_mix`'s layout, `TrackPeaks(mix=...)`,
`Delivery(mix=...)`, demucs_amd/stream.py): what a `mix` accepts and how it is refused -- before `random` is touched and before a
group opens a slot --, how a row is packed, and the header's constants."""
import random
import re

import numpy as np
import pytest
import torch

from demucs_amd import _lib, audio
from demucs_amd.api import Delivery, Separator, TrackPeaks
from demucs_amd.apply import apply_model_stream, apply_model_stream_group
from demucs_amd.stream import _mix_rows
from test_deliver_rate_host import M, SOURCES, engine_model

MIX = {"practice": {"mix": 1, "vocals": 10 ** -0.6 - 1}, "minus_vocals": {"mix": 1, "vocals": -1}, "bass_up": {"bass": 2, "drums": 0}}
F = np.float32


# ---- the gains -----------------------------------------------------------------------------------------------------------------------
def test_gains_are_resolved_per_source_and_rounded_once():
    assert SOURCES == ["drums", "bass", "other", "vocals"]
    got = audio.mix_gains(MIX, SOURCES)
    g = float(F(10 ** -0.6 - 1))
    assert got == [("practice", (1.0, 0.0, 0.0, 0.0, g)), ("minus_vocals", (1.0, 0.0, 0.0, 0.0, -1.0)),
                   ("bass_up", (0.0, 0.0, 2.0, 0.0, 0.0))]
    assert [name for name, _ in got] == list(MIX)                              # dict order
    assert audio.mix_gains(MIX) == [("practice", {"mix": 1.0, "vocals": g}), ("minus_vocals", {"mix": 1.0, "vocals": -1.0}),
                                    ("bass_up", {"bass": 2.0, "drums": 0.0})]
    assert audio.mix_gains({"a": {"vocals": np.float64(0.1)}}, SOURCES)[0][1][4] == float(F(0.1)) != 0.1
    assert audio.mix_outputs(got) == [("practice", None, 0), ("minus_vocals", None, 1), ("bass_up", None, 2)]
    assert audio.mix_identity(got) == tuple(got)


BAD_MIXES = [
    ({}, SOURCES, "non-empty"),
    (None, SOURCES, "non-empty"),
    ([("a", {"mix": 1})], SOURCES, "non-empty"),
    ({"a": {"mix": 1, "piano": 1}}, SOURCES, "'piano'.*neither 'mix' nor one of the separated sources"),
    ({"a": {"mix": 1}}, ["drums", "mix"], "named 'mix'"),
    ({"a": {"vocals": float("nan")}}, SOURCES, "finite"),
    ({"a": {"vocals": float("inf")}}, SOURCES, "finite"),
    ({"a": {"vocals": 1e39}}, SOURCES, "finite in float32"),
    ({"a": {"vocals": 0, "mix": -0.0}}, SOURCES, "every gain of output 'a' is 0"),
    ({"a": {}}, SOURCES, "every gain"),
    ({"a": {"vocals": 1e-60}}, SOURCES, "every gain"),                         # 0 once rounded to float32
    ({"a": {"s0": 1}}, [f"s{i}" for i in range(9)], "at most 8 sources"),
    ({"a": 1.0}, SOURCES, "output 'a' needs"),
    ({"a": {"vocals": "1"}}, SOURCES, "needs"),
    ({"a": {"vocals": True}}, SOURCES, "needs"),
    ({3: {"vocals": 1}}, SOURCES, "output name is a string"),
]


@pytest.mark.parametrize("mix,sources,match", BAD_MIXES)
def test_mix_validation(mix, sources, match):
    with pytest.raises(ValueError, match=match):
        audio.mix_gains(mix, sources)
    with pytest.raises(ValueError, match=match):
        audio.deliver_mix(torch.zeros(2, 8), {k: torch.zeros(2, 8) for k in sources}, mix)      # before any device work


# ---- the rows ------------------------------------------------------------------------------------------------------------------------
def test_a_row_carries_its_gains_bit_exact_the_affine_and_the_pitch():
    gains = audio.mix_gains({"a": {"mix": 0.1, "vocals": -0.7, "drums": 1}, "b": {"other": 1e-30}}, SOURCES)
    offs, total = audio.deliver_layout(audio.mix_outputs(gains), 321, 2, "i16")
    assert offs == [0, 1296] and total == 1296 + 1284                        # deliver's layout: 16-byte boundaries
    rows = audio.mix_rows(gains, 0x7000, 321, 0x9004, 5000, (0.25, 1.5), 2, 6, "i16", offs)
    assert len(rows) == 2 * audio.MIX_COLS
    a, b = rows[:audio.MIX_COLS], rows[audio.MIX_COLS:]
    assert a[:4] == [0x7000, 321, 0x9004, 5000] and a[5] == 1 and a[11:] == [2, 6, 0, 0] and b[11:] == [2, 7, 0, 1296]
    assert np.array(a[4:5], dtype=np.int64).view(F).tolist() == [0.25, 1.5]   # mean low, s high
    packed = np.array(a[6:11], dtype=np.int64).view(F)
    assert packed.tobytes() == np.array([0.1, 1, 0, 0, -0.7, 0, 0, 0, 0, 0], dtype=F).tobytes()
    assert np.array(b[6:11], dtype=np.int64).view(F).tolist() == [0, 0, 0, float(F(1e-30)), 0, 0, 0, 0, 0, 0]
    # no affine: the flag is clear; rows without a destination; "f32"
    free = audio.mix_rows(gains[:1], 0x7000, 8, 0, 0, None, 1, 0, "f32", None)
    assert free[2:6] == [0, 0, 0, 0] and free[11:] == [1, 0, 1, 0]
    # eight sources fill the nine gains
    eight = audio.mix_gains({"x": {f"s{i}": i + 1 for i in range(8)}}, [f"s{i}" for i in range(8)])
    assert np.array(audio.mix_rows(eight, 1, 1, 0, 0, None, 0, 0, "i16", [0])[6:11], dtype=np.int64).view(F).tolist() == \
        [0, 1, 2, 3, 4, 5, 6, 7, 8, 0]


def test_a_stream_row_names_the_window_at_the_emit_point():
    model = engine_model()
    random.seed(1)
    st = apply_model_stream(model, shifts=1, device="cuda", deliver=Delivery(mix=MIX, fmt="f32"))
    assert st.gains == audio.mix_gains(MIX, SOURCES) and [n for n, _, _ in st.outputs] == list(MIX) and st.affine is None
    rows = _mix_rows(st, 0x7000, 100, 5000, 0x100000, 4400, 9000, [0, 800, 1600])
    assert [rows[i * audio.MIX_COLS + 2] for i in range(3)] == [0x100000 + 4 * 600] * 3        # position `emitted` of the window
    assert [rows[i * audio.MIX_COLS + 3] for i in range(3)] == [9000] * 3 and rows[5] == 0
    with pytest.raises(AssertionError, match="past the emit point"):
        _mix_rows(st, 0x7000, 100, 5000, 0x100000, 5001, 9000, [0, 800, 1600])
    # no remix reads the mix: no address, whatever the window
    random.seed(1)
    st = apply_model_stream(model, shifts=1, device="cuda", deliver=Delivery(mix={"b": {"bass": 2}}))
    assert _mix_rows(st, 0x7000, 100, 5000, 0x100000, 5001, 9000, [0])[2] == 0
    # the Separator's affine rides in the row: (float32 mean, float32 std + 1e-8)
    sep = Separator(model, device="cuda", shifts=1)
    ss = sep.separate_stream(0.02, 0.5, deliver=Delivery(mix=MIX))
    row = _mix_rows(ss.stream, 0x7000, 100, 0, 0x100000, 0, 9000, [0, 400, 800])
    assert row[5] == 1 and np.array(row[4:5], dtype=np.int64).view(F).tolist() == [F(0.02), F(0.5) + F(1e-8)]


# ---- TrackPeaks ----------------------------------------------------------------------------------------------------------------------
def test_track_peaks_mix_identity():
    ident = audio.mix_identity(audio.mix_gains(MIX, SOURCES))
    pk = TrackPeaks(list(MIX), [1, 2, 3], mix=ident)
    assert pk.mix == ident and pk.stem is None and "mix=" in repr(pk)
    assert pk == TrackPeaks(list(MIX), [1, 2, 3], mix=[(n, list(g)) for n, g in ident])
    assert hash(pk) == hash(TrackPeaks(list(MIX), [1, 2, 3], mix=ident))
    assert pk != TrackPeaks(list(MIX), [1, 2, 3]) and TrackPeaks(SOURCES, [1, 2, 3, 4]).mix is None
    other = audio.mix_identity(audio.mix_gains({**MIX, "bass_up": {"bass": 3}}, SOURCES))
    assert pk != TrackPeaks(list(MIX), [1, 2, 3], mix=other)
    assert "mix=" not in repr(TrackPeaks(SOURCES, [1, 2, 3, 4]))
    for bad, kw in ((ident[:2], {}), (ident[::-1], {}), ("abc", {}), (ident, dict(stem="vocals")),
                    (tuple((n, g[:1]) for n, g in ident), {}), (tuple((n, (float("nan"),) * 5) for n, _ in ident), {})):
        with pytest.raises(ValueError, match="mix"):
            TrackPeaks(list(MIX) if "stem" not in kw else ["vocals", "no_vocals"], [1, 2, 3][:3 if "stem" not in kw else 2], mix=bad, **kw)


# ---- Delivery ------------------------------------------------------------------------------------------------------------------------
def peaks_for(mix, **kw):
    return TrackPeaks(list(mix), [0x3FC00000] * len(mix), mix=audio.mix_identity(audio.mix_gains(mix, SOURCES)), **kw)


def test_delivery_takes_a_mix_alone():
    dl = Delivery(mix=MIX, fmt="f32")
    assert dl.mix == MIX and dl.mix is not MIX and "mix=" in repr(dl) and "mix=" not in repr(Delivery("vocals"))
    assert dl.outputs(SOURCES) == [("practice", None, 0), ("minus_vocals", None, 1), ("bass_up", None, 2)]
    assert dl.gains(SOURCES) == audio.mix_gains(MIX, SOURCES) and Delivery("vocals").gains(SOURCES) is None
    pk = peaks_for(MIX)
    kept = Delivery(mix=MIX, clip="rescale", peaks="measure").with_peaks(pk)
    assert kept.mix == MIX and kept.peaks is pk and kept.for_stream(SOURCES, True, M, 2) == dl.outputs(SOURCES)
    for kw, match in ((dict(stem="vocals"), "stem=None"), (dict(other_method="minus"), "default other_method"),
                      (dict(other_method="none"), "default other_method"), (dict(samplerate=48000), "model's sample rate only"),
                      (dict(samplerate=M), "model's sample rate only")):
        with pytest.raises(ValueError, match=match):
            Delivery(mix=MIX, **kw)
    for mix, _, match in BAD_MIXES[:1] + BAD_MIXES[2:3] + BAD_MIXES[5:11] + BAD_MIXES[12:]:      # None is "no mix"
        with pytest.raises(ValueError, match=match):
            Delivery(mix=mix)
    # the spellings the existing tests pin stay refused
    with pytest.raises(ValueError, match="minus"):
        Delivery("vocals", "minus").for_stream(SOURCES, True, M, 2)
    with pytest.raises(ValueError, match="Invalid format"):
        Delivery(mix=MIX, fmt="i24")


REFUSALS = [
    (dict(mix={"a": {"piano": 1}}), "'piano'"),
    (dict(mix=MIX, clip="rescale"), "rescale"),
    (dict(mix=MIX, clip="rescale", peaks=peaks_for({"practice": MIX["practice"]})), "other gains"),
    (dict(mix=MIX, clip="rescale", peaks=peaks_for({**MIX, "bass_up": {"bass": 2.5}})), "other gains"),
    (dict(mix=MIX, clip="rescale", peaks=TrackPeaks(list(MIX), [1, 2, 3])), "other gains"),
    (dict(clip="rescale", peaks=TrackPeaks(SOURCES, [1, 2, 3, 4], mix=tuple((n, (0.0, 1.0, 1.0, 1.0, 1.0)) for n in SOURCES))),
     "other gains"),
    (dict(mix=MIX, clip="rescale", peaks=peaks_for(MIX, samplerate=48000)), "measured at 48000"),
]


@pytest.mark.parametrize("kw,match", REFUSALS)
def test_refusals_come_before_random_and_open_no_slot(kw, match, monkeypatch):
    model = engine_model()
    sep = Separator(model, device="cuda", shifts=1)
    calls, touched = [], []

    def source():
        calls.append(1)
        return iter([torch.zeros(2, 100)])

    for name in ("randint", "randrange"):
        monkeypatch.setattr(random, name, lambda *a, _n=name: touched.append(_n) or 0)
    state = random.getstate()
    with pytest.raises(ValueError, match=match):
        next(sep.separate_blocks(source, deliver=Delivery(**kw)))
    with pytest.raises(ValueError, match=match):
        sep.separate_stream(0.0, 1.0, deliver=Delivery(**kw))
    with pytest.raises(ValueError, match=match):
        sep.separate_stream(0.0, 1.0, sr=48000, convert=True, pcm="i16", deliver=Delivery(**kw))
    with pytest.raises(ValueError, match=match):
        apply_model_stream(model, shifts=1, device="cuda", deliver=Delivery(**kw))
    g = sep.separate_stream_group()
    with pytest.raises(ValueError, match=match):
        g.open(0.0, 1.0, deliver=Delivery(**kw))
    g2 = apply_model_stream_group(model, shifts=1, device="cuda")
    with pytest.raises(ValueError, match=match):
        g2.open(deliver=Delivery(**kw))
    assert calls == [] and random.getstate() == state and not touched
    assert g.open_keys == [] and g2.open_keys == []


def test_a_mixing_stream_runs_on_the_gpu_engines_only():
    state = random.getstate()
    with pytest.raises(ValueError, match="GPU engines"):
        Separator(engine_model(), device="cpu", shifts=1).separate_stream(0.0, 1.0, deliver=Delivery(mix=MIX))
    assert random.getstate() == state


def test_a_mixing_stream_draws_the_plain_streams_rng_calls():
    model = engine_model()
    random.seed(4)
    plain = apply_model_stream(model, shifts=1, device="cuda", deliver=Delivery("vocals"))
    want = random.getstate()
    for dl in (Delivery(mix=MIX), Delivery(mix=MIX, clip="rescale", peaks="measure"),
               Delivery(mix=MIX, clip="rescale", peaks=peaks_for(MIX))):
        random.seed(4)
        st = apply_model_stream(model, shifts=1, device="cuda", deliver=dl)
        assert random.getstate() == want and [p.shift for p in st.passes] == [p.shift for p in plain.passes]
        assert st.measure == dl.measures and st.rate is None and st.peak_off is None and len(st.outputs) == 3
    assert plain.gains is None


# ---- the header ----------------------------------------------------------------------------------------------------------------------
def test_constants_match_the_header():
    text = open(re.sub(r"tests.test_deliver_mix_host\.py$", "include/demucs_amd.h", __file__.replace("\\", "/"))).read()
    mix = {k: int(v) for k, v in re.findall(r"#define MI_MIX_([A-Z0-9_]+) (\d+)", text)}
    assert mix == dict(SRC=0, N=1, ORIGIN=2, ORIGIN_PITCH=3, ORIGIN_AFFINE=4, AFFINE_ON=5, GAINS=6, CLIP=11, PEAK=12, FMT=13,
                       DST_OFF=14, COLS=15, MAX_SOURCES=8)
    assert (audio.MIX_COLS, audio.MIX_GAINS_AT, audio.MIX_CLIP_AT, audio.MIX_MAX_SOURCES) == (15, 6, 11, 8)
    # the existing entries' rows are as they were
    dlv = dict(re.findall(r"#define MI_DELIVER_([A-Z0-9_]+) (\d+)", text))
    assert [int(dlv[k]) for k in ("SRC", "ORIGIN", "N", "KIND", "SEL", "CLIP", "PEAK", "FMT", "DST_OFF", "COLS")] == list(range(10))
    sig = _lib.SIGNATURES
    for new, old in (("mi_deliver_mix_pcm", "mi_deliver_pcm"), ("mi_deliver_mix_peaks", "mi_deliver_peaks"),
                     ("mi_deliver_mix_peaks_update", "mi_deliver_peaks_update")):
        assert sig[new] == sig[old] and re.search(r"\bint %s\(" % new, text)
    assert "No kernel uses scratch memory and nothing synchronises with the host" in text
