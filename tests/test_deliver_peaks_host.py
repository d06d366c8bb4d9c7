"""Host side of `clip="rescale"` on a stream (`audio.TrackPeaks`, `Delivery(clip="rescale", peaks=...)`, demucs_amd/stream.py):
what a `TrackPeaks` accepts, every refusal of a rescaling stream -- before `source()` is called and before `random` is touched --
and the header's constants."""
import random
import re

import numpy as np
import pytest
import torch

from demucs_amd import _lib, audio
from demucs_amd.api import Delivery, Separator, TrackPeaks
from demucs_amd.apply import apply_model_stream, apply_model_stream_group
from demucs_amd.stream import _deliver_rows, _packed_slots
from test_deliver_rate_host import M, SOURCES, engine_model
from test_stream_host import Refusing


def bits_of(v) -> int:
    return int(np.float32(v).view(np.uint32))


# ---- TrackPeaks -------------------------------------------------------------------------------------------------------------------
def test_track_peaks_holds_what_a_measuring_pass_found():
    pk = TrackPeaks(SOURCES, [bits_of(0.5), 0, bits_of(2.0), 0x7FC00000], length=1000)
    assert pk is not None and audio.TrackPeaks is TrackPeaks
    assert pk.names == tuple(SOURCES) and pk.bits == (0x3F000000, 0, 0x40000000, 0x7FC00000)
    assert (pk.samplerate, pk.stem, pk.other_method, pk.length) == (None, None, "add", 1000)
    assert pk.peak("other") == np.float32(2.0) and np.isnan(pk.peak("vocals"))
    # clip_divisor of post_ops.h: one float32 product
    assert pk.divisor("other") == np.float32(2.0) * np.float32(1.01) and pk.divisor("other").dtype == np.float32
    assert pk.divisor("bass") == 0 and np.isnan(pk.divisor("vocals"))
    two = TrackPeaks(["vocals", "no_vocals"], [1, 2], samplerate=48000, stem="vocals")
    assert two == TrackPeaks(("vocals", "no_vocals"), (1, 2), 48000, "vocals", "add", 1) and hash(two) == hash(two)
    assert two != TrackPeaks(["vocals", "no_vocals"], [1, 3], samplerate=48000, stem="vocals")
    assert TrackPeaks(["bass"], [5], stem="bass", other_method="none").names == ("bass",)
    assert TrackPeaks.from_values(SOURCES, [0.5, -0.0, -2.0, float("nan")]).bits[:3] == pk.bits[:3]
    with pytest.raises(AttributeError):
        pk.bits = (1, 2, 3, 4)
    assert "0x40000000" in repr(pk)


@pytest.mark.parametrize("names,bits,kw,match", [
    (SOURCES, [1, 2, 3], {}, "4 outputs need 4 peaks"),                           # wrong count
    (SOURCES, [1, 2, 3, 4, 5], {}, "4 outputs need 4 peaks"),
    (SOURCES, [0.5, 1, 2, 3], {}, "bit pattern"),                                 # a float is not its bit pattern
    (SOURCES, [np.float32(1.0), 1, 2, 3], {}, "bit pattern"),
    (SOURCES, [True, 1, 2, 3], {}, "bit pattern"),
    (SOURCES, ["1", 1, 2, 3], {}, "bit pattern"),
    (SOURCES, [-1, 1, 2, 3], {}, "bit pattern"),
    (SOURCES, [1 << 32, 1, 2, 3], {}, "bit pattern"),
    (SOURCES, [0x80000001, 1, 2, 3], {}, "sign bit"),                             # a peak is a magnitude
    (SOURCES, 7, {}, "sequence"),
    ("vocals", [1], {}, "names"),
    ([], [], {}, "names"),
    (["a", "a"], [1, 2], {}, "names"),
    (["no_vocals", "vocals"], [1, 2], dict(stem="vocals"), "save order"),         # not delivery_outputs' order
    (["vocals"], [1], dict(stem="vocals"), "save order"),                         # "add" has two outputs
    (["vocals", "no_vocals"], [1, 2], dict(stem="vocals", other_method="none"), "save order"),
    (["minus_vocals", "vocals"], [1, 2], dict(stem="vocals", other_method="add"), "save order"),
    (["vocals", "no_vocals"], [1, 2], dict(stem="vocals", other_method="sub"), "other_method"),
    (SOURCES, [1, 2, 3, 4], dict(samplerate=0), "samplerate"),
    (SOURCES, [1, 2, 3, 4], dict(samplerate=48000.0), "samplerate"),
    (SOURCES, [1, 2, 3, 4], dict(length=0), "length"),
    (SOURCES, [1, 2, 3, 4], dict(length=2.5), "length"),
])
def test_track_peaks_validation(names, bits, kw, match):
    with pytest.raises(ValueError, match=match):
        TrackPeaks(names, bits, **kw)


def test_two_stems_names_are_delivery_outputs_names():
    for stem in SOURCES:
        for method in ("add", "none"):
            names = [n for n, _, _ in audio.delivery_outputs(SOURCES, stem, method)]
            assert TrackPeaks(names, [0] * len(names), stem=stem, other_method=method).names == tuple(names)


# ---- Delivery ---------------------------------------------------------------------------------------------------------------------
def test_delivery_takes_peaks_only_with_rescale():
    pk = TrackPeaks(SOURCES, [1, 2, 3, 4])
    for clip in ("clamp", "tanh", None):
        with pytest.raises(ValueError, match="rescale"):
            Delivery(clip=clip, peaks="measure")
        with pytest.raises(ValueError, match="rescale"):
            Delivery(clip=clip, peaks=pk)
    with pytest.raises(ValueError, match="rescale"):
        Delivery(peaks="measure")                                                 # the default clip is "clamp"
    for bad in ("measured", 3, [1, 2], {"a": 1}):
        with pytest.raises(ValueError, match="peaks must be"):
            Delivery(clip="rescale", peaks=bad)
    m = Delivery("vocals", clip="rescale", fmt="f32", samplerate=48000, peaks="measure")
    assert m.measures and "peaks='measure'" in repr(m)
    d = m.with_peaks(TrackPeaks(["vocals", "no_vocals"], [1, 2], samplerate=48000, stem="vocals"))
    assert not d.measures and (d.stem, d.other_method, d.clip, d.fmt, d.samplerate) == ("vocals", "add", "rescale", "f32", 48000)
    assert not Delivery("vocals").measures and Delivery("vocals").peaks is None


def test_a_rescaling_row_names_its_peak_slot():
    pk = TrackPeaks(["vocals", "no_vocals"], [1, 2], stem="vocals")
    dl = Delivery("vocals", clip="rescale", peaks=pk)
    outs = dl.for_stream(SOURCES, True, M, 2)
    assert _deliver_rows(outs, dl, 0x7000, 321, [0, 1296], 6) == [0x7000, 0, 321, 0, 3, 1, 6, 0, 0, 0x7000, 0, 321, 1, 3, 1, 7, 0, 1296]
    # a measuring stream's rows name no destination
    ms = Delivery("vocals", clip="rescale", peaks="measure")
    assert _deliver_rows(outs, ms, 0x7000, 321, None, 2) == [0x7000, 0, 321, 0, 3, 1, 2, 0, 0, 0x7000, 0, 321, 1, 3, 1, 3, 0, 0]
    # int32 slots ride in the int64 table, two a word
    packed = np.array(_packed_slots([3, -1, 7]), dtype=np.int64).view(np.int32)
    assert packed.tolist() == [3, -1, 7, 0]
    assert _packed_slots([]) == []


def peaks_for(**kw):
    names = [n for n, _, _ in audio.delivery_outputs(SOURCES, kw.get("stem"), kw.get("other_method", "add"))]
    return TrackPeaks(names, [bits_of(1.5)] * len(names), **kw)


REFUSALS = [
    (dict(clip="rescale"), "rescale"),                                                            # no peaks: today's refusal
    (dict(stem="vocals", clip="rescale", samplerate=48000), "rescale"),
    (dict(stem="vocals", other_method="minus", clip="rescale", peaks="measure"), "minus"),
    (dict(stem="vocals", other_method="minus", clip="rescale",
          peaks=TrackPeaks(["minus_vocals", "vocals"], [1, 2], stem="vocals", other_method="minus")), "minus"),
    (dict(stem="vocals", clip="rescale", peaks=peaks_for(stem="bass")), "measured for the outputs"),      # another stem
    (dict(stem="vocals", clip="rescale", peaks=peaks_for(stem="vocals", other_method="none")), "measured for"),   # another method
    (dict(stem="vocals", other_method="none", clip="rescale", peaks=peaks_for(stem="vocals")), "measured for"),
    (dict(clip="rescale", peaks=peaks_for(stem="vocals")), "measured for"),
    (dict(clip="rescale", peaks=TrackPeaks(SOURCES[::-1], [1, 2, 3, 4])), "measured for the outputs"),    # another order
    (dict(clip="rescale", peaks=peaks_for(samplerate=48000)), "measured at 48000"),                        # another rate
    (dict(clip="rescale", samplerate=48000, peaks=peaks_for()), "measured at the model's rate"),
    (dict(clip="rescale", samplerate=48000, peaks=peaks_for(samplerate=16000)), "measured at 16000"),
    (dict(clip="rescale", samplerate=44101, peaks="measure"), "44100 -> 44101"),
]


@pytest.mark.parametrize("kw,match", REFUSALS)
def test_refusals_come_before_the_source_and_before_random(kw, match, monkeypatch):
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


@pytest.mark.parametrize("make,device", [(engine_model, "cpu"), (Refusing, "cpu"), (Refusing, "cuda")])
def test_a_measuring_stream_runs_on_the_gpu_engines(make, device):
    sep = Separator(make(), device=device, shifts=1)
    stem = "a" if make is Refusing else "vocals"
    state = random.getstate()
    with pytest.raises(ValueError, match="GPU engines"):
        sep.separate_stream(0.0, 1.0, deliver=Delivery(stem, clip="rescale", peaks="measure"))
    assert random.getstate() == state


def test_matching_peaks_open_a_stream_without_a_gpu():
    """The same peaks at the model's rate named or not; the RNG calls of a rescaling stream are those of any other."""
    model = engine_model()
    random.seed(4)
    plain = apply_model_stream(model, shifts=1, device="cuda", deliver=Delivery("vocals"))
    want = random.getstate()
    for dl in (Delivery("vocals", clip="rescale", peaks="measure"),
               Delivery("vocals", clip="rescale", peaks=peaks_for(stem="vocals")),
               Delivery("vocals", clip="rescale", samplerate=M, peaks=peaks_for(stem="vocals")),
               Delivery("vocals", clip="rescale", peaks=peaks_for(stem="vocals", samplerate=M)),
               Delivery("vocals", clip="rescale", samplerate=48000, peaks=peaks_for(stem="vocals", samplerate=48000))):
        random.seed(4)
        st = apply_model_stream(model, shifts=1, device="cuda", deliver=dl)
        assert random.getstate() == want and st.outputs == plain.outputs
        assert st.measure == dl.measures and st.peak_off is None and (st.rate is not None) == (dl.samplerate == 48000)
    assert not plain.measure


# ---- the header ---------------------------------------------------------------------------------------------------------------------
def test_constants_match_the_header():
    text = open(re.sub(r"tests.test_deliver_peaks_host\.py$", "include/demucs_amd.h", __file__.replace("\\", "/"))).read()
    rate = dict(re.findall(r"#define MI_RATE_([A-Z0-9_]+) (\d+)", text))
    dlv = dict(re.findall(r"#define MI_DELIVER_([A-Z0-9_]+) (\d+)", text))
    clip = dict(re.findall(r"#define MI_CLIP_([A-Z0-9_]+) (\d+)", text))
    assert int(rate["COLS"]) == audio.RATE_COLS == 20 and int(dlv["COLS"]) == audio.DELIVER_COLS == 9
    assert [int(dlv[k]) for k in ("SRC", "ORIGIN", "N", "KIND", "SEL", "CLIP", "PEAK", "FMT", "DST_OFF")] == list(range(9))
    assert (int(rate["CLIP"]), int(rate["FMT"]), int(rate["DST_OFF"])) == (5, 6, 19)
    assert int(clip["RESCALE"]) == audio.clip_code("rescale") == 1
    assert (int(clip["CLAMP"]), int(clip["TANH"])) == (audio.clip_code("clamp"), audio.clip_code("tanh")) == (2, 3)
    sig = _lib.SIGNATURES
    assert len(sig["mi_deliver_peaks_update"][1]) == len(sig["mi_deliver_peaks"][1]) - 1 == 8
    assert len(sig["mi_deliver_resample_pcm"][1]) == 13                            # unchanged
    assert len(sig["mi_deliver_resample_peaks"][1]) == 13 - 2 + 3 and len(sig["mi_deliver_resample_pcm_peaks"][1]) == 13 + 3
    for name in ("mi_deliver_peaks_update", "mi_deliver_resample_peaks", "mi_deliver_resample_pcm_peaks"):
        assert re.search(r"\bint %s\(" % name, text)
