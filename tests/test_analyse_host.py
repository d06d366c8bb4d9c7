"""Host logic of the streaming track statistics without a GPU: `audio.TrackStats`, the `stats=` keyword of
`Separator.separate_stream`, `SeparatorStreamGroup.open`, `ModelStream` and `StreamGroup.open`, and the refusals of
`Separator.analyse_stream` and `audio.MonoStatsStream` that need no device."""
import math
import random

import numpy as np
import pytest
import torch

from demucs_amd import _lib, audio
from demucs_amd.api import Separator
from demucs_amd.audio import MonoStatsStream, TrackStats
from demucs_amd.stream import ModelStream, StreamGroup
from test_apply_host import ToyModel
from test_convert_stream_host import Refusing1, Refusing4
from test_stream_host import Refusing

MEAN, S = float(np.float32(0.0123)), float(np.float32(0.3217))


# ---- TrackStats -------------------------------------------------------------------------------------------------------------------
def test_track_stats_holds_its_values_and_is_immutable():
    st = TrackStats(np.float32(0.0123), np.float32(0.3217), 1000)
    assert (st.mean, st.s, st.length, st.input_length) == (MEAN, S, 1000, 1000)
    assert type(st.mean) is float and type(st.s) is float and type(st.length) is int
    assert TrackStats(MEAN, S, 919, 1000).input_length == 1000
    assert st == TrackStats(MEAN, S, 1000, 1000) and hash(st) == hash(TrackStats(MEAN, S, 1000))
    assert st != TrackStats(MEAN, S, 1000, 1001)
    for name in ("mean", "s", "length", "input_length", "other"):
        with pytest.raises(AttributeError):
            setattr(st, name, 1)
    with pytest.raises(AttributeError):
        del st.mean
    assert repr(st) == f"TrackStats(mean={MEAN!r}, s={S!r}, length=1000, input_length=1000)"


def test_track_stats_of_one_sample_has_a_nan_normaliser():
    st = TrackStats(0.5, float("nan"), 1)
    assert math.isnan(st.s) and st == TrackStats(0.5, float("nan"), 1)


@pytest.mark.parametrize("args,match", [
    ((0.1, S, 10), "mean must be a float32 value"),            # 0.1 is not a float32: the kernel cannot have written it
    ((MEAN, 0.3217, 10), "s must be a float32 value"),
    ((MEAN, 1e300, 10), "s must be a float32 value"),
    (("0", S, 10), "mean must be a real number"),
    ((MEAN, None, 10), "s must be a real number"),
    ((True, S, 10), "mean must be a real number"),
    ((torch.tensor(0.0), S, 10), "mean must be a real number"),
    ((MEAN, S, 0), "length must be a positive integer"),
    ((MEAN, S, -3), "length must be a positive integer"),
    ((MEAN, S, 10.0), "length must be a positive integer"),
    ((MEAN, S, True), "length must be a positive integer"),
    ((MEAN, S, 10, 0), "input_length must be a positive integer"),
    ((MEAN, S, 10, 2.5), "input_length must be a positive integer"),
])
def test_track_stats_validation(args, match):
    with pytest.raises(ValueError, match=match):
        TrackStats(*args)


# ---- stats= ------------------------------------------------------------------------------------------------------------------------
def test_stats_become_the_affine_as_they_are():
    """`mean=` / `std=` add 1e-8 to std in float32; `stats=` names the normaliser itself.  1e-8 is above half an ulp of s here, so
    the two routes are told apart."""
    s = float(np.float32(1e-7))
    assert float(np.float32(s) + np.float32(1e-8)) != s
    st = ModelStream(Refusing(), shifts=0, stats=TrackStats(MEAN, s, 77))
    assert st.affine == (MEAN, s)
    old = ModelStream(Refusing(), shifts=0, affine=(MEAN, s))
    assert old.affine == (MEAN, float(np.float32(s) + np.float32(1e-8)))
    sep = Separator(Refusing(), device="cpu", shifts=0)
    assert sep.separate_stream(stats=TrackStats(MEAN, s, 77)).stream.affine == (MEAN, s)
    g = sep.separate_stream_group()
    key = g.open(stats=TrackStats(MEAN, s, 77))
    assert g.group._stream(key).affine == (MEAN, s) and g.group._stream(key).length == 77
    nan = ModelStream(Refusing(), shifts=0, stats=TrackStats(0.5, float("nan"), 1))
    assert nan.affine[0] == 0.5 and math.isnan(nan.affine[1])


def test_stats_together_with_mean_or_std_is_refused():
    sep = Separator(Refusing(), device="cpu", shifts=1)
    stats = TrackStats(MEAN, S, 500)
    state = random.getstate()
    for kw in (dict(mean=0.0, std=1.0), dict(mean=0.0), dict(std=1.0)):
        with pytest.raises(ValueError):
            sep.separate_stream(stats=stats, **kw)
    with pytest.raises(ValueError, match="stats, or mean and std, not both"):
        sep.separate_stream(0.0, 1.0, stats=stats)
    with pytest.raises(ValueError, match="stats, or mean and std, not both"):
        sep.separate_stream_group().open(0.0, 1.0, stats=stats)
    with pytest.raises(ValueError, match="stats, or mean and std, not both"):
        ModelStream(Refusing(), shifts=0, affine=(0.0, 1.0), stats=stats)
    with pytest.raises(ValueError, match="stats, or mean and std, not both"):
        StreamGroup(Refusing(), shifts=0).open(affine=(0.0, 1.0), stats=stats)
    with pytest.raises(ValueError, match="TrackStats"):
        sep.separate_stream(stats=(MEAN, S))
    assert random.getstate() == state


def test_length_defaults_to_the_input_length():
    sep = Separator(Refusing(), device="cpu", shifts=1)
    random.seed(4)
    ss = sep.separate_stream(stats=TrackStats(MEAN, S, 919, 919))
    drawn = random.getstate()
    assert ss.stream.length == 919 and ss.stream.predrawn
    random.seed(4)
    assert sep.separate_stream(MEAN, S, length=919).stream.length == 919
    assert random.getstate() == drawn                        # the same RNG calls as the stream with a declared length
    assert sep.separate_stream(stats=TrackStats(MEAN, S, 919), length=500).stream.length == 500      # a given length stands
    g = sep.separate_stream_group()
    key = g.open(stats=TrackStats(MEAN, S, 919), length=500)
    assert g.group._stream(key).length == 500


def test_a_stream_with_stats_normalises_as_the_mean_std_route_on_the_same_normaliser():
    """On the plain-torch route: stems of `stats=(mean, s)` equal those of `mean=, std=` when float32(std) + 1e-8 == s."""
    std = float(np.float32(0.5))
    s = float(np.float32(std) + np.float32(1e-8))
    assert s == std                                          # 1e-8 is far below half an ulp of 0.5
    x = torch.from_numpy(np.random.default_rng(0).standard_normal((2, 950)).astype(np.float32))
    outs = []
    for kw in (dict(mean=MEAN, std=std), dict(stats=TrackStats(MEAN, s, 950))):
        sep = Separator(ToyModel(), device="cpu", shifts=0)
        ss = sep.separate_stream(**kw)
        parts = [ss.push(x[:, :450]), ss.push(x[:, 450:]), ss.finish()]
        outs.append({k: torch.cat([p[k] for p in parts], -1) for k in parts[0]})
    for k in outs[0]:
        assert outs[0][k].shape == (2, 950) and torch.equal(outs[0][k], outs[1][k])


# ---- analyse_stream / MonoStatsStream: what needs no device ----------------------------------------------------------------------------
@pytest.mark.parametrize("model,kw", [
    (Refusing, dict(sr=0, convert=True)),
    (Refusing, dict(sr=-48000, convert=True)),
    (Refusing1, dict(sr=100, channels=2, convert=True)),
    (Refusing4, dict(sr=100, channels=3, convert=True)),
    (Refusing, dict(sr=48000, convert=True)),
    (Refusing, dict(sr=100, channels=1, convert=True)),
    (Refusing, dict(sr=48000)),
    (Refusing, dict(channels=1)),
    (Refusing, dict(pcm="i8")),
    (Refusing, dict(pcm="i16")),
    (Refusing, dict(pcm="i16", sr=48000, channels=1, convert=True)),
])
def test_analyse_stream_refuses_what_separate_stream_refuses(model, kw):
    sep = Separator(model(), device="cpu", shifts=1)
    state = random.getstate()
    with pytest.raises(ValueError) as want:
        sep.separate_stream(0.0, 1.0, **kw)
    with pytest.raises(ValueError) as got:
        sep.analyse_stream(**kw)
    assert str(got.value) == str(want.value)
    assert random.getstate() == state


def test_no_cpu_statistics():
    with pytest.raises(_lib.EngineError):
        MonoStatsStream(2, device="cpu")
    with pytest.raises(_lib.EngineError):
        Separator(ToyModel(), device="cpu").analyse_stream()
    with pytest.raises(ValueError, match="channels"):
        MonoStatsStream(0)
    with pytest.raises(ValueError, match="src_channels"):
        MonoStatsStream(2, pcm="i16")
    with pytest.raises(ValueError, match="less channels"):
        MonoStatsStream(4, pcm="i16", src_channels=3)
    with pytest.raises(ValueError, match="Invalid PCM format"):
        MonoStatsStream(2, pcm="u8", src_channels=2)


def test_finish_without_samples_and_push_after_finish_are_refused():
    """Neither reaches the device: nothing was pushed, so no state exists."""
    st = MonoStatsStream(2, device="cuda", pcm="i16", src_channels=2)
    st.push(b"")                                             # no whole frame: no device work
    st.push(b"\x01\x02\x03")
    assert st.pushed == 0 and st.trailing_bytes == 3 and st.device_bytes() == 0
    with pytest.raises(ValueError, match="before any sample"):
        st.finish()
    assert not st.finished
    planar = MonoStatsStream(2, device="cuda")
    with pytest.raises(ValueError, match=r"expected a \(2, n\) block"):
        planar.push(torch.zeros(3, 10))
    with pytest.raises(ValueError, match=r"expected a \(2, n\) block"):
        planar.push(b"1234")
    planar.push(torch.zeros(2, 0))
    with pytest.raises(ValueError, match="before any sample"):
        planar.finish()
    planar.finished = True                                   # as finish() leaves it
    with pytest.raises(RuntimeError, match="push after finish"):
        planar.push(torch.zeros(2, 10))
    with pytest.raises(RuntimeError, match="twice"):
        planar.finish()


def test_separate_blocks_refuses_before_it_reads_the_source():
    from demucs_amd.api import Delivery
    calls = []

    def source():
        calls.append(1)
        return iter([torch.zeros(2, 100)])

    sep = Separator(Refusing(), device="cpu", shifts=1)
    state = random.getstate()
    with pytest.raises(ValueError, match="rescale"):
        next(sep.separate_blocks(source, deliver=Delivery("a", clip="rescale")))
    with pytest.raises(ValueError, match="GPU engines"):
        next(sep.separate_blocks(source, sr=48000))
    with pytest.raises(ValueError, match="Invalid PCM format"):
        next(sep.separate_blocks(source, pcm="i8"))
    assert calls == [] and random.getstate() == state
    assert audio.TrackStats is TrackStats
