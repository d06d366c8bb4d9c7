"""Host logic of the nSDR scoring without a GPU: `audio.summarise_scores` against numbers worked out by hand, `audio.TrackScore`,
and the refusals of `audio.SdrStream`, `audio.new_sdr`, `Separator.evaluate_blocks` and `Separator.score_tensor` that need no
device."""
import math
import random

import numpy as np
import pytest
import torch

from demucs_amd import _lib, audio
from demucs_amd.api import Separator
from demucs_amd.audio import SdrStream, TrackScore, summarise_scores
from demucs_amd.pretrained import get_model
from test_stream_host import Refusing

NAN = float("nan")


def one(v):
    """The score of one source as an `SdrStream` per source would return it."""
    return TrackScore([v], [1.0], [1.0], 10)


# ---- summarise_scores: demucs/evaluate.py:157-173 for the nsdr metric ------------------------------------------------------------------
def test_summarise_scores_by_hand():
    """drums 4, 6, 11: mean 7, median 6.  vocals 7.5, 3, 1.5: mean 4, median 3.  nsdr (7 + 4) / 2, nsdr_med (6 + 3) / 2."""
    tracks = {"a": {"drums": one(4.0), "vocals": one(7.5)},
              "b": {"drums": one(6.0), "vocals": one(3.0)},
              "c": {"drums": one(11.0), "vocals": one(1.5)}}
    got = summarise_scores(tracks, ["drums", "vocals"])
    assert got == {"nsdr_drums": 7.0, "nsdr_med_drums": 6.0, "nsdr_vocals": 4.0, "nsdr_med_vocals": 3.0, "nsdr": 5.5, "nsdr_med": 4.5}
    assert list(got) == ["nsdr_drums", "nsdr_med_drums", "nsdr_vocals", "nsdr_med_vocals", "nsdr", "nsdr_med"]
    assert all(type(v) is float for v in got.values())
    # the same figures from plain numbers and from whole-track scores in the sources' order
    plain = {k: {s: float(v.nsdr[0]) for s, v in d.items()} for k, d in tracks.items()}
    assert summarise_scores(plain, ["drums", "vocals"]) == got
    whole = {k: TrackScore([d["drums"].nsdr[0], d["vocals"].nsdr[0]], [1.0, 1.0], [1.0, 1.0], 10) for k, d in tracks.items()}
    assert summarise_scores(whole, ["drums", "vocals"]) == got


@pytest.mark.filterwarnings("ignore::RuntimeWarning")
def test_summarise_scores_with_a_nan_score():
    """A NaN among a source's values makes numpy's mean and median NaN, and with them both averages over the sources; the other
    source keeps its figures: drums 4, 6, 11 -> 7 and 6."""
    tracks = {"a": {"drums": one(4.0), "vocals": one(7.5)},
              "b": {"drums": one(6.0), "vocals": one(NAN)},
              "c": {"drums": one(11.0), "vocals": one(1.5)}}
    got = summarise_scores(tracks, ["drums", "vocals"])
    assert got["nsdr_drums"] == 7.0 and got["nsdr_med_drums"] == 6.0
    for key in ("nsdr_vocals", "nsdr_med_vocals", "nsdr", "nsdr_med"):
        assert math.isnan(got[key]), key
    assert len(got) == 6


def test_summarise_scores_refusals():
    with pytest.raises(ValueError, match="at least one track"):
        summarise_scores({}, ["drums"])
    with pytest.raises(ValueError, match="2 sources for 1 names"):
        summarise_scores({"a": TrackScore([1.0, 2.0], [1.0, 1.0], [1.0, 1.0], 5)}, ["drums"])
    with pytest.raises(ValueError, match="one source's"):
        summarise_scores({"a": {"drums": TrackScore([1.0, 2.0], [1.0, 1.0], [1.0, 1.0], 5)}}, ["drums"])


# ---- TrackScore ------------------------------------------------------------------------------------------------------------------------
def test_track_score_holds_its_values_and_is_immutable():
    sc = TrackScore([3.5, -1.25], np.array([10.0, 20.0]), (1.0, 2.0), 1000)
    assert sc.nsdr.tolist() == [3.5, -1.25] and sc.num.tolist() == [10.0, 20.0] and sc.den.tolist() == [1.0, 2.0]
    assert all(a.dtype == np.float64 and not a.flags.writeable for a in (sc.nsdr, sc.num, sc.den))
    assert sc.length == 1000 and type(sc.length) is int
    assert sc == TrackScore([3.5, -1.25], [10.0, 20.0], [1.0, 2.0], 1000)
    assert hash(sc) == hash(TrackScore([3.5, -1.25], [10.0, 20.0], [1.0, 2.0], 1000))
    assert sc != TrackScore([3.5, -1.25], [10.0, 20.0], [1.0, 2.0], 1001)
    assert sc != TrackScore([3.5, np.nextafter(-1.25, 0)], [10.0, 20.0], [1.0, 2.0], 1000)      # one bit
    assert sc != TrackScore([3.5], [10.0], [1.0], 1000)
    for name in ("nsdr", "num", "den", "length", "other"):
        with pytest.raises(AttributeError):
            setattr(sc, name, 1)
    with pytest.raises(AttributeError):
        del sc.nsdr
    with pytest.raises(ValueError):
        sc.nsdr[0] = 0.0
    assert repr(sc) == "TrackScore(nsdr=[3.5, -1.25], num=[10.0, 20.0], den=[1.0, 2.0], length=1000)"
    nan = TrackScore([NAN], [NAN], [1.0], 3)
    assert nan == TrackScore([NAN], [NAN], [1.0], 3) and hash(nan) == hash(TrackScore([NAN], [NAN], [1.0], 3))
    assert TrackScore([0.0], [0.0], [0.0], 0).length == 0                   # an empty track scores 0 dB


@pytest.mark.parametrize("args,match", [
    (([1.0], [1.0, 2.0], [1.0], 5), "one length"),
    (([[1.0]], [[1.0]], [[1.0]], 5), "one value per source"),
    (([], [], [], 5), "one value per source"),
    (([1.0] * 9, [1.0] * 9, [1.0] * 9, 5), "one value per source"),
    (([1.0], [1.0], [1.0], -1), "non-negative integer"),
    (([1.0], [1.0], [1.0], 2.0), "non-negative integer"),
    (([1.0], [1.0], [1.0], True), "non-negative integer"),
])
def test_track_score_validation(args, match):
    with pytest.raises(ValueError, match=match):
        TrackScore(*args)


def test_track_score_from_sums_is_the_reference_formula():
    sums = torch.tensor([[4.0, 1.0], [0.0, 0.0], [2.5, 0.0]], dtype=torch.float64)
    sc = TrackScore.from_sums(sums, 7)
    want = [10 * math.log10((4.0 + 1e-7) / (1.0 + 1e-7)), 0.0, 10 * math.log10((2.5 + 1e-7) / 1e-7)]
    assert sc.nsdr[1] == 0.0 and np.allclose(sc.nsdr, want, rtol=1e-15, atol=0)
    assert sc.num.tolist() == [4.0, 0.0, 2.5] and sc.den.tolist() == [1.0, 0.0, 0.0] and sc.length == 7


# ---- refusals that need no device ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_sources", [0, 9, -1, 2.5, True])
def test_sdr_stream_refuses_a_bad_source_count(n_sources):
    with pytest.raises(ValueError, match="1 to 8 sources"):
        SdrStream(n_sources, 2)


def test_sdr_stream_constructor_refusals():
    with pytest.raises(ValueError, match="channels must be >= 1"):
        SdrStream(4, 0)
    with pytest.raises(ValueError, match="Invalid PCM format"):
        SdrStream(4, 2, pcm="u8", src_channels=2)
    with pytest.raises(ValueError, match="needs src_channels"):
        SdrStream(4, 2, pcm="i16")
    with pytest.raises(ValueError, match="less channels"):
        SdrStream(4, 3, pcm="i16", src_channels=2)
    with pytest.raises(_lib.EngineError, match="only runs on a GPU device"):
        SdrStream(4, 2, device="cpu")


def test_sdr_stream_refuses_blocks_before_any_device_work():
    st = SdrStream(4, 2, device="cuda", pcm="i16", src_channels=2)
    for block in ([b"\x00" * 8] * 3, [b"\x00" * 8] * 5, b"\x00" * 8, torch.zeros(4, 2, 10)):
        with pytest.raises(ValueError, match="a list of 4 PCM chunks"):
            st.push_references(block)
    with pytest.raises(ValueError, match="the same number of frames"):
        st.push_references([b"\x00" * 8, b"\x00" * 8, b"\x00" * 4, b"\x00" * 8])
    assert st.trailing_bytes == 0                            # a refused push leaves the feeds as they were
    st.push_references([b"\x01\x02\x03"] * 4)                # no whole frame: carried, no device work
    assert st.trailing_bytes == 3 and st.references_pushed == 0 and st.device_bytes() == 0
    with pytest.raises(ValueError, match=r"expected a \(4, 2, n\) block"):
        st.push_estimates(torch.zeros(4, 3, 10))
    with pytest.raises(ValueError, match=r"expected a \(4, 2, n\) block"):
        st.push_estimates(torch.zeros(2, 10))
    with pytest.raises(TypeError, match="floating-point"):
        st.push_estimates(torch.zeros(4, 2, 10, dtype=torch.int16))
    st.push_estimates(torch.zeros(4, 2, 0))                  # an empty block: nothing to do
    with pytest.raises(ValueError, match="before any sample"):
        st.finish()
    assert not st.finished
    planar = SdrStream(1, 1, device="cuda")
    with pytest.raises(ValueError, match=r"expected a \(1, 1, n\) block"):
        planar.push_references([b"\x00" * 8])
    planar.finished = True                                   # as finish() leaves it
    with pytest.raises(RuntimeError, match="push after finish"):
        planar.push_references(torch.zeros(1, 1, 4))
    with pytest.raises(RuntimeError, match="push after finish"):
        planar.push_estimates(torch.zeros(1, 1, 4))
    with pytest.raises(RuntimeError, match="twice"):
        planar.finish()


def test_new_sdr_refuses_bad_shapes():
    with pytest.raises(ValueError, match="batch, sources, channels, length"):
        audio.new_sdr(torch.zeros(4, 2, 10), torch.zeros(4, 2, 10))
    with pytest.raises(ValueError, match="differ in shape"):
        audio.new_sdr(torch.zeros(1, 4, 2, 10), torch.zeros(1, 4, 2, 11))
    with pytest.raises(ValueError, match="1 to 8 sources"):
        audio.new_sdr(torch.zeros(1, 9, 2, 10), torch.zeros(1, 9, 2, 10))


def test_evaluate_blocks_and_score_tensor_refuse_before_they_read_anything():
    calls = []

    def source():
        calls.append("mix")
        return iter([torch.zeros(2, 100)])

    def references():
        calls.append("refs")
        return iter([torch.zeros(4, 2, 100)])

    state = random.getstate()
    engine = get_model("demucs_unittest")
    for sep in (Separator(Refusing(), device="cuda", shifts=1),        # not an engine model
                Separator(Refusing(), device="cpu", shifts=1),
                Separator(engine, device="cpu", shifts=1)):            # an engine model on a CPU device
        with pytest.raises(ValueError, match="GPU engines"):
            sep.evaluate_blocks(source, references)
        with pytest.raises(ValueError, match="GPU engines"):
            sep.score_tensor(torch.zeros(2, 100), torch.zeros(4, 2, 100))
    sep = Separator(engine, device="cuda", shifts=1)
    with pytest.raises(ValueError, match="Invalid PCM format"):
        sep.evaluate_blocks(source, references, pcm="i8")
    with pytest.raises(ValueError, match="Invalid PCM format"):
        sep.evaluate_blocks(source, references, ref_pcm="u8")
    with pytest.raises(ValueError, match="positive integer"):
        sep.evaluate_blocks(source, references, sr=0)
    with pytest.raises(ValueError, match=r"references must be \(4, 2, length\)"):
        sep.score_tensor(torch.zeros(2, 100), torch.zeros(3, 2, 100))
    assert calls == [] and random.getstate() == state
