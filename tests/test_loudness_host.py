"""The host side of the loudness pass (demucs_amd/audio.py: k_weighting, loudness_warmup, gated_loudness, TrackLoudness and the
refusals of LoudnessStream / loudness) against ITU-R BS.1770-4's table and formulas restated here in plain numpy.  No GPU."""
import math

import numpy as np
import pytest
import torch

from demucs_amd import audio

TABLE_48K = [[[1.53512485958697, -2.69169618940638, 1.19839281085285], [1.0, -1.69065929318241, 0.73248077421585]],
             [[1.0, -2.0, 1.0], [1.0, -1.99004745483398, 0.99007225036621]]]


def test_k_weighting_reproduces_the_recommendations_table_at_48k():
    k = audio.k_weighting(48000)
    assert k.dtype == np.float64 and k.shape == (2, 2, 3)
    assert np.abs(k - np.array(TABLE_48K)).max() <= 1e-12
    other = audio.k_weighting(44100)
    assert other[1, 0].tolist() == [1.0, -2.0, 1.0] and np.abs(other - k).max() > 1e-3


def test_warmup_scales_with_the_sample_rate():
    assert audio.loudness_warmup(44100) == 16384
    assert audio.loudness_warmup(48000) == 16384
    assert audio.loudness_warmup(96000) == 32768
    assert audio.loudness_warmup(192000) == 65536


def integrated(e, hop):
    """BS.1770-4 from (channels, Hn) energies, spelled with loops."""
    e = np.asarray(e, dtype=np.float64)
    if np.isnan(e).any():
        return float("nan")
    hn = e.shape[1]
    powers = [sum(e[c][j] + e[c][j + 1] + e[c][j + 2] + e[c][j + 3] for c in range(e.shape[0])) / (4 * hop) for j in range(hn - 3)]
    lufs = [-0.691 + 10 * math.log10(p) if p > 0 else -math.inf for p in powers]
    first = [p for p, l in zip(powers, lufs) if l > -70]
    if not first:
        return -math.inf
    gate = -0.691 + 10 * math.log10(sum(first) / len(first)) - 10
    second = [p for p, l in zip(powers, lufs) if l > -70 and l > gate]
    if not second:
        return -math.inf
    return -0.691 + 10 * math.log10(sum(second) / len(second))


def test_gating_from_hand_made_energies():
    hop = 4800
    rng = np.random.default_rng(0)
    # fewer than four sub-blocks
    for hn in range(4):
        assert audio.gated_loudness(np.full((2, hn), 100.0), hop) == -math.inf
    # every block below the absolute gate: -70 LUFS is a block power of 10 ** -6.9309
    quiet = np.full((2, 12), 0.5 * hop * 10 ** -7.0)
    assert audio.gated_loudness(quiet, hop) == -math.inf == integrated(quiet, hop)
    # just above it, the blocks count
    above = np.full((1, 12), hop * 10 ** -6.9)
    assert audio.gated_loudness(above, hop) == pytest.approx(integrated(above, hop), abs=1e-12) == pytest.approx(-69.691, abs=1e-9)
    # a loud passage and a passage 30 LU below it: the relative gate removes the quiet blocks, the absolute gate keeps them
    loud, soft = hop * 10 ** -2.0, hop * 10 ** -5.0
    e = np.concatenate([np.full(20, loud), np.full(20, soft)])[None] * (1 + 0.01 * rng.standard_normal((2, 40)))
    want = integrated(e, hop)
    assert audio.gated_loudness(e, hop) == pytest.approx(want, abs=1e-12)
    ungated = -0.691 + 10 * math.log10(np.mean([(e[:, j:j + 4]).sum() / (4 * hop) for j in range(37)]))
    # what survives: 17 blocks inside the loud passage and the 3 across the edge, which hold 3/4, 1/2 and 1/4 of its power
    survivors = -0.691 + 10 * math.log10(2 * loud / hop * (17 + 1.5) / 20)
    assert want > ungated + 2.0 and abs(want - survivors) < 0.05
    # a NaN energy anywhere
    e[1, 7] = float("nan")
    assert math.isnan(audio.gated_loudness(e, hop)) and math.isnan(integrated(e, hop))


def a_track(**kw):
    rng = np.random.default_rng(1)
    args = dict(names=["karaoke", "loud"], sources=["drums", "vocals"], samplerate=48000, channels=2, length=48000 * 2 + 77,
                energies=4800 * 10 ** -2.5 * (1 + 0.1 * rng.random((2, 2, 20))),
                mix=(("karaoke", (1.0, 0.0, -1.0)), ("loud", (0.0, 2.0, 0.5))))
    args.update(kw)
    return audio.TrackLoudness(**args)


def test_track_loudness_is_immutable_and_compares_by_value():
    a, b = a_track(), a_track()
    assert a == b and hash(a) == hash(b) and a.hop == 4800
    with pytest.raises(AttributeError):
        a.length = 3
    with pytest.raises(AttributeError):
        del a.names
    with pytest.raises(ValueError):
        a.energies[0, 0, 0] = 1.0
    e = a.energies.copy()
    e[1, 1, 19] = np.nextafter(e[1, 1, 19], 1.0)
    assert a_track(energies=e) != a
    assert a_track(samplerate=44100, energies=np.ones((2, 2, (48000 * 2 + 77) // 4410))) != a
    for bad in (dict(energies=np.ones((2, 2, 19))), dict(names=["a", "a"]), dict(mix=(("karaoke", (1.0, 0.0)), ("loud", (0.0, 2.0)))),
                dict(samplerate=44101), dict(channels=3), dict(length=-1), dict(mix=(("loud", (0.0, 2.0, 0.5)), ("karaoke", (1.0, 0.0, -1.0))))):
        with pytest.raises(ValueError):
            a_track(**bad)
    assert "karaoke" in repr(a)


def test_figures_and_normalised_gains():
    t = a_track()
    for i, name in enumerate(t.names):
        assert t.integrated(name) == pytest.approx(integrated(t.energies[i], 4800), abs=1e-12)
        m = t.momentary(name)
        assert m.shape == (17,)
        assert m[3] == pytest.approx(-0.691 + 10 * math.log10(t.energies[i][:, 3:7].sum() / (4 * 4800)), abs=1e-12)
        assert t.gain(name, -14.0) == pytest.approx(10 ** ((-14.0 - t.integrated(name)) / 20), rel=1e-15)
    with pytest.raises(KeyError):
        t.integrated("vocals")
    norm = t.normalised(-16.0)
    ka, lo = t.gain("karaoke", -16.0), t.gain("loud", -16.0)
    assert norm == {"karaoke": {"mix": 1.0 * ka, "vocals": -1.0 * ka}, "loud": {"drums": 2.0 * lo, "vocals": 0.5 * lo}}
    assert list(norm) == ["karaoke", "loud"]
    assert audio.mix_gains(norm, ["drums", "vocals"])[0][1][1] == 0.0          # the muted term stays muted
    assert t.normalised() == t.normalised(-14.0)
    # silence and NaN have no gain
    silent = a_track(energies=np.zeros((2, 2, 20)))
    assert silent.integrated("loud") == -math.inf
    with pytest.raises(ValueError, match="-inf LUFS"):
        silent.gain("loud", -14.0)
    e = t.energies.copy()
    e[0, 0, 5] = float("nan")
    broken = a_track(energies=e)
    assert math.isnan(broken.integrated("karaoke")) and math.isfinite(broken.integrated("loud"))
    with pytest.raises(ValueError, match="nan LUFS"):
        broken.normalised()
    short = a_track(length=4800 * 3, energies=np.ones((2, 2, 3)))
    assert short.integrated("loud") == -math.inf and short.momentary("loud").shape == (0,)


def test_refusals_need_no_gpu():
    src = ["drums", "vocals"]
    with pytest.raises(ValueError, match="no multiple of 10"):
        audio.LoudnessStream(src, 2, 44101)
    with pytest.raises(ValueError, match="1 or 2 channels"):
        audio.LoudnessStream(src, 3, 44100)
    with pytest.raises(ValueError, match="neither 'mix' nor one of the separated sources"):
        audio.LoudnessStream(src, 2, 44100, mix={"a": {"bass": 1}})
    with pytest.raises(ValueError, match="must be finite"):
        audio.LoudnessStream(src, 2, 44100, mix={"a": {"drums": float("inf")}})
    with pytest.raises(ValueError, match="every gain of output 'a' is 0"):
        audio.LoudnessStream(src, 2, 44100, mix={"a": {"drums": 0.0, "mix": 0}})
    with pytest.raises(ValueError, match="at most 8 sources"):
        audio.LoudnessStream([f"s{i}" for i in range(9)], 2, 44100)
    stems = {k: torch.zeros(2, 100) for k in src}
    with pytest.raises(ValueError, match="pass the mix as origin"):
        audio.loudness(None, stems, {"a": {"mix": 1, "vocals": -1}})
    with pytest.raises(ValueError, match="no multiple of 10"):
        audio.loudness(None, stems, samplerate=22055)
    with pytest.raises(ValueError, match="1 or 2 channels"):
        audio.loudness(None, {k: torch.zeros(3, 100) for k in src})
    with pytest.raises(ValueError, match="the mix is"):
        audio.loudness(torch.zeros(2, 99), stems, {"a": {"mix": 1}})
    # a stream refuses a push without the mix it needs before it touches the device
    st = audio.LoudnessStream(src, 2, 44100, mix={"a": {"mix": 1, "vocals": -1}})
    with pytest.raises(ValueError, match="push the mix"):
        st.push(torch.zeros(2, 2, 10))
    with pytest.raises(ValueError, match="block of stems"):
        st.push(torch.zeros(2, 1, 10), torch.zeros(1, 10))
    assert st.device_bytes == 0 and st.pushed == 0
    # the default measures every source by itself
    assert [n for n, _ in audio.LoudnessStream(src, 1, 48000).gains] == src
