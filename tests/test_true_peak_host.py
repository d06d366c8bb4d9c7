"""The host side of the true-peak pass (demucs_amd/audio.py: true_peak_bank, TrackTruePeaks, TrackLoudness.normalised with a
ceiling, the refusals of TruePeakStream) and the numpy-float32 restatement of mi_true_peak_update's chain that the GPU tests compare
bit patterns with, checked here by itself against EBU Tech 3341's true-peak tolerance.  No GPU."""
import math
import os
import re

import numpy as np
import pytest

from demucs_amd import _lib, audio

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCES = ("drums", "vocals")
MIX = (("karaoke", (1.0, 0.0, -1.0)), ("loud", (0.0, 2.0, 0.5)))


# ---- the restatement ---------------------------------------------------------------------------------------------------------------
def chains(v, bank):
    """acc[p][c][n] for n in [0, L + T - 1) of (C, L) float32 values: acc = 0, then acc = acc + h[p][k] * v[c][n - k] for k
    ascending, the product and the sum each rounded to float32 (numpy float32 arithmetic), v = 0 outside [0, L)."""
    v = np.ascontiguousarray(v, dtype=np.float32)
    bank = np.asarray(bank, dtype=np.float32)
    (P, T), (C, L) = bank.shape, v.shape
    pad = np.zeros((C, L + 2 * (T - 1)), dtype=np.float32)
    pad[:, T - 1:T - 1 + L] = v
    acc = np.zeros((P, C, L + T - 1), dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for p in range(P):
            for k in range(T):
                prod = bank[p, k] * pad[:, T - 1 - k:T - 1 - k + L + T - 1]
                assert prod.dtype == np.float32
                acc[p] = acc[p] + prod
    return acc


def max_bits(a):
    """The largest uint32 pattern of |a| (a NaN orders above +inf), 0 for an empty array: abs_bits + atomicMax."""
    a = np.abs(np.asarray(a, dtype=np.float32)).view(np.uint32)
    return int(a.max()) if a.size else 0


def restated(v, bank):
    """(over bits, sample bits) of (C, L) float32 values."""
    return max_bits(chains(v, bank)), max_bits(v)


def value_of(bits):
    return float(np.uint32(bits).view(np.float32))


def db(x):
    return 20.0 * math.log10(x)


# (cycles per sample as a fraction, phase in degrees, amplitude, nominal dBTP, the reading the float32 chain gives)
TONES = [((1, 4), 45.0, 0.5, -6.0, -5.976), ((1, 4), 0.0, 0.5, -6.0, -6.218), ((1, 6), 60.0, 0.5, -6.0, -6.316),
         ((1, 8), 67.5, 0.5, -6.0, -6.028), ((1, 4), 45.0, 1.41, 3.0, 3.029)]


def tone(fs, frac, phase, amplitude):
    """Half a second of a sine at fs * frac with 10 ms raised-cosine fades, float64 (1, n)."""
    n, ramp = fs // 2, fs // 100
    j = np.arange(n, dtype=np.float64)
    x = amplitude * np.sin(2.0 * math.pi * frac[0] * j / frac[1] + math.radians(phase))
    env = np.ones(n)
    up = 0.5 - 0.5 * np.cos(math.pi * (np.arange(ramp) + 0.5) / ramp)
    env[:ramp], env[n - ramp:] = up, up[::-1]
    return (x * env)[None]


# ---- the bank ----------------------------------------------------------------------------------------------------------------------
def test_bank_is_the_annex_2_table():
    for fs in (8000, 44100, 48000, 95999):
        bank = audio.true_peak_bank(fs)
        assert bank.dtype == np.float32 and bank.shape == (4, 12)
        scaled = bank.astype(np.float64) * 2 ** 13
        assert (scaled == np.round(scaled)).all()              # multiples of 2^-13: exact in float32
        inter = bank.T.reshape(-1)                              # the 48-tap filter the phases were cut from
        assert (inter == inter[::-1]).all()
        sums = bank.astype(np.float64).sum(1)
        assert np.abs(sums - [1.00159, 0.97302, 0.97302, 1.00159]).max() < 5e-6
        assert bank[0, 6] == np.float32(0.97216796875) and bank[3, 5] == bank[0, 6] and bank[2, 0] == bank[1, 11]
    for fs in (96000, 192000, 0, -44100, 44100.5, True):
        with pytest.raises(ValueError, match="true peak"):
            audio.true_peak_bank(fs)


def test_header_columns_and_signature():
    text = open(os.path.join(ROOT, "include", "demucs_amd.h")).read()
    h = {k: int(v) for k, v in re.findall(r"#define (MI_[A-Z0-9_]+) (\d+)\n", text)}
    assert (h["MI_TP_COLS"], h["MI_TP_MAX_PHASES"], h["MI_TP_MAX_TAPS"]) == (audio.TP_COLS, audio.TP_MAX_PHASES, audio.TP_MAX_TAPS)
    for col in ("SRC", "N", "ORIGIN", "ORIGIN_PITCH", "ORIGIN_AFFINE", "AFFINE_ON", "GAINS"):
        assert h["MI_TP_" + col] == h["MI_MIX_" + col]
    assert h["MI_TP_SRC_PITCH"] == h["MI_LOUD_SRC_PITCH"] and h["MI_TP_BEFORE"] == h["MI_LOUD_BEFORE"]
    cols = sorted(v for k, v in h.items() if k.startswith("MI_TP_") and k not in ("MI_TP_COLS", "MI_TP_MAX_PHASES", "MI_TP_MAX_TAPS"))
    assert cols == [0, 1, 2, 3, 4, 5, 6, 11, 12, 13, 14, 15, 16, 17, 18, 19] and h["MI_TP_COLS"] == 20
    # true_peak_rows puts every value at the header's column
    gains = [("a", (0.5, 1.0, -2.0)), ("b", (0.0, 0.0, 1.0))]
    rows = audio.true_peak_rows(gains, 1000, 77, 64, 2000, 99, (0.25, 3.0), 640, 11, 13, 1, 629, 693, 2)
    assert len(rows) == 2 * audio.TP_COLS
    for i in range(2):
        r = rows[i * audio.TP_COLS:(i + 1) * audio.TP_COLS]
        want = dict(SRC=1000, N=64, ORIGIN=2000, ORIGIN_PITCH=99, AFFINE_ON=1, SRC_PITCH=77, BEFORE=640, TAIL=11, HIST_LEN=13,
                    HIST_RD=(2 + i) * 26, HIST_WR=i * 26, HIST_START=629, HIST_NEXT=693, PEAK=i)
        for k, v in want.items():
            assert r[h["MI_TP_" + k]] == v, k
        assert np.array([r[h["MI_TP_ORIGIN_AFFINE"]]], dtype=np.int64).view(np.float32).tolist() == [0.25, 3.0]
        packed = np.array(r[h["MI_TP_GAINS"]:h["MI_TP_GAINS"] + 5], dtype=np.int64).view(np.float32)
        assert packed[:3].tolist() == [float(np.float32(g)) for g in gains[i][1]] and not packed[3:].any()
    # the declaration and the ctypes signature have the same number of arguments
    decl = re.search(r"int mi_true_peak_update\(([^)]*)\);", text).group(1)
    res, args = _lib.SIGNATURES["mi_true_peak_update"]
    assert len(args) == len(decl.split(",")) == 13
    kinds = ["p" if "*" in a else "64" if "int64_t" in a else "32" for a in decl.split(",")]
    import ctypes as C
    assert [{"p": C.c_void_p, "64": C.c_int64, "32": C.c_int32}[k] for k in kinds] == list(args) and res is C.c_int


# ---- TrackTruePeaks ----------------------------------------------------------------------------------------------------------------
def bits_of(x):
    return int(np.float32(x).view(np.uint32))


def peaks_of(over, sample, **kw):
    args = dict(names=("karaoke", "loud"), sources=SOURCES, samplerate=44100, channels=2, length=1000,
                bits=[bits_of(v) for v in over], sample_bits=[bits_of(v) for v in sample], mix=MIX)
    args.update(kw)
    return audio.TrackTruePeaks(**args)


def test_track_true_peaks_validates_and_is_immutable():
    p = peaks_of([0.5, 0.25], [0.4, 0.3])
    assert p.names == ("karaoke", "loud") and p.sources == SOURCES and p.length == 1000 and p.channels == 2
    assert p.bits == (0x3F000000, 0x3E800000) and p.sample_bits == (bits_of(0.4), bits_of(0.3))
    assert p.mix == (("karaoke", (1.0, 0.0, -1.0)), ("loud", (0.0, 2.0, 0.5)))
    assert p == peaks_of([0.5, 0.25], [0.4, 0.3]) and hash(p) == hash(peaks_of([0.5, 0.25], [0.4, 0.3]))
    assert p != peaks_of([0.5, 0.25], [0.4, 0.25]) and p != peaks_of([0.5, 0.26], [0.4, 0.3]) and p != peaks_of([0.5, 0.25], [0.4, 0.3], length=999)
    assert p != "x" and "TrackTruePeaks" in repr(p)
    for op in (lambda: setattr(p, "length", 3), lambda: delattr(p, "bits"), lambda: setattr(p, "extra", 1)):
        with pytest.raises(AttributeError):
            op()
    bad = [dict(names=["karaoke", "karaoke"]), dict(names="ab"), dict(names=[]), dict(sources=[]), dict(sources=("drums", 3)),
           dict(samplerate=96000), dict(samplerate=0), dict(samplerate=44100.5), dict(channels=0), dict(channels=True),
           dict(length=-1), dict(length=2.0), dict(bits=[1]), dict(bits=[1, 2, 3]), dict(bits=[0x80000000, 0]), dict(bits=[-1, 0]),
           dict(bits=[0.5, 0.5]), dict(bits="ab"), dict(sample_bits=[1]), dict(sample_bits=[1 << 32, 0]), dict(sample_bits=[True, 0]),
           dict(mix=None), dict(mix=MIX[:1]), dict(mix=MIX[::-1]), dict(mix=(("karaoke", (1.0, 0.0)), ("loud", (0.0, 2.0)))),
           dict(mix=(("karaoke", (1.0, float("nan"), 0.0)), MIX[1])), dict(mix=(("karaoke", "abc"), MIX[1]))]
    for kw in bad:
        with pytest.raises(ValueError, match="TrackTruePeaks|true peak"):
            peaks_of([0.5, 0.25], [0.4, 0.3], **kw)
    zero = peaks_of([0.0, 0.0], [0.0, 0.0], length=0)
    assert zero.length == 0 and zero.bits == (0, 0)


def test_dbtp_and_gain_limit_arithmetic():
    nan_bits = 0x7FC00000
    p = audio.TrackTruePeaks(("a", "b", "c", "d"), ("s",), 48000, 1, 10, [bits_of(0.5), 0, nan_bits, bits_of(0.4)],
                             [bits_of(0.25), 0, nan_bits, bits_of(0.5)], [(n, (0.0, 1.0)) for n in "abcd"])
    assert p.true_peak("a") == 0.5 and p.sample_peak("a") == 0.25
    assert p.dbtp("a") == pytest.approx(-6.020599913279624, abs=1e-12)
    assert p.dbtp("b") == -math.inf and p.true_peak("b") == 0.0 and math.isnan(p.dbtp("c")) and math.isnan(p.true_peak("c"))
    ceiling = 10 ** (-1 / 20)
    assert p.gain_limit("a") == pytest.approx(ceiling / 0.5, rel=1e-15) == p.gain_limit("a", -1.0)
    assert p.gain_limit("a", 0.0) == 2.0 and p.gain_limit("a", -6.0) == pytest.approx(10 ** -0.3 / 0.5, rel=1e-15)
    assert p.gain_limit("b") == math.inf
    # the sample peak above the oversampled one: the larger of the two binds
    assert p.true_peak("d") == float(np.float32(0.4)) and p.gain_limit("d") == pytest.approx(ceiling / 0.5, rel=1e-15)
    assert p.dbtp("d") == pytest.approx(db(float(np.float32(0.4))), abs=1e-12)
    with pytest.raises(ValueError, match="no gain"):
        p.gain_limit("c")
    only_sample = audio.TrackTruePeaks(("a",), ("s",), 48000, 1, 10, [bits_of(0.5)], [nan_bits], [("a", (0.0, 1.0))])
    with pytest.raises(ValueError, match="no gain"):
        only_sample.gain_limit("a")
    with pytest.raises(ValueError, match="no gain"):
        p.gain_limit("a", float("nan"))
    for f in (p.true_peak, p.sample_peak, p.dbtp, p.gain_limit):
        with pytest.raises(KeyError):
            f("z")


# ---- TrackLoudness.normalised --------------------------------------------------------------------------------------------------
def loudness_of(levels, **kw):
    """A hand-made TrackLoudness of 1 s whose outputs read `levels` LUFS: constant energies, every block over both gates."""
    hop = 4410
    e = np.zeros((len(levels), 2, 10))
    for i, l in enumerate(levels):
        e[i] = 10 ** ((l + 0.691) / 10) * hop / 2               # both channels: block power 10 ** ((l + 0.691) / 10)
    args = dict(names=("karaoke", "loud"), sources=SOURCES, samplerate=44100, channels=2, length=44100, energies=e, mix=MIX)
    args.update(kw)
    return audio.TrackLoudness(**args)


def parent_normalised(loud, target):
    """`normalised` as it was before it took true peaks."""
    terms = ("mix",) + loud.sources
    return {name: {t: g * loud.gain(name, target) for t, g in zip(terms, gains) if g != 0} for name, gains in loud.mix}


def test_normalised_without_true_peaks_is_unchanged():
    loud = loudness_of([-20.0, -9.5])
    assert loud.integrated("karaoke") == pytest.approx(-20.0, abs=1e-9) and loud.integrated("loud") == pytest.approx(-9.5, abs=1e-9)
    for target in (-14.0, -23.0):
        assert loud.normalised(target) == parent_normalised(loud, target) == loud.normalised(target, None) == \
            loud.normalised(target, true_peaks=None, ceiling=-3.0)
    assert loud.normalised() == parent_normalised(loud, -14.0)
    assert list(loud.normalised()["karaoke"]) == ["mix", "vocals"] and list(loud.normalised()["loud"]) == ["drums", "vocals"]


def test_normalised_caps_the_output_that_would_exceed_the_ceiling():
    loud = loudness_of([-20.0, -9.5])
    # karaoke: +6 dB to the target with peaks at 0.8 -> capped.  loud: -4.5 dB with peaks at 0.9 -> its loudness gain
    peaks = peaks_of([0.8, 0.9], [0.7, 0.95], length=44100)
    got = loud.normalised(-14.0, true_peaks=peaks)
    free = parent_normalised(loud, -14.0)
    k = peaks.gain_limit("karaoke", -1.0)
    assert k == 10 ** (-1 / 20) / float(np.float32(0.8)) and k < loud.gain("karaoke", -14.0)
    assert got["karaoke"] == {"mix": 1.0 * k, "vocals": -1.0 * k}
    assert got["loud"] == free["loud"] and loud.gain("loud", -14.0) < peaks.gain_limit("loud")
    # another ceiling: both free at +12, both capped at -12
    assert loud.normalised(-14.0, peaks, ceiling=12.0) == free
    low = loud.normalised(-14.0, peaks, ceiling=-12.0)
    assert low["loud"] == {"drums": 2.0 * peaks.gain_limit("loud", -12.0), "vocals": 0.5 * peaks.gain_limit("loud", -12.0)}
    assert peaks.gain_limit("loud", -12.0) == 10 ** (-12 / 20) / float(np.float32(0.95))      # the sample peak binds
    # silence has no limit; a NaN peak has no gain
    assert loud.normalised(-14.0, peaks_of([0.0, 0.9], [0.0, 0.9], length=44100))["karaoke"] == free["karaoke"]
    with pytest.raises(ValueError, match="no gain"):
        loud.normalised(-14.0, peaks_of([float("nan"), 0.9], [0.1, 0.9], length=44100))


def test_normalised_refuses_true_peaks_of_something_else():
    loud = loudness_of([-20.0, -9.5])
    other_mix = (("karaoke", (1.0, 0.0, -0.5)), MIX[1])
    renamed = (("k", MIX[0][1]), ("loud", MIX[1][1]))
    for kw in (dict(length=44099), dict(samplerate=48000), dict(channels=1), dict(sources=("drums", "bass")), dict(mix=other_mix),
               dict(names=("k", "loud"), mix=renamed)):
        with pytest.raises(ValueError, match="the true peaks were measured with"):
            loud.normalised(-14.0, true_peaks=peaks_of([0.5, 0.5], [0.5, 0.5], **{"length": 44100, **kw}))
    with pytest.raises(ValueError, match="must be a TrackTruePeaks"):
        loud.normalised(-14.0, true_peaks={"karaoke": 0.5})


def test_streams_refuse_before_any_device_work():
    with pytest.raises(_lib.EngineError, match="only runs on a GPU"):
        audio.TruePeakStream(["a"], 2, 44100, device="cpu")
    with pytest.raises(ValueError, match="below 96 kHz"):
        audio.TruePeakStream(["a"], 2, 96000)
    with pytest.raises(ValueError, match="at least one"):
        audio.TruePeakStream([], 2, 44100)
    with pytest.raises(ValueError, match="at least one channel"):
        audio.TruePeakStream(["a"], 0, 44100)
    with pytest.raises(ValueError, match="neither 'mix' nor one of the separated sources"):
        audio.TruePeakStream(["a"], 2, 44100, mix={"x": {"piano": 1.0}})


# ---- the restatement by itself ---------------------------------------------------------------------------------------------------
def test_restatement_on_hand_worked_cases():
    bank = audio.true_peak_bank(48000)
    # a lone last sample of 0.75: the peak is 0.75 * 0.97216796875 at phase 0, k = 6 -- five positions past the end
    v = np.zeros((1, 2), dtype=np.float32)
    v[0, 1] = 0.75
    acc = chains(v, bank)
    assert acc.shape == (4, 1, 13)
    p, c, n = np.unravel_index(np.abs(acc).argmax(), acc.shape)
    assert (p, n) == (0, 1 + 6) and n - (v.shape[1] - 1) - 1 == 5 and acc[p, c, n] == np.float32(0.75 * 0.97216796875)
    assert value_of(restated(v, bank)[0]) == pytest.approx(0.729126, abs=5e-7) and restated(v, bank)[1] == bits_of(0.75)
    # recognisable coefficients on a ramp
    small = np.array([[1, 2, 4], [8, 16, 32]], dtype=np.float32)
    ramp = np.arange(1, 6, dtype=np.float32)[None]
    acc = chains(ramp, small)
    assert acc[0, 0].tolist() == [1, 4, 11, 18, 25, 26, 20] and acc[1, 0].tolist() == [8, 32, 88, 144, 200, 208, 160]
    assert restated(ramp, small) == (bits_of(208.0), bits_of(5.0))      # the maximum lies past the end, in the tail
    assert restated(np.zeros((2, 0), dtype=np.float32), bank) == (0, 0)
    nan = ramp.copy()
    nan[0, 2] = float("nan")
    assert restated(nan, small) == (0x7FC00000, 0x7FC00000)


@pytest.mark.parametrize("fs", [44100, 48000])
def test_restatement_reads_the_faded_tones_within_the_tolerance(fs):
    """EBU Tech 3341's true-peak tolerance is +0.2 / -0.4 dB around the nominal peak; the restatement alone meets it."""
    bank = audio.true_peak_bank(fs)
    for frac, phase, amplitude, nominal, table in TONES:
        x = tone(fs, frac, phase, amplitude)
        over, sample = restated(x.astype(np.float32), bank)
        reading = db(value_of(over))
        print(f"fs {fs} tone {frac[0]}/{frac[1]} phase {phase} amplitude {amplitude}: {reading:.4f} dBTP, sample peak "
              f"{db(value_of(sample)):.4f} dBFS")
        assert nominal - 0.4 <= reading <= nominal + 0.2
        assert abs(reading - table) <= 0.0015                   # the reading the float32 chain is known to give
    # the fs/4 tone sampled at its crests: the oversampled estimate lies below the sample peak
    over, sample = restated(tone(fs, (1, 4), 90.0, 0.5).astype(np.float32), bank)
    assert value_of(sample) == 0.5 and value_of(over) < 0.5
    # at 45 degrees the samples are 3 dB below the peak
    over, sample = restated(tone(fs, (1, 4), 45.0, 0.5).astype(np.float32), bank)
    assert db(value_of(sample)) == pytest.approx(-9.03, abs=0.01)
