"""True peaks through `audio.true_peak`, `audio.TruePeakStream` and the Separator on the MI355X: the whole-track call against the
stream and the restatement of tests/test_true_peak_host.py, EBU Tech 3341's tones, the ceiling of `TrackLoudness.normalised` on
delivered frames, and `levels_blocks` -- both meters fed by one separating pass -- against `levels_tensor`."""
import random

import numpy as np
import pytest
import torch

from demucs_amd import audio
from demucs_amd.api import Separator, TrackLoudness, TrackTruePeaks
from test_gpu_deliver_mix import mix_value
from test_gpu_ingest import to_i16
from test_gpu_stream import hd, track
from test_true_peak_host import TONES, db, restated, tone, value_of

pytestmark = pytest.mark.gpu
SR = 44100
NAMES = ["drums", "bass", "other", "vocals"]
REMIX = {"karaoke": {"mix": 1.0, "vocals": -1.0}, "practice": {"drums": 2.0, "bass": 0.5, "other": 0.5, "vocals": 0.5}}


# ---- 1. the whole-track call ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def separated():
    g = torch.Generator().manual_seed(13)
    block = (torch.randn(4, 2, 3 * SR, generator=g) * 0.3).cuda()
    origin = (torch.randn(2, 3 * SR, generator=g) * 0.3).cuda()
    return origin, dict(zip(NAMES, block))


@pytest.mark.parametrize("mix", [REMIX, None], ids=["remixes", "default"])
def test_whole_track_equals_the_stream_and_the_restatement(separated, mix):
    origin, stems = separated
    whole = audio.true_peak(origin, stems, mix, SR)
    n = origin.shape[1]
    names = tuple(mix) if mix is not None else (*NAMES, "mix")
    assert isinstance(whole, TrackTruePeaks) and whole.names == names and whole.sources == tuple(NAMES)
    assert (whole.samplerate, whole.channels, whole.length) == (SR, 2, n)
    explicit = mix if mix is not None else {**{k: {k: 1.0} for k in NAMES}, "mix": {"mix": 1.0}}
    resolved = audio.mix_gains(explicit, NAMES)
    assert whole.mix == audio.mix_identity(resolved)
    x, o = torch.stack(list(stems.values())).cpu(), origin.cpu()
    want = [restated(mix_value(x, o, g).numpy(), audio.true_peak_bank(SR)) for _, g in resolved]
    assert list(zip(whole.bits, whole.sample_bits)) == want
    for name in names:
        print(f"{name}: {whole.dbtp(name):.4f} dBTP, sample peak {db(whole.sample_peak(name)):.4f} dBFS")
    mixed = any(g[0] != 0 for _, g in resolved)
    st = audio.TruePeakStream(NAMES, 2, SR, explicit, device="cuda")
    block = torch.stack(list(stems.values()))
    rng, at = np.random.default_rng(2), 0
    while at < n:
        b = int(rng.choice([0, 1, 7, int(rng.integers(1, SR))]))
        st.push(block[:, :, at:at + b], origin[:, at:at + b] if mixed else None)
        at = min(n, at + b)
    got = st.finish()
    assert got == whole and got.bits == whole.bits and got.sample_bits == whole.sample_bits
    # host stems are uploaded; the result is the same
    assert audio.true_peak(o, {k: v.cpu() for k, v in stems.items()}, mix, SR) == whole
    empty = audio.true_peak(None, {"a": torch.zeros(2, 0, device="cuda")}, samplerate=SR)
    assert empty.length == 0 and empty.bits == (0,) and empty.sample_bits == (0,)
    st = audio.TruePeakStream(["a"], 2, SR, device="cuda")
    st.push(torch.zeros(1, 2, 0, device="cuda"))
    assert st.finish() == empty


@pytest.mark.parametrize("fs", [44100, 48000])
def test_the_faded_tones_read_within_the_tolerance(fs):
    """EBU Tech 3341: +0.2 / -0.4 dB around the nominal true peak; and the float32 chain against the float64 convolution."""
    bank = audio.true_peak_bank(fs).astype(np.float64)
    for frac, phase, amplitude, nominal, _ in TONES:
        x = tone(fs, frac, phase, amplitude).astype(np.float32)
        got = audio.true_peak(None, {"tone": torch.from_numpy(np.concatenate([x, -x])).cuda()}, samplerate=fs)
        exact = max(np.abs(np.convolve(bank[p], x[0].astype(np.float64))).max() for p in range(4))
        reading = got.dbtp("tone")
        print(f"fs {fs} tone {frac[0]}/{frac[1]} phase {phase}: {reading:.4f} dBTP, float64 {db(exact):.4f}, relative "
              f"{abs(got.true_peak('tone') - exact) / exact:.2e}")
        assert nominal - 0.4 <= reading <= nominal + 0.2
        assert abs(got.true_peak("tone") - exact) <= 1e-5 * exact
        assert (got.bits[0], got.sample_bits[0]) == restated(x, audio.true_peak_bank(fs))
        assert got.sample_peak("tone") == float(np.abs(x).max())


# ---- 2. the ceiling ------------------------------------------------------------------------------------------------------------
def test_normalised_with_a_ceiling_delivers_below_it():
    fs, ch, n = 48000, 2, 48000 + 321
    g = torch.Generator().manual_seed(9)
    t = torch.arange(n, dtype=torch.float32) / fs
    names = ["drums", "bass", "vocals"]
    stems = {k: (a * torch.sin(2 * np.pi * f * t)[None] * torch.tensor([[1.0], [0.8]]) + 0.01 * torch.randn(ch, n, generator=g))
             for k, a, f in zip(names, (0.02, 0.05, 0.1), (180.0, 60.0, 900.0))}
    stems["drums"][:, 100::4800] += torch.tensor([[0.45], [-0.4]])             # sparse clicks: high peaks, little loudness
    stems["drums"][:, 2500::4800] += 0.3
    stems["drums"][:, 2501::4800] += 0.3                                       # pairs of samples: the peak lies between them
    origin = sum(stems.values()) + 0.001 * torch.randn(ch, n, generator=g)
    mix = {"dynamic": {"mix": 0.5, "drums": 1.5, "bass": -0.5}, "vocals": {"vocals": 1.0}}          # |gain| <= 2
    dev, org = {k: v.cuda() for k, v in stems.items()}, origin.cuda()
    loud = audio.loudness(org, dev, mix, samplerate=fs)
    peaks = audio.true_peak(org, dev, mix, samplerate=fs)
    ceiling = 10 ** (-1 / 20)
    for name in mix:
        print(f"{name}: {loud.integrated(name):.3f} LUFS, {peaks.dbtp(name):.3f} dBTP, sample peak {db(peaks.sample_peak(name)):.3f}; "
              f"gain to -14 LUFS {loud.gain(name, -14.0):.4f}, limit {peaks.gain_limit(name):.4f}")
    assert loud.gain("dynamic", -14.0) > peaks.gain_limit("dynamic") and loud.gain("vocals", -14.0) < peaks.gain_limit("vocals")
    norm = loud.normalised(-14.0, true_peaks=peaks, ceiling=-1.0)
    k = peaks.gain_limit("dynamic", -1.0)
    assert norm["dynamic"] == {"mix": 0.5 * k, "drums": 1.5 * k, "bass": -0.5 * k} and norm["vocals"] == loud.normalised(-14.0)["vocals"]
    frames = audio.deliver_mix(org, dev, norm, clip=None, fmt="f32")
    clamped = audio.deliver_mix(org, dev, norm, clip="clamp", fmt="f32")
    for name in mix:
        assert frames[name].shape == (n, ch)
        assert clamped[name].view(torch.int32).equal(frames[name].view(torch.int32))          # the clamp never acts
        again = audio.true_peak(None, {name: frames[name].t().contiguous()}, samplerate=fs)
        top = max(again.true_peak(name), again.sample_peak(name))
        print(f"{name}: delivered with max(true, sample) = {top:.6f} ({db(top):.4f} dBTP), ceiling {ceiling:.6f}")
        assert top <= ceiling * (1 + 1e-4)
    assert max(again.true_peak("vocals"), again.sample_peak("vocals")) < 0.5
    top = audio.true_peak(None, {"d": frames["dynamic"].t().contiguous()}, samplerate=fs)
    assert max(top.true_peak("d"), top.sample_peak("d")) >= ceiling * (1 - 1e-4)               # capped AT the ceiling
    # the output that was not capped reads the target
    delivered = audio.loudness(None, {"vocals": frames["vocals"].t().contiguous()}, samplerate=fs)
    assert abs(delivered.integrated("vocals") + 14.0) <= 1e-3
    quiet = audio.loudness(None, {"dynamic": frames["dynamic"].t().contiguous()}, samplerate=fs)
    assert quiet.integrated("dynamic") < -14.0 - 1.0


# ---- 3. the Separator ----------------------------------------------------------------------------------------------------------
BLOCK = 16384


@pytest.fixture(scope="module")
def sep():
    s = Separator(hd("f32", max_batch=2, channels=4, segment=3), device="cuda", shifts=1)
    assert list(s.model.sources) == NAMES
    return s


def feed(kind):
    """7 s and a few odd samples: (wav, sr, channels, pcm, blocks)."""
    if kind == "float blocks":
        wav = track(7 * SR + 123, seed=15) * 0.9
        return wav, None, None, None, [wav[:, i:i + BLOCK] for i in range(0, wav.shape[1], BLOCK)]
    q, wav = to_i16(track(7 * 48000 + 77, seed=17) * 0.9)
    data, frame = q.numpy().tobytes(), 2 * q.shape[1]
    return wav, 48000, 2, "i16", [data[i:i + BLOCK * frame] for i in range(0, len(data), BLOCK * frame)]


@pytest.mark.parametrize("kind,mix", [("float blocks", None), ("int16 at 48 kHz", REMIX)], ids=["float blocks", "int16 at 48 kHz"])
def test_levels_blocks_equal_levels_tensor(sep, kind, mix):
    wav, sr, channels, pcm, blocks = feed(kind)
    random.seed(5)
    loud, peaks, origin, stems = sep.levels_tensor(wav, mix, sr)
    after = random.getstate()
    length = wav.shape[1] if sr is None else wav.shape[1] * 147 // 160
    assert isinstance(loud, TrackLoudness) and isinstance(peaks, TrackTruePeaks)
    assert loud.length == peaks.length == length == origin.shape[1] and peaks.samplerate == SR and peaks.channels == 2
    assert peaks.names == loud.names == (tuple(mix) if mix is not None else (*NAMES, "mix"))
    assert peaks.mix == loud.mix and peaks.sources == loud.sources == tuple(NAMES)
    assert all(t.device.type == "cpu" for t in [origin, *stems.values()])
    assert all(0 < b < 0x7F800000 for b in (*peaks.bits, *peaks.sample_bits))
    # both are those of what came back
    assert audio.true_peak(origin, stems, mix, SR) == peaks and audio.loudness(origin, stems, mix, SR) == loud
    random.seed(5)
    only, _, _ = sep.loudness_tensor(wav, mix, sr)
    assert only == loud and random.getstate() == after
    reads = []

    def source():
        reads.append(1)
        return iter(blocks)

    random.seed(5)
    before = random.getstate()
    got_loud, got_peaks = sep.levels_blocks(source, mix, sr=sr, channels=channels, pcm=pcm)
    assert random.getstate() == before and before != after and len(reads) == 2
    assert got_peaks == peaks and got_peaks.bits == peaks.bits and got_peaks.sample_bits == peaks.sample_bits
    assert got_loud == loud and got_loud.energies.tobytes() == loud.energies.tobytes()
    assert sep.loudness_blocks(source, mix, sr=sr, channels=channels, pcm=pcm) == got_loud and random.getstate() == before
    # the two results belong together
    assert set(loud.normalised(-14.0, true_peaks=peaks)) == set(peaks.names)


def test_refusals_come_before_any_rng_call(sep, monkeypatch):
    wav = track(SR, seed=3)
    random.seed(11)
    state = random.getstate()
    with pytest.raises(ValueError, match="neither 'mix' nor one of the separated sources"):
        sep.levels_blocks(lambda: iter([wav]), {"a": {"piano": 1}})
    with pytest.raises(ValueError, match="neither 'mix' nor one of the separated sources"):
        sep.levels_tensor(wav, {"a": {"piano": 1}})
    cpu = Separator(sep.model, device="cpu")
    with pytest.raises(ValueError, match="runs on the GPU engines"):
        cpu.levels_blocks(lambda: iter([wav]))
    with pytest.raises(ValueError, match="runs on the GPU engines"):
        cpu.levels_tensor(wav)
    monkeypatch.setattr(sep.model, "sources", [f"s{i}" for i in range(9)])
    with pytest.raises(ValueError, match="1 to 8 sources"):
        sep.levels_blocks(lambda: iter([wav]))
    with pytest.raises(ValueError, match="1 to 8 sources"):
        sep.levels_tensor(wav)
    monkeypatch.undo()
    assert random.getstate() == state
