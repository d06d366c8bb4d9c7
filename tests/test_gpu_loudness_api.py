"""Loudness through the Separator on the MI355X: `loudness_blocks` -- a track that never exists whole, its mix queued at the
model's rate until the stems of the same positions arrive -- has the bits of `loudness_tensor`, leaves `random` where it found it,
and its normalised gains make the next `separate_blocks` deliver at the target.  The float64 restatement is
tests/test_gpu_loudness.py's."""
import random

import numpy as np
import pytest
import torch

from demucs_amd import audio
from demucs_amd.api import Delivery, Separator
from test_gpu_ingest import to_i16
from test_gpu_loudness import lufs, whole_energies
from test_gpu_stream import track

pytestmark = pytest.mark.gpu
SR = 44100
BLOCK = 4096
REMIX = {"karaoke": {"mix": 1.0, "vocals": -1.0}, "practice": {"drums": 2.0, "bass": 0.5, "other": 0.5, "vocals": 0.5}}
NO_MIX = {"backing": {"drums": 1.0, "bass": 1.0, "other": 1.0}, "vocals": {"vocals": 1.0}}


def feed(kind):
    """A 1.3 s track as the floats of an int16 feed: (wav, sr, channels, int16 frames)."""
    if kind == "model":
        q, wav = to_i16(track(int(1.3 * SR), seed=15) * 0.9)
        return wav, None, None, q
    q, wav = to_i16(track(int(1.3 * 48000), seed=17)[:1] * 0.9)
    return wav, 48000, 1, q


def blocks_of(wav, q, pcm):
    if pcm is None:
        return [wav[:, i:i + BLOCK] for i in range(0, wav.shape[1], BLOCK)]
    data, frame = q.numpy().tobytes(), 2 * q.shape[1]
    return [data[i:i + BLOCK * frame] for i in range(0, len(data), BLOCK * frame)]


@pytest.fixture(scope="module")
def sep():
    s = Separator("demucs_unittest", device="cuda", shifts=1)
    assert s.model.sources == ["drums", "bass", "other", "vocals"]
    return s


@pytest.mark.parametrize("pcm", [None, "i16"])
@pytest.mark.parametrize("kind", ["model", "48k mono"])
@pytest.mark.parametrize("mix", [REMIX, NO_MIX, None], ids=["mix term", "stems only", "default"])
def test_blocks_equal_the_whole_track(sep, mix, kind, pcm):
    wav, sr, channels, q = feed(kind)
    random.seed(5)
    want, origin, stems = sep.loudness_tensor(wav, mix, sr)
    after = random.getstate()
    length = wav.shape[1] if sr is None else wav.shape[1] * 147 // 160
    assert want.length == length == origin.shape[1] and origin.shape[0] == 2 and want.samplerate == SR
    assert want.energies.shape == (len(want.names), 2, length // 4410) and np.isfinite(want.energies).all()
    assert want.names == (tuple(mix) if mix is not None else ("drums", "bass", "other", "vocals", "mix"))
    assert all(t.device.type == "cpu" for t in [origin, *stems.values()])
    # the TrackLoudness is that of what came back
    again = audio.loudness(origin, stems, mix, SR)
    assert again == want
    reads = []

    def source():
        reads.append(1)
        return iter(blocks_of(wav, q, pcm))

    random.seed(5)
    before = random.getstate()
    got = sep.loudness_blocks(source, mix, sr=sr, channels=channels, pcm=pcm)
    assert random.getstate() == before and before != after
    assert len(reads) == 2
    assert got.energies.tobytes() == want.energies.tobytes()
    assert got == want


def test_the_normalised_gains_deliver_the_target(sep):
    wav, _, _, _ = feed("model")
    source = lambda: iter(blocks_of(wav, None, None))       # noqa: E731
    random.seed(7)
    measured = sep.loudness_blocks(source, REMIX)
    target = -20.0
    frames = {}
    for out in sep.separate_blocks(source, deliver=Delivery(mix=measured.normalised(target), clip=None, fmt="f32")):
        for name, f in out.items():
            frames.setdefault(name, []).append(f.cpu())
    coef = audio.k_weighting(SR)
    for name in REMIX:
        v = torch.cat(frames[name]).t().numpy()
        assert v.shape == (2, wav.shape[1])
        got, blocks = lufs(whole_energies(v, coef, SR // 10), SR // 10)
        have = measured.integrated(name)
        print(f"{name}: measured {have:.4f} LUFS, delivered at {got:.6f} LUFS")
        # every block over the absolute gate before and after, so that scaling moves the reading by exactly the gain
        assert min(blocks) > -70 and min(blocks) - (target - have) > -70
        assert abs(got - target) <= 1e-3


def test_refusals(sep):
    wav, _, _, _ = feed("model")
    with pytest.raises(ValueError, match="neither 'mix' nor one of the separated sources"):
        sep.loudness_blocks(lambda: iter([wav]), {"a": {"piano": 1}})
    with pytest.raises(ValueError, match="runs on the GPU engines"):
        Separator(sep.model, device="cpu").loudness_blocks(lambda: iter([wav]))
    with pytest.raises(ValueError, match="runs on the GPU engines"):
        Separator(sep.model, device="cpu").loudness_tensor(wav)
