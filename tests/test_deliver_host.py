"""Host side of the delivery path (demucs_amd/audio.py `deliver` / `wav_header`, demucs_amd/stream.py `Delivery`): the names and
order of the outputs follow the reference's save loop (demucs/separate.py:178-218), every refusal of a delivering stream comes
before `random` is touched or a model is called, and the WAVE headers are what the standard library reads."""
import io
import random
import struct
import wave

import pytest
import torch

from demucs_amd import audio
from demucs_amd.api import Delivery, Separator
from demucs_amd.apply import BagOfModels, apply_model_stream, apply_model_stream_group
from demucs_amd.hdemucs import HDemucs
from demucs_amd.hdemucs_weights import HDemucsConfig
from test_apply_host import ToyModel
from test_stream_host import Refusing

SOURCES = ["drums", "bass", "other", "vocals"]


# ---- the outputs and their order ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stem,method,want", [
    (None, "add", [("drums", 0, 0), ("bass", 0, 1), ("other", 0, 2), ("vocals", 0, 3)]),
    (None, "minus", [("drums", 0, 0), ("bass", 0, 1), ("other", 0, 2), ("vocals", 0, 3)]),
    ("vocals", "add", [("vocals", 0, 3), ("no_vocals", 1, 3)]),
    ("vocals", "minus", [("minus_vocals", 2, 3), ("vocals", 0, 3)]),
    ("vocals", "none", [("vocals", 0, 3)]),
    ("drums", "add", [("drums", 0, 0), ("no_drums", 1, 0)]),
    ("bass", "minus", [("minus_bass", 2, 1), ("bass", 0, 1)]),
])
def test_outputs_follow_the_reference_save_loop(stem, method, want):
    assert audio.delivery_outputs(SOURCES, stem, method) == want
    assert Delivery(stem, method).outputs(SOURCES) == want
    # the names `audio.two_stems` gives the same request, in the same order
    if stem is not None:
        names = {"add": [stem, "no_" + stem], "minus": ["minus_" + stem, stem], "none": [stem]}[method]
        assert [n for n, _, _ in want] == names


def test_layout_is_16_byte_aligned_and_dense():
    outs = audio.delivery_outputs(SOURCES, "vocals", "add")
    offs, end = audio.deliver_layout(outs, 3, 2, "i16")            # 12 bytes per output
    assert offs == [0, 16] and end == 28
    offs, end = audio.deliver_layout(outs, 3, 2, "f32", at=28)
    assert offs == [32, 64] and end == 88
    buf = torch.arange(28, dtype=torch.uint8)
    views = audio.deliver_views(buf, outs, [0, 16], 3, 2, "i16")
    assert list(views) == ["vocals", "no_vocals"] and views["no_vocals"].shape == (3, 2) and views["no_vocals"].dtype == torch.int16
    assert views["no_vocals"][0, 0].item() == 16 + 17 * 256


# ---- Delivery validation and the refusals of a stream ----------------------------------------------------------------------------
@pytest.mark.parametrize("kw,match", [
    (dict(other_method="sum"), "other_method"),
    (dict(clip="loud"), "mode"),
    (dict(fmt="i24"), "format"),
])
def test_delivery_validates_its_arguments(kw, match):
    with pytest.raises(ValueError, match=match):
        Delivery("vocals", **kw)


def test_delivery_defaults():
    d = Delivery()
    assert (d.stem, d.other_method, d.clip, d.fmt) == (None, "add", "clamp", "i16")
    assert Delivery(clip=None).clip_code == 0 and Delivery(clip="none").clip_code == 0 and Delivery(clip="tanh").clip_code == 3


def engine_model():
    return HDemucs(HDemucsConfig().sources, max_batch=1, channels=4)


REFUSALS = [
    (Refusing, "cpu", dict(stem="a", clip="rescale"), "rescale"),
    (Refusing, "cpu", dict(stem="a", other_method="minus"), "minus"),
    (Refusing, "cpu", dict(stem="kazoo"), "kazoo"),
    (Refusing, "cpu", dict(stem="a"), "GPU engines"),                  # plain-torch route: no delivery kernels there
    (Refusing, "cuda", dict(), "GPU engines"),
    (engine_model, "cpu", dict(stem="vocals"), "GPU engines"),           # an engine on a CPU device
    (engine_model, "cuda", dict(stem="vocals", clip="rescale"), "rescale"),
    (engine_model, "cuda", dict(stem="vocals", other_method="minus"), "minus"),
    (engine_model, "cuda", dict(stem="a"), "not in the separated sources"),
]


@pytest.mark.parametrize("make,device,kw,match", REFUSALS)
def test_stream_refusals_come_before_random(make, device, kw, match, monkeypatch):
    model = make()
    sep = Separator(model, device=device, shifts=1)
    touched = []
    for name in ("randint", "randrange"):
        monkeypatch.setattr(random, name, lambda *a, _n=name: touched.append(_n) or 0)
    state = random.getstate()
    with pytest.raises(ValueError, match=match):
        sep.separate_stream(0.0, 1.0, deliver=Delivery(**kw))
    with pytest.raises(ValueError, match=match):
        apply_model_stream(model, shifts=1, device=device, deliver=Delivery(**kw))
    g = sep.separate_stream_group()
    with pytest.raises(ValueError, match=match):
        g.open(0.0, 1.0, deliver=Delivery(**kw))
    g2 = apply_model_stream_group(model, shifts=1, device=device)
    with pytest.raises(ValueError, match=match):
        g2.open(deliver=Delivery(**kw))
    assert random.getstate() == state and not touched
    assert g.open_keys == [] and g2.open_keys == []


def test_bag_of_generic_models_is_refused():
    state = random.getstate()
    with pytest.raises(ValueError, match="GPU engines"):
        apply_model_stream(BagOfModels([Refusing(), Refusing()]), shifts=0, deliver=Delivery("a"))
    assert random.getstate() == state


def test_an_accepted_delivery_draws_what_the_plain_stream_draws():
    """On an engine with a GPU device the stream is accepted without a GPU at hand (nothing runs before the first push), and it
    makes the RNG calls of the same stream without `deliver`."""
    model = engine_model()
    random.seed(5)
    apply_model_stream(model, shifts=1, device="cuda")
    want = random.getstate()
    random.seed(5)
    st = apply_model_stream(model, shifts=1, device="cuda", deliver=Delivery("vocals"))
    assert random.getstate() == want
    assert [n for n, _, _ in st.outputs] == ["vocals", "no_vocals"]


def test_without_deliver_a_stream_is_unchanged():
    st = apply_model_stream(ToyModel(), shifts=0)
    out = st.push(torch.zeros(2, 450))
    assert isinstance(out, torch.Tensor) and out.shape[:2] == (3, 2)
    sep = Separator(ToyModel(), device="cpu", shifts=0)
    assert set(sep.separate_stream().push(torch.zeros(2, 450))) == set(ToyModel.sources)


def test_deliver_argument_errors_need_no_gpu():
    stems = {k: torch.zeros(2, 5) for k in SOURCES}
    with pytest.raises(ValueError, match="kazoo"):
        audio.deliver(torch.zeros(2, 5), stems, stem="kazoo")
    with pytest.raises(ValueError, match="other_method"):
        audio.deliver(torch.zeros(2, 5), stems, stem="vocals", other_method="sum")
    with pytest.raises(ValueError, match="mode"):
        audio.deliver(torch.zeros(2, 5), stems, clip="loud")
    with pytest.raises(ValueError, match="format"):
        audio.deliver(torch.zeros(2, 5), stems, fmt="i24")
    with pytest.raises(TypeError):
        audio.deliver(torch.zeros(2, 5), {k: torch.zeros(2, 5, dtype=torch.int16) for k in SOURCES})
    empty = audio.deliver(torch.zeros(2, 0), {k: torch.zeros(2, 0) for k in SOURCES}, stem="vocals")
    assert list(empty) == ["vocals", "no_vocals"] and all(v.shape == (0, 2) and v.dtype == torch.int16 for v in empty.values())


# ---- WAVE headers --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("channels,rate,frames", [(2, 44100, 1000), (1, 8000, 1), (2, 48000, 0), (6, 96000, 17)])
def test_int16_header_round_trips_through_wave(channels, rate, frames):
    g = torch.Generator().manual_seed(frames)
    pcm = torch.randint(-32768, 32768, (frames, channels), generator=g, dtype=torch.int32).to(torch.int16)
    head = audio.wav_header(frames, rate, channels, "i16")
    assert len(head) == 44
    with wave.open(io.BytesIO(head + pcm.numpy().tobytes()), "rb") as w:
        assert (w.getnchannels(), w.getframerate(), w.getnframes(), w.getsampwidth()) == (channels, rate, frames, 2)
        data = w.readframes(frames)
    got = torch.frombuffer(bytearray(data), dtype=torch.int16).view(frames, channels) if frames else pcm
    assert torch.equal(got, pcm)


def test_float_header_fields():
    head = audio.wav_header(1000, 44100, 2, "f32")
    assert len(head) == 58
    riff, size, wave_id, fmt_id, fmt_len = struct.unpack_from("<4sI4s4sI", head, 0)
    assert (riff, wave_id, fmt_id, fmt_len) == (b"RIFF", b"WAVE", b"fmt ", 18)
    tag, channels, rate, byte_rate, align, bits, ext = struct.unpack_from("<HHIIHHH", head, 20)
    assert (tag, channels, rate, byte_rate, align, bits, ext) == (3, 2, 44100, 44100 * 8, 8, 32, 0)
    fact_id, fact_len, fact_frames, data_id, data_len = struct.unpack_from("<4sII4sI", head, 38)
    assert (fact_id, fact_len, fact_frames, data_id, data_len) == (b"fact", 4, 1000, b"data", 8000)
    assert size == len(head) - 8 + 8000


def test_live_stream_sizes():
    head = audio.wav_header(None, 44100, 2, "i16")
    assert struct.unpack_from("<I", head, 4)[0] == 0xFFFFFFFF and struct.unpack_from("<I", head, 40)[0] == 0xFFFFFFFF
    assert head[8:36] == audio.wav_header(5, 44100, 2, "i16")[8:36]          # the format chunk does not depend on the length
    head = audio.wav_header(None, 44100, 2, "f32")
    assert [struct.unpack_from("<I", head, o)[0] for o in (4, 46, 54)] == [0xFFFFFFFF] * 3


def test_header_refusals():
    with pytest.raises(ValueError, match="format"):
        audio.wav_header(1, 44100, 2, "i24")
    with pytest.raises(ValueError, match="32-bit"):
        audio.wav_header(2 ** 30, 44100, 2, "i16")                 # 4 GiB of data
    with pytest.raises(ValueError, match="32-bit"):
        audio.wav_header(-1, 44100, 2, "i16")
    with pytest.raises(ValueError, match="channels"):
        audio.wav_header(1, 44100, 0, "i16")
