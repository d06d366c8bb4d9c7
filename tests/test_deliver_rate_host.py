"""Host side of delivery at another sample rate (`Delivery(samplerate=R)`, demucs_amd/stream.py; the arithmetic is
`audio.ConvertPlan(M, R)` with the model-rate samples a stream has emitted as the resampler's input): the per-call frame counts of
every partition sum to the whole track's, the hold bound holds and is reached, the carried span fits the history, every refusal
comes before `random` is touched, and a `Delivery` at the model's own rate builds today's rows."""
import math
import random
import re

import pytest
import torch

from demucs_amd import _lib, audio
from demucs_amd.api import Delivery, Separator
from demucs_amd.apply import apply_model_stream, apply_model_stream_group
from demucs_amd.hdemucs import HDemucs
from demucs_amd.hdemucs_weights import HDemucsConfig
from demucs_amd.stream import _deliver_rows, _Rate
from test_stream_host import Refusing

M = 44100
SOURCES = ["drums", "bass", "other", "vocals"]


def engine_model():
    return HDemucs(HDemucsConfig().sources, max_batch=1, channels=4)


# ---- the streaming arithmetic ---------------------------------------------------------------------------------------------------
def test_the_pairs_the_issue_names():
    p = audio.ConvertPlan(M, 48000)
    assert (p.old, p.new, p.width, p.klen, p.hold, p.carry) == (147, 160, 26, 199, 187, 198)
    assert (audio.ConvertPlan(M, 16000).old, audio.ConvertPlan(M, 16000).new) == (441, 160)
    assert (audio.ConvertPlan(M, 22050).old, audio.ConvertPlan(M, 22050).new) == (2, 1)
    assert (audio.ConvertPlan(2, 3).old, audio.ConvertPlan(2, 3).new) == (2, 3)


@pytest.mark.parametrize("rates", [(M, 48000), (M, 16000), (M, 22050), (2, 3)])
def test_every_partition_of_the_emitted_growth(rates):
    """A stream's `emitted` grows by arbitrary steps (0 and 1 among them); the rows `_Rate` builds per call carry the counts."""
    plan = audio.ConvertPlan(*rates)
    dl = Delivery("vocals")
    outputs = dl.outputs(SOURCES)
    reached, seen = False, set()
    for seed in range(12):
        g = random.Random(seed)
        L = g.choice([1, plan.width, plan.klen, 3 * plan.klen + 1, g.randint(1, 40 * plan.old)])
        if seed == 0:
            L = 5 * plan.klen
        rt = _Rate(plan, len(outputs), 2)
        rt.off = 0
        emitted = delivered = 0
        steps = []
        while emitted < L:
            steps.append(min(L - emitted, g.choice([0, 1, g.randint(1, plan.old), g.randint(1, 5 * plan.klen)])))
            emitted += steps[-1]
        if seed == 0:                                 # a push that stops one sample before the first frame completes
            steps = [plan.width + plan.old - 1, 0, 1, L - plan.width - plan.old]
        seen |= set(steps)
        emitted = 0
        calls = [(n, False) for n in steps] + [(0, True)]
        if seed % 2:                                  # finish() may emit the last samples itself
            calls = [(n, False) for n in steps[:-1]] + [(steps[-1], True)]
        for n, final in calls:
            side, h0 = rt.side, rt.h0
            rows = rt.rows(outputs, dl, 0x1000, n, emitted, final, 0, [0, 16])
            assert len(rows) == audio.RATE_COLS * len(outputs)
            first, second = rows[:audio.RATE_COLS], rows[audio.RATE_COLS:]
            n_in, before, out0, n_out, total = first[1], first[2], first[11], first[12], first[13]
            h_len, h_rd, h_wr, h_start, h_next = first[14:19]
            assert (n_in, before, out0) == (n, emitted, delivered) and out0 % plan.new == 0
            assert first[0] == (0x1000 if n else 0)
            assert total == (emitted + n if final else -1)
            # the history the call reads starts where the last call said, and covers what the first new frame needs
            assert h_len == plan.carry and h_start == h0 <= emitted and emitted - h_start <= plan.carry
            assert {h_rd, h_wr} == {0, 2 * plan.carry} and h_rd == side * 2 * plan.carry
            assert second[15] == h_rd + 4 * plan.carry and second[16] == h_wr + 4 * plan.carry
            emitted += n
            delivered += n_out
            if final:
                assert h_next == -1
            else:
                assert delivered == plan.ready(emitted)
                assert h_next == plan.carry_start(emitted) and 0 <= emitted - h_next <= plan.klen - 1      # the carried span
                assert (rt.side, rt.h0) == (1 - side, h_next)
                held = plan.new * emitted // plan.old - delivered
                assert 0 <= held <= plan.hold
                reached = reached or held == plan.hold
        assert emitted == L and delivered == plan.final_count(L) == math.floor(plan.new * L / plan.old)
    assert reached and {0, 1} <= seen


def test_the_bound_is_reached_one_sample_before_a_frame_completes():
    for rates in [(M, 48000), (M, 16000), (M, 22050), (2, 3)]:
        plan = audio.ConvertPlan(*rates)
        worst = max(plan.new * e // plan.old - plan.ready(e) for e in range(0, 6 * plan.klen))
        assert worst == plan.hold
        st = apply_model_stream(engine_model(), shifts=0, device="cuda", deliver=Delivery(samplerate=rates[1])) if rates[0] == M else None
        if st is not None:
            assert st.output_hold == plan.hold and st.delivered == 0 and st.rate.plan.klen == plan.klen


def test_kernel_geometry_matches_the_header():
    text = open(re.sub(r"tests.test_deliver_rate_host\.py$", "include/demucs_amd.h", __file__.replace("\\", "/"))).read()
    cols = dict(re.findall(r"#define MI_RATE_([A-Z0-9_]+) (\d+)", text))
    assert int(cols["COLS"]) == audio.RATE_COLS and int(cols["LDS_FLOATS"]) == audio.RATE_LDS_FLOATS
    order = ["SRC", "N_IN", "BEFORE", "KIND", "SEL", "CLIP", "FMT", "OLD", "NEW", "WIDTH", "BANK_OFF", "OUT0", "N_OUT", "TOTAL",
             "HIST_LEN", "HIST_RD", "HIST_WR", "HIST_START", "HIST_NEXT", "DST_OFF"]
    assert [int(cols[k]) for k in order] == list(range(audio.RATE_COLS))       # the order `_Rate.rows` writes
    assert "mi_deliver_resample_pcm" in _lib.SIGNATURES and len(_lib.SIGNATURES["mi_deliver_resample_pcm"][1]) == 13
    for rates, channels, runs in [((M, 48000), 2, 4), ((M, 16000), 2, 2), ((M, 16000), 1, 4), ((M, 48000), 8, 1)]:
        plan = audio.ConvertPlan(*rates)
        assert audio.rate_subruns(plan, channels) == runs
        lds = audio.rate_lds_floats(plan, channels)
        assert lds == channels * (8 * runs * plan.old + 2 * plan.width) <= audio.RATE_LDS_FLOATS
        per_group = 8 * runs * plan.new
        assert [audio.rate_groups(plan, channels, n) for n in (0, 1, per_group, per_group + 1)] == [1, 1, 1, 2]


# ---- refusals -------------------------------------------------------------------------------------------------------------------
REFUSALS = [
    (engine_model, "cuda", dict(stem="vocals", clip="rescale", samplerate=48000), "rescale"),
    (engine_model, "cuda", dict(stem="vocals", other_method="minus", samplerate=48000), "minus"),
    (engine_model, "cuda", dict(samplerate=44101), "44100 -> 44101"),            # a frame of 44100 samples: ConvertPlan's refusal
    (engine_model, "cuda", dict(samplerate=44058), "44100 -> 44058"),            # 1050:1049 fits one channel, not the model's two
    (engine_model, "cpu", dict(stem="vocals", samplerate=48000), "GPU engines"),
    (Refusing, "cpu", dict(stem="a", samplerate=48000), "GPU engines"),            # a non-engine model
    (Refusing, "cuda", dict(samplerate=48000), "GPU engines"),
]


@pytest.mark.parametrize("make,device,kw,match", REFUSALS)
def test_refusals_come_before_random(make, device, kw, match, monkeypatch):
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


def test_the_too_long_pair_is_a_matter_of_channels():
    assert audio.ConvertPlan(M, 44058).old == 1050                                # the converter itself takes it
    assert audio.delivery_rate_plan(M, 44058, 1) is not None
    with pytest.raises(ValueError, match="44100 -> 44058"):
        audio.delivery_rate_plan(M, 44058, 2)
    for bad in (0, -48000, 48000.5):
        with pytest.raises(ValueError, match="positive integer"):
            Delivery(samplerate=bad)


# ---- the model's own rate is today's path -----------------------------------------------------------------------------------------
def test_the_models_rate_and_none_build_todays_rows():
    plain = Delivery("vocals")
    assert repr(plain) == "Delivery(stem='vocals', other_method='add', clip='clamp', fmt='i16', samplerate=None)"
    assert "samplerate=48000" in repr(Delivery(samplerate=48000))
    model = engine_model()
    streams = []
    for dl in (plain, Delivery("vocals", samplerate=None), Delivery("vocals", samplerate=M)):
        assert dl.rate_plan(M, 2) is None
        random.seed(4)
        st = apply_model_stream(model, shifts=1, device="cuda", deliver=dl)
        assert st.rate is None and st.output_hold == 0 and st.delivered == 0
        streams.append((st.outputs, _deliver_rows(st.outputs, dl, 0x7000, 321, [0, 1296]), random.getstate()))
    assert streams[0] == streams[1] == streams[2]
    assert streams[0][1] == [0x7000, 0, 321, 0, 3, 2, 0, 0, 0, 0x7000, 0, 321, 1, 3, 2, 0, 0, 1296]
    random.seed(4)
    st = apply_model_stream(model, shifts=1, device="cuda", deliver=Delivery("vocals", samplerate=48000))
    assert random.getstate() == streams[0][2]                                      # the same RNG calls
    assert st.rate is not None and st.outputs == streams[0][0] and st.rate.size == 2 * 2 * 2 * 198


def test_deliver_samplerate_argument_errors_need_no_gpu():
    stems = {k: torch.zeros(2, 5) for k in SOURCES}
    with pytest.raises(ValueError, match="kazoo"):
        audio.deliver(torch.zeros(2, 5), stems, stem="kazoo", samplerate=(M, 48000))
    with pytest.raises(ValueError, match="format"):
        audio.deliver(torch.zeros(2, 5), stems, fmt="i24", samplerate=(M, 48000))
    with pytest.raises(ValueError, match="mode"):
        audio.deliver(torch.zeros(2, 5), stems, clip="loud", samplerate=(M, 48000))
    with pytest.raises(TypeError):
        audio.deliver(torch.zeros(2, 5), {k: torch.zeros(2, 5, dtype=torch.int16) for k in SOURCES}, samplerate=(M, 48000))
