"""Host side of gain automation (`audio.mix_changes`, `audio.auto_span`, `audio.auto_table`, `Delivery(changes=)`,
`ModelStream.change_mix`, demucs_amd/stream.py): what a schedule accepts and how it is refused, which changes a call passes to the
kernel with which base gains, how the table is packed, and the header's constants.  Nothing here runs on a device."""
import random
import re

import numpy as np
import pytest

from demucs_amd import _lib, audio
from demucs_amd.api import Delivery, Separator, TrackPeaks
from demucs_amd.apply import apply_model_stream, apply_model_stream_group
from demucs_amd.stream import _auto_rows
from test_deliver_rate_host import M, SOURCES, engine_model

MIX = {"practice": {"mix": 1, "vocals": 10 ** -0.6 - 1}, "bass_up": {"bass": 2, "drums": 0}}
CHANGES = {"practice": [(5000, 0, {"mix": 1}), (1000, 2000, {"mix": 1, "vocals": -1}), (3000, 0, {})],
           "bass_up": [(0, 10, {"bass": 0.1})]}
F = np.float32


def f32(v):
    return float(F(v))


# ---- the resolver ---------------------------------------------------------------------------------------------------------------
def test_changes_are_ordered_resolved_and_rounded_once():
    gains = audio.mix_gains(MIX, SOURCES)
    got = audio.mix_changes(CHANGES, gains, SOURCES)
    assert list(got) == ["practice", "bass_up"]
    assert got["practice"] == [(1000, 2000, (1.0, 0.0, 0.0, 0.0, -1.0)), (3000, 0, (0.0,) * 5), (5000, 0, (1.0, 0.0, 0.0, 0.0, 0.0))]
    assert got["bass_up"] == [(0, 10, (0.0, 0.0, f32(0.1), 0.0, 0.0))]
    # without the sources: what can be checked is, and the terms stay named
    loose = audio.mix_changes(CHANGES, audio.mix_gains(MIX))
    assert loose["practice"][0] == (1000, 2000, {"mix": 1.0, "vocals": -1.0}) and loose["bass_up"] == [(0, 10, {"bass": f32(0.1)})]
    assert audio.mix_changes(loose, gains, SOURCES) == got             # what a Delivery keeps resolves to the same
    # nothing scheduled
    assert audio.mix_changes(None, gains, SOURCES) == {} and audio.mix_changes({}, gains) == {}
    assert audio.mix_changes({"practice": []}, gains, SOURCES) == {}
    # changes at one position keep their order; a change may begin where the ramp before it ends; floats that are whole numbers
    two = audio.mix_changes({"practice": [(7, 0, {"bass": 1}), (7, 3.0, {"bass": 2}), (10.0, 0, {"bass": 3})]}, gains, SOURCES)
    assert [(a, r, g[2]) for a, r, g in two["practice"]] == [(7, 0, 1.0), (7, 3, 2.0), (10, 0, 3.0)]
    # the largest gain a change takes
    big = audio.mix_changes({"practice": [(0, 0, {"bass": 2.0 ** 64, "drums": -2.0 ** 64})]}, gains, SOURCES)
    assert big["practice"][0][2][1:3] == (-2.0 ** 64, 2.0 ** 64)


BAD_CHANGES = [
    ({"karaoke": [(0, 0, {"mix": 1})]}, "none of the outputs"),
    ({"practice": [(0, 0, {"piano": 1})]}, "'piano'"),
    ({"practice": [(0, 0, {"mix": float("nan")})]}, "finite"),
    ({"practice": [(0, 0, {"mix": float("inf")})]}, "finite"),
    ({"practice": [(0, 0, {"mix": 1e39})]}, "finite"),
    ({"practice": [(0, 0, {"bass": 2.0 ** 65})]}, r"2\*\*64"),
    ({"practice": [(0, 0, {"bass": -3e19})]}, r"2\*\*64"),
    ({"practice": [(0, 0, {"bass": "1"})]}, "must be a number"),
    ({"practice": [(0, 0, {"bass": True})]}, "must be a number"),
    ({"practice": [(-1, 0, {"mix": 1})]}, "`at`"),
    ({"practice": [(1.5, 0, {"mix": 1})]}, "`at`"),
    ({"practice": [(None, 0, {"mix": 1})]}, "`at`"),
    ({"practice": [(0, -1, {"mix": 1})]}, "`ramp`"),
    ({"practice": [(0, 0.5, {"mix": 1})]}, "`ramp`"),
    ({"practice": [(0, 2 ** 61, {"mix": 1})]}, "`ramp`"),
    ({"practice": [(100, 50, {"mix": 1}), (149, 0, {"mix": 0})]}, "before the ramp from 100 ends at 150"),
    ({"practice": [(149, 0, {"mix": 0}), (100, 50, {"mix": 1})]}, "do not overlap"),
    ({"practice": [(0, 0, [1.0])]}, "needs"),
    ({"practice": [(0, {"mix": 1})]}, "needs"),
    ({"practice": (0, 0, {"mix": 1})}, "needs"),
    ({"practice": 5}, "needs a list"),
    ([("practice", [])], "is expected"),
]


@pytest.mark.parametrize("changes,match", BAD_CHANGES)
def test_change_validation(changes, match):
    with pytest.raises(ValueError, match=match):
        audio.mix_changes(changes, audio.mix_gains(MIX, SOURCES), SOURCES)
    if "piano" not in match:                               # all but an unknown term is refused before the sources are known
        with pytest.raises(ValueError, match=match):
            Delivery(mix=MIX, changes=changes)


# ---- Delivery -------------------------------------------------------------------------------------------------------------------
def test_delivery_carries_a_schedule():
    dl = Delivery(mix=MIX, fmt="f32", changes=CHANGES)
    assert dl.changes == audio.mix_changes(CHANGES, audio.mix_gains(MIX)) and dl.mix == MIX
    assert dl.schedule(SOURCES) == audio.mix_changes(CHANGES, audio.mix_gains(MIX, SOURCES), SOURCES)
    assert "changes={'practice': [(1000, 2000, " in repr(dl) and repr(dl).endswith("})]})")
    kept = Delivery(mix=MIX, changes=CHANGES, clip="tanh").with_peaks(None)
    assert kept.changes == dl.changes and kept.mix == MIX and kept.clip == "tanh"
    assert Delivery(mix=MIX, changes=dl.changes).changes == dl.changes                 # what it keeps can be passed again
    assert dl.for_stream(SOURCES, True, M, 2) == dl.outputs(SOURCES)
    # nothing scheduled is no schedule: the delivery of the fixed gains, and its repr
    for none in (None, {}, {"practice": []}):
        plain = Delivery(mix=MIX, changes=none)
        assert plain.changes is None and plain.schedule(SOURCES) == {} and "changes" not in repr(plain)
        assert repr(plain) == repr(Delivery(mix=MIX))
    assert Delivery("vocals").changes is None and Delivery("vocals", changes={}).changes is None
    # positional: `changes` is the last argument, behind `mix`
    assert Delivery(None, "add", "clamp", "i16", None, None, MIX, CHANGES).changes == dl.changes


def test_changes_go_with_a_mix():
    with pytest.raises(ValueError, match="goes with mix="):
        Delivery(changes=CHANGES)
    with pytest.raises(ValueError, match="goes with mix="):
        Delivery("vocals", changes={"vocals": [(0, 0, {"vocals": 1})]})


def peaks_for(mix):
    return TrackPeaks(list(mix), [0x3FC00000] * len(mix), mix=audio.mix_identity(audio.mix_gains(mix, SOURCES)))


STREAM_REFUSALS = [
    (dict(mix=MIX, changes=CHANGES, clip="rescale"), "gain changes.*clip='rescale'"),
    (dict(mix=MIX, changes=CHANGES, clip="rescale", peaks="measure"), "gain changes.*clip='rescale'"),
    (dict(mix=MIX, changes=CHANGES, clip="rescale", peaks=peaks_for(MIX)), "TrackPeaks carries none"),
    (dict(mix=MIX, changes={"practice": [(0, 0, {"piano": 1})]}), "'piano'"),
]


@pytest.mark.parametrize("kw,match", STREAM_REFUSALS)
def test_stream_refusals_come_before_random_and_open_no_slot(kw, match, monkeypatch):
    model = engine_model()
    sep = Separator(model, device="cuda", shifts=1)
    touched = []
    for name in ("randint", "randrange"):
        monkeypatch.setattr(random, name, lambda *a, _n=name: touched.append(_n) or 0)
    dl = Delivery(**kw)                                    # the Delivery itself stands: the whole-track call rescales with changes
    with pytest.raises(ValueError, match=match):
        dl.for_stream(SOURCES, True, M, 2)
    with pytest.raises(ValueError, match=match):
        next(sep.separate_blocks(lambda: iter([]), deliver=dl))
    with pytest.raises(ValueError, match=match):
        sep.separate_stream(0.0, 1.0, deliver=dl)
    with pytest.raises(ValueError, match=match):
        apply_model_stream(model, shifts=1, device="cuda", deliver=dl)
    g = sep.separate_stream_group()
    with pytest.raises(ValueError, match=match):
        g.open(0.0, 1.0, deliver=dl)
    g2 = apply_model_stream_group(model, shifts=1, device="cuda")
    with pytest.raises(ValueError, match=match):
        g2.open(deliver=dl)
    assert not touched and g.open_keys == [] and g2.open_keys == []


# ---- what a call passes ---------------------------------------------------------------------------------------------------------
BASE = (1.0, 0.0, 0.0, 0.0, 0.5)
G1, G2 = (0.0, 1.0, 0.0, 0.0, 0.0), (0.25, 0.0, 2.0, 0.0, 0.0)
SCHEDULE = [(1000, 500, G1), (2000, 0, G2)]                # a ramp over [1000, 1500), a step at 2000


@pytest.mark.parametrize("t0,n,want", [
    (0, 1000, (BASE, [], 0)),                               # before the ramp: frame 999 is the last one, the change begins at 1000
    (0, 1001, (BASE, SCHEDULE[:1], 0)),                     # frame 1000 is the change's first (it still has the old gains)
    (990, 20, (BASE, SCHEDULE[:1], 0)),
    (1200, 100, (BASE, SCHEDULE[:1], 0)),                   # inside the ramp
    (1499, 1, (BASE, SCHEDULE[:1], 0)),                     # its last moving frame
    (1500, 100, (G1, [], 1)),                               # frame at + ramp has the new gains exactly: the change is behind
    (1400, 700, (BASE, SCHEDULE, 0)),                       # across both
    (1500, 501, (G1, SCHEDULE[1:], 1)),
    (1999, 1, (G1, [], 1)),
    (2000, 1, (G2, [], 2)),                                 # a step is reached at its own frame
    (5000, 64, (G2, [], 2)),                                # after everything
])
def test_a_call_passes_the_changes_that_reach_into_its_span(t0, n, want):
    assert audio.auto_span(BASE, SCHEDULE, t0, n) == want
    assert audio.auto_span(BASE, [], t0, n) == (BASE, [], 0)


def test_the_table_carries_rows_positions_and_changes_bit_exact():
    gains = [("a", BASE), ("b", G2)]
    rows = audio.mix_rows(gains, 0x7000, 321, 0x9004, 5000, (0.25, 1.5), 2, 6, "i16", [0, 1296])
    table = audio.auto_table(rows, [1400, 77], [SCHEDULE, []])
    R, K = audio.AUTO_COLS, audio.AUTO_CHG_COLS
    assert (R, K) == (18, 7) and len(table) == 2 * R + 2 * K
    a, b = table[:R], table[R:2 * R]
    assert a[:15] == rows[:15] and b[:15] == rows[15:]      # MI_MIX_*'s columns where they were, the base gains among them
    assert a[15:] == [1400, 2 * R, 2] and b[15:] == [77, 2 * R + 2 * K, 0]
    first, second = table[2 * R:2 * R + K], table[2 * R + K:]
    assert first[:2] == [1000, 500] and second[:2] == [2000, 0]
    assert np.array(first[2:], dtype=np.int64).view(F).tolist() == list(G1) + [0.0] * 5
    assert np.array(second[2:], dtype=np.int64).view(F).tobytes() == np.array(list(G2) + [0.0] * 5, dtype=F).tobytes()
    assert all(isinstance(v, int) for v in table)
    assert audio.auto_table([], [], []) == []


def open_stream(**kw):
    random.seed(1)
    return apply_model_stream(engine_model(), shifts=1, device="cuda", deliver=Delivery(mix=MIX, fmt="f32", **kw))


def test_a_streams_rows_follow_the_emit_point_and_drop_what_is_behind():
    st = open_stream(changes={"practice": [(1000, 500, {"bass": 1}), (2000, 0, {"mix": 0.25, "other": 2})]})
    assert st.schedule == [[(1000, 500, G1[:1] + (0.0, 1.0, 0.0, 0.0)), (2000, 0, (0.25, 0.0, 0.0, 2.0, 0.0))], []]
    assert st.auto_end == [2000, 0] and st.auto_base == [g for _, g in audio.mix_gains(MIX, SOURCES)]
    ramp, step = st.schedule[0]
    practice, bass_up = st.auto_base
    # before the ramp: no change is passed; the mix is named because the base gains read it
    rows, changes = _auto_rows(st, 0x7000, 100, 0, 0x100000, 0, 9000, [0, 800])
    assert changes == [[], []] and rows == audio.mix_rows(audio.mix_gains(MIX, SOURCES), 0x7000, 100, 0x100000, 9000, None, 2, 0,
                                                           "f32", [0, 800])
    # into the ramp: the mix at the emit point of the window
    rows, changes = _auto_rows(st, 0x7000, 200, 900, 0x100000, 400, 9000, [0, 1600])
    assert changes == [[ramp], []] and rows[2] == 0x100000 + 4 * 500 and len(st.schedule[0]) == 2
    # past it: the ramp is behind for good and its gains are the base; they read no mix, the step ahead in the span does
    rows, changes = _auto_rows(st, 0x7000, 600, 1500, 0x100000, 1500, 9000, [0, 4800])
    assert changes == [[step], []] and st.schedule == [[step], []] and st.auto_base == [ramp[2], bass_up]
    assert np.array(rows[6:11], dtype=np.int64).view(F).tolist()[:5] == list(ramp[2]) and rows[2] == 0x100000
    # a span in which no gain reads the mix names no window, whatever its start
    assert _auto_rows(st, 0x7000, 100, 1600, 0x100000, 9999, 9000, [0, 800])[0][2] == 0
    with pytest.raises(AssertionError, match="past the emit point"):
        _auto_rows(st, 0x7000, 500, 1600, 0x100000, 1601, 9000, [0, 4000])
    rows, changes = _auto_rows(st, 0x7000, 10, 2100, 0x100000, 0, 9000, [0, 80])
    assert changes == [[], []] and st.schedule == [[], []] and st.auto_base == [step[2], bass_up] and st.auto_end == [2000, 0]
    assert practice == audio.mix_gains(MIX, SOURCES)[0][1]


# ---- change_mix -----------------------------------------------------------------------------------------------------------------
def test_change_mix_appends_and_never_contradicts_what_was_delivered():
    st = open_stream()
    assert st.schedule is None and st.auto_base is None     # no change yet: the fixed gains' launches
    st.emitted = 4000
    st.change_mix({"practice": {"mix": 1, "vocals": -1}}, ramp=100)            # at=None: at `emitted`
    assert st.schedule == [[(4000, 100, (1.0, 0.0, 0.0, 0.0, -1.0))], []] and st.auto_end == [4100, 0]
    st.change_mix({"practice": {}, "bass_up": {"bass": 1}})                    # None: the end of the last ramp, or `emitted`
    assert st.schedule[0][1] == (4100, 0, (0.0,) * 5) and st.schedule[1] == [(4000, 0, (0.0, 0.0, 1.0, 0.0, 0.0))]
    st.change_mix({"bass_up": {"bass": 2}}, at=4000, ramp=7)                   # at the end of a step: allowed
    st.emitted = 4200
    st.change_mix({"practice": {"mix": 1}}, at=4200)
    assert st.auto_end == [4200, 4007]
    before = [list(s) for s in st.schedule]
    with pytest.raises(ValueError, match=r"at=4199 lies before the 4200 frames"):
        st.change_mix({"bass_up": {"bass": 1}}, at=4199)
    st.change_mix({"practice": {"mix": 1}}, at=5000, ramp=1000)
    with pytest.raises(ValueError, match=r"at=5999 lies before 6000, where the last ramp of output 'practice' ends"):
        st.change_mix({"practice": {"mix": 0}}, at=5999)
    before[0].append((5000, 1000, (1.0, 0.0, 0.0, 0.0, 0.0)))
    # all or none: the second output's refusal leaves the first untouched
    with pytest.raises(ValueError, match="at=5500 lies before 6000"):
        st.change_mix({"bass_up": {"bass": 1}, "practice": {"mix": 0}}, at=5500)
    for bad, match in (({"karaoke": {"mix": 1}}, "none of the outputs"), ({"practice": {"piano": 1}}, "'piano'"),
                       ({"practice": {"mix": float("inf")}}, "finite"), ({}, "non-empty"), (None, "non-empty")):
        with pytest.raises(ValueError, match=match):
            st.change_mix(bad)
    with pytest.raises(ValueError, match="`ramp`"):
        st.change_mix({"practice": {"mix": 1}}, ramp=-1)
    with pytest.raises(ValueError, match="`at`"):
        st.change_mix({"practice": {"mix": 1}}, at=-5)
    assert st.schedule == before


def test_change_mix_needs_a_remixing_stream():
    model = engine_model()
    for dl in (None, Delivery("vocals"), Delivery()):
        random.seed(1)
        st = apply_model_stream(model, shifts=1, device="cuda", deliver=dl)
        with pytest.raises(ValueError, match=r"open it with Delivery\(mix="):
            st.change_mix({"practice": {"mix": 1}})
    random.seed(1)
    st = apply_model_stream(model, shifts=1, device="cuda", deliver=Delivery(mix=MIX, clip="rescale", peaks=peaks_for(MIX)))
    with pytest.raises(ValueError, match="carries no schedule"):
        st.change_mix({"practice": {"mix": 1}})
    assert st.schedule is None


def test_the_wrappers_pass_change_mix_on():
    model = engine_model()
    sep = Separator(model, device="cuda", shifts=1)
    ss = sep.separate_stream(0.0, 1.0, deliver=Delivery(mix=MIX))
    ss.change_mix({"practice": {"mix": 0.5}}, at=10, ramp=5)
    assert ss.stream.schedule == [[(10, 5, (0.5, 0.0, 0.0, 0.0, 0.0))], []]
    cs = sep.separate_stream(0.0, 1.0, sr=48000, convert=True, deliver=Delivery(mix=MIX))
    cs.change_mix({"bass_up": {}})                          # model-rate frames on a converting stream too
    assert cs.stream.schedule == [[], [(0, 0, (0.0,) * 5)]]
    for g in (sep.separate_stream_group(), apply_model_stream_group(model, shifts=1, device="cuda")):
        key = g.open(0.0, 1.0, deliver=Delivery(mix=MIX)) if g.__class__.__name__ == "SeparatorStreamGroup" else \
            g.open(deliver=Delivery(mix=MIX))
        other = g.open(0.0, 1.0) if g.__class__.__name__ == "SeparatorStreamGroup" else g.open()
        g.change_mix(key, {"practice": {"vocals": 1}}, ramp=3)
        group = getattr(g, "group", g)
        assert group._streams[key].schedule == [[(0, 3, (0.0, 0.0, 0.0, 0.0, 1.0))], []]
        with pytest.raises(ValueError, match=r"open it with Delivery\(mix="):
            g.change_mix(other, {"practice": {"vocals": 1}})
        with pytest.raises(ValueError, match="unknown or finished stream key"):
            g.change_mix(99, {"practice": {"vocals": 1}})


# ---- the header -----------------------------------------------------------------------------------------------------------------
def test_constants_match_the_header():
    text = open(re.sub(r"tests.test_deliver_auto_host\.py$", "include/demucs_amd.h", __file__.replace("\\", "/"))).read()
    auto = {k: int(v) for k, v in re.findall(r"#define MI_AUTO_([A-Z0-9_]+) (\d+)", text)}
    mix = {k: int(v) for k, v in re.findall(r"#define MI_MIX_([A-Z0-9_]+) (\d+)", text)}
    for col in ("SRC", "N", "ORIGIN", "ORIGIN_PITCH", "ORIGIN_AFFINE", "AFFINE_ON", "GAINS", "CLIP", "PEAK", "FMT", "DST_OFF"):
        assert auto[col] == mix[col]                        # a MI_MIX_* row is the head of a MI_AUTO_* row
    assert (auto["T0"], auto["CHG_OFF"], auto["CHG_N"], auto["COLS"]) == (15, 16, 17, audio.AUTO_COLS)
    assert (auto["CHG_AT"], auto["CHG_RAMP"], auto["CHG_GAINS"], auto["CHG_COLS"]) == (0, 1, 2, audio.AUTO_CHG_COLS)
    assert auto["CHG_COLS"] - auto["CHG_GAINS"] == audio.MIX_CLIP_AT - audio.MIX_GAINS_AT and audio.AUTO_GAIN_MAX == 2.0 ** 64
    sig = _lib.SIGNATURES
    for new, old in (("mi_deliver_mix_auto_pcm", "mi_deliver_mix_pcm"), ("mi_deliver_mix_auto_peaks", "mi_deliver_mix_peaks")):
        res, args = sig[old]                                # the fixed gains' arguments with table_len behind the table
        assert sig[new] == (res, [args[0], _lib.C.c_int64] + args[1:]) and re.search(r"\bint %s\(" % new, text)
