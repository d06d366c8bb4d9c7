"""The true-peak kernel alone, through ctypes (demucs_amd/csrc/true_peak.hip: mi_true_peak_update), against its exact CPU
restatement: the value of a row is the remix as tests/test_gpu_deliver_mix.py restates it, the chains are
tests/test_true_peak_host.py's numpy-float32 ones.  Bit patterns are compared with ==, for every partition of a track into calls."""
import ctypes as C
from collections import Counter

import numpy as np
import pytest
import torch

from demucs_amd import _lib, audio
from test_gpu_deliver import stream_ptr
from test_gpu_deliver_mix import mix_value
from test_true_peak_host import bits_of, chains, max_bits, restated

pytestmark = pytest.mark.gpu
COLS = 20                                                  # MI_TP_COLS
(SRC, N, ORIGIN, ORIGIN_PITCH, ORIGIN_AFFINE, AFFINE_ON, GAINS, SRC_PITCH, BEFORE, TAIL, HIST_LEN, HIST_RD, HIST_WR, HIST_START,
 HIST_NEXT, PEAK) = (0, 1, 2, 3, 4, 5, 6, 11, 12, 13, 14, 15, 16, 17, 18, 19)
AFFINE = (0.0123, 0.73)
BANK = audio.true_peak_bank(48000)
T = BANK.shape[1]
GUARD = 64
FILL = 0x25A5A5A5                                          # of the history and its guards: a float no chain produces here
NAN = 0x7F800000                                           # patterns above this are NaNs


class Window:
    """The mix on the device as a stream keeps it: rows `pitch` > L floats apart, NaN between them."""

    def __init__(self, o, extra):
        ch, n = o.shape
        self.pitch = n + extra
        self.buf = torch.full((ch, self.pitch), float("nan"), device="cuda")
        self.buf[:, :n] = o.cuda()

    def at(self, a):
        return self.buf.data_ptr() + 4 * a


class Meter:
    """A stream's bookkeeping around mi_true_peak_update, spelled here independently of audio.TruePeakStream.  `gains[i]` are
    output i's gains, `affines[i]` its (mean, s) or None.  The history lies between guard words."""

    def __init__(self, gains, S, ch, bank=BANK, affines=None, history=True):
        self.gains, self.S, self.ch = gains, S, ch
        self.affines = affines or [None] * len(gains)
        self.bank = torch.from_numpy(np.ascontiguousarray(bank, dtype=np.float32)).cuda()
        self.keep = self.bank.shape[1] - 1 if history else 0
        R = len(gains)
        self.body = 2 * R * ch * self.keep
        self.area = torch.empty(GUARD + self.body + GUARD, dtype=torch.int32, device="cuda").fill_(FILL)
        self.peaks = torch.zeros(2 * R, dtype=torch.int32, device="cuda")
        self.side = self.h0 = self.pushed = 0
        self.calls = 0

    @property
    def hist_ptr(self):
        return self.area.data_ptr() + 4 * GUARD

    def rows(self, src, n, origin=0, pitch=0, tail=0, final=False, src_pitch=None):
        """The rows of the next call: `n` samples at device address `src`, the mix's frame 0 at `origin`."""
        end = self.pushed + n
        self.nxt = -1 if final or not self.keep else max(0, end - self.keep)
        per = self.ch * self.keep
        R, rows = len(self.gains), []
        for i, g in enumerate(self.gains):
            packed = np.zeros(10, dtype=np.float32)
            packed[:len(g)] = g
            aff = self.affines[i]
            rows.append([src, n, origin, pitch, int(np.array(aff or (0.0, 0.0), dtype=np.float32).view(np.int64)[0]), int(aff is not None),
                         *packed.view(np.int64).tolist(), n if src_pitch is None else src_pitch, self.pushed, tail, self.keep,
                         (self.side * R + i) * per, ((1 - self.side) * R + i) * per, self.h0, self.nxt, i])
        return rows

    def launch(self, rows, area=None, peaks=None, max_n=None):
        area = self.area if area is None else area
        peaks = self.peaks if peaks is None else peaks
        need = max(1, max(r[N] + r[TAIL] for r in rows)) if max_n is None else max_n
        table = torch.tensor([v for r in rows for v in r], dtype=torch.int64).cuda()
        _lib.check(_lib.load().mi_true_peak_update(
            table.data_ptr(), len(rows), min(need, 1 << 20), self.S, self.ch, self.bank.data_ptr(), self.bank.shape[0], self.bank.shape[1],
            area.data_ptr() + 4 * GUARD if self.body else 0, self.body, peaks.data_ptr(), peaks.numel() // 2, stream_ptr()),
            "mi_true_peak_update")
        torch.cuda.synchronize()
        self.calls += 1

    def push(self, piece, origin=0, pitch=0, tail=0, final=False):
        """`piece`: (S, C, n) on the CPU.  An empty push without a tail is a call whose rows are all skipped."""
        n = piece.shape[2]
        dev = piece.contiguous().cuda()
        self.launch(self.rows(dev.data_ptr() if n else 0, n, origin if n else 0, pitch, tail, final))
        if n and not final:
            self.side, self.h0 = 1 - self.side, self.nxt
        self.pushed += n

    def bits(self):
        assert bool((self.area[:GUARD] == FILL).all()) and bool((self.area[GUARD + self.body:] == FILL).all())
        v = [b & 0xFFFFFFFF for b in self.peaks.cpu().tolist()]
        return list(zip(v[0::2], v[1::2]))


def signal(S, ch, n, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    x = (torch.rand(S, ch, n, generator=g) * 2 - 1) * scale
    o = (torch.rand(ch, n, generator=g) * 2 - 1) * scale
    return x, o


def run(x, o, gains, affines, blocks, last_with_block, bank=BANK):
    """The slots of the input taken in calls of `blocks` samples and then the rest; the final call carries the rest
    (`last_with_block`) or comes after it with no sample.  blocks None: the whole track in one call without a history."""
    S, ch, n = x.shape
    win = Window(o, 36 if n % 4 == 0 else 37)
    tail = bank.shape[1] - 1
    if blocks is None:
        m = Meter(gains, S, ch, bank, affines, history=False)
        m.push(x, win.at(0), win.pitch, tail=tail, final=True)
        assert m.calls == 1
        return m.bits()
    m = Meter(gains, S, ch, bank, affines)
    at = 0
    for b in blocks:
        m.push(x[:, :, at:at + b], win.at(at), win.pitch)
        at += b
    assert at <= n
    if last_with_block:
        m.push(x[:, :, at:], win.at(at), win.pitch, tail=tail, final=True)
    else:
        m.push(x[:, :, at:], win.at(at), win.pitch)
        m.push(x[:, :, n:], tail=tail, final=True)
    assert m.pushed == n
    return m.bits()


def remixes(S):
    """[g_mix, g_0 .. g_{S-1}]: a single stem; a remix with the mix, read through a pitched window with the affine on; another
    remix.  All three mute stem 1, which the tests fill with NaN."""
    return [[0.0] * S + [1.0], [0.5, 1.0, 0.0, -0.7] + [0.25] * (S - 3), [0.0, 0.1, 0.0, -1.0] + [0.0] * (S - 3)], [None, AFFINE, None]


@pytest.mark.parametrize("S,ch", [(4, 2), (6, 1)])
@pytest.mark.parametrize("n", [3 * 1024 + 517, 4 * 1024], ids=["scalar loads, partial workgroup", "16-byte loads"])
def test_every_partition_gives_the_restatements_bits(S, ch, n):
    x, o = signal(S, ch, n, seed=S * n)
    x[1] = float("nan")
    gains, affines = remixes(S)
    want = [restated(mix_value(x, o, g, a).numpy(), BANK) for g, a in zip(gains, affines)]
    assert all(0 < over < NAN and 0 < sample < NAN for over, sample in want)
    whole = run(x, o, gains, affines, None, True)
    print(f"S {S} channels {ch} n {n}: whole {[(hex(a), hex(b)) for a, b in whole]}")
    assert whole == want
    assert run(x, o, gains, affines, [n], False) == want                  # one push, then the tail call
    mixed = [0, 1, 3, T - 1, T, 1024, 1025]
    assert run(x, o, gains, affines, mixed, True) == want
    assert run(x, o, gains, affines, mixed, False) == want
    assert run(x, o, gains, affines, [5, 0, 2, 1, 1, 1, 1030, 7], False) == want       # pushes shorter than the history


def piecewise(v, cuts, bank=BANK, history=True, tail=True):
    """The restatement call by call: (over bits, sample bits) of (C, L) values cut at `cuts`, each call seeing the T - 1 values
    before it (`history`) or zeros, the last one evaluating the T - 1 positions past the end (`tail`) or not."""
    keep = bank.shape[1] - 1
    edges = [0, *cuts, v.shape[1]]
    over = 0
    for i, (a, b) in enumerate(zip(edges[:-1], edges[1:])):
        lead = min(a, keep) if history else 0
        acc = chains(v[:, a - lead:b], bank)[:, :, lead:]
        if not (tail and i == len(edges) - 2):
            acc = acc[:, :, :b - a]
        over = max(over, max_bits(acc))
    return over, max_bits(v)


PLACED_N, PLACED_CUT = 2 * 1024 + 100, 1500
PLACED = [(0, "position 0"), (PLACED_CUT - 3, "the peak within the first T - 1 of a call"),
          (PLACED_CUT + 2, "the sample within the first T - 1 of a call"), (1023, "the last of a workgroup"),
          (1024, "the first of a workgroup"), (PLACED_N - 1, "the last sample: the peak lies in the tail")]


@pytest.mark.parametrize("at,what", PLACED, ids=[w for _, w in PLACED])
def test_placed_maxima(at, what):
    n, cut = PLACED_N, PLACED_CUT
    x, o = signal(1, 2, n, seed=at + 1, scale=0.3)
    x[0, 1, at] = 0.9
    gains = [[0.0, 1.0]]
    v = x[0].numpy()
    acc = chains(v, BANK)
    p, c, where = np.unravel_index(np.abs(acc).argmax(), acc.shape)
    assert c == 1 and where - at in (5, 6) and abs(acc[p, c, where]) > 0.8                 # the peak is the placed sample's
    want = restated(v, BANK)
    assert piecewise(v, [cut]) == want == piecewise(v, [1, 7, cut, cut + 1])
    if at == n - 1:
        assert where >= n and piecewise(v, [cut], tail=False) != want                      # the case bites: the tail is needed
    if cut - T < at < cut + T:
        assert piecewise(v, [cut], history=False) != want                                  # ... the history is
    if at == 0:
        assert piecewise(v, [3], history=False) != want
    if at in (1023, 1024):
        assert where // 1024 == 1                                                          # read by the second workgroup
    assert run(x, o, gains, [None], None, True) == [want]
    assert run(x, o, gains, [None], [cut], True) == [want]
    assert run(x, o, gains, [None], [3, cut - 3], False) == [want]


def test_generic_bank_on_a_ramp():
    bank = np.array([[1, 2, 4], [8, 16, 32]], dtype=np.float32)
    ramp = torch.arange(1, 6, dtype=torch.float32)[None, None]
    o = torch.zeros(1, 5)
    assert run(ramp, o, [[0.0, 1.0]], [None], None, True, bank) == [(bits_of(208.0), bits_of(5.0))]
    assert run(ramp, o, [[0.0, 1.0]], [None], [1, 1, 2], False, bank) == [(bits_of(208.0), bits_of(5.0))]
    # more than one workgroup, two channels, a descending ramp in the second: exact integers throughout
    n = 1024 + 37
    x = torch.stack([torch.arange(1, n + 1, dtype=torch.float32), torch.arange(n, 0, -1, dtype=torch.float32)])[None]
    want = restated(x[0].numpy(), bank)
    assert want == (bits_of(8.0 * (n - 2) + 16.0 * (n - 1) + 32.0 * n), bits_of(float(n)))     # position 2 of the descending ramp
    o = torch.zeros(2, n)
    assert run(x, o, [[0.0, 1.0]], [None], None, True, bank) == [want]
    assert run(x, o, [[0.0, 1.0]], [None], [1000, 30], True, bank) == [want]
    # the largest bank the entry takes, random coefficients
    big = np.random.default_rng(3).standard_normal((audio.TP_MAX_PHASES, audio.TP_MAX_TAPS)).astype(np.float32)
    x, o = signal(2, 2, 1024 + 300, seed=8)
    g = [[0.5, 1.0, -0.25]]
    want = [restated(mix_value(x, o, g[0], AFFINE).numpy(), big)]
    assert run(x, o, g, [AFFINE], None, True, big) == want
    assert run(x, o, g, [AFFINE], [10, 1, 1100], False, big) == want


def test_sample_slot_equals_deliver_mix_peaks():
    S, ch, n = 4, 2, 1024 + 259
    x, o = signal(S, ch, n, seed=21)
    gains, affines = remixes(S)
    got = run(x, o, gains, affines, [700], True)
    dev = x.contiguous().cuda()
    win = Window(o, 37)
    rows = []
    for i, (g, aff) in enumerate(zip(gains, affines)):
        packed = np.zeros(10, dtype=np.float32)
        packed[:len(g)] = g
        rows += [dev.data_ptr(), n, win.at(0), win.pitch, int(np.array(aff or (0.0, 0.0), dtype=np.float32).view(np.int64)[0]),
                 int(aff is not None), *packed.view(np.int64).tolist(), 1, i, 0, 0]       # MI_CLIP_RESCALE, PEAK, MI_DELIVER_I16, DST_OFF
    table = torch.tensor(rows, dtype=torch.int64).cuda()
    peaks = torch.zeros(len(gains), dtype=torch.int32, device="cuda")
    _lib.check(_lib.load().mi_deliver_mix_peaks(table.data_ptr(), len(gains), n, S, ch, peaks.data_ptr(), len(gains), 1 << 40,
                                                stream_ptr()), "mi_deliver_mix_peaks")
    torch.cuda.synchronize()
    assert [sample for _, sample in got] == [b & 0xFFFFFFFF for b in peaks.cpu().tolist()]


def test_nan_and_inf():
    S, ch, n = 4, 2, 1024 + 77
    x, o = signal(S, ch, n, seed=31)
    gains, affines = remixes(S)
    clean = run(x, o, gains, affines, [500], True)
    muted = x.clone()
    muted[1, :, ::3] = float("nan")
    muted[1, :, 1::3] = float("inf")
    assert run(muted, o, gains, affines, [500], True) == clean            # stem 1 has gain 0 in every row: it is not read
    # a NaN in stem 3 reaches rows 0 and 1 (gains 1 and 0.25), not row 2; an Inf likewise (a chain meets it once: Inf, no NaN)
    for bad, is_nan in ((float("nan"), True), (float("-inf"), False)):
        y = x.clone()
        y[3, 1, 600] = bad
        for blocks in (None, [500], [601]):
            got = run(y, o, gains, affines, blocks, True)
            for over, sample in got[:2]:
                assert (over > NAN and sample > NAN) if is_nan else (over == NAN and sample == NAN)
            assert got[2] == clean[2]
    # two Infs of opposite sign within a chain's reach: Inf - Inf is a NaN in the chains, the samples' maximum stays Inf
    y = x.clone()
    y[3, 1, 600], y[3, 1, 601] = float("inf"), float("inf")                # phase 0's taps 6 and 7 have opposite signs
    got = run(y, o, gains, affines, [601], True)
    assert got[0][0] > NAN and got[0][1] == NAN and got[2] == clean[2]
    # the mix is read by row 1 alone
    o2 = o.clone()
    o2[0, 3] = float("nan")
    got = run(x, o2, gains, affines, [2], False)
    assert got[0] == clean[0] and got[2] == clean[2] and got[1][0] > NAN and got[1][1] > NAN


def test_silence_leaves_the_slots_zero():
    x = torch.zeros(2, 2, 1024 + 5)
    x[1, 0, 7] = -0.0
    o = torch.zeros(2, 1024 + 5)
    assert run(x, o, [[0.0, 1.0, 1.0], [1.0, -1.0, 0.0]], [None, None], None, True) == [(0, 0), (0, 0)]
    assert run(x, o, [[0.0, 1.0, 1.0], [1.0, -1.0, 0.0]], [None, None], [1, 1024], False) == [(0, 0), (0, 0)]


def test_every_skip_rule_writes_nothing():
    S, ch, n = 3, 2, 592
    x, o = signal(S, ch, n, seed=5)
    win = Window(o, 37)
    gains = [[0.5, 1.0, 0.0, -0.7]]
    m = Meter(gains, S, ch)
    m.push(x[:, :, :400], win.at(0), win.pitch)
    piece = x[:, :, 400:592].contiguous().cuda()
    good = m.rows(piece.data_ptr(), 192, win.at(400), win.pitch)[0]
    keep = T - 1
    per = ch * keep
    assert (good[BEFORE], good[HIST_START], good[HIST_NEXT], good[HIST_LEN], good[HIST_RD], good[HIST_WR], good[TAIL], good[PEAK]) == \
        (400, 400 - keep, 592 - keep, keep, per, 0, 0, 0) and m.body == 2 * per

    def bad(**cols):
        r = list(good)
        for k, v in cols.items():
            r[globals()[k]] = v
        return r

    def with_gains(g):
        r = list(good)
        packed = np.zeros(10, dtype=np.float32)
        packed[:len(g)] = g
        r[GAINS:GAINS + 5] = packed.view(np.int64).tolist()
        return r

    nan, inf = float("nan"), float("inf")
    rows = [
        bad(SRC=0), bad(N=0), bad(N=-5), bad(N=-5, TAIL=3), bad(N=(1 << 61) + 1, SRC_PITCH=1 << 62, ORIGIN_PITCH=1 << 62),
        with_gains([0.1, nan, 1.0, 1.0]), with_gains([inf, 1.0, 1.0, 1.0]), with_gains([0.0, 1.0, 1.0, -inf]),
        with_gains([0.0, 0.0, -0.0, 0.0]),
        bad(ORIGIN=0), bad(ORIGIN_PITCH=191), bad(SRC_PITCH=191),
        bad(BEFORE=-1), bad(BEFORE=(1 << 61) + 1), bad(HIST_START=-1), bad(HIST_START=401),
        bad(HIST_LEN=keep - 1),                                      # the carried values do not fit a side
        bad(HIST_LEN=-1),
        bad(HIST_RD=-1), bad(HIST_RD=per + 1), bad(HIST_RD=1 << 62), bad(HIST_WR=-4), bad(HIST_WR=per + 1),
        bad(HIST_WR=good[HIST_RD]), bad(HIST_WR=good[HIST_RD] - 1), bad(HIST_RD=good[HIST_WR] + 1),       # the sides overlap
        bad(HIST_NEXT=593), bad(HIST_NEXT=400 - keep - 1), bad(HIST_NEXT=592 - keep - 1),     # outside [hist_start, end]; too much to carry
        bad(HIST_START=395),                                         # five values carried from a start above 0: fewer than T - 1
        bad(TAIL=-1), bad(TAIL=T), bad(TAIL=1 << 40),
        bad(PEAK=-1), bad(PEAK=1), bad(PEAK=1 << 33),
    ]
    area0 = m.area.clone()
    slots0 = torch.ones(2, dtype=torch.int32, device="cuda")           # 1: below every pattern a row that ran would leave

    def untouched(rows):
        area, slots = area0.clone(), slots0.clone()
        m.launch(rows, area=area, peaks=slots)
        return area.equal(area0) and slots.equal(slots0)

    assert untouched(rows)
    for r in rows:
        assert untouched([r]), r
    # the good row beside them is served: slots and history are those of the stream that was not disturbed
    area, slots = area0.clone(), m.peaks.clone()
    m.launch(rows[:14] + [good] + rows[14:], area=area, peaks=slots)
    m.launch([good])
    assert area.equal(m.area) and slots.equal(m.peaks) and not area.equal(area0)
    assert bool((area[:GUARD] == FILL).all()) and bool((area[GUARD + m.body:] == FILL).all())
    m.side, m.h0, m.pushed = 1 - m.side, m.nxt, 592
    m.push(x[:, :, n:], tail=keep, final=True)
    assert m.bits() == [restated(mix_value(x, o, gains[0]).numpy(), BANK)]
    # the carried values are the last T - 1 of the remix
    side = m.area[GUARD:GUARD + m.body].view(torch.float32).view(2, 1, ch, keep)[m.side, 0].cpu()
    assert side.equal(mix_value(x, o, gains[0])[:, n - keep:])
    lib = _lib.load()
    t = torch.zeros(COLS, dtype=torch.int64, device="cuda")
    tail = (m.hist_ptr, m.body, m.peaks.data_ptr(), 1, stream_ptr())
    bank = m.bank.data_ptr()
    assert lib.mi_true_peak_update(t.data_ptr(), 1, 1, 9, 2, bank, 4, 12, *tail) != 0           # nine sources
    assert lib.mi_true_peak_update(t.data_ptr(), 0, 1, 3, 2, bank, 4, 12, *tail) != 0
    assert lib.mi_true_peak_update(t.data_ptr(), 1, 0, 3, 2, bank, 4, 12, *tail) != 0
    assert lib.mi_true_peak_update(t.data_ptr(), 1, 1, 3, 2, bank, 9, 12, *tail) != 0
    assert lib.mi_true_peak_update(t.data_ptr(), 1, 1, 3, 2, bank, 4, 33, *tail) != 0
    assert lib.mi_true_peak_update(t.data_ptr(), 1, 1, 3, 2, 0, 4, 12, *tail) != 0
    assert lib.mi_true_peak_update(t.data_ptr(), 1, 1, 3, 2, bank, 4, 12, *tail) == 0           # an all-zero row: skipped
    torch.cuda.synchronize()


def test_stream_is_one_call_a_push(monkeypatch):
    S, ch, n = 4, 2, 3000
    x, o = signal(S, ch, n, seed=41)
    names = ["a", "b", "c", "d"]
    mix = {"k": {"mix": 0.5, "a": 1.0, "c": -0.7, "d": 0.25}, "d": {"d": 1.0}}
    dev, org = x.cuda(), o.cuda()
    lib = _lib.load()
    counts = Counter()
    for name in _lib.SIGNATURES:
        real = getattr(lib, name)

        def wrapped(*args, _real=real, _name=name):
            counts[_name] += 1
            return _real(*args)

        monkeypatch.setattr(lib, name, wrapped)
    st = audio.TruePeakStream(names, ch, 44100, mix, device="cuda")
    sizes, at = [], 0
    for b in (1, 700, 0, 5, 1024, 1270):
        counts.clear()
        st.push(dev[:, :, at:at + b], org[:, at:at + b])                  # spans of the whole track, read in place
        assert counts == (Counter({"mi_true_peak_update": 1}) if b else Counter())
        at += b
        sizes.append(st.device_bytes)
    assert at == n and len(set(sizes)) == 1 and sizes[0] == 2 * 2 * ch * (T - 1) * 4 + 2 * 2 * 4 + BANK.nbytes
    counts.clear()
    got = st.finish()
    assert counts == Counter({"mi_true_peak_update": 1})
    counts.clear()
    whole = audio.true_peak(org, dict(zip(names, dev)), mix, 44100)
    assert counts == Counter({"mi_true_peak_update": 1})
    monkeypatch.undo()
    assert got == whole and got.length == n and got.names == ("k", "d")
    want = [restated(mix_value(x, o, g).numpy(), BANK) for _, g in audio.mix_gains(mix, names)]
    assert list(zip(got.bits, got.sample_bits)) == want
