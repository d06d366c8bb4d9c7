"""The loudness kernels alone, through ctypes (demucs_amd/csrc/loudness.hip: mi_loudness_update), and `audio.loudness` /
`audio.LoudnessStream` on top of them, against ITU-R BS.1770-4 restated in float64 with plain loops: the value of a row is the CPU
restatement of the remix that tests/test_gpu_deliver_mix.py uses, the recursion runs sample by sample in Python floats.  Energies
are compared within relative 1e-9 of that oracle, and as bytes wherever two partitions of one input are compared."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from demucs_amd import _lib, audio
from test_gpu_deliver import stream_ptr
from test_gpu_deliver_mix import mix_value

pytestmark = pytest.mark.gpu
COLS = 22                                                  # MI_LOUD_COLS
(SRC, N, ORIGIN, ORIGIN_PITCH, ORIGIN_AFFINE, AFFINE_ON, GAINS, SRC_PITCH, BEFORE, HIST_LEN, HIST_RD, HIST_WR, HIST_START, HIST_NEXT,
 E_OFF, E_PITCH, WORK_OFF, WORK_PITCH) = (0, 1, 2, 3, 4, 5, 6, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21)
AFFINE = (0.0123, 0.73)
HOP, WARM = 64, 256
REL = 1e-9


def kfilter(x, coef):
    """Both biquads over a 1-D signal from zero state, sequentially, in Python floats (float64)."""
    y = [float(v) for v in x]
    for (b0, b1, b2), (_, a1, a2) in np.asarray(coef).tolist():
        x1 = x2 = y1 = y2 = 0.0
        out = []
        for v in y:
            w = b0 * v + b1 * x1 + b2 * x2 - a1 * y1 - a2 * y2
            x2, x1, y2, y1 = x1, v, y1, w
            out.append(w)
        y = out
    return np.array(y, dtype=np.float64)


def whole_energies(v, coef, hop):
    """e[c][h] of (C, L) values from ONE recursion over the whole signal."""
    hn = v.shape[1] // hop
    y = np.stack([kfilter(row, coef) for row in np.asarray(v, dtype=np.float64)])
    return (y[:, :hn * hop].reshape(v.shape[0], hn, hop) ** 2).sum(-1)


def window_energies(v, coef, hop, warm):
    """e[c][h] as the kernel defines it: each sub-block's own recursion from zero state, `warm` samples before it."""
    v = np.asarray(v, dtype=np.float64)
    hn = v.shape[1] // hop
    e = np.zeros((v.shape[0], hn))
    for c in range(v.shape[0]):
        for h in range(hn):
            y = kfilter(v[c, max(0, h * hop - warm):(h + 1) * hop], coef)
            e[c, h] = (y[-hop:] ** 2).sum()
    return e


def lufs(e, hop):
    """Integrated loudness and the blocks' loudness from (C, Hn) energies: the formulas, with loops."""
    p = [sum(e[c][j + i] for c in range(len(e)) for i in range(4)) / (4 * hop) for j in range(len(e[0]) - 3)]
    l = [-0.691 + 10 * math.log10(v) if v > 0 else -math.inf for v in p]
    first = [v for v, w in zip(p, l) if w > -70]
    if not first:
        return -math.inf, l
    gate = -0.691 + 10 * math.log10(sum(first) / len(first)) - 10
    second = [v for v, w in zip(p, l) if w > -70 and w > gate]
    return -0.691 + 10 * math.log10(sum(second) / len(second)), l


def close(got, want):
    """Same NaNs, and the rest within relative REL."""
    got, want = np.asarray(got), np.asarray(want)
    nan = np.isnan(want)
    return got.shape == want.shape and bool((np.isnan(got) == nan).all()) and \
        bool((np.abs(got[~nan] - want[~nan]) <= REL * np.abs(want[~nan])).all())


def worst(got, want):
    ok = ~np.isnan(want)
    return float((np.abs(got[ok] - want[ok]) / np.abs(want[ok])).max())


class Window:
    """The mix on the device as a stream keeps it: rows `pitch` > L floats apart, NaN between them."""

    def __init__(self, o, extra=37):
        ch, n = o.shape
        self.pitch = n + extra
        self.buf = torch.full((ch, self.pitch), float("nan"), device="cuda")
        self.buf[:, :n] = o.cuda()

    def at(self, a):
        return self.buf.data_ptr() + 4 * a


class Meter:
    """A stream's bookkeeping around mi_loudness_update, spelled here independently of audio.LoudnessStream.  `gains[i]` are
    output i's nine gains, `affines[i]` its (mean, s) or None."""

    def __init__(self, gains, S, ch, hop, warm, coef, blocks, affines=None):
        self.gains, self.S, self.ch, self.hop, self.warm = gains, S, ch, hop, warm
        self.affines = affines or [None] * len(gains)
        k = np.asarray(coef, dtype=np.float64)
        self.coef = (C.c_double * 10)(*k[0, 0], *k[0, 1, 1:], *k[1, 0], *k[1, 1, 1:])
        self.hist_len = warm + hop
        R = len(gains)
        self.hist = torch.full((2, R, ch, self.hist_len), float("nan"), device="cuda")
        self.energies = torch.full((R, ch, blocks), -1.0, dtype=torch.float64, device="cuda")
        self.side = self.h0 = self.pushed = 0

    def rows(self, src, n, origin=0, pitch=0):
        """The rows of the next push of `n` samples at device address `src` (contiguous), the mix's frame 0 at `origin`."""
        end = self.pushed + n
        self.nxt = max(0, end // self.hop * self.hop - self.warm)
        kept = self.pushed - self.h0
        per = self.ch * self.hist_len
        R, rows = len(self.gains), []
        for i, g in enumerate(self.gains):
            packed = np.zeros(10, dtype=np.float32)
            packed[:len(g)] = g
            aff = self.affines[i]
            rows.append([src, n, origin, pitch, int(np.array(aff or (0.0, 0.0), dtype=np.float32).view(np.int64)[0]), int(aff is not None),
                         *packed.view(np.int64).tolist(), n, self.pushed, self.hist_len, (self.side * R + i) * per,
                         ((1 - self.side) * R + i) * per, self.h0, self.nxt, i * self.ch * self.energies.shape[2],
                         self.energies.shape[2], i * self.ch * (kept + n), kept + n])
        return rows

    def launch(self, rows, hist=None, energies=None, work=None, hop=None, warm=None):
        hist = self.hist if hist is None else hist
        energies = self.energies if energies is None else energies
        need = max(1, max(r[BEFORE] - r[HIST_START] + r[N] for r in rows))
        if work is None:
            work = torch.full((len(rows) * self.ch * need,), float("nan"), device="cuda")
        blocks = max(0, max((r[BEFORE] + r[N]) // self.hop - r[BEFORE] // self.hop for r in rows))
        table = torch.tensor([v for r in rows for v in r], dtype=torch.int64).cuda()
        _lib.check(_lib.load().mi_loudness_update(
            table.data_ptr(), len(rows), min(need, 1 << 16), min(blocks, 1 << 12), self.S, self.ch, self.coef,
            self.hop if hop is None else hop, self.warm if warm is None else warm, hist.data_ptr(), hist.numel(), energies.data_ptr(),
            energies.numel(), work.data_ptr(), work.numel(), stream_ptr()), "mi_loudness_update")
        torch.cuda.synchronize()

    def push(self, piece, origin=0, pitch=0):
        """`piece`: (S, C, n) on the CPU; an empty push is a call whose rows are all skipped."""
        n = piece.shape[2]
        dev = piece.contiguous().cuda()
        self.launch(self.rows(dev.data_ptr() if n else 0, n, origin, pitch))
        if n:
            self.side, self.h0, self.pushed = 1 - self.side, self.nxt, self.pushed + n

    def result(self):
        return self.energies[:, :, :self.pushed // self.hop].cpu().numpy()


def signal(S, ch, n, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(S, ch, n, generator=g) * 2 - 1
    o = torch.rand(ch, n, generator=g) * 2 - 1
    return x, o


def run(x, o, gains, affines, cuts, coef, hop=HOP, warm=WARM):
    """The energies of the input pushed in the pieces `cuts` name, the mix read from one window by address and pitch."""
    S, ch, n = x.shape
    win = Window(o)
    m = Meter(gains, S, ch, hop, warm, coef, n // hop + 2, affines)
    edges = [0, *cuts, n]
    for a, b in zip(edges[:-1], edges[1:]):
        m.push(x[:, :, a:b], win.at(a), win.pitch)
    tail = m.energies[:, :, n // hop:].cpu()
    assert bool((tail == -1.0).all())                       # nothing past the complete sub-blocks
    return m.result()


# [g_mix, g_0, g_1, g_2]: a single stem; a remix with the mix, read through a pitched window with the affine on; another remix.
# All three mute stem 1, which the tests fill with NaN
REMIXES = [[0.0, 0.0, 0.0, 1.0], [0.5, 1.0, 0.0, -0.7], [0.0, 0.1, 0.0, -1.0]]
AFFINES = [None, AFFINE, None]


def test_index_logic_at_hop_64_warm_256():
    coef = audio.k_weighting(48000)
    S, ch, n = 3, 2, 64 * 9 + 17
    x, o = signal(S, ch, n, seed=1)
    x[1] = float("nan")
    gains, affines = REMIXES, AFFINES
    got = run(x, o, gains, affines, (), coef)
    assert got.shape == (3, ch, 9)
    for i, g in enumerate(gains):
        v = mix_value(x, o, g, affines[i]).numpy()
        assert np.isfinite(v).all()
        want = window_energies(v, coef, HOP, WARM)
        assert close(got[i], want), (i, worst(got[i], want))
    assert np.isfinite(got).all()                           # the muted NaN reached nothing
    # an unmuted NaN sample: exactly the sub-blocks whose window [h * hop - warm, (h + 1) * hop) holds it
    x2, _ = signal(S, ch, n, seed=2)
    at = 3 * HOP + 5
    x2[0, 1, at] = float("nan")
    o2 = o.clone()
    o2[0, 8 * HOP + 1] = float("nan")
    g2 = [[0.0, 1.0, 0.0, 0.5], [1.0, 0.0, 0.0, 1.0], [0.0, 0.0, 1.0, 1.0]]
    got = run(x2, o2, g2, [None] * 3, (), coef)
    holds = np.array([h * HOP - WARM <= at < (h + 1) * HOP for h in range(9)])
    assert holds.tolist() == [False] * 3 + [True] * 5 + [False]
    assert (np.isnan(got[0, 1]) == holds).all() and np.isfinite(got[0, 0]).all()
    assert np.isnan(got[1, 0]).tolist() == [False] * 8 + [True] and np.isfinite(got[1, 1]).all()
    assert np.isfinite(got[2]).all()
    for i, g in enumerate(g2):
        want = window_energies(mix_value(x2, o2, g).numpy(), coef, HOP, WARM)
        assert close(got[i], want), i


def test_every_partition_gives_the_same_bytes():
    coef = audio.k_weighting(48000)
    S, ch, n = 3, 2, 64 * 9 + 17
    x, o = signal(S, ch, n, seed=3)
    x[1] = float("nan")
    whole = run(x, o, REMIXES[:2], AFFINES[:2], (), coef)
    assert np.isfinite(whole).all()
    for cuts in [(1,), (HOP - 1,), (HOP,), (HOP + 1,), (WARM + HOP + 3,), (100, 100), (0, 1, 1, 63, 64, 129, 400, n),
                 (WARM + HOP - 1, WARM + HOP, 2 * WARM)]:
        assert run(x, o, REMIXES[:2], AFFINES[:2], cuts, coef).tobytes() == whole.tobytes(), cuts
    n = 3 * HOP + 5
    xs, os_ = x[:, :, :n].contiguous(), o[:, :n].contiguous()
    short = run(xs, os_, REMIXES[:2], AFFINES[:2], (), coef)
    assert short.tobytes() == whole[:, :, :3].tobytes()     # a prefix of the track: a sub-block looks at nothing after itself
    for cut in range(1, n):
        assert run(xs, os_, REMIXES[:2], AFFINES[:2], (cut,), coef).tobytes() == short.tobytes(), cut


def hard_input(fs, ch, n, seed):
    """DC, a 20 Hz sine and noise: what is left of a short warm-up shows in the high-pass."""
    g = torch.Generator().manual_seed(seed)
    t = torch.arange(n, dtype=torch.float64) / fs
    x = 0.9 + 0.3 * torch.sin(2 * math.pi * 20.0 * t)[None] + 0.1 * torch.randn(ch, n, generator=g, dtype=torch.float64)
    return x.float()


@pytest.mark.parametrize("fs,ch", [(44100, 2), (48000, 2), (44100, 1)])
def test_real_parameters_against_the_whole_signal_recursion(fs, ch):
    """Measured on an MI355X: the largest relative error over the sub-blocks is 1.4e-13 at 44.1 kHz stereo, 2.2e-13 at 48 kHz
    stereo and 1.7e-13 at 44.1 kHz mono."""
    H, W = fs // 10, audio.loudness_warmup(fs)
    assert W == 16384
    n = W + 4 * H + 123
    x = hard_input(fs, ch, n, seed=fs + ch)
    want = whole_energies(x.numpy(), audio.k_weighting(fs), H)
    dev = x.cuda()
    whole = audio.loudness(None, {"a": dev}, samplerate=fs)
    assert whole.names == ("a",) and whole.length == n and whole.energies.shape == (1, ch, n // H)
    print(f"fs {fs} channels {ch}: worst relative error {worst(whole.energies[0], want):.3e}")
    assert close(whole.energies[0], want), worst(whole.energies[0], want)
    st = audio.LoudnessStream(["a"], ch, fs, device="cuda")
    cut = W + H + 1
    st.push(dev[None, :, :cut].contiguous())
    st.push(dev[None, :, cut:].contiguous())
    assert st.device_bytes == 2 * ch * (W + H) * 4 + st._energies.numel() * 8
    split = st.finish()
    assert split.energies.tobytes() == whole.energies.tobytes() and split == whole


def test_conformance_sines():
    """EBU Tech 3341 case 1: a stereo 1 kHz sine at -23 dBFS reads -23.0 +- 0.1 LUFS; at -33 dBFS, -33.0."""
    fs, n = 48000, 3 * 48000
    t = torch.arange(n, dtype=torch.float64) / fs
    for level in (-23.0, -33.0):
        x = (10 ** (level / 20) * torch.sin(2 * math.pi * 1000.0 * t)).float()
        e1 = whole_energies(x[None].numpy(), audio.k_weighting(fs), fs // 10)
        want, _ = lufs(np.concatenate([e1, e1]), fs // 10)
        got = audio.loudness(None, {"tone": torch.stack([x, x]).cuda()}, samplerate=fs).integrated("tone")
        print(f"{level} dBFS: device {got:.6f} LUFS, oracle {want:.6f} LUFS")
        assert abs(want - level) <= 0.1 and abs(got - level) <= 0.1
        assert abs(got - want) <= 1e-6


def test_every_skip_rule_writes_nothing():
    coef = audio.k_weighting(48000)
    S, ch, n = 3, 2, 64 * 9 + 17
    x, o = signal(S, ch, n, seed=5)
    win = Window(o)
    gains = [[0.5, 1.0, 0.0, -0.7]]
    m = Meter(gains, S, ch, HOP, WARM, coef, 12)
    m.push(x[:, :, :400], win.at(0), win.pitch)
    piece = x[:, :, 400:592].contiguous().cuda()
    good = m.rows(piece.data_ptr(), 192, win.at(400), win.pitch)[0]
    assert (good[BEFORE], good[HIST_START], good[HIST_NEXT], good[HIST_LEN], good[E_PITCH]) == (400, 128, 320, 320, 12)
    per = ch * 320

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
        bad(SRC=0), bad(N=0), bad(N=-5), bad(N=(1 << 61) + 1, SRC_PITCH=1 << 62, ORIGIN_PITCH=1 << 62),
        with_gains([0.1, nan, 1.0, 1.0]), with_gains([inf, 1.0, 1.0, 1.0]), with_gains([0.0, 1.0, 1.0, -inf]),
        with_gains([0.0, 0.0, -0.0, 0.0]),
        bad(ORIGIN=0), bad(ORIGIN_PITCH=191), bad(SRC_PITCH=191),
        bad(BEFORE=-1), bad(BEFORE=(1 << 61) + 1), bad(HIST_START=-1), bad(HIST_START=401),
        bad(HIST_LEN=271),                                           # the carried values do not fit a side
        bad(HIST_LEN=-1),
        bad(HIST_RD=-1), bad(HIST_RD=2 * per + 1), bad(HIST_WR=-4), bad(HIST_WR=2 * per - per + 1),
        bad(HIST_WR=good[HIST_RD]), bad(HIST_WR=good[HIST_RD] + per - 1), bad(HIST_RD=good[HIST_WR] + 1),     # the sides overlap
        bad(HIST_NEXT=593), bad(HIST_NEXT=127), bad(HIST_NEXT=271),      # outside [hist_start, end]; more than a side to carry
        bad(HIST_START=200),                                         # the first window begins at 128, before what is carried
        bad(E_OFF=-1), bad(E_OFF=1), bad(E_PITCH=8), bad(E_PITCH=13), bad(E_OFF=1 << 62),
        bad(WORK_OFF=-1), bad(WORK_OFF=1), bad(WORK_PITCH=463), bad(WORK_PITCH=465), bad(WORK_OFF=1 << 62),
    ]
    hist0, e0 = m.hist.clone(), m.energies.clone()

    def untouched(rows, **kw):
        hist, energies = hist0.clone(), e0.clone()
        work = torch.full((ch * 464,), float("nan"), device="cuda")
        work.view(torch.int32).fill_(0x25A5A5A5)
        m.launch(rows, hist=hist, energies=energies, work=work, **kw)
        return (hist.view(torch.int32).equal(hist0.view(torch.int32)) and energies.view(torch.int64).equal(e0.view(torch.int64))
                and bool((work.view(torch.int32) == 0x25A5A5A5).all()))

    assert untouched(rows)
    for r in rows:
        assert untouched([r]), r
    for kw in (dict(hop=0), dict(hop=-64), dict(warm=-1)):
        assert untouched([good], **kw), kw
    # the good row beside them is taken: its three sub-blocks and its history are those of the stream that was not disturbed
    hist, energies = hist0.clone(), e0.clone()
    work = torch.full((2 * ch * 464,), float("nan"), device="cuda")
    second = list(good)
    second[WORK_OFF] = ch * 464
    second[E_OFF] = 1 << 40                                  # this one leaves the energies
    m.launch(rows[:12] + [good, second], hist=hist, energies=energies, work=work[:ch * 464 * 2])
    m.launch([good])
    m.side, m.h0, m.pushed = 1 - m.side, m.nxt, 592
    assert energies.view(torch.int64).equal(m.energies.view(torch.int64)) and hist.view(torch.int32).equal(m.hist.view(torch.int32))
    got = m.result()[0]
    want = window_energies(mix_value(x[:, :, :592], o[:, :592], gains[0]).numpy(), coef, HOP, WARM)
    assert got.shape == (ch, 9) and close(got, want)
    lib = _lib.load()
    t = torch.zeros(COLS, dtype=torch.int64, device="cuda")
    args = (m.coef, 64, 256, m.hist.data_ptr(), m.hist.numel(), m.energies.data_ptr(), m.energies.numel(), work.data_ptr(), work.numel(),
            stream_ptr())
    assert lib.mi_loudness_update(t.data_ptr(), 1, 1, 1, 9, 2, *args) != 0          # nine sources
    assert lib.mi_loudness_update(t.data_ptr(), 0, 1, 1, 3, 2, *args) != 0
    assert lib.mi_loudness_update(t.data_ptr(), 1, 0, 1, 3, 2, *args) != 0
    assert lib.mi_loudness_update(t.data_ptr(), 1, 1, 1, 3, 2, *args) == 0          # an all-zero row: skipped
    torch.cuda.synchronize()


def test_normalised_gains_deliver_the_target():
    fs, ch, n = 48000, 2, 48000 + 321
    g = torch.Generator().manual_seed(9)
    t = torch.arange(n, dtype=torch.float32) / fs
    names = ["drums", "bass", "vocals"]
    stems = {k: (a * torch.sin(2 * math.pi * f * t)[None] * torch.tensor([[1.0], [0.8]]) + 0.02 * torch.randn(ch, n, generator=g))
             for k, a, f in zip(names, (0.2, 0.3, 0.1), (180.0, 60.0, 900.0))}
    origin = sum(stems.values()) + 0.001 * torch.randn(ch, n, generator=g)
    mix = {"karaoke": {"mix": 1.0, "vocals": -1.0}, "practice": {"drums": 2.0, "bass": 0.5, "vocals": 0.5}}
    dev = {k: v.cuda() for k, v in stems.items()}
    measured = audio.loudness(origin.cuda(), dev, mix, samplerate=fs)
    x = torch.stack(list(stems.values()))
    coef = audio.k_weighting(fs)
    for i, (name, gains) in enumerate(audio.mix_gains(mix, names)):
        e = whole_energies(mix_value(x, origin, gains).numpy(), coef, fs // 10)
        want, blocks = lufs(e, fs // 10)
        assert close(measured.energies[i], e) and abs(measured.integrated(name) - want) <= 1e-6
        assert min(blocks) > -70 and min(blocks) + (-14.0 - want) > -70       # every block over the absolute gate, before and after
    norm = measured.normalised(-14.0)
    frames = audio.deliver_mix(origin.cuda(), dev, norm, clip=None, fmt="f32")
    again = audio.loudness(None, {k: v.t().contiguous() for k, v in frames.items()}, samplerate=fs)
    for name in mix:
        print(f"{name}: {measured.integrated(name):.4f} LUFS -> {again.integrated(name):.6f} LUFS")
        assert abs(again.integrated(name) + 14.0) <= 1e-3
    assert measured.mix == audio.mix_identity(audio.mix_gains(mix, names)) and measured.sources == tuple(names)
