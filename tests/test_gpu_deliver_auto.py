"""The gain-automation kernels alone, through ctypes (demucs_amd/csrc/deliver_mix_auto.hip: mi_deliver_mix_auto_pcm,
mi_deliver_mix_auto_peaks).  The frames are bit for bit what the CPU computes with separate float32 torch operations: per frame the
gains `P + (G - P) * (k.to(float32) / float32(ramp))` of the change in force, then `torch.where(g != 0, g * x, 0)` added in order
onto zeros for the mix and the stems, then `prevent_clip`, `i16_pcm`, channels interleaved.  The clip and PCM steps, `same`, and the
placement of stems and mix on the device are shared with tests/test_gpu_deliver.py and tests/test_gpu_deliver_mix.py."""
import itertools

import numpy as np
import pytest
import torch

from demucs_amd import _lib
from test_gpu_deliver import frames_of, same, stream_ptr
from test_gpu_deliver_mix import AFFINE, Placed, frames_at, noise
from test_gpu_deliver_mix import launch as mix_launch
from test_gpu_deliver_mix import row as mix_row

pytestmark = pytest.mark.gpu
COLS, CHG_COLS = 18, 7                                     # MI_AUTO_COLS, MI_AUTO_CHG_COLS
NS = [1, 3, 4, 5, 1023, 1024, 1025, 2049]                  # around the 4-frame thread and the 1024-frame block, three blocks


def packed(gains):
    g = np.zeros(10, dtype=np.float32)
    g[:len(gains)] = gains
    return g.view(np.int64).tolist()


def table_of(rows):
    """The MI_AUTO_* table of rows [(the 15 MI_MIX_* words, T0, [(at, ramp, gains)])], packed here independently of
    audio.auto_table: the change lists lie behind the rows in REVERSE row order, with a word of padding between two lists."""
    head, tail, at = [], {}, len(rows) * COLS
    for i in reversed(range(len(rows))):
        tail[i] = at + 1
        at += 1 + CHG_COLS * len(rows[i][2])
    for i, (words, t0, changes) in enumerate(rows):
        head += [*words, t0, tail[i], len(changes)]
    body = []
    for i in reversed(range(len(rows))):
        body.append(-1)
        for c_at, ramp, gains in rows[i][2]:
            body += [c_at, ramp, *packed(gains)]
    return head + body


def launch(rows, S, C_, n_peaks, dst, max_n, dst_cap=None, peaks=None, table=None, table_len=None):
    lib = _lib.load()
    words = table_of(rows) if table is None else table
    t = torch.tensor(words, dtype=torch.int64).cuda()
    length = len(words) if table_len is None else table_len
    cap = dst.numel() if dst_cap is None else dst_cap
    if n_peaks:
        _lib.check(lib.mi_deliver_mix_auto_peaks(t.data_ptr(), length, len(rows), max_n, S, C_, peaks.data_ptr(), n_peaks, cap,
                                                 stream_ptr()), "mi_deliver_mix_auto_peaks")
    _lib.check(lib.mi_deliver_mix_auto_pcm(t.data_ptr(), length, len(rows), max_n, S, C_, peaks.data_ptr() if n_peaks else None,
                                           n_peaks, dst.data_ptr(), cap, stream_ptr()), "mi_deliver_mix_auto_pcm")
    torch.cuda.synchronize()


# ---- the CPU restatement ------------------------------------------------------------------------------------------------------
def gains_along(base, changes, t0, n, S):
    """(S + 1, n) float32: every term's gain at track positions t0 .. t0 + n - 1."""
    p = torch.arange(n, dtype=torch.int64) + t0
    P = torch.tensor(list(base[:S + 1]), dtype=torch.float32)
    g = P[:, None].expand(S + 1, n).clone()
    for at, ramp, target in changes:
        G = torch.tensor(list(target[:S + 1]), dtype=torch.float32)
        k = p - at
        new = G[:, None].expand(S + 1, n)
        if ramp > 0:
            t = k.to(torch.float32) / torch.tensor(ramp, dtype=torch.int64).to(torch.float32)
            moving = P[:, None] + (G - P)[:, None] * t[None, :]
            new = torch.where((k >= ramp)[None, :], new, moving)
        g = torch.where((k >= 0)[None, :], new, g)
        P = G
    return g


def auto_value(x, o, g, affine=None):
    """x (S, C, n), o (C, n) as the window stores it, g (S + 1, n): the tensor the user hands to save_audio."""
    org = o
    if affine is not None:                                 # api._restore_on_device: w * s, then + mean
        org = o * torch.tensor(affine[1], dtype=torch.float32) + torch.tensor(affine[0], dtype=torch.float32)
    acc = torch.zeros_like(x[0])
    zero = torch.zeros((), dtype=torch.float32)
    for i, term in enumerate([org] + [x[k] for k in range(x.shape[0])]):
        acc = acc + torch.where(g[i][None, :] != 0, g[i][None, :] * term, zero)
    return acc


def test_the_restatement_of_the_gains():
    g = gains_along([1.0, 0.5], [(10, 4, [0.0, 0.5]), (20, 0, [2.0, 0.0])], 8, 16, 1)
    assert g[0].tolist() == [1.0, 1.0, 1.0, 0.75, 0.5, 0.25] + [0.0] * 6 + [2.0] * 4           # frame `at` still has the old gain
    assert g[1].tolist() == [0.5] * 12 + [0.0] * 4


# ---- schedules ----------------------------------------------------------------------------------------------------------------
def gain_sets(S):
    cyc = [-0.7, 0.0, 1.0, 0.1, -1.0]
    a = [1.0, -1.0] + [0.0] * (S - 1)                       # "minus" of source 0: the base gains
    b = [0.1] + [cyc[k % 5] for k in range(S)]
    c = [0.0] + [0.37] * S
    z = [0.0] * (S + 1)
    return a, b, c, z


def schedules(S):
    """[(name, T0, base gains, changes)] in track positions: every case of the definition."""
    a, b, c, z = gain_sets(S)
    many = [(4950 + 7 * i, (0, 3, 7)[i % 3], (b, z, c, a)[i % 4]) for i in range(300)]            # 300 changes over 2100 frames
    return [
        ("none", 7, a, []),
        ("step at 0", 0, a, [(0, 0, b)]),
        ("step at 2", 5000, a, [(5002, 0, b)]),
        ("steps at the block edge", 5000, a, [(6023, 0, b), (6024, 0, c), (6025, 0, a)]),
        ("a ramp from before T0", 1000, a, [(900, 300, b)]),
        ("a ramp past the row's end", 1000, a, [(1001, 5000, b)]),
        ("ramp 1", 5000, a, [(5001, 1, b), (5003, 1, c), (5004, 0, a), (5004, 1, b)]),
        ("to silence and back", 5000, a, [(5000, 3, z), (5003, 0, z), (5004, 4, b)]),
        ("to silence and back over the block edge", 5000, a, [(5500, 600, z), (6100, 200, b), (6300, 0, z), (6400, 1600, c)]),
        ("300 changes", 5000, c, many),
        ("changes that are all behind", 1 << 40, a, [(5, 10, b), (20, 0, c)]),
        ("changes that are all ahead", 5000, b, [(1 << 40, 10, a)]),
    ]


@pytest.mark.parametrize("S,C_", [(1, 1), (4, 2), (8, 1)])
def test_kernel_equals_the_cpu_restatement(S, C_):
    """Every (n, schedule, clip, format) as one row of ONE launch, the mix's placement, the affine and the stems' alignment cycling
    through the rows; destinations at 0, 4, 8 and 12 mod 16; 0xA5 stays wherever no row writes; a rescaling row's peak is
    abs().max() bit for bit."""
    data = {n: noise(S, C_, n, seed=2000 * S + 100 * C_ + i) for i, n in enumerate(NS)}
    placed = {n: Placed(*data[n]) for n in NS}
    scheds = schedules(S)
    specs, rows, at = [], [], 0
    for i, (n, si, clip, fmt) in enumerate(itertools.product(NS, range(len(scheds)), (0, 1, 2, 3), (0, 1))):
        where = ("tight", "wide", "off1")[i % 3]
        affine = AFFINE if (i // 3) % 2 else None
        shift = 1 if i % 5 == 3 else 0
        at = -(-at // 16) * 16 + 4 * (i % 4)
        org, pitch = placed[n].org[where]
        _, t0, base, changes = scheds[si]
        rows.append((mix_row(placed[n].src[shift], n, org, pitch, affine, base, clip, i, fmt, at), t0, changes))
        specs.append((n, si, affine, clip, fmt, at))
        at += n * C_ * (4 if fmt else 2)
    assert {r[0][14] % 16 for r in rows} == {0, 4, 8, 12} and {r[0][0] % 16 for r in rows} == {0, 4}
    assert {r[0][3] - r[0][1] for r in rows} == {0, 37} and {r[0][5] for r in rows} == {0, 1}
    dst = torch.full((at + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    peaks = torch.full((len(rows) + 2,), -1, dtype=torch.int32, device="cuda")
    launch(rows, S, C_, len(rows), dst, max(NS), dst_cap=at, peaks=peaks)
    host, pk = dst.cpu(), peaks.cpu()
    assert pk[-2:].tolist() == [-1, -1]
    written = torch.zeros(at + 64, dtype=torch.bool)
    values = {}
    for i, (n, si, affine, clip, fmt, off) in enumerate(specs):
        x, o = data[n]
        name, t0, base, changes = scheds[si]
        if (n, si, affine) not in values:
            values[n, si, affine] = auto_value(x, o, gains_along(base, changes, t0, n, S), affine)
        v = values[n, si, affine]
        got = frames_at(host, off, n, C_, fmt)
        assert same(got, frames_of(v, clip, fmt)), (i, n, name, affine, clip, fmt)
        written[off:off + got.numel() * got.element_size()] = True
        if clip == 1:
            assert int(pk[i]) & 0xFFFFFFFF == int(v.abs().max().view(torch.int32)) & 0xFFFFFFFF, (i, n, name)
        else:
            assert int(pk[i]) == 0, i                       # zeroed by the entry, written by rescaling rows only
    assert bool((host[~written] == 0xA5).all())


@pytest.mark.parametrize("S,C_,n", [(4, 2, 2049), (8, 1, 1024), (1, 1, 5)])
def test_changes_that_equal_the_base_gains_give_the_fixed_gain_bytes(S, C_, n):
    """A row whose changes all name its base gains (steps and ramps, at the block edge and inside a thread's frames), and one
    without changes: mi_deliver_mix_pcm's bytes and peaks for the same MI_MIX_* words."""
    x, o = noise(S, C_, n, seed=31 * n + S)
    p = Placed(x, o)
    org, pitch = p.org["wide"]
    _, b, c, _ = gain_sets(S)
    fixed, auto, at = [], [], 0
    for i, (gains, clip, fmt) in enumerate(itertools.product((b, c), (0, 1, 2, 3), (0, 1))):
        words = mix_row(p.src[0], n, org, pitch, AFFINE if i % 2 else None, gains, clip, i, fmt, at)
        same_gains = [(100, 0, gains), (102, 1, gains), (103, 900, gains), (1123, 0, gains), (1124, 2, gains), (1126, 5000, gains)]
        fixed.append(words)
        auto.append((words, 100, same_gains if i % 3 else []))
        at += -(-n * C_ * 4 // 16) * 16
    a = torch.full((at,), 0xA5, dtype=torch.uint8, device="cuda")
    d = torch.full((at,), 0xA5, dtype=torch.uint8, device="cuda")
    pa = torch.zeros(len(fixed), dtype=torch.int32, device="cuda")
    pd = torch.zeros(len(fixed), dtype=torch.int32, device="cuda")
    mix_launch(fixed, S, C_, len(fixed), a, n, peaks=pa)
    launch(auto, S, C_, len(auto), d, n, peaks=pd)
    assert torch.equal(pa.cpu(), pd.cpu())
    assert torch.equal(a.cpu(), d.cpu())
    assert not bool((a.cpu() == 0xA5).all())


def test_a_planted_nan_shows_exactly_where_its_stem_is_heard():
    """A stem that is NaN everywhere, and a NaN mix: the float32 frames are NaN in exactly the frames at which that term's gain is
    not 0 -- through steps, a ramp down to 0 (its first frame of silence is at + ramp) and a ramp up from 0 (frame `at` is still
    silent) -- and equal the restatement on finite data everywhere else."""
    S, C_, n, t0 = 4, 2, 2049, 300
    x, o = noise(S, C_, n, seed=91)
    bad_x, bad_o = x.clone(), o.clone()
    bad_x[2] = float("nan")
    bad_o[:] = float("nan")
    p_stem, p_mix = Placed(bad_x, o), Placed(x, bad_o)
    base = [0.0, 1.0, -0.7, 0.0, 0.1]
    on, off = [0.0, 1.0, -0.7, 0.5, 0.1], [0.0, 1.0, 0.0, 0.0, 0.1]
    mix_on = [0.3, 1.0, 0.0, 0.0, 0.1]
    changes = [(302, 0, on), (310, 5, off), (1320, 9, on), (1400, 0, base), (1401, 0, mix_on), (1403, 640, off), (2300, 3, on)]
    g = gains_along(base, changes, t0, n, S)
    rows = [(mix_row(p_stem.src[0], n, p_stem.org["wide"][0], n + 37, None, base, 0, 0, 1, 0), t0, changes),
            (mix_row(p_mix.src[0], n, p_mix.org["wide"][0], n + 37, None, base, 0, 0, 1, n * C_ * 4), t0, changes)]
    dst = torch.full((2 * n * C_ * 4,), 0xA5, dtype=torch.uint8, device="cuda")
    launch(rows, S, C_, 0, dst, n)
    host = dst.cpu()
    clean = auto_value(x, o, g).t()
    for i, term in ((0, 3), (1, 0)):                        # row 0: stem 2 (term 3) is NaN; row 1: the mix (term 0) is
        got = frames_at(host, i * n * C_ * 4, n, C_, 1)
        heard = g[term] != 0
        assert 0 < int(heard.sum()) < n
        assert torch.equal(torch.isnan(got), heard[:, None].expand(n, C_)), i
        assert torch.equal(got[~heard], clean[~heard]), i
    # the frames the definition names: `at` still old, `at + ramp` the first with the new gains
    heard = (g[3] != 0).tolist()
    assert heard[0:2] == [False, False] and heard[2] and heard[14] and not heard[15]           # 302 on; 310 + 5 = 315 is silent
    assert not heard[1020] and heard[1021]                                                      # 1320 still silent, 1321 is not


def test_every_rule_breaking_row_writes_nothing_and_its_neighbours_are_whole():
    S, C_, n = 4, 2, 64
    x, o = noise(S, C_, n, seed=3)
    p = Placed(x, o)
    org, pitch = p.org["wide"]
    good = [0.1, 1.0, -0.7, 0.0, 1.0]
    other = [0.0, 0.5, 0.0, 0.0, -1.0]
    nan, inf = float("nan"), float("inf")
    cap = 4096
    ok_changes = [(10, 4, other), (30, 0, good)]

    def words(clip=2, peak=0, fmt=0, off=0, gains=good, src=p.src[0], n_=n, org_=org, pitch_=pitch):
        return mix_row(src, n_, org_, pitch_, None, gains, clip, peak, fmt, off)

    bad = [
        (words(fmt=1, off=cap - n * C_ * 4 + 4), 0, ok_changes),                 # the frames leave dst_capacity
        (words(off=-4), 0, ok_changes),
        (words(off=2), 0, ok_changes),                                           # DST_OFF no multiple of 4
        (words(n_=0), 0, ok_changes),
        (words(src=0), 0, ok_changes),
        (words(clip=4), 0, ok_changes),
        (words(fmt=2), 0, ok_changes),
        (words(clip=1, peak=3), 0, ok_changes),                                  # PEAK outside [0, n_peaks)
        (words(gains=[0.1, nan, 1.0, 1.0, 1.0]), 0, ok_changes),                 # a base gain that is not finite
        (words(org_=0), 0, ok_changes),                                          # g_mix != 0 without ORIGIN
        (words(pitch_=n - 1), 0, ok_changes),                                    # ORIGIN_PITCH < N
        (words(gains=other, org_=0), 0, [(1000, 0, good)]),                      # only a change far ahead reads the mix: no ORIGIN
        (words(), 0, [(30, 0, other), (10, 4, good)]),                           # out of order
        (words(), 0, [(10, 4, other), (13, 0, good)]),                           # overlapping: the ramp ends at 14
        (words(), 0, [(10, -1, other)]),                                         # RAMP < 0
        (words(), 0, [(10, 4, other), (20, -3, good), (30, 0, other)]),
        (words(), 0, [(10, 0, [0.0, inf, 0.0, 0.0, 0.0])]),                      # a gain of a change that is not finite
        (words(), 0, [(10, 0, [0.0, nan, 0.0, 0.0, 0.0])]),
        (words(), 0, [(10, 0, [0.0, 2.0 ** 65, 0.0, 0.0, 0.0])]),               # above 2^64
        (words(), 1 << 62, []),                                                  # T0 out of range
        (words(), 0, [(1 << 62, 0, other)]),
        (words(), 0, [(10, 1 << 62, other)]),
        (words(), 0, [(10, 0, other)] * 150 + [(9, 0, good)] + [(10, 0, other)] * 149),        # one of 300 out of order
    ]
    for rows in [bad] + [[r] for r in bad]:
        dst = torch.full((cap + 64,), 0xA5, dtype=torch.uint8, device="cuda")
        peaks = torch.full((3,), -1, dtype=torch.int32, device="cuda")
        launch(rows, S, C_, 3, dst, n, dst_cap=cap, peaks=peaks)
        assert bool((dst.cpu() == 0xA5).all()), rows
        assert peaks.cpu().tolist() == [0, 0, 0]           # zeroed, and no skipped row's peak
    # a change list that reaches outside the table: CHG_OFF / CHG_N negative, past the end, or ending one word too late
    whole = table_of([(words(), 0, ok_changes)])
    for off_, cnt in ((-1, 1), (COLS + 1, -1), (len(whole), 1), (COLS + 1, 3), (COLS + 2, 2), (1 << 40, 1), (COLS + 1, 1 << 40)):
        t = list(whole)
        t[16], t[17] = off_, cnt
        dst = torch.full((cap,), 0xA5, dtype=torch.uint8, device="cuda")
        launch([None], S, C_, 0, dst, n, table=t)
        assert bool((dst.cpu() == 0xA5).all()), (off_, cnt)
    dst = torch.full((cap,), 0xA5, dtype=torch.uint8, device="cuda")
    launch([None], S, C_, 0, dst, n, table=whole, table_len=len(whole) - 1)    # the same list, the table one word shorter
    assert bool((dst.cpu() == 0xA5).all())
    # the rows beside them are written whole: all-zero gains are silence, a gain past n_sources is not read, ORIGIN is not when no
    # gain of the row reads the mix
    zero = [0.0] * 5
    ok = [(words(gains=good + [nan, inf]), 0, [(10, 4, other + [nan]), (30, 0, good)]),
          (words(gains=[0.0] + good[1:], org_=0, pitch_=0, off=256), 0, [(10, 4, other)]),
          (words(gains=zero, off=512), 0, []),
          (words(gains=zero, off=768), 50, [(60, 8, good), (100, 0, zero)])]
    dst = torch.full((cap,), 0xA5, dtype=torch.uint8, device="cuda")
    launch(bad[:12] + ok[:2] + bad[12:] + ok[2:], S, C_, 0, dst, n)
    host = dst.cpu()
    for (w, t0, changes), base in zip(ok, (good, [0.0] + good[1:], zero, zero)):
        want = frames_of(auto_value(x, o, gains_along(base, changes, t0, n, S)), 2, 0)
        assert same(frames_at(host, w[14], n, C_, 0), want), w[14]
    assert bool((host[1024:] == 0xA5).all())


def test_entries_refuse_bad_arguments():
    lib = _lib.load()
    t = torch.zeros(COLS, dtype=torch.int64, device="cuda")
    dst = torch.zeros(64, dtype=torch.uint8, device="cuda")
    assert lib.mi_deliver_mix_auto_pcm(t.data_ptr(), COLS, 1, 4, 9, 2, None, 0, dst.data_ptr(), 64, stream_ptr()) != 0      # nine sources
    assert lib.mi_deliver_mix_auto_pcm(t.data_ptr(), COLS, 1, 4, 4, 2, None, 0, dst.data_ptr() + 2, 60, stream_ptr()) != 0  # alignment
    assert lib.mi_deliver_mix_auto_pcm(t.data_ptr(), COLS - 1, 1, 4, 4, 2, None, 0, dst.data_ptr(), 64, stream_ptr()) != 0  # rows past the table
    assert lib.mi_deliver_mix_auto_pcm(t.data_ptr(), 1 << 31, 1, 4, 4, 2, None, 0, dst.data_ptr(), 64, stream_ptr()) != 0
    assert lib.mi_deliver_mix_auto_peaks(t.data_ptr(), COLS, 1, 4, 4, 2, None, 1, 64, stream_ptr()) != 0
    assert lib.mi_deliver_mix_auto_pcm(t.data_ptr(), COLS, 1, 4, 4, 2, None, 0, dst.data_ptr(), 64, stream_ptr()) == 0      # SRC 0: skipped
    torch.cuda.synchronize()
    assert bool((dst.cpu() == 0).all())
