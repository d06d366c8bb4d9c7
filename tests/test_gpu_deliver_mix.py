"""The remix delivery kernels alone, through ctypes (demucs_amd/csrc/deliver_mix.hip: mi_deliver_mix_pcm, mi_deliver_mix_peaks,
mi_deliver_mix_peaks_update): the frames are bit for bit what a user of the reference computes on the CPU as
`save_audio(sum(g * x for ...))` -- `torch.tensor(g, dtype=float32) * x` added in order onto zeros, a term with gain 0 left out,
then `prevent_clip`, `i16_pcm`, channels interleaved.  Every comparison is `torch.equal` / bytes; tanh, whose libm differs, goes
through the project's own `audio.prevent_clip`, as in tests/test_gpu_deliver.py, whose restatement of the clip and PCM steps this
file shares."""
import itertools

import numpy as np
import pytest
import torch

from demucs_amd import _lib
from test_gpu_deliver import frames_of, same, stream_ptr

pytestmark = pytest.mark.gpu
COLS = 15                                                  # MI_MIX_COLS
NS = [1, 3, 4, 5, 1023, 1024, 1025]                        # around the 4-frame thread and the 1024-frame block
PLANTED = [1.0, -1.0, 0.99, -0.99, 0.99997, 0.5, -0.5, -0.0, 1e-6]
AFFINE = (0.0123, 0.73)                                    # (mean, s) of a Separator stream


def row(src, n, origin, pitch, affine, gains, clip, peak, fmt, off):
    """One MI_MIX_* row, packed here independently of audio.mix_rows."""
    g = np.zeros(10, dtype=np.float32)
    g[:len(gains)] = gains
    aff = int(np.array(affine or (0.0, 0.0), dtype=np.float32).view(np.int64)[0])
    return [src, n, origin, pitch, aff, int(affine is not None), *g.view(np.int64).tolist(), clip, peak, fmt, off]


def mix_value(x, o, gains, affine=None):
    """The tensor the user hands to save_audio: x (S, C, n), o (C, n) as the window stores it, on the CPU."""
    acc = torch.zeros_like(x[0])
    if gains[0] != 0:
        org = o
        if affine is not None:                             # api._restore_on_device: w * s, then + mean
            org = o * torch.tensor(affine[1], dtype=torch.float32) + torch.tensor(affine[0], dtype=torch.float32)
        acc = acc + torch.tensor(gains[0], dtype=torch.float32) * org
    for k in range(x.shape[0]):
        if gains[1 + k] != 0:
            acc = acc + torch.tensor(gains[1 + k], dtype=torch.float32) * x[k]
    return acc


def gain_sets(S):
    """[g_mix, g_0 .. g_{S-1}]: 0, +-1, 0.1 and -0.7 in every role."""
    cyc = [-0.7, 0.0, 1.0, 0.1, -1.0]
    return [
        [1.0, -1.0] + [0.0] * (S - 1),                      # "minus" of source 0
        [0.0] + [0.0 if k == S - 1 else 1.0 for k in range(S)] if S > 1 else [0.0, 1.0],      # "add" without the last
        [0.1] + [cyc[k % 5] for k in range(S)],
        [0.0] + [0.0] * (S - 1) + [0.1],                    # one quiet source alone
        [-1.0] + [-0.7] * S,
    ]


def noise(S, C_, n, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(S, C_, n, generator=g) * 3 - 1.5
    o = torch.rand(C_, n, generator=g) * 3 - 1.5
    k = min(n, len(PLANTED))
    x[:, :, :k] = torch.tensor(PLANTED[:k])
    o[:, n - k:] = torch.tensor(PLANTED[:k])
    return x, o


class Placed:
    """Stems and mix on the device in every placement the kernel distinguishes: stems at a 16-byte boundary or one float behind
    it; the mix with pitch n, with pitch n + 37, or one float behind a boundary.  What lies between the mix's rows is NaN: a
    read past N would show."""

    def __init__(self, x, o):
        S, C_, n = x.shape
        self.keep, self.src, self.org = [], {}, {}
        for shift in (0, 1):
            bx = torch.zeros(x.numel() + 4, device="cuda")
            bx[shift:shift + x.numel()] = x.reshape(-1).cuda()
            self.keep.append(bx)
            self.src[shift] = bx.data_ptr() + 4 * shift
        for name, pitch, shift in (("tight", n, 0), ("wide", n + 37, 0), ("off1", n, 1)):
            bo = torch.full((C_ * pitch + 4,), float("nan"), device="cuda")
            bo[shift:shift + C_ * pitch].view(C_, pitch)[:, :n] = o.cuda()
            self.keep.append(bo)
            self.org[name] = (bo.data_ptr() + 4 * shift, pitch)


def launch(rows, S, C_, n_peaks, dst, max_n, dst_cap=None, peaks=None):
    lib = _lib.load()
    table = torch.tensor([v for r in rows for v in r], dtype=torch.int64).cuda()
    cap = dst.numel() if dst_cap is None else dst_cap
    if n_peaks:
        _lib.check(lib.mi_deliver_mix_peaks(table.data_ptr(), len(rows), max_n, S, C_, peaks.data_ptr(), n_peaks, cap, stream_ptr()),
                   "mi_deliver_mix_peaks")
    _lib.check(lib.mi_deliver_mix_pcm(table.data_ptr(), len(rows), max_n, S, C_, peaks.data_ptr() if n_peaks else None, n_peaks,
                                      dst.data_ptr(), cap, stream_ptr()), "mi_deliver_mix_pcm")
    torch.cuda.synchronize()


def frames_at(host, off, n, C_, fmt):
    nbytes = n * C_ * (4 if fmt else 2)
    return host[off:off + nbytes].clone().view(torch.float32 if fmt else torch.int16).view(n, C_)


@pytest.mark.parametrize("S,C_", [(1, 1), (1, 2), (4, 1), (4, 2), (8, 1), (8, 2)])
def test_kernel_equals_the_cpu_restatement(S, C_):
    """Every (n, gains, clip, format) as one row of ONE launch, the mix's placement, the affine and the stems' alignment cycling
    through the rows; destinations at 16-byte boundaries and at 4, 8 and 12 mod 16; 0xA5 stays wherever no row writes."""
    data = {n: noise(S, C_, n, seed=1000 * S + 100 * C_ + i) for i, n in enumerate(NS)}
    placed = {n: Placed(*data[n]) for n in NS}
    sets = gain_sets(S)
    specs, rows, at = [], [], 0
    for i, (n, gi, clip, fmt) in enumerate(itertools.product(NS, range(len(sets)), (0, 1, 2, 3), (0, 1))):
        where = ("tight", "wide", "off1")[i % 3]
        affine = AFFINE if (i // 3) % 2 else None
        shift = 1 if i % 5 == 3 else 0
        at = -(-at // 16) * 16 + 4 * (i % 4)
        org, pitch = placed[n].org[where]
        rows.append(row(placed[n].src[shift], n, org, pitch, affine, sets[gi], clip, i, fmt, at))
        specs.append((n, gi, affine, clip, fmt, at))
        at += n * C_ * (4 if fmt else 2)
    assert {r[14] % 16 for r in rows} == {0, 4, 8, 12} and {r[0] % 16 for r in rows} == {0, 4}
    assert {(r[2] % 16, r[3] - r[1], r[5]) for r in rows} == set(itertools.product((0, 4), (0, 37), (0, 1))) - {(4, 37, 0), (4, 37, 1)}
    dst = torch.full((at + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    peaks = torch.full((len(rows) + 2,), -1, dtype=torch.int32, device="cuda")
    launch(rows, S, C_, len(rows), dst, max(NS), dst_cap=at, peaks=peaks)
    host, pk = dst.cpu(), peaks.cpu()
    assert pk[-2:].tolist() == [-1, -1]
    written = torch.zeros(at + 64, dtype=torch.bool)
    values = {}
    for i, (n, gi, affine, clip, fmt, off) in enumerate(specs):
        x, o = data[n]
        if (n, gi, affine) not in values:
            values[n, gi, affine] = mix_value(x, o, sets[gi], affine)
        v = values[n, gi, affine]
        want = frames_of(v, clip, fmt)
        got = frames_at(host, off, n, C_, fmt)
        assert same(got, want), (i, n, sets[gi], affine, clip, fmt)
        written[off:off + got.numel() * got.element_size()] = True
        if clip == 1:
            assert int(pk[i]) & 0xFFFFFFFF == int(v.abs().max().view(torch.int32)) & 0xFFFFFFFF, (i, n)
        else:
            assert int(pk[i]) == 0, i                       # zeroed by the entry, written by rescaling rows only
    assert bool((host[~written] == 0xA5).all())


def test_a_muted_term_is_not_read_and_a_used_one_propagates():
    """NaN and Inf planted in zero-gain stems and in a zero-gain mix leave the output finite and equal to the restatement; with a
    gain they propagate: NaN frames (int16: 0), a NaN peak."""
    S, C_, n = 4, 2, 1025
    x, o = noise(S, C_, n, seed=77)
    x[2, 1, 777] = float("nan")
    x[3, 0, 5] = float("inf")
    o_bad = o.clone()
    o_bad[0, 1000] = float("nan")
    pl, pl_bad = Placed(x, o), Placed(x, o_bad)
    muted = [0.1, 1.0, -0.7, 0.0, 0.0]
    no_mix = [0.0, 1.0, -0.7, 0.0, 0.0]
    used = [0.0, 1.0, 0.0, 0.1, -0.7]
    specs = [(pl, muted, o), (pl_bad, no_mix, o_bad), (pl, used, o)]
    for clip, fmt in itertools.product((0, 1, 2, 3), (0, 1)):
        rows, at = [], 0
        for i, (p, gains, _) in enumerate(specs):
            org, pitch = p.org["wide"]
            rows.append(row(p.src[0], n, org, pitch, None, gains, clip, i, fmt, at))
            at += -(-n * C_ * 4 // 16) * 16
        dst = torch.full((at,), 0xA5, dtype=torch.uint8, device="cuda")
        peaks = torch.zeros(3, dtype=torch.int32, device="cuda")
        launch(rows, S, C_, 3, dst, n, peaks=peaks)
        host = dst.cpu()
        for i, (p, gains, org) in enumerate(specs):
            v = mix_value(x, org, gains)
            got = frames_at(host, rows[i][14], n, C_, fmt)
            if i < 2:
                assert bool(torch.isfinite(v).all())
                if fmt:
                    assert bool(torch.isfinite(got).all())
                assert same(got, frames_of(v, clip, fmt)), (i, clip, fmt)
            elif clip != 1:                                 # rescale: the NaN peak makes every frame NaN, below
                assert not bool(torch.isfinite(v).all())
                assert same(got, frames_of(v, clip, fmt)), (i, clip, fmt)
                if fmt:
                    assert bool(torch.isnan(got[777, 1])) and bool(torch.isinf(got[5, 0])) == (clip in (0,))
            else:
                assert same(got, frames_of(v, clip, fmt)), (i, clip, fmt)
                bits = int(peaks.cpu()[2]) & 0xFFFFFFFF
                assert bits > 0x7F800000                    # a NaN pattern: orders above +inf


def test_every_skip_rule_writes_nothing():
    S, C_, n = 4, 2, 64
    x, o = noise(S, C_, n, seed=3)
    p = Placed(x, o)
    org, pitch = p.org["wide"]
    good = [0.1, 1.0, -0.7, 0.0, 1.0]
    nan, inf = float("nan"), float("inf")
    cap = 4096
    bad = [
        row(p.src[0], n, org, pitch, None, good, 2, 0, 1, cap - n * C_ * 4 + 4),       # the frames leave dst_capacity
        row(p.src[0], n, org, pitch, None, good, 2, 0, 0, -4),
        row(p.src[0], n, org, pitch, None, good, 2, 0, 0, 2),                          # DST_OFF no multiple of 4
        row(p.src[0], 0, org, pitch, None, good, 2, 0, 0, 0),
        row(p.src[0], -5, org, pitch, None, good, 2, 0, 0, 0),
        row(0, n, org, pitch, None, good, 2, 0, 0, 0),
        row(p.src[0], n, org, pitch, None, good, 4, 0, 0, 0),
        row(p.src[0], n, org, pitch, None, good, -1, 0, 0, 0),
        row(p.src[0], n, org, pitch, None, good, 2, 0, 2, 0),                          # "i24" is no format here either
        row(p.src[0], n, org, pitch, None, good, 2, 0, -1, 0),
        row(p.src[0], n, org, pitch, None, good, 1, 3, 0, 0),                          # PEAK outside [0, n_peaks)
        row(p.src[0], n, org, pitch, None, good, 1, -1, 0, 0),
        row(p.src[0], n, org, pitch, None, [0.1, nan, 1.0, 1.0, 1.0], 2, 0, 0, 0),
        row(p.src[0], n, org, pitch, None, [inf, 1.0, 1.0, 1.0, 1.0], 2, 0, 0, 0),
        row(p.src[0], n, org, pitch, None, [0.0, 1.0, 1.0, 1.0, -inf], 2, 0, 0, 0),
        row(p.src[0], n, org, pitch, None, [0.0, 0.0, -0.0, 0.0, 0.0], 2, 0, 0, 0),  # every gain 0
        row(p.src[0], n, 0, pitch, None, good, 2, 0, 0, 0),                            # g_mix != 0 without ORIGIN
        row(p.src[0], n, org, n - 1, None, good, 2, 0, 0, 0),                          # ORIGIN_PITCH < N
        row(p.src[0], n, org, 0, AFFINE, good, 1, 0, 0, 0),
    ]
    for rows in [bad] + [[r] for r in bad]:
        dst = torch.full((cap + 64,), 0xA5, dtype=torch.uint8, device="cuda")
        peaks = torch.full((3,), -1, dtype=torch.int32, device="cuda")
        launch(rows, S, C_, 3, dst, n, dst_cap=cap, peaks=peaks)
        assert bool((dst.cpu() == 0xA5).all()), rows
        assert peaks.cpu().tolist() == [0, 0, 0]           # zeroed, and no skipped row's peak
        lib = _lib.load()
        table = torch.tensor([v for r in rows for v in r], dtype=torch.int64).cuda()
        peaks.fill_(7)
        _lib.check(lib.mi_deliver_mix_peaks_update(table.data_ptr(), len(rows), n, S, C_, peaks.data_ptr(), 3, stream_ptr()),
                   "mi_deliver_mix_peaks_update")
        torch.cuda.synchronize()
        assert peaks.cpu().tolist() == [7, 7, 7]           # none of them rescales and is whole
    # the update reads no destination: a rescaling row is not skipped for its FMT or DST_OFF
    free = row(p.src[0], n, org, pitch, None, good, 1, 1, 2, 2)
    table = torch.tensor(free, dtype=torch.int64).cuda()
    peaks = torch.zeros(3, dtype=torch.int32, device="cuda")
    _lib.check(_lib.load().mi_deliver_mix_peaks_update(table.data_ptr(), 1, n, S, C_, peaks.data_ptr(), 3, stream_ptr()),
               "mi_deliver_mix_peaks_update")
    assert peaks.cpu().tolist() == [0, int(mix_value(x, o, good).abs().max().view(torch.int32)), 0]
    # the rows beside them are written: a gain past n_sources is not read, ORIGIN and its pitch are not when g_mix is 0
    ok = [row(p.src[0], n, org, pitch, None, good + [nan, inf], 2, 0, 0, 0),
          row(p.src[0], n, 0, 0, None, [0.0] + good[1:], 2, 0, 0, 256)]
    dst = torch.full((cap,), 0xA5, dtype=torch.uint8, device="cuda")
    launch(bad + ok, S, C_, 0, dst, n, peaks=None)
    host = dst.cpu()
    assert same(frames_at(host, 0, n, C_, 0), frames_of(mix_value(x, o, good), 2, 0))
    assert same(frames_at(host, 256, n, C_, 0), frames_of(mix_value(x, o, [0.0] + good[1:]), 2, 0))
    assert bool((host[512:] == 0xA5).all())


def deliver_rows_launch(rows, S, C_, n_peaks, dst, max_n, peaks):
    """mi_deliver_peaks + mi_deliver_pcm on MI_DELIVER_* rows: the entries the equivalences are stated against."""
    lib = _lib.load()
    table = torch.tensor([v for r in rows for v in r], dtype=torch.int64).cuda()
    _lib.check(lib.mi_deliver_peaks(table.data_ptr(), len(rows), max_n, S, C_, peaks.data_ptr(), n_peaks, dst.numel(), stream_ptr()),
               "mi_deliver_peaks")
    _lib.check(lib.mi_deliver_pcm(table.data_ptr(), len(rows), max_n, S, C_, peaks.data_ptr(), n_peaks, dst.data_ptr(), dst.numel(),
                                  stream_ptr()), "mi_deliver_pcm")
    torch.cuda.synchronize()


@pytest.mark.parametrize("S,C_,n", [(4, 2, 1025), (4, 2, 1024), (8, 1, 1023), (2, 2, 5)])
def test_add_and_minus_equivalent_gains_equal_the_delivery_rows(S, C_, n):
    """Gains of 1 on every stem but SEL: MI_DELIVER_ADD's bits.  {mix: 1, SEL: -1}: MI_DELIVER_MINUS's int16 bytes, its float32
    frames as numbers (only a -0.0 may come out as +0.0).  The peaks of both entries agree bit for bit."""
    x, o = noise(S, C_, n, seed=11 * n + S)
    p = Placed(x, o)
    org, _ = p.org["tight"]
    old, new, at = [], [], 0
    for i, (kind, sel, clip, fmt) in enumerate(itertools.product((1, 2), (0, S - 1), (0, 1, 2, 3), (0, 1))):
        if kind == 1:
            gains = [0.0] + [0.0 if k == sel else 1.0 for k in range(S)]
        else:
            gains = [1.0] + [-1.0 if k == sel else 0.0 for k in range(S)]
        old.append([p.src[0], org if kind == 2 else 0, n, kind, sel, clip, i, fmt, at])
        new.append(row(p.src[0], n, org, n, None, gains, clip, i, fmt, at))
        at += -(-n * C_ * 4 // 16) * 16
    a = torch.full((at,), 0xA5, dtype=torch.uint8, device="cuda")
    b = torch.full((at,), 0xA5, dtype=torch.uint8, device="cuda")
    pa = torch.zeros(len(old), dtype=torch.int32, device="cuda")
    pb = torch.zeros(len(old), dtype=torch.int32, device="cuda")
    deliver_rows_launch(old, S, C_, len(old), a, n, pa)
    launch(new, S, C_, len(new), b, n, peaks=pb)
    assert torch.equal(pa.cpu(), pb.cpu())
    ha, hb = a.cpu(), b.cpu()
    for r_old, r_new in zip(old, new):
        kind, fmt, off = r_old[3], r_old[7], r_old[8]
        nbytes = n * C_ * (4 if fmt else 2)
        if kind == 1 or fmt == 0:
            assert torch.equal(ha[off:off + nbytes], hb[off:off + nbytes]), r_old
        else:
            assert torch.equal(frames_at(ha, off, n, C_, 1), frames_at(hb, off, n, C_, 1)), r_old
    gaps = torch.ones(at, dtype=torch.bool)
    for r_old in old:
        gaps[r_old[8]:r_old[8] + n * C_ * (4 if r_old[7] else 2)] = False
    assert bool((hb[gaps] == 0xA5).all())


@pytest.mark.parametrize("cuts", [(), (1,), (4, 8), (1023, 1024), (5, 300, 301, 1500)])
def test_peaks_update_over_any_partition_equals_the_one_shot(cuts):
    """mi_deliver_mix_peaks_update on consecutive pieces of a track, the mix read from ONE window by address and pitch as a stream
    does, leaves mi_deliver_mix_peaks' bits on the whole."""
    S, C_, n = 4, 2, 2050
    x, o = noise(S, C_, n, seed=5)
    p = Placed(x, o)
    org, pitch = p.org["wide"]
    sets = gain_sets(S)
    lib = _lib.load()
    whole = [row(p.src[0], n, org, pitch, AFFINE if i % 2 else None, g, 1, i, 0, 0) for i, g in enumerate(sets)]
    want = torch.full((len(sets),), -1, dtype=torch.int32, device="cuda")
    table = torch.tensor([v for r in whole for v in r], dtype=torch.int64).cuda()
    _lib.check(lib.mi_deliver_mix_peaks(table.data_ptr(), len(whole), n, S, C_, want.data_ptr(), len(sets), 1 << 30, stream_ptr()),
               "mi_deliver_mix_peaks")
    got = torch.zeros(len(sets), dtype=torch.int32, device="cuda")
    edges = [0, *cuts, n]
    for a, b in zip(edges[:-1], edges[1:]):
        piece = x[:, :, a:b].contiguous().cuda()
        rows = [row(piece.data_ptr(), b - a, org + 4 * a, pitch, AFFINE if i % 2 else None, g, 1, i, 0, 0) for i, g in enumerate(sets)]
        t = torch.tensor([v for r in rows for v in r], dtype=torch.int64).cuda()
        _lib.check(lib.mi_deliver_mix_peaks_update(t.data_ptr(), len(rows), b - a, S, C_, got.data_ptr(), len(sets), stream_ptr()),
                   "mi_deliver_mix_peaks_update")
    torch.cuda.synchronize()
    assert torch.equal(got.cpu(), want.cpu())
    for i, g in enumerate(sets):
        v = mix_value(x, o, g, AFFINE if i % 2 else None)
        assert int(want.cpu()[i]) & 0xFFFFFFFF == int(v.abs().max().view(torch.int32)) & 0xFFFFFFFF


def test_entries_refuse_bad_arguments():
    lib = _lib.load()
    t = torch.zeros(COLS, dtype=torch.int64, device="cuda")
    dst = torch.zeros(64, dtype=torch.uint8, device="cuda")
    pk = torch.zeros(1, dtype=torch.int32, device="cuda")
    assert lib.mi_deliver_mix_pcm(t.data_ptr(), 1, 4, 9, 2, None, 0, dst.data_ptr(), 64, stream_ptr()) != 0       # nine sources
    assert lib.mi_deliver_mix_pcm(t.data_ptr(), 1, 4, 4, 2, None, 0, dst.data_ptr() + 2, 60, stream_ptr()) != 0   # alignment
    assert lib.mi_deliver_mix_peaks(t.data_ptr(), 1, 4, 4, 2, None, 1, 64, stream_ptr()) != 0
    assert lib.mi_deliver_mix_peaks_update(t.data_ptr(), 0, 4, 4, 2, pk.data_ptr(), 1, stream_ptr()) != 0
    assert lib.mi_deliver_mix_pcm(t.data_ptr(), 1, 4, 4, 2, None, 0, dst.data_ptr(), 64, stream_ptr()) == 0       # an all-zero row: skipped
    torch.cuda.synchronize()
    assert bool((dst.cpu() == 0).all())
