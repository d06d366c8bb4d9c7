"""The device side of the segment scheduler (ola.hip), each entry alone through the C ABI, bit for bit: `mi_segments_gather`,
`mi_ola_accumulate`, `mi_ola_finish` and their packed twins.  Every streaming, packed and group test compares these kernels with
one another (or takes them as its reference), and one kernel body serves the one-track and the packed entry: this file is where that
body meets something that is not itself.

Reference.  The kernels are specified as sequences of separately rounded float32 operations in a fixed order (ascending item index;
product and sum rounded separately; one correctly rounded division), so the plain numpy float32 restatements below are exact: the
comparison is on bit patterns, NaN positions equal, with no tolerance.  The restatements are vectorised over positions and loop
over items.

    gather       seg[b, c, i] = track[c, start_b + i] inside [0, len), else 0
    accumulate   for i ascending, for p in [max(span_lo, 0), min(span_hi, acc_len)) with j = p - off_i, 0 <= j < min(len_i, W),
                 0 <= trim_i + j < valid:   acc[row, p] = f32(acc[row, p] + f32(w[j] * out[i, row, trim_i + j]))
    finish       sw[q] = 0; for i ascending, j = acc_off0 + q - off_i, 0 <= j < min(len_i, W): sw[q] = f32(sw[q] + w[j]);
                 acc[row, q] = f32(acc[row, q] / sw[q])      (an uncovered position becomes +-inf or NaN on both sides)

Order.  At two-fold overlap from a zero accumulator the float32 sum is commutative and any order passes.  The order cases use
four-fold overlap (ramp 64, stride 16) and assert on the inputs themselves that the descending-order reference differs from the
ascending one at 1000 or more of the 3300 positions of each row: a kernel that ignored the order could not pass them.

Buffers the kernels write lie between guard floats that must keep their value; a gather output starts as a sentinel, so an
unwritten element shows.  Magnitudes stay within [1e-6, 1e3]: nothing here reaches the denormal range."""
import ctypes as C

import numpy as np
import pytest
import torch

from demucs_amd import _lib
from demucs_amd import packed as K

pytestmark = pytest.mark.gpu
F = np.float32
GUARD, GUARD_VALUE, SENTINEL = 64, -12345.0, 54321.0
RAMP, STRIDE = 64, 16                                   # four-fold overlap
ORDER_MIN = 1000                                        # positions (of 3300) at which the summation order must matter


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return _lib.load()


def stream():
    return C.c_void_p(_lib.current_stream_ptr())


def bits(a):
    """The bit patterns of a float32 array, every NaN as one pattern (a NaN's payload is not compared)."""
    a = np.ascontiguousarray(a, dtype=F)
    return np.where(np.isnan(a), np.uint32(0x7FC00000), a.view(np.uint32))


def assert_same_bits(got, want, what=""):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    a, b = bits(got), bits(want)
    bad = np.argwhere(a != b)
    if len(bad):
        eg = [(tuple(int(v) for v in i), float(got[tuple(i)]), float(want[tuple(i)]), hex(int(a[tuple(i)])), hex(int(b[tuple(i)])))
              for i in bad[:4]]
        raise AssertionError(f"{what}: {len(bad)} of {got.size} differ, e.g. (index, got, want, got bits, want bits) {eg}")


class Guarded:
    """A float32 device buffer holding `values` between guard floats."""

    def __init__(self, values):
        values = np.ascontiguousarray(values, dtype=F)
        self.shape, self.n = values.shape, values.size
        self.buf = torch.full((self.n + 2 * GUARD,), GUARD_VALUE, device="cuda")
        self.buf[GUARD:GUARD + self.n] = torch.from_numpy(values.reshape(-1)).cuda()

    def ptr(self):
        return self.buf.data_ptr() + 4 * GUARD

    def read(self):
        """The values on the host, after checking that the guards are as they were."""
        host = self.buf.cpu().numpy()
        guards = np.concatenate([host[:GUARD], host[GUARD + self.n:]])
        assert np.array_equal(guards.view(np.uint32), np.full(2 * GUARD, GUARD_VALUE, F).view(np.uint32)), "written outside the buffer"
        return host[GUARD:GUARD + self.n].reshape(self.shape).copy()


def i64(values):
    return torch.tensor(np.asarray(values, dtype=np.int64).reshape(-1)).cuda()


def i32(values):
    return torch.tensor(np.asarray(values, dtype=np.int32).reshape(-1)).cuda()


def ramp(rng, n=RAMP):
    """Random weights away from powers of two: every product and every partial sum rounds."""
    return rng.uniform(0.1, 1.1, n).astype(F)


# ---- references ------------------------------------------------------------------------------------------------------------------
def ref_gather(track, starts, valid):
    """track (channels, len) -> (B, channels, valid)"""
    n = track.shape[1]
    idx = np.asarray(starts, dtype=np.int64)[:, None] + np.arange(valid, dtype=np.int64)[None, :]
    inside = (idx >= 0) & (idx < n)
    picked = track[:, np.clip(idx, 0, n - 1)].transpose(1, 0, 2)
    return np.where(inside[:, None, :], picked, F(0)).astype(F)


def ref_accumulate(acc, mo, w, items, valid, span_lo, span_hi, order):
    """acc (rows, acc_len); mo (B, rows, valid); items[i] = (off, len, trim); `order`: the item indices in summation order."""
    acc = acc.astype(F).copy()
    lo, hi = max(span_lo, 0), min(span_hi, acc.shape[1])
    for i in order:
        off, ln, trim = items[i]
        j = np.arange(max(0, min(ln, len(w))), dtype=np.int64)
        p, src = off + j, trim + j
        ok = (p >= lo) & (p < hi) & (src >= 0) & (src < valid)
        j, p, src = j[ok], p[ok], src[ok]
        prod = (w[j][None, :] * mo[i][:, src]).astype(F)
        acc[:, p] = (acc[:, p] + prod).astype(F)
    return acc


def ref_sum_weight(acc_len, acc_off0, segs, w, order):
    sw = np.zeros(acc_len, F)
    for i in order:
        off, ln = segs[i]
        j = np.arange(max(0, min(ln, len(w))), dtype=np.int64)
        q = off + j - acc_off0
        ok = (q >= 0) & (q < acc_len)
        sw[q[ok]] = (sw[q[ok]] + w[j[ok]]).astype(F)
    return sw


def ref_finish(acc, acc_off0, segs, w):
    sw = ref_sum_weight(acc.shape[1], acc_off0, segs, w, range(len(segs)))
    with np.errstate(all="ignore"):
        return (acc.astype(F) / sw[None, :]).astype(F)


def order_matters(asc, desc):
    """Positions per row at which the two summation orders gave other bits."""
    return (bits(asc) != bits(desc)).reshape(-1, asc.shape[-1]).sum(axis=1)


# ---- 1. gather -------------------------------------------------------------------------------------------------------------------
TRACK_LEN = 1000


def gather_starts(valid, n):
    """Wholly before the track, ending at 0, straddling 0, at 0, inside, ending at len, straddling len, at len, past len."""
    return [-valid - 5, -valid, -(valid // 2), 0, 100, n - valid, n - (valid + 1) // 2, n, n + 37]


@pytest.mark.parametrize("valid", [1, 255, 256, 257, 700])
@pytest.mark.parametrize("channels", [1, 2])
def test_segments_gather(lib, channels, valid):
    rng = np.random.default_rng(100 * channels + valid)
    track = rng.standard_normal((channels, TRACK_LEN)).astype(F)
    starts = gather_starts(valid, TRACK_LEN)
    want = ref_gather(track, starts, valid)
    src, seg = Guarded(track), Guarded(np.full(want.shape, SENTINEL, F))
    t_starts = i64(starts)
    _lib.check(lib.mi_segments_gather(src.ptr(), TRACK_LEN, channels, t_starts.data_ptr(), len(starts), valid, seg.ptr(), seg.n,
                                      stream()), "mi_segments_gather")
    assert_same_bits(seg.read(), want, "gather")


@pytest.mark.parametrize("valid", [1, 255, 256, 257, 700])
@pytest.mark.parametrize("channels", [1, 2])
def test_segments_gather_packed(lib, channels, valid):
    """Two tracks of different lengths in one buffer, their items interleaved, and one item whose track would leave the declared
    capacity: the kernel's `ok` rule drops its reads, so it comes out as zeros."""
    rng = np.random.default_rng(200 * channels + valid)
    lens = [TRACK_LEN, 613]
    tracks = [rng.standard_normal((channels, n)).astype(F) for n in lens]
    src_offs = [0, channels * lens[0]]
    cap = channels * sum(lens)
    per_track = [gather_starts(valid, n) for n in lens]
    items, want = [], []
    for k in range(len(per_track[0])):
        for t in (0, 1):
            items.append([src_offs[t], lens[t], per_track[t][k], 0, 0, 0, 0, 0])
            want.append(ref_gather(tracks[t], [per_track[t][k]], valid)[0])
    # a window inside a "track" that ends one sample per channel behind the capacity: SRC_OFF + channels * SRC_LEN > capacity
    items.insert(5, [src_offs[1], lens[1] + 1, 10, 0, 0, 0, 0, 0])
    want.insert(5, np.zeros((channels, valid), F))
    assert items[5][0] + channels * items[5][1] > cap
    want = np.stack(want)
    src = Guarded(np.concatenate([t.reshape(-1) for t in tracks]))
    seg = Guarded(np.full(want.shape, SENTINEL, F))
    t_items = i64(items)
    assert len(items[0]) == K.ITEM_COLS
    _lib.check(lib.mi_segments_gather_packed(src.ptr(), cap, channels, t_items.data_ptr(), len(items), valid, seg.ptr(), seg.n,
                                             stream()), "mi_segments_gather_packed")
    assert_same_bits(seg.read(), want, "gather_packed")


# ---- 2. accumulate ---------------------------------------------------------------------------------------------------------------
def run_accumulate(lib, acc0, mo, w, items, valid, span_lo, span_hi):
    """mi_ola_accumulate on guarded copies; returns (status, acc)."""
    rows, acc_len = acc0.shape
    acc, d_mo, d_w = Guarded(acc0), Guarded(mo), Guarded(w)
    offs, lens, trims = i64([x[0] for x in items]), i32([x[1] for x in items]), i32([x[2] for x in items])
    status = lib.mi_ola_accumulate(acc.ptr(), acc_len, rows, d_mo.ptr(), valid, d_mo.n, offs.data_ptr(), lens.data_ptr(),
                                   trims.data_ptr(), len(items), span_lo, span_hi, d_w.ptr(), len(w), stream())
    torch.cuda.synchronize()
    return status, acc.read()


def fourfold(n, first=-20, length=RAMP, trim=7):
    return [(first + STRIDE * i, length, trim) for i in range(n)]


def order_inputs(rows, zero_start=False, B=200, acc_len=3300, valid=100, seed=0):
    rng = np.random.default_rng(seed)
    acc0 = np.zeros((rows, acc_len), F) if zero_start else rng.standard_normal((rows, acc_len)).astype(F)
    mo = rng.standard_normal((B, rows, valid)).astype(F)
    return acc0, mo, ramp(rng), fourfold(B), valid


@pytest.mark.parametrize("rows", [1, 3])
def test_ola_accumulate_sums_in_ascending_item_order(lib, rows):
    """200 items at four-fold overlap onto a random accumulator: every 1024-position tile collects hits whose item indices cross
    the 64, 128 and 192 wave boundaries of the kernel's compaction."""
    acc0, mo, w, items, valid = order_inputs(rows)
    want = ref_accumulate(acc0, mo, w, items, valid, 0, acc0.shape[1], range(len(items)))
    desc = ref_accumulate(acc0, mo, w, items, valid, 0, acc0.shape[1], reversed(range(len(items))))
    differ = order_matters(want, desc)
    print("positions per row at which the order matters:", differ.tolist())
    assert (differ >= ORDER_MIN).all(), f"the inputs do not tell the orders apart: {differ.tolist()}"
    status, got = run_accumulate(lib, acc0, mo, w, items, valid, 0, acc0.shape[1])
    assert status == 0, lib.mi_last_error()
    assert_same_bits(got, want, "accumulate, ascending order")


@pytest.mark.parametrize("rows", [1, 3])
def test_ola_accumulate_from_a_zero_accumulator(lib, rows):
    """The first call of a track."""
    acc0, mo, w, items, valid = order_inputs(rows, zero_start=True, seed=1)
    want = ref_accumulate(acc0, mo, w, items, valid, 0, acc0.shape[1], range(len(items)))
    status, got = run_accumulate(lib, acc0, mo, w, items, valid, 0, acc0.shape[1])
    assert status == 0, lib.mi_last_error()
    assert_same_bits(got, want, "accumulate from zero")


@pytest.mark.parametrize("rows", [1, 3])
def test_ola_accumulate_keeps_what_lies_outside_the_span(lib, rows):
    span_lo, span_hi = 1500, 2600                       # neither a multiple of 1024; the items cover both sides
    acc0, mo, w, items, valid = order_inputs(rows, seed=2)
    assert min(x[0] for x in items) < span_lo - RAMP and max(x[0] + x[1] for x in items) > span_hi + RAMP
    want = ref_accumulate(acc0, mo, w, items, valid, span_lo, span_hi, range(len(items)))
    status, got = run_accumulate(lib, acc0, mo, w, items, valid, span_lo, span_hi)
    assert status == 0, lib.mi_last_error()
    outside = np.r_[0:span_lo, span_hi:acc0.shape[1]]
    assert_same_bits(got[:, outside], acc0[:, outside], "outside the span")
    assert not np.array_equal(bits(want[:, span_lo:span_hi]), bits(acc0[:, span_lo:span_hi]))
    assert_same_bits(got, want, "accumulate on a span")


EDGE_ACC_LEN, EDGE_VALID = 3000, 100
EDGE_ITEMS = [                                          # (off, len, trim), in no offset order: the order is the item index
    (-30, 64, 0),                                       # off < 0
    (EDGE_ACC_LEN - 20, 64, 0),                         # off + len > acc_len
    (200, 90, 0),                                       # len > weight_len: clamps at the ramp
    (400, 64, 50),                                      # trim + len > valid: clamps at the model output
    (600, 1, 3),                                        # one sample
    (700, 64, -5),                                      # trim < 0: the first five samples have no source
    (960, 64, 7),                                       # last position 1023
    (961, 64, 7),                                       # last position 1024
    (1024, 64, 7),                                      # off at the tile boundary
    (1023, 1, 0),                                       # p = 1023 alone
    (1024, 1, 1),                                       # p = 1024 alone
    (2047 - 63, 64, 30),                                # last position 2047
    (2048, 64, 36),                                     # off at the second boundary, trim + len == valid
    (210, 64, 11),                                      # a second and a third layer over item 2
    (215, 64, 13),
    (EDGE_ACC_LEN - 1, 64, 2),                          # only its first sample lies inside
    (EDGE_ACC_LEN, 64, 2),                              # wholly behind the accumulator
    (-64, 64, 2),                                       # wholly before it
]


@pytest.mark.parametrize("rows", [1, 3])
def test_ola_accumulate_clamps_at_every_extent(lib, rows):
    rng = np.random.default_rng(3)
    acc0 = rng.standard_normal((rows, EDGE_ACC_LEN)).astype(F)
    mo = rng.standard_normal((len(EDGE_ITEMS), rows, EDGE_VALID)).astype(F)
    w = ramp(rng)
    want = ref_accumulate(acc0, mo, w, EDGE_ITEMS, EDGE_VALID, 0, EDGE_ACC_LEN, range(len(EDGE_ITEMS)))
    status, got = run_accumulate(lib, acc0, mo, w, EDGE_ITEMS, EDGE_VALID, 0, EDGE_ACC_LEN)
    assert status == 0, lib.mi_last_error()
    untouched = np.ones(EDGE_ACC_LEN, bool)
    for off, ln, _ in EDGE_ITEMS:
        untouched[max(off, 0):max(off + ln, 0)] = False
    assert_same_bits(got[:, untouched], acc0[:, untouched], "positions no item covers")
    assert_same_bits(got, want, "accumulate at the edges")


def test_ola_accumulate_takes_256_items_and_refuses_257(lib):
    rows, valid, acc_len = 2, 100, 4200
    rng = np.random.default_rng(4)
    acc0 = rng.standard_normal((rows, acc_len)).astype(F)
    mo = rng.standard_normal((257, rows, valid)).astype(F)
    w = ramp(rng)
    items = fourfold(257)
    want = ref_accumulate(acc0, mo[:256], w, items[:256], valid, 0, acc_len, range(256))
    status, got = run_accumulate(lib, acc0, mo[:256], w, items[:256], valid, 0, acc_len)
    assert status == 0, lib.mi_last_error()
    assert_same_bits(got, want, "accumulate, 256 items")
    status, got = run_accumulate(lib, acc0, mo, w, items, valid, 0, acc_len)
    assert status != 0
    assert_same_bits(got, acc0, "a refused call")


@pytest.mark.parametrize("rows", [1, 3])
def test_ola_accumulate_packed(lib, rows):
    """Two accumulators of different lengths in one buffer; in the one item table their items alternate, so every tile's item range
    holds foreign items that the accumulator filter must skip, and each accumulator has a ramp of its own length."""
    rng = np.random.default_rng(5)
    valid, n_each = 100, 120
    acc_lens = [2100, 1777]                             # the second one ends before its last items do
    acc_base = [0, rows * acc_lens[0]]
    w_off, w_len = [0, RAMP], [RAMP, 48]                # the second ramp is shorter than the items: they clamp at it
    weights = ramp(rng, sum(w_len))
    mine = [fourfold(n_each), fourfold(n_each, first=-7, trim=20)]
    table, owner = [], []
    for k in range(n_each):
        for a in (0, 1):
            off, ln, trim = mine[a][k]
            table.append([0, 0, 0, acc_base[a], acc_lens[a], off, ln, trim])
            owner.append(a)
    B = len(table)
    assert B <= 256 and len(table[0]) == K.ITEM_COLS
    items = [(r[5], r[6], r[7]) for r in table]
    acc0 = [rng.standard_normal((rows, n)).astype(F) for n in acc_lens]
    mo = rng.standard_normal((B, rows, valid)).astype(F)
    tiles, want = [], []
    for a in (0, 1):
        lo = max(0, min(x[0] for x in mine[a]))
        hi = min(acc_lens[a], max(x[0] + x[1] for x in mine[a]))
        tiles += [v for pos in range(lo, hi, K.TILE_SPAN) for v in (acc_base[a], acc_lens[a], pos, 0, B, w_off[a], w_len[a])]
        order = [i for i in range(B) if owner[i] == a]
        asc = ref_accumulate(acc0[a], mo, weights[w_off[a]:w_off[a] + w_len[a]], items, valid, 0, acc_lens[a], order)
        desc = ref_accumulate(acc0[a], mo, weights[w_off[a]:w_off[a] + w_len[a]], items, valid, 0, acc_lens[a], order[::-1])
        assert (order_matters(asc, desc) >= acc_lens[a] // 4).all()            # the packed case is order-sensitive as well
        want.append(asc)
    assert len(tiles) % K.TILE_COLS == 0
    acc, d_mo, d_w = Guarded(np.concatenate([a.reshape(-1) for a in acc0])), Guarded(mo), Guarded(weights)
    t_items, t_tiles = i64(table), i64(tiles)
    _lib.check(lib.mi_ola_accumulate_packed(acc.ptr(), acc.n, rows, d_mo.ptr(), valid, d_mo.n, t_items.data_ptr(), B,
                                            t_tiles.data_ptr(), len(tiles) // K.TILE_COLS, d_w.ptr(), d_w.n, stream()),
               "mi_ola_accumulate_packed")
    got = acc.read()
    for a in (0, 1):
        part = got[acc_base[a]:acc_base[a] + rows * acc_lens[a]].reshape(rows, acc_lens[a])
        assert_same_bits(part, want[a], f"packed accumulator {a}")


# ---- 3. finish -------------------------------------------------------------------------------------------------------------------
def run_finish(lib, acc0, acc_off0, segs, w):
    rows, acc_len = acc0.shape
    acc, d_w = Guarded(acc0), Guarded(w)
    offs, lens = i64([s[0] for s in segs]), i32([s[1] for s in segs])
    status = lib.mi_ola_finish(acc.ptr(), acc_len, rows, acc_off0, offs.data_ptr(), lens.data_ptr(), len(segs), len(w), d_w.ptr(),
                               stream())
    torch.cuda.synchronize()
    return status, acc.read()


def fourfold_segments(total):
    """Stride-16 segments over [0, total): the last ones are shorter, and one in the middle is longer than the ramp."""
    segs = [(o, min(total - o, RAMP)) for o in range(0, total, STRIDE)]
    if len(segs) > 20:
        segs[10] = (segs[10][0], 100)
    return segs


@pytest.mark.parametrize("acc_off0", [0, 777])
@pytest.mark.parametrize("acc_len", [1, 1023, 1024, 1025, 3300])
def test_ola_finish_divides_by_the_ascending_sum_of_weights(lib, acc_len, acc_off0):
    """With acc_off0 = 777 the segments start before the accumulator's origin."""
    rng = np.random.default_rng(acc_len + acc_off0)
    rows = 2
    # away from the ends sum_weight repeats every 16 positions, so the order matters at k / 16 of them: this ramp has k = 7
    w = ramp(np.random.default_rng(1))
    segs = fourfold_segments(acc_off0 + acc_len)
    acc0 = rng.standard_normal((rows, acc_len)).astype(F)
    if acc_len == 3300:
        assert len(segs) > 150
        asc = ref_sum_weight(acc_len, acc_off0, segs, w, range(len(segs)))
        desc = ref_sum_weight(acc_len, acc_off0, segs, w, reversed(range(len(segs))))
        differ = order_matters(asc, desc)
        print("sum_weight positions at which the order matters:", differ.tolist())
        assert (differ >= ORDER_MIN).all(), f"the inputs do not tell the orders apart: {differ.tolist()}"
    want = ref_finish(acc0, acc_off0, segs, w)
    assert np.isfinite(want).all()
    status, got = run_finish(lib, acc0, acc_off0, segs, w)
    assert status == 0, lib.mi_last_error()
    assert_same_bits(got, want, "finish")


def search_edge_segments(acc_len, acc_off0):
    """Four-fold background with a gap, and around the second and the third tile (first position pb, absolute) one segment each that
    ends just before pb, that covers exactly pb, that starts on the tile's last position and that starts on the next tile."""
    total = acc_off0 + acc_len
    segs = [(o, min(total - o, RAMP)) for o in range(0, total, STRIDE) if not 1300 <= o < 1500]
    for t in (1, 2):
        pb = acc_off0 + t * K.TILE_SPAN
        segs += [(pb - RAMP, RAMP), (pb - RAMP + 1, RAMP), (pb + K.TILE_SPAN - 1, RAMP), (pb + K.TILE_SPAN, RAMP)]
    segs += [(500, 100), (520, 10)]                    # longer than the ramp; shorter than its neighbours
    return sorted((o, min(n, total - o)) for o, n in segs if o < total)


@pytest.mark.parametrize("acc_off0", [0, 777])
def test_ola_finish_search_edges_and_a_gap(lib, acc_off0):
    rng = np.random.default_rng(50 + acc_off0)
    rows, acc_len = 2, 3300
    w = ramp(rng)
    segs = search_edge_segments(acc_len, acc_off0)
    acc0 = rng.standard_normal((rows, acc_len)).astype(F)
    sw = ref_sum_weight(acc_len, acc_off0, segs, w, range(len(segs)))
    gap = np.flatnonzero(sw == 0)
    assert len(gap) > 3 and (np.diff(gap) == 1).all() and gap[0] > 0 and gap[-1] < acc_len - 1, "one gap inside the accumulator"
    acc0[0, gap[3]] = 0.0                               # 0 / 0
    want = ref_finish(acc0, acc_off0, segs, w)
    assert np.isnan(want[0, gap[3]]) and np.isinf(want[1, gap]).all()
    status, got = run_finish(lib, acc0, acc_off0, segs, w)
    assert status == 0, lib.mi_last_error()
    assert_same_bits(got, want, "finish at the search edges")


def test_ola_finish_packed(lib):
    """Two accumulators in one buffer, each with its own range of the segment list and its own ramp."""
    rng = np.random.default_rng(6)
    rows = 3
    acc_lens = [3300, 1025]
    acc_base = [0, rows * acc_lens[0]]
    w_off, w_len = [0, RAMP], [RAMP, 48]
    weights = ramp(rng, sum(w_len))
    per_acc = [search_edge_segments(acc_lens[0], 0), fourfold_segments(acc_lens[1])]
    acc0 = [rng.standard_normal((rows, n)).astype(F) for n in acc_lens]
    segs, tiles, want = [], [], []
    for a in (0, 1):
        s0 = len(segs) // 2
        for o, n in per_acc[a]:
            segs += [o, n]
        tiles += [v for pos in range(0, acc_lens[a], K.TILE_SPAN)
                  for v in (acc_base[a], acc_lens[a], pos, s0, len(segs) // 2, w_off[a], w_len[a])]
        want.append(ref_finish(acc0[a], 0, per_acc[a], weights[w_off[a]:w_off[a] + w_len[a]]))
    acc, d_w = Guarded(np.concatenate([a.reshape(-1) for a in acc0])), Guarded(weights)
    t_tiles, t_segs = i64(tiles), i64(segs)
    _lib.check(lib.mi_ola_finish_packed(acc.ptr(), acc.n, rows, t_tiles.data_ptr(), len(tiles) // K.TILE_COLS, t_segs.data_ptr(),
                                        len(segs) // 2, d_w.ptr(), d_w.n, stream()), "mi_ola_finish_packed")
    got = acc.read()
    for a in (0, 1):
        part = got[acc_base[a]:acc_base[a] + rows * acc_lens[a]].reshape(rows, acc_lens[a])
        assert_same_bits(part, want[a], f"packed accumulator {a}")


# ---- 4. what does not fit a launch grid is refused before anything is launched ---------------------------------------------------
TOO_MANY = 65536                                        # one more than a grid's y or z extent; every buffer has its full size


def test_segments_gather_refuses_what_its_grid_cannot_hold(lib):
    seg = Guarded(np.full(TOO_MANY, SENTINEL, F))
    track, starts = Guarded(np.ones(TOO_MANY, F)), i64(np.zeros(TOO_MANY))
    for channels, B in [(TOO_MANY, 1), (1, TOO_MANY)]:
        status = lib.mi_segments_gather(track.ptr(), 1, channels, starts.data_ptr(), B, 1, seg.ptr(), seg.n, stream())
        assert status != 0, (channels, B)
    torch.cuda.synchronize()
    assert_same_bits(seg.read(), np.full(TOO_MANY, SENTINEL, F), "a refused gather")


def test_ola_accumulate_refuses_more_rows_than_its_grid_holds(lib):
    acc = Guarded(np.full((TOO_MANY, 1), SENTINEL, F))
    mo, w = Guarded(np.ones(TOO_MANY, F)), Guarded(np.ones(4, F))
    offs, lens, trims = i64([0]), i32([1]), i32([0])
    status = lib.mi_ola_accumulate(acc.ptr(), 1, TOO_MANY, mo.ptr(), 1, mo.n, offs.data_ptr(), lens.data_ptr(), trims.data_ptr(), 1,
                                   0, 1, w.ptr(), 4, stream())
    assert status != 0
    torch.cuda.synchronize()
    assert_same_bits(acc.read(), np.full((TOO_MANY, 1), SENTINEL, F), "a refused accumulate")


def test_ola_finish_refuses_more_rows_than_its_grid_holds(lib):
    acc, w = Guarded(np.full((TOO_MANY, 1), SENTINEL, F)), Guarded(np.ones(4, F))
    offs, lens = i64([0]), i32([1])
    status = lib.mi_ola_finish(acc.ptr(), 1, TOO_MANY, 0, offs.data_ptr(), lens.data_ptr(), 1, 4, w.ptr(), stream())
    assert status != 0
    torch.cuda.synchronize()
    assert_same_bits(acc.read(), np.full((TOO_MANY, 1), SENTINEL, F), "a refused finish")
