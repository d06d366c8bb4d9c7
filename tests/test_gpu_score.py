"""The nSDR sums alone through the C ABI: `mi_sdr_update` x k + `mi_sdr_finish` against `mi_sdr` on the whole track, and both
against the float64 formula of the oracle's `new_sdr`.

Position p of a track belongs to slot p % K, K = 131 072 (demucs_amd/csrc/sdr_sums.h); a slot adds its positions in ascending order
in float64 and a fixed tree reduces the slots, so the (num, den) of every source are the same for EVERY partition of the track: the
comparison is of bit patterns (every NaN as one pattern).  Lengths 1 .. 2 K + 1 leave a slot empty, hit it once, twice and three
times; the partitions put block edges on the 256-thread and the K-slot boundaries, and blocks across the wrap.

Bound against the oracle (derived, not measured).  Each sum is of n <= 2^21 non-negative doubles (the squares themselves are exact
products of float32-derived doubles up to one rounding): in any order it is within n * 2^-53 ~ 2.4e-10 of exact, relative, which
already allows one more rounding per term.  Two sums on each of two sides: ~1e-9 on the ratio; 10 / ln 10 ~ 4.35, so the scores
differ by at most ~4e-9 dB.  1e-8 dB leaves a factor of two.

The state and the sums lie between guard floats that must keep their value; the sums start as a sentinel."""
import ctypes as C

import numpy as np
import pytest
import torch

from demucs_amd import _lib, audio
from demucs_amd.audio import PCM_FORMATS, PCM_PLANAR
from oracle import apply_oracle as A
from test_gpu_ingest import device_bytes, encode, wire_values
from test_gpu_post import SENTINEL, Guarded

pytestmark = pytest.mark.gpu
F = np.float32
K = 131072
LENGTHS = [1, 2, 255, 256, 257, K - 1, K, K + 1, 2 * K + 1]
SHAPES = [(1, 1), (4, 2), (8, 2), (3, 3)]
FAMILIES = ["noise", "offset", "zeros", "same", "nan", "inf"]
BOUND_DB = 1e-8


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    lib = _lib.load()
    assert audio.SDR_SLOTS == K
    for S in range(1, 9):
        assert lib.mi_sdr_state_bytes(S) == S * 2 * K * 8 and lib.mi_sdr_scratch_bytes(S) > 0
    assert lib.mi_sdr_state_bytes(0) == 0 and lib.mi_sdr_state_bytes(9) == 0
    return lib


def stream():
    return C.c_void_p(_lib.current_stream_ptr())


def pair(family, S, ch, L):
    """(references, estimates), float32 (S, ch, L)."""
    rng = np.random.default_rng(10000 * S + 100 * ch + L % 1000 + len(family))
    if family == "zeros":
        return np.zeros((S, ch, L), F), np.zeros((S, ch, L), F)
    if family == "offset":                                   # noise at 1e-3 on a DC offset of 0.5, a small error
        ref = (0.5 + 1e-3 * rng.standard_normal((S, ch, L))).astype(F)
        return ref, (ref + 1e-4 * rng.standard_normal((S, ch, L))).astype(F)
    ref = rng.standard_normal((S, ch, L)).astype(F)
    if family == "same":
        return ref, ref.copy()
    est = (ref + 0.3 * rng.standard_normal((S, ch, L))).astype(F)
    if family == "nan":
        ref[S - 1, ch - 1, L // 3] = F("nan")
    if family == "inf":
        est[0, 0, L // 2] = F("-inf")
    return ref, est


def bits(sums):
    """The bit patterns of float64 sums, every NaN as one pattern."""
    sums = np.ascontiguousarray(sums, dtype=np.float64)
    return np.where(np.isnan(sums), np.uint64(0x7FF8000000000000), sums.view(np.uint64))


def assert_same_bits(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.array_equal(bits(got), bits(want)), (what, got.tolist(), want.tolist())


def scores(sums):
    with np.errstate(all="ignore"):                          # an infinite den gives log10(0)
        return 10 * np.log10((sums[..., 0] + 1e-7) / (sums[..., 1] + 1e-7))


class Scorer:
    """The carried sums as all-zero bytes between guards, and the entries on them."""

    def __init__(self, lib, S, ch):
        self.lib, self.S, self.ch = lib, S, ch
        self.state = Guarded(np.zeros(lib.mi_sdr_state_bytes(S) // 4, F))
        assert self.state.ptr() % 8 == 0
        self.scratch = torch.empty(lib.mi_sdr_scratch_bytes(S), dtype=torch.uint8, device="cuda")

    def update(self, refs, fmt, src_ch, ref_stride, est_ptr, est_stride, n, before):
        ptrs = (C.c_void_p * len(refs))(*refs) if refs is not None else None
        return self.lib.mi_sdr_update(ptrs, fmt, src_ch, ref_stride, est_ptr, est_stride, self.S, self.ch, n, before, self.state.ptr(),
                                      stream())

    def planar(self, ref, est, cuts, base=0):
        """The device tracks (S, ch, L) in blocks [cuts[i], cuts[i + 1]), read in place: the row stride is the track's length."""
        L = ref.shape[2]
        for a, b in zip(cuts[:-1], cuts[1:]):
            _lib.check(self.update([ref.data_ptr() + 4 * a], PCM_PLANAR, self.ch, L, est.data_ptr() + 4 * a, L, b - a, base + a),
                       "mi_sdr_update")

    def finish(self):
        sums = Guarded(np.full(4 * self.S, SENTINEL, F))
        assert sums.ptr() % 8 == 0
        _lib.check(self.lib.mi_sdr_finish(self.state.ptr(), self.S, self.scratch.data_ptr(), sums.ptr(), stream()), "mi_sdr_finish")
        return sums.read().view(np.float64).reshape(self.S, 2)

    def words(self):
        """The state's bits, after checking the guards."""
        return self.state.read().view(np.uint32)


def whole(lib, ref, est):
    """`mi_sdr` on (B, S, ch, L) device tensors: (B, S, 2) float64."""
    B, S, ch, L = ref.shape
    state = Guarded(np.full(lib.mi_sdr_state_bytes(S) // 4, SENTINEL, F))       # mi_sdr zeroes it itself
    scratch = torch.empty(lib.mi_sdr_scratch_bytes(S), dtype=torch.uint8, device="cuda")
    sums = Guarded(np.full(4 * B * S, SENTINEL, F))
    _lib.check(lib.mi_sdr(ref.data_ptr() if L else None, est.data_ptr() if L else None, B, S, ch, L, state.ptr(), scratch.data_ptr(),
                          sums.ptr(), stream()), "mi_sdr")
    state.read()
    return sums.read().view(np.float64).reshape(B, S, 2)


def streamed(lib, ref, est, cuts, base=0):
    sc = Scorer(lib, ref.shape[0], ref.shape[1])
    sc.planar(ref, est, cuts, base)
    got = sc.finish()
    sc.words()
    return got


def partitions(L):
    out = {"three blocks off every boundary": sorted({0, L // 3, (2 * L) // 3 + 1 if L > 2 else L, L})}
    if L <= 257:
        out["one block per sample"] = list(range(L + 1))
    if L > 256:
        out["blocks that end on 256 and on K"] = sorted({0, 256, min(K, L), L})
    if L > K:
        out["a block across the slot wrap"] = sorted({0, K - 2, min(K + 5, L), L})
    return out


# ---- 1. partition independence, and 2. the float64 formula ------------------------------------------------------------------------------
@pytest.mark.parametrize("L", LENGTHS)
@pytest.mark.parametrize("S,ch", SHAPES)
def test_blocks_give_the_whole_track_bits_and_the_oracle_score(lib, S, ch, L):
    assert ch * L <= 1 << 21
    for family in FAMILIES:
        ref_h, est_h = pair(family, S, ch, L)
        ref, est = torch.from_numpy(ref_h).cuda(), torch.from_numpy(est_h).cuda()
        want = whole(lib, ref[None], est[None])[0]
        for name, cuts in partitions(L).items():
            assert_same_bits(streamed(lib, ref, est, cuts), want, f"{family} ({S}, {ch}, {L}): {name}")
        got = scores(want)
        with np.errstate(all="ignore"):
            oracle = A.new_sdr(torch.from_numpy(ref_h).double()[None], torch.from_numpy(est_h).double()[None])[0].numpy()
        print(f"{family} ({S}, {ch}, {L}): kernel {got.tolist()} oracle {oracle.tolist()}")
        if family in ("nan", "inf"):
            assert np.array_equal(np.isnan(got), np.isnan(oracle)) and np.isnan(got).any() == (family == "nan")
            inf = np.isinf(oracle)
            assert np.array_equal(np.isinf(got), inf) and np.array_equal(np.sign(got[inf]), np.sign(oracle[inf]))
            fin = np.isfinite(oracle)
            assert np.abs(got[fin] - oracle[fin]).max(initial=0.0) <= BOUND_DB
            continue
        assert np.isfinite(got).all()
        err = np.abs(got - oracle).max()
        print(f"    max |score - oracle| {err:.3e} dB")
        assert err <= BOUND_DB, (family, S, ch, L, err)
        if family == "zeros":
            assert_same_bits(want, np.zeros((S, 2)), "silence")
            assert (got == 0.0).all()
        if family == "same":
            assert (want[:, 1] == 0.0).all()
            assert np.abs(got - 10 * np.log10((want[:, 0] + 1e-7) / 1e-7)).max() <= BOUND_DB


def test_an_empty_track_scores_exactly_zero(lib):
    empty = torch.empty(2, 4, 2, 0, device="cuda")
    sums = whole(lib, empty, empty)
    assert_same_bits(sums, np.zeros((2, 4, 2)), "L = 0")
    assert np.array_equal(scores(sums), np.zeros((2, 4))) and not np.signbit(scores(sums)).any()


def test_a_batch_is_independent_tracks(lib):
    refs, ests = zip(*(pair(f, 4, 2, 3001) for f in ("noise", "offset", "inf")))
    ref, est = torch.from_numpy(np.stack(refs)).cuda(), torch.from_numpy(np.stack(ests)).cuda()
    got = whole(lib, ref, est)
    for b in range(3):
        assert_same_bits(got[b], whole(lib, ref[b:b + 1].contiguous(), est[b:b + 1].contiguous())[0], f"track {b}")
        assert_same_bits(got[b], streamed(lib, ref[b].contiguous(), est[b].contiguous(), [0, 1000, 3001]), f"track {b} in blocks")


def test_positions_past_2_to_the_31_keep_their_slots(lib):
    """`before` is a 64-bit position: a track that starts a multiple of K later lands in the same slots."""
    ref_h, est_h = pair("offset", 4, 2, K + 1)
    ref, est = torch.from_numpy(ref_h).cuda(), torch.from_numpy(est_h).cuda()
    want = whole(lib, ref[None], est[None])[0]
    for base in (K * (1 << 15), K * (1 << 41)):              # 2^32 and 2^58
        assert_same_bits(streamed(lib, ref, est, [0, 1, 257, K - 1, K + 1], base=base), want, f"base {base}")


def test_estimates_and_references_are_read_in_place_out_of_longer_tensors(lib):
    S, ch, L, N = 4, 2, K + 257, K + 300
    ref_h, est_h = pair("noise", S, ch, L)
    want = whole(lib, torch.from_numpy(ref_h).cuda()[None], torch.from_numpy(est_h).cuda()[None])[0]
    rng = np.random.default_rng(5)
    long_est, long_ref = (torch.from_numpy(rng.standard_normal((S, ch, N)).astype(F)).cuda() for _ in range(2))
    long_est[:, :, 5:5 + L] = torch.from_numpy(est_h).cuda()
    long_ref[:, :, 40:40 + L] = torch.from_numpy(ref_h).cuda()
    sc = Scorer(lib, S, ch)
    for a, b in [(0, 1000), (1000, K + 1), (K + 1, L)]:
        _lib.check(sc.update([long_ref.data_ptr() + 4 * (40 + a)], PCM_PLANAR, ch, N, long_est.data_ptr() + 4 * (5 + a), N, b - a, a),
                   "mi_sdr_update")
    assert_same_bits(sc.finish(), want, "strides greater than n")
    sc.words()


def test_finish_only_reads_the_state_and_more_blocks_may_follow(lib):
    S, ch, L = 4, 2, K + 1000
    ref_h, est_h = pair("noise", S, ch, L)
    ref, est = torch.from_numpy(ref_h).cuda(), torch.from_numpy(est_h).cuda()
    sc = Scorer(lib, S, ch)
    sc.planar(ref, est, [0, 70000])
    before = sc.words().copy()
    first = sc.finish()
    second = sc.finish()
    assert_same_bits(second, first, "a second finish")
    assert np.array_equal(sc.words(), before)
    prefix = whole(lib, ref[None, :, :, :70000].contiguous(), est[None, :, :, :70000].contiguous())[0]
    assert_same_bits(first, prefix, "the prefix")
    sc.planar(ref, est, [70000, L])
    assert_same_bits(sc.finish(), whole(lib, ref[None], est[None])[0], "the whole track after a finish on its prefix")


# ---- 3. wire PCM references ---------------------------------------------------------------------------------------------------------------
def pcm_values(fmt, count, seed):
    if fmt != "f32":
        return wire_values(fmt, count, seed)
    v = np.random.default_rng(seed).standard_normal(count).astype(F)       # finite: a NaN would hide every other sample
    v[::7] = np.array([0x80000000, 0x00000001, 0x807FFFFF, 0x00400000], dtype=np.uint32).view(F)[np.arange(len(v[::7])) % 4]
    return v


@pytest.mark.parametrize("src_ch", [1, 2])
@pytest.mark.parametrize("fmt", ["i16", "i24", "f32"])
def test_pcm_references_equal_the_planar_route(lib, fmt, src_ch):
    """One block per source, each the last bytes of its own allocation: a read past a block's end would leave the allocation."""
    code, width, _ = PCM_FORMATS[fmt]
    S, ch, n = 4, 2, K + 4099
    cuts = [0, 1, 1000, K + 1, n]
    frame = src_ch * width
    data = [encode(fmt, pcm_values(fmt, n * src_ch, seed=n + src_ch + 10 * s)) for s in range(S)]
    est = torch.from_numpy(np.random.default_rng(8).standard_normal((S, ch, n)).astype(F)).cuda()
    sc = Scorer(lib, S, ch)
    for i, (a, b) in enumerate(zip(cuts[:-1], cuts[1:])):
        blocks = []
        for s in range(S):
            shift = (1 + 2 * (i + s)) * (1 if fmt == "i24" else width)            # off 16-byte alignment; i24: odd byte addresses
            blk = device_bytes(data[s][a * frame:b * frame], shift, pad=0)
            assert blk.data_ptr() % 16 != 0 and (blk.data_ptr() % 2 == 1 or fmt != "i24")
            blocks.append(blk)
        _lib.check(sc.update([t.data_ptr() for t in blocks], code, src_ch, 0, est.data_ptr() + 4 * a, n, b - a, a), "mi_sdr_update")
    got = sc.finish()
    sc.words()
    rows = []
    for s in range(S):
        dec = audio.pcm_to_tensor(data[s], fmt, src_ch)                           # (src_ch, n) on the device: v / 32768, v / 8388608
        rows.append(dec.expand(ch, n) if src_ch == 1 else dec[:ch])
    ref = torch.stack(rows).contiguous()
    want = streamed(lib, ref, est, [0, n])
    assert np.isfinite(want).all() and (want > 0).all()
    assert_same_bits(got, want, f"{fmt} src_ch {src_ch}")
    assert_same_bits(want, whole(lib, ref[None], est[None])[0], "the planar route itself")


# ---- 4. refusals -----------------------------------------------------------------------------------------------------------------------------
def test_refused_calls_touch_nothing(lib):
    S, ch, n = 4, 2, 1000
    ref_h, est_h = pair("noise", S, ch, n)
    ref, est = torch.from_numpy(ref_h).cuda(), torch.from_numpy(est_h).cuda()
    sc = Scorer(lib, S, ch)
    sc.planar(ref, est, [0, n])
    before = sc.words().copy()
    raw = torch.zeros(64 + 12 * n, dtype=torch.uint8, device="cuda")
    p, r, e = raw.data_ptr(), ref.data_ptr(), est.data_ptr()
    assert p % 16 == 0
    i16, i24, f32 = (PCM_FORMATS[k][0] for k in ("i16", "i24", "f32"))
    ok = dict(refs=[p] * S, fmt=i16, src_ch=2, ref_stride=0, est_ptr=e, est_stride=n, n=n, before=n)
    refused = [
        ("i16 at an odd address", dict(refs=[p, p, p + 1, p])),
        ("f32 two bytes off", dict(refs=[p + 2] * S, fmt=f32)),
        ("planar two bytes off", dict(refs=[r + 2], fmt=PCM_PLANAR, ref_stride=n)),
        ("estimates two bytes off", dict(est_ptr=e + 2)),
        ("format 4", dict(fmt=4)),
        ("format -1", dict(fmt=-1)),
        ("two channels into three rows", dict(src_ch=2, refs=[p] * S), 3),
        ("no source channel", dict(src_ch=0, fmt=i24)),
        ("a negative position", dict(before=-1)),
        ("a negative count", dict(n=-1)),
        ("an estimates stride below n", dict(est_stride=n - 1)),
        ("a planar stride below n", dict(refs=[r], fmt=PCM_PLANAR, ref_stride=n - 1)),
        ("a null reference", dict(refs=[p, None, p, p])),
        ("no references", dict(refs=None)),
        ("no estimates", dict(est_ptr=None)),
    ]
    for what, change, *rows in refused:
        sc.ch = rows[0] if rows else ch
        assert sc.update(**{**ok, **change}) != 0, what
        assert lib.mi_last_error()
    sc.ch = ch
    for bad in (0, 9, -1):
        sc.S = bad
        assert sc.update(**{**ok, "refs": [p] * 8}) != 0, f"{bad} sources"
        sums = Guarded(np.full(4 * 8, SENTINEL, F))
        assert lib.mi_sdr_finish(sc.state.ptr(), bad, sc.scratch.data_ptr(), sums.ptr(), stream()) != 0
        assert lib.mi_sdr(r, e, 1, bad, ch, 10, sc.state.ptr(), sc.scratch.data_ptr(), sums.ptr(), stream()) != 0
        assert np.array_equal(sums.read(), np.full(4 * 8, SENTINEL, F))
    sc.S = S
    torch.cuda.synchronize()
    assert np.array_equal(sc.words(), before), "a refused update changed the state"
    ptrs = (C.c_void_p * S)(*[p] * S)
    assert lib.mi_sdr_update(ptrs, i16, 2, 0, e, n, S, ch, n, n, None, stream()) != 0
    assert lib.mi_sdr_update(ptrs, i16, 2, 0, e, n, S, ch, n, n, sc.state.ptr() + 4, stream()) != 0      # doubles 4 bytes off
    assert sc.update(**{**ok, "refs": None, "est_ptr": None, "n": 0}) == 0        # n = 0 does nothing, whatever the pointers
    assert sc.update(**{**ok, "refs": [p + 1] * S, "fmt": i24, "src_ch": 3}) == 0  # i24 takes any byte address
    sums = Guarded(np.full(4 * S, SENTINEL, F))
    assert lib.mi_sdr_finish(None, S, sc.scratch.data_ptr(), sums.ptr(), stream()) != 0
    assert lib.mi_sdr_finish(sc.state.ptr(), S, None, sums.ptr(), stream()) != 0
    assert lib.mi_sdr_finish(sc.state.ptr(), S, sc.scratch.data_ptr(), None, stream()) != 0
    assert lib.mi_sdr_finish(sc.state.ptr(), S, sc.scratch.data_ptr(), sums.ptr() + 4, stream()) != 0
    assert lib.mi_sdr(r, e, 1, S, ch, -1, sc.state.ptr(), sc.scratch.data_ptr(), sums.ptr(), stream()) != 0
    assert lib.mi_sdr(r, e, 0, S, ch, 10, sc.state.ptr(), sc.scratch.data_ptr(), sums.ptr(), stream()) != 0
    assert lib.mi_sdr(None, e, 1, S, ch, 10, sc.state.ptr(), sc.scratch.data_ptr(), sums.ptr(), stream()) != 0
    assert np.array_equal(sums.read(), np.full(4 * S, SENTINEL, F)), "the sums after refused calls"
    # the accepted i24 block of zeros against the estimates: den grows by sum est^2, num by nothing
    got = sc.finish()
    first = whole(lib, ref[None], est[None])[0]
    assert_same_bits(got[:, 0], first[:, 0], "num after a block of zero references")
    assert (got[:, 1] > first[:, 1]).all()
