"""The track-level kernels around `apply_model` (post.hip), each entry alone through the C ABI: `mi_mono_stats`, `mi_track_affine`,
`mi_prevent_clip` and `mi_two_stems`.  The streaming tests take the first two as helpers and references; the last two were
checked on one fixture of one size.

Reference.  Except for the statistics and tanh, every operation is a sequence of separately rounded float32 operations, so a plain
numpy float32 restatement is exact and the comparison is on bit patterns, NaN positions equal:

    affine      mode 0: f32(f32(x - mean) / s);  mode 1: f32(f32(x * s) + mean)
    rescale     peak = max |x|;  d = f32(peak * f32(1.01));  y = f32(x / d) if d > 1 or d is NaN, else x
    clamp       x if x is NaN, else min(max(x, -0.99), 0.99)
    add         a = f32(0); for k != sel in index order: a = f32(a + stem_k)
    minus       f32(origin - stem_sel)

`mi_mono_stats` reduces in float64: m = (float32 sum of the channels in index order) / f32(channels) per sample, then the float64
mean and unbiased std of m, rounded to float32, and 1e-8 added in float32.  A float64 reduction of at most 300 001 float32 values is
wrong by a few 1e-16 of its result; with the DC offset of 0.5 under noise of 1e-3 the one-pass variance `q - n mean^2` loses
log2(0.25 / 1e-6) = 18 of 53 bits, which leaves an error near 1e-10 of the std: orders of magnitude below half a float32 ulp
(3e-8).  So the only freedom is the rounding neighbour and the bound is one float32 ulp of the wanted value, for both outputs.
tanh keeps the project's bound of 2e-7 against the float64 tanh (libm).

Buffers that a kernel writes lie between guard floats that must keep their value, and an output starts as a sentinel.  Magnitudes
stay within [1e-6, 1e3]."""
import ctypes as C

import numpy as np
import pytest
import torch

from demucs_amd import _lib

pytestmark = pytest.mark.gpu
F = np.float32
GUARD, GUARD_VALUE, SENTINEL = 64, -12345.0, 54321.0
NAN, INF = float("nan"), float("inf")
CLIP_RESCALE, CLIP_CLAMP, CLIP_TANH = 1, 2, 3
TANH_BOUND = 2e-7


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
    """A float32 device buffer holding `values` between guard floats, `shift` floats behind a 16-byte boundary."""

    def __init__(self, values, shift=0):
        values = np.ascontiguousarray(values, dtype=F)
        self.shape, self.n, self.lo = values.shape, values.size, GUARD + shift
        self.buf = torch.full((self.n + 2 * GUARD + 4,), GUARD_VALUE, device="cuda")
        assert self.buf.data_ptr() % 16 == 0
        self.buf[self.lo:self.lo + self.n] = torch.from_numpy(values.reshape(-1)).cuda()

    def ptr(self):
        return self.buf.data_ptr() + 4 * self.lo

    def read(self):
        """The values on the host, after checking that the guards are as they were."""
        host = self.buf.cpu().numpy()
        guards = np.concatenate([host[:self.lo], host[self.lo + self.n:]])
        assert np.array_equal(guards.view(np.uint32), np.full(guards.size, GUARD_VALUE, F).view(np.uint32)), "written outside the buffer"
        return host[self.lo:self.lo + self.n].reshape(self.shape).copy()


# ---- mi_mono_stats ---------------------------------------------------------------------------------------------------------------
def run_mono_stats(lib, wav):
    channels, length = wav.shape
    dev = torch.from_numpy(wav).cuda()
    scratch = torch.empty(lib.mi_mono_stats_scratch_bytes(), dtype=torch.uint8, device="cuda")
    stats = Guarded(np.full(2, SENTINEL, F))
    _lib.check(lib.mi_mono_stats(dev.data_ptr(), channels, length, scratch.data_ptr(), stats.ptr(), stream()), "mi_mono_stats")
    return stats.read()


def mono(wav):
    a = wav[0].copy()
    for c in range(1, wav.shape[0]):
        a = (a + wav[c]).astype(F)
    return (a / F(wav.shape[0])).astype(F)


def ref_mono_stats(wav):
    m = mono(wav).astype(np.float64)
    return F(m.mean()), F(F(m.std(ddof=1)) + F(1e-8))


def mono_input(family, channels, length):
    rng = np.random.default_rng(1000 * channels + length % 1000)
    if family == "zeros":
        return np.zeros((channels, length), F)
    if family == "offset":                              # noise at 1e-3 on a DC offset of 0.5
        return (0.5 + 1e-3 * rng.standard_normal((channels, length))).astype(F)
    return rng.standard_normal((channels, length)).astype(F)


# one pass of the statistics grid is 1024 x 256 = 262 144 samples
@pytest.mark.parametrize("length", [2, 255, 256, 257, 262144, 262145, 300001])
@pytest.mark.parametrize("channels", [1, 2, 3])
@pytest.mark.parametrize("family", ["noise", "offset", "zeros"])
def test_mono_stats(lib, family, channels, length):
    wav = mono_input(family, channels, length)
    want = ref_mono_stats(wav)
    got = run_mono_stats(lib, wav)
    if family == "zeros":
        assert_same_bits(got, np.array([0.0, F(1e-8)], F), "statistics of silence")
        return
    for name, g, w in zip(("mean", "std + 1e-8"), got, want):
        ulps = abs(float(g) - float(w)) / float(np.spacing(np.abs(w)))
        print(f"{family} channels {channels} length {length}: {name} kernel {float(g):.9g} float64 {float(w):.9g}, {ulps:.2f} ulp")
        assert ulps <= 1.0, (name, float(g), float(w), ulps)


@pytest.mark.parametrize("channels", [1, 2, 3])
def test_mono_stats_of_one_sample_has_no_std(lib, channels):
    """torch's unbiased std of one element is NaN."""
    wav = np.random.default_rng(channels).standard_normal((channels, 1)).astype(F)
    got = run_mono_stats(lib, wav)
    assert_same_bits(got[:1], mono(wav), "mean of one sample")
    assert np.isnan(got[1])


# ---- mi_track_affine -------------------------------------------------------------------------------------------------------------
AFFINE_STATS = [(F(0.25), F(1.75)), (F(-3e-3), F(1e-8 + 2e-4))]


def ref_affine(x, mean, s, mode):
    with np.errstate(all="ignore"):
        return ((x - mean).astype(F) / s).astype(F) if mode == 0 else ((x * s).astype(F) + mean).astype(F)


@pytest.mark.parametrize("shift", [0, 1, 2, 3])
@pytest.mark.parametrize("n", [1, 3, 4, 5, 1023, 1024, 1025, 4099])
def test_track_affine(lib, n, shift):
    """A buffer that starts `shift` floats behind a 16-byte boundary: 1 to 3 take the 4-byte path, 0 the 16-byte path and its tail."""
    rng = np.random.default_rng(10 * n + shift)
    x = rng.standard_normal(n).astype(F)
    for k, special in enumerate([NAN, INF, -INF, -0.0]):
        x[(7 * k + shift) % n] = special                # n = 1 meets one special per shift
    for mean, s in AFFINE_STATS:
        stats = torch.tensor([mean, s], dtype=torch.float32).cuda()
        for mode in (0, 1):
            buf = Guarded(x, shift)
            assert buf.ptr() % 16 == 4 * shift
            _lib.check(lib.mi_track_affine(buf.ptr(), n, stats.data_ptr(), mode, stream()), "mi_track_affine")
            assert_same_bits(buf.read(), ref_affine(x, mean, s, mode), f"affine mode {mode}, stats ({mean}, {s})")


# ---- mi_prevent_clip -------------------------------------------------------------------------------------------------------------
def run_clip(lib, x, mode):
    src, y = Guarded(x), Guarded(np.full(x.shape, SENTINEL, F))
    peak = torch.full((1,), 0x55555555, dtype=torch.int32, device="cuda")       # the entry clears it itself
    status = lib.mi_prevent_clip(src.ptr(), x.size, mode, peak.data_ptr(), y.ptr(), stream())
    torch.cuda.synchronize()
    assert_same_bits(src.read(), x, "the input of prevent_clip")
    return status, y.read()


def ref_rescale(x):
    with np.errstate(all="ignore"):
        a = np.abs(x)
        peak = F(NAN) if np.isnan(a).any() else a.max()
        d = F(peak * F(1.01))
        return (x / d).astype(F) if (d > 1 or np.isnan(d)) else x.copy()


CLIP_SIZES = [1, 255, 256, 257, 2048 * 256 + 1]         # the last one enters the grid-stride loop of the peak reduction


def quiet(n, seed):
    """Samples below 0.9: 1.01 times their peak stays under 1."""
    return np.random.default_rng(seed).uniform(-0.9, 0.9, n).astype(F)


@pytest.mark.parametrize("where,peak", [("last", 3.7), ("last", -3.7), ("first", 3.7), ("first", -3.7)])
@pytest.mark.parametrize("n", CLIP_SIZES)
def test_rescale_finds_a_peak_that_one_thread_sees(lib, n, where, peak):
    x = quiet(n, n)
    x[-1 if where == "last" else 0] = peak
    want = ref_rescale(x)
    assert float(np.abs(want).max()) < 1.0
    status, got = run_clip(lib, x, CLIP_RESCALE)
    assert status == 0, lib.mi_last_error()
    assert_same_bits(got, want, "rescale")


@pytest.mark.parametrize("n", CLIP_SIZES)
def test_rescale_special_peaks(lib, n):
    cases = {"quiet": quiet(n, n + 1)}                  # 1.01 peak <= 1: the input's bits
    cases["one"] = cases["quiet"].copy()
    cases["one"][n // 2] = F(1.0) / F(1.01)             # 1.01 peak rounds to 1 or just beside it: the reference decides
    cases["inf"] = cases["quiet"].copy()
    cases["inf"][-1] = -INF                             # finite / inf = +-0, inf / inf = NaN
    cases["nan"] = cases["quiet"].copy()
    cases["nan"][n // 3] = NAN                          # every output NaN
    for name, x in cases.items():
        want = ref_rescale(x)
        if name == "quiet":
            assert_same_bits(want, x, "the reference on a quiet input")
        if name == "nan":
            assert np.isnan(want).all()
        status, got = run_clip(lib, x, CLIP_RESCALE)
        assert status == 0, lib.mi_last_error()
        assert_same_bits(got, want, f"rescale, {name}")


@pytest.mark.parametrize("n", CLIP_SIZES)
def test_clamp_and_tanh(lib, n):
    x = (np.random.default_rng(n + 2).standard_normal(n) * 1.5).astype(F)
    for k, special in enumerate([NAN, INF, -INF, -0.0, 0.99, -0.99, np.nextafter(F(0.99), F(1)), np.nextafter(F(-0.99), F(-1))]):
        x[(7 * k) % n] = special
    status, got = run_clip(lib, x, CLIP_CLAMP)
    assert status == 0, lib.mi_last_error()
    with np.errstate(all="ignore"):
        want = np.where(np.isnan(x), x, np.minimum(np.maximum(x, F(-0.99)), F(0.99))).astype(F)
    assert_same_bits(got, want, "clamp")
    status, got = run_clip(lib, x, CLIP_TANH)
    assert status == 0, lib.mi_last_error()
    want = np.tanh(x.astype(np.float64))
    assert np.array_equal(np.isnan(got), np.isnan(want))
    finite = ~np.isnan(want)
    err = float(np.abs(got[finite].astype(np.float64) - want[finite]).max()) if finite.any() else 0.0
    print(f"tanh n {n}: {err:.2e} (bound {TANH_BOUND:.0e})")
    assert err <= TANH_BOUND


def test_prevent_clip_refuses_an_unknown_mode(lib):
    x = quiet(257, 0)
    for mode in (0, 4):
        status, got = run_clip(lib, x, mode)
        assert status != 0
        assert_same_bits(got, np.full(x.shape, SENTINEL, F), "a refused call")


# ---- mi_two_stems ----------------------------------------------------------------------------------------------------------------
def run_two_stems(lib, stems, n_stems, sel, origin, minus, n):
    """`stems`: Guarded buffers (at least n_stems of them unless the call is to be refused); returns (status, y)."""
    y = Guarded(np.full(n, SENTINEL, F))
    ptrs = (C.c_void_p * max(n_stems, 1))(*[s.ptr() for s in stems[:n_stems]])
    status = lib.mi_two_stems(ptrs, n_stems, sel, origin.ptr() if origin is not None else None, int(minus), n, y.ptr(), stream())
    torch.cuda.synchronize()
    return status, y.read()


def ref_add(stems, sel):
    a = np.zeros_like(stems[0])
    for k, s in enumerate(stems):
        if k != sel:
            a = (a + s).astype(F)
    return a


@pytest.mark.parametrize("n", [1, 255, 257])
@pytest.mark.parametrize("n_stems", [1, 2, 4, 6, 8])
def test_two_stems(lib, n_stems, n):
    rng = np.random.default_rng(100 * n_stems + n)
    # magnitudes over three decades: the float32 sum of four or more of them depends on the order
    stems = [(rng.standard_normal(n) * 10.0 ** rng.uniform(-1, 2, n)).astype(F) for _ in range(n_stems)]
    for s in stems:
        s[0] = -0.0                                     # with one stem left, 0 + -0.0 = +0.0: the sum starts from zero
    origin = rng.standard_normal(n).astype(F)
    d_stems, d_origin = [Guarded(s) for s in stems], Guarded(origin)
    for sel in range(n_stems):
        want = ref_add(stems, sel)
        if n_stems == 2:
            assert bits(want)[0] == 0 and bits(stems[1 - sel])[0] == 0x80000000
        if n_stems >= 4 and n > 1:                      # (with n = 1 the one sample is the -0.0 of every stem)
            rev = ref_add(stems[::-1], n_stems - 1 - sel)
            assert (bits(rev) != bits(want)).any(), "the inputs do not tell the stem orders apart"
        status, got = run_two_stems(lib, d_stems, n_stems, sel, None, False, n)
        assert status == 0, lib.mi_last_error()
        assert_same_bits(got, want, f"add, without stem {sel} of {n_stems}")
        status, got = run_two_stems(lib, d_stems, n_stems, sel, d_origin, True, n)
        assert status == 0, lib.mi_last_error()
        assert_same_bits(got, (origin - stems[sel]).astype(F), f"minus, stem {sel} of {n_stems}")
    for s, d in zip(stems + [origin], d_stems + [d_origin]):
        assert_same_bits(d.read(), s, "an input of two_stems")


def test_two_stems_refuses_nine_stems_and_a_selection_outside(lib):
    n = 257
    stems = [Guarded(np.ones(n, F)) for _ in range(9)]
    for n_stems, sel in [(9, 0), (4, 4), (8, 8), (4, -1), (0, 0)]:
        status, got = run_two_stems(lib, stems, n_stems, sel, None, False, n)
        assert status != 0, (n_stems, sel)
        assert_same_bits(got, np.full(n, SENTINEL, F), "a refused call")
    status, got = run_two_stems(lib, stems, 4, 1, None, True, n)              # "minus" without the mix
    assert status != 0
    assert_same_bits(got, np.full(n, SENTINEL, F), "a refused call")
