"""The streaming track statistics alone through the C ABI: `mi_mono_stats_update` x k + `mi_mono_stats_finish` against
`mi_mono_stats` on the whole track.

`mi_mono_stats` runs on a fixed grid of 1024 x 256 = 262 144 threads; position p belongs to thread p % 262144, which adds its
positions in ascending order in float64.  The streaming entries carry one (sum, sum of squares) pair per thread and add a block's
positions to them in that order, so the result is the one-shot kernel's for EVERY partition of the track: the comparison is of
bit patterns (every NaN as one pattern).  Lengths 1 .. 524 289 leave a slot empty, hit it once and hit it twice; the partitions
put block edges on the 256-thread and the 262 144-slot boundaries, and blocks across the wrap.

Independent reference.  For lengths up to 300 001 both values are also within one float32 ulp of the float64 statistics:
test_gpu_post.py derives that bound for `mi_mono_stats` (a float64 reduction of at most 300 001 float32 values is wrong by a few
1e-16 of its result, the one-pass variance of the "offset" family loses 18 of 53 bits, which leaves an error near 1e-10 of the std
against half a float32 ulp of 3e-8; so the only freedom is the rounding neighbour).  The bound is restated here, not re-measured.

The state lies between guard floats that must keep their value; the statistics start as a sentinel."""
import ctypes as C

import numpy as np
import pytest
import torch

from demucs_amd import _lib, audio
from demucs_amd.audio import PCM_FORMATS, PCM_PLANAR
from test_gpu_ingest import device_bytes, encode, wire_values
from test_gpu_post import SENTINEL, Guarded, assert_same_bits, mono, mono_input, ref_mono_stats, run_mono_stats

pytestmark = pytest.mark.gpu
F = np.float32
SLOTS = 1024 * 256
LENGTHS = [1, 2, 255, 256, 257, 262143, 262144, 262145, 300001, 524289]
FAMILIES = ["noise", "offset", "zeros", "nan", "inf"]


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    lib = _lib.load()
    assert lib.mi_mono_stats_state_bytes() == 2 * SLOTS * 8
    return lib


def stream():
    return C.c_void_p(_lib.current_stream_ptr())


def track(family, channels, length):
    if family in ("nan", "inf"):
        wav = mono_input("noise", channels, length)
        wav[(channels - 1) % channels, length // 3] = F("nan") if family == "nan" else F("inf")
        return wav
    return mono_input(family, channels, length)


class State:
    """The carried sums as all-zero bytes between guards, and the entries on them."""

    def __init__(self, lib):
        self.lib = lib
        self.buf = Guarded(np.zeros(lib.mi_mono_stats_state_bytes() // 4, F))
        assert self.buf.ptr() % 8 == 0
        self.scratch = torch.empty(lib.mi_mono_stats_scratch_bytes(), dtype=torch.uint8, device="cuda")

    def update(self, src_ptr, fmt, src_ch, n, channels, before):
        return self.lib.mi_mono_stats_update(src_ptr, fmt, src_ch, n, channels, before, self.buf.ptr(), stream())

    def planar(self, wav, cuts, base=0):
        """The (channels, length) track in blocks [cuts[i], cuts[i + 1]), each a contiguous device block of its own size."""
        channels = wav.shape[0]
        for a, b in zip(cuts[:-1], cuts[1:]):
            blk = torch.from_numpy(np.ascontiguousarray(wav[:, a:b])).cuda() if b > a else None
            _lib.check(self.update(blk.data_ptr() if blk is not None else None, PCM_PLANAR, channels, b - a, channels, base + a),
                       "mi_mono_stats_update")

    def finish(self, length):
        stats = Guarded(np.full(2, SENTINEL, F))
        _lib.check(self.lib.mi_mono_stats_finish(self.buf.ptr(), length, self.scratch.data_ptr(), stats.ptr(), stream()),
                   "mi_mono_stats_finish")
        return stats.read()

    def words(self):
        """The state's bits, after checking the guards."""
        return self.buf.read().view(np.uint32)


def streamed(lib, wav, cuts, base=0):
    st = State(lib)
    st.planar(wav, cuts, base)
    got = st.finish(wav.shape[1])
    st.words()
    return got


def default_cuts(length):
    """Three blocks with edges off every boundary (fewer for the shortest tracks)."""
    return sorted({0, length // 3, (2 * length) // 3 + 1 if length > 2 else length, length})


_ONE_SHOT = {}


def one_shot(lib, family, channels, length):
    """`mi_mono_stats` on the whole track: computed once per track, shared, never changed."""
    key = (family, channels, length)
    if key not in _ONE_SHOT:
        got = run_mono_stats(lib, track(family, channels, length))
        got.setflags(write=False)
        _ONE_SHOT[key] = got
    return _ONE_SHOT[key]


# ---- 1. bit equality with the one-shot kernel, and the float64 reference ---------------------------------------------------------
@pytest.mark.parametrize("length", LENGTHS)
@pytest.mark.parametrize("channels", [1, 2, 3])
def test_blocks_give_the_one_shot_bits(lib, channels, length):
    for family in FAMILIES:
        wav = track(family, channels, length)
        want = one_shot(lib, family, channels, length)
        got = streamed(lib, wav, default_cuts(length))
        assert_same_bits(got, want, f"{family} channels {channels} length {length}")
        if family == "zeros" and length > 1:
            assert_same_bits(got, np.array([0.0, F(1e-8)], F), "statistics of silence")
        if family in ("noise", "offset") and 2 <= length <= 300001:
            for name, g, w in zip(("mean", "std + 1e-8"), got, ref_mono_stats(wav)):
                ulps = abs(float(g) - float(w)) / float(np.spacing(np.abs(w)))
                print(f"{family} channels {channels} length {length}: {name} stream {float(g):.9g} float64 {float(w):.9g}, {ulps:.2f} ulp")
                assert ulps <= 1.0, (name, float(g), float(w), ulps)


@pytest.mark.parametrize("channels", [1, 2, 3])
def test_one_sample_has_a_mean_and_no_std(lib, channels):
    """torch's unbiased std of one element is NaN."""
    wav = np.random.default_rng(channels).standard_normal((channels, 1)).astype(F)
    got = streamed(lib, wav, [0, 1])
    assert_same_bits(got[:1], mono(wav), "mean of one sample")
    assert np.isnan(got[1])
    assert_same_bits(got, run_mono_stats(lib, wav), "one sample")


# ---- 2. partitions ---------------------------------------------------------------------------------------------------------------
def around(length, centre):
    """1-sample blocks on both sides of `centre`."""
    return sorted({0, length} | {p for p in range(centre - 2, centre + 3) if 0 < p < length})


PARTITIONS = {
    "one block": lambda L: [0, L],
    "single samples around 256": lambda L: around(L, 256),
    "single samples around 262144": lambda L: around(L, SLOTS),
    "empty blocks between the others": lambda L: [0, 0, L // 5, L // 5, L // 5, L // 2, L // 2, L, L],
    "300 000 samples from 200 000": lambda L: [0, 200000, 500000, L],
    "seeded random": lambda L: [0] + sorted(int(v) for v in np.random.default_rng(L).integers(0, L + 1, 23)) + [L],
}


@pytest.mark.parametrize("name", list(PARTITIONS))
def test_every_partition_gives_the_same_bits(lib, name):
    ran = 0
    for family, channels, length in [("offset", 2, 524289), ("noise", 3, 300001), ("noise", 1, 262145)]:
        cuts = PARTITIONS[name](length)
        if cuts != sorted(cuts):
            continue                                        # the 300 000-sample block needs the longest track
        assert cuts[0] == 0 and cuts[-1] == length
        wav = track(family, channels, length)
        got = streamed(lib, wav, cuts)
        assert_same_bits(got, one_shot(lib, family, channels, length), f"{name}: {family} channels {channels} length {length}")
        ran += 1
    assert ran == (1 if name.startswith("300 000") else 3)


def test_positions_past_2_to_the_31_keep_their_slots(lib):
    """`before` is a 64-bit position: a track that starts a multiple of 262 144 later lands in the same slots."""
    wav = track("offset", 2, 300001)
    want = one_shot(lib, "offset", 2, 300001)
    for base in (SLOTS * (1 << 14), SLOTS * (1 << 40)):      # 2^32 and 2^58
        assert_same_bits(streamed(lib, wav, [0, 1, 257, 262145, 300001], base=base), want, f"base {base}")


# ---- 3. wire PCM blocks ------------------------------------------------------------------------------------------------------------
def pcm_values(fmt, count, seed):
    if fmt != "f32":
        return wire_values(fmt, count, seed)
    v = np.random.default_rng(seed).standard_normal(count).astype(F)       # finite: a NaN would hide every other sample
    v[::7] = np.array([0x80000000, 0x00000001, 0x807FFFFF, 0x00400000], dtype=np.uint32).view(F)[np.arange(len(v[::7])) % 4]
    return v


@pytest.mark.parametrize("src_ch", [1, 2, 3])
@pytest.mark.parametrize("fmt", ["i16", "i24", "f32"])
def test_pcm_blocks_equal_the_planar_route(lib, fmt, src_ch):
    code, width, _ = PCM_FORMATS[fmt]
    channels = 2
    for n, cuts in [(4099, [0, 1, 1000, 4099]), (SLOTS + 4099, [0, 777, SLOTS + 1, SLOTS + 4099])]:
        data = encode(fmt, pcm_values(fmt, n * src_ch, seed=n + src_ch))
        frame = src_ch * width
        st = State(lib)
        for i, (a, b) in enumerate(zip(cuts[:-1], cuts[1:])):
            shift = (1 + 2 * i) * (1 if fmt == "i24" else width)             # i24: odd byte addresses
            blk = device_bytes(data[a * frame:b * frame], shift)
            assert blk.data_ptr() % 2 == 1 or fmt != "i24"
            _lib.check(st.update(blk.data_ptr(), code, src_ch, b - a, channels, a), "mi_mono_stats_update")
        got = st.finish(n)
        st.words()
        dec = audio.pcm_to_tensor(data, fmt, src_ch)                         # (src_ch, n) on the device
        assert dec.shape == (src_ch, n)
        rows = (dec.expand(channels, n) if src_ch == 1 else dec[:channels]).contiguous().cpu().numpy()
        want = streamed(lib, rows, [0, n])
        assert np.isfinite(want).all()
        assert_same_bits(got, want, f"{fmt} src_ch {src_ch} n {n}")
        assert_same_bits(want, run_mono_stats(lib, rows), "the planar route itself")


# ---- 4. guards and refusals ------------------------------------------------------------------------------------------------------------
def test_finish_only_reads_the_state(lib):
    wav = track("noise", 2, 300001)
    st = State(lib)
    st.planar(wav, [0, 100000])
    before = st.words().copy()
    first = st.finish(100000)
    second = st.finish(100000)
    assert_same_bits(second, first, "a second finish")
    assert np.array_equal(st.words(), before)
    assert_same_bits(first, run_mono_stats(lib, np.ascontiguousarray(wav[:, :100000])), "the prefix")
    st.planar(wav, [100000, 300001])                                         # more blocks may follow a finish
    assert_same_bits(st.finish(300001), one_shot(lib, "noise", 2, 300001), "the whole track after a finish on its prefix")


def test_refused_calls_touch_nothing(lib):
    st = State(lib)
    wav = track("noise", 2, 1000)
    st.planar(wav, [0, 1000])
    before = st.words().copy()
    raw = torch.zeros(64 + 12 * 1000, dtype=torch.uint8, device="cuda")
    p = raw.data_ptr()
    assert p % 16 == 0
    i16, i24, f32 = (PCM_FORMATS[k][0] for k in ("i16", "i24", "f32"))
    refused = [
        ("i16 at an odd address", (p + 1, i16, 2, 1000, 2, 1000)),
        ("f32 two bytes off", (p + 2, f32, 2, 1000, 2, 1000)),
        ("planar two bytes off", (p + 2, PCM_PLANAR, 2, 1000, 2, 1000)),
        ("format 4", (p, 4, 2, 1000, 2, 1000)),
        ("format -1", (p, -1, 2, 1000, 2, 1000)),
        ("two channels into three rows", (p, i16, 2, 1000, 3, 1000)),
        ("no source channel", (p, i24, 0, 1000, 2, 1000)),
        ("no row", (p, f32, 2, 1000, 0, 1000)),
        ("no planar row", (p, PCM_PLANAR, 2, 1000, 0, 1000)),
        ("a negative position", (p, i16, 2, 1000, 2, -1)),
        ("a negative count", (p, i16, 2, -1, 2, 1000)),
        ("no source", (None, i16, 2, 1000, 2, 1000)),
    ]
    for what, args in refused:
        assert st.update(*args) != 0, what
        assert lib.mi_last_error()
    torch.cuda.synchronize()
    assert np.array_equal(st.words(), before), "a refused update changed the state"
    assert lib.mi_mono_stats_update(p, i16, 2, 1000, 2, 1000, None, stream()) != 0
    assert lib.mi_mono_stats_update(p, i16, 2, 1000, 2, 1000, st.buf.ptr() + 4, stream()) != 0       # doubles 4 bytes off
    assert st.update(None, i16, 2, 0, 2, 1000) == 0                           # n = 0 does nothing, whatever the source
    assert st.update(p + 1, i24, 3, 1000, 2, 2000) == 0                       # i24 takes any byte address (zeros: sums unchanged)
    stats = Guarded(np.full(2, SENTINEL, F))
    for length in (0, -5):
        assert lib.mi_mono_stats_finish(st.buf.ptr(), length, st.scratch.data_ptr(), stats.ptr(), stream()) != 0
    assert lib.mi_mono_stats_finish(None, 1000, st.scratch.data_ptr(), stats.ptr(), stream()) != 0
    assert lib.mi_mono_stats_finish(st.buf.ptr(), 1000, None, stats.ptr(), stream()) != 0
    assert lib.mi_mono_stats_finish(st.buf.ptr(), 1000, st.scratch.data_ptr(), None, stream()) != 0
    assert_same_bits(stats.read(), np.full(2, SENTINEL, F), "the statistics after refused calls")
    assert np.array_equal(st.words(), before), "adding zeros or nothing changed the sums"
    assert_same_bits(st.finish(1000), run_mono_stats(lib, wav), "the state after the refused calls")
