"""The transforms at both ends of every forward and the per-item normalisation around them, each alone through the C ABI, against
float64: fft.hip (`mi_stft_cac`, `mi_stft_norm`: walking STFT + float64 statistics + finalisation + normalising transpose into a
pitched conv layout; `mi_istft_full`: de-normalising transpose of a pitched spectrogram + fused inverse transform / overlap-add +
the time branch's `xt * std_t + mean_t`) and norms.hip (`mi_item_norm`: row_stats + finalize_stats mode 1 + row_affine;
`mi_item_denorm`: row_denorm).

Reference: `oracle.htdemucs_oracle.stft_cac` / `istft_from_cac` in float64 (restatements of demucs/htdemucs.py:420-471 with pad1d's
short-input rule) and plain torch float64 for the means, the unbiased stds, `(v - mean) / (1e-5 + std)`, `v * std + mean` and the
time-branch add.

Inputs are drawn in float64 from seeded generators and rounded to float32 once.  Two families:
    plain    N(0, 1)
    offset   8 + N(0, 1) for the STFT's waveform (the DC bin is about 250 times the others and carries 99 % of the spectrogram's
             energy: |x| max is 60 std), 3 + N(0, 1) for the item-norm rows and for the time branch's xt; the de-normalisation pairs of
             the iSTFT have means around 3
iSTFT inputs are random in every plane, so the DC bin has an imaginary part, which the kernels must ignore as irfft does.  Outputs
start as NaN between guard floats; the pitch columns of outputs start as a sentinel and must keep it; those of inputs are NaN.

Lengths (T = ceil(L / 1024)): 1, 2, 1 023 (pad1d zero-pads on both sides, one frame), 1 024 (last T = 1), 1 025, 1 792 / 1 793 and
2 304 / 2 305 (pad1d zero-pads while L <= 1536 + 1024 T - L: the last length that does and the first that does not, at T = 2 and at
T = 3), 2 559 / 2 560, 4 096 / 4 097, 5 000, 12 000 (fused iSTFT: 13 hop blocks in two runs of 7: the seam),
33 793 (T = 34: 34 STFT workgroups on 32 statistics slots), 344 065 (T = 337: a second strip of one frame, 4-byte accesses),
348 160 (T = 340: a second strip of four frames, 16-byte accesses).  Row pitches T and max(32, T rounded up to 4) for spectrograms,
L and L rounded up to 4 for xt: T = 4, 12 (pitch 32) take the 16-byte path with a pitch that differs from T, odd T the 4-byte path.

Tolerances.  None is taken from the kernels.  The same oracle evaluated in float32 on the CPU (torch's float32 FFT, mean and std) is
the yardstick: its largest distance from float64 over every case of a family in this file is RESTATED[family][quantity], and the
kernels get 4x that (another summation order, another factorisation of the transform; the rule of test_gpu_token_norm.py and
test_gpu_dconv_fused.py).  Quantities: the raw spectrogram relative to max(1, |want| max); the normalised spectrogram, absolute; the
waveform relative to |want| max; a mean as |error| / std; a std as relative error; the item-norm output, absolute.  The statistics
have a floor of two float32 ulps (2^-22 of the std; 2^-22 max(|mean|, std) / std for a mean), because the float32 restatement can
land exactly on the rounded float64 value.  The restatement's figures vary a little with the host's FFT and reduction code: they
are printed next to the kernel's with each bound, not asserted; the constants are the smaller figures seen.  `row_denorm` is one
float32 product and one sum: |y - y64| <= 2^-24 (|x std| + |y|) elementwise.  DESIGN.md (kernel-level parity) lists the constants."""
import ctypes as C

import pytest
import torch

from demucs_amd import _lib
from oracle import htdemucs_oracle as O

pytestmark = pytest.mark.gpu
NAN = float("nan")
EPS = 1e-5
GUARD, GUARD_VALUE, SENTINEL = 64, -12345.0, 54321.0
FAMILIES = ["plain", "offset"]
ULP = 2.0 ** -23

# largest distance of the float32 evaluation of the oracle from float64 over every case of the family in this file
RESTATED = {
    "plain": {"raw": 2.07e-7, "norm": 1.11e-6, "spec_mean": 1.48e-8, "spec_std": 8.50e-8, "wav": 3.03e-7,
              "item_y": 5.82e-7, "item_mean": 3.41e-8, "item_std": 4.81e-8},
    # norm: the DC bins are 60 std; wav: worst with the de-normalisation's mean of 3 on every bin and no time branch (the transform
    # cancels it); item_mean: the three rows of two elements, one of them with a std of 0.02 under a mean of 3
    "offset": {"raw": 1.49e-7, "norm": 1.24e-5, "spec_mean": 7.14e-9, "spec_std": 6.10e-8, "wav": 2.88e-6,
               "item_y": 1.59e-6, "item_mean": 1.55e-6, "item_std": 5.77e-8},
}
BOUND = {f: {q: 4 * v for q, v in d.items()} for f, d in RESTATED.items()}
STAT_FLOOR = 2 * ULP

LENGTHS = [1, 2, 1023, 1024, 1025, 1792, 1793, 2304, 2305, 2559, 2560, 4096, 4097, 5000, 12000, 33793]      # B = 2 (STFT), B = S = 2 (iSTFT)
LONG_LENGTHS = [344065, 348160]                                                      # B = S = 1
WALKS = [(512, 5000), (768, 3000)]           # (B, L): launch_stft_frames gives R = 2 in runs of 2, 2, 1 frames / of 2, 1 frames
ISTFT_OPTION_SHAPES = [(1, 1), (2, 2), (3, 3)]                                       # B S = 1, 4, 9
ISTFT_OPTION_LENGTHS = [5000, 12000]
ITEM_COUNTS = [2, 4096, 4097, 135168, 687960, 1048577]


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return _lib.load()


def stream():
    return C.c_void_p(_lib.current_stream_ptr())


def rup(v, m):
    return (v + m - 1) // m * m


def frames(L):
    return -(-L // 1024)


def conv_pitch(T):
    return max(32, rup(T, 4))


def draw(seed, *shape, offset=0.0, scale=1.0):
    gen = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=gen, dtype=torch.float64) * scale + offset).float()


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def expand(v, like):
    """(B,) -> (B, 1, ..., 1) against `like`."""
    return v.reshape(-1, *([1] * (like.dim() - 1)))


class Guarded:
    """A float32 device buffer of `shape` between guard floats.  Output: NaN in the first `valid` columns of each row, the sentinel
    in the pitch columns behind them.  Input (`src`): the values, NaN in the pitch columns."""

    def __init__(self, shape, valid=None, src=None):
        self.shape, self.valid, self.is_input = tuple(shape), shape[-1] if valid is None else valid, src is not None
        n = 1
        for d in shape:
            n *= d
        self.buf = torch.full((n + 2 * GUARD,), GUARD_VALUE, device="cuda")
        self.t = self.buf[GUARD:GUARD + n].view(*shape)
        self.t.fill_(SENTINEL if src is None else NAN)
        self.t[..., :self.valid] = NAN if src is None else src.cuda()

    def ptr(self):
        return self.t.data_ptr()

    def read(self):
        """The valid columns on the CPU, after checking that the guards and an output's pitch columns are as they were."""
        n = self.t.numel()
        assert bool((self.buf[:GUARD] == GUARD_VALUE).all()) and bool((self.buf[GUARD + n:] == GUARD_VALUE).all()), "written outside the buffer"
        if self.valid < self.shape[-1]:
            pad = self.t[..., self.valid:]
            assert bool((torch.isnan(pad) if self.is_input else pad == SENTINEL).all()), "pitch columns were written"
        return self.t[..., :self.valid].cpu()


def report(tag, family, kernel, restated):
    """Print restatement and kernel next to each bound, then assert."""
    parts, bad = [], []
    for q, (dev, floor) in kernel.items():
        bound = max(BOUND[family][q], floor)
        parts.append(f"{q} kernel {dev:.2e} restated {restated.get(q, float('nan')):.2e} bound {bound:.2e}")
        if not dev <= bound:
            bad.append((q, dev, bound))
    print(f"{tag} {family}: " + "; ".join(parts))
    assert not bad, (tag, family, bad)


# ---- STFT -------------------------------------------------------------------------------------------------------------------------
def spec_stats(raw):
    """(mean, unbiased std) over each item of raw (B, 4, 2048, T), in raw's own precision."""
    flat = raw.reshape(raw.shape[0], -1)
    return flat.mean(1), flat.std(1)


def normalise(v, mean, std):
    return (v - expand(mean, v)) / (EPS + expand(std, v))


def stft_deviation(raw, norm, mean, std, ref):
    """Distances from the float64 reference `ref` = (raw, norm, mean, std); None entries are left out."""
    r_raw, r_norm, r_mean, r_std = ref
    out = {}
    if raw is not None:
        out["raw"] = (float((raw.double() - r_raw).abs().max()) / max(1.0, float(r_raw.abs().max())), 0.0)
    if norm is not None:
        out["norm"] = (float((norm.double() - r_norm).abs().max()), 0.0)
    if mean is not None:
        out["spec_mean"] = (float(((mean.double() - r_mean).abs() / r_std).max()), STAT_FLOOR * float((torch.maximum(r_mean.abs(), r_std) / r_std).max()))
        out["spec_std"] = (float((std.double() / r_std - 1.0).abs().max()), STAT_FLOOR)
    return out


_STFT = {}


def stft_case(B, L, family, items=None):
    """float32 mix (B, 2, L); for the items `items` (default: all) the float64 reference (raw, norm, mean, std) and the float32
    restatement's distances from it.  Computed once."""
    key = (B, L, family)
    if key not in _STFT:
        mix = draw(10 * L + B + 5 * FAMILIES.index(family), B, 2, L, offset=8.0 if family == "offset" else 0.0)
        sub = mix if items is None else mix[items]
        raw = O.stft_cac(sub.double())
        mean, std = spec_stats(raw)
        ref = (raw, normalise(raw, mean, std), mean, std)
        raw32 = O.stft_cac(sub)
        m32, s32 = spec_stats(raw32)
        restated = {q: v[0] for q, v in stft_deviation(raw32, normalise(raw32, m32, s32), m32, s32, ref).items()}
        _STFT[key] = (mix, ref, restated)
    return _STFT[key]


def run_stft(lib, mix, pitch, items=None):
    """mi_stft_norm -> (x (B, 4, 2048, T), norm (B, 2), denorm (B, 2)) on the CPU (the items `items` only)."""
    B, _, L = mix.shape
    T = frames(L)
    x, norm, denorm = Guarded((B, 4, 2048, pitch), T), Guarded((B, 2)), Guarded((B, 2))
    mixd = mix.cuda()
    _lib.check(lib.mi_stft_norm(mixd.data_ptr(), B, L, x.ptr(), 0 if pitch == T else pitch, norm.ptr(), denorm.ptr(), stream()), "mi_stft_norm")
    torch.cuda.synchronize()
    assert same_bits(mixd.cpu(), mix), "the input changed"
    got = (x.read(), norm.read(), denorm.read())
    return got if items is None else tuple(t[items] for t in got)


def run_stft_raw(lib, mix, items=None):
    B, _, L = mix.shape
    x = Guarded((B, 4, 2048, frames(L)))
    mixd = mix.cuda()
    _lib.check(lib.mi_stft_cac(mixd.data_ptr(), B, L, x.ptr(), stream()), "mi_stft_cac")
    torch.cuda.synchronize()
    return x.read() if items is None else x.read()[items]


def check_stft(lib, B, L, family, pitches, items=None):
    mix, ref, restated = stft_case(B, L, family, items)
    T = frames(L)
    tag = f"stft B {B} L {L} T {T}"
    raw = run_stft_raw(lib, mix, items)
    assert bool(torch.isfinite(raw).all()), "non-finite spectrogram"
    first = None
    for pitch in pitches:
        x, norm, denorm = run_stft(lib, mix, pitch, items)
        assert bool(torch.isfinite(x).all()) and bool(torch.isfinite(norm).all()) and bool(torch.isfinite(denorm).all())
        mean, std = denorm[:, 0], denorm[:, 1]
        report(f"{tag} pitch {pitch}", family, stft_deviation(raw if first is None else None, x, mean, std, ref), restated)
        # the two pairs are one set of statistics: norm = (mean, 1 / (eps + std)) with the float32 division of finalize_stats
        assert same_bits(norm[:, 0], mean) and same_bits(norm[:, 1], torch.tensor(1.0) / (torch.tensor(EPS) + std))
        # and x is the raw spectrogram under exactly these pairs: one float32 subtraction, one product
        assert same_bits(x, (raw - expand(mean, raw)) * expand(norm[:, 1], raw)), "x is not (raw - mean) * inv of the returned pairs"
        if T <= 32:                                      # one atomic per statistics slot: the same bits whenever it runs
            again = run_stft(lib, mix, pitch, items)
            assert all(same_bits(a, b) for a, b in zip(again, (x, norm, denorm))), "a second call differs"
            if first is not None:
                assert all(same_bits(a, b) for a, b in zip(first, (x, norm, denorm))), "the result depends on the row pitch"
            first = first or (x, norm, denorm)
        else:
            first = first or (x, norm, denorm)


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("L", LENGTHS + LONG_LENGTHS)
def test_stft_norm_matches_float64(lib, L, family):
    """Raw and normalised spectrogram and the per-item (mean, std) at every length of the module docstring, both row pitches."""
    T = frames(L)
    check_stft(lib, 1 if L in LONG_LENGTHS else 2, L, family, [T, conv_pitch(T)] if conv_pitch(T) != T else [T])


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("B,L", WALKS)
def test_stft_walk_of_several_frames_matches_float64(lib, B, L, family):
    """launch_stft_frames gives a workgroup R = ceil(T / runs) frames with runs = min(T, ceil(1536 / B)): at these batch sizes
    R = 2 with a shorter last run, so a workgroup transforms a frame whose samples it fetched under the previous one.  First,
    last and two inner items against float64, statistics included."""
    T = frames(L)
    runs = max(1, min(T, -(-1536 // B)))
    R = -(-T // runs)
    assert R == 2 and T % R == 1, "the shape no longer reaches a walk of two frames with a one-frame last run"
    check_stft(lib, B, L, family, [T], items=[0, 1, B // 2 - 1, B - 1])


# ---- iSTFT ------------------------------------------------------------------------------------------------------------------------
_ISTFT = {}


def istft_case(B, S, L, family):
    """float32 y (B, S, 4, 2048, T), xt (B, S, 2, L), de-normalisation pairs (B, 2) of the spectrogram and of the time branch: every
    item has its own (mean, std)."""
    key = (B, S, L, family)
    if key not in _ISTFT:
        T, off = frames(L), 3.0 if family == "offset" else 0.0
        seed = 20 * L + 7 * B + S + 3 * FAMILIES.index(family)
        y = draw(seed, B, S, 4, 2048, T)
        xt = draw(seed + 1, B, S, 2, L, offset=off)
        p = draw(seed + 2, B, 4)
        dn_f = torch.stack([off + 0.3 * p[:, 0], 0.5 + p[:, 1].abs()], 1).contiguous()
        dn_t = torch.stack([off + 0.3 * p[:, 2], 0.5 + p[:, 3].abs()], 1).contiguous()
        _ISTFT[key] = {"y": y, "xt": xt, "dn_f": dn_f, "dn_t": dn_t, "L": L, "ref": {}}
    return _ISTFT[key]


def istft_eval(case, use_f, use_t, dtype):
    y = case["y"].to(dtype)
    if use_f:
        d = case["dn_f"].to(dtype)
        y = y * expand(d[:, 1], y) + expand(d[:, 0], y)
    w = O.istft_from_cac(y, case["L"])
    if use_t:
        d = case["dn_t"].to(dtype)
        w = w + case["xt"].to(dtype) * expand(d[:, 1], w) + expand(d[:, 0], w)
    return w


def istft_reference(case, use_f, use_t):
    """(float64 waveform (B, S, 2, L), the float32 restatement's distance relative to |want| max); computed once per option set."""
    if (use_f, use_t) not in case["ref"]:
        want = istft_eval(case, use_f, use_t, torch.float64)
        r32 = istft_eval(case, use_f, use_t, torch.float32)
        case["ref"][(use_f, use_t)] = (want, float((r32.double() - want).abs().max() / want.abs().max()))
    return case["ref"][(use_f, use_t)]


def run_istft(lib, case, use_f, use_t, y_pitch, xt_pitch):
    y, xt, L = case["y"], case["xt"], case["L"]
    B, S, _, _, T = y.shape
    yd = Guarded((B, S, 4, 2048, y_pitch), T, src=y)
    xd = Guarded((B, S, 2, xt_pitch), L, src=xt) if use_t else None
    dn_f, dn_t = Guarded((B, 2), src=case["dn_f"]), Guarded((B, 2), src=case["dn_t"])
    wav = Guarded((B, S, 2, L))
    rc = lib.mi_istft_full(yd.ptr(), B, S, L, 0 if y_pitch == T else y_pitch, dn_f.ptr() if use_f else None, xd.ptr() if use_t else None,
                           0 if xt_pitch == L else xt_pitch, dn_t.ptr() if use_t else None, wav.ptr(), stream())
    _lib.check(rc, "mi_istft_full")
    torch.cuda.synchronize()
    assert same_bits(yd.read(), y), "the input changed"
    return wav.read()


def check_istft(lib, B, S, L, family, use_f, use_t, y_pitch, xt_pitch):
    case = istft_case(B, S, L, family)
    want, restated = istft_reference(case, use_f, use_t)
    got = run_istft(lib, case, use_f, use_t, y_pitch, xt_pitch)
    assert bool(torch.isfinite(got).all()), "non-finite (or unwritten) waveform samples"
    dev = float((got.double() - want).abs().max() / want.abs().max())
    report(f"istft B {B} S {S} L {L} denorm_f {int(use_f)} xt {int(use_t)} pitches {y_pitch} {xt_pitch}", family, {"wav": (dev, 0.0)},
           {"wav": restated})
    return got


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("L", LENGTHS + LONG_LENGTHS)
def test_istft_full_matches_float64(lib, L, family):
    """Every length of the module docstring: with de-normalisation, time branch and both pitches rounded up, and with none of them
    (which is also what mi_istft_cac runs: equal bits); a second call returns the same bits; the pitches change no bit."""
    B = S = 1 if L in LONG_LENGTHS else 2
    T = frames(L)
    full = check_istft(lib, B, S, L, family, True, True, conv_pitch(T), rup(L, 4))
    assert same_bits(check_istft(lib, B, S, L, family, True, True, T, L), full), "the result depends on the row pitches"
    bare = check_istft(lib, B, S, L, family, False, False, T, L)
    assert same_bits(run_istft(lib, istft_case(B, S, L, family), False, False, T, L), bare), "a second call differs"
    yd = istft_case(B, S, L, family)["y"].cuda()
    wav = Guarded((B, S, 2, L))
    _lib.check(lib.mi_istft_cac(yd.data_ptr(), B, S, L, wav.ptr(), stream()), "mi_istft_cac")
    torch.cuda.synchronize()
    assert same_bits(wav.read(), bare), "mi_istft_cac differs from mi_istft_full without options"


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("B,S", ISTFT_OPTION_SHAPES)
@pytest.mark.parametrize("L", ISTFT_OPTION_LENGTHS)
def test_istft_options(lib, L, B, S, family):
    """B S = 1, 4 and 9 with each of the four option sets; with B S = 9 the item index bs / S picks another (mean_t, std_t) for each
    batch item.  Spectrogram pitch 32 (T = 5: 4-byte path, T = 12: 16-byte path with a pitch that is not T), xt pitch L and L + 4."""
    T = frames(L)
    for use_f in (False, True):
        for use_t in (False, True):
            check_istft(lib, B, S, L, family, use_f, use_t, conv_pitch(T), L + 4 if use_f else L)


# ---- item normalisation -----------------------------------------------------------------------------------------------------------
_ITEM = {}


def item_case(rows, count, family):
    key = (rows, count, family)
    if key not in _ITEM:
        x = draw(30 * count + rows + 11 * FAMILIES.index(family), rows, count, offset=3.0 if family == "offset" else 0.0)
        x64 = x.double()
        mean, std = x64.mean(1), x64.std(1)
        ref = (normalise(x64, mean, std), mean, std)
        m32, s32 = x.mean(1), x.std(1)
        restated = {q: v[0] for q, v in item_deviation(normalise(x, m32, s32), m32, s32, ref).items()}
        _ITEM[key] = (x, ref, restated)
    return _ITEM[key]


def item_deviation(y, mean, std, ref):
    r_y, r_mean, r_std = ref
    return {"item_y": (float((y.double() - r_y).abs().max()), 0.0),
            "item_mean": (float(((mean.double() - r_mean).abs() / r_std).max()), STAT_FLOOR * float((torch.maximum(r_mean.abs(), r_std) / r_std).max())),
            "item_std": (float((std.double() / r_std - 1.0).abs().max()), STAT_FLOOR)}


def run_item_norm(lib, x):
    rows, count = x.shape
    y, norm, denorm = Guarded((rows, count)), Guarded((rows, 2)), Guarded((rows, 2))
    xd = x.cuda()
    _lib.check(lib.mi_item_norm(xd.data_ptr(), rows, count, y.ptr(), norm.ptr(), denorm.ptr(), stream()), "mi_item_norm")
    torch.cuda.synchronize()
    assert same_bits(xd.cpu(), x), "the input changed"
    return y.read(), norm.read(), denorm.read()


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("rows", [1, 3])
@pytest.mark.parametrize("count", ITEM_COUNTS)
def test_item_norm_matches_float64(lib, count, rows, family):
    """count 2 (a one-sample stereo chunk), 4 096 / 4 097 (one workgroup with float64 squares / two with float32 partial squares),
    135 168 (33 workgroups on 32 slots), 687 960 (the engine's two channels of a segment), 1 048 577 (the grid's cap of 256
    workgroups, whose loop takes a second step)."""
    x, ref, restated = item_case(rows, count, family)
    y, norm, denorm = run_item_norm(lib, x)
    assert bool(torch.isfinite(y).all()) and bool(torch.isfinite(norm).all()) and bool(torch.isfinite(denorm).all())
    mean, std = denorm[:, 0], denorm[:, 1]
    report(f"item_norm rows {rows} count {count}", family, item_deviation(y, mean, std, ref), restated)
    assert same_bits(norm[:, 0], mean) and same_bits(norm[:, 1], torch.tensor(1.0) / (torch.tensor(EPS) + std))
    assert same_bits(y, (x - expand(mean, x)) * expand(norm[:, 1], x)), "y is not (x - mean) * inv of the returned pairs"
    if count <= 32 * 4096:                               # one atomic per statistics slot
        assert all(same_bits(a, b) for a, b in zip(run_item_norm(lib, x), (y, norm, denorm))), "a second call differs"


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("rows", [1, 3])
@pytest.mark.parametrize("count", ITEM_COUNTS)
def test_item_denorm_matches_float64(lib, count, rows, family):
    """y = x * std + mean with each row's own pair: a float32 product and a float32 sum, |y - y64| <= 2^-24 (|x std| + |y|)."""
    x = item_case(rows, count, family)[0]
    p = draw(count + rows, rows, 2)
    dn = torch.stack([(3.0 if family == "offset" else 0.0) + p[:, 0], 0.5 + p[:, 1].abs()], 1).contiguous()
    y, dnd, xd = Guarded((rows, count)), Guarded((rows, 2), src=dn), x.cuda()
    _lib.check(lib.mi_item_denorm(xd.data_ptr(), rows, count, dnd.ptr(), y.ptr(), stream()), "mi_item_denorm")
    torch.cuda.synchronize()
    got = y.read()
    prod = x.double() * expand(dn[:, 1].double(), x)
    want = prod + expand(dn[:, 0].double(), x)
    tol = 2.0 ** -24 * (prod.abs() + want.abs()) * (1 + 1e-6) + 1e-30
    d = (got.double() - want).abs()
    print(f"item_denorm rows {rows} count {count} {family}: max-abs vs float64 {float(d.max()):.2e}, largest share of its bound {float((d / tol).max()):.2f}")
    assert bool(torch.isfinite(got).all()) and bool((d <= tol).all())


# ---- properties beyond parity -----------------------------------------------------------------------------------------------------
def test_nan_item_changes_no_other_item(lib):
    """B = 3 with item 1 all NaN (waveform, spectrogram, time branch and its pairs), T = 5: items 0 and 2 have the bits of their
    own B = 1 runs -- x, the (mean, 1 / (eps + std)) and (mean, std) pairs, the waveform, the item norm's rows."""
    L, T = 5000, 5
    mix = stft_case(3, L, "offset")[0].clone()
    mix[1] = NAN
    x, norm, denorm = run_stft(lib, mix, 32)
    assert bool(torch.isnan(x[1]).all()) and bool(torch.isnan(denorm[1]).all())
    for b in (0, 2):
        alone = run_stft(lib, mix[b:b + 1].contiguous(), 32)
        assert all(same_bits(a[0], t[b]) for a, t in zip(alone, (x, norm, denorm))), f"STFT item {b} differs from its own run"

    case = {k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in istft_case(3, 2, L, "offset").items()}
    for k in ("y", "xt", "dn_f", "dn_t"):
        case[k][1] = NAN
    wav = run_istft(lib, case, True, True, 32, rup(L, 4))
    assert bool(torch.isnan(wav[1]).all())
    for b in (0, 2):
        one = {k: (v[b:b + 1].contiguous() if isinstance(v, torch.Tensor) else v) for k, v in case.items()}
        assert same_bits(run_istft(lib, one, True, True, 32, rup(L, 4))[0], wav[b]), f"iSTFT item {b} differs from its own run"

    rows = item_case(3, 4097, "offset")[0].clone()
    rows[1] = NAN
    got = run_item_norm(lib, rows)
    for b in (0, 2):
        alone = run_item_norm(lib, rows[b:b + 1].contiguous())
        assert all(same_bits(a[0], t[b]) for a, t in zip(alone, got)), f"item-norm row {b} differs from its own run"


def test_entries_refuse_bad_arguments(lib):
    """Every refusal returns non-zero before anything is launched: the outputs keep their fill."""
    B, S, L, T = 2, 2, 3000, 3
    mix = torch.zeros(B, 2, L, device="cuda")
    y = torch.zeros(B, S, 4, 2048, 32, device="cuda")
    xt = torch.zeros(B, S, 2, L + 4, device="cuda")
    pairs = torch.ones(B * S, 2, device="cuda")
    out = torch.full((B * S * 4 * 2048 * 32,), GUARD_VALUE, device="cuda")
    o2, o3 = torch.full((64,), GUARD_VALUE, device="cuda"), torch.full((64,), GUARD_VALUE, device="cuda")
    m, yp, xp, pp, op, o2p, o3p = (t.data_ptr() for t in (mix, y, xt, pairs, out, o2, o3))
    st = stream()
    ok = [lib.mi_stft_norm(m, B, L, op, 32, o2p, o3p, st), lib.mi_stft_cac(m, B, L, op, st),
          lib.mi_istft_full(yp, B, S, L, 32, pp, xp, L + 4, pp, op, st), lib.mi_istft_cac(yp, B, S, L, op, st),
          lib.mi_item_norm(m, B, 2 * L, op, o2p, o3p, st), lib.mi_item_denorm(m, B, 2 * L, pp, op, st)]
    torch.cuda.synchronize()
    assert ok == [0] * 6, ok                                     # the refusals below are not an accident of these calls' form
    for t in (out, o2, o3):
        t.fill_(GUARD_VALUE)
    refused = {
        "stft mix null": lib.mi_stft_norm(None, B, L, op, 32, o2p, o3p, st), "stft x null": lib.mi_stft_norm(m, B, L, None, 32, o2p, o3p, st),
        "stft norm null": lib.mi_stft_norm(m, B, L, op, 32, None, o3p, st), "stft denorm null": lib.mi_stft_norm(m, B, L, op, 32, o2p, None, st),
        "stft B 0": lib.mi_stft_norm(m, 0, L, op, 32, o2p, o3p, st), "stft B -1": lib.mi_stft_norm(m, -1, L, op, 32, o2p, o3p, st),
        "stft L 0": lib.mi_stft_norm(m, B, 0, op, 32, o2p, o3p, st), "stft L -5": lib.mi_stft_norm(m, B, -5, op, 32, o2p, o3p, st),
        "stft pitch 2 < T": lib.mi_stft_norm(m, B, L, op, T - 1, o2p, o3p, st), "stft pitch -4": lib.mi_stft_norm(m, B, L, op, -4, o2p, o3p, st),
        "stft_cac L 0": lib.mi_stft_cac(m, B, 0, op, st), "stft_cac B 0": lib.mi_stft_cac(m, 0, L, op, st),
        "stft_cac null": lib.mi_stft_cac(m, B, L, None, st),
        "istft y null": lib.mi_istft_full(None, B, S, L, 32, pp, xp, L + 4, pp, op, st),
        "istft wav null": lib.mi_istft_full(yp, B, S, L, 32, pp, xp, L + 4, pp, None, st),
        "istft B 0": lib.mi_istft_full(yp, 0, S, L, 32, pp, xp, L + 4, pp, op, st),
        "istft S 0": lib.mi_istft_full(yp, B, 0, L, 32, pp, xp, L + 4, pp, op, st),
        "istft L 0": lib.mi_istft_full(yp, B, S, 0, 32, pp, xp, L + 4, pp, op, st),
        "istft y pitch 2 < T": lib.mi_istft_full(yp, B, S, L, T - 1, pp, xp, L + 4, pp, op, st),
        "istft xt pitch < L": lib.mi_istft_full(yp, B, S, L, 32, pp, xp, L - 1, pp, op, st),
        "istft xt without denorm_t": lib.mi_istft_full(yp, B, S, L, 32, pp, xp, L + 4, None, op, st),
        "istft denorm_t without xt": lib.mi_istft_full(yp, B, S, L, 32, pp, None, L + 4, pp, op, st),
        "istft_cac L 0": lib.mi_istft_cac(yp, B, S, 0, op, st), "istft_cac null": lib.mi_istft_cac(None, B, S, L, op, st),
        "item_norm x null": lib.mi_item_norm(None, B, 2 * L, op, o2p, o3p, st), "item_norm y null": lib.mi_item_norm(m, B, 2 * L, None, o2p, o3p, st),
        "item_norm norm null": lib.mi_item_norm(m, B, 2 * L, op, None, o3p, st), "item_norm denorm null": lib.mi_item_norm(m, B, 2 * L, op, o2p, None, st),
        "item_norm rows 0": lib.mi_item_norm(m, 0, 2 * L, op, o2p, o3p, st), "item_norm rows 65536": lib.mi_item_norm(m, 65536, 2, op, o2p, o3p, st),
        "item_norm count 1": lib.mi_item_norm(m, B, 1, op, o2p, o3p, st), "item_norm count 0": lib.mi_item_norm(m, B, 0, op, o2p, o3p, st),
        "item_denorm x null": lib.mi_item_denorm(None, B, 2 * L, pp, op, st), "item_denorm pairs null": lib.mi_item_denorm(m, B, 2 * L, None, op, st),
        "item_denorm y null": lib.mi_item_denorm(m, B, 2 * L, pp, None, st), "item_denorm rows 0": lib.mi_item_denorm(m, 0, 2 * L, pp, op, st),
        "item_denorm count 0": lib.mi_item_denorm(m, B, 0, pp, op, st),
    }
    torch.cuda.synchronize()
    assert all(rc != 0 for rc in refused.values()), [k for k, rc in refused.items() if rc == 0]
    assert all(bool((t == GUARD_VALUE).all()) for t in (out, o2, o3)), "a refused call wrote to an output"
    assert b"mi_item_denorm" in lib.mi_last_error()
