"""The fused DConv kernels alone, through the C ABI, against float64: dconv_row.hip (`mi_dconv_row`: both residual layers of the
frequency branch on one (batch, bin) row per wave, and the LDS-resident variant) and dconv_time.hip (`mi_dconv_time_layer`: one
residual layer of the time branch in three streaming passes, the second GroupNorm's statistics from a Gram matrix in self-cleaning
float64 slot buffers).  The entries pack the checkpoint's natural-layout tensors with the function EngineCore::load_dconv uses.

Reference: torch on the CPU in float64 of demucs/demucs.py:133-154,
    conv1d(dilation d, padding d) -> GroupNorm(1) -> GELU -> 1x1 -> GroupNorm(1) -> GLU -> LayerScale -> + x,
for the row entry applied twice (d = 1, then d = 2) to the rows permuted out of (B, C, Fr, T).

Inputs are drawn in float64 from seeded generators and rounded to float32 once; x = N(0, 1).  Two families of weights:
    plain    the distributions of test_gpu_kernels.py::test_dconv_layer_three_passes
    offset   W0 scale 0.05, b0 = 3 + 0.3 N, b3 = 3 + N: mean^2 / var of the hidden tensor is about 20 and that of the 1x1's output
             about 9 -- the float32 partial sums in front of the float64 subtractions of the one-pass variances
Outputs start as NaN between guard floats; the time entry's pitch columns of x and its whole hidden buffer start as NaN.

Tolerances.  None is taken from the kernels.  `dconv_layer(..., torch.float32)` is the reference's own arithmetic in float32 on the
CPU; its largest max-abs distance from float64 over every case of a family in this file (measured with 256 compute units for the
persistent-loop shapes) is RESTATED_*, and the kernels get 4x that (the precedent of test_gpu_token_norm.py: another summation order,
and the hardware exp2 / rcp of the row kernel's sigmoid).  The time entry's (mean, rstd) outputs get 4x the deviation of torch's
float32 var_mean on the float32 hidden / 1x1 tensors: mean absolute, rstd relative.  Every case prints the restatement's and the
kernel's deviation next to the bound.

The restatement's own figures depend on the host (torch picks its float32 conv and reduction code by CPU and thread count: the
single-row T = 330 offset case has been seen at 3.2e-6 and at 7.6e-6), so they are printed, not asserted; the constants are the
smaller set (the stricter bounds).  DESIGN.md (kernel-level
parity) records what these cases changed in the kernels."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from demucs_amd import _lib

pytestmark = pytest.mark.gpu
NAN = float("nan")
EPS = 1e-5
GUARD, GUARD_VALUE = 64, -12345.0
FAMILIES = ["plain", "offset"]
SLOTS, GRAM_MAX = 32, 96                    # csrc/common.h kStatSlots, csrc/dconv_time.hip kGramMax

# largest max-abs distance of the float32 restatement from float64 over the family's cases: y of the row entry, y of the time entry
RESTATED_ROW = {"plain": 4.3e-6, "offset": 3.9e-6}         # |y| up to 12; worst at C = 96, T = 384 and at the 259-row T = 336 case
RESTATED_TIME = {"plain": 4.2e-6, "offset": 4.0e-6}        # worst at C = 96, Lv = 21 499
# the same for the statistics: {family: ((mean abs, rstd rel) of the first GroupNorm, (mean abs, rstd rel) of the second)}
RESTATED_STATS = {"plain": ((1.7e-7, 8.7e-8), (3.9e-8, 9.7e-8)), "offset": ((1.3e-7, 2.7e-7), (1.6e-7, 3.5e-7))}
ROW_BOUND = {f: 4 * v for f, v in RESTATED_ROW.items()}
TIME_BOUND = {f: 4 * v for f, v in RESTATED_TIME.items()}
STAT_BOUND = {f: tuple((4 * m, 4 * r) for m, r in v) for f, v in RESTATED_STATS.items()}

ROW_KERNELS = {"c48-wave": (48, 0), "c48-lds": (48, 1), "c96-wave": (96, 0)}
ROW_T = [6, 12, 330, 336, 378, 384]          # one lane, two, the engine's 56 and its neighbour, 63 lanes, the full wave
ROW_SHAPES = [(1, 1), (1, 5), (3, 3)]        # 1, 5, 9 rows: partly filled 4- and 8-row workgroups
# rows(compute units) and T of the shapes at which a wave (a workgroup of the LDS kernel) walks to a second row
ROW_PERSISTENT = {"c48-wave": ("c48-wave", lambda cus: 12 * cus + 3, 12), "c96-wave": ("c96-wave", lambda cus: 8 * cus + 5, 12),
                  "c48-lds": ("c48-lds", lambda cus: cus + 3, 12), "c48-lds-T336": ("c48-lds", lambda cus: cus + 3, 336)}
TIME_LV = [1, 5, 6, 7, 1535, 1536, 1537, 21499]      # a workgroup covers 1536 columns, a lane 6
TIME_PITCHES = [(6, 6), (1538, 1538), (6, 16), (1536, 1546)]     # (Lv, Lp): Lp = Lv and Lp = Lv + 10 (the engine rounds Lv up to 4)
TIME_WRAP_LV = 49159                         # 33 workgroups per item: the 33rd shares slot 0 with the first


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return _lib.load()


def stream():
    return C.c_void_p(_lib.current_stream_ptr())


def rup(v, m):
    return (v + m - 1) // m * m


def noise(gen, *shape):
    return torch.randn(*shape, generator=gen, dtype=torch.float64)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


_WEIGHTS = {}


def layer_weights(Cn, family, layer):
    """The nine float32 tensors of one DConv layer in the checkpoint's layout and the entries' order."""
    key = (Cn, family, layer)
    if key not in _WEIGHTS:
        gen = torch.Generator().manual_seed(7000 + 100 * Cn + 10 * FAMILIES.index(family) + layer)
        h = Cn // 8
        W0, b0 = noise(gen, h, Cn, 3) * 0.2, noise(gen, h)
        g1w, g1b = 1 + 0.2 * noise(gen, h), 0.1 * noise(gen, h)
        W3, b3 = noise(gen, 2 * Cn, h, 1) * 0.5, noise(gen, 2 * Cn)
        g2w, g2b = 1 + 0.2 * noise(gen, 2 * Cn), 0.1 * noise(gen, 2 * Cn)
        ls = 1 + 0.3 * noise(gen, Cn)
        if family == "offset":
            W0, b0, b3 = W0 * 0.25, 3 + 0.3 * b0, 3 + b3
        _WEIGHTS[key] = tuple(t.float() for t in (W0, b0, g1w, g1b, W3, b3, g2w, g2b, ls))
    return _WEIGHTS[key]


def flat(*layers):
    """weights_host of the entries: every tensor of every layer, concatenated."""
    return np.ascontiguousarray(torch.cat([t.reshape(-1) for w in layers for t in w]).numpy())


def dconv_layer(x, w, dil, dtype):
    """One DConv residual layer on rows x (N, C, L) in `dtype` -> (y, hidden tensor before its GroupNorm, 1x1 output before its)."""
    W0, b0, g1w, g1b, W3, b3, g2w, g2b, ls = (t.to(dtype) for t in w)
    h = F.conv1d(x, W0, b0, dilation=dil, padding=dil)
    z = F.conv1d(F.gelu(F.group_norm(h, 1, g1w, g1b, eps=EPS)), W3, b3)
    return x + ls[:, None] * F.glu(F.group_norm(z, 1, g2w, g2b, eps=EPS), dim=1), h, z


def row_stats(t):
    """(mean, 1 / sqrt(biased variance + eps)) over everything but the first axis, in t's own precision (torch's var_mean)."""
    var, mean = torch.var_mean(t.reshape(t.shape[0], -1), dim=1, unbiased=False)
    return torch.stack([mean, 1.0 / torch.sqrt(var + EPS)], 1)


def stat_deviation(got, want):
    """(max |mean - mean64|, max |rstd / rstd64 - 1|) of (N, 2) statistics."""
    got, want = got.double(), want.double()
    return float((got[:, 0] - want[:, 0]).abs().max()), float((got[:, 1] / want[:, 1] - 1.0).abs().max())


# ---- the row kernels -------------------------------------------------------------------------------------------------------------
_ROW_REF = {}


def row_case(Cn, B, Fr, T, family):
    """float32 x (B, C, Fr, T), weights_host, the float64 expectation and the float32 restatement's distance from it; computed once."""
    key = (Cn, B, Fr, T, family)
    if key not in _ROW_REF:
        gen = torch.Generator().manual_seed(100000 * FAMILIES.index(family) + 1000 * Cn + 7 * T + B * Fr)
        x = noise(gen, B, Cn, Fr, T).float()
        w = [layer_weights(Cn, family, d) for d in (0, 1)]

        def both(dtype):
            rows = x.to(dtype).permute(0, 2, 1, 3).reshape(B * Fr, Cn, T)
            for d in (0, 1):
                rows = dconv_layer(rows, w[d], 1 << d, dtype)[0]
            return rows.view(B, Fr, Cn, T).permute(0, 2, 1, 3)
        want = both(torch.float64)
        _ROW_REF[key] = (x, flat(*w), want, float((both(torch.float32).double() - want).abs().max()))
    return _ROW_REF[key]


def run_row(lib, x, wflat, variant, alias=False):
    """x (B, C, Fr, T) float32 on the host -> the entry's y; y lies between guard floats, starts as NaN (or, aliased, as x)."""
    B, Cn, Fr, T = x.shape
    n = x.numel()
    buf = torch.full((n + 2 * GUARD,), GUARD_VALUE, device="cuda")
    y = buf[GUARD:GUARD + n]
    if alias:
        y.copy_(x.reshape(-1))
        xd = y
    else:
        y.fill_(NAN)
        xd = x.reshape(-1).cuda()
    _lib.check(lib.mi_dconv_row(xd.data_ptr(), y.data_ptr(), B, Cn, Fr, T, wflat.ctypes.data, variant, stream()), "mi_dconv_row")
    torch.cuda.synchronize()
    out = buf.cpu()
    assert bool((out[:GUARD] == GUARD_VALUE).all()) and bool((out[GUARD + n:] == GUARD_VALUE).all()), "written outside y"
    if not alias:
        assert same_bits(xd.cpu(), x.reshape(-1)), "x changed although y is another buffer"
    return out[GUARD:GUARD + n].view(B, Cn, Fr, T)


def check_row(lib, kernel, B, Fr, T, family):
    Cn, variant = ROW_KERNELS[kernel]
    x, wflat, want, restated = row_case(Cn, B, Fr, T, family)
    got = run_row(lib, x, wflat, variant)
    assert bool(torch.isfinite(got).all()), "non-finite output"
    err = float((got.double() - want).abs().max())
    print(f"dconv_row {kernel} rows {B} x {Fr} T {T} {family}: max-abs vs float64 {err:.2e} (float32 restatement {restated:.2e}, "
          f"bound {ROW_BOUND[family]:.2e}, largest |y| {float(want.abs().max()):.1f})")
    assert same_bits(run_row(lib, x, wflat, variant, alias=True), got), "y == x gives another result than separate buffers"
    assert err <= ROW_BOUND[family]
    return x, wflat, got


def poison_row(x, row):
    """A copy of x (B, C, Fr, T) with NaN in every element of row `row` = b * Fr + fr."""
    xp = x.clone()
    xp[row // x.shape[2], :, row % x.shape[2], :] = NAN
    return xp


def check_row_isolation(lib, kernel, x, wflat, clean, row):
    """NaN in every element of one row: every other row keeps its bits."""
    got = run_row(lib, poison_row(x, row), wflat, ROW_KERNELS[kernel][1])
    B, Cn, Fr, T = x.shape
    keep = torch.ones(B * Fr, dtype=torch.bool)
    keep[row] = False
    a, b = (t.permute(0, 2, 1, 3).reshape(B * Fr, Cn, T)[keep] for t in (got, clean))
    bad = (a.view(torch.int32) != b.view(torch.int32)).any(2).any(1)
    assert not bool(bad.any()), f"NaN in row {row} changed rows {torch.nonzero(keep).flatten()[bad].tolist()[:8]}"


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("T", ROW_T)
@pytest.mark.parametrize("kernel", list(ROW_KERNELS))
def test_row_matches_float64(lib, kernel, T, family):
    """Row ends at 1, 2, 55, 56, 63 and 64 lanes (the conv's zero padding comes from DPP wave shifts: lanes past the row must hold
    zeros, and at T = 384 the shift's bound control supplies the zero) in 1, 5 and 9 rows; separate and aliased buffers agree bit
    for bit; guards around y and, with separate buffers, x itself are untouched."""
    for B, Fr in ROW_SHAPES:
        check_row(lib, kernel, B, Fr, T, family)


def split_rows(rows):
    B = next((d for d in (7, 5, 3, 2) if rows % d == 0), 1)
    return B, rows // B


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("case", list(ROW_PERSISTENT))
def test_row_persistent_loop_second_step(lib, case, family):
    """More rows than one sweep of the grid holds (3 CUs workgroups of 4 waves at C = 48, CUs of 8 at C = 96, CUs workgroups of the
    LDS kernel, which fetches row r + grid under the arithmetic of row r): the rows of the second step match float64, and NaN in
    one of THEM changes no other row -- not those of the same wave's or workgroup's first step either."""
    kernel, rows_of, T = ROW_PERSISTENT[case]
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    rows = rows_of(cus)
    B, Fr = split_rows(rows)
    x, wflat, got = check_row(lib, kernel, B, Fr, T, family)
    check_row_isolation(lib, kernel, x, wflat, got, rows - 2)         # the middle one of the (at least three) second-step rows


@pytest.mark.parametrize("T", [12, 336, 384])
@pytest.mark.parametrize("kernel", list(ROW_KERNELS))
def test_row_nan_stays_in_its_row(lib, kernel, T):
    """NaN in row 5 of 9 (the second wave of the second 4-row workgroup, the sixth wave of the 8-row one): the other eight rows
    keep their bits."""
    Cn, variant = ROW_KERNELS[kernel]
    x, wflat, _, _ = row_case(Cn, 3, 3, T, "plain")
    check_row_isolation(lib, kernel, x, wflat, run_row(lib, x, wflat, variant), 5)


@pytest.mark.parametrize("T", [12, 336])
@pytest.mark.parametrize("kernel", list(ROW_KERNELS))
def test_row_result_does_not_depend_on_its_place(lib, kernel, T):
    """A row computed alone (row 0 of a one-row call) and at another index of a nine-row call: the same bits; so are two identical
    calls."""
    Cn, variant = ROW_KERNELS[kernel]
    x, wflat, _, _ = row_case(Cn, 3, 3, T, "offset")
    full = run_row(lib, x, wflat, variant)
    assert same_bits(run_row(lib, x, wflat, variant), full), "two identical calls differ"
    for b, fr in ((0, 0), (1, 1), (2, 2)):
        alone = run_row(lib, x[b:b + 1, :, fr:fr + 1, :].contiguous(), wflat, variant)
        assert same_bits(alone[0, :, 0, :], full[b, :, fr, :]), f"row ({b}, {fr}) alone differs from the same row inside the batch"


def test_row_entry_refuses_what_the_kernels_cannot_take(lib):
    """Each refusal returns non-zero before anything is launched: y keeps its fill."""
    B, Cn, Fr, T = 1, 48, 2, 12
    x = torch.zeros(B * 96 * Fr * 400 + 2, device="cuda")
    y = torch.full_like(x, GUARD_VALUE)
    w = flat(layer_weights(96, "plain", 0), layer_weights(96, "plain", 1))

    def call(xp=None, yp=None, B=B, Cn=Cn, Fr=Fr, T=T, wp=w.ctypes.data, variant=0):
        return lib.mi_dconv_row(x.data_ptr() if xp is None else xp, y.data_ptr() if yp is None else yp, B, Cn, Fr, T, wp, variant, stream())
    assert call() == 0                                           # the refusals below are not an accident of this call's form
    torch.cuda.synchronize()
    y.fill_(GUARD_VALUE)
    refused = {
        "C = 64": call(Cn=64), "C = 24": call(Cn=24), "T = 10": call(T=10), "T = 9": call(T=9), "T = 390": call(T=390), "T = 0": call(T=0),
        # the LDS kernel's own T limit (kRowLdsT = 384) coincides with the general one today: T = 390 is refused by the general check
        "LDS kernel, C = 96": call(Cn=96, variant=1), "LDS kernel, T = 390": call(T=390, variant=1), "variant 2": call(variant=2),
        "variant -1": call(variant=-1), "x misaligned": call(xp=x.data_ptr() + 4), "y misaligned": call(yp=y.data_ptr() + 4),
        "x null": call(xp=0), "y null": call(yp=0), "weights null": call(wp=None), "B = 0": call(B=0), "Fr = 0": call(Fr=0),
        "y overlaps x": call(yp=x.data_ptr() + 8),
    }
    torch.cuda.synchronize()
    assert all(rc != 0 for rc in refused.values()), [k for k, rc in refused.items() if rc == 0]
    assert bool((y == GUARD_VALUE).all()), "a refused call wrote to y"
    assert b"mi_dconv_row" in lib.mi_last_error()


# ---- the time kernels ------------------------------------------------------------------------------------------------------------
def time_case(Cn, dil, family, Lv, B):
    """float32 x (B, C, Lv), weights_host, float64 y / first / second statistics, and the float32 restatement's deviations."""
    gen = torch.Generator().manual_seed(200000 * FAMILIES.index(family) + 1000 * Cn + Lv)
    x = noise(gen, B, Cn, Lv).float()
    w = layer_weights(Cn, family, dil - 1)
    y64, h64, z64 = dconv_layer(x.double(), w, dil, torch.float64)
    y32, h32, z32 = dconv_layer(x, w, dil, torch.float32)
    st = (row_stats(h64), row_stats(z64))
    restated = (float((y32.double() - y64).abs().max()), stat_deviation(row_stats(h32), st[0]), stat_deviation(row_stats(z32), st[1]))
    return x, flat(w), y64, st, restated


def guarded(n, fill, dtype=torch.float32):
    buf = torch.full((n + 2 * GUARD,), GUARD_VALUE, dtype=dtype, device="cuda")
    buf[GUARD:GUARD + n] = fill
    return buf


def guards_intact(buf):
    h = buf.cpu()
    return bool((h[:GUARD] == GUARD_VALUE).all()) and bool((h[-GUARD:] == GUARD_VALUE).all())


def run_time(lib, x, wflat, dil, Lp, ws=None):
    """x (B, C, Lv) float32 on the host -> (y (B, C, Lv), st (2B, 2), workspace).  Pitch columns of x are NaN; a fresh workspace
    has NaN in the whole hidden buffer and zeros in the slot buffers."""
    B, Cn, Lv = x.shape
    HA = rup(Cn // 8, 4)
    xd = torch.full((B, Cn, Lp), NAN)
    xd[..., :Lv] = x
    xd = xd.cuda()
    if ws is None:
        ws = dict(hbuf=guarded(B * HA * Lp, NAN), stats=torch.zeros(B * SLOTS * 2, dtype=torch.float64, device="cuda"),
                  gram=torch.zeros(B * SLOTS * GRAM_MAX, dtype=torch.float64, device="cuda"))
    ybuf = guarded(B * Cn * Lp, NAN)
    st = torch.full((2 * B, 2), NAN, device="cuda")
    _lib.check(lib.mi_dconv_time_layer(xd.data_ptr(), ybuf[GUARD:].data_ptr(), B, Cn, Lv, Lp, dil, wflat.ctypes.data, ws["hbuf"][GUARD:].data_ptr(),
                                       ws["stats"].data_ptr(), ws["gram"].data_ptr(), st.data_ptr(), stream()), "mi_dconv_time_layer")
    torch.cuda.synchronize()
    assert guards_intact(ybuf), "written outside y"
    assert guards_intact(ws["hbuf"]), "written outside the hidden buffer"
    assert float(ws["stats"].abs().max()) == 0.0 and float(ws["gram"].abs().max()) == 0.0, "slot buffers not zero again after the call"
    assert same_bits(xd[..., :Lv].cpu(), x), "x changed"
    return ybuf[GUARD:GUARD + B * Cn * Lp].view(B, Cn, Lp)[..., :Lv].cpu(), st.cpu(), ws


def check_time(lib, Cn, dil, family, Lv, Lp, B):
    x, wflat, want, st64, restated = time_case(Cn, dil, family, Lv, B)
    y, st, ws = run_time(lib, x, wflat, dil, Lp)
    assert bool(torch.isfinite(y).all()) and bool(torch.isfinite(st).all()), "non-finite output: a pitch column or stale hidden value was used"
    err = float((y.double() - want).abs().max())
    d1, d2 = stat_deviation(st[:B], st64[0]), stat_deviation(st[B:], st64[1])
    b1, b2 = STAT_BOUND[family]
    tag = f"dconv_time C {Cn} dil {dil} {family} Lv {Lv} Lp {Lp} B {B}"
    print(f"{tag}: y max-abs vs float64 {err:.2e} (float32 restatement {restated[0]:.2e}, bound {TIME_BOUND[family]:.2e}, largest |y| "
          f"{float(want.abs().max()):.1f})")
    print(f"{tag}: (mean abs, rstd rel) first GroupNorm ({d1[0]:.2e}, {d1[1]:.2e}), restatement ({restated[1][0]:.2e}, {restated[1][1]:.2e}), "
          f"bound ({b1[0]:.2e}, {b1[1]:.2e}); second ({d2[0]:.2e}, {d2[1]:.2e}), restatement ({restated[2][0]:.2e}, {restated[2][1]:.2e}), "
          f"bound ({b2[0]:.2e}, {b2[1]:.2e})")
    y2, st2, _ = run_time(lib, x, wflat, dil, Lp, ws)           # the same workspace again: the hidden buffer now holds the first call's values
    assert same_bits(y2, y) and same_bits(st2, st), "a second call on the same workspace differs"
    assert d1[0] <= b1[0] and d1[1] <= b1[1], ("first GroupNorm's statistics", d1, b1)
    assert d2[0] <= b2[0] and d2[1] <= b2[1], ("second GroupNorm's statistics", d2, b2)
    assert err <= TIME_BOUND[family]
    return x, wflat, y, st


@pytest.mark.parametrize("Lv", TIME_LV)
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("dil", [1, 2])
@pytest.mark.parametrize("Cn", [48, 96])
def test_time_layer_matches_float64(lib, Cn, dil, family, Lv):
    """One column, fewer than a lane's six, six, seven, odd lengths (float2 loads straddle Lv), one column either side of the
    1 536-column workgroup, a level-2 length; Lp = Lv rounded up to 4 as the engine does, NaN in the pitch columns and the hidden
    buffer.  A batch of 3, then item 1 of it alone: y and both statistics of that item keep their bits."""
    Lp = rup(Lv, 4)
    x, wflat, y, st = check_time(lib, Cn, dil, family, Lv, Lp, 3)
    y1, st1, _ = run_time(lib, x[1:2].contiguous(), wflat, dil, Lp)
    assert same_bits(y1[0], y[1]) and same_bits(st1, st[[1, 4]]), "item 1 alone differs from item 1 of the batch"


@pytest.mark.parametrize("Lv,Lp", TIME_PITCHES)
@pytest.mark.parametrize("dil", [1, 2])
@pytest.mark.parametrize("Cn", [48, 96])
def test_time_layer_other_pitches(lib, Cn, dil, Lv, Lp):
    """No pitch columns at all (Lp = Lv, not a multiple of 4) and ten of them, all NaN."""
    check_time(lib, Cn, dil, "plain", Lv, Lp, 1)
    check_time(lib, Cn, dil, "plain", Lv, Lp, 3)


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("Cn", [48, 96])
def test_time_layer_slot_wrap(lib, Cn, family):
    """33 workgroups per item: the last one adds its sums to the slot the first one used (blockIdx.x % 32)."""
    check_time(lib, Cn, 2, family, TIME_WRAP_LV, rup(TIME_WRAP_LV, 4), 1)


def test_time_entry_refuses_what_the_kernels_cannot_take(lib):
    """Each refusal returns non-zero before anything is launched: y, the statistics and the slot buffers keep their fill."""
    B, Cn, Lv, Lp = 1, 48, 10, 12
    x = torch.zeros(2 * 96 * 16 + 2, device="cuda")
    y = torch.full_like(x, GUARD_VALUE)
    hbuf = torch.zeros(2 * 12 * 16 + 2, device="cuda")
    stats = torch.zeros(2 * SLOTS * 2 + 1, dtype=torch.float64, device="cuda")
    gram = torch.zeros(2 * SLOTS * GRAM_MAX + 1, dtype=torch.float64, device="cuda")
    st = torch.full((8,), GUARD_VALUE, device="cuda")
    w = flat(layer_weights(96, "plain", 0))
    ptrs = dict(x=x.data_ptr(), y=y.data_ptr(), w=w.ctypes.data, hbuf=hbuf.data_ptr(), stats=stats.data_ptr(), gram=gram.data_ptr(),
                st=st.data_ptr())

    def call(B=B, Cn=Cn, Lv=Lv, Lp=Lp, dil=1, **other):
        p = dict(ptrs, **other)
        return lib.mi_dconv_time_layer(p["x"], p["y"], B, Cn, Lv, Lp, dil, p["w"], p["hbuf"], p["stats"], p["gram"], p["st"], stream())
    assert call() == 0                                           # the refusals below are not an accident of this call's form
    torch.cuda.synchronize()
    y.fill_(GUARD_VALUE)
    st.fill_(GUARD_VALUE)
    refused = {"odd Lp": call(Lp=11), "Lp < Lv": call(Lv=14), "Lv = 0": call(Lv=0), "dil = 0": call(dil=0), "dil = 3": call(dil=3),
               "dil = 4": call(dil=4), "y == x": call(y=ptrs["x"]), "y overlaps x": call(y=ptrs["x"] + 8), "C = 64": call(Cn=64),
               "B = 0": call(B=0), "B = 65536": call(B=65536), "B = -1": call(B=-1)}
    for name in ptrs:
        refused[name + " null"] = call(**{name: None})
        if name != "w":
            refused[name + " misaligned"] = call(**{name: ptrs[name] + 4})
    torch.cuda.synchronize()
    assert all(rc != 0 for rc in refused.values()), [k for k, rc in refused.items() if rc == 0]
    assert bool((y == GUARD_VALUE).all()) and bool((st == GUARD_VALUE).all()), "a refused call wrote its outputs"
    assert float(stats.abs().max()) == 0.0 and float(gram.abs().max()) == 0.0, "a refused call touched the slot buffers"
    assert b"mi_dconv_time_layer" in lib.mi_last_error()
