"""The statistics epilogues of the implicit-GEMM convs (MI_EPI_BIAS_STATS, MI_EPI_STATS_ONLY; csrc/gemm_tile.h conv_epilogue) when
the statistics row is the batch ITEM (row_mode 0) and an item has fewer than 32 columns: what the time-branch DConv blocks of the
hdemucs engine run on a batch of short chunks (csrc/engine_core.hip run_dconv, row pitch round_up(ceil(L / 4^(i+1)), 4) at level i).

The epilogue reduces a wave's 32 consecutive columns into the row of the wave's first column and ONE other row, so three items in
such a run would lose the middle ones' sums to the last.  `launch_conv` runs those layers one item per launch (csrc/conv_route.hip
conv_stats_per_item).  Checked here through `mi_conv_forward`: a k = 3 Conv1d/2d, dilation 1 (one case 2), C -> C / 4 on the 32- and
the 64-row tile, in float32 (stated geometry: the DMA tap loop where the pitch allows it; and the table-driven gather) and in the
bf16 / f16 modes.  AFFECTED geometries put three or more items into one aligned 32-column window; CONTROLS never do.

Item b is drawn as (b + 1) * randn + b: a sum credited to another item's row cannot pass.  Padding columns of the input hold NaN
and y starts as NaN: padding is neither stored nor counted.

Bounds.  Stored tensor, float32: 6e-6 * max|want| against float64, the bar of the DMA-tap statistics test in test_gpu_kernels.py.
Half modes: against float64 on operands rounded to the 16-bit type, by the rule of tests/test_gpu_half_linear.py -- 4 x the largest
distance of the SAME formula evaluated in torch float32 on the CPU from float64, over every case of this file with that type and
K (the kernels sum in another order); nothing is taken from the kernels.  Statistics: the 32 slots of an item summed in float64
against the float64 sum / sum of squares of the tensor the launch STORED (valid columns, rows < M: exactly the values it summed),
|diff| / max(|ref|, 1) < 2e-5; STATS_ONLY against BIAS_STATS, and a second BIAS_STATS launch on a re-zeroed buffer against the first,
to 1e-9 relative (the order of the float64 atomics differs between launches).

Without a GPU: tools/conv_route_table.hip `stats` prints, for every (epilogue, row_mode, B, O1, O2) up to 13 items of 40 columns,
what conv_validate says and whether launch_conv goes item by item; the test counts the rows in every aligned 32-column window
itself and holds the two together."""
import ctypes as C
import functools
import os
import subprocess

import pytest
import torch
import torch.nn.functional as F

from demucs_amd import _lib
from gpu_helpers import EPI_BIAS_STATS, EPI_STATS_ONLY, SLOTS, conv_desc, ktab, pack_w

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "demucs_amd", "csrc")
HDT = {"bf16": torch.bfloat16, "f16": torch.float16}
WEIGHTS = [(12, 48), (48, 192)]                  # (M, Cin): the smallest that use the 32- and the 64-row statistics tile
# (B, O1, O2 = row pitch, valid o2)
AFFECTED = [(3, 1, 4, 3), (8, 1, 4, 4), (3, 1, 8, 5), (3, 1, 12, 11), (12, 1, 12, 12),      # 12 x 12: N = 144 crosses a 128-column tile
            (4, 1, 20, 18), (7, 1, 20, 20), (3, 3, 4, 4),                                  # O1 > 1 with a per-item row: P = 12
            (4, 1, 17, 17)]                                                                # no multiple of 4: exact O2, table-driven gather
CONTROLS = [(5, 1, 16, 13), (7, 1, 28, 25), (3, 1, 32, 30), (2, 1, 12, 11)]
CASES = [(g, 1) for g in AFFECTED + CONTROLS] + [((4, 1, 20, 18), 2)]                      # (geometry, dilation)
MODES = ["f32tap", "f32table", "bf16", "f16"]
SLACK = 32                                       # floats on both sides of x, as the engine's buffers carry (shifted-run loaders)


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return _lib.load()


def stream():
    return C.c_void_p(_lib.current_stream_ptr())


@functools.lru_cache(maxsize=None)
def operands(M, Cin, geo, dil, half):
    """(x, W, bias) as float32 tensors whose values the mode's operand type holds exactly, and the float64 conv of them with its
    float32 restatement's distance from it."""
    B, O1, O2, valid = geo
    g = torch.Generator().manual_seed(100003 * M + 1009 * (B * 64 + O1 * 1600 + O2 * 40 + valid) + dil)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)          # noqa: E731
    x = torch.stack([(b + 1) * rn(Cin, O1, valid) + b for b in range(B)]).float()
    W = (rn(M, Cin, 1, 3) * (3 * Cin) ** -0.5).float()
    bias = rn(M).float()
    if half:
        x, W = x.to(HDT[half]).float(), W.to(HDT[half]).float()
    conv = lambda dt: F.conv2d(x.to(dt), W.to(dt), bias.to(dt), padding=(0, dil), dilation=(1, dil))      # noqa: E731
    want = conv(torch.float64)
    return x, W, bias, want, (conv(torch.float32).double() - want).abs().max().item()


@functools.lru_cache(maxsize=None)
def half_bound(M, Cin, half):
    return 4 * max(operands(M, Cin, geo, dil, half)[4] for geo, dil in CASES)


def launch(lib, mode, epi, x, W, bias, geo, dil, y, stats):
    B, O1, O2, valid = geo
    M, Cin = W.shape[:2]
    P = O1 * O2
    wt, bd, M, Mpad, K, Kpad, tile = pack_w(W.reshape(M, -1), bias)
    xp = torch.full((B, Cin, O1, O2), float("nan"))
    xp[..., :valid] = x
    buf = torch.full((B * Cin * P + 2 * SLACK,), float("nan"), device="cuda")
    buf[SLACK:SLACK + B * Cin * P] = xp.reshape(-1).cuda()
    kt = ktab(Cin, 1, 3, 1, dil, 0, dil, P, O2, Kpad)
    taps = dict(ntaps=3, tap_k2=3, tap_pad1=0, tap_pad2=dil, tap_dil2=dil) if mode == "f32tap" else {}
    out = dict(y=y, y_bstride=M * P, y_cstride=P) if y is not None else {}
    d, keep = conv_desc(x6=mode if mode in HDT else False, wt=wt, M=M, Mpad=Mpad, K=K, Kpad=Kpad, ktab=kt, x=buf[SLACK:SLACK + B * Cin * P],
                        x_bstride=Cin * P, B=B, D1=O1, D2=valid, O1=O1, O2=O2, S1=1, S2=1, row_mode=0, epi=epi, bias=bd, stats=stats, tile_m=tile,
                        o2_valid=valid if valid != O2 else 0, x_ld=O2 if valid != O2 else 0, **out, **taps)
    _lib.check(lib.mi_conv_forward(C.byref(d), stream()), "mi_conv_forward")
    torch.cuda.synchronize()
    return lib.mi_debug_last_conv_route(), lib.mi_debug_last_conv_tile()


def rel(a, b):
    return ((a - b).abs() / b.abs().clamp_min(1.0)).max().item()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("M,Cin", WEIGHTS)
@pytest.mark.parametrize("geo,dil", CASES, ids=[f"{'x'.join(map(str, g))}d{d}" for g, d in CASES])
def test_every_item_row_gets_its_own_sums(lib, geo, dil, M, Cin, mode):
    B, O1, O2, valid = geo
    half = mode if mode in HDT else None
    x, W, bias, want, _ = operands(M, Cin, geo, dil, half)
    what = f"{mode} M {M} K {3 * Cin} geo {geo} dil {dil}"
    new_y = lambda: torch.full((B, M, O1, O2), float("nan"), device="cuda")                     # noqa: E731
    new_stats = lambda: torch.zeros(B, SLOTS, 2, dtype=torch.float64, device="cuda")            # noqa: E731

    y, stats = new_y(), new_stats()
    route = launch(lib, mode, EPI_BIAS_STATS, x, W, bias, geo, dil, y, stats)
    got = y[..., :valid].cpu()
    err, scale = (got.double() - want).abs().max().item(), want.abs().max().item()
    bound = half_bound(M, Cin, half) if half else 6e-6 * scale
    yd = got.double()
    ref = torch.stack([yd.sum((1, 2, 3)), (yd ** 2).sum((1, 2, 3))], 1)
    s = stats.sum(1).cpu()

    stats2 = new_stats()
    route2 = launch(lib, mode, EPI_STATS_ONLY, x, W, bias, geo, dil, None, stats2)
    s2 = stats2.sum(1).cpu()

    y3 = new_y()
    stats.zero_()
    launch(lib, mode, EPI_BIAS_STATS, x, W, bias, geo, dil, y3, stats)
    s3 = stats.sum(1).cpu()

    print(f"{what}: BIAS_STATS route/tile {route}, STATS_ONLY {route2}; stored err {err:.2e} (bound {bound:.2e}, max|want| {scale:.1f}); "
          f"sums vs stored {rel(s, ref):.2e}, STATS_ONLY vs BIAS_STATS {rel(s2, s):.2e}, second launch vs first {rel(s3, s):.2e}")
    assert bool(torch.isfinite(got).all()), f"{what}: padding reached a stored value"
    assert valid == O2 or bool(torch.isnan(y[..., valid:]).all()), f"{what}: a padding column was stored"
    assert err < bound, f"{what}: stored tensor {err:.3e} >= {bound:.3e}"
    assert rel(s, ref) < 2e-5, f"{what}: BIAS_STATS sums\n{s}\nstored tensor's\n{ref}"
    assert rel(s2, ref) < 2e-5, f"{what}: STATS_ONLY sums\n{s2}\nstored tensor's\n{ref}"
    assert rel(s2, s) < 1e-9, f"{what}: STATS_ONLY {s2} vs BIAS_STATS {s}"
    assert torch.equal(y3[..., :valid].cpu(), got) and rel(s3, s) < 1e-9, f"{what}: second launch on the re-zeroed buffer {s3} vs {s}"


# ---- without a GPU -----------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def stats_table(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("conv_route_stats") / "conv_route_table")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-std=c++17", "-O1", os.path.join(ROOT, "tools", "conv_route_table.hip"),
                        os.path.join(CSRC, "conv_route.hip"), os.path.join(CSRC, "switches.hip"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    env = {k: v for k, v in os.environ.items() if not k.startswith("MI_")}
    r = subprocess.run([exe, "stats"], env=env, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr[-2000:]
    out = {}
    for line in r.stdout.splitlines():
        name, rest = line.split(" ", 1)
        _, e, rm, B, o = name.split("_")
        key = (int(e[1:]), int(rm[1:]), int(B[1:]), *map(int, o.split("x")))
        assert key not in out
        out[key] = rest if rest.startswith("invalid:") else tuple(int(v) for v in rest.split())
    return out


def rows_in_a_window(row_mode, B, O1, O2):
    """most statistics rows among the columns of one aligned 32-column window (a wave's columns: tiles start at multiples of 128)"""
    P, N = O1 * O2, B * O1 * O2
    row = (lambda n: n // O2) if row_mode else (lambda n: n // P)        # b * O1 + o1 / b
    return max(len({row(n) for n in range(w, min(w + 32, N))}) for w in range(0, N, 32))


def test_what_conv_validate_accepts_the_epilogue_counts(stats_table):
    """Whatever conv_validate accepts for a statistics epilogue reaches the kernels with at most two rows per wave: the launch as
    it stands, or item by item (one row per launch).  Per-item rows are accepted at any width, rows (b, o1) below 32 columns are
    refused with their message, and a layer whose item has 32 columns or more, or a batch of up to two, is never taken apart."""
    assert len(stats_table) == 2 * 2 * 13 * 2 * 40
    for (epi, row_mode, B, O1, O2), got in stats_table.items():
        what = f"epi {epi} row_mode {row_mode} B {B} {O1} x {O2}"
        if row_mode == 1 and O2 < 32:
            assert isinstance(got, str) and "row_mode 1) needs O2 >= 32" in got, (what, got)
            continue
        assert not isinstance(got, str), (what, got)
        per_item = got[3]
        assert per_item in (0, 1)
        assert per_item or rows_in_a_window(row_mode, B, O1, O2) <= 2, f"{what}: {rows_in_a_window(row_mode, B, O1, O2)} rows in one wave's columns"
        if row_mode == 1 or B <= 2 or O1 * O2 >= 32:
            assert per_item == 0, what


def test_the_affected_and_control_geometries_are_what_they_say():
    for B, O1, O2, _ in AFFECTED:
        assert rows_in_a_window(0, B, O1, O2) > 2, (B, O1, O2)
    for B, O1, O2, _ in CONTROLS:
        assert rows_in_a_window(0, B, O1, O2) <= 2, (B, O1, O2)
