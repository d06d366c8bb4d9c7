"""The float32 decoders' rewrite convs (3 x 3 and k = 3, stride 1, + GLU) on the split-bf16 main loop fed by LDS-DMA shifted-run
taps (gemm_x6.hip conv_tap_x6_kernel, route 7), which the float32 htdemucs engine takes by default.

  * against F.conv2d / F.conv1d + GLU in float64, no worse than three times the native DMA tap route's (route 2) error on the same
    layer: 96- and 128-row tiles, a row pitch wider than the valid width, N not a multiple of 128, B > 1, Fr = 8 with T = 336;
  * bit for bit: one item alone (the 64-row small-batch tile reading the 128-row image) against the same item inside a batch that
    runs the 128-row tile; mi_set_split_bf16(0) gives route 2 and the bits of a call without a split image;
  * non-finite isolation: NaN / Inf in the neighbouring row's samples that the shifted runs drag in, and in the pitch padding,
    never reach an output outside the conv's receptive field;
  * the engine: a default float32 forward runs the 44 linears and the 8 rewrite convs on the split loops, MI_X6=0 neither.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from demucs_amd import _lib
from gpu_helpers import EPI_GLU, conv_call, maxerr, pack_w

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROUTE_TAP_X6, ROUTE_DMATAP = 7, 2      # mi_debug_last_conv_route: split-bf16 + DMA taps, native fp32 DMA taps
SLACK = 32                             # floats on both sides of the input, as the engine's decoder-input buffers carry


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return _lib.load()


def rnd(*shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g, dtype=torch.float64) * scale


def _layer(C, ntaps, seed):
    """GLU rewrite conv C -> 2C (3 x 3 or k = 3 along time) and its packed weights."""
    shape = (2 * C, C, 3, 3) if ntaps == 9 else (2 * C, C, 1, 3)
    W, b = rnd(*shape, seed=seed, scale=0.5 / (C * ntaps) ** 0.5), rnd(2 * C, seed=seed + 1, scale=0.2)
    return W, b, pack_w(W.reshape(2 * C, -1), b, glu=True)


def _want(x, W, b, ntaps):
    return F.glu(F.conv2d(x, W, b, padding=1 if ntaps == 9 else (0, 1)), dim=1)


def _input(x, pitch, fill=float("nan")):
    """x (B, C, Fr, T) float64 -> device view of the padded rows inside a buffer whose pitch columns and slack hold `fill`."""
    B, C, Fr, T = x.shape
    xp = torch.full((B, C, Fr, pitch), fill)
    xp[..., :T] = x.float()
    n = B * C * Fr * pitch
    buf = torch.full((n + 2 * SLACK,), fill, device="cuda")
    buf[SLACK:SLACK + n] = xp.reshape(-1).cuda()
    return buf[SLACK:SLACK + n]


def _run(lib, x, pack, ntaps, pitch, x6=True):
    """One rewrite conv on the DMA tap geometry -> (valid outputs (B, C, Fr, T) on the host, route)."""
    B, C, Fr, T = x.shape
    wt, bias, M, Mpad, K, Kpad, tile = pack
    xin = _input(x, pitch)
    P = Fr * pitch
    y = torch.full((B, C, Fr, pitch), float("nan"), device="cuda")
    conv_call(x6=x6, wt=wt, M=M, Mpad=Mpad, K=K, Kpad=Kpad, x=xin, x_bstride=C * P, B=B, D1=Fr, D2=T, O1=Fr, O2=pitch, S1=1, S2=1,
              row_mode=1 if ntaps == 9 else 0, epi=EPI_GLU, bias=bias, y=y, y_bstride=C * P, y_cstride=P, tile_m=tile,
              o2_valid=T if pitch != T else 0, x_ld=pitch if pitch != T else 0, ntaps=ntaps, tap_k2=3,
              tap_pad1=1 if ntaps == 9 else 0, tap_pad2=1)
    return y[..., :T].cpu(), lib.mi_debug_last_conv_route()


def _workgroups(Mpad, B, Fr, pitch):
    return Mpad // 128 * -(-B * Fr * pitch // 128)


#         C  ntaps B  Fr  T    pitch       (a 128-row layer with < 200 workgroups runs the 64-row small-batch tile)
CASES = [(192, 9, 4, 8, 336, 336),         # 128 rows (M = 384), the deepest decoder's Fr x T, 252 workgroups
         (128, 9, 2, 8, 336, 336),         # 128 rows, 84 workgroups: the small-batch tile
         (64, 9, 3, 3, 37, 40),            # 128 rows (small-batch tile), pitch 40 > 37, N = 360
         (48, 9, 3, 5, 61, 64),            # 96 rows (M = 96), pitch 64 > 61
         (96, 9, 2, 12, 100, 100),         # 96 rows (M = 192)
         (192, 3, 2, 1, 5375, 5376),       # k = 3, 128 rows, pitch 5376 > 5375
         (96, 3, 3, 1, 1001, 1004),        # k = 3, 96 rows, N = 3012
         (40, 3, 2, 1, 333, 336)]          # k = 3, 96 rows (M = 80), K = 120: padding past K in the last K step


@pytest.mark.parametrize("C,ntaps,B,Fr,T,pitch", CASES)
def test_tap_split_matches_float64(lib, C, ntaps, B, Fr, T, pitch):
    W, b, pack = _layer(C, ntaps, seed=10 + C + ntaps)
    assert pack[-1] in (96, 128)
    x = rnd(B, C, Fr, T, seed=20 + C)
    want = _want(x, W, b, ntaps)
    got, route = _run(lib, x, pack, ntaps, pitch)
    assert route == ROUTE_TAP_X6
    nat, route_nat = _run(lib, x, pack, ntaps, pitch, x6=False)
    assert route_nat == ROUTE_DMATAP
    err, err_nat = maxerr(got, want), maxerr(nat, want)
    print(f"C {C} taps {ntaps} B {B} {Fr}x{T} pitch {pitch} tile {pack[-1]}: split {err:.2e}, native fp32 {err_nat:.2e}")
    assert bool(torch.isfinite(got).all())
    assert err < 2e-5 and err <= 3 * err_nat + 2e-6


@pytest.mark.parametrize("ntaps", [9, 3])
def test_tap_split_single_item_equals_batched(lib, ntaps):
    """Item 1 of a batch that runs the 128-row tile, alone (B = 1: under 200 workgroups, so the 64-row small-batch tile reading
    the 128-row image), gives the same bits as inside the batch."""
    C = 192
    B, Fr, T, pitch = (4, 8, 336, 336) if ntaps == 9 else (3, 1, 8445, 8448)
    W, b, pack = _layer(C, ntaps, seed=40 + ntaps)
    Mpad = pack[3]
    assert pack[-1] == 128 and _workgroups(Mpad, B, Fr, pitch) >= 200 > _workgroups(Mpad, 1, Fr, pitch)
    x = rnd(B, C, Fr, T, seed=50 + ntaps)
    batched, route = _run(lib, x, pack, ntaps, pitch)
    assert route == ROUTE_TAP_X6
    alone, route = _run(lib, x[1:2], pack, ntaps, pitch)
    assert route == ROUTE_TAP_X6
    assert torch.equal(batched[1:2], alone)


@pytest.mark.parametrize("ntaps", [9, 3])
def test_split_switch_selects_native_tap_route(lib, ntaps):
    """mi_set_split_bf16(0) sends a rewrite conv WITH a split image to the native DMA tap loop, bit-identical to a call without one."""
    C, B, Fr, T, pitch = (96, 2, 8, 50, 52) if ntaps == 9 else (96, 2, 1, 999, 1000)
    W, b, pack = _layer(C, ntaps, seed=60 + ntaps)
    x = rnd(B, C, Fr, T, seed=70 + ntaps)
    nat, route = _run(lib, x, pack, ntaps, pitch, x6=False)
    assert route == ROUTE_DMATAP
    old = lib.mi_set_split_bf16(0)
    try:
        off, route = _run(lib, x, pack, ntaps, pitch)
        assert route == ROUTE_DMATAP
    finally:
        lib.mi_set_split_bf16(old)
    assert old == 1
    assert torch.equal(off, nat)
    _run(lib, x, pack, ntaps, pitch)
    assert lib.mi_debug_last_conv_route() == ROUTE_TAP_X6


@pytest.mark.parametrize("ntaps,pitch_pad", [(9, 0), (9, 3), (3, 0), (3, 3)])
def test_tap_split_non_finite_isolation(lib, ntaps, pitch_pad):
    """NaN at the end of one input row and Inf at the start of another: with no pitch padding the shifted runs of the neighbouring
    rows' outputs read them from memory; with pitch padding, the padding columns are NaN too.  Outputs outside the conv's receptive
    field of the poisoned samples equal the clean run bit for bit, and stay finite."""
    C, B = 64, 3
    Fr, pitch = (6, 132) if ntaps == 9 else (1, 508)
    T = pitch - pitch_pad
    W, b, pack = _layer(C, ntaps, seed=80 + ntaps)
    x = rnd(B, C, Fr, T, seed=90 + ntaps)
    clean, route = _run(lib, x, pack, ntaps, pitch)
    assert route == ROUTE_TAP_X6
    xp = x.clone()
    # the last sample of a row and the first of the next row in memory (next frequency row, or next channel of the time branch),
    # plus the last sample of item 0's last channel and the first of item 1's first channel (adjacent across the batch boundary)
    hits = [(0, 5, Fr - 1, T - 1, float("nan")), (1, 7, 0, 0, float("inf")), (0, C - 1, Fr - 1, T - 1, float("nan")),
            (1, 0, 0, 0, float("-inf"))]
    if Fr > 1:
        hits += [(2, 9, 2, T - 1, float("nan")), (2, 9, 3, 0, float("inf"))]
    for bb, cc, rr, tt, v in hits:
        xp[bb, cc, rr, tt] = v
    got, route = _run(lib, xp, pack, ntaps, pitch)
    assert route == ROUTE_TAP_X6
    # receptive field: every output channel of the poisoned item, rows rr - 1 .. rr + 1 (3 x 3), columns tt - 1 .. tt + 1
    mask = torch.ones(B, C, Fr, T, dtype=torch.bool)
    for bb, cc, rr, tt, _ in hits:
        r0, r1 = (max(rr - 1, 0), min(rr + 2, Fr)) if ntaps == 9 else (rr, rr + 1)
        mask[bb, :, r0:r1, max(tt - 1, 0):min(tt + 2, T)] = False
    assert bool(torch.isfinite(got[mask]).all())
    assert torch.equal(got[mask], clean[mask])
    assert not bool(torch.isfinite(got[~mask]).all())         # the poison did reach the outputs that depend on it


# ---- the engine's default ------------------------------------------------------------------------
_ENGINE = r"""
import sys
import numpy as np
import torch
from demucs_amd.htdemucs import HTDemucs
from demucs_amd.synth import synth_mix
from demucs_amd.weights import HTDemucsConfig, synthetic_state_dict
cfg = HTDemucsConfig()
m = HTDemucs(cfg.sources, max_batch=1)
m.load_state_dict(synthetic_state_dict(cfg, 0))
m.to("cuda").eval()
mix = torch.from_numpy(synth_mix(3, cfg.segment_length, "tones"))[None].cuda()
m(mix)
m.profile_begin()
out = m(mix)
rows = m.profile_end()
np.save(sys.argv[1] + ".npy", out.cpu().numpy())
with open(sys.argv[1] + ".txt", "w") as f:
    for r in rows:
        f.write(f"{r['name']} {r['launches']}\n")
"""


def _engine_run(tmp_path, tag, env_extra):
    env = {k: v for k, v in os.environ.items() if k != "MI_X6"}
    env.update(env_extra, PYTHONPATH=ROOT)
    out = str(tmp_path / tag)
    r = subprocess.run([sys.executable, "-c", _ENGINE, out], env=env, capture_output=True, text=True, cwd=ROOT, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    rows = {}
    for line in open(out + ".txt"):
        name, n = line.rsplit(" ", 1)
        rows[name] = int(n)
    return np.load(out + ".npy"), rows


def test_engine_default_runs_rewrites_on_the_tap_split_loop(tmp_path):
    """float32 htdemucs forward, one fresh process each: by default the 44 transformer linears on the split loop and the eight
    decoder rewrite convs (four 3 x 3, four k = 3) on the tap split loop, nothing else; MI_X6=0 runs neither; the two forwards stay
    within the engine's 1e-4 parity target of each other."""
    y_def, rows_def = _engine_run(tmp_path, "default", {})
    x6 = {k: v for k, v in rows_def.items() if k.startswith("conv_gemm_x6")}
    tap = {k: v for k, v in rows_def.items() if k.startswith("conv_tap_x6")}
    assert all(k.startswith("conv_gemm_x6<linear,") for k in x6) and sum(x6.values()) == 44, rows_def
    assert all(k.startswith("conv_tap_x6<glu,") for k in tap) and sum(tap.values()) == 8, rows_def
    assert sum(v for k, v in tap.items() if k.endswith("taps9>")) == 4, tap
    y_off, rows_off = _engine_run(tmp_path, "mi_x6_0", {"MI_X6": "0"})
    assert not any(k.startswith(("conv_gemm_x6", "conv_tap_x6")) for k in rows_off), rows_off
    d = np.abs(y_def.astype(np.float64) - y_off).max()
    print(f"split (linears + rewrite convs) vs native fp32 forward: max-abs {d:.3e}")
    assert 0 < d < 1e-4
