"""The float32 row-tap layers -- the frequency branch's encoder convs (k = 8, s = 4, + GELU) and transposed convs as two-tap GEMMs
(rows q, q - 1), and the encoders' 128-row 1 x 1 + GLU rewrites (identity table) -- on the split-bf16 main loop fed by the LDS-DMA
row loader (gemm_x6.hip conv_rows_x6_kernel, route 8), which the float32 htdemucs engine takes by default.

  * against F.conv2d / F.conv_transpose2d in float64, no worse than three times the native DMA row route's (route 3) error on the
    same layer: 96- and 128-row tiles, a row pitch wider than the valid width, N not a multiple of 128, B > 1, Fr = 8 with T = 336;
  * bit for bit: one item alone (the 64-row small-batch tile reading the 128-row image) against the same item inside a batch that
    runs the 128-row tile; mi_set_split_bf16(0) gives route 3 and the bits of a call without a split image;
  * non-finite isolation: NaN / Inf in rows outside a tap's reach (the neighbouring item's last row, the memory around the tensor,
    the pitch padding) never reach an output;
  * the engine: a default float32 forward runs exactly the three encoder convs of levels 1-3, the three inner transposed convs and
    the four 128-row rewrites (levels 2-3, both branches) on this route; MI_X6=0 and MI_NO_DMA_ROWS=1 none.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from demucs_amd import _lib
from gpu_helpers import EPI_CONVTR, EPI_GLU, EPI_LINEAR, FLAG_GELU, FLAG_RES, FLAG_TR_FREQ, conv_call, ktab, maxerr, pack_w

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROUTE_ROWS_X6, ROUTE_DMAROW = 8, 3     # mi_debug_last_conv_route: split-bf16 + DMA row taps, native fp32 DMA row taps
SLACK = 4096                           # floats on both sides of the input (poisoned in the isolation tests)


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return _lib.load()


def rnd(*shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g, dtype=torch.float64) * scale


def _device_input(xp, fill=float("nan")):
    """xp (B, C, Fr, pitch) -> contiguous device view inside a buffer whose SLACK floats on both sides hold `fill`."""
    n = xp.numel()
    buf = torch.full((n + 2 * SLACK,), fill, device="cuda")
    buf[SLACK:SLACK + n] = xp.float().reshape(-1).cuda()
    return buf[SLACK:SLACK + n]


def _workgroups(Mpad, N):
    return Mpad // 128 * -(-N // 128)


# ---- encoder conv: Conv2d k = (8, 1), s = (4, 1), p = (2, 0) + GELU --------------------------------------------
def _enc_layer(Cin, Cout, seed):
    W, b = rnd(Cout, Cin, 8, 1, seed=seed, scale=1.0 / (8 * Cin) ** 0.5), rnd(Cout, seed=seed + 1, scale=0.2)
    return W, b, pack_w(W.reshape(Cout, -1), b)


def _enc_want(x, W, b):
    return F.gelu(F.conv2d(x, W, b, stride=(4, 1), padding=(2, 0)))


def _enc_run(lib, x, pack, pitch, x6=True, fill=float("nan"), xp=None):
    """-> (valid outputs (B, Cout, Fr / 4, T) on the host, route).  The pitch padding holds `fill`."""
    B, Cin, Fr, T = x.shape
    wt, bias, M, Mpad, K, Kpad, tile = pack
    if xp is None:
        xp = torch.full((B, Cin, Fr, pitch), fill, dtype=torch.float64)
        xp[..., :T] = x
    xin = _device_input(xp)
    kt = ktab(Cin, 8, 1, 1, 1, 2, 0, Fr * pitch, pitch, Kpad)
    P = Fr // 4 * pitch
    y = torch.full((B, M, Fr // 4, pitch), float("nan"), device="cuda")
    conv_call(x6=x6, wt=wt, M=M, Mpad=Mpad, K=K, Kpad=Kpad, ktab=kt, x=xin, x_bstride=Cin * Fr * pitch, B=B, D1=Fr, D2=T,
              O1=Fr // 4, O2=pitch, S1=4, S2=1, row_mode=1, epi=EPI_LINEAR, flags=FLAG_GELU, bias=bias, y=y, y_bstride=M * P,
              y_cstride=P, tile_m=tile, o2_valid=T if pitch != T else 0, x_ld=pitch if pitch != T else 0, dma_rows=1)
    return y[..., :T].cpu(), lib.mi_debug_last_conv_route()


#           Cin  Cout B  Fr  T    pitch   (a 128-row layer with < 200 workgroups runs the 64-row small-batch tile)
ENC_CASES = [(48, 96, 2, 32, 336, 336),    # 96 rows, K = 384 (encoder level 1's shape at Fr = 32)
             (96, 192, 3, 16, 100, 100),   # 96 rows (M = 192), K = 768
             (192, 384, 4, 32, 336, 336),  # 128 rows, K = 1536, Fr = 32 -> 8 with T = 336, 252 workgroups
             (192, 384, 1, 32, 336, 336),  # the same layer at B = 1: the small-batch tile
             (24, 128, 3, 16, 37, 40),     # 128 rows (small-batch tile), pitch 40 > 37, N = 480
             (20, 96, 2, 8, 61, 64)]       # 96 rows, K = 160, Fr = 8 -> 2, pitch 64 > 61


@pytest.mark.parametrize("Cin,Cout,B,Fr,T,pitch", ENC_CASES)
def test_rows_split_encoder_conv_matches_float64(lib, Cin, Cout, B, Fr, T, pitch):
    W, b, pack = _enc_layer(Cin, Cout, seed=10 + Cin)
    assert pack[-1] in (96, 128)
    x = rnd(B, Cin, Fr, T, seed=20 + Cin)
    want = _enc_want(x, W, b)
    got, route = _enc_run(lib, x, pack, pitch)
    assert route == ROUTE_ROWS_X6
    nat, route_nat = _enc_run(lib, x, pack, pitch, x6=False)
    assert route_nat == ROUTE_DMAROW
    err, err_nat = maxerr(got, want), maxerr(nat, want)
    print(f"enc Cin {Cin} Cout {Cout} B {B} {Fr}x{T} pitch {pitch} tile {pack[-1]}: split {err:.2e}, native fp32 {err_nat:.2e}")
    assert bool(torch.isfinite(got).all())
    assert err < 2e-5 and err <= 3 * err_nat + 2e-6


# ---- transposed conv: ConvTranspose2d k = (8, 1), s = (4, 1), cropped by 2 (+ GELU + skip) ----------------------
def _tr_layer(Cc, Co, seed):
    W, b = rnd(Cc, Co, 8, 1, seed=seed, scale=1.0 / (2 * Cc) ** 0.5), rnd(Co, seed=seed + 1, scale=0.2)
    Wr = W.reshape(Cc, Co, 8)
    W2 = torch.zeros(4 * Co, 2 * Cc, dtype=torch.float64)       # row 4co+r, col 2ci+j  <- W[ci][co][r+4j]
    for r in range(4):
        for j in range(2):
            W2[r::4, j::2] = Wr[:, :, r + 4 * j].t()
    return W, b, pack_w(W2, b.repeat_interleave(4))


def _tr_want(x, W, b, skip):
    y = F.conv_transpose2d(x, W, b, stride=(4, 1))[..., 2:-2, :]
    return y if skip is None else F.gelu(y) + skip


def _tr_run(lib, x, pack, skip, x6=True, xp=None):
    """-> (outputs (B, Co, 4 Fr, T) on the host, route)"""
    B, Cc, Fr, T = x.shape
    wt, bias, M, Mpad, K, Kpad, tile = pack
    Co = M // 4
    xin = _device_input(x if xp is None else xp)
    kt = ktab(Cc, 2, 1, -1, 1, 0, 0, Fr * T, T, Kpad)
    y = torch.full((B, Co, 4 * Fr, T), float("nan"), device="cuda")
    flags = FLAG_TR_FREQ | (FLAG_GELU | FLAG_RES if skip is not None else 0)
    res = skip.float().cuda().contiguous() if skip is not None else 0
    conv_call(x6=x6, wt=wt, M=M, Mpad=Mpad, K=K, Kpad=Kpad, ktab=kt, x=xin, x_bstride=Cc * Fr * T, B=B, D1=Fr, D2=T, O1=Fr + 1,
              O2=T, S1=1, S2=1, row_mode=1, epi=EPI_CONVTR, flags=flags, res=res, bias=bias, y=y, y_bstride=Co * 4 * Fr * T,
              y_cstride=4 * Fr * T, out_len=4 * Fr, tile_m=tile, dma_rows=1)
    return y.cpu(), lib.mi_debug_last_conv_route()


#          Cc   Co   B  Fr  T    skip   (M = 4 Co)
TR_CASES = [(384, 192, 2, 8, 336, True),   # 128 rows (M = 768), K = 768, Fr = 8 with T = 336: decoder 0's shape, 288 workgroups
            (192, 96, 2, 32, 100, True),   # 128 rows (M = 384), K = 384
            (192, 96, 1, 8, 336, False),   # 128 rows, B = 1: the small-batch tile, no flags
            (96, 48, 3, 9, 132, False),    # 96 rows (M = 192), N = 3 x 10 x 132 (not a multiple of 128)
            (96, 48, 2, 16, 100, True),    # 96 rows with GELU | RES
            (36, 32, 2, 9, 132, True)]     # 128 rows (M = 128, small-batch tile), K = 72: K padding in the last K step


@pytest.mark.parametrize("Cc,Co,B,Fr,T,skip_on", TR_CASES)
def test_rows_split_transposed_conv_matches_float64(lib, Cc, Co, B, Fr, T, skip_on):
    W, b, pack = _tr_layer(Cc, Co, seed=30 + Cc)
    assert pack[-1] in (96, 128)
    x = rnd(B, Cc, Fr, T, seed=40 + Cc)
    skip = rnd(B, Co, 4 * Fr, T, seed=41) if skip_on else None
    want = _tr_want(x, W, b, skip)
    got, route = _tr_run(lib, x, pack, skip)
    assert route == ROUTE_ROWS_X6
    nat, route_nat = _tr_run(lib, x, pack, skip, x6=False)
    assert route_nat == ROUTE_DMAROW
    err, err_nat = maxerr(got, want), maxerr(nat, want)
    print(f"convtr Cc {Cc} Co {Co} B {B} {Fr}x{T} skip {skip_on} tile {pack[-1]}: split {err:.2e}, native fp32 {err_nat:.2e}")
    assert bool(torch.isfinite(got).all())
    assert err < 2e-5 and err <= 3 * err_nat + 2e-6


# ---- encoder rewrite: 1 x 1 conv + GLU, a plain layer (its table is the identity) ------------------------------
def _glu_layer(C, seed):
    W, b = rnd(2 * C, C, 1, 1, seed=seed, scale=1.0 / C ** 0.5), rnd(2 * C, seed=seed + 1, scale=0.2)
    return W, b, pack_w(W.reshape(2 * C, -1), b, glu=True)


def _glu_run(lib, x, pack, pitch, x6=True, xp=None):
    """-> (valid outputs (B, C, Fr, T) on the host, route).  The pitch padding holds NaN."""
    B, C, Fr, T = x.shape
    wt, bias, M, Mpad, K, Kpad, tile = pack
    if xp is None:
        xp = torch.full((B, C, Fr, pitch), float("nan"), dtype=torch.float64)
        xp[..., :T] = x
    xin = _device_input(xp)
    P = Fr * pitch
    y = torch.full((B, C, Fr, pitch), float("nan"), device="cuda")
    conv_call(x6=x6, wt=wt, M=M, Mpad=Mpad, K=K, Kpad=Kpad, ktab=ktab(C, 1, 1, 1, 1, 0, 0, P, P, Kpad), x=xin, x_bstride=C * P, B=B,
              D1=1, D2=P, O1=1, O2=P, S1=1, S2=1, epi=EPI_GLU, bias=bias, y=y, y_bstride=C * P, y_cstride=P, tile_m=tile, plain=1,
              o2_valid=0)
    return y[..., :T].cpu(), lib.mi_debug_last_conv_route()


#           C    B  Fr  T     pitch
GLU_CASES = [(192, 2, 32, 336, 336),       # encoder level 2's shape (M = 384), 252 workgroups
             (384, 1, 8, 336, 336),        # level 3 at B = 1 (M = 768): 126 workgroups, the small-batch tile
             (64, 3, 1, 1001, 1004)]       # time-branch-like rows, pitch 1004 > 1001 (NaN padding), N not a multiple of 128


@pytest.mark.parametrize("C,B,Fr,T,pitch", GLU_CASES)
def test_rows_split_rewrite_glu_matches_float64(lib, C, B, Fr, T, pitch):
    W, b, pack = _glu_layer(C, seed=80 + C)
    assert pack[-1] == 128
    x = rnd(B, C, Fr, T, seed=81 + C)
    want = F.glu(F.conv2d(x, W, b), dim=1)
    got, route = _glu_run(lib, x, pack, pitch)
    assert route == ROUTE_ROWS_X6
    nat, route_nat = _glu_run(lib, x, pack, pitch, x6=False)
    assert route_nat == ROUTE_DMAROW
    err, err_nat = maxerr(got, want), maxerr(nat, want)
    print(f"glu C {C} B {B} {Fr}x{T} pitch {pitch}: split {err:.2e}, native fp32 {err_nat:.2e}")
    assert bool(torch.isfinite(got).all())
    assert err < 2e-5 and err <= 3 * err_nat + 2e-6


# ---- bit identity ----------------------------------------------------------------------------------------------
def test_rows_split_single_item_equals_batched_encoder(lib):
    """Item 1 of a batch that runs the 128-row tile, alone (under 200 workgroups: the 64-row tile reading the 128-row image)."""
    Cin, Cout, B, Fr, T = 192, 384, 4, 32, 336
    W, b, pack = _enc_layer(Cin, Cout, seed=50)
    Mpad = pack[3]
    assert pack[-1] == 128 and _workgroups(Mpad, B * Fr // 4 * T) >= 200 > _workgroups(Mpad, Fr // 4 * T)
    x = rnd(B, Cin, Fr, T, seed=51)
    batched, route = _enc_run(lib, x, pack, T)
    assert route == ROUTE_ROWS_X6
    alone, route = _enc_run(lib, x[1:2], pack, T)
    assert route == ROUTE_ROWS_X6
    assert torch.equal(batched[1:2], alone)


def test_rows_split_single_item_equals_batched_transposed(lib):
    Cc, Co, B, Fr, T = 384, 192, 2, 8, 336
    W, b, pack = _tr_layer(Cc, Co, seed=52)
    Mpad = pack[3]
    assert pack[-1] == 128 and _workgroups(Mpad, B * (Fr + 1) * T) >= 200 > _workgroups(Mpad, (Fr + 1) * T)
    x, skip = rnd(B, Cc, Fr, T, seed=53), rnd(B, Co, 4 * Fr, T, seed=54)
    batched, route = _tr_run(lib, x, pack, skip)
    assert route == ROUTE_ROWS_X6
    alone, route = _tr_run(lib, x[1:2], pack, skip[1:2])
    assert route == ROUTE_ROWS_X6
    assert torch.equal(batched[1:2], alone)


def test_rows_split_single_item_equals_batched_rewrite(lib):
    C, B, Fr, T = 384, 2, 8, 336
    W, b, pack = _glu_layer(C, seed=55)
    Mpad = pack[3]
    assert _workgroups(Mpad, B * Fr * T) >= 200 > _workgroups(Mpad, Fr * T)
    x = rnd(B, C, Fr, T, seed=56)
    batched, route = _glu_run(lib, x, pack, T)
    assert route == ROUTE_ROWS_X6
    alone, route = _glu_run(lib, x[1:2], pack, T)
    assert route == ROUTE_ROWS_X6
    assert torch.equal(batched[1:2], alone)


def test_split_switch_selects_native_row_route(lib):
    """mi_set_split_bf16(0) sends a layer WITH a split image to the native DMA row loop, bit-identical to a call without one."""
    W, b, pack = _enc_layer(96, 192, seed=60)
    x = rnd(2, 96, 16, 50, seed=61)
    Wt, bt, packt = _tr_layer(192, 96, seed=62)
    xt, skip = rnd(2, 192, 8, 52, seed=63), rnd(2, 96, 32, 52, seed=64)
    Wg, bg, packg = _glu_layer(192, seed=65)
    xg = rnd(2, 192, 4, 100, seed=66)
    nat, route = _enc_run(lib, x, pack, 52, x6=False)
    assert route == ROUTE_DMAROW
    natt, route = _tr_run(lib, xt, packt, skip, x6=False)
    assert route == ROUTE_DMAROW
    natg, route = _glu_run(lib, xg, packg, 100, x6=False)
    assert route == ROUTE_DMAROW
    old = lib.mi_set_split_bf16(0)
    try:
        off, route = _enc_run(lib, x, pack, 52)
        assert route == ROUTE_DMAROW
        offt, route = _tr_run(lib, xt, packt, skip)
        assert route == ROUTE_DMAROW
        offg, route = _glu_run(lib, xg, packg, 100)
        assert route == ROUTE_DMAROW
    finally:
        lib.mi_set_split_bf16(old)
    assert old == 1
    assert torch.equal(off, nat) and torch.equal(offt, natt) and torch.equal(offg, natg)
    _enc_run(lib, x, pack, 52)
    assert lib.mi_debug_last_conv_route() == ROUTE_ROWS_X6


# ---- non-finite isolation --------------------------------------------------------------------------------------
def test_rows_split_encoder_non_finite_isolation(lib):
    """NaN / Inf in input samples: only the outputs whose taps reach them (rows 4 o1 - 2 .. 4 o1 + 5, the same column, every
    output channel of that item) change.  The memory around the tensor (what rows -2, -1 of item 0 and rows Fr, Fr + 1 of the
    last item would address) and the pitch padding hold NaN; item 0's last row of its last channel is what item 1's rows -2 / -1
    of channel 0 would address."""
    Cin, Cout, B, Fr, T, pitch = 64, 128, 3, 16, 61, 64
    W, b, pack = _enc_layer(Cin, Cout, seed=70)
    x = rnd(B, Cin, Fr, T, seed=71)
    clean, route = _enc_run(lib, x, pack, pitch)
    assert route == ROUTE_ROWS_X6
    hits = [(0, Cin - 1, Fr - 1, 5, float("nan")), (0, Cin - 1, Fr - 2, 9, float("inf")), (1, 0, 0, 7, float("-inf")),
            (2, 3, 6, T - 1, float("nan")), (1, 10, 1, 0, float("nan"))]
    xp = torch.full((B, Cin, Fr, pitch), float("nan"), dtype=torch.float64)
    xp[..., :T] = x
    for bb, cc, rr, tt, v in hits:
        xp[bb, cc, rr, tt] = v
    got, route = _enc_run(lib, x, pack, pitch, xp=xp)
    assert route == ROUTE_ROWS_X6
    mask = torch.ones(B, Cout, Fr // 4, T, dtype=torch.bool)
    for bb, cc, rr, tt, _ in hits:
        for o1 in range(Fr // 4):
            if 4 * o1 - 2 <= rr <= 4 * o1 + 5:
                mask[bb, :, o1, tt] = False
    assert bool(torch.isfinite(got[mask]).all())
    assert torch.equal(got[mask], clean[mask])
    assert not bool(torch.isfinite(got[~mask]).all())         # the poison did reach the outputs that depend on it


def test_rows_split_transposed_non_finite_isolation(lib):
    """Transposed conv: output row 4 q + r - 2 reads input rows q and q - 1.  A poisoned last row of item 0's last channel sits
    where item 1's row -1 of channel 0 would be; the memory around the tensor holds NaN."""
    Cc, Co, B, Fr, T = 48, 32, 3, 9, 132
    W, b, pack = _tr_layer(Cc, Co, seed=72)
    x = rnd(B, Cc, Fr, T, seed=73)
    clean, route = _tr_run(lib, x, pack, None)
    assert route == ROUTE_ROWS_X6
    hits = [(0, Cc - 1, Fr - 1, 3, float("nan")), (1, 0, 0, 8, float("inf")), (2, 5, 4, T - 1, float("-inf")),
            (1, Cc - 1, Fr - 1, 0, float("nan"))]
    xp = x.clone()
    for bb, cc, rr, tt, v in hits:
        xp[bb, cc, rr, tt] = v
    got, route = _tr_run(lib, x, pack, None, xp=xp)
    assert route == ROUTE_ROWS_X6
    mask = torch.ones(B, Co, 4 * Fr, T, dtype=torch.bool)
    for bb, cc, rr, tt, _ in hits:
        for q in (rr, rr + 1):               # input row rr is tap j = 0 of q = rr and tap j = 1 of q = rr + 1
            for r in range(4):
                o = 4 * q + r - 2
                if 0 <= o < 4 * Fr:
                    mask[bb, :, o, tt] = False
    assert bool(torch.isfinite(got[mask]).all())
    assert torch.equal(got[mask], clean[mask])
    assert not bool(torch.isfinite(got[~mask]).all())


# ---- the engine's default ----------------------------------------------------------------------------------------
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
    env = {k: v for k, v in os.environ.items() if k not in ("MI_X6", "MI_NO_DMA_ROWS")}
    env.update(env_extra, PYTHONPATH=ROOT)
    out = str(tmp_path / tag)
    r = subprocess.run([sys.executable, "-c", _ENGINE, out], env=env, capture_output=True, text=True, cwd=ROOT, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    rows = {}
    for line in open(out + ".txt"):
        name, n = line.rsplit(" ", 1)
        rows[name] = int(n)
    return np.load(out + ".npy"), rows


def test_engine_default_runs_frequency_row_convs_on_the_split_loop(tmp_path):
    """float32 htdemucs forward, one fresh process each: by default the encoder convs of levels 1-3 (K = 384 / 768 on 96 rows,
    1536 on 128), the transposed convs of decoders 0-2 (128, 128, 96 rows) and the 1 x 1 + GLU rewrites of encoder levels 2-3 in
    both branches on the row split loop, nothing else; MI_X6=0 and
    MI_NO_DMA_ROWS=1 run none, and every forward stays within the engine's 1e-4 parity target of the others."""
    y_def, rows_def = _engine_run(tmp_path, "default", {})
    rx6 = {k: v for k, v in rows_def.items() if k.startswith("conv_rows_x6")}
    assert rx6 == {"conv_rows_x6<linear,tile96>": 2, "conv_rows_x6<linear,tile128>": 1,
                   "conv_rows_x6<convtr,tile128>": 2, "conv_rows_x6<convtr,tile96>": 1, "conv_rows_x6<glu,tile128>": 4}, rows_def
    for tag, env in (("mi_x6_0", {"MI_X6": "0"}), ("no_dma_rows", {"MI_NO_DMA_ROWS": "1"})):
        y_off, rows_off = _engine_run(tmp_path, tag, env)
        assert not any(k.startswith("conv_rows_x6") for k in rows_off), rows_off
        d = np.abs(y_def.astype(np.float64) - y_off).max()
        print(f"default vs {tag}: max-abs {d:.3e}")
        assert d < 1e-4
