"""The 192-row tile of the split-bf16 main loop (gemm_x6.hip conv_x6_body<2, 2, 3, 2>): a float32 layer with M % 192 == 0 states
`tile_m = 192`, carries its split image in the 96-row layout and runs the 192-row tile on pairs of those images when its
workgroups fill the chip, else the 96-row tile on the same image.

  * per loader family and epilogue -- plain LINEAR on LayerNorm-ed tokens (route 4), the tap convs + GLU with 9 and 3 taps
    (route 7), the row-tap encoder conv + GELU, transposed conv and 1 x 1 + GLU (route 8) -- at M = 192 (one tile; the 1 x 1 + GLU
    family, whose row loader needs a 128-row layer, at M = 384 and 768) and M = 384 (two tiles: the image-pair indexing):
    against float64 within the sibling test's bound, bit-identical to `tile_m = 96` on the same image, and
    `mi_debug_last_conv_tile() == 192` on the family's route.  Every family runs a K with an odd number of K steps (3 or 5);
    the tap and encoder-conv loaders run, at both M, an odd count and K = 120 (Kpad 128, eight steps, padding inside the last
    one), the transposed conv K = 120 at M = 192; the two plain loaders (LINEAR + LN, 1 x 1 + GLU) need K == Kpad and have no K = 120.
    N is no multiple of 128 and just clears the under-fill threshold; rows are wider than their valid width with NaN in the
    padding and around the tensor, as in tests/test_gpu_x6_tap.py and test_gpu_x6_rows.py;
  * an under-filled call runs the 96-row tile, and item 1 alone equals item 1 inside a batch that ran the 192-row tile;
  * mi_set_split_bf16(0): the native route on conv_pick_tile(M), bit-identical to a call without an image;
  * non-finite isolation for the tap loader on the 192-row tile, 9 and 3 taps;
  * the route table through mi_debug_conv_route;
  * the engine: float32 htdemucs, max_batch = 2, two segments.
"""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from demucs_amd import _lib
from gpu_helpers import (EPI_CONVTR, EPI_GLU, EPI_LINEAR, FLAG_GELU, FLAG_RES, FLAG_TR_FREQ, conv_desc, ktab, maxerr, pack_vec,
                         pack_w, pick_tile)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAG_LN = 32
TABLE, DMA, DMATAP, DMAROW, X6, HALF, TAP_HALF, TAP_X6, ROWS_X6 = range(9)      # enum mi_conv_route (include/demucs_amd.h)
SLACK = 4096                           # floats on both sides of every input, NaN


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return _lib.load()


def rnd(*shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g, dtype=torch.float64) * scale


def _device_input(xp):
    """contiguous device view of xp inside a buffer whose SLACK floats on both sides hold NaN"""
    n = xp.numel()
    buf = torch.full((n + 2 * SLACK,), float("nan"), device="cuda")
    buf[SLACK:SLACK + n] = xp.float().reshape(-1).cuda()
    return buf[SLACK:SLACK + n]


def _padded(x, pitch):
    """x (..., T) -> (..., pitch) with NaN in the padding columns"""
    xp = torch.full(x.shape[:-1] + (pitch,), float("nan"), dtype=torch.float64)
    xp[..., :x.shape[-1]] = x
    return xp


def _image(lib, pack):
    """the layer's split image in the 96-row layout (what tile_m = 192 packs)"""
    wt, bias, M, Mpad, K, Kpad, tile = pack
    assert M % 192 == 0 and Mpad == M
    wx = torch.empty(6 * Kpad * Mpad, dtype=torch.uint8, device="cuda")
    _lib.check(lib.mi_conv_pack_split(wt.data_ptr(), Kpad, Mpad, 192, wx.data_ptr(), C.c_void_p(_lib.current_stream_ptr())), "pack")
    wx96 = torch.empty_like(wx)
    _lib.check(lib.mi_conv_pack_split(wt.data_ptr(), Kpad, Mpad, 96, wx96.data_ptr(), C.c_void_p(_lib.current_stream_ptr())), "pack")
    torch.cuda.synchronize()
    assert torch.equal(wx, wx96)
    return wx


def _launch(lib, kw, y, tile_m, wx):
    """-> (route, tile) of one mi_conv_forward of the layer `kw` into y"""
    kw = dict(kw, y=y, tile_m=tile_m)
    if wx is not None:
        kw["wx"] = wx
    d, keep = conv_desc(**kw)
    y.fill_(float("nan"))
    _lib.check(lib.mi_conv_forward(C.byref(d), C.c_void_p(_lib.current_stream_ptr())), "mi_conv_forward")
    torch.cuda.synchronize()
    return lib.mi_debug_last_conv_route(), lib.mi_debug_last_conv_tile()


# ---- the families: each builder returns (kw, y buffer, valid-output view of y, float64 expectation, pack) ------------------
def _fam_linear_ln(M, K, B, Tn, seed):
    """plain LINEAR with MI_FLAG_LN on tokens (B, K, Tn): the self-attention in_proj"""
    x = rnd(B, K, Tn, seed=seed)
    W, b = rnd(M, K, seed=seed + 1, scale=K ** -0.5), rnd(M, seed=seed + 2, scale=0.2)
    pack = pack_w(W, b)
    wt, bias, _, Mpad, _, Kpad, _ = pack
    xf = x.float().double()
    mean, rstd = xf.mean(1), 1.0 / torch.sqrt(xf.var(1, unbiased=False) + 1e-5)
    c1 = W.float().double().sum(1)
    stats = torch.stack([mean, rstd], -1).reshape(B * Tn, 2).float().cuda().contiguous()
    stf = stats.double().cpu().reshape(B, Tn, 2)
    acc = torch.einsum("mk,bkt->bmt", W, x)
    want = stf[:, None, :, 1] * (acc - stf[:, None, :, 0] * c1.float().double()[None, :, None]) + b[None, :, None]
    kw = dict(wt=wt, M=M, Mpad=Mpad, K=K, Kpad=Kpad, ktab=ktab(K, 1, 1, 1, 1, 0, 0, Tn, Tn, Kpad), x=_device_input(x),
              x_bstride=K * Tn, B=B, D1=1, D2=Tn, O1=1, O2=Tn, S1=1, S2=1, plain=1, epi=EPI_LINEAR, flags=FLAG_LN, bias=bias,
              y_bstride=M * Tn, y_cstride=Tn, pro_stats=stats, scale=pack_vec(c1, Mpad))
    y = torch.empty(B, M, Tn, device="cuda")
    return kw, y, y, want, pack


def _fam_tap(M, Cin, ntaps, B, Fr, T, pitch, seed, x=None):
    """stride-1 3 x 3 (ntaps 9) or k = 3 (ntaps 3) conv Cin -> M / 2 + GLU: the decoders' rewrites"""
    Co = M // 2
    shape = (M, Cin, 3, 3) if ntaps == 9 else (M, Cin, 1, 3)
    W, b = rnd(*shape, seed=seed, scale=0.5 / (Cin * ntaps) ** 0.5), rnd(M, seed=seed + 1, scale=0.2)
    pack = pack_w(W.reshape(M, -1), b, glu=True)
    wt, bias, _, Mpad, K, Kpad, _ = pack
    if x is None:
        x = rnd(B, Cin, Fr, T, seed=seed + 2)
    want = F.glu(F.conv2d(x, W, b, padding=1 if ntaps == 9 else (0, 1)), dim=1)
    P = Fr * pitch
    kw = dict(wt=wt, M=M, Mpad=Mpad, K=K, Kpad=Kpad, x=_device_input(_padded(x, pitch)), x_bstride=Cin * P, B=B, D1=Fr, D2=T, O1=Fr,
              O2=pitch, S1=1, S2=1, row_mode=1 if ntaps == 9 else 0, epi=EPI_GLU, bias=bias, y_bstride=Co * P, y_cstride=P,
              o2_valid=T if pitch != T else 0, x_ld=pitch if pitch != T else 0, ntaps=ntaps, tap_k2=3,
              tap_pad1=1 if ntaps == 9 else 0, tap_pad2=1)
    y = torch.empty(B, Co, Fr, pitch, device="cuda")
    return kw, y, y[..., :T], want, pack


def _fam_enc(M, Cin, B, Fr, T, pitch, seed):
    """Conv2d k = (8, 1), s = (4, 1), p = (2, 0) + GELU: the frequency branch's encoder convs"""
    W, b = rnd(M, Cin, 8, 1, seed=seed, scale=1.0 / (8 * Cin) ** 0.5), rnd(M, seed=seed + 1, scale=0.2)
    pack = pack_w(W.reshape(M, -1), b)
    wt, bias, _, Mpad, K, Kpad, _ = pack
    x = rnd(B, Cin, Fr, T, seed=seed + 2)
    want = F.gelu(F.conv2d(x, W, b, stride=(4, 1), padding=(2, 0)))
    P = Fr // 4 * pitch
    kw = dict(wt=wt, M=M, Mpad=Mpad, K=K, Kpad=Kpad, ktab=ktab(Cin, 8, 1, 1, 1, 2, 0, Fr * pitch, pitch, Kpad),
              x=_device_input(_padded(x, pitch)), x_bstride=Cin * Fr * pitch, B=B, D1=Fr, D2=T, O1=Fr // 4, O2=pitch, S1=4, S2=1,
              row_mode=1, epi=EPI_LINEAR, flags=FLAG_GELU, bias=bias, y_bstride=M * P, y_cstride=P, o2_valid=T if pitch != T else 0,
              x_ld=pitch if pitch != T else 0, dma_rows=1)
    y = torch.empty(B, M, Fr // 4, pitch, device="cuda")
    return kw, y, y[..., :T], want, pack


def _fam_convtr(M, Cc, B, Fr, T, skip_on, seed):
    """ConvTranspose2d k = (8, 1), s = (4, 1), cropped by 2 (+ GELU + skip): the frequency branch's transposed convs (rows of T floats,
    no pitch padding, as in tests/test_gpu_x6_rows.py)"""
    Co = M // 4
    W, b = rnd(Cc, Co, 8, 1, seed=seed, scale=1.0 / (2 * Cc) ** 0.5), rnd(Co, seed=seed + 1, scale=0.2)
    Wr = W.reshape(Cc, Co, 8)
    W2 = torch.zeros(4 * Co, 2 * Cc, dtype=torch.float64)       # row 4co+r, col 2ci+j  <- W[ci][co][r+4j]
    for r in range(4):
        for j in range(2):
            W2[r::4, j::2] = Wr[:, :, r + 4 * j].t()
    pack = pack_w(W2, b.repeat_interleave(4))
    wt, bias, _, Mpad, K, Kpad, _ = pack
    x = rnd(B, Cc, Fr, T, seed=seed + 2)
    skip = rnd(B, Co, 4 * Fr, T, seed=seed + 3) if skip_on else None
    want = F.conv_transpose2d(x, W, b, stride=(4, 1))[..., 2:-2, :]
    if skip_on:
        want = F.gelu(want) + skip
    flags = FLAG_TR_FREQ | (FLAG_GELU | FLAG_RES if skip_on else 0)
    kw = dict(wt=wt, M=M, Mpad=Mpad, K=K, Kpad=Kpad, ktab=ktab(Cc, 2, 1, -1, 1, 0, 0, Fr * T, T, Kpad), x=_device_input(x),
              x_bstride=Cc * Fr * T, B=B, D1=Fr, D2=T, O1=Fr + 1, O2=T, S1=1, S2=1, row_mode=1, epi=EPI_CONVTR, flags=flags,
              res=skip.float().cuda().contiguous() if skip_on else 0, bias=bias, y_bstride=Co * 4 * Fr * T, y_cstride=4 * Fr * T,
              out_len=4 * Fr, dma_rows=1)
    y = torch.empty(B, Co, 4 * Fr, T, device="cuda")
    return kw, y, y, want, pack


def _fam_glu1x1(M, Cin, B, Fr, T, pitch, seed):
    """1 x 1 conv Cin -> M / 2 + GLU, a plain layer on the row loader: the encoders' rewrites"""
    Co = M // 2
    W, b = rnd(M, Cin, 1, 1, seed=seed, scale=1.0 / Cin ** 0.5), rnd(M, seed=seed + 1, scale=0.2)
    pack = pack_w(W.reshape(M, -1), b, glu=True)
    wt, bias, _, Mpad, K, Kpad, _ = pack
    x = rnd(B, Cin, Fr, T, seed=seed + 2)
    want = F.glu(F.conv2d(x, W, b), dim=1)
    P = Fr * pitch
    kw = dict(wt=wt, M=M, Mpad=Mpad, K=K, Kpad=Kpad, ktab=ktab(Cin, 1, 1, 1, 1, 0, 0, P, P, Kpad), x=_device_input(_padded(x, pitch)),
              x_bstride=Cin * P, B=B, D1=1, D2=P, O1=1, O2=P, S1=1, S2=1, epi=EPI_GLU, bias=bias, y_bstride=Co * P, y_cstride=P,
              plain=1)
    y = torch.empty(B, Co, Fr, pitch, device="cuda")
    return kw, y, y[..., :T], want, pack


# N = 25 536 = 199.5 x 128 (M = 192: 1 x 200 workgroups) or 12 768 = 99.75 x 128 (M = 384: 2 x 100; M = 768: 6 384, 4 x 50): just at
# the threshold of 200, never a multiple of 128.  K: 80 = 5 K steps, 72 -> Kpad 80 (5 steps, padding in the last), 48 = 3 steps,
# 120 -> Kpad 128 (8 steps, padding in the last).  The parity of the step count decides which stage of the raw-tile ring the last
# transfer, fix-up and re-split touch, so every loader that admits it runs an odd count and K = 120 at both M
#        id                   builder                                                         route    bound    native route
FAMILIES = [
    ("linear_ln-192-k80",     lambda: _fam_linear_ln(192, 80, 3, 8512, 100),                  X6,      3e-5,    TABLE),
    ("linear_ln-384-k80",     lambda: _fam_linear_ln(384, 80, 3, 4256, 110),                  X6,      3e-5,    DMA),
    ("tap9-192-k72",          lambda: _fam_tap(192, 8, 9, 3, 8, 1061, 1064, 120),             TAP_X6,  2e-5,    DMATAP),
    ("tap9-384-k72",          lambda: _fam_tap(384, 8, 9, 3, 4, 1061, 1064, 130),             TAP_X6,  2e-5,    DMATAP),
    ("tap3-192-k120",         lambda: _fam_tap(192, 40, 3, 3, 1, 8509, 8512, 140),            TAP_X6,  2e-5,    DMATAP),
    ("tap3-384-k120",         lambda: _fam_tap(384, 40, 3, 3, 1, 4253, 4256, 150),            TAP_X6,  2e-5,    DMATAP),
    ("tap3-192-k72",          lambda: _fam_tap(192, 24, 3, 3, 1, 8509, 8512, 155),            TAP_X6,  2e-5,    DMATAP),
    ("tap3-384-k72",          lambda: _fam_tap(384, 24, 3, 3, 1, 4253, 4256, 157),            TAP_X6,  2e-5,    DMATAP),
    ("enc_gelu-192-k120",     lambda: _fam_enc(192, 15, 3, 16, 2125, 2128, 160),              ROWS_X6, 2e-5,    DMAROW),
    ("enc_gelu-192-k48",      lambda: _fam_enc(192, 6, 3, 16, 2125, 2128, 165),               ROWS_X6, 2e-5,    DMAROW),
    ("enc_gelu-384-k48",      lambda: _fam_enc(384, 6, 3, 16, 1061, 1064, 170),               ROWS_X6, 2e-5,    DMAROW),
    ("enc_gelu-384-k120",     lambda: _fam_enc(384, 15, 3, 16, 1061, 1064, 175),              ROWS_X6, 2e-5,    DMAROW),
    ("convtr-192-k120",       lambda: _fam_convtr(192, 60, 3, 7, 1064, False, 180),           ROWS_X6, 2e-5,    DMAROW),
    ("convtr-384-k48",        lambda: _fam_convtr(384, 24, 3, 3, 1064, False, 185),           ROWS_X6, 2e-5,    DMAROW),
    ("convtr_skip-384-k48",   lambda: _fam_convtr(384, 24, 3, 3, 1064, True, 190),            ROWS_X6, 2e-5,    DMAROW),
    ("convtr_skip-192-k48",   lambda: _fam_convtr(192, 24, 3, 7, 1064, True, 200),            ROWS_X6, 2e-5,    DMAROW),
    ("glu1x1-384-k80",        lambda: _fam_glu1x1(384, 80, 3, 4, 1061, 1064, 210),            ROWS_X6, 2e-5,    DMAROW),
    ("glu1x1-768-k48",        lambda: _fam_glu1x1(768, 48, 3, 2, 1061, 1064, 220),            ROWS_X6, 2e-5,    DMAROW),
]


@pytest.mark.parametrize("name,build,route,bound,native_route", FAMILIES, ids=[f[0] for f in FAMILIES])
def test_tile192_matches_float64_and_the_96_row_tile(lib, name, build, route, bound, native_route):
    kw, y, yv, want, pack = build()
    M = pack[2]
    N = kw["B"] * kw["O1"] * kw["O2"]
    assert M // 192 * -(-N // 128) >= 200 and N % 128 != 0
    wx = _image(lib, pack)
    got_rt = _launch(lib, kw, y, 192, wx)
    y192 = yv.cpu()
    assert got_rt == (route, 192), got_rt
    got_rt = _launch(lib, kw, y, 96, wx)
    y96 = yv.cpu()
    assert got_rt == (X6 if name.startswith("glu1x1") else route, 96), got_rt      # 1 x 1 + GLU on 96 rows: no row loader, the table
    nat_rt = _launch(lib, kw, y, pick_tile(M), None)
    ynat = yv.cpu()
    assert nat_rt == (native_route, pick_tile(M)), nat_rt
    err, err_nat = maxerr(y192, want), maxerr(ynat, want)
    print(f"{name}: N {N} split 192-row tile {err:.2e}, native fp32 {err_nat:.2e}")
    assert bool(torch.isfinite(y192).all())
    assert err < bound and err <= 3 * err_nat + 2e-6
    assert torch.equal(y192, y96)


UNDER = [("linear_ln", lambda B: _fam_linear_ln(384, 80, B, 4256, 300), X6),
         ("tap9", lambda B: _fam_tap(384, 8, 9, B, 4, 1061, 1064, 310), TAP_X6),
         ("tap3", lambda B: _fam_tap(192, 40, 3, B, 1, 8509, 8512, 320), TAP_X6),
         ("enc_gelu", lambda B: _fam_enc(192, 15, B, 16, 2125, 2128, 330), ROWS_X6),
         ("convtr_skip", lambda B: _fam_convtr(384, 24, B, 3, 1064, True, 340), ROWS_X6),
         ("glu1x1", lambda B: _fam_glu1x1(384, 80, B, 4, 1061, 1064, 350), ROWS_X6)]


@pytest.mark.parametrize("name,build,route", UNDER, ids=[u[0] for u in UNDER])
def test_under_filled_call_runs_96_rows_and_equals_the_batched_item(lib, name, build, route):
    """B = 3 clears the threshold (192-row tile); item 1 alone is under it: the 96-row tile on the same image, the same bits.  (The
    builders draw their tensors from seeded generators item by item, so item 1 of the batch is rebuilt by slicing.)"""
    kw, y, yv, want, pack = build(3)
    wx = _image(lib, pack)
    assert _launch(lib, kw, y, 192, wx) == (route, 192)
    batched = yv.cpu()[1:2]
    B = kw["B"]
    one = dict(kw, B=1)
    for key in ("x", "res"):
        if isinstance(kw.get(key), torch.Tensor):
            n = kw[key].numel() // B
            buf = torch.full((n + 2 * SLACK,), float("nan"), device="cuda")
            buf[SLACK:SLACK + n] = kw[key].reshape(-1)[n:2 * n]
            one[key] = buf[SLACK:SLACK + n]
    if "pro_stats" in kw:
        n = kw["pro_stats"].shape[0] // B
        one["pro_stats"] = kw["pro_stats"][n:2 * n].contiguous()
    y1 = torch.empty((1,) + tuple(y.shape[1:]), device="cuda")
    got_rt = _launch(lib, one, y1, 192, wx)
    assert got_rt == (route, 96), got_rt
    alone = y1[..., :yv.shape[-1]].cpu()
    assert torch.equal(alone, batched)


def test_split_switch_selects_native_route_on_the_layers_own_tile(lib):
    """mi_set_split_bf16(0): a tile_m = 192 descriptor WITH an image runs the native kernel on conv_pick_tile(M), bit-identical to a
    call without an image (tile_m = 192 and tile_m = conv_pick_tile(M) alike)."""
    for build, native_route in ((lambda: _fam_linear_ln(384, 80, 3, 4256, 400), DMA), (lambda: _fam_tap(192, 8, 9, 3, 8, 1061, 1064, 410), DMATAP),
                                (lambda: _fam_enc(384, 6, 3, 16, 1061, 1064, 420), DMAROW)):
        kw, y, yv, want, pack = build()
        M = pack[2]
        wx = _image(lib, pack)
        assert _launch(lib, kw, y, pick_tile(M), None) == (native_route, pick_tile(M))
        nat = yv.cpu()
        assert _launch(lib, kw, y, 192, None) == (native_route, pick_tile(M))
        assert torch.equal(yv.cpu(), nat)
        old = lib.mi_set_split_bf16(0)
        try:
            assert _launch(lib, kw, y, 192, wx) == (native_route, pick_tile(M))
            off = yv.cpu()
        finally:
            lib.mi_set_split_bf16(old)
        assert old == 1
        assert torch.equal(off, nat)
        assert _launch(lib, kw, y, 192, wx)[1] == 192


@pytest.mark.parametrize("ntaps,pitch_pad", [(9, 0), (9, 3), (3, 0), (3, 3)])
def test_tile192_tap_non_finite_isolation(lib, ntaps, pitch_pad):
    """As tests/test_gpu_x6_tap.py test_tap_split_non_finite_isolation, on the 192-row tile: NaN at the end of one input row and Inf
    at the start of another; outputs outside the receptive field of the poisoned samples equal the clean run bit for bit."""
    Cin, M, B = 8, 192, 3
    Fr, pitch = (8, 1064) if ntaps == 9 else (1, 8512)
    T = pitch - pitch_pad
    x = rnd(B, Cin, Fr, T, seed=500 + ntaps)
    kw, y, yv, want, pack = _fam_tap(M, Cin, ntaps, B, Fr, T, pitch, 510 + ntaps, x=x)
    wx = _image(lib, pack)
    assert _launch(lib, kw, y, 192, wx) == (TAP_X6, 192)
    clean = yv.cpu()
    xp = x.clone()
    hits = [(0, 5, Fr - 1, T - 1, float("nan")), (1, 7, 0, 0, float("inf")), (0, Cin - 1, Fr - 1, T - 1, float("nan")),
            (1, 0, 0, 0, float("-inf"))]
    if Fr > 1:
        hits += [(2, 3, 2, T - 1, float("nan")), (2, 3, 3, 0, float("inf"))]
    for bb, cc, rr, tt, v in hits:
        xp[bb, cc, rr, tt] = v
    kw2, y2, yv2, _, _ = _fam_tap(M, Cin, ntaps, B, Fr, T, pitch, 510 + ntaps, x=xp)
    assert _launch(lib, kw2, y2, 192, wx) == (TAP_X6, 192)
    got = yv2.cpu()
    mask = torch.ones(B, M // 2, Fr, T, dtype=torch.bool)
    for bb, cc, rr, tt, _ in hits:
        r0, r1 = (max(rr - 1, 0), min(rr + 2, Fr)) if ntaps == 9 else (rr, rr + 1)
        mask[bb, :, r0:r1, max(tt - 1, 0):min(tt + 2, T)] = False
    assert bool(torch.isfinite(got[mask]).all())
    assert torch.equal(got[mask], clean[mask])
    assert not bool(torch.isfinite(got[~mask]).all())         # the poison did reach the outputs that depend on it


# ---- the route table (host code only) ---------------------------------------------------------------------------------------
def _route(lib, d):
    tile = C.c_int(-1)
    return lib.mi_debug_conv_route(C.byref(d), C.byref(tile)), tile.value


def _desc(M, N, tile_m, image, kind="linear", Mpad=None, flags=FLAG_LN):
    """a descriptor for mi_debug_conv_route alone: no pointer is followed, so wx / ktab / x are just non-null, aligned numbers"""
    K = 64
    d = _lib.MiConvDesc()
    d.M, d.Mpad, d.K, d.Kpad, d.tile_m = M, Mpad or -(-M // pick_tile(M)) * pick_tile(M), K, K, tile_m
    d.B, d.S1, d.S2 = 1, 1, 1
    d.x, d.ktab, d.wx = 4096, 8192, 16384 if image else 0
    if kind == "linear":
        d.D1, d.D2, d.O1, d.O2, d.x_bstride, d.plain, d.epi, d.flags = 1, N, 1, N, K * N, 1, EPI_LINEAR, flags
    elif kind == "tap":                                  # 3 x 3 + GLU on 8 rows of N / 8
        Cin = 8
        d.K, d.Kpad = 72, 80
        d.D1, d.D2, d.O1, d.O2, d.x_bstride, d.epi = 8, N // 8, 8, N // 8, Cin * N, EPI_GLU
        d.ntaps, d.tap_k2, d.tap_pad1, d.tap_pad2 = 9, 3, 1, 1
    elif kind == "enc":                                  # k = 8, s = 4 along 16 rows + GELU
        d.D1, d.D2, d.O1, d.O2, d.S1, d.x_bstride, d.epi, d.flags, d.dma_rows = 16, N // 4, 4, N // 4, 4, 8 * 16 * (N // 4), EPI_LINEAR, FLAG_GELU, 1
    return d


def test_route_table(lib):
    big, small = 200 * 128, 60 * 128
    # tile_m 64 / 96 / 128 descriptors: unchanged
    assert _route(lib, _desc(512, big, 128, True)) == (X6, 128)
    assert _route(lib, _desc(512, 49 * 128, 128, True, flags=0)) == (X6, 64)
    assert _route(lib, _desc(384, big, 128, True)) == (X6, 128)
    assert _route(lib, _desc(384, small, 128, True)) == (X6, 64)
    assert _route(lib, _desc(192, big, 96, True)) == (X6, 96)
    assert _route(lib, _desc(192, big, 64, True, Mpad=192)) == (X6, 64)
    assert _route(lib, _desc(384, big, 128, True, kind="tap")) == (TAP_X6, 128)
    assert _route(lib, _desc(384, small, 128, True, kind="tap")) == (TAP_X6, 64)
    assert _route(lib, _desc(192, big, 96, True, kind="enc")) == (ROWS_X6, 96)
    # 192 with an image: filled -> 192, under-filled -> 96 (the threshold counts 192-row tiles)
    for kind, route in (("linear", X6), ("tap", TAP_X6), ("enc", ROWS_X6)):
        assert _route(lib, _desc(192, 200 * 128, 192, True, kind=kind)) == (route, 192)
        assert _route(lib, _desc(192, 199 * 128, 192, True, kind=kind)) == (route, 96)
        assert _route(lib, _desc(384, 100 * 128, 192, True, kind=kind)) == (route, 192)
        assert _route(lib, _desc(384, 99 * 128, 192, True, kind=kind)) == (route, 96)
    assert _route(lib, _desc(1536, 3000, 192, True)) == (X6, 96)           # 8 x 24 workgroups
    assert _route(lib, _desc(1536, 3200, 192, True)) == (X6, 192)          # 8 x 25
    # an epilogue the 192-row tile is not compiled for: the 96-row tile on the same image
    assert _route(lib, _desc(384, big, 192, True, flags=0)) == (X6, 96)
    # 192 without an image, or with the switch off: the native kernels on conv_pick_tile(M), as tile_m = 0
    for M, N, kind, want in ((384, big, "linear", (DMA, 128)), (192, big, "linear", (TABLE, 96)), (384, small, "linear", (TABLE, 64)),
                             (384, big, "tap", (DMATAP, 128)), (384, small, "tap", (DMATAP, 96)), (192, big, "enc", (DMAROW, 96))):
        assert _route(lib, _desc(M, N, 192, False, kind=kind)) == want == _route(lib, _desc(M, N, 0, False, kind=kind))
        old = lib.mi_set_split_bf16(0)
        try:
            assert _route(lib, _desc(M, N, 192, True, kind=kind)) == want
        finally:
            lib.mi_set_split_bf16(old)
    # M % 192 != 0 with tile_m = 192: rejected, and the error names it
    for M, Mpad in ((256, 256), (96, 96), (192, 384)):
        assert _route(lib, _desc(M, big, 192, True, Mpad=Mpad))[0] == -1
        msg = lib.mi_last_error().decode()
        assert "tile_m 192" in msg and "192 == 0" in msg, msg
    d = _desc(256, big, 192, True, flags=0)
    assert lib.mi_conv_forward(C.byref(d), None) != 0 and "tile_m 192" in lib.mi_last_error().decode()


# ---- the engine ---------------------------------------------------------------------------------------------------------
_ENGINE = r"""
import json
import sys
import numpy as np
import torch
from demucs_amd.htdemucs import HTDemucs
from demucs_amd.synth import synth_mix
from demucs_amd.weights import HTDemucsConfig, synthetic_state_dict
cfg = HTDemucsConfig()
m = HTDemucs(cfg.sources, max_batch=2)
m.load_state_dict(synthetic_state_dict(cfg, 0))
m.to("cuda").eval()
mix = torch.from_numpy(np.stack([synth_mix(3, cfg.segment_length, "tones"), synth_mix(4, cfg.segment_length, "tones")])).cuda()
m(mix)
m.profile_begin()
out = m(mix)
rows = m.profile_end()
# (route, tile) of the conv launches of one more forward: the hook runs after EVERY launch and reads what the last conv took
import ctypes as C
from demucs_amd import _lib
lib = _lib.load()
def census(x):
    seen = set()
    hook = C.CFUNCTYPE(None, C.c_void_p)(lambda st: seen.add((lib.mi_debug_last_conv_route(), lib.mi_debug_last_conv_tile())))
    lib.mi_debug_set_post_launch_hook(C.cast(hook, C.c_void_p))
    try:
        m(x)
        torch.cuda.synchronize()
    finally:
        lib.mi_debug_set_post_launch_hook(None)
    return sorted(seen)
tiles2 = census(mix)
one = torch.cat([m(mix[0:1]), m(mix[1:2])])
tiles1 = census(mix[1:2])
np.save(sys.argv[1] + ".npy", out.cpu().numpy())
np.save(sys.argv[1] + "_one.npy", one.cpu().numpy())
with open(sys.argv[1] + ".json", "w") as f:
    json.dump({"rows": {r["name"]: r["launches"] for r in rows}, "tiles2": tiles2, "tiles1": tiles1}, f, indent=0, sort_keys=True)
"""


def _engine_run(tmp_path, tag, env_extra):
    env = {k: v for k, v in os.environ.items() if k != "MI_X6"}
    env.update(env_extra, PYTHONPATH=ROOT)
    out = str(tmp_path / tag)
    r = subprocess.run([sys.executable, "-c", _ENGINE, out], env=env, capture_output=True, text=True, cwd=ROOT, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    return np.load(out + ".npy"), np.load(out + "_one.npy"), json.load(open(out + ".json"))


def test_engine_batch_of_two(tmp_path):
    """float32 htdemucs, max_batch = 2, two segments, one fresh process per setting: the default forward stays within the engine's
    1e-4 parity target of the MI_X6=0 forward; each item equals the B = 1 forward of the same handle bit for bit (the 192-row layers
    run 192 or 96 rows by their fill: asserted below from the tiles the launches took); the profiler's row names and launch counts
    are the ones recorded from the commit before the 192-row tile (tests/golden/x6_tile192_profile_rows.json), since rows stay keyed by conv_pick_tile(M)."""
    y_def, one_def, rep = _engine_run(tmp_path, "default", {})
    y_off, one_off, rep_off = _engine_run(tmp_path, "mi_x6_0", {"MI_X6": "0"})
    rows = rep["rows"]
    d = np.abs(y_def.astype(np.float64) - y_off).max()
    print(f"default vs MI_X6=0 forward, B = 2: max-abs {d:.3e}")
    assert 0 < d < 1e-4
    assert np.array_equal(y_def, one_def)
    assert np.array_equal(y_off, one_off)
    want = json.load(open(os.path.join(ROOT, "tests", "golden", "x6_tile192_profile_rows.json")))
    assert rows == want, {k: (rows.get(k), want.get(k)) for k in set(rows) | set(want) if rows.get(k) != want.get(k)}
    # The layers with M % 192 == 0 do state tile_m = 192.  The frequency branch's self-attention in_proj (M = 1536) have 8 x 42
    # workgroups at B = 2 and run the 192-row tile, 8 x 21 at B = 1 and run 96 rows (no other linear of the engine is anything but
    # a 128-row layer, so only they can show 96 rows on route 4).  On the tap and row-tap routes the outer layers (decoder 2:
    # M = 192 on 128 x 336 positions) fill the chip even at B = 1 and run 192 rows, the deep ones (decoder 0: M = 768 on 8 x 336) run
    # 96 at both sizes; a 128-row image would show there as the 128-row tile or the 64-row one.  MI_X6=0: no split route at all
    t2, t1 = {tuple(t) for t in rep["tiles2"]}, {tuple(t) for t in rep["tiles1"]}
    print(f"(route, tile) of the conv launches: B = 2 {sorted(t2)}, B = 1 {sorted(t1)}")
    assert (X6, 192) in t2 and (X6, 192) not in t1 and (X6, 96) in t1
    for t in (t2, t1):
        assert {tile for route, tile in t if route == TAP_X6} == {96, 192}, sorted(t)
        assert {tile for route, tile in t if route == ROWS_X6} == {96, 192}, sorted(t)
    assert not any(route in (X6, TAP_X6, ROWS_X6) for route, _ in {tuple(t) for t in rep_off["tiles2"] + rep_off["tiles1"]})
