"""The float32 time branch's strided encoder convs (Conv1d k = 8, s = 4, pad 2, + GELU) and transposed convs (ConvTranspose1d
k = 8, s = 4, cropped by 2, bare or + GELU + skip; two-tap GEMMs) on the split-bf16 main loop, fed by the time-axis LDS-DMA loaders
(gemm_x6.hip conv_time_enc_x6_kernel / conv_time_tr_x6_kernel, gemm_loop.h TimeEncTaps / TimeTrTaps, route 11), which the float32
htdemucs engine takes by default for tenc[1 .. 3].conv and tdec[0 .. 2].convtr.  The layers are described as the engine describes
them, `dma_time` set: the encoder's input rows on a pitch of round_up(L, 4) floats with D2 = L; the transposed conv's columns
q = 0 .. Lv on a pitch O2 = round_up(Lv + 1, 4) with o2_valid = Lv + 1.

  * against F.conv1d / F.conv_transpose1d in float64, no worse than three times the native table route's (route 0) error on the same
    call: 128-row layers on their own image (filled, and the 64-row small-batch tile), 96-row layers, 192-row layers on 96-row images
    (the 96-row and the 192-row tile), a pitch wider than the valid length, an output pitch equal to the valid width, item
    boundaries inside a tile, K padding in the last K step (an odd Cin: one real and one padding channel);
  * bit for bit: an item alone (small-batch tile) against the same item inside a filled batch; the 192-row tile against the 96-row
    tile on the same image; mi_set_split_bf16(0) gives route 0 and the bits of a call without an image; an output does not depend
    on the other items of its batch;
  * non-finite isolation: NaN / Inf in the pitch padding, in the memory around the tensor, in the neighbouring channel's first and
    last samples and in the neighbouring item never reach an output, while one inside a tap's reach does;
  * the engine: a default float32 forward runs exactly the three inner encoder convs and the three inner transposed convs of the
    time branch on this route, MI_X6=0 none, and both forwards stay within the engine's 1e-4 parity target of each other.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from demucs_amd import _lib
from gpu_helpers import EPI_CONVTR, EPI_LINEAR, FLAG_GELU, FLAG_RES, conv_desc, ktab, maxerr, pack_w, rup

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROUTE_TABLE, ROUTE_TIME_X6 = 0, 11     # mi_debug_last_conv_route: native table-driven gather, split-bf16 + time-axis DMA taps
SLACK = 4096                           # floats on both sides of the input, NaN


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return _lib.load()


def rnd(*shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g, dtype=torch.float64) * scale


def _device_input(xp, fill=float("nan")):
    n = xp.numel()
    buf = torch.full((n + 2 * SLACK,), fill, device="cuda")
    buf[SLACK:SLACK + n] = xp.float().reshape(-1).cuda()
    return buf[SLACK:SLACK + n]


def _layer(Cc, Co, seed):
    """-> (W (Cc, Co, 8), b, pack of the 4-phase GEMM: row 4 co + r, column 2 ci + j <- W[ci][co][r + 4 j])"""
    W, b = rnd(Cc, Co, 8, seed=seed, scale=1.0 / (2 * Cc) ** 0.5), rnd(Co, seed=seed + 1, scale=0.2)
    W2 = torch.zeros(4 * Co, 2 * Cc, dtype=torch.float64)
    for r in range(4):
        for j in range(2):
            W2[r::4, j::2] = W[:, :, r + 4 * j].t()
    return W, b, pack_w(W2, b.repeat_interleave(4))


def _image(lib, pack, tile):
    wt, bias, M, Mpad, K, Kpad, _ = pack
    wx = torch.empty(6 * Kpad * Mpad, dtype=torch.uint8, device="cuda")
    _lib.check(lib.mi_conv_pack_split(wt.data_ptr(), Kpad, Mpad, tile, wx.data_ptr(), C.c_void_p(_lib.current_stream_ptr())), "pack")
    torch.cuda.synchronize()
    return wx


def _want(x, W, b, skip):
    y = F.conv_transpose1d(x, W, b, stride=4)[..., 2:-2]
    return y if skip is None else F.gelu(y) + skip


def _run(lib, x, pack, skip, pitch, mode, xp=None):
    """x (B, Cc, Lv) on rows of `pitch` floats (NaN in the padding, NaN around the tensor) -> (outputs (B, Co, 4 Lv) on the host,
    route, tile).  mode: None = no image; "own" = the image of the layer's own tile; 192 = the 96-row images as a tile_m = 192
    layer; 96 = the same images as a 96-row layer."""
    B, Cc, Lv = x.shape
    wt, bias, M, Mpad, K, Kpad, tile = pack
    Co = M // 4
    if xp is None:
        xp = torch.full((B, Cc, pitch), float("nan"), dtype=torch.float64)
        xp[..., :Lv] = x
    kw = dict(wt=wt, M=M, Mpad=Mpad, K=K, Kpad=Kpad, ktab=ktab(Cc, 1, 2, 1, -1, 0, 0, pitch, pitch, Kpad), x=_device_input(xp),
              x_bstride=Cc * pitch, B=B, D1=1, D2=Lv, O1=1, O2=rup(Lv + 1, 4), o2_valid=Lv + 1, S1=1, S2=1, epi=EPI_CONVTR,
              flags=FLAG_GELU | FLAG_RES if skip is not None else 0, res=skip.float().cuda().contiguous() if skip is not None else 0,
              bias=bias, y_bstride=Co * 4 * Lv, y_cstride=4 * Lv, out_len=4 * Lv, x_ld=pitch if pitch != Lv else 0, dma_time=1,
              tile_m=tile if mode in (None, "own") else mode)
    if mode is not None:
        kw["wx"] = _image(lib, pack, tile if mode == "own" else 96)
    y = torch.full((B, Co, 4 * Lv), float("nan"), device="cuda")
    d, keep = conv_desc(**kw, y=y)
    _lib.check(lib.mi_conv_forward(C.byref(d), C.c_void_p(_lib.current_stream_ptr())), "mi_conv_forward")
    torch.cuda.synchronize()
    return y.cpu(), lib.mi_debug_last_conv_route(), lib.mi_debug_last_conv_tile()


#        Cc   Co   B   Lv    pitch mode   tile the kernel runs
CASES = [(384, 192, 2, 1344, 1344, 192, 96),     # tdec[0]'s shape (M = 768, K = 768): under-filled, the 96-row tile; pitch == Lv
         (192, 96, 3, 37, 40, 192, 96),          # M = 384, pitch 40 > 37 (NaN padding), N = 120: item boundaries inside a tile
         (192, 96, 3, 37, 40, "own", 64),        # the same layer as a 128-row layer: the small-batch tile on the 128-row image
         (96, 48, 2, 336, 336, 192, 96),         # tdec[2]'s channels (M = 192): the 96-row tile
         (96, 48, 76, 336, 336, 192, 192),       # ... at a batch that fills the chip: the 192-row tile (200 workgroups)
         (192, 96, 1, 336, 336, "own", 64),      # B = 1: the small-batch tile
         (192, 96, 25, 336, 340, "own", 128),    # the 128-row tile, filled (3 x 67 workgroups)
         (36, 32, 2, 131, 132, "own", 64)]       # K = 72 in Kpad 80: K padding in the last K step; N = 264, odd valid length


@pytest.mark.parametrize("skip_on", [False, True], ids=["bare", "gelu_skip"])
@pytest.mark.parametrize("Cc,Co,B,Lv,pitch,mode,runs", CASES)
def test_time_transposed_conv_matches_float64(lib, Cc, Co, B, Lv, pitch, mode, runs, skip_on):
    W, b, pack = _layer(Cc, Co, seed=30 + Cc)
    x = rnd(B, Cc, Lv, seed=40 + Cc + Lv)
    skip = rnd(B, Co, 4 * Lv, seed=41) if skip_on else None
    want = _want(x, W, b, skip)
    got, route, tile = _run(lib, x, pack, skip, pitch, mode)
    assert (route, tile) == (ROUTE_TIME_X6, runs)
    nat, route_nat, _ = _run(lib, x, pack, skip, pitch, None)
    assert route_nat == ROUTE_TABLE
    err, err_nat = maxerr(got, want), maxerr(nat, want)
    print(f"time convtr Cc {Cc} Co {Co} B {B} Lv {Lv} pitch {pitch} skip {skip_on} tile {tile}: split {err:.2e}, native fp32 {err_nat:.2e}")
    assert bool(torch.isfinite(got).all())
    assert err < 2e-5 and err <= 3 * err_nat + 2e-6


# ---- encoder conv: Conv1d k = 8, s = 4, pad 2, + GELU ------------------------------------------------------------
def _enc_layer(Cin, Cout, seed):
    W, b = rnd(Cout, Cin, 8, seed=seed, scale=1.0 / (8 * Cin) ** 0.5), rnd(Cout, seed=seed + 1, scale=0.2)
    return W, b, pack_w(W.reshape(Cout, -1), b)


def _enc_want(x, W, b):
    L = x.shape[-1]
    return F.gelu(F.conv1d(F.pad(x, (0, rup(L, 4) - L)), W, b, stride=4, padding=2))


def _enc_run(lib, x, pack, mode, xp=None):
    """x (B, Cin, L) on rows of round_up(L, 4) floats (NaN in the padding, NaN around the tensor) -> (valid outputs (B, Cout,
    ceil(L / 4)) on the host, route, tile).  mode as for _run."""
    B, Cin, L = x.shape
    wt, bias, M, Mpad, K, Kpad, tile = pack
    pitch, Lo = rup(L, 4), (L + 3) // 4
    O2 = rup(Lo, 4)
    if xp is None:
        xp = torch.full((B, Cin, pitch), float("nan"), dtype=torch.float64)
        xp[..., :L] = x
    kw = dict(wt=wt, M=M, Mpad=Mpad, K=K, Kpad=Kpad, ktab=ktab(Cin, 1, 8, 1, 1, 0, 2, pitch, pitch, Kpad), x=_device_input(xp),
              x_bstride=Cin * pitch, B=B, D1=1, D2=L, O1=1, O2=O2, o2_valid=Lo if O2 != Lo else 0, S1=1, S2=4, epi=EPI_LINEAR,
              flags=FLAG_GELU, bias=bias, y_bstride=M * O2, y_cstride=O2, x_ld=pitch if pitch != L else 0, dma_time=1,
              tile_m=tile if mode in (None, "own") else mode)
    if mode is not None:
        kw["wx"] = _image(lib, pack, tile if mode == "own" else 96)
    y = torch.full((B, M, O2), float("nan"), device="cuda")
    d, keep = conv_desc(**kw, y=y)
    _lib.check(lib.mi_conv_forward(C.byref(d), C.c_void_p(_lib.current_stream_ptr())), "mi_conv_forward")
    torch.cuda.synchronize()
    return y[..., :Lo].cpu(), lib.mi_debug_last_conv_route(), lib.mi_debug_last_conv_tile()


#            Cin  Cout B  L      mode   tile the kernel runs
ENC_CASES = [(48, 96, 2, 1021, "own", 96),      # 96 rows; output pitch 256 == valid width: the last valid column's taps 4 .. 7 meet the next item
             (96, 192, 3, 402, 192, 96),        # M = 192, under-filled: the 96-row tile; valid 101 in pitch 104; N = 312: item boundaries in a tile
             (192, 384, 4, 12800, 192, 192),    # the 192-row tile, filled (2 x 100 workgroups)
             (192, 384, 1, 5375, 192, 96),      # tenc[3]'s shape at B = 1: the small-batch tile
             (5, 96, 2, 61, "own", 96),         # K = 40 in Kpad 48: one real and one padding channel in the last K step
             (24, 128, 3, 149, "own", 64)]      # 128-row image, 64-row tile


@pytest.mark.parametrize("Cin,Cout,B,L,mode,runs", ENC_CASES)
def test_time_encoder_conv_matches_float64(lib, Cin, Cout, B, L, mode, runs):
    W, b, pack = _enc_layer(Cin, Cout, seed=10 + Cin)
    x = rnd(B, Cin, L, seed=20 + Cin)
    want = _enc_want(x, W, b)
    got, route, tile = _enc_run(lib, x, pack, mode)
    assert (route, tile) == (ROUTE_TIME_X6, runs)
    nat, route_nat, _ = _enc_run(lib, x, pack, None)
    assert route_nat == ROUTE_TABLE
    err, err_nat = maxerr(got, want), maxerr(nat, want)
    print(f"time enc Cin {Cin} Cout {Cout} B {B} L {L} tile {tile}: split {err:.2e}, native fp32 {err_nat:.2e}")
    assert got.shape == want.shape and bool(torch.isfinite(got).all())
    assert err < 2e-5 and err <= 3 * err_nat + 2e-6


# ---- bit identity ----------------------------------------------------------------------------------------------
def test_time_encoder_single_item_equals_batched(lib):
    """Item 9 of a batch that fills the chip with 128-row tiles (200 workgroups), alone (the 64-row tile on the 128-row image)."""
    Cin, Cout, B, L = 24, 128, 64, 1597
    W, b, pack = _enc_layer(Cin, Cout, seed=80)
    x = rnd(B, Cin, L, seed=81)
    batched, route, tile = _enc_run(lib, x, pack, "own")
    assert (route, tile) == (ROUTE_TIME_X6, 128)
    alone, route, tile = _enc_run(lib, x[9:10], pack, "own")
    assert (route, tile) == (ROUTE_TIME_X6, 64)
    assert torch.equal(batched[9:10], alone)


def test_time_encoder_tile192_equals_tile96(lib):
    Cin, Cout, B, L = 96, 192, 64, 1600
    W, b, pack = _enc_layer(Cin, Cout, seed=82)
    x = rnd(B, Cin, L, seed=83)
    wide, route, tile = _enc_run(lib, x, pack, 192)
    assert (route, tile) == (ROUTE_TIME_X6, 192)
    narrow, route, tile = _enc_run(lib, x, pack, 96)
    assert (route, tile) == (ROUTE_TIME_X6, 96)
    assert torch.equal(wide, narrow)
    alone, route, tile = _enc_run(lib, x[5:6], pack, 192)      # under-filled: the 96-row tile
    assert (route, tile) == (ROUTE_TIME_X6, 96)
    assert torch.equal(wide[5:6], alone)


def test_time_single_item_equals_batched(lib):
    """Item 7 of a batch that fills the chip with 128-row tiles, alone (the 64-row tile reading the 128-row image)."""
    Cc, Co, B, Lv = 192, 96, 25, 336
    W, b, pack = _layer(Cc, Co, seed=50)
    x, skip = rnd(B, Cc, Lv, seed=51), rnd(B, Co, 4 * Lv, seed=52)
    batched, route, tile = _run(lib, x, pack, skip, Lv, "own")
    assert (route, tile) == (ROUTE_TIME_X6, 128)
    alone, route, tile = _run(lib, x[7:8], pack, skip[7:8], Lv, "own")
    assert (route, tile) == (ROUTE_TIME_X6, 64)
    assert torch.equal(batched[7:8], alone)


def test_time_tile192_equals_tile96(lib):
    Cc, Co, B, Lv = 96, 48, 76, 336
    W, b, pack = _layer(Cc, Co, seed=53)
    x, skip = rnd(B, Cc, Lv, seed=54), rnd(B, Co, 4 * Lv, seed=55)
    wide, route, tile = _run(lib, x, pack, skip, Lv, 192)
    assert (route, tile) == (ROUTE_TIME_X6, 192)
    narrow, route, tile = _run(lib, x, pack, skip, Lv, 96)
    assert (route, tile) == (ROUTE_TIME_X6, 96)
    assert torch.equal(wide, narrow)
    alone, route, tile = _run(lib, x[5:6], pack, skip[5:6], Lv, 192)      # under-filled: the 96-row tile
    assert (route, tile) == (ROUTE_TIME_X6, 96)
    assert torch.equal(wide[5:6], alone)


def test_split_switch_selects_the_table_route(lib):
    """mi_set_split_bf16(0) sends the layer WITH an image to the table-driven native kernel, bit-identical to a call without one."""
    Cc, Co, B, Lv, pitch = 192, 96, 2, 101, 104
    W, b, pack = _layer(Cc, Co, seed=56)
    x, skip = rnd(B, Cc, Lv, seed=57), rnd(B, Co, 4 * Lv, seed=58)
    We, be, packe = _enc_layer(96, 192, seed=66)
    xe = rnd(2, 96, 402, seed=67)
    nat, route, _ = _run(lib, x, pack, skip, pitch, None)
    assert route == ROUTE_TABLE
    nate, route, _ = _enc_run(lib, xe, packe, None)
    assert route == ROUTE_TABLE
    old = lib.mi_set_split_bf16(0)
    try:
        off, route, _ = _run(lib, x, pack, skip, pitch, 192)
        assert route == ROUTE_TABLE
        offe, route, _ = _enc_run(lib, xe, packe, 192)
        assert route == ROUTE_TABLE
    finally:
        lib.mi_set_split_bf16(old)
    assert old == 1
    assert torch.equal(off, nat) and torch.equal(offe, nate)
    _, route, _ = _run(lib, x, pack, skip, pitch, 192)
    assert route == ROUTE_TIME_X6
    _, route, _ = _enc_run(lib, xe, packe, 192)
    assert route == ROUTE_TIME_X6


def test_time_output_does_not_depend_on_other_items(lib):
    Cc, Co, B, Lv, pitch = 96, 48, 3, 37, 40
    W, b, pack = _layer(Cc, Co, seed=59)
    x = rnd(B, Cc, Lv, seed=60)
    first, route, _ = _run(lib, x, pack, None, pitch, 192)
    assert route == ROUTE_TIME_X6
    x2 = rnd(B, Cc, Lv, seed=61, scale=3.0)
    x2[1] = x[1]
    second, route, _ = _run(lib, x2, pack, None, pitch, 192)
    assert route == ROUTE_TIME_X6
    assert torch.equal(first[1], second[1]) and not torch.equal(first[0], second[0])
    We, be, packe = _enc_layer(48, 96, seed=62)
    xe = rnd(B, 48, 149, seed=63)
    first, route, _ = _enc_run(lib, xe, packe, "own")
    assert route == ROUTE_TIME_X6
    xe2 = rnd(B, 48, 149, seed=64, scale=3.0)
    xe2[1] = xe[1]
    second, route, _ = _enc_run(lib, xe2, packe, "own")
    assert route == ROUTE_TIME_X6
    assert torch.equal(first[1], second[1]) and not torch.equal(first[0], second[0])


# ---- non-finite isolation --------------------------------------------------------------------------------------
@pytest.mark.parametrize("Lv,pitch", [(37, 40), (36, 36), (39, 40)])
def test_time_non_finite_isolation(lib, Lv, pitch):
    """Output 4 q + r - 2 reads samples q and q - 1 of every channel of its item.  The pitch padding and the memory around the tensor
    hold NaN.  Poisoned first and last samples of channels sit where the neighbouring channel's (or item's) tap -1 of column 0 and
    tap 0 of column Lv would read (pitch == Lv: directly; else behind the padding): they change only the outputs of their own
    columns."""
    Cc, Co, B = 48, 32, 3
    W, b, pack = _layer(Cc, Co, seed=70)
    x = rnd(B, Cc, Lv, seed=71)
    clean, route, _ = _run(lib, x, pack, None, pitch, "own")
    assert route == ROUTE_TIME_X6
    hits = [(0, Cc - 1, Lv - 1, float("nan")),      # before item 1's channel 0
            (1, 0, 0, float("inf")),                # after item 0's last channel
            (1, 7, Lv - 1, float("-inf")), (1, 9, 0, float("nan")),       # neighbours of channels 8 / 8 inside an item
            (2, Cc - 1, Lv - 1, float("nan")),      # the tensor's last sample
            (2, 5, 17, float("nan"))]
    xp = torch.full((B, Cc, pitch), float("nan"), dtype=torch.float64)
    xp[..., :Lv] = x
    for bb, cc, ii, v in hits:
        xp[bb, cc, ii] = v
    got, route, _ = _run(lib, x, pack, None, pitch, "own", xp=xp)
    assert route == ROUTE_TIME_X6
    mask = torch.ones(B, Co, 4 * Lv, dtype=torch.bool)
    for bb, cc, ii, _ in hits:
        for q in (ii, ii + 1):               # sample ii is tap j = 0 of q = ii and tap j = 1 of q = ii + 1
            for r in range(4):
                o = 4 * q + r - 2
                if 0 <= o < 4 * Lv:
                    mask[bb, :, o] = False
    assert bool(torch.isfinite(got[mask]).all())
    assert torch.equal(got[mask], clean[mask])
    assert not bool(torch.isfinite(got[~mask]).any())         # the poison reached every output that depends on it


@pytest.mark.parametrize("L", [149, 148, 61, 1021])
def test_time_encoder_non_finite_isolation(lib, L):
    """Output o reads samples 4 o - 2 .. 4 o + 5 of every channel of its item.  The pitch padding (L % 4 != 0) and the memory around
    the tensor hold NaN.  Poisoned first and last samples of channels sit where the neighbouring channel's (or item's) samples -2, -1
    of column 0 and the samples past the end of the last column would be read (L % 4 == 0: directly; else behind the padding).
    L = 1021: the output pitch 256 equals the valid width, so the column after an item's last one is the next item's first."""
    Cin, Cout, B = 48, 128, 3
    W, b, pack = _enc_layer(Cin, Cout, seed=74)
    x = rnd(B, Cin, L, seed=75)
    clean, route, _ = _enc_run(lib, x, pack, "own")
    assert route == ROUTE_TIME_X6
    hits = [(0, Cin - 1, L - 1, float("nan")), (1, 0, 0, float("inf")), (1, 0, 1, float("nan")), (1, 7, L - 1, float("-inf")),
            (1, 7, L - 2, float("nan")), (1, 9, 0, float("nan")), (2, Cin - 1, L - 1, float("nan")), (2, 5, 17, float("nan"))]
    pitch = rup(L, 4)
    xp = torch.full((B, Cin, pitch), float("nan"), dtype=torch.float64)
    xp[..., :L] = x
    for bb, cc, ii, v in hits:
        xp[bb, cc, ii] = v
    got, route, _ = _enc_run(lib, x, pack, "own", xp=xp)
    assert route == ROUTE_TIME_X6
    Lo = (L + 3) // 4
    mask = torch.ones(B, Cout, Lo, dtype=torch.bool)
    for bb, cc, ii, _ in hits:
        for o in range(Lo):
            if 4 * o - 2 <= ii <= 4 * o + 5:
                mask[bb, :, o] = False
    assert bool(torch.isfinite(got[mask]).all())
    assert torch.equal(got[mask], clean[mask])
    assert not bool(torch.isfinite(got[~mask]).any())         # the poison reached every output that depends on it


# ---- the engine's default ----------------------------------------------------------------------------------------
_ENGINE = r"""
import sys
import numpy as np
import torch
from demucs_amd import _lib
from demucs_amd.htdemucs import HTDemucs
from demucs_amd.synth import synth_mix
from demucs_amd.weights import HTDemucsConfig, synthetic_state_dict
lib = _lib.load()
cfg = HTDemucsConfig()
m = HTDemucs(cfg.sources, max_batch=1)
m.load_state_dict(synthetic_state_dict(cfg, 0))
m.to("cuda").eval()
mix = torch.from_numpy(synth_mix(3, cfg.segment_length, "tones"))[None].cuda()
m(mix)
before = [lib.mi_debug_conv_route_launches(11, e) for e in (0, 5, -1)]      # LINEAR, CONVTR, any epilogue
m.profile_begin()
out = m(mix)
rows = m.profile_end()
after = [lib.mi_debug_conv_route_launches(11, e) for e in (0, 5, -1)]
np.save(sys.argv[1] + ".npy", out.cpu().numpy())
with open(sys.argv[1] + ".txt", "w") as f:
    f.write("route11 " + " ".join(str(a - b) for a, b in zip(after, before)) + "\n")
    for r in rows:
        f.write(f"{r['name']} {r['launches']}\n")
"""


def _engine_run(tmp_path, tag, env_extra):
    env = {k: v for k, v in os.environ.items() if not k.startswith("MI_")}
    env.update(env_extra, PYTHONPATH=ROOT)
    out = str(tmp_path / tag)
    r = subprocess.run([sys.executable, "-c", _ENGINE, out], env=env, capture_output=True, text=True, cwd=ROOT, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    lines = open(out + ".txt").read().splitlines()
    counts = tuple(int(v) for v in lines[0].split()[1:])
    rows = {}
    for line in lines[1:]:
        name, n = line.rsplit(" ", 1)
        rows[name] = int(n)
    return np.load(out + ".npy"), counts, rows


def test_engine_default_runs_time_convs_on_the_split_loop(tmp_path):
    """float32 htdemucs forward, one fresh process each.  By default one forward launches exactly three LINEAR layers
    (tenc[1 .. 3].conv) and three CONVTR layers (tdec[0 .. 2].convtr) on route 11 and nothing else there
    (mi_debug_conv_route_launches around the forward); MI_X6=0 none.  The layers keep the profiler rows they had on the table route
    (the recorded launch census lists every row), which in the default engine hold just these six launches.  Both forwards are
    within the engine's 1e-4 parity target of each other."""
    native = ("conv_gemm<convtr,tile128>", "conv_gemm<convtr,tile96>", "conv_gemm<linear,tile128>", "conv_gemm<linear,tile96>")
    y_def, counts, rows_def = _engine_run(tmp_path, "default", {})
    assert counts == (3, 3, 6), counts
    assert [rows_def.get(k) for k in native] == [2, 1, 1, 2], rows_def
    y_off, counts_off, rows_off = _engine_run(tmp_path, "mi_x6_0", {"MI_X6": "0"})
    assert counts_off == (0, 0, 0), counts_off
    assert [rows_off.get(k) for k in native] == [4, 2, 2, 4], rows_off
    d = np.abs(y_def.astype(np.float64) - y_off).max()
    print(f"default vs MI_X6=0: max-abs {d:.3e}")
    assert d < 1e-4
