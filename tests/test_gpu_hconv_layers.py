"""The conv / linear layers that only the Hybrid Demucs engine builds (demucs_amd/csrc/hmodel.hip hforward_impl, run_deep), each
alone through `mi_conv_forward` against float64 CPU math written from the reference model's definition (demucs/hdemucs.py HEncLayer /
HDecLayer: F.conv1d, F.conv2d, F.conv_transpose1d, F.conv_transpose2d, F.pad) -- not from the engine's phase algebra.

Every descriptor is built field by field as hmodel.hip builds it (base_desc + the fields the layer overrides), nothing else set:
  A  un-cropped transposed convs (EPI_CONVTR with tr_stride / tr_pad): decoder.0 (k 4, s 2: the LG = 1 scatter with cout = M >> 1),
     tdecoder.0 (k 8, s 4, pad 0), decoder.1 (one frequency row to eight, MI_FLAG_TR_FREQ), and the cropped conv spelled both ways;
  B  the strided convs of layers 4 and 5: encoder.5 (k 4, s 2, p 1, right padding only as the gather's D2 bound), encoder.4's merge
     conv (8 pitched rows -> 1, + the injected tencoder.4 output), tencoder.4 (k 8, s 4, p 2, no GELU, pitched input);
  C  the deep DConv's plain linears: LocalState's q / k / content projection (M = 3 H + 16 < Mpad on a row pitch round_up(Tn, 4))
     and the BLSTM's input projection (B * F items of W columns) and output linear (+ residual).

Every case runs in the four main loops (native fp32 MFMA, split-bf16, bf16, fp16).  In the half modes `rnd` draws values that are
exact in bf16 and fp16, so the float32 bound applies unchanged: 2e-5, the bound tests/test_gpu_kernels.py uses for the same kernels
against float64 (inputs O(1), weights scaled by K ** -0.5, K <= 64 here).

Each case asserts
  * the route: `mi_debug_conv_route` before the launch and `mi_debug_last_conv_route` / `mi_debug_last_conv_tile` after it equal
    the literal (route, tile) written beside the shape -- derived by hand from conv_route.hip, one per main loop:
        native TABLE 32   A1 M 16, C2 output linear (also with the split switch on: a 32-row layer has no split image)
        native TABLE 64   the M 40 cases of A1-A3 and B1-B3, A4; under-filled plain linears: C1 Tn 76, C2 input projection W 200
        native TABLE 96   A1 M 96, B1 T 2, B2 C 96
        native TABLE 128  the M 128 cases of A1-A3 and B1-B3, C1 Tn 37 and C2 input projection W 37 (P % 4 != 0: not plain)
        native DMA 128    C1 Tn 12800: 200 workgroups, M 112 < Mpad 128
        X6 64 / 96 / 128  the cases of native TABLE 64 / 96 / 128; C1 Tn 12800 on 128
        HALF 32 / 64 / 96 / 128   the cases of native TABLE on that tile, except: C1 Tn 76 and Tn 12800 on 128 (no small-batch tile)
        HALF 256          C2 input projection W 200 (plain LINEAR, Mpad 256);
  * the result against float64 under 2e-5, every position the reference defines finite (the output is NaN before the launch);
  * the guard words: the output lies inside a larger device buffer prefilled with a bit pattern, 256 words on each side and, for
    C1, the pitch columns of every row -- all still hold the pattern bit for bit;
  * item isolation: item b of the batched call equals bit for bit the B = 1 call on item b alone (column decomposition across
    item boundaries inside a wave's 32 columns and inside a 128-column tile).
"""
import ctypes as C
import math

import pytest
import torch
import torch.nn.functional as F

from demucs_amd import _lib
from gpu_helpers import (EPI_CONVTR, EPI_LINEAR, FLAG_GELU, FLAG_RES, FLAG_TR_FREQ, conv_desc, ktab, maxerr, pack_w, rup)

pytestmark = pytest.mark.gpu

TABLE, DMA, X6, HALF = 0, 1, 4, 5      # enum mi_conv_route (include/demucs_amd.h)
TOL = 2e-5
GUARD = 256                            # words on each side of the output
PATTERN = 0x4B1D4B1D                   # as a float: finite, about 1.03e7


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return _lib.load()


_HALF_MODE = [None]      # set by the `x6` fixture: "bf16" / "f16" while a reduced-precision case runs


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    t = torch.randn(*shape, generator=g, dtype=torch.float64) * scale
    if _HALF_MODE[0]:
        # values exactly representable in bf16 AND fp16: the operand rounding of the reduced-precision GEMMs is then the
        # identity, products are exact in float32, and the SAME tolerance as the float32 kernels applies to them
        t = t.float().bfloat16().double()
        t = torch.where(t.abs() < 2.0 ** -14, torch.zeros_like(t), t)
    return t


@pytest.fixture(params=[False, True, "bf16", "f16"], ids=["fp32mfma", "bf16x6", "bf16", "f16"])
def x6(request):
    """Every GEMM main loop: native fp32 MFMA, the exact 3-term bf16 split (gemm_x6.hip), bf16 / fp16 operands (gemm_half.hip)."""
    _HALF_MODE[0] = request.param if isinstance(request.param, str) else None
    yield request.param
    _HALF_MODE[0] = None


def routes(tile, split=None, native=None, half=None):
    """(native, split-bf16, half) literals of a case: TABLE / X6 / HALF on `tile` unless stated."""
    return (native or (TABLE, tile), split or (X6, tile), half or (HALF, tile))


def expected(rt, mode):
    return rt[2] if isinstance(mode, str) else rt[1] if mode else rt[0]


class Guarded:
    """An output tensor of `shape` (last dim: the row pitch, `valid` real columns) inside a pattern-filled device buffer."""

    def __init__(self, shape, valid=None):
        n = math.prod(shape)
        self.buf = torch.full((GUARD + n + GUARD,), PATTERN, dtype=torch.int32, device="cuda")
        self.ints = self.buf[GUARD:GUARD + n].view(shape)
        self.y = self.ints.view(torch.float32)
        self.cols = shape[-1] if valid is None else valid
        self.y[..., :self.cols] = float("nan")
        self.n = n

    def check(self, what):
        torch.cuda.synchronize()
        assert bool((self.buf[:GUARD] == PATTERN).all()), f"{what}: the {GUARD} guard words BEFORE the output were written"
        assert bool((self.buf[GUARD + self.n:] == PATTERN).all()), f"{what}: the {GUARD} guard words AFTER the output were written"
        assert bool((self.ints[..., self.cols:] == PATTERN).all()), f"{what}: pitch columns of the output rows were written"
        got = self.y[..., :self.cols].cpu()
        assert bool(torch.isfinite(got).all()), (f"{what}: {int((~torch.isfinite(got)).sum())} positions the reference defines are not finite "
                                                 "(never written, or computed from a NaN pitch column)")
        return got


def launch(lib, mode, want, kw, what):
    d, keep = conv_desc(x6=mode, **kw)
    tile = C.c_int(-1)
    before = (lib.mi_debug_conv_route(C.byref(d), C.byref(tile)), tile.value)
    if want is not None:
        assert before == want, f"{what}: conv_route answers {before} for the descriptor, the case expects {want}"
    _lib.check(lib.mi_conv_forward(C.byref(d), C.c_void_p(_lib.current_stream_ptr())), "mi_conv_forward")
    torch.cuda.synchronize()
    after = (lib.mi_debug_last_conv_route(), lib.mi_debug_last_conv_tile())
    assert after == before, f"{what}: launched {after}, conv_route said {before}"
    del keep


def check_layer(lib, mode, rt, what, x, res, want, item_shape, desc, valid=None):
    """desc(B, x, res, y) -> the descriptor's keyword arguments for B items; want (B, *item_shape[:-1], valid) float64."""
    B = x.shape[0]
    xd = x.float().cuda().contiguous()
    rd = res.float().cuda().contiguous() if res is not None else None
    g = Guarded((B, *item_shape), valid)
    launch(lib, mode, expected(rt, mode), desc(B, xd, rd, g.y), what)
    got = g.check(what)
    err = maxerr(got, want)
    print(f"{what} [{mode}]: route {expected(rt, mode)}, max error vs float64 {err:.3e}")
    assert err < TOL, f"{what}: max error {err:.3e} vs float64"
    for b in range(B):
        g1 = Guarded((1, *item_shape), valid)
        launch(lib, mode, None, desc(1, xd[b:b + 1].clone(), rd[b:b + 1].clone() if rd is not None else None, g1.y), f"{what} item {b} alone")
        alone = g1.check(f"{what} item {b} alone")
        assert torch.equal(alone[0], got[b]), f"{what}: item {b} of the batch differs from the same item run alone"


def phase_matrix(W, s):
    """EngineCore::pack_convtr's phase-GEMM matrix of a transposed conv W (Cin, Cout, 2 s): row s * co + r, column 2 * ci + j
    take W[ci][co][r + s * j]; its bias is b.repeat_interleave(s)."""
    Cin, Cout = W.shape[:2]
    W2 = torch.zeros(s * Cout, 2 * Cin, dtype=torch.float64)
    for r in range(s):
        for j in range(2):
            W2[r::s, j::2] = W[:, :, r + s * j].t()
    return W2


# ---- A. un-cropped transposed convs ----------------------------------------------------------------------------------------------
def convtr_time(lib, mode, rt, s, B, Cin, Cout, T, what):
    """ConvTranspose1d(Cin, Cout, 2 s, s) with NO crop: all s * (T + 1) samples (hdemucs.py HDecLayer: the GroupNorm that follows
    decoder.0 / tdecoder.0's transposed conv reads them all before the crop)."""
    x, W, b = rnd(B, Cin, T, seed=101), rnd(Cin, Cout, 2 * s, seed=102, scale=(2 * Cin) ** -0.5), rnd(Cout, seed=103)
    want = F.conv_transpose1d(x, W, b, stride=s)
    Lu = s * T + s
    assert want.shape == (B, Cout, Lu)
    wt, bias, M, Mpad, K, Kpad, tile = pack_w(phase_matrix(W, s), b.repeat_interleave(s))
    kt = ktab(Cin, 1, 2, 1, -1, 0, 0, T, T, Kpad)

    def desc(n, xd, rd, y):
        return dict(wt=wt, M=M, Mpad=Mpad, K=K, Kpad=Kpad, ktab=kt, bias=bias, tile_m=tile, x=xd, x_bstride=Cin * T, B=n, D1=1, D2=T, O1=1,
                    O2=T + 1, S1=1, S2=1, row_mode=0, o2_valid=0, epi=EPI_CONVTR, flags=0, tr_stride=s, tr_pad=0, out_len=Lu, y=y,
                    y_cstride=Lu, y_bstride=Cout * Lu)
    check_layer(lib, mode, rt, what, x, None, want, (Cout, Lu), desc)


@pytest.mark.parametrize("B,Cin,Cout,T5,rt", [
    (3, 24, 64, 37, routes(128)),     # M 128; 114 columns: one partly filled column tile, item edges inside a wave's 32 columns
    (2, 24, 20, 75, routes(64)),      # M 40 on a 64-row tile, 24 padding rows: the co < cout mask with cout = M >> 1; two column tiles
    (2, 16, 48, 5, routes(96)),       # M 96; every column an edge
    (1, 8, 8, 1, routes(32, split=(TABLE, 32))),      # M 16; one input sample feeds both taps
], ids=["M128", "M40", "M96", "M16"])
def test_decoder0_uncropped_stride2(lib, x6, B, Cin, Cout, T5, rt):
    """A1: decoder.0, ConvTranspose1d(k 4, s 2) on the frame axis, flags 0: tr_stride 2, tr_pad 0, out_len 2 T5 + 2."""
    convtr_time(lib, x6, rt, 2, B, Cin, Cout, T5, f"decoder.0 ({B}, {Cin}, {Cout}, {T5})")


@pytest.mark.parametrize("B,Cin,Cout,T,rt", [(3, 24, 32, 37, routes(128)), (2, 24, 10, 75, routes(64))], ids=["M128", "M40"])
def test_tdecoder0_uncropped_stride4(lib, x6, B, Cin, Cout, T, rt):
    """A2: tdecoder.0, ConvTranspose1d(k 8, s 4), flags 0: tr_stride 4, tr_pad 0, out_len 4 T + 4."""
    convtr_time(lib, x6, rt, 4, B, Cin, Cout, T, f"tdecoder.0 ({B}, {Cin}, {Cout}, {T})")


@pytest.mark.parametrize("B,Cin,Cout,T,rt", [(3, 24, 32, 37, routes(128)), (2, 24, 10, 76, routes(64))], ids=["M128", "M40"])
def test_decoder1_one_row_to_eight(lib, x6, B, Cin, Cout, T, rt):
    """A3: decoder.1, ConvTranspose2d(k (8, 1), s (4, 1)) from ONE frequency row to eight, un-cropped, on rows of exactly T
    frames (T is neither padded nor a multiple of 4 in the engine)."""
    x, W, b = rnd(B, Cin, 1, T, seed=111), rnd(Cin, Cout, 8, 1, seed=112, scale=(2 * Cin) ** -0.5), rnd(Cout, seed=113)
    want = F.conv_transpose2d(x, W, b, stride=(4, 1))
    assert want.shape == (B, Cout, 8, T)
    wt, bias, M, Mpad, K, Kpad, tile = pack_w(phase_matrix(W[..., 0], 4), b.repeat_interleave(4))
    kt = ktab(Cin, 2, 1, -1, 1, 0, 0, T, T, Kpad)

    def desc(n, xd, rd, y):
        return dict(wt=wt, M=M, Mpad=Mpad, K=K, Kpad=Kpad, ktab=kt, bias=bias, tile_m=tile, x=xd, x_bstride=Cin * T, B=n, D1=1, D2=T, O1=2,
                    O2=T, S1=1, S2=1, row_mode=1, epi=EPI_CONVTR, flags=FLAG_TR_FREQ, tr_stride=4, tr_pad=0, out_len=8, y=y,
                    y_cstride=8 * T, y_bstride=Cout * 8 * T)
    check_layer(lib, x6, rt, f"decoder.1 ({B}, {Cin}, {Cout}, {T})", x, None, want, (Cout, 8, T), desc)


def test_cropped_transposed_conv_spelled_both_ways(lib, x6):
    """A4: the cropped ConvTranspose1d(k 8, s 4) + GELU + skip of test_conv_transpose_4phase's time-axis case, stated as
    tr_stride 4 / tr_pad 2 and as tr_stride 0 (the default that means the same): bit-identical, and right against float64."""
    B, Cin, Co, L, Lout = 2, 24, 12, 345, 1377
    x, W, b = rnd(B, Cin, L, seed=21), rnd(Cin, Co, 8, seed=22, scale=0.2), rnd(Co, seed=23)
    skip = rnd(B, Co, Lout, seed=24)
    want = F.gelu(F.conv_transpose1d(x, W, b, stride=4)[..., 2:2 + Lout]) + skip
    wt, bias, M, Mpad, K, Kpad, tile = pack_w(phase_matrix(W, 4), b.repeat_interleave(4))
    kt = ktab(Cin, 1, 2, 1, -1, 0, 0, L, L, Kpad)
    xd, rd = x.float().cuda(), skip.float().cuda()
    got = []
    for stride, pad in ((4, 2), (0, 0)):
        g = Guarded((B, Co, Lout))
        kw = dict(wt=wt, M=M, Mpad=Mpad, K=K, Kpad=Kpad, ktab=kt, bias=bias, tile_m=tile, x=xd, x_bstride=Cin * L, B=B, D1=1, D2=L, O1=1,
                  O2=L + 1, S1=1, S2=1, epi=EPI_CONVTR, flags=FLAG_GELU | FLAG_RES, res=rd, tr_stride=stride, tr_pad=pad, out_len=Lout,
                  y=g.y, y_cstride=Lout, y_bstride=Co * Lout)
        launch(lib, x6, expected(routes(64), x6), kw, f"cropped transposed conv tr_stride {stride}")
        got.append(g.check(f"cropped transposed conv tr_stride {stride}"))
    err = maxerr(got[0], want)
    print(f"cropped transposed conv [{x6}]: max error vs float64 {err:.3e}")
    assert err < TOL
    assert torch.equal(got[0], got[1])


# ---- B. strided convs of layers 4 and 5 --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,Cin,Cout,T,rt", [
    (3, 12, 128, 75, routes(128)),    # odd T: the last tap falls into the implicit right pad
    (2, 12, 40, 74, routes(64)),      # odd O2 = 37
    (1, 12, 96, 2, routes(96)),
], ids=["T75", "T74", "T2"])
def test_encoder5_conv_k4_s2(lib, x6, B, Cin, Cout, T, rt):
    """B1: encoder.5's Conv1d(k 4, s 2, p 1) on the frame axis, flags 0; HEncLayer pads the input on the right to a multiple of
    the stride first -- in the engine that padding exists only as the gather's D2 bound."""
    x, W, b = rnd(B, Cin, T, seed=121), rnd(Cout, Cin, 4, seed=122, scale=(4 * Cin) ** -0.5), rnd(Cout, seed=123)
    want = F.conv1d(F.pad(x, (0, T % 2)), W, b, stride=2, padding=1)
    T5 = (T + 1) // 2
    assert want.shape == (B, Cout, T5)
    wt, bias, M, Mpad, K, Kpad, tile = pack_w(W.reshape(Cout, -1), b)
    kt = ktab(Cin, 1, 4, 1, 1, 0, 1, T, T, Kpad)

    def desc(n, xd, rd, y):
        return dict(wt=wt, M=M, Mpad=Mpad, K=K, Kpad=Kpad, ktab=kt, bias=bias, tile_m=tile, x=xd, x_bstride=Cin * T, B=n, D1=1, D2=T, O1=1,
                    O2=T5, o2_valid=0, S1=1, S2=2, row_mode=0, epi=EPI_LINEAR, flags=0, y=y, y_bstride=Cout * T5, y_cstride=T5)
    check_layer(lib, x6, rt, f"encoder.5 conv ({B}, {Cin}, {Cout}, {T})", x, None, want, (Cout, T5), desc)


@pytest.mark.parametrize("B,Cin,Cc,D1,T,Tp,rt", [
    (3, 6, 128, 8, 37, 40, routes(128)),
    (2, 6, 40, 8, 75, 76, routes(64)),
    (2, 6, 96, 8, 36, 36, routes(96)),
    # not a layer of the model: the same conv on 12 rows, so that an output row o1 > 0 exists and the loaders' row term
    # o1 * S1 * x_ld of the column base is not zero (with O1 = 1 a loader that stepped rows by D2 would go unnoticed here)
    (2, 6, 40, 12, 37, 40, routes(64)),
], ids=["C128-T37", "C40-T75", "C96-T36", "two-output-rows"])
def test_encoder4_merge_conv_with_injection(lib, x6, B, Cin, Cc, D1, T, Tp, rt):
    """B2: encoder.4's Conv2d(k (8, 1), s (4, 1), no padding) that merges the last 8 frequency rows into one, + the injected
    tencoder.4 output (MI_FLAG_RES).  The input rows have pitch Tp (x_ld) with NaN in the pitch columns; the output enumerates
    exactly T columns (o2_valid 0)."""
    O1 = (D1 - 8) // 4 + 1
    x = torch.full((B, Cin, D1, Tp), float("nan"), dtype=torch.float64)
    x[..., :T] = rnd(B, Cin, D1, T, seed=131)
    W, b, res = rnd(Cc, Cin, 8, 1, seed=132, scale=(8 * Cin) ** -0.5), rnd(Cc, seed=133), rnd(B, Cc, O1, T, seed=134)
    want = F.conv2d(x[..., :T], W, b, stride=(4, 1)) + res
    assert want.shape == (B, Cc, O1, T)
    wt, bias, M, Mpad, K, Kpad, tile = pack_w(W.reshape(Cc, -1), b)
    kt = ktab(Cin, 8, 1, 1, 1, 0, 0, D1 * Tp, Tp, Kpad)

    def desc(n, xd, rd, y):
        return dict(wt=wt, M=M, Mpad=Mpad, K=K, Kpad=Kpad, ktab=kt, bias=bias, tile_m=tile, x=xd, x_bstride=Cin * D1 * Tp, B=n, D1=D1, D2=T,
                    x_ld=Tp if Tp != T else 0, O1=O1, O2=T, o2_valid=0, S1=4, S2=1, row_mode=1, epi=EPI_LINEAR, flags=FLAG_RES, res=rd,
                    y=y, y_bstride=Cc * O1 * T, y_cstride=O1 * T)
    check_layer(lib, x6, rt, f"encoder.4 merge conv ({B}, {Cin}, {Cc}, {D1}, {T}, {Tp})", x, res, want, (Cc, O1, T), desc)


@pytest.mark.parametrize("B,Cin,Cc,Lt,Lp,rt", [(3, 6, 128, 147, 148, routes(128)), (2, 6, 40, 298, 300, routes(64))], ids=["C128", "C40"])
def test_tencoder4_conv_no_gelu_pitched_input(lib, x6, B, Cin, Cc, Lt, Lp, rt):
    """B3: tencoder.4 (`empty`: the conv alone, no GELU), Conv1d(k 8, s 4, p 2) on rows of Lt samples at pitch Lp (NaN in the
    pitch), output of exactly ceil(Lt / 4) frames."""
    x = torch.full((B, Cin, Lp), float("nan"), dtype=torch.float64)
    x[..., :Lt] = rnd(B, Cin, Lt, seed=141)
    W, b = rnd(Cc, Cin, 8, seed=142, scale=(8 * Cin) ** -0.5), rnd(Cc, seed=143)
    want = F.conv1d(F.pad(x[..., :Lt], (0, -Lt % 4)), W, b, stride=4, padding=2)
    T = (Lt + 3) // 4
    assert want.shape == (B, Cc, T)
    wt, bias, M, Mpad, K, Kpad, tile = pack_w(W.reshape(Cc, -1), b)
    kt = ktab(Cin, 1, 8, 1, 1, 0, 2, Lp, Lp, Kpad)

    def desc(n, xd, rd, y):
        return dict(wt=wt, M=M, Mpad=Mpad, K=K, Kpad=Kpad, ktab=kt, bias=bias, tile_m=tile, x=xd, x_bstride=Cin * Lp, B=n, D1=1, D2=Lt,
                    x_ld=Lp, O1=1, O2=T, o2_valid=0, S1=1, S2=4, row_mode=0, epi=EPI_LINEAR, flags=0, y=y, y_bstride=Cc * T, y_cstride=T)
    check_layer(lib, x6, rt, f"tencoder.4 ({B}, {Cin}, {Cc}, {Lt}, {Lp})", x, None, want, (Cc, T), desc)


# ---- C. the deep DConv's plain linears -----------------------------------------------------------------------------------------------
def plain_linear(lib, mode, rt, what, N, M, K, W, seed, pitch=None, residual=False):
    """y[n] = W x[n] + b (+ res) on N items of W columns (Conv1d k 1 / nn.Linear on channel-first tokens), plain = 1, rows of the
    output at pitch `pitch`."""
    pitch = pitch or W
    x, Wm, b = rnd(N, K, W, seed=seed), rnd(M, K, seed=seed + 1, scale=K ** -0.5), rnd(M, seed=seed + 2)
    res = rnd(N, M, W, seed=seed + 3) if residual else None
    want = torch.einsum("mk,nkw->nmw", Wm, x) + b[None, :, None]
    if residual:
        want = want + res
    wt, bias, M_, Mpad, K_, Kpad, tile = pack_w(Wm, b)
    kt = ktab(K, 1, 1, 1, 1, 0, 0, W, W, Kpad)

    def desc(n, xd, rd, y):
        return dict(wt=wt, M=M, Mpad=Mpad, K=K, Kpad=Kpad, ktab=kt, bias=bias, tile_m=tile, x=xd, x_bstride=K * W, B=n, D1=1, D2=W, O1=1,
                    O2=W, S1=1, S2=1, row_mode=0, plain=1, epi=EPI_LINEAR, flags=FLAG_RES if residual else 0, res=rd, y=y,
                    y_bstride=M * pitch, y_cstride=pitch)
    check_layer(lib, mode, rt, what, x, res, want, (M, pitch), desc, valid=W)


@pytest.mark.parametrize("B,H,Tn,rt", [
    (3, 32, 37, routes(128)),                                         # M 112 on a 128-row tile; P % 4 != 0: the table loader
    (2, 32, 76, routes(64, half=(HALF, 128))),                        # float4 loader; under-filled: the 64-row small-batch tile
    (2, 32, 12800, routes(128, native=(DMA, 128))),                   # 200 workgroups: the native LDS-DMA tile, 16 padding rows
], ids=["Tn37", "Tn76", "Tn12800"])
def test_local_state_projection_rows_on_a_pitch(lib, x6, B, H, Tn, rt):
    """C1: LocalState's query / key / content (+ decay) projection, M = 3 H + 16 rows of Tn columns written at the row pitch
    round_up(Tn, 4): rows past M belong to nobody, pitch columns stay untouched."""
    plain_linear(lib, x6, rt, f"LocalState projection ({B}, {H}, {Tn})", B, 3 * H + 16, H, Tn, 151, pitch=rup(Tn, 4))


@pytest.mark.parametrize("N,H,W,rt", [
    (4, 32, 37, routes(128)),
    (3, 32, 200, routes(64, half=(HALF, 256))),                       # plain, Mpad 256: the half modes' 256-row tile
], ids=["W37", "W200"])
def test_blstm_input_projection(lib, x6, N, H, W, rt):
    """C2: the BLSTM's input projection, M = 8 H gate rows, on N = B * F items (frames) of W <= 200 columns."""
    plain_linear(lib, x6, rt, f"BLSTM input projection ({N}, {H}, {W})", N, 8 * H, H, W, 161)


def test_blstm_output_linear_with_residual(lib, x6):
    """C2: the BLSTM's output linear 2 H -> H with the skip added (the unframed form, MI_FLAG_RES)."""
    plain_linear(lib, x6, routes(32, split=(TABLE, 32)), "BLSTM output linear (2, 32, 37)", 2, 32, 64, 37, 171, residual=True)
