"""The kernel route of a conv / linear layer is a value: `mi_debug_conv_route` answers (route, tile) for a descriptor BEFORE any
launch, and the launch then takes that route on that tile (`mi_debug_last_conv_route`, `mi_debug_last_conv_tile`).

One descriptor per branch of the decision (demucs_amd/csrc/conv_route.hip conv_route), each with and without a split weight image:
  * plain linear layers on the two sides of the 200-workgroup line (4 x 49 and 4 x 50 workgroups of 128 rows): the 64-row
    small-batch tile below it, the 128-row tile (LDS-DMA when native) from it on;
  * 3 x 3 GLU convs with and without the tap geometry, and with Mpad a multiple of 96 or not: the native route's small-batch tile
    is the 96-row one, the split route's the 64-row tile that reads the 128-row image;
  * strided encoder convs with and without the row-tap promise (`dma_rows`), on 128- and 96-row tiles;
  * half-mode layers: the register-staged kernel on its 128- and 256-row tiles, and the two operand-image families.
`mi_set_split_bf16(0)` turns every "with" answer into the "without" one.  No numerics here: tests/test_gpu_x6_*.py and
tests/test_gpu_kernels.py compare these routes against float64 and bit for bit at sibling shapes."""
import ctypes as C

import pytest
import torch

from demucs_amd import _lib
from gpu_helpers import EPI_GLU, EPI_LINEAR, FLAG_GELU, FLAG_RES, FLAG_SCALE, conv_desc, ktab, pack_w

pytestmark = pytest.mark.gpu

TABLE, DMA, DMATAP, DMAROW, X6, HALF, TAP_HALF, TAP_X6, ROWS_X6, HALF_IMG, HALF_IMG256 = range(11)      # enum mi_conv_route (include/demucs_amd.h)
FLAG_LN, FLAG_HEADS = 32, 128


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return _lib.load()


def _w(M, K, glu=False):
    g = torch.Generator().manual_seed(M * 1000 + K)
    return pack_w(torch.randn(M, K, generator=g) * K ** -0.5, torch.zeros(M), glu=glu)


def _linear(x6, O2, M=512):
    """plain LINEAR, M = 512, K = 64, B = 2 on O2 tokens"""
    B, K = 2, 64
    wt, bias, M, Mpad, K, Kpad, tile = _w(M, K)
    return dict(x6=x6, wt=wt, M=M, Mpad=Mpad, K=K, Kpad=Kpad, ktab=ktab(K, 1, 1, 1, 1, 0, 0, O2, O2, Kpad),
                x=torch.randn(B, K, O2, device="cuda"), x_bstride=K * O2, B=B, D1=1, D2=O2, O1=1, O2=O2, S1=1, S2=1, plain=1,
                epi=EPI_LINEAR, flags=0, bias=bias, y=torch.empty(B, M, O2, device="cuda"), y_bstride=M * O2, y_cstride=O2, tile_m=tile)


def _image_linear(M, flags):
    """bf16 plain LINEAR on 2 x 64 tokens whose input is a 16-bit operand image [K / 8][N][8], weights packed for 128-row tiles:
    SCALE|RES (out_proj / lin2) or LN|HEADS (the attention in-projections, per-head 16-bit output)"""
    B, K, T = 2, 64, 64
    g = torch.Generator().manual_seed(M)
    wt, bias, M, Mpad, K, Kpad, tile = pack_w(torch.randn(M, K, generator=g) * K ** -0.5, torch.zeros(M), tile=128)
    kw = dict(x6="bf16", wt=wt, M=M, Mpad=Mpad, K=K, Kpad=Kpad, xh=torch.zeros(K // 8, B * T, 8, dtype=torch.bfloat16, device="cuda"), xh_n=B * T,
              B=B, D1=1, D2=T, O1=1, O2=T, S1=1, S2=1, plain=1, epi=EPI_LINEAR, flags=flags, bias=bias, scale=torch.ones(Mpad, device="cuda"),
              y=torch.empty(B, M, T, device="cuda"), y_bstride=M * T, y_cstride=T, tile_m=tile)
    if flags & FLAG_RES:
        kw.update(res=torch.zeros(B, M, T, device="cuda"))
    if flags & FLAG_LN:
        kw.update(pro_stats=torch.tensor([0.0, 1.0], device="cuda").repeat(B * T).contiguous())
    if flags & FLAG_HEADS:
        kw.update(yh=torch.empty(M // 512, B, 8, T, 64, dtype=torch.bfloat16, device="cuda"), yh_n=T)
    return kw


def _glu3x3(x6, Cc, B, geometry=True):
    """3 x 3 conv Cc -> 2 Cc + GLU on (Fr, T) = (8, 48), pitch = T; `geometry`: the descriptor states its taps"""
    Fr, T = 8, 48
    wt, bias, M, Mpad, K, Kpad, tile = _w(2 * Cc, 9 * Cc, glu=True)
    P = Fr * T
    kw = dict(x6=x6, wt=wt, M=M, Mpad=Mpad, K=K, Kpad=Kpad, ktab=ktab(Cc, 3, 3, 1, 1, 1, 1, P, T, Kpad),
              x=torch.randn(B, Cc, Fr, T, device="cuda"), x_bstride=Cc * P, B=B, D1=Fr, D2=T, O1=Fr, O2=T, S1=1, S2=1, row_mode=1,
              epi=EPI_GLU, bias=bias, y=torch.empty(B, Cc, Fr, T, device="cuda"), y_bstride=Cc * P, y_cstride=P, tile_m=tile)
    if geometry:
        kw.update(ntaps=9, tap_k2=3, tap_pad1=1, tap_pad2=1)
    return kw


def _encoder(x6, Cin, Cout, B, Fr, T, pitch, dma_rows):
    """Conv2d k = (8, 1), s = (4, 1), p = (2, 0) + GELU on rows of `pitch` >= T floats"""
    wt, bias, M, Mpad, K, Kpad, tile = _w(Cout, 8 * Cin)
    P = Fr // 4 * pitch
    return dict(x6=x6, wt=wt, M=M, Mpad=Mpad, K=K, Kpad=Kpad, ktab=ktab(Cin, 8, 1, 1, 1, 2, 0, Fr * pitch, pitch, Kpad),
                x=torch.randn(B, Cin, Fr, pitch, device="cuda"), x_bstride=Cin * Fr * pitch, B=B, D1=Fr, D2=T, O1=Fr // 4, O2=pitch,
                S1=4, S2=1, row_mode=1, epi=EPI_LINEAR, flags=FLAG_GELU, bias=bias, y=torch.empty(B, M, Fr // 4, pitch, device="cuda"),
                y_bstride=M * P, y_cstride=P, tile_m=tile, o2_valid=T, x_ld=pitch, dma_rows=dma_rows)


#        id   layer                                                             (route, tile) with split   without
CASES = [("A", lambda x6: _linear(x6, 3136),                                    (X6, 64),       (TABLE, 64)),     # 4 x 49 workgroups
         ("B", lambda x6: _linear(x6, 3200),                                    (X6, 128),      (DMA, 128)),      # 4 x 50
         ("C", lambda x6: _glu3x3(x6, 48, 2),                                   (TAP_X6, 96),   (DMATAP, 96)),
         ("D", lambda x6: _glu3x3(x6, 48, 2, geometry=False),                   (X6, 96),       (TABLE, 96)),
         ("E", lambda x6: _glu3x3(x6, 64, 1),                                   (TAP_X6, 64),   (DMATAP, 128)),   # Mpad 128: no 96-row tile
         ("F", lambda x6: _glu3x3(x6, 192, 1),                                  (TAP_X6, 64),   (DMATAP, 96)),    # Mpad 384 = 4 x 96
         ("G", lambda x6: _encoder(x6, 24, 128, 3, 16, 37, 40, dma_rows=1),     (ROWS_X6, 64),  (DMAROW, 128)),
         ("H", lambda x6: _encoder(x6, 20, 96, 2, 8, 61, 64, dma_rows=1),       (ROWS_X6, 96),  (DMAROW, 96)),
         ("I", lambda x6: _encoder(x6, 24, 128, 3, 16, 37, 40, dma_rows=0),     (X6, 128),      (TABLE, 128)),
         # bf16, Mpad % 256 == 0: the register-staged kernel's 256-row <2, 2, 4, 2> tile (MI_HALF_TILE256 defaults to 1)
         ("J", lambda x6: _linear("bf16", 3136),                                None,           (HALF, 256)),
         ("K", lambda x6: _linear("bf16", 3136, M=128),                         None,           (HALF, 128)),
         ("L", lambda x6: _image_linear(384, FLAG_SCALE | FLAG_RES),            None,           (HALF_IMG, 128)),  # Mpad 384: no 256-row tile
         ("M", lambda x6: _image_linear(512, FLAG_LN | FLAG_HEADS),             None,           (HALF_IMG256, 256))]


def _route(lib, d):
    tile = C.c_int(-1)
    return lib.mi_debug_conv_route(C.byref(d), C.byref(tile)), tile.value


def _forward(lib, d):
    _lib.check(lib.mi_conv_forward(C.byref(d), C.c_void_p(_lib.current_stream_ptr())), "mi_conv_forward")
    torch.cuda.synchronize()
    return lib.mi_debug_last_conv_route(), lib.mi_debug_last_conv_tile()


@pytest.mark.parametrize("name,layer,with_split,without", CASES, ids=[c[0] for c in CASES])
def test_route_is_decided_before_the_launch(lib, name, layer, with_split, without):
    for x6, want in ((True, with_split), (False, without)):
        if want is None:
            continue
        d, keep = conv_desc(**layer(x6))
        assert bool(d.wx) == (x6 and with_split is not None)
        got = _route(lib, d)
        print(f"row {name} split image {x6}: (route, tile) {got}, expected {want}")
        assert got == want
        assert _forward(lib, d) == want
        if x6 and with_split is not None:
            old = lib.mi_set_split_bf16(0)
            try:
                assert _route(lib, d) == without
                assert _forward(lib, d) == without
                lib.mi_set_split_bf16(1)
                assert _route(lib, d) == with_split
            finally:
                lib.mi_set_split_bf16(old)


def test_null_descriptor_has_no_route(lib):
    assert lib.mi_debug_conv_route(None, None) == -1
