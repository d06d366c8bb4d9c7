"""The half modes' tap-image convs (gemm_tap.hip, route 6) and the three epilogues that write the next layer's 16-bit operand image
instead of a float32 tensor (gemm_tile.h: GLU|IMG, CONVTR with GELU|RES|IMG, LINEAR with RES|IMG), each alone through
`mi_conv_forward`, in both modes, against float64.  In the engines the tensors between these layers exist only as images, so a
wrong octet, a missed frame edge or a stray float32 store shows at the end of a forward only.

What the cases reach that the tests of test_gpu_kernels.py do not: the 128-row configuration (2 x 2 waves, the second A-row
transfer), more than one M tile, a last M tile that is partly empty (M = 160 in two 128-row tiles), two 96-row tiles, a single K
step (fewer than the ring has stages) and a partial last one, the scattered 2-byte stores of the transposed conv's image, the plain
GLU image, dilated k = 3 LINEAR convs, the outermost transposed conv on a 64-row tile, a 3 x 3 conv on pitched rows, the
neighbouring items of the image (a NaN item next to the one under test), and the three layers of an HDemucs decoder level chained
through the images they write.

Operands: `rnd16` draws values exactly representable in bf16 AND fp16 (as `rnd` of test_gpu_kernels.py does under a half mode), so
the operand rounding is the identity, products are exact in float32 and the reference is float64 on the same operands.  The test
builds the input image [C / 8][positions][8] on the host (gpu_helpers.image_of; pitch columns and the columns past the tensor hold
NaN, the encoder convs read a host-built phase-split image, gpu_helpers.phase_image) and the library's `mi_conv_pack_tap` orders
the weights by (channel octet, tap, channel % 8): that packer is part of what is under test.

Bounds.  None is taken from the kernels.  RESTATED[(family, type, K)] is the largest distance of the SAME formula evaluated in
torch float32 on the CPU from float64, over every case of the family in this file (tests/test_tap_image_bounds.py recomputes the
table); a float32 output may be 4x that from float64 (the kernels sum in another order).  A 16-bit output must equal, bit for bit,
the host rounding of the float32 y of the same descriptor launched without the IMG bit, laid out by `image_of`; every slot the
layer does not own -- pitch columns, positions past `out_len`, rows >= M, the slack of an image with yh_n larger than needed --
must still hold the sentinel the image was filled with, and the float32 y passed to an IMG launch must come back untouched (in
the engines y and yh are one buffer).  Every case prints restated, kernel, bound and their ratio.

After every launch `mi_debug_last_conv_route` / `mi_debug_last_conv_tile` must name route 6 (5 for the register-staged cases) and
the tile the case states, which is also what `mi_debug_conv_route` (conv_route.hip) answers for the descriptor.  Every launch
passes a caller-owned sink -- guard, 256 dump floats, 64 zeros, guard -- and the zeros and the guards must survive."""
import ctypes as C
import functools
import zlib
from types import SimpleNamespace

import pytest
import torch
import torch.nn.functional as F

from demucs_amd import _lib
from gpu_helpers import (EPI_CONVTR, EPI_GLU, EPI_LINEAR, FLAG_GELU, FLAG_RES, FLAG_TR_FREQ, conv_desc, image_of, image_to, ktab,
                         pack_w, phase_image, pick_tile, rup)

pytestmark = pytest.mark.gpu
IMG = 64
GR = FLAG_GELU | FLAG_RES
HDT = {"bf16": torch.bfloat16, "f16": torch.float16}
DT = {"bf16": 1, "f16": 2}
MODES = ["bf16", "f16"]
SINK, ZERO, GUARD, GUARD_VALUE = 256, 64, 64, -12345.0          # csrc/gemm_conv.h MI_SINK_FLOATS, MI_ZERO_PAGE_FLOATS
SENT16 = 0x7FC1                                                  # 16-bit outputs start as this pattern: a NaN in both types
HALF, TAP_HALF = 5, 6                                            # enum mi_conv_route (include/demucs_amd.h)
NAN = float("nan")
FAMILY_FLAGS = {"glu": 0, "convtr": 0, "convtr_gelu_res": GR, "lin_res": FLAG_RES, "enc_gelu": FLAG_GELU, "lin_k3": 0}

# largest max-abs distance of the float32 restatement from float64 over the family's cases, {(family, type, K): distance}
RESTATED = {
    ('convtr', 'bf16', 64): 9.24e-07, ('convtr', 'bf16', 96): 1.34e-06, ('convtr', 'f16', 64): 1.09e-06,
    ('convtr', 'f16', 96): 1.52e-06, ('convtr_gelu_res', 'bf16', 64): 1.24e-06, ('convtr_gelu_res', 'bf16', 96): 1.57e-06,
    ('convtr_gelu_res', 'f16', 64): 2.15e-06, ('convtr_gelu_res', 'f16', 96): 1.89e-06, ('enc_gelu', 'bf16', 256): 2.99e-06,
    ('enc_gelu', 'f16', 256): 2.55e-06, ('glu', 'bf16', 24): 2.92e-07, ('glu', 'bf16', 48): 6.15e-07,
    ('glu', 'bf16', 144): 1.08e-06, ('glu', 'bf16', 192): 1.73e-06, ('glu', 'bf16', 288): 8.47e-07, ('glu', 'bf16', 576): 1.25e-06,
    ('glu', 'bf16', 720): 1.68e-06, ('glu', 'bf16', 864): 2.60e-06, ('glu', 'f16', 24): 6.56e-07, ('glu', 'f16', 48): 6.42e-07,
    ('glu', 'f16', 144): 1.90e-06, ('glu', 'f16', 192): 1.50e-06, ('glu', 'f16', 288): 1.37e-06, ('glu', 'f16', 576): 2.14e-06,
    ('glu', 'f16', 720): 1.66e-06, ('glu', 'f16', 864): 2.09e-06, ('lin_k3', 'bf16', 96): 1.04e-06,
    ('lin_k3', 'f16', 96): 1.02e-06, ('lin_res', 'bf16', 64): 7.67e-07, ('lin_res', 'f16', 64): 5.96e-07,
}

# 3 x 3 / k = 3 GLU rewrites: (C, Fr, T, pitch, B, tile, float32 y, IMG, yh slack).  Fr = 1: k = 3 on time
GLU_CASES = [
    (64, 5, 37, 40, 2, 128, True, True, 5),       # M = 128, 72 pairs; N = 400: an item boundary inside a column tile, ragged last tile
    (80, 3, 40, 40, 2, 128, True, True, 0),       # M = 160, Mpad = 256: the second 128-row tile a quarter full; 90 pairs: partial last K step
    (96, 4, 33, 36, 1, 96, True, True, 0),        # M = 192: two 96-row tiles
    (64, 1, 301, 304, 2, 128, True, True, 0),     # k = 3 on time, 128-row tile
    (8, 1, 77, 80, 2, 32, True, False, 0),        # M = 16 on the 32-row tile; 3 pairs: ONE K step (the ring has three stages)
    (16, 1, 77, 80, 2, 32, True, True, 3),        # M = 32; 6 pairs: two K steps
]
# transposed convs, on both axes: (Cout, C, tile, flag sets)
CONVTR_CASES = [
    (32, 32, 128, (0, GR, GR | IMG)),             # M = 128, two K steps
    (40, 48, 128, (0, GR, GR | IMG)),             # M = 160, Mpad = 256: the second tile partly empty, the co < cout mask
    (24, 32, 96, (0, GR, GR | IMG)),
    (16, 32, 64, (0,)),                           # the HDemucs outermost form: TR_FREQ alone / no flags
]
TR_FREQ_GEO = (6, 21, 24)                         # Fr, T, pitch
TR_TIME_GEO = (345, 348, 1377, 1380)              # L, pitch, out_len, output pitch
LIN_RES_CASES = [(64, 96, 100), (64, 128, 100)]   # (K, M, P): plain 1 x 1 on the register-staged route
ENC_CASES = [(128, 128), (192, 96)]               # (Co, tile), on both axes; C = 32
K3_CASES = [1, 2]                                 # dilation; C = 32, M = 128, T = 203 on the pitch 204
CHAIN = (32, 16, 4, 21, 24)                       # C -> Cout, Fr, T, pitch


def rnd16(g, *shape, scale=1.0):
    """Values exactly representable in bf16 AND fp16 (8 significant bits, normal in fp16)."""
    t = (torch.randn(*shape, generator=g, dtype=torch.float64) * scale).float().bfloat16().double()
    return torch.where(t.abs() < 2.0 ** -14, torch.zeros_like(t), t)


def gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


# ---- the layers: operands, descriptor geometry and the formula (CPU) -----------------------------------------------------

def new_layer(mode, family, x, W2d, bias, glu=False, **kw):
    """x (B, C, D1, D2): the valid input; W2d (M, K) with k = ci * ntaps + tap; output (B, Cy, R, Wp), Wv valid columns per row."""
    L = SimpleNamespace(mode=mode, family=family, x=x, B=x.shape[0], C=x.shape[1], W2d=W2d, bias=bias, glu=glu, M=W2d.shape[0],
                        K=W2d.shape[1], tile=pick_tile(W2d.shape[0]), flags=0, res=None, plain=0, dev=None, wants={}, **kw)
    L.name = f"{family} {mode} C {L.C} M {L.M} K {L.K} B {L.B} out {L.R} x {L.Wv} (pitch {L.Wp})"
    return L


def glu_layer(mode, C, Fr, T, Tp, B=2, x=None):
    """The decoders' 3 x 3 (Fr > 1) / k = 3 (Fr = 1) rewrite conv C -> 2 C + GLU on rows of pitch Tp."""
    time = Fr == 1
    g = gen("glu", mode, C, Fr, T, B)
    x0 = rnd16(g, B, C, Fr, T)
    W = rnd16(g, 2 * C, C, 1 if time else 3, 3, scale=0.2 if time else 0.1)
    b = torch.randn(2 * C, generator=g).float()
    L = new_layer(mode, "glu", x0 if x is None else x, W.reshape(2 * C, -1), b, glu=True, epi=EPI_GLU, chan_div=2, Cy=C, R=Fr, Wp=Tp,
                  Wv=T, x_ld=Tp, ntaps=W.shape[2] * 3, cin=C,
                  geo=dict(D1=Fr, D2=T, O1=Fr, O2=Tp, row_mode=0 if time else 1, o2_valid=T if Tp != T else 0, x_ld=Tp if Tp != T else 0),
                  tapgeo=dict(ntaps=W.shape[2] * 3, tap_k2=3, tap_pad1=0 if time else 1, tap_pad2=1),
                  ktab_args=(C, W.shape[2], 3, 1, 1, 0 if time else 1, 1, Fr * Tp, Tp))

    def formula(flags, dt):
        z = F.conv2d(L.x.to(dt), W.to(dt), b.to(dt), padding=(0 if time else 1, 1))
        return z[:, :C] * torch.sigmoid(z[:, C:])
    L.formula = formula
    return L


def convtr_layer(mode, C, Cout, freq, geo=None, B=2, x=None):
    """ConvTranspose k = 8, s = 4 cropped by 2 [+ GELU + skip] as a 4-phase GEMM over the taps q and q - 1; frequency axis
    (TR_FREQ: an extra output row, rows of pitch Tp) or ragged time axis (L + 1 columns on the input pitch, out_len on the output's)."""
    g = gen("convtr", mode, C, Cout, freq, geo, B)
    W = rnd16(g, C, Cout, 8, scale=0.2)
    b = torch.randn(Cout, generator=g).float()
    W2 = W.reshape(C, Cout, 2, 4).permute(1, 3, 0, 2).reshape(4 * Cout, 2 * C)       # row 4 co + r, column 2 ci + j  <-  W[ci][co][r + 4 j]
    if freq:
        Fr, T, Tp = geo or TR_FREQ_GEO
        x0, res = rnd16(g, B, C, Fr, T), torch.randn(B, Cout, 4 * Fr, T, generator=g).float()
        kw = dict(R=4 * Fr, Wp=Tp, Wv=T, x_ld=Tp, ktab_args=(C, 2, 1, -1, 1, 0, 0, Fr * Tp, Tp),
                  geo=dict(D1=Fr, D2=T, O1=Fr + 1, O2=Tp, o2_valid=T if Tp != T else 0, x_ld=Tp if Tp != T else 0, row_mode=1, out_len=4 * Fr),
                  tapgeo=dict(ntaps=2, tap_k2=1, tap_dil1=-1))
    else:
        Ln, Lp, Lout, Lpo = geo or TR_TIME_GEO
        x0, res = rnd16(g, B, C, 1, Ln), torch.randn(B, Cout, 1, Lout, generator=g).float()
        kw = dict(R=1, Wp=Lpo, Wv=Lout, x_ld=Lp, ktab_args=(C, 1, 2, 1, -1, 0, 0, Lp, Lp),
                  geo=dict(D1=1, D2=Ln, O1=1, O2=Ln + 1, x_ld=Lp, out_len=Lout), tapgeo=dict(ntaps=2, tap_k2=2, tap_dil2=-1))
    L = new_layer(mode, "convtr", x0 if x is None else x, W2, b.repeat_interleave(4), epi=EPI_CONVTR, chan_div=4, Cy=Cout, ntaps=2, cin=C, **kw)
    L.flags, L.res = FLAG_TR_FREQ if freq else 0, res

    def formula(flags, dt):
        if freq:
            v = F.conv_transpose2d(L.x.to(dt), W.to(dt)[..., None], b.to(dt), stride=(4, 1))[..., 2:-2, :]
        else:
            v = F.conv_transpose1d(L.x.to(dt)[:, :, 0], W.to(dt), b.to(dt), stride=4)[..., None, 2:2 + L.Wv]
        return F.gelu(v) + res.to(dt) if flags & FLAG_GELU else v
    L.formula = formula
    return L


def lin_res_layer(mode, K, M, P, B=2):
    """The channel down-sampler in front of the decoders: plain 1 x 1, bias + residual, on the register-staged route."""
    g = gen("lin_res", mode, K, M, P, B)
    x, W = rnd16(g, B, K, 1, P), rnd16(g, M, K, scale=K ** -0.5)
    b, res = torch.randn(M, generator=g).float(), torch.randn(B, M, 1, P, generator=g).float()
    L = new_layer(mode, "lin_res", x, W, b, epi=EPI_LINEAR, chan_div=1, Cy=M, R=1, Wp=P, Wv=P, x_ld=P, ntaps=0, cin=K,
                  geo=dict(D1=1, D2=P, O1=1, O2=P), tapgeo={}, ktab_args=(K, 1, 1, 1, 1, 0, 0, P, P))
    L.res, L.plain = res, 1
    L.formula = lambda flags, dt: torch.einsum("mk,bkrp->bmrp", W.to(dt), L.x.to(dt)) + b.to(dt)[None, :, None, None] + res.to(dt)
    return L


def enc_layer(mode, Co, freq, C=32, B=2):
    """Encoder levels 1-3: the strided conv (k = 8, s = 4, pad 2) + GELU as a stride-1 two-tap conv over 4 C channels of the
    phase-split image of its input, built here on the host; frequency rows, or a ragged time axis (L = 1373 -> 344)."""
    g = gen("enc", mode, Co, freq, C, B)
    W, b = rnd16(g, Co, C, 8, scale=0.2), torch.randn(Co, generator=g).float()
    wt2d = torch.zeros(Co, 8 * C, dtype=torch.float64)       # k' = ((oct * 4 + rho) * 8 + c8) * 2 + j  <-  tap 4 (j - (rho >= 2)) + rho + 2
    for ci in range(C):
        for rho in range(4):
            for j in range(2):
                wt2d[:, (((ci // 8) * 4 + rho) * 8 + ci % 8) * 2 + j] = W[:, ci, 4 * (j - (1 if rho >= 2 else 0)) + rho + 2]
    if freq:
        Fr, T = 32, 40
        Q, Lo = Fr // 4 + 1, Fr // 4
        x, pq = rnd16(g, B, C, Fr, T), Q * T
        kw = dict(R=Lo, Wp=T, Wv=T, geo=dict(D1=Q, D2=T, O1=Lo, O2=T, row_mode=1), tapgeo=dict(ntaps=2, tap_k2=1))
    else:
        Ln = 1373
        Q, Lo = (Ln + 3) // 4 + 1, (Ln + 3) // 4
        x, pq, Lop = rnd16(g, B, C, Ln), rup(Q, 4), rup(Lo, 4)
        kw = dict(R=1, Wp=Lop, Wv=Lo, geo=dict(D1=1, D2=pq, x_ld=pq, O1=1, O2=Lop, o2_valid=Lo), tapgeo=dict(ntaps=2, tap_k2=2))
    L = new_layer(mode, "enc_gelu", x, wt2d, b, epi=EPI_LINEAR, chan_div=1, Cy=Co, x_ld=0, ntaps=2, cin=4 * C, ktab_args=None, **kw)
    L.flags = FLAG_GELU

    def ximage(fill, nan_item):
        img = phase_image(x, x.shape[2], pq, freq, T if freq else 0, HDT[mode]).view(HDT[mode])
        if not freq:              # output o reads the slots o and o + 1 <= Lo of every plane: the rest of the pitch is never read
            img.view(-1, B, pq, 8)[:, :, Lo + 1:] = NAN
        return img
    L.ximage = ximage

    def formula(flags, dt):
        if freq:
            return F.gelu(F.conv2d(x.to(dt), W.to(dt)[..., None], b.to(dt), stride=(4, 1), padding=(2, 0)))
        return F.gelu(F.conv1d(F.pad(x.to(dt), (0, (-x.shape[2]) % 4)), W.to(dt), b.to(dt), stride=4, padding=2))[:, :, None]
    L.formula = formula
    return L


def k3_layer(mode, dil, C=32, M=128, T=203, Tp=204, B=2):
    """HDemucs layers 4 / 5: LINEAR with no flags, k = 3 on time with dilation 1 / 2."""
    g = gen("k3", mode, dil, C, M, T, B)
    x, W, b = rnd16(g, B, C, 1, T), rnd16(g, M, C, 3, scale=0.2), torch.randn(M, generator=g).float()
    L = new_layer(mode, "lin_k3", x, W.reshape(M, -1), b, epi=EPI_LINEAR, chan_div=1, Cy=M, R=1, Wp=Tp, Wv=T, x_ld=Tp, ntaps=3, cin=C,
                  geo=dict(D1=1, D2=T, O1=1, O2=Tp, o2_valid=T, x_ld=Tp), tapgeo=dict(ntaps=3, tap_k2=3, tap_pad2=dil, tap_dil2=dil),
                  ktab_args=(C, 1, 3, 1, dil, 0, dil, Tp, Tp))
    L.formula = lambda flags, dt: F.conv1d(L.x.to(dt)[:, :, 0], W.to(dt), b.to(dt), padding=dil, dilation=dil)[:, :, None]
    return L


def chain_layers(mode, x2=None, x3=None):
    """The three layers of an HDemucs decoder level on the frequency axis: GLU|IMG rewrite, CONVTR|GELU|RES|IMG, 3 x 3 GLU.  x2, x3:
    the operands the second and third layer actually read (decoded from the device's images); without them, the host rounding of
    the float64 result of the layer before -- the same values up to a few roundings that fall the other way, which is what the
    CPU-only bound table is computed on."""
    Cc, Co, Fr, T, Tp = CHAIN
    hdt = HDT[mode]
    L1 = glu_layer(mode, Cc, Fr, T, Tp)
    if x2 is None:
        x2 = L1.formula(0, torch.float64).to(hdt).double()
    L2 = convtr_layer(mode, Cc, Co, True, geo=(Fr, T, Tp), x=x2)
    if x3 is None:
        x3 = L2.formula(GR, torch.float64).to(hdt).double()
    L3 = glu_layer(mode, Co, 4 * Fr, T, Tp, x=x3)
    return L1, L2, L3


_BUILDERS = {"glu": glu_layer, "convtr": convtr_layer, "lin_res": lin_res_layer, "enc": enc_layer, "k3": k3_layer}


@functools.lru_cache(maxsize=None)
def layer(kind, mode, *args):
    """One layer object per case and mode: its operands and float64 references are computed once and shared."""
    return _BUILDERS[kind](mode, *args)


@functools.lru_cache(maxsize=None)
def chain_standins(mode):
    return chain_layers(mode)


def want_of(L, fam):
    """(float64 result, distance of the float32 restatement from it) of the layer under the family's flags."""
    if fam not in L.wants:
        w = L.formula(FAMILY_FLAGS[fam], torch.float64)
        L.wants[fam] = (w, (L.formula(FAMILY_FLAGS[fam], torch.float32).double() - w).abs().max().item())
    return L.wants[fam]


def fam_of(L, flags):
    return "convtr_gelu_res" if L.family == "convtr" and flags & FLAG_GELU else L.family


def family_cases(mode):
    """Every (layer, family) this file checks a float32 output of: the cases RESTATED is a maximum over."""
    out = [(layer("glu", mode, *c[:5]), "glu") for c in GLU_CASES]
    for freq in (True, False):
        for Cout, Cin, _, sets in CONVTR_CASES:
            out += [(layer("convtr", mode, Cin, Cout, freq), fam_of(SimpleNamespace(family="convtr"), f)) for f in sets if not f & IMG]
        out += [(layer("enc", mode, Co, freq), "enc_gelu") for Co, _ in ENC_CASES]
    out += [(layer("lin_res", mode, *c), "lin_res") for c in LIN_RES_CASES]
    out += [(layer("k3", mode, dil), "lin_k3") for dil in K3_CASES]
    L1, L2, L3 = chain_standins(mode)
    return out + [(L1, "glu"), (L2, "convtr_gelu_res"), (L3, "glu")]


# ---- launches ------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return _lib.load()


def stream():
    return C.c_void_p(_lib.current_stream_ptr())


def device_side(lib, L):
    if L.dev is None:
        d = SimpleNamespace()
        d.wt, d.bias, _, d.Mpad, _, d.Kpad, d.tile = pack_w(L.W2d, L.bias, glu=L.glu)
        assert d.tile == L.tile
        if L.ntaps:
            pairs = (L.cin // 8 * L.ntaps + 3) // 4 * 4
            d.wtap = torch.empty(pairs * d.Mpad * 8, dtype=torch.int16, device="cuda")
            _lib.check(lib.mi_conv_pack_tap(d.wt.data_ptr(), d.Mpad, L.cin, L.ntaps, DT[L.mode], d.wtap.data_ptr(), stream()), "mi_conv_pack_tap")
        if L.res is not None:
            r = torch.full((L.B, L.Cy, L.R, L.Wp), NAN)
            r[..., :L.Wv] = L.res
            d.res = r.cuda()
        L.dev = d
    return L.dev


def padded_input(L, fill=NAN, nan_item=None):
    """(B, C, D1, row pitch) float64: the valid input, `fill` in the pitch columns, one item all NaN on request."""
    B, Cn, D1, D2 = L.x.shape
    xp = torch.full((B, Cn, D1, L.x_ld), fill, dtype=torch.float64)
    xp[..., :D2] = L.x
    if nan_item is not None:
        xp[nan_item] = NAN
    return xp


def input_image(L, fill=NAN, nan_item=None, xpad=3):
    """The layer's input as the 16-bit image it reads, with xpad NaN columns behind the tensor."""
    img = L.ximage(fill, nan_item) if hasattr(L, "ximage") else image_of(padded_input(L, fill, nan_item).to(HDT[L.mode]))
    return torch.cat([img, torch.full((img.shape[0], xpad, 8), NAN, dtype=HDT[L.mode])], 1).contiguous().cuda()


def new_sink():
    buf = torch.full((GUARD + SINK + ZERO + GUARD,), GUARD_VALUE, device="cuda")
    buf[GUARD:GUARD + SINK + ZERO] = 0.0
    return buf


def check_sink(buf, what):
    b = buf.cpu()
    assert bool((b[GUARD + SINK:GUARD + SINK + ZERO] == 0).all()), f"{what}: the zero page behind the sink was written"
    assert bool((b[:GUARD] == GUARD_VALUE).all()) and bool((b[-GUARD:] == GUARD_VALUE).all()), f"{what}: store outside the sink"


def run(lib, L, flags=0, tap=True, fill=NAN, nan_item=None, ypad=0, xh=None):
    """One launch.  y starts as NaN, yh as SENT16.  tap: the input image + tap-ordered weights (route 6); else the float32 input and
    the gather table (route 5).  xh: a device image to read instead of the host-built one."""
    d = device_side(lib, L)
    B, Cy, R, Wp = L.B, L.Cy, L.R, L.Wp
    out = SimpleNamespace(sink=new_sink(), y=torch.full((B, Cy, R, Wp), NAN, device="cuda"), yh=None)
    kw = dict(x6=L.mode, wt=d.wt, M=L.M, Mpad=d.Mpad, K=L.K, Kpad=d.Kpad, B=B, S1=1, S2=1, epi=L.epi, flags=L.flags | flags, bias=d.bias,
              y=out.y, y_bstride=Cy * R * Wp, y_cstride=R * Wp, tile_m=d.tile, sink=out.sink[GUARD:], plain=L.plain, **L.geo)
    if tap:
        img = input_image(L, fill, nan_item) if xh is None else xh
        kw.update(xh=img, xh_n=img.shape[1], wtap=d.wtap, **L.tapgeo)
    else:
        x = padded_input(L, fill, nan_item).float().cuda()
        kw.update(x=x, x_bstride=x[0].numel(), ktab=ktab(*L.ktab_args, d.Kpad))
    if flags & FLAG_RES:
        kw.update(res=d.res)
    if flags & IMG:
        out.yh = torch.full((d.Mpad // L.chan_div // 8, B * R * Wp + ypad, 8), SENT16, dtype=torch.int16, device="cuda")
        kw.update(yh=out.yh, yh_n=out.yh.shape[1])
    desc, keep = conv_desc(**kw)
    _lib.check(lib.mi_conv_forward(C.byref(desc), stream()), "mi_conv_forward")
    torch.cuda.synchronize()
    what = f"{L.name} flags {L.flags | flags}"
    tile = C.c_int(0)
    took, want = (lib.mi_debug_last_conv_route(), lib.mi_debug_last_conv_tile()), (TAP_HALF if tap else HALF, L.tile)
    assert took == want, f"{what}: (route, tile) {took}, expected {want}"
    assert (lib.mi_debug_conv_route(C.byref(desc), C.byref(tile)), tile.value) == want, f"{what}: conv_route disagrees with {want}"
    check_sink(out.sink, what)
    del keep
    return out


# ---- checks ----------------------------------------------------------------------------------------------------------------

def check_y(L, flags, out, what):
    fam = fam_of(L, flags)
    w64, restated = want_of(L, fam)
    y = out.y.cpu()
    assert bool(torch.isfinite(y[..., :L.Wv]).all()), f"{what}: non-finite y"
    assert bool(torch.isnan(y[..., L.Wv:]).all()), f"{what}: pitch / padding columns of y written"
    err, bound = (y[..., :L.Wv].double() - w64).abs().max().item(), 4 * RESTATED[(fam, L.mode, L.K)]
    print(f"{what} {L.name}: restated {restated:.2e}  kernel {err:.2e}  bound {bound:.2e}  ratio {err / bound:.2f}")
    assert err <= bound, f"{what} {L.name}: {err:.3e} > {bound:.3e}"


def check_image(L, out, ref, what):
    """out: an IMG launch; ref: the launch of the same descriptor without the IMG bit (its y was held to float64 by check_y)."""
    assert bool(torch.isnan(out.y).all()), f"{what} {L.name}: the IMG launch stored float32 values to y"
    yh = out.yh.cpu()
    n, oc = L.B * L.R * L.Wp, L.Cy // 8
    valid = torch.zeros(L.B, L.Cy, L.R, L.Wp, dtype=torch.bool)
    valid[..., :L.Wv] = True
    exp = torch.full_like(yh, SENT16)
    exp[:oc, :n] = torch.where(image_of(valid), image_of(ref.y.cpu().to(HDT[L.mode]).view(torch.int16)), exp[:oc, :n])
    if not torch.equal(yh, exp):
        bad = yh != exp
        own = torch.zeros_like(bad)
        own[:oc, :n] = image_of(valid)
        raise AssertionError(f"{what} {L.name}: image != rounding of y: {int((bad & own).sum())} of its own slots differ, "
                             f"{int((bad & ~own).sum())} slots it does not own were written; first {bad.nonzero()[0].tolist()}")
    print(f"{what} {L.name}: image == rounding of y, {int((exp == SENT16).sum())} sentinel slots intact")


def item_of(L, out, b):
    """Item b of a launch's output: its float32 rows, or its columns of the image."""
    if out.yh is None:
        return out.y[b].cpu().view(torch.int32)
    P = L.R * L.Wp
    return out.yh[:, b * P:(b + 1) * P].cpu()


# ---- 1. GLU rewrites -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", GLU_CASES, ids=["C%d-Fr%d-T%d-p%d-B%d" % c[:5] for c in GLU_CASES])
def test_glu_rewrite_on_the_tap_route(lib, mode, case):
    *shape, tile, f32, img, ypad = case
    L = layer("glu", mode, *shape)
    assert L.tile == tile
    a = run(lib, L)
    check_y(L, 0, a, "glu")
    if img:
        check_image(L, run(lib, L, IMG, ypad=ypad), a, "glu|img")


# ---- 2. transposed convs -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("freq", [True, False], ids=["freq", "time"])
@pytest.mark.parametrize("case", CONVTR_CASES, ids=["Co%d-C%d" % c[:2] for c in CONVTR_CASES])
def test_transposed_conv_on_the_tap_route(lib, mode, freq, case):
    Cout, Cin, tile, sets = case
    L = layer("convtr", mode, Cin, Cout, freq)
    assert L.tile == tile
    ref = {}
    for f in sets:
        if f & IMG:
            check_image(L, run(lib, L, f, ypad=5), ref[f & ~IMG], "convtr|img")
        else:
            ref[f] = run(lib, L, f)
            check_y(L, f, ref[f], "convtr")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("freq", [True, False], ids=["freq", "time"])
def test_transposed_conv_image_behind_the_gather_table(lib, mode, freq):
    """Without wtap / xh the same scatter epilogue runs behind the table-driven gather of gemm_half.hip (route 5), which the engines
    reach when a layer has no tap image."""
    Cout, Cin, tile, _ = CONVTR_CASES[1]
    L = layer("convtr", mode, Cin, Cout, freq)
    a = run(lib, L, GR, tap=False)
    check_y(L, GR, a, "convtr, gather route")
    check_image(L, run(lib, L, GR | IMG, tap=False, ypad=5), a, "convtr|img, gather route")


# ---- 3. LINEAR with RES | IMG on the register-staged route ------------------------------------------------------------------

@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", LIN_RES_CASES, ids=["K%d-M%d-P%d" % c for c in LIN_RES_CASES])
def test_linear_res_image_on_the_register_route(lib, mode, case):
    L = layer("lin_res", mode, *case)
    a = run(lib, L, FLAG_RES, tap=False)
    check_y(L, FLAG_RES, a, "linear res")
    check_image(L, run(lib, L, FLAG_RES | IMG, tap=False, ypad=2), a, "linear res|img")


# ---- 4. encoder convs on a host-built phase-split image -----------------------------------------------------------------------

@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("freq", [True, False], ids=["freq", "time"])
@pytest.mark.parametrize("case", ENC_CASES, ids=["Co%d" % c[0] for c in ENC_CASES])
def test_encoder_conv_on_a_host_built_phase_image(lib, mode, freq, case):
    Co, tile = case
    L = layer("enc", mode, Co, freq)
    assert L.tile == tile
    check_y(L, FLAG_GELU, run(lib, L), "encoder conv")


# ---- 5. LINEAR k = 3, dilated -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dil", K3_CASES)
def test_linear_k3_dilated_on_the_tap_route(lib, mode, dil):
    L = layer("k3", mode, dil)
    assert L.tile == 128
    check_y(L, 0, run(lib, L), f"k3 dilation {dil}")


# ---- 6. neighbouring items -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("which", ["glu", "glu-img", "convtr-freq", "convtr-time"])
def test_a_nan_item_and_nan_pitch_columns_stay_out_of_the_other_item(lib, mode, which):
    """In the image the last row of item b and the first row of item b + 1 are adjacent; only the bounds test before the zero-page
    substitution keeps a tap from reading across.  One item all NaN, NaN in every pitch column: the other item's output is finite
    and bit for bit that of the all-finite run (zeros in the pitch columns)."""
    if which.startswith("glu"):
        L, flags = layer("glu", mode, *GLU_CASES[0][:5]), IMG if which == "glu-img" else 0
    else:
        L, flags = layer("convtr", mode, 32, 32, which == "convtr-freq"), GR | IMG
    clean = run(lib, L, flags, fill=0.0)
    for bad in (0, 1):
        dirty = run(lib, L, flags, nan_item=bad)
        got, ref = item_of(L, dirty, 1 - bad), item_of(L, clean, 1 - bad)
        vals = got.view(HDT[mode])[got != SENT16] if dirty.yh is not None else dirty.y[1 - bad, ..., :L.Wv]
        assert bool(torch.isfinite(vals.float()).all()), f"{which} {mode}: item {1 - bad} is not finite next to a NaN item"
        assert torch.equal(got, ref), f"{which} {mode}: item {1 - bad} differs next to a NaN item {bad}"


# ---- 7. producer feeds consumer ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", MODES)
def test_decoder_level_chained_through_its_images(lib, mode):
    """GLU|IMG rewrite -> CONVTR|GELU|RES|IMG reading that image -> 3 x 3 GLU reading that one, as an HDemucs decoder level runs them.
    Each consumer is held to float64 on the image actually read back from the device (no compounded rounding): writer and reader
    agree on the layout.  The bounds are the table's, computed on the host roundings of the float64 results."""
    Cc, Co, Fr, T, Tp = CHAIN
    hdt = HDT[mode]
    S1, S2, S3 = chain_standins(mode)
    a1 = run(lib, S1)
    check_y(S1, 0, a1, "chain 1")
    i1 = run(lib, S1, IMG)
    check_image(S1, i1, a1, "chain 1|img")
    x2 = image_to(i1.yh.cpu().view(hdt), S1.B, Fr, Tp)[..., :T].double()
    assert bool(torch.isfinite(x2).all())
    _, L2, _ = chain_layers(mode, x2=x2, x3=S3.x)
    a2 = run(lib, L2, GR, xh=i1.yh)
    check_y(L2, GR, a2, "chain 2")
    i2 = run(lib, L2, GR | IMG, xh=i1.yh, ypad=3)
    check_image(L2, i2, a2, "chain 2|img")
    x3 = image_to(i2.yh.cpu().view(hdt), L2.B, 4 * Fr, Tp)[..., :T].double()
    assert bool(torch.isfinite(x3).all())
    _, _, L3 = chain_layers(mode, x2=x2, x3=x3)
    check_y(L3, 0, run(lib, L3, xh=i2.yh), "chain 3")
