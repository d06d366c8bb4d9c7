"""The half modes' linear kernels alone (gemm_half.hip), through `mi_conv_forward`, against float64: the operand-image kernels
`conv_gemm_half_img256_kernel` (512 threads, 4-stage DMA ring; LN|HEADS, LN|GELU|IMG, and SCALE|RES under MI_IMG256=1) and
`conv_gemm_half_img_kernel<TM = 2, 4>` (3-stage ring; SCALE|RES[|STATS]), and the register-staged `conv_gemm_half_kernel` on 128- and
256-row tiles with the flag sets of the MI_NO_INPUT_IMAGE / MI_NO_FFN_IMAGE / MI_NO_QKV_HEADS fall-backs.

Inputs are general float64 draws: x ~ N(0.5, 1) (so the LayerNorm fold's mean * c1 term matters), W ~ N(0, 1 / K).  The test rounds
x (through float32, as the device does) and W to the operand type itself and builds the input image [K / 8][xh_n][8] on the host;
the rounded weights go in as float32 [Kpad][Mpad] and the library's `mi_conv_pack_half` lays them out as the gather-free image
Wh[K / 8][Mpad][8] (exact on rounded values): that packer is part of what is under test.  Image octets past K / 8 (the image has ceil(K / 32) * 4) and image columns past N hold NaN and must never reach a product.

Reference: float64 on the rounded operands, from the definition in csrc/gemm_conv.h,
    v = rstd[n] * (acc - mean[n] * c1[m]) + c2[m],  GELU (erf form),  * scale[m],  + res
with (mean, rstd) the true per-token statistics of the raw x (float64, cast to float32), c1 = sum_k W'[m][k] of the rounded
weights (float64, cast to float32).

Bounds.  None is taken from the kernels.  RESTATED[(family, type, K)] is the largest distance of the SAME formula evaluated in torch
float32 on the CPU from float64, over every case of the family in this file; float32 outputs get 4x that (the kernels sum in another
order); 16-bit outputs (HEADS, IMG) get that plus half an ulp of the output type at |want| (for |want| in [2^(e-1), 2^e): 2^(e-9)
bf16, 2^(e-12) f16, at least 2^-25 for f16's subnormals).  On the register-staged route the 16-bit tensor must equal the rounding of
the float32 y of the same launch without IMG / HEADS bit for bit.  STATS: the 32 slots of an item summed in float64 against the float64
sums of the stored y itself (each lane adds at most 64 values in float32 before its float64 reduction: 64 * 2^-24 * sum|y|, 65 *
2^-24 * sum y^2) and against the reference (count * bound more).  Every case prints restated, kernel, bound and their ratio.

After every launch `mi_debug_last_conv_route` / `mi_debug_last_conv_tile` must name the family and the tile that the rules of
conv_route (csrc/conv_route.hip) give for the descriptor under the switches the process was started with.

Every launch passes a caller-owned sink -- guard, 256 dump floats, 64 zeros, guard -- and the zeros and guards must survive: the
512-thread kernel's SCALE|RES form used to store its masked values over the zero page (and past a 320-float sink)."""
import ctypes as C
import functools
import os
import re
import subprocess
import sys
from types import SimpleNamespace

import pytest
import torch
import torch.nn.functional as F

from demucs_amd import _lib
from gpu_helpers import EPI_LINEAR, FLAG_GELU, FLAG_RES, FLAG_SCALE, SLOTS, conv_desc, ktab, pack_vec, pack_w

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LN, IMG, HEADS, STATS = 32, 64, 128, 256
HDT = {"bf16": torch.bfloat16, "f16": torch.float16}
DT = {"bf16": 1, "f16": 2}
MODES = ["bf16", "f16"]
EPS = 1e-5
SINK, ZERO, GUARD, GUARD_VALUE = 256, 64, 64, -12345.0          # csrc/gemm_conv.h MI_SINK_FLOATS, MI_ZERO_PAGE_FLOATS
SENT16 = 0x5A5A                                                  # 16-bit outputs start as this pattern
KS = [8, 32, 40, 64, 96, 128, 160, 512]     # one live octet; nk = 1; nk = 2 with a masked tail; 64; 3- and 4-stage ring full; first reuse; the model's
NS = [1, 31, 64, 127, 128, 129, 255, 256, 257, 2049]             # around the 128- / 256-column tiles; 2049: NT = 9, a second XCD group
HALF, HALF_IMG, HALF_IMG256 = 5, 9, 10                          # enum mi_conv_route (include/demucs_amd.h)
FAMILY = {LN: "ln", LN | FLAG_GELU: "ln_gelu", FLAG_SCALE | FLAG_RES: "scale_res", FLAG_RES: "res"}

# largest max-abs distance of the float32 restatement from float64 over the family's cases, {(family, type, K): distance}
RESTATED = {
    ('ln', 'bf16', 8): 3.78e-07, ('ln', 'bf16', 32): 6.45e-07, ('ln', 'bf16', 40): 6.80e-07, ('ln', 'bf16', 64): 1.33e-06,
    ('ln', 'bf16', 96): 9.51e-07, ('ln', 'bf16', 128): 1.07e-06, ('ln', 'bf16', 160): 1.39e-06, ('ln', 'bf16', 512): 1.24e-06,
    ('ln', 'f16', 8): 8.21e-07, ('ln', 'f16', 32): 1.35e-06, ('ln', 'f16', 40): 2.02e-06, ('ln', 'f16', 64): 2.02e-06,
    ('ln', 'f16', 96): 2.00e-06, ('ln', 'f16', 128): 1.99e-06, ('ln', 'f16', 160): 2.35e-06, ('ln', 'f16', 512): 2.30e-06,
    ('ln_gelu', 'bf16', 8): 5.25e-07, ('ln_gelu', 'bf16', 32): 7.62e-07, ('ln_gelu', 'bf16', 40): 6.24e-07, ('ln_gelu', 'bf16', 64): 1.31e-06,
    ('ln_gelu', 'bf16', 96): 8.50e-07, ('ln_gelu', 'bf16', 128): 8.73e-07, ('ln_gelu', 'bf16', 160): 1.44e-06, ('ln_gelu', 'bf16', 512): 1.03e-06,
    ('ln_gelu', 'f16', 8): 9.93e-07, ('ln_gelu', 'f16', 32): 1.15e-06, ('ln_gelu', 'f16', 40): 1.09e-06, ('ln_gelu', 'f16', 64): 2.15e-06,
    ('ln_gelu', 'f16', 96): 1.80e-06, ('ln_gelu', 'f16', 128): 1.95e-06, ('ln_gelu', 'f16', 160): 2.69e-06, ('ln_gelu', 'f16', 512): 1.94e-06,
    ('res', 'bf16', 32): 5.96e-07, ('res', 'bf16', 64): 1.04e-06, ('res', 'bf16', 96): 8.64e-07, ('res', 'bf16', 160): 1.16e-06,
    ('res', 'bf16', 512): 9.93e-07, ('res', 'f16', 32): 9.83e-07, ('res', 'f16', 64): 1.97e-06, ('res', 'f16', 96): 1.58e-06,
    ('res', 'f16', 160): 2.26e-06, ('res', 'f16', 512): 2.35e-06, ('scale_res', 'bf16', 8): 8.11e-07, ('scale_res', 'bf16', 32): 7.78e-07,
    ('scale_res', 'bf16', 40): 8.17e-07, ('scale_res', 'bf16', 64): 1.68e-06, ('scale_res', 'bf16', 96): 9.70e-07, ('scale_res', 'bf16', 128): 1.19e-06,
    ('scale_res', 'bf16', 160): 1.19e-06, ('scale_res', 'bf16', 512): 1.23e-06, ('scale_res', 'f16', 8): 8.95e-07, ('scale_res', 'f16', 32): 1.25e-06,
    ('scale_res', 'f16', 40): 1.37e-06, ('scale_res', 'f16', 64): 2.58e-06, ('scale_res', 'f16', 96): 2.19e-06, ('scale_res', 'f16', 128): 2.16e-06,
    ('scale_res', 'f16', 160): 2.52e-06, ('scale_res', 'f16', 512): 3.80e-06,
}


def heads_cases():
    """LN|HEADS on the 256 x 256 kernel: (K, B, T, M, extra image columns, extra yh token rows)."""
    cs = [(K, 2, 40, 512, 0, 5 if i % 2 else 0) for i, K in enumerate(KS)]
    cs += [(64, 1, T, 512, 3, 0) for T in NS]
    cs += [(64, 3, 33, 512, 3, 5), (64, 2, 40, 1024, 3, 0), (64, 2, 40, 1024, 0, 5), (64, 2, 40, 1536, 3, 0), (64, 2, 40, 1536, 0, 5)]
    return cs


def ffn_cases():
    """LN|GELU|IMG on the 256 x 256 kernel; M = 248: the last octet of the 256-row tile is masked."""
    return [(K, 2, 40, 256, 0, 2) for K in KS] + [(64, 1, T, 248, 3, 2) for T in NS] + [(64, 3, 33, 256, 3, 0), (64, 3, 33, 248, 0, 2)]


def res_cases():
    """SCALE|RES (and, from T = 32 on, SCALE|RES|STATS) on the 3-stage kernel: TM = 2 (M = 120, 128, 384), TM = 4 (256, 512)."""
    cs = [(K, 2, 40, M, 0, 0) for M in (128, 256) for K in KS]
    cs += [(64, 1, T, M, 3, 0) for M in (120, 256) for T in NS]
    cs += [(64, 3, 33, M, 3, 0) for M in (120, 128, 256, 384, 512)] + [(64, 2, 40, M, 3, 0) for M in (120, 384, 512)]
    return cs


REG_SHAPES = [(K, 2, 40, 256) for K in (32, 96, 160, 512)] + \
             [(64, B, T, M) for M in (128, 256) for B, T in ((1, 4), (1, 128), (1, 132), (1, 260), (3, 36), (2, 40))]
REG_HEADS_SHAPES = [(64, 2, 40, 512), (96, 3, 36, 512), (64, 1, 132, 1024)]
IMG256_CHILD = [(K, 2, 40, 256, 0, 0) for K in (8, 40, 128, 160)] + [(64, 1, T, 256, 3, 0) for T in (1, 129, 257, 2049)] + \
               [(64, 3, 33, 512, 3, 0), (64, 3, 33, 120, 3, 0)]
TILE128_CHILD = [(64, 2, 40, 256), (160, 3, 36, 256), (64, 1, 132, 256)]


def family_cases():
    """Every (family, K, B, T, M) this file runs: the cases RESTATED is a maximum over."""
    out = set()
    for K, B, T, M, _, _ in heads_cases():
        out.add(("ln", K, B, T, M))
    for K, B, T, M, _, _ in ffn_cases():
        out.add(("ln_gelu", K, B, T, M))
    for K, B, T, M, _, _ in res_cases() + IMG256_CHILD:
        out.add(("scale_res", K, B, T, M))
    for K, B, T, M in REG_SHAPES + TILE128_CHILD:
        out.update({("ln", K, B, T, M), ("ln_gelu", K, B, T, M), ("res", K, B, T, M)})
    for K, B, T, M in REG_HEADS_SHAPES:
        out.add(("ln", K, B, T, M))
    out.add(("ln", 64, 2, 40, 1536))        # the attention case
    return sorted(out)


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return _lib.load()


def stream():
    return C.c_void_p(_lib.current_stream_ptr())


def same_bits(a, b):
    a, b = a.contiguous(), b.contiguous()
    if a.dtype == torch.float32:
        a, b = a.view(torch.int32), b.view(torch.int32)
    return a.shape == b.shape and torch.equal(a, b)


# ---- operands and references (CPU) -------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=6)
def operands(mode, K, B, T, M):
    g = torch.Generator().manual_seed(1000003 * K + 10007 * B + 101 * T + M + (1 << 24) * DT[mode])
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    o = SimpleNamespace(mode=mode, K=K, B=B, T=T, M=M, N=B * T)
    o.x32 = (0.5 + rn(B, K, T)).float()                                   # the raw input: what the statistics are taken over
    o.xr = o.x32.to(HDT[mode])                                            # its rounding to the operand type
    o.Wr = (rn(M, K) * K ** -0.5 * (1 + 0.2 * rn(K))).float().to(HDT[mode])     # W' = W diag(ln_w), rounded
    xd = o.x32.double()
    mean, var = xd.mean(1), xd.var(1, unbiased=False)
    o.st = torch.stack([mean, 1.0 / torch.sqrt(var + EPS)], -1).reshape(B * T, 2).float().contiguous()
    o.c1 = o.Wr.double().sum(1).float()
    o.c2 = (0.3 * rn(M)).float()
    o.scale = (1 + 0.3 * rn(M)).float()
    o.res = rn(B, M, T).float()
    o.want, o.dev = {}, None
    return o


def formula(o, flags, dt):
    """The epilogue's definition (csrc/gemm_conv.h) on the rounded operands, in `dt`."""
    acc = torch.einsum("mk,bkt->bmt", o.Wr.to(dt), o.xr.to(dt))
    col = lambda v: v.to(dt)[None, :, None]
    if flags & LN:
        st = o.st.to(dt).view(o.B, o.T, 2)
        v = st[:, None, :, 1] * (acc - st[:, None, :, 0] * col(o.c1)) + col(o.c2)
    else:
        v = acc + col(o.c2)
    if flags & FLAG_GELU:
        v = F.gelu(v)
    if flags & FLAG_SCALE:
        v = v * col(o.scale)
    if flags & FLAG_RES:
        v = v + o.res.to(dt)
    return v


def want_of(o, flags):
    f = flags & (LN | FLAG_GELU | FLAG_SCALE | FLAG_RES)
    if f not in o.want:
        w = formula(o, f, torch.float64)
        o.want[f] = (w, (formula(o, f, torch.float32).double() - w).abs().max().item())
    return o.want[f]


def bound32(o, flags):
    return 4 * RESTATED[(FAMILY[flags & (LN | FLAG_GELU | FLAG_SCALE | FLAG_RES)], o.mode, o.K)]


def half_ulp(want, mode):
    _, e = torch.frexp(want.abs())                                        # |want| in [2^(e-1), 2^e)
    h = torch.ldexp(torch.ones_like(want), e - (9 if mode == "bf16" else 12))
    return h if mode == "bf16" else h.clamp_min(2.0 ** -25)


def report(o, flags, what, err, bound):
    fam = FAMILY[flags & (LN | FLAG_GELU | FLAG_SCALE | FLAG_RES)]
    print(f"{what} {fam} {o.mode} K {o.K} B {o.B} T {o.T} M {o.M}: restated {want_of(o, flags)[1]:.2e}  kernel {err:.2e}  "
          f"bound {bound:.2e}  ratio {err / bound:.2f}")


# ---- launches ------------------------------------------------------------------------------------------------------------

def device_side(o):
    if o.dev is None:
        d = SimpleNamespace()
        d.wt, d.bias, _, d.Mpad, _, d.Kpad, _ = pack_w(o.Wr.float(), o.c2, tile=128)
        d.c1, d.scale = pack_vec(o.c1, d.Mpad), pack_vec(o.scale, d.Mpad)
        d.st, d.res, d.x = o.st.cuda(), o.res.cuda(), o.x32.cuda()
        o.dev = d
    return o.dev


def image_of(o, xh_n, nan_col=None):
    """[ceil(K / 32) * 4][xh_n][8]: column n = b * T + t; NaN in the octets past K / 8 and the columns past N."""
    K8 = (o.K + 31) // 32 * 4
    img = torch.full((K8, xh_n, 8), float("nan"), dtype=HDT[o.mode])
    img[:o.K // 8, :o.N] = o.xr.permute(1, 0, 2).reshape(o.K // 8, 8, o.N).permute(0, 2, 1)
    if nan_col is not None:
        img[:, nan_col] = float("nan")
    return img.contiguous().cuda()


def new_sink():
    buf = torch.full((GUARD + SINK + ZERO + GUARD,), GUARD_VALUE, device="cuda")
    buf[GUARD:GUARD + SINK + ZERO] = 0.0
    return buf


def check_sink(buf, what):
    b = buf.cpu()
    assert bool((b[GUARD + SINK:GUARD + SINK + ZERO] == 0).all()), f"{what}: the zero page behind the sink was written"
    assert bool((b[:GUARD] == GUARD_VALUE).all()) and bool((b[-GUARD:] == GUARD_VALUE).all()), f"{what}: store outside the sink"


def describe(o, flags, xh=True, xpad=0, ypad=0, nan_col=None, **over):
    """The descriptor of one launch and its output tensors: y starts as NaN, yh as SENT16, the statistics as zero."""
    d = device_side(o)
    B, K, T, M, N = o.B, o.K, o.T, o.M, o.N
    out = SimpleNamespace(sink=new_sink(), y=torch.full((B, M, T), float("nan"), device="cuda"), yh=None, stats=None)
    kw = dict(x6=o.mode, wt=d.wt, M=M, Mpad=d.Mpad, K=K, Kpad=d.Kpad, B=B, D1=1, D2=T, O1=1, O2=T, S1=1, S2=1, plain=1, tile_m=128,
              epi=EPI_LINEAR, flags=flags, bias=d.bias, y=out.y, y_bstride=M * T, y_cstride=T, sink=out.sink[GUARD:])
    if xh:
        kw.update(xh=image_of(o, N + xpad, nan_col), xh_n=N + xpad)
    else:
        kw.update(x=d.x, x_bstride=K * T, ktab=ktab(K, 1, 1, 1, 1, 0, 0, T, T, d.Kpad))
    if flags & LN:
        kw.update(scale=d.c1, pro_stats=d.st)
    if flags & FLAG_SCALE:
        kw.update(scale=d.scale)
    if flags & FLAG_RES:
        kw.update(res=d.res)
    if flags & HEADS:
        out.yh = torch.full((max(1, M // 512), B, 8, T + ypad, 64), SENT16, dtype=torch.int16, device="cuda")
        kw.update(yh=out.yh, yh_n=T + ypad)
    if flags & IMG:
        out.yh = torch.full((d.Mpad // 8, N + ypad, 8), SENT16, dtype=torch.int16, device="cuda")
        kw.update(yh=out.yh, yh_n=N + ypad)
    if flags & STATS:
        out.stats = torch.zeros(B, SLOTS, 2, dtype=torch.float64, device="cuda")
        kw.update(stats=out.stats)
    kw.update(over)
    return kw, out


@functools.lru_cache(maxsize=1)
def switches(lib):
    """The MI_* switches as the library parsed them when it was loaded."""
    n = lib.mi_debug_switches(None, 0)
    buf = C.create_string_buffer(n + 1)
    lib.mi_debug_switches(buf, n + 1)
    return dict(line.split("=", 1) for line in buf.value.decode().splitlines())


def expected_route(lib, o, flags, xh):
    """(route, tile): the 512-thread kernel for LN|HEADS and LN|GELU|IMG (and, under MI_IMG256=1, for SCALE|RES where Mpad % 256 == 0);
    the 3-stage kernel for SCALE|RES[|STATS], 256 rows where Mpad % 256 == 0, else 128; without an input image the register-staged
    kernel, 256 rows where Mpad % 256 == 0 unless MI_HALF_TILE256=0."""
    wide = device_side(o).Mpad % 256 == 0
    if not xh:
        return HALF, 256 if wide and switches(lib)["MI_HALF_TILE256"] == "1" else 128
    if flags & LN or (switches(lib)["MI_IMG256"] == "1" and wide and not flags & STATS):
        return HALF_IMG256, 256
    return HALF_IMG, 256 if wide else 128


def run(lib, o, flags, **opt):
    kw, out = describe(o, flags, **opt)
    desc, keep = conv_desc(**kw)
    _lib.check(lib.mi_conv_forward(C.byref(desc), stream()), "mi_conv_forward")
    torch.cuda.synchronize()
    took, want = (lib.mi_debug_last_conv_route(), lib.mi_debug_last_conv_tile()), expected_route(lib, o, flags, opt.get("xh", True))
    assert took == want, f"flags {flags} {o.mode} K {o.K} B {o.B} T {o.T} M {o.M}: (route, tile) {took}, expected {want}"
    check_sink(out.sink, f"flags {flags} {o.mode} K {o.K} B {o.B} T {o.T} M {o.M}")
    del keep
    return out


def run_twice(lib, o, flags, **opt):
    """Non-atomic outputs repeat bit for bit."""
    a, b = run(lib, o, flags, **opt), run(lib, o, flags, **opt)
    assert same_bits(a.y, b.y), "y differs between two launches"
    assert a.yh is None or same_bits(a.yh, b.yh), "yh differs between two launches"
    return a


# ---- checks ----------------------------------------------------------------------------------------------------------------

def check_y(o, flags, out, what):
    want, _ = want_of(o, flags)
    y = out.y.cpu()
    assert bool(torch.isfinite(y).all()), f"{what}: non-finite y"
    err, bound = (y.double() - want).abs().max().item(), bound32(o, flags)
    report(o, flags, what, err, bound)
    assert err <= bound, f"{what}: {err:.3e} > {bound:.3e}"


def check_half(o, flags, got, want, what):
    """got: the 16-bit values as float64, laid out like want."""
    assert bool(torch.isfinite(got).all()), f"{what}: non-finite 16-bit output"
    b32 = bound32(o, flags)
    excess = ((got - want).abs() - half_ulp(want, o.mode)).max().item()
    report(o, flags, what, max(excess, 0.0), b32)
    assert excess <= b32, f"{what}: {excess:.3e} beyond half an ulp > {b32:.3e}"


def heads_perm(v, pitch):
    """(B, M, T) -> [M / 512][B][8][pitch][64], token rows past T dropped: the layout csrc/gemm_conv.h states for MI_FLAG_HEADS."""
    B, M, T = v.shape
    return v.view(B, M // 512, 8, 64, T).permute(1, 0, 2, 4, 3)


def check_heads(o, flags, out, what):
    assert bool(torch.isnan(out.y).all()), f"{what}: HEADS wrote y"
    yh = out.yh.cpu()
    assert bool((yh[:, :, :, o.T:] == SENT16).all()), f"{what}: token rows past T written"
    got = yh[:, :, :, :o.T].contiguous().view(HDT[o.mode]).double()
    check_half(o, flags, got, heads_perm(want_of(o, flags)[0], o.T), what)


def image_perm(v, octets):
    """(B, M, T) -> [M / 8][N][8], n = b * T + t."""
    B, M, T = v.shape
    return v.permute(1, 0, 2).reshape(octets, 8, B * T).permute(0, 2, 1)


def check_image(o, flags, out, what):
    assert bool(torch.isnan(out.y).all()), f"{what}: IMG wrote y"
    yh, oc = out.yh.cpu(), o.M // 8
    assert bool((yh[:, o.N:] == SENT16).all()) and bool((yh[oc:] == SENT16).all()), f"{what}: image columns past N / octets past M written"
    got = yh[:oc, :o.N].contiguous().view(HDT[o.mode]).double()
    check_half(o, flags, got, image_perm(want_of(o, flags)[0], oc), what)


def check_stats(o, flags, out, what):
    """The item sums against the stored y itself (float32 lane partials only) and against the reference."""
    y, want = out.y.cpu().double(), want_of(o, flags)[0]
    got = out.stats.cpu().sum(1)                                           # (B, 2)
    s1, s2 = y.sum((1, 2)), (y * y).sum((1, 2))
    a1, a2 = y.abs().sum((1, 2)), s2
    t1, t2 = 64 * 2.0 ** -24 * a1, 65 * 2.0 ** -24 * a2
    e1, e2 = (got[:, 0] - s1).abs(), (got[:, 1] - s2).abs()
    print(f"{what}: sums vs stored y {float((e1 / t1).max()):.3f} / {float((e2 / t2).max()):.3f} of the lane-partial bound")
    assert bool((e1 <= t1).all()) and bool((e2 <= t2).all()), f"{what}: item sums differ from the sums of the stored y"
    b32, cnt = bound32(o, flags), o.M * o.T
    r1 = (got[:, 0] - want.sum((1, 2))).abs()
    r2 = (got[:, 1] - (want * want).sum((1, 2))).abs()
    assert bool((r1 <= t1 + cnt * b32).all()), f"{what}: item sum differs from the reference"
    assert bool((r2 <= t2 + b32 * (2 * want.abs().sum((1, 2)) + cnt * b32)).all()), f"{what}: item sum of squares differs from the reference"


def ids(cs):
    return ["K%d-B%d-T%d-M%d-x%d-y%d" % c for c in cs]


# ---- the operand-image kernels ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", heads_cases(), ids=ids(heads_cases()))
def test_img256_ln_heads(lib, mode, case):
    K, B, T, M, xpad, ypad = case
    o = operands(mode, K, B, T, M)
    check_heads(o, LN | HEADS, run_twice(lib, o, LN | HEADS, xpad=xpad, ypad=ypad), "img256 heads")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", ffn_cases(), ids=ids(ffn_cases()))
def test_img256_ln_gelu_img(lib, mode, case):
    K, B, T, M, xpad, ypad = case
    o = operands(mode, K, B, T, M)
    check_image(o, LN | FLAG_GELU | IMG, run_twice(lib, o, LN | FLAG_GELU | IMG, xpad=xpad, ypad=ypad), "img256 image")


def scale_res_case(lib, o, xpad, what):
    f = FLAG_SCALE | FLAG_RES
    a = run_twice(lib, o, f, xpad=xpad)
    check_y(o, f, a, what)
    if o.T >= 32:
        s = run(lib, o, f | STATS, xpad=xpad)
        assert same_bits(s.y, a.y), f"{what}: STATS changes y"
        check_stats(o, f, s, what + " stats")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", res_cases(), ids=ids(res_cases()))
def test_img_scale_res_stats(lib, mode, case):
    K, B, T, M, xpad, _ = case
    scale_res_case(lib, operands(mode, K, B, T, M), xpad, "img scale_res")


@pytest.mark.parametrize("mode", MODES)
def test_heads_feed_attention(lib, mode):
    """The QKV projection's output is exactly what `mi_attention_heads` reads: float64 softmax of the tensors the kernel wrote,
    decoded by the stated layout (which test_img256_ln_heads holds to the reference), at the bounds of
    test_gpu_kernels.py::test_attention_heads_matches_softmax for un-spiked data."""
    B, T, pitch = 2, 40, 45
    o = operands(mode, 64, B, T, 1536)
    out = run(lib, o, LN | HEADS, xpad=3, ypad=pitch - T)
    check_heads(o, LN | HEADS, out, "qkv heads")
    q, k, v = (out.yh[i, :, :, :T].contiguous().view(HDT[mode]).double().cpu() for i in range(3))       # (B, 8, T, 64)
    want = (torch.softmax(q @ k.transpose(-1, -2) / 8.0, dim=-1) @ v).transpose(2, 3).reshape(B, 512, T)
    att = torch.full((B, 512, T), float("nan"), device="cuda")
    _lib.check(lib.mi_attention_heads(out.yh[0].data_ptr(), out.yh[1].data_ptr(), out.yh[2].data_ptr(), att.data_ptr(), B, 8, T, T,
                                      pitch, pitch, DT[mode], stream()), "mi_attention_heads")
    torch.cuda.synchronize()
    err = (att.cpu().double() - want).abs().max().item()
    print(f"attention on the projected heads, {mode}: {err:.2e}")
    assert bool(torch.isfinite(att).all()) and err < {"bf16": 6e-3, "f16": 8e-4}[mode]


@pytest.mark.parametrize("mode", MODES)
def test_nan_token_stays_in_its_column(lib, mode):
    """A NaN image column changes that token's outputs only -- and under STATS its item's sums only; the rest bit for bit."""
    K, B, T, bad = 64, 3, 33, 33 + 17                                     # a token of item 1
    for flags, M in ((LN | HEADS, 512), (LN | FLAG_GELU | IMG, 248), (FLAG_SCALE | FLAG_RES | STATS, 256), (FLAG_SCALE | FLAG_RES | STATS, 384)):
        o = operands(mode, K, B, T, M)
        clean, dirty = run(lib, o, flags, xpad=3), run(lib, o, flags, xpad=3, nan_col=bad)
        if flags & HEADS:
            c, d = clean.yh.view(HDT[mode]).cpu(), dirty.yh.view(HDT[mode]).cpu()          # [1][B][8][T][64]
            assert bool(torch.isnan(d[0, 1, :, 17]).all())
            d[0, 1, :, 17] = c[0, 1, :, 17]
        elif flags & IMG:
            c, d = clean.yh.view(HDT[mode]).cpu(), dirty.yh.view(HDT[mode]).cpu()          # [Mpad / 8][N][8]
            assert bool(torch.isnan(d[:M // 8, bad]).all())
            d[:, bad] = c[:, bad]
        else:
            c, d = clean.y.cpu(), dirty.y.cpu()
            assert bool(torch.isnan(d[1, :, 17]).all())
            d[1, :, 17] = c[1, :, 17]
            cs, ds = clean.stats.cpu(), dirty.stats.cpu()
            assert bool(torch.isnan(ds[1].sum(0)).all()), "the NaN token is missing from its item's sums"
            assert torch.equal(cs[0], ds[0]) and torch.equal(cs[2], ds[2]), "a NaN token changed another item's sums"
        assert torch.equal(c.view(torch.int16) if c.dtype != torch.float32 else c.view(torch.int32),
                           d.view(torch.int16) if d.dtype != torch.float32 else d.view(torch.int32)), f"flags {flags}: NaN spread"


# ---- the register-staged route --------------------------------------------------------------------------------------------

def reg_case(lib, o, what):
    """LN, LN|GELU, RES against float64; LN|GELU|IMG and RES|IMG bit for bit the rounding of the float32 y of the launch without IMG."""
    for f in (LN, LN | FLAG_GELU, FLAG_RES):
        a = run_twice(lib, o, f, xh=False)
        check_y(o, f, a, f"{what} y")
        if f == LN:
            continue
        b = run_twice(lib, o, f | IMG, xh=False, ypad=2)
        check_image(o, f | IMG, b, f"{what} image")
        oc = o.M // 8
        rounded = image_perm(a.y.cpu(), oc).to(HDT[o.mode]).contiguous().view(torch.int16)
        assert torch.equal(b.yh.cpu()[:oc, :o.N], rounded), f"{what}: image != rounding of y (flags {f})"


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", REG_SHAPES, ids=["K%d-B%d-T%d-M%d" % s for s in REG_SHAPES])
def test_register_route(lib, mode, shape):
    reg_case(lib, operands(mode, *shape), "reg")


def reg_heads_case(lib, o, what):
    a, b = run_twice(lib, o, LN, xh=False), run_twice(lib, o, LN | HEADS, xh=False, ypad=5)
    check_y(o, LN, a, f"{what} y")
    check_heads(o, LN | HEADS, b, f"{what} heads")
    rounded = heads_perm(a.y.cpu(), o.T).to(HDT[o.mode]).contiguous().view(torch.int16)
    assert torch.equal(b.yh.cpu()[:, :, :, :o.T], rounded), f"{what}: heads != rounding of y"


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", REG_HEADS_SHAPES, ids=["K%d-B%d-T%d-M%d" % s for s in REG_HEADS_SHAPES])
def test_register_route_heads(lib, mode, shape):
    reg_heads_case(lib, operands(mode, *shape), "reg")


# ---- refusals --------------------------------------------------------------------------------------------------------------

def test_refusals_launch_nothing(lib):
    o = operands("bf16", 64, 2, 40, 512)
    o36 = operands("bf16", 40, 2, 40, 256)
    launches = [0]
    hook = C.CFUNCTYPE(None, C.c_void_p)(lambda st: launches.__setitem__(0, launches[0] + 1))

    def refused(o, flags, needle, edit=None, **over):
        kw, out = describe(o, flags, **over)
        desc, keep = conv_desc(**kw)
        if edit:
            edit(desc)
        torch.cuda.synchronize()
        launches[0] = 0
        lib.mi_debug_set_post_launch_hook(hook)
        try:
            rc = lib.mi_conv_forward(C.byref(desc), stream())
        finally:
            lib.mi_debug_set_post_launch_hook(None)
        torch.cuda.synchronize()
        msg = lib.mi_last_error().decode()
        assert rc != 0 and needle in msg, (rc, msg)
        assert launches[0] == 0, f"{needle}: {launches[0]} launches"
        assert bool(torch.isnan(out.y).all()) and (out.yh is None or bool((out.yh == SENT16).all()))
        check_sink(out.sink, needle)

    def bump(field):
        return lambda d: setattr(d, field, getattr(d, field) + 8)

    refused(o, FLAG_GELU, "not instantiated")                                             # xh with a flag set that has no kernel
    refused(operands("bf16", 64, 2, 40, 128), LN | FLAG_GELU | IMG, "256-row tile")       # Mpad = 128 on the 256-row kernel
    refused(o36, LN | FLAG_GELU | IMG, "K % 8", K=36)                                     # K % 8 != 0 (Kpad = 48 either way)
    refused(o, LN | HEADS, "operand image has", xh_n=o.N - 1)                             # image narrower than the tensor
    refused(operands("bf16", 64, 2, 40, 256), LN | HEADS, "MI_FLAG_HEADS")                # M % 512 != 0
    refused(o, LN | HEADS, "MI_FLAG_HEADS", O1=2, O2=20, D1=2, D2=20)                     # tokens as a 2 x 20 frame
    refused(o, LN | HEADS, "K % 8", edit=bump("xh"))                                      # xh 8 bytes off
    refused(o, LN | HEADS, "MI_FLAG_HEADS", edit=bump("yh"))                              # yh 8 bytes off
    refused(operands("bf16", 64, 2, 40, 256), LN | FLAG_GELU | IMG, "MI_FLAG_IMG", edit=bump("yh"))


# ---- the default and the switch routes, each in one fresh process --------------------------------------------------------------------------

def kernel_names(fn):
    """Names of the device kernels launched inside fn(), from the profiler's device activity records."""
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return {e.name for e in prof.events() if str(e.device_type).endswith("CUDA")}


def child_main(which):
    lib = _lib.load()
    got = switches(lib)
    # what run() holds every launch below to, spelled out for this child's switches: (M, flags, input image) -> (route, tile)
    SR = FLAG_SCALE | FLAG_RES
    pinned = {"default": {(512, LN | HEADS, True): (HALF_IMG256, 256), (256, SR, True): (HALF_IMG, 256), (384, SR | STATS, True): (HALF_IMG, 128),
                          (256, LN, False): (HALF, 256), (128, LN, False): (HALF, 128)},
              "img256": {(256, SR, True): (HALF_IMG256, 256), (512, SR, True): (HALF_IMG256, 256), (120, SR, True): (HALF_IMG, 128),
                         (256, SR | STATS, True): (HALF_IMG, 256)},
              "tile128": {(256, LN, False): (HALF, 128), (512, LN | HEADS, False): (HALF, 128)}}[which]
    for (M, flags, xh), want in pinned.items():
        assert expected_route(lib, operands("bf16", 64, 2, 40, M), flags, xh) == want, (which, M, flags, xh)

    def body():
        for mode in MODES:
            if which == "default":
                check_heads(operands(mode, 64, 2, 40, 512), LN | HEADS, run(lib, operands(mode, 64, 2, 40, 512), LN | HEADS), "img256 heads")
                check_image(operands(mode, 64, 2, 40, 256), LN | FLAG_GELU | IMG, run(lib, operands(mode, 64, 2, 40, 256), LN | FLAG_GELU | IMG),
                            "img256 image")
                for M in (256, 384):
                    scale_res_case(lib, operands(mode, 64, 2, 40, M), 0, "img scale_res")
                for M in (128, 256):
                    check_y(operands(mode, 64, 2, 40, M), LN, run(lib, operands(mode, 64, 2, 40, M), LN, xh=False), "reg y")
            elif which == "img256":
                for K, B, T, M, xpad, _ in IMG256_CHILD:
                    scale_res_case(lib, operands(mode, K, B, T, M), xpad, "img256 scale_res")
            else:
                for shape in TILE128_CHILD:
                    reg_case(lib, operands(mode, *shape), "reg tile128")
                reg_heads_case(lib, operands(mode, *REG_HEADS_SHAPES[0]), "reg tile128")
    names = kernel_names(body)
    print("kernels:", *sorted(k for k in names if "conv_gemm_half" in k), sep="\n  ")
    # kernel name and template arguments alone (no return type, namespace or signature): {("conv_gemm_half_img_kernel", "1,4,6"), ...}
    gemm = {(m.group(1), re.sub(r"\(int\)|\s", "", m.group(2))) for m in (re.search(r"(conv_gemm_half\w*)<([^>]*)>", k) for k in names) if m}
    img256, img, reg = "conv_gemm_half_img256_kernel", "conv_gemm_half_img_kernel", "conv_gemm_half_kernel"
    hts = ("1", "2")
    if which == "default":
        assert got["MI_IMG256"] == "0" and got["MI_HALF_TILE256"] == "1"
        # LN|HEADS (160) and LN|GELU|IMG (97) on the 512-thread kernel; SCALE|RES (6) and with STATS (262) on the 3-stage one, TM = 4
        # (Mpad 256) and TM = 2 (Mpad 384); the register-staged LN (32) on the 256-row <2, 2, 4, 2> and the 128-row <2, 2, 2, 2> tile
        assert gemm == {(k, f"{ht},{a}") for ht in hts for k, a in (
            (img256, "160"), (img256, "97"), (img, "4,6"), (img, "4,262"), (img, "2,6"), (img, "2,262"),
            (reg, "2,2,2,2,0,32,true"), (reg, "2,2,4,2,0,32,true"))}, gemm
    elif which == "img256":
        assert got["MI_IMG256"] == "1"
        # SCALE|RES (6): Mpad = 256 / 512 on the 512-thread kernel, M = 120 (Mpad 128) on the 3-stage one with TM = 2 and never with
        # TM = 4; STATS (262) stays on the 3-stage kernel
        assert gemm == {(k, f"{ht},{a}") for ht in hts for k, a in ((img256, "6"), (img, "2,6"), (img, "2,262"), (img, "4,262"))}, gemm
    else:
        assert got["MI_HALF_TILE256"] == "0"
        # <HT, WM, WN, TM, TN, EPI, LFLAGS, PLAIN>: only the 128-row tile <2, 2, 2, 2>, for LN, LN|GELU, LN|GELU|IMG, RES, RES|IMG, LN|HEADS
        assert gemm == {(reg, f"{ht},2,2,2,2,0,{f},true") for ht in hts for f in (32, 33, 97, 4, 68, 160)}, gemm
    print("child ok")


_CHILD = "import sys; sys.path.insert(0, sys.argv[1]); import test_gpu_half_linear as t; t.child_main(sys.argv[2])"


@pytest.mark.parametrize("which,env", [("default", {}), ("img256", {"MI_IMG256": "1"}), ("tile128", {"MI_HALF_TILE256": "0"})])
def test_switch_route(which, env):
    e = {k: v for k, v in os.environ.items() if not k.startswith("MI_")}
    e.update(env, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-c", _CHILD, os.path.dirname(os.path.abspath(__file__)), which], env=e, capture_output=True,
                       text=True, cwd=ROOT, timeout=300)
    print(r.stdout[-6000:])
    assert r.returncode == 0 and "child ok" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
