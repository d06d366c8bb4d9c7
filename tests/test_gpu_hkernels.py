"""Kernel-level parity of the hand-written kernels that only the Hybrid Demucs (`hdemucs_mmi`) path runs (hkernels.hip), each
driven alone through the C ABI and compared with a float64 CPU reference written from the operation's definition:

  * LocalState attention (`mi_local_attn`): the matrix-pipe kernels (C = 192 / 384) and the generic one (head dimension <= 16),
  * the GroupNorm apply with its GLU / GELU / LayerScale / residual / window / row-pair forms (`mi_group_norm_apply`),
  * the BLSTM's overlapping frames (`mi_blstm_unfold`, `mi_blstm_restitch`),
  * the waveform branch's input normalisation into pitched rows (`mi_row_affine_pitch`).

Inputs are drawn in float64 from a seeded generator and rounded to float32 ONCE; the rounded values go to both sides.  Outputs
start as NaN and every padding column of every input holds NaN: padding must be neither read nor written."""
import ctypes as C
import math

import pytest
import torch
import torch.nn.functional as F

from demucs_amd import _lib
from oracle import hdemucs_oracle as HO

pytestmark = pytest.mark.gpu
NAN = float("nan")


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return _lib.load()


def stream():
    return C.c_void_p(_lib.current_stream_ptr())


def rup(v, m):
    return (v + m - 1) // m * m


def ptr(t):
    return t.data_ptr() if t is not None else None


def noise(gen, *shape):
    return torch.randn(*shape, generator=gen, dtype=torch.float64)


def padded(t, pitch):
    """t (..., n) float32 -> device rows of `pitch` columns, the columns past n NaN."""
    out = torch.full(t.shape[:-1] + (pitch,), NAN, dtype=torch.float32)
    out[..., :t.shape[-1]] = t
    return out.cuda().contiguous()


# ---- LocalState attention ------------------------------------------------------------------------------------------------------
ATTN_C = [192, 384, 16, 32, 64, 20]          # head dimensions 48, 96 (matrix pipe) and 4, 8, 16, 5 (generic kernel)
ATTN_T = [1, 2, 31, 32, 33, 63, 64, 65, 130, 257]
FAMILIES = ["plain", "spike", "rising", "diag"]
ATTN_TOL = 2e-5


def attn_inputs(Cn, T, family, B=2):
    """float32 q, k, content (B, 4, dh, T) and decay logits (B, 4, 4, T) of one input family."""
    dh = Cn // 4
    gen = torch.Generator().manual_seed(100000 * FAMILIES.index(family) + 1000 * dh + T)
    q, k, c = noise(gen, B, 4, dh, T), noise(gen, B, 4, dh, T), noise(gen, B, 4, dh, T)
    d = noise(gen, B, 4, 4, T) * 3.0
    u = noise(gen, dh)
    u = (u / u.norm())[:, None]
    if family == "spike" and T > 40:
        k[..., 40] *= 6.0                                     # a large jump of the running maximum in the middle of the stream
    elif family == "rising":
        amp = 3.0 * dh ** 0.25                                # key t scores 9 t / (T - 1) more than key 0: the maximum rises in every tile
        q = q + amp * u
        k = k + amp * u * (torch.arange(T, dtype=torch.float64) / max(T - 1, 1))
    elif family == "diag":
        a = math.sqrt(110.0 * math.sqrt(dh))                  # q . k / sqrt(dh) ~ -110, slope 2.5: the -100 of the diagonal is the largest score
        q, k = 0.05 * q + a * u, 0.05 * k - a * u
        d = torch.full_like(d, 20.0)
    return q.float(), k.float(), c.float(), d.float()


def run_local_attn(lib, q, k, c, d, ld, ld_o):
    """Pack (B, 3C + 16, ld) with NaN pitch columns, launch, return the whole (B, C, ld_o) output (NaN where nothing was written)."""
    B, _, dh, T = q.shape
    Cn = 4 * dh
    qkc = torch.cat([q.reshape(B, Cn, T), k.reshape(B, Cn, T), c.reshape(B, Cn, T), d.reshape(B, 16, T)], 1)
    qkc_d = padded(qkc, ld)
    out = torch.full((B, Cn, ld_o), NAN, device="cuda")
    _lib.check(lib.mi_local_attn(qkc_d.data_ptr(), B, Cn, T, ld, out.data_ptr(), ld_o, stream()), "mi_local_attn")
    torch.cuda.synchronize()
    return out.cpu()


def check_local_attn(lib, Cn, T, family, ld, ld_o):
    q, k, c, d = attn_inputs(Cn, T, family)
    want = HO.local_attention(q.double(), k.double(), c.double(), d.double())
    if family == "diag" and T > 1:
        # the property the family exists for: the query's OWN content comes back (its neighbours' would without the -100 fill)
        own = c.double().reshape(want.shape)
        assert float((want - own).abs().max()) < 1e-3 and float((want - own.roll(1, -1)).abs().max()) > 1.0
    out = run_local_attn(lib, q, k, c, d, ld, ld_o)
    got = out[..., :T]
    assert bool(torch.isfinite(got).all()), "non-finite output: padding or a masked key entered a product"
    assert bool(torch.isnan(out[..., T:]).all()), "the output's pitch padding was written"
    err = float((got.double() - want).abs().max())
    print(f"local_attn C {Cn} (dh {Cn // 4}) T {T} {family} ld {ld} ld_o {ld_o}: max-abs vs float64 {err:.2e}")
    assert err <= ATTN_TOL
    return got, c


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("T", ATTN_T)
@pytest.mark.parametrize("Cn", ATTN_C)
def test_local_attention_matches_float64(lib, Cn, T, family):
    """One query, the 32-key sub-tile and 64-key tile edges, the workgroup-uniform break and several key tiles; a spiked key, a
    maximum that rises in every tile (every rescale branch) and the family in which the diagonal's -100 wins the softmax.
    2e-5 is the bound of test_attention_matches_softmax for the float32 attention kernel (content N(0, 1)); the float32 torch
    restatement of the reference stays within 4.6e-6 of float64 on these families."""
    got, c = check_local_attn(lib, Cn, T, family, rup(T, 4), T)
    if T == 1:
        assert torch.equal(got[..., 0], c.reshape(got.shape)[..., 0])          # softmax over one key: weight exactly 1


@pytest.mark.parametrize("T", [33, 130])
@pytest.mark.parametrize("Cn", ATTN_C)
def test_local_attention_pitched_rows(lib, Cn, T):
    """Input rows 8 columns wider than round_up(T, 4) and output rows 5 columns wider than T, all of it NaN."""
    check_local_attn(lib, Cn, T, "plain", rup(T, 4) + 8, T + 5)


# ---- GroupNorm apply -----------------------------------------------------------------------------------------------------------
GN_TOL, GN_STAT_RTOL = 2e-5, 1e-6
GN_FORMS = {         # the call sites of HModel::group_norm
    "g1_gelu": dict(G=1, gelu=1),
    "g1_glu_scale_res": dict(G=1, glu=1, scale=True, res=True),
    "g4_gelu": dict(G=4, gelu=1),
    "g4_glu": dict(G=4, glu=1),                               # the value half and the gate half of an output channel lie in different groups
    "g4_gelu_res_off1": dict(G=4, gelu=1, res=True, off=1, extra=3, out_pad=5),
    "g4_gelu_res_off2": dict(G=4, gelu=1, res=True, off=2, extra=3, out_pad=5),
    "g4_gelu_rows8": dict(G=4, gelu=1, chan_div=8),
}
GN_LONG = 64 * 256 + 1                                        # the grid is capped at 64 blocks of 256: the stride loop's second trip


def gn_cases():
    for name, f in GN_FORMS.items():
        widths = [32, 64] if f.get("chan_div", 1) == 8 else [8, 16]
        for Cin in widths:
            for n in [1, 255, 256, 257] + ([GN_LONG] if Cin == widths[0] else []):
                yield pytest.param(name, Cin, n, id=f"{name}-C{Cin}-L{n}")


def gn_reference(x, G, w, b, glu, gelu, scale, res, off, out_len, chan_div):
    B, Cin, L = x.shape
    if chan_div > 1:                                          # rows are (channel, row) pairs: GroupNorm of the (B, c, chan_div * L) view
        n = F.group_norm(x.reshape(B, Cin // chan_div, chan_div * L), G, w, b, eps=1e-5).reshape(B, Cin, L)
    else:
        n = F.group_norm(x, G, w, b, eps=1e-5)
    n = n[..., off:off + out_len]
    if glu:
        n = n[:, :Cin // 2] * torch.sigmoid(n[:, Cin // 2:])
    if gelu:
        n = F.gelu(n)
    if scale is not None:
        n = n * scale.repeat_interleave(chan_div)[:, None]
    return n + res if res is not None else n


@pytest.mark.parametrize("form,Cin,out_len", gn_cases())
def test_group_norm_apply_matches_float64(lib, form, Cin, out_len):
    """float64 F.group_norm + the same GLU / erf-GELU / per-channel scale / residual / column window.  y within 2e-5 (the bound
    test_dconv_layer_three_passes works to for GroupNorm + GELU on inputs of this scale); the (mean, rstd) pairs within 1e-6
    relative of float64 (float64 sums rounded once, 6e-8, with headroom for the float32 partials of 16 elements); the float64
    statistic slots are zero again afterwards; pitch padding of the output stays NaN."""
    f = GN_FORMS[form]
    G, glu, gelu, off, cd = f["G"], f.get("glu", 0), f.get("gelu", 0), f.get("off", 0), f.get("chan_div", 1)
    B, in_len, Cout = 2, out_len + f.get("extra", 0), Cin // 2 if glu else Cin
    out_pitch, res_pitch = out_len + f.get("out_pad", 0), out_len + 3
    gen = torch.Generator().manual_seed(7 * Cin + out_len + 1000 * list(GN_FORMS).index(form))
    x = noise(gen, B, Cin, in_len) * 2.0 + 3.0
    x += 2.0 * (torch.arange(Cin) // (Cin // G))[None, :, None]          # another offset per group: a wrong group index shows
    nw = Cin // cd
    w, b = 1.0 + 0.5 * noise(gen, nw), noise(gen, nw)
    scale = noise(gen, Cout // cd) if f.get("scale") else None
    res = noise(gen, B, Cout, out_len) if f.get("res") else None
    x, w, b = x.float(), w.float(), b.float()
    scale, res = (scale.float() if scale is not None else None), (res.float() if res is not None else None)
    want = gn_reference(x.double(), G, w.double(), b.double(), glu, gelu, scale.double() if scale is not None else None,
                        res.double() if res is not None else None, off, out_len, cd)
    xg = x.double().reshape(B * G, -1)
    want_stats = torch.stack([xg.mean(1), 1.0 / torch.sqrt(xg.var(1, unbiased=False) + 1e-5)], 1)

    xd, wd, bd = x.cuda().contiguous(), w.cuda(), b.cuda()
    sd = scale.cuda() if scale is not None else None
    rd = padded(res, res_pitch) if res is not None else None
    y = torch.full((B, Cout, out_pitch), NAN, device="cuda")
    ws = torch.zeros(B * G * 64, dtype=torch.float64, device="cuda")
    st = torch.full((B * G, 2), NAN, device="cuda")
    _lib.check(lib.mi_group_norm_apply(xd.data_ptr(), B, Cin, G, in_len, in_len, off, wd.data_ptr(), bd.data_ptr(), glu, gelu, ptr(sd),
                                       ptr(rd), res_pitch if res is not None else 0, y.data_ptr(), Cout, out_len, out_pitch, cd,
                                       ws.data_ptr(), st.data_ptr(), stream()), "mi_group_norm_apply")
    torch.cuda.synchronize()
    y, st = y.cpu(), st.cpu().double()
    assert int(torch.count_nonzero(ws)) == 0, "the statistic slots were not left zero"
    rel = ((st - want_stats).abs() / want_stats.abs()).max(0).values
    err = float((y[..., :out_len].double() - want).abs().max())
    print(f"gn_apply {form} Cin {Cin} out_len {out_len}: y max-abs vs float64 {err:.2e}; mean rel {float(rel[0]):.2e}, rstd rel {float(rel[1]):.2e}")
    assert bool(torch.isnan(y[..., out_len:]).all()), "the output's pitch padding was written"
    assert bool(torch.isfinite(y[..., :out_len]).all())
    assert err <= GN_TOL
    assert float(rel.max()) <= GN_STAT_RTOL


# ---- BLSTM framing -------------------------------------------------------------------------------------------------------------
FRAME_T = [201, 250, 299, 300, 301, 349, 350, 351, 1004]       # both sides of a frame boundary and of the last frame's kept range; F = 3; production
W, S = 200, 100


@pytest.mark.parametrize("T", FRAME_T)
def test_blstm_unfold_is_the_reference_unfold(lib, T):
    B, Cn = 2, 3
    nf = math.ceil(T / S)
    x = noise(torch.Generator().manual_seed(T), B, Cn, T).float()
    want = HO.unfold(x, W, S).permute(0, 2, 1, 3).reshape(B * nf, Cn, W)      # zero past T
    fr = torch.full((B * nf, Cn, W), NAN, device="cuda")
    xd = x.cuda().contiguous()
    _lib.check(lib.mi_blstm_unfold(xd.data_ptr(), B, Cn, T, nf, W, S, fr.data_ptr(), stream()), "mi_blstm_unfold")
    torch.cuda.synchronize()
    assert torch.equal(fr.cpu(), want)


@pytest.mark.parametrize("with_skip", [True, False], ids=["skip", "noskip"])
@pytest.mark.parametrize("T", FRAME_T)
def test_blstm_restitch_is_the_reference_concatenation(lib, T, with_skip):
    """Frame values f * 1000 + column (+ a fraction naming item and channel): a wrong (frame, column) shows as a value.  One
    float32 add of the skip on either side: exact equality."""
    B, Cn = 2, 3
    nf = math.ceil(T / S)
    fr = (torch.arange(nf)[None, :, None, None] * 1000.0 + torch.arange(W)[None, None, None, :] + torch.arange(Cn)[None, None, :, None] * 0.25
          + torch.arange(B)[:, None, None, None] * 0.125).float()                                                    # (B, F, C, W)
    skip = noise(torch.Generator().manual_seed(T + 1), B, Cn, T).float() if with_skip else None
    want = HO.restitch(fr, S, T)
    if with_skip:
        want = want + skip
    frd = fr.reshape(B * nf, Cn, W).cuda().contiguous()
    sk = skip.cuda().contiguous() if with_skip else None
    y = torch.full((B, Cn, T), NAN, device="cuda")
    _lib.check(lib.mi_blstm_restitch(frd.data_ptr(), B, Cn, T, nf, W, S, ptr(sk), y.data_ptr(), stream()), "mi_blstm_restitch")
    torch.cuda.synchronize()
    y = y.cpu()
    bad = (y != want).nonzero()
    assert torch.equal(y, want), f"first mismatch at (b, c, t) = {bad[0].tolist()}: {float(y[tuple(bad[0])])} != {float(want[tuple(bad[0])])}"


# ---- waveform normalisation into pitched rows ----------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [1, 255, 257, 5000])
def test_row_affine_pitch_normalises_and_zeroes_the_padding(lib, L):
    """y = (x - mean) * inv as one float32 subtraction and one multiplication (exact equality), and every pitch column exactly
    0.0 afterwards: the DMA convolutions that follow read them."""
    B, Cn = 2, 2
    pitch = rup(L, 4) + 4
    gen = torch.Generator().manual_seed(L)
    x = (noise(gen, B, Cn, L) * 0.3 + 0.1).float()
    norm = torch.stack([noise(gen, B) * 0.1, 1.0 / (1e-5 + 0.3 + 0.1 * torch.rand(B, generator=gen, dtype=torch.float64))], 1).float()
    want = (x - norm[:, 0, None, None]) * norm[:, 1, None, None]
    xd, nd = x.cuda().contiguous(), norm.cuda().contiguous()
    y = torch.full((B, Cn, pitch), NAN, device="cuda")
    _lib.check(lib.mi_row_affine_pitch(xd.data_ptr(), B, Cn, L, pitch, nd.data_ptr(), y.data_ptr(), stream()), "mi_row_affine_pitch")
    torch.cuda.synchronize()
    y = y.cpu()
    assert torch.equal(y[..., :L], want)
    assert torch.equal(y[..., L:], torch.zeros(B, Cn, pitch - L)), "pitch padding is not exactly zero"


def test_entry_points_refuse_what_the_kernels_cannot_take(lib):
    """Argument checks of the wrappers: nothing is launched for a pitch below the length, a window outside the input, frames
    that do not cover T, or channel counts without a kernel."""
    one = torch.zeros(64, device="cuda")
    p = one.data_ptr()
    assert lib.mi_local_attn(p, 1, 16, 8, 8, p, 7, stream()) != 0                     # ld_o < T
    assert lib.mi_local_attn(p, 1, 16, 8, 10, p, 8, stream()) != 0                    # ld % 4 != 0
    assert lib.mi_local_attn(p, 1, 128, 8, 8, p, 8, stream()) != 0                    # head dimension 32: no kernel
    assert lib.mi_blstm_restitch(p, 1, 1, 401, 3, 200, 100, None, p, stream()) != 0   # three frames end at 400
    assert lib.mi_row_affine_pitch(p, 1, 1, 8, 7, p, p, stream()) != 0
    assert lib.mi_group_norm_apply(p, 1, 4, 1, 8, 8, 2, p, p, 0, 1, None, None, 0, p, 4, 7, 7, 1, p, p, stream()) != 0   # window past in_len
    assert b"window" in lib.mi_last_error()
