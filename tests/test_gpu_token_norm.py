"""The transformer's token kernel (norms.hip token_tile_kernel) alone, through `mi_token_norm`: LayerNorm over channels with the
positional table (mode 0), the statistics-only pass (mode 1) and the GroupNorm(1) apply (mode 2), each with the per-token
(mean, rstd) output that the next GEMM's folded LayerNorm consumes and with the 16-bit operand images the half modes feed to
the next projection -- against float64, at the engine's width and at the smallest widths that take each code path (one
eight-channel trip per wave, a trip plus the scalar tail, the tail alone), at token counts around the 64-token tile.

Inputs: x = N(0, 1) * 3 + 40 (a large mean against a one-pass variance).  Item 0 has one token that is constant over the
channels (variance exactly 0); item 1 has one token whose FIRST channel lies 1e3 away from the others, so that the value the
kernel shifts its sums by is far from the mean.

Tolerance of the (mean, rstd) outputs.  `restated_stats` below is the kernel's formula in float32 on the CPU (serial sums of
v - v0 and (v - v0)^2 over the channels, var = s2 / C - (s1 / C)^2).  Its deviation from float64 on exactly these inputs,
maximum over every case of this file (C in {4, 32, 36, 512}, T in {1, 63, 64, 65, 333}, the three modes):

    ordinary tokens      mean 6.3e-06 absolute     rstd 1.3e-05 relative
    the outlier token    mean 3.9e-04 absolute     rstd 2.6e-04 relative

The kernel sums four wave partials instead of one serial chain, so it gets 4x that: OSTAT_BOUND below.  Every case prints the
restatement's and the kernel's deviation.  The constant token is compared exactly.  (These cases are what moved the kernel's own
sums to float64: in float32 the outlier token's LayerNorm output was 2e-3 from float64 at C = 512, against Y_TOL.)"""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from demucs_amd import _lib

pytestmark = pytest.mark.gpu
NAN = float("nan")
EPS = 1e-5
WIDTHS = [512, 32, 36, 4]
TOKENS = [1, 63, 64, 65, 333]
Y_TOL = 3e-5                                   # test_layernorm_channel_first's bound
#                 (mean absolute, rstd relative): 4 x the float32 restatement's measured deviation (module docstring)
OSTAT_BOUND = {"ordinary": (4 * 6.3e-06, 4 * 1.3e-05), "outlier": (4 * 3.9e-04, 4 * 2.6e-04)}
SENTINEL = 0x5A5A


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return _lib.load()


def stream():
    return C.c_void_p(_lib.current_stream_ptr())


def ptr(t):
    return t.data_ptr() if t is not None else None


def const_token(T):
    return 0, T // 2


def outlier_token(T):
    return 1, T - 1


_INPUTS = {}


def inputs(Cn, T):
    """float32 x (2, C, T), w, b (C), pe (C, T), gstat (2, 2); computed once per shape and shared."""
    if (Cn, T) not in _INPUTS:
        gen = torch.Generator().manual_seed(1000 * Cn + T)
        x = torch.randn(2, Cn, T, generator=gen, dtype=torch.float64) * 3.0 + 40.0
        b0, t0 = const_token(T)
        x[b0, :, t0] = x[b0, 0, t0]
        b1, t1 = outlier_token(T)
        x[b1, 0, t1] += 1e3
        w, b = torch.randn(Cn, generator=gen, dtype=torch.float64), torch.randn(Cn, generator=gen, dtype=torch.float64)
        pe = torch.randn(Cn, T, generator=gen, dtype=torch.float64)
        x = x.float()
        xi = x.double().reshape(2, -1)
        gstat = torch.stack([xi.mean(1), 1.0 / torch.sqrt(xi.var(1, unbiased=False) + EPS)], 1).float()
        _INPUTS[(Cn, T)] = (x, w.float(), b.float(), pe.float(), gstat)
    return _INPUTS[(Cn, T)]


def reference_y(mode, x, w, b, pe, gstat):
    """float64 y (B, C, T) of mode 0 (LayerNorm + pe) / mode 2 (GroupNorm(1) apply with the given per-item statistics)."""
    x, w, b = x.double(), w.double(), b.double()
    if mode == 0:
        y = F.layer_norm(x.transpose(1, 2), (x.shape[1],), w, b, eps=EPS).transpose(1, 2)
        return y + pe.double()[None] if pe is not None else y
    g = gstat.double()
    return (x - g[:, 0, None, None]) * g[:, 1, None, None] * w[None, :, None] + b[None, :, None]


def token_stats(v):
    """float64 (mean over channels, 1 / sqrt(biased variance + eps)) of v (B, C, T) -> (B, T, 2)."""
    return torch.stack([v.mean(1), 1.0 / torch.sqrt(v.var(1, unbiased=False) + EPS)], -1)


def restated_stats(v):
    """The kernel's formula in float32, one serial chain over the channels: v (B, C, T) float32 -> (B, T, 2) float32."""
    v = v.numpy()
    Cn = v.shape[1]
    v0 = v[:, 0]
    s1, s2 = np.zeros_like(v0), np.zeros_like(v0)
    for c in range(Cn):
        d = v[:, c] - v0
        s1 = s1 + d
        s2 = s2 + d * d
    inv_c = np.float32(1.0) / np.float32(Cn)
    dm = s1 * inv_c
    var = np.maximum(s2 * inv_c - dm * dm, np.float32(0.0))
    rstd = np.float32(1.0) / np.sqrt(var + np.float32(EPS))
    return torch.from_numpy(np.stack([v0 + dm, rstd], -1).astype(np.float32))


def stat_deviation(got, want, T):
    """{'ordinary' | 'outlier': (max |mean - mean64|, max |rstd / rstd64 - 1|)} of (B, T, 2) statistics."""
    d_mean = (got[..., 0].double() - want[..., 0]).abs()
    d_rstd = (got[..., 1].double() / want[..., 1] - 1.0).abs()
    mask = torch.zeros(got.shape[:2], dtype=torch.bool)
    mask[outlier_token(T)] = True
    out = {"outlier": (float(d_mean[mask].max()), float(d_rstd[mask].max()))}
    out["ordinary"] = (float(d_mean[~mask].max()), float(d_rstd[~mask].max()))
    return out


def check_ostat(tag, got, want64, restated, T):
    dev_k, dev_r = stat_deviation(got, want64, T), stat_deviation(restated, want64, T)
    for cls in ("ordinary", "outlier"):
        print(f"{tag} {cls} tokens: (mean abs, rstd rel) kernel ({dev_k[cls][0]:.2e}, {dev_k[cls][1]:.2e}), float32 restatement "
              f"({dev_r[cls][0]:.2e}, {dev_r[cls][1]:.2e}), bound ({OSTAT_BOUND[cls][0]:.2e}, {OSTAT_BOUND[cls][1]:.2e})")
    assert bool(torch.isfinite(got).all())
    for cls in ("ordinary", "outlier"):
        assert dev_k[cls][0] <= OSTAT_BOUND[cls][0] and dev_k[cls][1] <= OSTAT_BOUND[cls][1], (tag, cls, dev_k[cls])


def run(lib, mode, x, w=None, b=None, pe=None, gstat=None, want_y=True, want_ostat=True, img_dtype=0, expect_ok=True):
    """One launch: -> (y, ostat, img) on the CPU (None where not requested); outputs start as NaN / the sentinel."""
    B, Cn, T = x.shape
    dev = [t.cuda().contiguous() if t is not None else None for t in (x, w, b, pe, gstat)]
    y = torch.full((B, Cn, T), NAN, device="cuda") if want_y else None
    ostat = torch.full((B, T, 2), NAN, device="cuda") if want_ostat else None
    img_n = B * T + 3
    img = torch.full((max(Cn // 8, 1), img_n, 8), SENTINEL, dtype=torch.int16, device="cuda") if img_dtype else None
    rc = lib.mi_token_norm(mode, dev[0].data_ptr(), B, Cn, T, ptr(dev[1]), ptr(dev[2]), ptr(dev[3]), ptr(dev[4]), ptr(y), ptr(ostat), ptr(img),
                           img_n, img_dtype, stream())
    torch.cuda.synchronize()
    if not expect_ok:
        assert rc != 0
        return None
    _lib.check(rc, "mi_token_norm")
    return tuple(t.cpu() if t is not None else None for t in (y, ostat, img))


def check_image(img, src, dtype):
    """Columns [0, B T) are exactly the 16-bit rounding of the float32 tensor the same launch wrote, [C / 8][b T + t][8]; the
    columns past B T still hold the sentinel."""
    B, Cn, T = src.shape
    hdt = torch.bfloat16 if dtype == 1 else torch.float16
    want = src.permute(1, 0, 2).reshape(Cn // 8, 8, B * T).permute(0, 2, 1).to(hdt).contiguous().view(torch.int16)
    assert torch.equal(img[:, :B * T], want)
    assert bool((img[:, B * T:] == SENTINEL).all()), "image columns past B * T were written"


@pytest.mark.parametrize("T", TOKENS)
@pytest.mark.parametrize("Cn", WIDTHS)
def test_layernorm_mode(lib, Cn, T):
    x, w, b, pe, _ = inputs(Cn, T)
    base = None
    for with_pe in (True, False):
        p = pe if with_pe else None
        want = reference_y(0, x, w, b, p, None)
        y_plain, _, _ = run(lib, 0, x, w, b, p, want_ostat=False)
        y, ostat, _ = run(lib, 0, x, w, b, p)
        err = float((y.double() - want).abs().max())
        print(f"token_norm mode 0 C {Cn} T {T} pe {with_pe}: y max-abs vs float64 {err:.2e}")
        assert bool(torch.isfinite(y).all()) and err <= Y_TOL
        assert torch.equal(y, y_plain), "y depends on whether the statistics are requested"
        # the constant token: variance exactly 0, so y = b (+ pe) with no rounding but that one add
        b0, t0 = const_token(T)
        assert torch.equal(y[b0, :, t0], b + p[:, t0] if with_pe else b)
        check_ostat(f"token_norm mode 0 C {Cn} T {T} pe {with_pe}", ostat, token_stats(want), restated_stats(want.float()), T)
        if with_pe:
            base = y
            xd, wd, bd, pd = x.cuda(), w.cuda(), b.cuda(), pe.cuda()
            y_cf = torch.full((2, Cn, T), NAN, device="cuda")
            _lib.check(lib.mi_layernorm_cf(xd.data_ptr(), 2, Cn, T, wd.data_ptr(), bd.data_ptr(), pd.data_ptr(), y_cf.data_ptr(), stream()),
                       "mi_layernorm_cf")
            torch.cuda.synchronize()
            assert torch.equal(y_cf.cpu(), y)
    if Cn % 32 == 0:
        for dtype in (1, 2):
            y, ostat, img = run(lib, 0, x, w, b, pe, img_dtype=dtype)
            assert torch.equal(y, base), "y depends on whether an operand image is requested"
            check_image(img, y, dtype)
    else:
        run(lib, 0, x, w, b, pe, img_dtype=1, expect_ok=False)       # no eight-channel octets per wave: the image must be refused


@pytest.mark.parametrize("T", TOKENS)
@pytest.mark.parametrize("Cn", WIDTHS)
def test_statistics_mode(lib, Cn, T):
    x, _, _, _, _ = inputs(Cn, T)
    want = token_stats(x.double())
    _, ostat, _ = run(lib, 1, x, want_y=False)                    # y_dev = NULL is accepted
    check_ostat(f"token_norm mode 1 C {Cn} T {T}", ostat, want, restated_stats(x), T)
    b0, t0 = const_token(T)
    exact = torch.tensor([float(x[b0, 0, t0]), float(np.float32(1.0) / np.sqrt(np.float32(0.0) + np.float32(EPS)))])
    assert torch.equal(ostat[b0, t0], exact), (ostat[b0, t0], exact)
    if Cn % 32 == 0:
        for dtype in (1, 2):
            _, o2, img = run(lib, 1, x, want_y=False, img_dtype=dtype)
            assert torch.equal(o2, ostat), "the statistics depend on whether an operand image is requested"
            check_image(img, x, dtype)
    else:
        run(lib, 1, x, want_y=False, img_dtype=2, expect_ok=False)
    run(lib, 1, x, want_y=False, want_ostat=False, expect_ok=False)      # nothing to write


@pytest.mark.parametrize("T", TOKENS)
@pytest.mark.parametrize("Cn", WIDTHS)
def test_groupnorm_apply_mode(lib, Cn, T):
    """y = (x - gm[b]) * gr[b] * w[c] + b[c]: three float32 roundings on the product's magnitude m and one on the sum, so
    |y - y64| <= 2^-22 (m + |y|) elementwise (first order, 4 x 2^-24)."""
    x, w, b, _, gstat = inputs(Cn, T)
    want = reference_y(2, x, w, b, None, gstat)
    tol = 2.0 ** -22 * ((want - b.double()[None, :, None]).abs() + want.abs()) + 1e-30
    y_plain, _, _ = run(lib, 2, x, w, b, gstat=gstat, want_ostat=False)
    y, ostat, _ = run(lib, 2, x, w, b, gstat=gstat)
    d = (y.double() - want).abs()
    print(f"token_norm mode 2 C {Cn} T {T}: y max-abs vs float64 {float(d.max()):.2e}, largest share of its bound {float((d / tol).max()):.2f}")
    assert bool(torch.isfinite(y).all()) and bool((d <= tol).all())
    assert torch.equal(y, y_plain)
    check_ostat(f"token_norm mode 2 C {Cn} T {T}", ostat, token_stats(want), restated_stats(want.float()), T)
    if Cn % 32 == 0:
        for dtype in (1, 2):
            y2, _, img = run(lib, 2, x, w, b, gstat=gstat, img_dtype=dtype)
            assert torch.equal(y2, y)
            check_image(img, y2, dtype)
    else:
        run(lib, 2, x, w, b, gstat=gstat, img_dtype=1, expect_ok=False)
