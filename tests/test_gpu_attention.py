"""The four attention kernels alone against float64, at every tile edge: `attention_kernel` (attention.hip, `mi_attention` dtype 0),
`attention_x6_kernel` (`mi_attention_split`), `attention_half_kernel<bf16 / f16>` (`mi_attention` dtype 1 / 2, `mi_attention_image`)
and `attention_heads_kernel<bf16 / f16>` (`mi_attention_heads`, and `mi_attention_heads_image`: the operand-image output that is the
only form the half-mode engine uses).

Operands are drawn in float64 and passed through float32.  The float32-input kernels get them packed as the projections write them:
self-attention (Tq == Tk) as ONE (B, 3 * heads * 64, T) buffer with batch strides 3x, cross-attention as q plus a (B, 2 * heads * 64,
Tk) buffer; every other case carries 12 floats of NaN between the items.  The heads kernel gets [B][heads][pitch][64] 16-bit tensors
with NaN in the rows past T, at pitches T, T + 8 and T rounded up to 64 in turn.  Float32 outputs start as NaN, images as 0x5A5A.

Reference: float64 softmax(Q K^T / 8) V of the operands exactly as the kernel consumes them: plain float32 values for the fp32 and
split kernels; for the half kernels the test rounds them itself -- attention_half rounds q * 0.125 (the scaling is exact), the heads
kernel q (the two differ only where q / 8 is subnormal in f16), both k and v.

Families (named functions, reused by test_attention_bounds.py): `gauss` q, k, v ~ N(0, 1); `spike_first` / `spike_last`: gauss with
one key times 6, in the first block / at key Tk - 1 (the last valid key of a ragged block); `ramp`: k_j = g (2 j / Tk - 1) + 0.3
noise for a fixed unit g, q_i = +/- 8 g + noise with the sign alternating with i, so inside every wave half the queries see the
running max move block after block while the other half keep their first (`__any(mnew != mrun)` with alpha == 1 on half the lanes);
`offset`: q + 6, k + 3, a common score of about 144 that overflows float32's exp without the max subtraction; `select`: q_i = 32
e_(i mod 5), k_j = -16 e_(j mod 5), exact in bf16 and f16, scores 0 or -64, so the output is the mean of v over the keys with j mod
5 != i mod 5 and nothing is left to round in P; 5 is coprime with the strides 4 / 8 / 16 / 32 of the accumulator row map (r & 3) +
8 (r >> 2) + 4 lh, so a mismatch between the P order and the V order changes values.

Bounds.  None is taken from a kernel.
  RESTATED[(family, type)]: the largest max-abs distance from float64 of torch's float32 evaluation softmax(Q K^T) V on the CPU (Q
      pre-scaled), over every case of the family in this file (test_attention_bounds.py keeps the table honest).
  float32 kernels (native and split):   |err| <= 4 * RESTATED  (the project's margin for another summation order)
  half kernels, elementwise:            |err[q, d]| <= sum_k delta(p_k) |v_kd| / L_q + 4 * RESTATED
      p_k = exp(s_k - max s), L = sum p, both float64; delta(p) = u p, u = 2^-8 (bf16) / 2^-11 (f16): half an ulp relative to the
      BOTTOM of p's binade (2^-9 / 2^-12 is the figure at the top); f16: delta(p) = max(u p, 2^-25) for its subnormal spacing.
      Why: the kernels round P once, in the block-local scale exp(s - m_local) with m_local the running max at that block; relative
      rounding is scale-free, and every later rescale factor exp(m_old - m_new) is <= 1, so in the final scale the error of p_k is at
      most u p_k (and an f16 subnormal's 2^-25 only shrinks); the denominator sums the UNROUNDED p, so it adds float32 noise only.
  `select`: no probability rounding is left, so the half kernels are held to 4 * RESTATED there.
Every case prints restated, kernel, bound and ratio.

Further: images equal the round-to-nearest-even of the float32 output of the same kernel on the same inputs bit for bit, with n_img =
B * Tq + 3 and the extra columns untouched; sentinels between the items of o survive o_batch_stride = heads * 64 * Tq + 20; outputs are
finite although every gap and padding row holds NaN; two launches agree bit for bit; a plane alone equals that plane inside a batch
bit for bit; NaN in one plane's K or V stays in that plane; every refusal is a host check that launches nothing."""
import ctypes as C
import functools
from types import SimpleNamespace

import pytest
import torch

from demucs_amd import _lib

pytestmark = pytest.mark.gpu
HDT = {"bf16": torch.bfloat16, "f16": torch.float16}
DT = {"f32": 0, "bf16": 1, "f16": 2}
U = {"bf16": 2.0 ** -8, "f16": 2.0 ** -11}
SENT16, SENTF, SLACK = 0x5A5A, -12345.0, 12
# (entry, operand type): the six instantiations
KERNELS = [("fp32", "f32"), ("split", "f32"), ("half", "bf16"), ("half", "f16"), ("heads", "bf16"), ("heads", "f16")]
FAMILIES = ["gauss", "spike_first", "spike_last", "ramp", "offset", "select"]

TQ_EDGES = [1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 300]
TK_EDGES = [4, 28, 32, 36, 60, 64, 68, 100, 124, 128, 132, 192, 196, 256, 260, 320, 324]
TK_ODD = [1, 3, 31, 33, 63, 65, 97, 127, 129, 191, 193, 257]                     # the heads kernel takes any Tk: nt = 1 .. 5, ring wrapped
BH = [(1, 1), (1, 3), (1, 8), (3, 3), (2, 8), (1, 9), (17, 1)]                   # planes 1, 3, 8, 9, 16, 9, 17
# (B, heads, Tq, Tk)
TQ_CASES = [(2, 3, Tq, Tk) for Tk in (68, 196) for Tq in TQ_EDGES]
TK_CASES = [(2, 3, Tq, Tk) for Tq in (33, 129) for Tk in TK_EDGES]
TK_ODD_CASES = [(2, 3, Tq, Tk) for Tq in (33, 129) for Tk in TK_ODD]
BH_CASES = [(B, H, 300, 132) for B, H in BH]
SELF_CASES = [(2, 3, 36, 36), (2, 3, 132, 132)]                                  # one packed QKV buffer
CASES = TQ_CASES + TK_CASES + BH_CASES + SELF_CASES
IMAGE_CASES = set(TQ_CASES + BH_CASES + SELF_CASES)

# largest max-abs distance of the float32 restatement from float64 over the family's cases, {(family, type): distance}
RESTATED = {
    ('gauss', 'bf16'): 8.38e-07, ('gauss', 'f16'): 1.99e-06, ('gauss', 'f32'): 1.63e-06,
    ('offset', 'bf16'): 1.58e-05, ('offset', 'f16'): 1.15e-04, ('offset', 'f32'): 1.11e-04,
    ('ramp', 'bf16'): 4.86e-07, ('ramp', 'f16'): 8.05e-07, ('ramp', 'f32'): 4.36e-07,
    ('select', 'bf16'): 1.79e-07, ('select', 'f16'): 1.92e-07, ('select', 'f32'): 1.80e-07,
    ('spike_first', 'bf16'): 4.40e-06, ('spike_first', 'f16'): 4.30e-06, ('spike_first', 'f32'): 4.43e-06,
    ('spike_last', 'bf16'): 1.24e-06, ('spike_last', 'f16'): 2.90e-06, ('spike_last', 'f32'): 2.88e-06,
}


def cases_of(entry):
    return CASES + TK_ODD_CASES if entry == "heads" else CASES


def kind_of(entry):
    return "heads" if entry == "heads" else "f32in"


def restated_cases():
    """Every (family, operand kind, type, case) this file runs: what RESTATED is a maximum over."""
    seen = set()
    for entry, typ in KERNELS:
        for case in cases_of(entry):
            for fam in FAMILIES:
                seen.add((fam, kind_of(entry), typ, case))
    return sorted(seen)


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return _lib.load()


def stream():
    return C.c_void_p(_lib.current_stream_ptr())


def same_bits(a, b):
    a, b = a.contiguous(), b.contiguous()
    v = torch.int32 if a.dtype == torch.float32 else torch.int16
    return a.shape == b.shape and torch.equal(a.view(v), b.view(v))


# ---- input families: float32 q (B, H, Tq, 64), k, v (B, H, Tk, 64) -------------------------------------------------------------

def _gen(B, H, Tq, Tk, salt):
    g = torch.Generator().manual_seed(7919 * B + 104729 * H + 1299709 * Tq + 15485863 * Tk + salt)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    return rn(B, H, Tq, 64), rn(B, H, Tk, 64), rn(B, H, Tk, 64)


def gauss(B, H, Tq, Tk):
    return _gen(B, H, Tq, Tk, 1)


def spike_first(B, H, Tq, Tk):
    q, k, v = _gen(B, H, Tq, Tk, 2)
    k[:, :, min(5, Tk - 1)] *= 6.0
    return q, k, v


def spike_last(B, H, Tq, Tk):
    q, k, v = _gen(B, H, Tq, Tk, 3)
    k[:, :, Tk - 1] *= 6.0
    return q, k, v


def ramp(B, H, Tq, Tk):
    q, k, v = _gen(B, H, Tq, Tk, 4)
    g = torch.randn(64, generator=torch.Generator().manual_seed(5), dtype=torch.float64)
    g /= g.norm()
    j = torch.arange(Tk, dtype=torch.float64)
    sign = 1.0 - 2.0 * (torch.arange(Tq) % 2).double()
    return sign[:, None] * 8.0 * g + q, g * (2.0 * j / Tk - 1.0)[:, None] + 0.3 * k, v


def offset(B, H, Tq, Tk):
    q, k, v = _gen(B, H, Tq, Tk, 6)
    return q + 6.0, k + 3.0, v


def select(B, H, Tq, Tk):
    _, _, v = _gen(B, H, Tq, Tk, 7)
    eye = torch.eye(5, 64, dtype=torch.float64)
    q = (32.0 * eye[torch.arange(Tq) % 5]).expand(B, H, Tq, 64)
    k = (-16.0 * eye[torch.arange(Tk) % 5]).expand(B, H, Tk, 64)
    return q.clone(), k.clone(), v


FAMILY_FN = {"gauss": gauss, "spike_first": spike_first, "spike_last": spike_last, "ramp": ramp, "offset": offset, "select": select}


@functools.lru_cache(maxsize=8)
def draw(fam, case):
    return tuple(t.float() for t in FAMILY_FN[fam](*case))


def consumed(q, k, v, kind, typ):
    """float64 (Q / 8, K, V) exactly as the kernel consumes the float32 tensors q, k, v."""
    if typ == "f32":
        return (q * 0.125).double(), k.double(), v.double()
    h = HDT[typ]
    qs = (q * 0.125).to(h).double() if kind == "f32in" else q.to(h).double() * 0.125
    return qs, k.to(h).double(), v.to(h).double()


def softmax_pv(Q, K, V):
    return torch.softmax(Q @ K.transpose(-1, -2), dim=-1) @ V


def half_allow(Q, K, V, typ):
    """sum_k delta(p_k) |v_kd| / L_q: what rounding P to `typ` once, in any block-local scale, may cost (module docstring)."""
    s = Q @ K.transpose(-1, -2)
    p = torch.exp(s - s.max(-1, keepdim=True).values)
    delta = U[typ] * p
    if typ == "f16":
        delta = delta.clamp_min(2.0 ** -25)
    return (delta @ V.abs()) / p.sum(-1, keepdim=True)


@functools.lru_cache(maxsize=24)
def reference(fam, kind, typ, case):
    q, k, v = draw(fam, case)
    Q, K, V = consumed(q, k, v, kind, typ)
    r = SimpleNamespace(fam=fam, typ=typ, case=case, want=softmax_pv(Q, K, V))
    r.restated = (softmax_pv(Q.float(), K.float(), V.float()).double() - r.want).abs().max().item()
    r.allow = half_allow(Q, K, V, typ) if typ != "f32" and fam != "select" else None
    return r


def ratio_to_bound(r, got):
    """(largest |err|, the float32 part of the bound, largest err / bound); got: (B, H, Tq, 64) float64."""
    b32 = 4 * RESTATED[(r.fam, r.typ)]
    err = (got - r.want).abs()
    bound = b32 if r.allow is None else r.allow + b32
    return err.max().item(), b32, (err / bound).max().item()


# ---- device layouts and launches -----------------------------------------------------------------------------------------------

def pack_f32in(q, k, v, slack):
    """Channel-first float32 buffers as the projections write them; `slack` floats of NaN behind every item."""
    B, H, Tq, _ = q.shape
    Tk, HD = k.shape[2], H * 64
    cf = lambda t: t.transpose(2, 3).reshape(B, HD, -1).reshape(B, -1)
    gap = torch.full((B, slack), float("nan"))
    d = SimpleNamespace()
    if Tq == Tk:
        d.buf = torch.cat([cf(q), cf(k), cf(v), gap], 1).contiguous().cuda()
        d.q, d.k, d.v = d.buf.data_ptr(), d.buf.data_ptr() + 4 * HD * Tq, d.buf.data_ptr() + 8 * HD * Tq
        d.q_bs = d.kv_bs = 3 * HD * Tq + slack
    else:
        d.qbuf = torch.cat([cf(q), gap], 1).contiguous().cuda()
        d.kvbuf = torch.cat([cf(k), cf(v), gap], 1).contiguous().cuda()
        d.q, d.k, d.v = d.qbuf.data_ptr(), d.kvbuf.data_ptr(), d.kvbuf.data_ptr() + 4 * HD * Tk
        d.q_bs, d.kv_bs = HD * Tq + slack, 2 * HD * Tk + slack
    return d


def pitch_of(T, sel):
    return (T, T + 8, (T + 63) // 64 * 64)[sel % 3]


def pack_heads(q, k, v, typ, sel):
    """[B][heads][pitch][64] in the operand type, NaN in the rows past T."""
    def padded(t, P):
        out = torch.full((t.shape[0], t.shape[1], P, 64), float("nan"), dtype=HDT[typ])
        out[:, :, :t.shape[2]] = t.to(HDT[typ])
        return out.contiguous().cuda()
    d = SimpleNamespace(Tqp=pitch_of(q.shape[2], sel), Tkp=pitch_of(k.shape[2], sel + 1))
    d.qt, d.kt, d.vt = padded(q, d.Tqp), padded(k, d.Tkp), padded(v, d.Tkp)
    d.q, d.k, d.v = d.qt.data_ptr(), d.kt.data_ptr(), d.vt.data_ptr()
    return d


def pack(entry, typ, q, k, v, variant):
    return pack_heads(q, k, v, typ, variant) if entry == "heads" else pack_f32in(q, k, v, SLACK * (variant % 2))


def call(lib, entry, typ, d, out_ptr, B, H, Tq, Tk, o_bs=None, n_img=None, **over):
    """One entry call; returns the status.  `over` replaces arguments (the refusal tests)."""
    a = dict(q=d.q, k=d.k, v=d.v, out=out_ptr, B=B, H=H, Tq=Tq, Tk=Tk, dtype=DT[typ], n_img=n_img, o_bs=o_bs,
             q_bs=getattr(d, "q_bs", 0), kv_bs=getattr(d, "kv_bs", 0), Tqp=getattr(d, "Tqp", 0), Tkp=getattr(d, "Tkp", 0))
    a.update(over)
    st = stream()
    if entry == "heads":
        if n_img is None:
            return lib.mi_attention_heads(a["q"], a["k"], a["v"], a["out"], a["B"], a["H"], a["Tq"], a["Tk"], a["Tqp"], a["Tkp"], a["dtype"], st)
        return lib.mi_attention_heads_image(a["q"], a["k"], a["v"], a["out"], a["n_img"], a["B"], a["H"], a["Tq"], a["Tk"], a["Tqp"], a["Tkp"],
                                            a["dtype"], st)
    if n_img is not None:
        return lib.mi_attention_image(a["q"], a["k"], a["v"], a["out"], a["n_img"], a["B"], a["H"], a["Tq"], a["Tk"], a["q_bs"], a["kv_bs"],
                                      a["dtype"], st)
    if entry == "split":
        return lib.mi_attention_split(a["q"], a["k"], a["v"], a["out"], a["B"], a["H"], a["Tq"], a["Tk"], a["q_bs"], a["kv_bs"], a["o_bs"], st)
    return lib.mi_attention(a["q"], a["k"], a["v"], a["out"], a["B"], a["H"], a["Tq"], a["Tk"], a["q_bs"], a["kv_bs"], a["o_bs"], a["dtype"], st)


def run(lib, entry, typ, q, k, v, variant=0, o_gap=0):
    """float32 output (B, heads * 64 * Tq + o_gap) on the CPU: NaN where the kernel must write, SENTF in the gaps."""
    B, H, Tq, _ = q.shape
    n = H * 64 * Tq
    d = pack(entry, typ, q, k, v, variant)
    out = torch.full((B, n + o_gap), float("nan"), device="cuda")
    out[:, n:] = SENTF
    _lib.check(call(lib, entry, typ, d, out.data_ptr(), B, H, Tq, k.shape[2], o_bs=n + o_gap), entry)
    torch.cuda.synchronize()
    return out.cpu()


def run_image(lib, entry, typ, q, k, v, variant=0):
    B, H, Tq, _ = q.shape
    d = pack(entry, typ, q, k, v, variant)
    img = torch.full((H * 8, B * Tq + 3, 8), SENT16, dtype=torch.int16, device="cuda")
    _lib.check(call(lib, entry, typ, d, img.data_ptr(), B, H, Tq, k.shape[2], n_img=B * Tq + 3), entry + " image")
    torch.cuda.synchronize()
    return img.cpu()


def logical(out, B, H, Tq):
    """(B, heads * 64 * Tq [+ gap]) channel-first -> (B, H, Tq, 64)."""
    return out[:, :H * 64 * Tq].reshape(B, H, 64, Tq).transpose(2, 3)


def image_of(out, B, H, Tq, typ):
    """The operand image [heads * 64 / 8][B * Tq][8] of a float32 output, rounded to nearest even."""
    y = out[:, :H * 64 * Tq].reshape(B, H * 64, Tq)
    return y.permute(1, 0, 2).reshape(H * 8, 8, B * Tq).permute(0, 2, 1).to(HDT[typ]).contiguous().view(torch.int16)


# ---- every kernel through the same case tables ------------------------------------------------------------------------------------

PAIRS = [(case, ki) for case in sorted(set(CASES + TK_ODD_CASES)) for ki, (entry, _) in enumerate(KERNELS) if case in cases_of(entry)]


@pytest.mark.parametrize("case,ki", PAIRS, ids=["B%d-H%d-Tq%d-Tk%d-" % c + "-".join(KERNELS[ki]) for c, ki in PAIRS])
def test_against_float64(lib, case, ki):
    entry, typ = KERNELS[ki]
    B, H, Tq, Tk = case
    bad = []
    for fi, fam in enumerate(FAMILIES):
        q, k, v = draw(fam, case)
        r = reference(fam, kind_of(entry), typ, case)
        variant = fi + Tq + Tk // 4                      # every case sees every pitch / both gap forms across its families
        out = run(lib, entry, typ, q, k, v, variant)
        what = f"{entry} {typ} {fam} B {B} H {H} Tq {Tq} Tk {Tk}"
        if not bool(torch.isfinite(out).all()):
            bad.append(f"{what}: non-finite or unwritten output")
            continue
        err, b32, ratio = ratio_to_bound(r, logical(out, B, H, Tq).double())
        print(f"{what}: restated {r.restated:.2e}  kernel {err:.2e}  bound(f32 part) {b32:.2e}  ratio {ratio:.2f}")
        if not ratio <= 1.0:
            bad.append(f"{what}: err {err:.3e}, {ratio:.2f} of the bound")
        if fam in ("gauss", "ramp") and not same_bits(out, run(lib, entry, typ, q, k, v, variant)):
            bad.append(f"{what}: two launches differ")
        if typ != "f32" and case in IMAGE_CASES:
            img = run_image(lib, entry, typ, q, k, v, variant)
            if not bool((img[:, B * Tq:] == SENT16).all()):
                bad.append(f"{what}: image columns past B * Tq written")
            if not torch.equal(img[:, :B * Tq], image_of(out, B, H, Tq, typ)):
                bad.append(f"{what}: image != rounding of the float32 output")
    assert not bad, "\n".join(bad)


F32IN = [ki for ki, (entry, _) in enumerate(KERNELS) if entry != "heads"]


@pytest.mark.parametrize("ki", F32IN, ids=["-".join(KERNELS[ki]) for ki in F32IN])
@pytest.mark.parametrize("case", [(3, 3, 300, 132), (2, 3, 33, 68), (2, 3, 132, 132)], ids=lambda c: "B%d-H%d-Tq%d-Tk%d" % c)
def test_output_stride_keeps_sentinels(lib, case, ki):
    """o_batch_stride = heads * 64 * Tq + 20: the 20 floats behind every item survive, the values are those of the packed launch."""
    entry, typ = KERNELS[ki]
    q, k, v = draw("gauss", case)
    plain, gapped = run(lib, entry, typ, q, k, v), run(lib, entry, typ, q, k, v, o_gap=20)
    n = case[1] * 64 * case[2]
    assert bool((gapped[:, n:] == SENTF).all()), "the gap between two items of o was written"
    assert bool(torch.isfinite(gapped[:, :n]).all()) and same_bits(plain, gapped[:, :n])


@pytest.mark.parametrize("ki", range(len(KERNELS)), ids=["-".join(k) for k in KERNELS])
@pytest.mark.parametrize("case", [(3, 3, 300, 132), (17, 1, 300, 132)], ids=lambda c: "B%d-H%d-Tq%d-Tk%d" % c)
def test_plane_alone_equals_plane_in_batch(lib, case, ki):
    """The (item, head) -> workgroup map: a plane run as B = 1, heads = 1 gives the bits it has inside the batch."""
    entry, typ = KERNELS[ki]
    B, H, Tq, Tk = case
    for fam in ("gauss", "ramp"):
        q, k, v = draw(fam, case)
        full = logical(run(lib, entry, typ, q, k, v), B, H, Tq)
        for pl in (0, 4, B * H - 1):
            b, h = pl // H, pl % H
            solo = logical(run(lib, entry, typ, q[b:b + 1, h:h + 1], k[b:b + 1, h:h + 1], v[b:b + 1, h:h + 1], variant=1), 1, 1, Tq)
            assert same_bits(solo[0, 0], full[b, h]), f"{entry} {typ} {fam}: plane {pl} alone differs from the batch"


@pytest.mark.parametrize("ki", range(len(KERNELS)), ids=["-".join(k) for k in KERNELS])
def test_nan_stays_in_its_plane(lib, ki):
    """NaN in one plane's K, then in its V: that plane's output is non-finite, every other plane keeps its bits."""
    entry, typ = KERNELS[ki]
    case = (3, 3, 300, 132)
    B, H, Tq, Tk = case
    q, k, v = draw("gauss", case)
    clean = logical(run(lib, entry, typ, q, k, v), B, H, Tq).clone()
    for which in ("k", "v"):
        k2, v2 = k.clone(), v.clone()
        (k2 if which == "k" else v2)[1, 1] = float("nan")
        dirty = logical(run(lib, entry, typ, q, k2, v2), B, H, Tq).clone()
        assert not bool(torch.isfinite(dirty[1, 1]).any()), f"NaN {which}: finite values in the poisoned plane"
        dirty[1, 1] = clean[1, 1]
        assert same_bits(dirty, clean), f"NaN in one plane's {which} changed another plane"


# ---- refusals ------------------------------------------------------------------------------------------------------------------------

def test_refusals_launch_nothing(lib):
    """Every refusal is MI_EINVAL with a message, from a host check: no launch, no output byte written."""
    case = (2, 3, 33, 68)
    B, H, Tq, Tk = case
    q, k, v = draw("gauss", case)
    launches = [0]
    hook = C.CFUNCTYPE(None, C.c_void_p)(lambda st: launches.__setitem__(0, launches[0] + 1))
    packs = {(e, t): pack(e, t, q, k, v, 1) for e, t in KERNELS}
    q3, k3, v3 = draw("gauss", (2, 3, 33, 66))
    pack66 = pack_f32in(q3, k3, v3, 0)                                    # Tk % 4 != 0 with real buffers of that size
    n = H * 64 * Tq

    def refused(entry, typ, why, image=False, d=None, **over):
        d = d or packs[(entry, typ)]
        if image:
            out = torch.full((H * 8, B * Tq + 3, 8), SENT16, dtype=torch.int16, device="cuda")
            kw = dict(n_img=B * Tq + 3)
        else:
            out = torch.full((B, n), SENTF, device="cuda")
            kw = dict(o_bs=n)
        if over.pop("null_out", False):
            over["out"] = None
        elif "out_off" in over:
            over["out"] = out.data_ptr() + over.pop("out_off")
        kw.update(over)
        torch.cuda.synchronize()
        launches[0] = 0
        lib.mi_debug_set_post_launch_hook(hook)
        try:
            dims = [kw.pop(name, val) for name, val in (("B", B), ("H", H), ("Tq", Tq), ("Tk", Tk))]
            rc = call(lib, entry, typ, d, out.data_ptr(), *dims, **kw)
        finally:
            lib.mi_debug_set_post_launch_hook(None)
        torch.cuda.synchronize()
        msg = lib.mi_last_error().decode()
        assert rc == -1 and msg, (entry, typ, why, rc, msg)                # MI_EINVAL
        assert launches[0] == 0, f"{entry} {typ} {why}: {launches[0]} launches"
        assert bool((out == (SENT16 if image else SENTF)).all()), f"{entry} {typ} {why}: output written"

    for entry, typ, image in (("fp32", "f32", False), ("split", "f32", False), ("half", "bf16", False), ("half", "f16", True)):
        d = packs[(entry, typ)]
        refused(entry, typ, "Tk % 4", image, d=pack66, Tk=66)
        refused(entry, typ, "k alignment", image, k=d.k + 4)
        refused(entry, typ, "v alignment", image, v=d.v + 8)
        refused(entry, typ, "kv_batch_stride % 4", image, kv_bs=d.kv_bs + 2)
    DT["bad"] = 3
    try:
        refused("fp32", "bad", "dtype 3", d=packs[("fp32", "f32")])
    finally:
        del DT["bad"]
    refused("half", "f32", "dtype 0", image=True, d=packs[("half", "bf16")])
    for image in (False, True):
        d = packs[("heads", "bf16")]
        refused("heads", "f32", "dtype 0", image, d=d)
        refused("heads", "bf16", "Tq pitch", image, Tqp=Tq - 1)
        refused("heads", "bf16", "Tk pitch", image, Tkp=Tk - 1)
        for name in ("q", "k", "v"):
            refused("heads", "f16", name + " alignment", image, d=packs[("heads", "f16")], **{name: getattr(packs[("heads", "f16")], name) + 8})
    for entry, typ in (("half", "bf16"), ("heads", "f16")):
        refused(entry, typ, "n_img", image=True, n_img=B * Tq - 1)
        refused(entry, typ, "image alignment", image=True, out_off=8)
    for entry, typ, image in (("fp32", "f32", False), ("split", "f32", False), ("half", "bf16", False), ("half", "f16", True),
                              ("heads", "bf16", False), ("heads", "f16", True)):
        for name in ("q", "k", "v"):
            refused(entry, typ, "null " + name, image, **{name: None})
        refused(entry, typ, "null output", image, null_out=True)
        for name in ("B", "H", "Tq", "Tk"):
            refused(entry, typ, "zero " + name, image, **{name: 0})
