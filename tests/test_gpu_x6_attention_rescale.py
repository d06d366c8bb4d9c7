"""The thresholded online-softmax rescale of the split-bf16 attention core (attention_x6.hip, C entry `mi_attention_split`).

The kernel keeps one reference max per query and moves it only when a 32-key sub-tile's max passes it by more than TAU = 8; the
other queries of the wave multiply by exactly 1.  The cases put the running max where that logic can go wrong:

  * a max that climbs in most sub-tiles but stays within TAU of the reference, and one that jumps past it (spiked keys at a
    sub-tile's first key, last key, mid-tile, the very first key and inside a ragged last sub-tile);
  * a max that only descends; all-equal scores (Q = 0: the output is the mean of V);
  * bit-exact independence of a query from the 31 others of its wave, determinism and plane isolation.

Yardsticks: the float64 softmax and the native fp32 kernel (`mi_attention`) on the same inputs, as tests/test_gpu_x6_attention.py:
err < 2e-5 and err <= 2 x the native kernel's error.  A float32 online softmax in 32-key blocks on the CPU stays under 1e-5 on
every input of the four float64 cases (8.9e-7 .. 5.5e-6), so the bounds test the kernel and not the inputs.
"""
import pytest
import torch

from demucs_amd import _lib
from gpu_helpers import maxerr

pytestmark = pytest.mark.gpu
H = 8


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return _lib.load()


def rnd(*shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g, dtype=torch.float64) * scale


def run(lib, q, k, v, split=True):
    """q (B, 512, Tq), k / v (B, 512, Tk): contiguous device float32 -> o (B, 512, Tq)."""
    B, _, Tq = q.shape
    Tk = k.shape[2]
    o = torch.empty(B, 512, Tq, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    if split:
        _lib.check(lib.mi_attention_split(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), B, H, Tq, Tk, 512 * Tq, 512 * Tk,
                                          512 * Tq, st), "mi_attention_split")
    else:
        _lib.check(lib.mi_attention(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), B, H, Tq, Tk, 512 * Tq, 512 * Tk,
                                    512 * Tq, 0, st), "mi_attention")
    torch.cuda.synchronize()
    return o


def reference(q, k, v):
    """float64 softmax(Q K^T / 8) V of float32 (B, 512, T) tensors -> (B, 512, Tq) float64 on the CPU."""
    B, _, Tq = q.shape
    Tk = k.shape[2]
    Q = q.double().cpu().view(B, H, 64, Tq).transpose(2, 3)
    K = k.double().cpu().view(B, H, 64, Tk).transpose(2, 3)
    V = v.double().cpu().view(B, H, 64, Tk).transpose(2, 3)
    return (torch.softmax(Q @ K.transpose(-1, -2) / 8.0, dim=-1) @ V).transpose(2, 3).reshape(B, 512, Tq)


def drift(B, Tk, seed, lo, hi):
    """Keys = 0.5 N(0, 1) + a_j u with one direction u per head (|u| = 8, so q . u / 8 ~ N(0, 1) = z) and a_j linear from lo to hi:
    query's scores move by z (hi - lo) across the keys, smoothly, upwards for z (hi - lo) > 0."""
    u = rnd(B, H, 64, 1, seed=seed + 7)
    u = 8.0 * u / u.norm(dim=2, keepdim=True)
    a = torch.linspace(lo, hi, Tk, dtype=torch.float64)
    return (rnd(B, H, 64, Tk, seed=seed + 1, scale=0.5) + u * a).reshape(B, 512, Tk)


def inputs(case):
    """-> q, k, v as float64 CPU tensors (B, 512, T)."""
    if case == "climb_small":          # per query the max rises (or falls) by |z| 0.45 per sub-tile over 10 sub-tiles: within TAU for |z| < 1.8
        B, Tq, Tk = 2, 200, 320
        return rnd(B, 512, Tq, seed=11), drift(B, Tk, 11, 0.0, 4.5), rnd(B, 512, Tk, seed=13)
    if case == "climb_large":          # jumps past TAU: x 6 at the very first key, a sub-tile's last key and mid-tile, x 12 at a first key
        B, Tq, Tk = 2, 200, 320
        k = rnd(B, 512, Tk, seed=22)
        for key, f in ((0, 6.0), (95, 6.0), (170, 6.0), (256, 12.0)):
            k[:, :, key] *= f
        return rnd(B, 512, Tq, seed=21), k, rnd(B, 512, Tk, seed=23)
    if case == "climb_large_ragged":   # Tk = 100: the last sub-tile holds keys 96 .. 99; spikes at keys 0, 63 (a tile's last) and 97 (x 12)
        B, Tq, Tk = 2, 128, 100
        k = rnd(B, 512, Tk, seed=32)
        for key, f in ((0, 6.0), (63, 6.0), (97, 12.0)):
            k[:, :, key] *= f
        return rnd(B, 512, Tq, seed=31), k, rnd(B, 512, Tk, seed=33)
    if case == "descending":           # key norms fall from 4 to 0.5: the first sub-tile holds the max, nothing passes it afterwards
        B, Tq, Tk = 2, 200, 384
        c = torch.linspace(4.0, 0.5, Tk, dtype=torch.float64)
        return rnd(B, 512, Tq, seed=41), rnd(B, 512, Tk, seed=42) * c, rnd(B, 512, Tk, seed=43)
    raise KeyError(case)


CASES = ["climb_small", "climb_large", "climb_large_ragged", "descending"]


@pytest.mark.parametrize("case", CASES)
def test_rescale_matches_softmax(lib, case):
    q, k, v = (t.float().cuda() for t in inputs(case))
    want = reference(q, k, v)
    err = maxerr(run(lib, q, k, v), want)
    err_native = maxerr(run(lib, q, k, v, split=False), want)
    print(f"{case}: split {err:.3e}, native fp32 {err_native:.3e}")
    assert err < 2e-5
    assert err <= 2 * err_native


def test_uniform_scores_give_the_mean_of_v(lib):
    B, Tq, Tk = 2, 200, 100
    q = torch.zeros(B, 512, Tq, device="cuda")
    k, v = rnd(B, 512, Tk, seed=51).float().cuda(), rnd(B, 512, Tk, seed=52).float().cuda()
    want = v.double().cpu().mean(dim=2, keepdim=True).expand(B, 512, Tq)
    err = maxerr(run(lib, q, k, v), want)
    print(f"uniform: {err:.3e}")
    assert err < 1e-6


@pytest.mark.parametrize("first", [128, 288])      # a wave's 32 queries inside Tq = 300, and the ragged last block (288 .. 299)
def test_a_query_does_not_see_its_waves_other_queries(lib, first):
    """Queries first .. first + 7 give the same bits whether the block's other queries carry x 12 scores (their reference max
    jumps again and again) or none at all (Q = 0: it never moves)."""
    B, Tq, Tk = 1, 300, 320
    q, k, v = rnd(B, 512, Tq, seed=61), rnd(B, 512, Tk, seed=62), rnd(B, 512, Tk, seed=63)
    last = min(first + 32, Tq)
    loud, quiet = q.clone(), q.clone()
    loud[:, :, first + 8:last] *= 12.0
    quiet[:, :, first + 8:last] = 0.0
    k, v = k.float().cuda(), v.float().cuda()
    o_loud, o_quiet = run(lib, loud.float().cuda(), k, v), run(lib, quiet.float().cuda(), k, v)
    assert torch.equal(o_loud[:, :, first:first + 8], o_quiet[:, :, first:first + 8])
    assert not torch.equal(o_loud[:, :, first + 8:last], o_quiet[:, :, first + 8:last])
    # and the 8 queries are right, not only equal
    assert maxerr(o_loud[:, :, first:first + 8], reference(loud.float(), k, v)[:, :, first:first + 8]) < 2e-5


def test_rescale_is_deterministic_and_planes_are_isolated(lib):
    q, k, v = (t.float().cuda() for t in inputs("climb_large"))
    o = run(lib, q, k, v)
    assert torch.equal(o, run(lib, q, k, v))
    for b in range(q.shape[0]):                 # the item alone (B = 1): same bits
        assert torch.equal(run(lib, q[b:b + 1].contiguous(), k[b:b + 1].contiguous(), v[b:b + 1].contiguous())[0], o[b])
