"""`mi_conv_forward` and the read slack of the shifted-run tap loaders (routes 2 and 7: up to 8 bytes before and 20 bytes after the
tensor at `x`).  A tensor that begins or ends with its device allocation has no such slack, and what lies beyond an allocation
need not be mapped.  The entry then runs the same kernel on a copy of `x` that has the slack (`mi_debug_conv_staged` counts
these calls): same route, same tile, same bits as with `x` inside a buffer that carries the slack itself, where nothing is copied.

One 3 x 3 GLU conv (64 -> 128 channels on (8, 48), B = 1) with and without a split weight image.  Where `x` lies in its
allocation is read from the allocator's own segment list, not assumed."""
import ctypes as C

import pytest
import torch

from demucs_amd import _lib
from gpu_helpers import EPI_GLU, conv_desc, ktab, pack_w

pytestmark = pytest.mark.gpu

DMATAP, TAP_X6 = 2, 7                                        # enum mi_conv_route (include/demucs_amd.h)
CC, FR, T = 64, 8, 48
N = CC * FR * T
BIG = 32 << 20                                               # bytes: past the allocator's 10 MiB line, a segment of its own


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return _lib.load()


@pytest.fixture(scope="module")
def values():
    return torch.randn(N, generator=torch.Generator().manual_seed(7))


def _segment(ptr):
    for s in torch.cuda.memory_snapshot():
        if s["address"] <= ptr < s["address"] + s["total_size"]:
            return s["address"], s["address"] + s["total_size"]
    raise AssertionError("tensor outside every segment of the allocator")


def _run(lib, x6, x):
    wt, bias, M, Mpad, K, Kpad, tile = pack_w(torch.randn(2 * CC, 9 * CC, generator=torch.Generator().manual_seed(3)) * (9 * CC) ** -0.5,
                                              torch.zeros(2 * CC), glu=True)
    P = FR * T
    y = torch.full((1, CC, FR, T), float("nan"), device="cuda")
    d, keep = conv_desc(x6=x6, wt=wt, M=M, Mpad=Mpad, K=K, Kpad=Kpad, ktab=ktab(CC, 3, 3, 1, 1, 1, 1, P, T, Kpad), x=x, x_bstride=CC * P,
                        B=1, D1=FR, D2=T, O1=FR, O2=T, S1=1, S2=1, row_mode=1, epi=EPI_GLU, bias=bias, y=y, y_bstride=CC * P, y_cstride=P,
                        tile_m=tile, ntaps=9, tap_k2=3, tap_pad1=1, tap_pad2=1)
    before = lib.mi_debug_conv_staged()
    _lib.check(lib.mi_conv_forward(C.byref(d), C.c_void_p(_lib.current_stream_ptr())), "mi_conv_forward")
    torch.cuda.synchronize()
    return y.cpu(), lib.mi_debug_last_conv_route(), lib.mi_debug_conv_staged() - before


@pytest.mark.parametrize("x6", [True, False], ids=["split", "native"])
def test_tensor_at_an_end_of_its_allocation_runs_on_a_copy(lib, values, x6):
    buf = torch.full((N + 64,), float("nan"), device="cuda")             # 32 floats of slack on both sides, as the engines' buffers carry
    buf[32:32 + N] = values.cuda()
    want, route, staged = _run(lib, x6, buf[32:32 + N])
    assert route == (TAP_X6 if x6 else DMATAP)
    assert staged == 0, "a tensor with slack of its own is read in place"
    assert bool(torch.isfinite(want).all())

    torch.cuda.empty_cache()
    big = torch.empty(BIG // 4, device="cuda")
    lo, hi = _segment(big.data_ptr())
    assert (lo, hi) == (big.data_ptr(), big.data_ptr() + BIG), "the large tensor was expected to fill a segment of its own"
    for x in (big[:N], big[-N:]):                                           # begins / ends with the allocation
        x.copy_(values)
        got, route_x, staged = _run(lib, x6, x)
        print(f"x at {x.data_ptr() - lo} of {hi - lo} bytes: route {route_x}, staged {staged}")
        assert route_x == route
        assert staged == 1
        assert torch.equal(got, want)
