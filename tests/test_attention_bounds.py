"""The bound constants and the bound formula of test_gpu_attention.py, on the CPU.

RESTATED must have exactly one entry per (family, operand type) that file runs, and each entry must still be the largest
float32-restatement distance over the family's cases.  The restatement's figures depend a little on the host's float32 matmul
(kernel-level parity), so an entry may differ from this host's figure by a factor of 2 either way before a stale table
is reported: a changed case list, family or seed moves it by more or drops a key.

The half-mode bound sum_k delta(p_k) |v_kd| / L_q + 4 * RESTATED is exercised against a torch emulation of what the kernels do:
float32 online softmax over 32-key blocks, P rounded to the operand type once per block in the block-local scale, the denominator
summed from the unrounded p.  The emulation must stay inside the bound, or the formula itself is wrong."""
import pytest
import torch

import test_gpu_attention as t


def test_restated_table_matches_the_cases():
    now = {}
    for fam, kind, typ, case in t.restated_cases():
        q, k, v = t.draw(fam, case)
        Q, K, V = t.consumed(q, k, v, kind, typ)
        d = (t.softmax_pv(Q.float(), K.float(), V.float()).double() - t.softmax_pv(Q, K, V)).abs().max().item()
        now[(fam, typ)] = max(now.get((fam, typ), 0.0), d)
    assert set(now) == set(t.RESTATED), sorted(set(now) ^ set(t.RESTATED))
    off = {k: (t.RESTATED[k], v) for k, v in now.items() if not 0.5 <= v / t.RESTATED[k] <= 2.0}
    assert not off, off


def blockwise(Q, K, V, typ):
    """float32 online softmax over 32-key blocks as the kernels run it; Q pre-scaled; operands already rounded."""
    Q, K, V = Q.float(), K.float(), V.float()
    m = torch.full(Q.shape[:-1] + (1,), float("-inf"))
    l, o = torch.zeros_like(m), torch.zeros(Q.shape[:-1] + (64,))
    for k0 in range(0, K.shape[-2], 32):
        s = Q @ K[..., k0:k0 + 32, :].transpose(-1, -2)
        mnew = torch.maximum(m, s.max(-1, keepdim=True).values)
        alpha, p = torch.exp(m - mnew), torch.exp(s - mnew)
        l = l * alpha + p.sum(-1, keepdim=True)
        o = o * alpha + p.to(t.HDT[typ]).float() @ V[..., k0:k0 + 32, :]
        m = mnew
    return o / l


@pytest.mark.parametrize("typ", ["bf16", "f16"])
@pytest.mark.parametrize("kind", ["f32in", "heads"])
def test_half_bound_holds_for_a_blockwise_emulation(kind, typ):
    worst = 0.0
    for case in ((2, 3, 33, 36), (2, 3, 129, 196), (1, 3, 300, 132)):
        for fam in t.FAMILIES:
            r = t.reference(fam, kind, typ, case)
            Q, K, V = t.consumed(*t.draw(fam, case), kind, typ)
            err, _, ratio = t.ratio_to_bound(r, blockwise(Q, K, V, typ).double())
            print(f"{kind} {typ} {fam} {case}: emulation {err:.2e}, {ratio:.2f} of the bound")
            worst = max(worst, ratio)
    assert worst <= 1.0, worst
