"""mi_attention_split (attention_x6_kernel) alone at the float32 model's four attention shapes, 31 segments x 8 heads, random data:
one small case against the float64 softmax first, then HIP-event times over 20 launches per shape.  A/B of two builds:
DEMUCS_AMD_LIB=<other libdemucs_amd.so> python tools/micro/attn_x6_bench.py, one process per library, alternating."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from demucs_amd import _lib  # noqa: E402

lib = _lib.load()
H = 8


def call(q, k, v, o, B, Tq, Tk):
    _lib.check(lib.mi_attention_split(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), B, H, Tq, Tk, 512 * Tq, 512 * Tk, 512 * Tq,
                                      torch.cuda.current_stream().cuda_stream), "mi_attention_split")


g = torch.Generator().manual_seed(1)
B, Tq, Tk = 2, 200, 320
q, k, v = (torch.randn(B, 512, T, generator=g).cuda() for T in (Tq, Tk, Tk))
o = torch.empty(B, 512, Tq, device="cuda")
call(q, k, v, o, B, Tq, Tk)
torch.cuda.synchronize()
Q, K, V = (t.double().view(B, H, 64, -1).transpose(2, 3) for t in (q, k, v))
want = (torch.softmax(Q @ K.transpose(-1, -2) / 8, -1) @ V).transpose(2, 3).reshape(B, 512, Tq)
err = (o.double() - want).abs().max().item()
assert err < 2e-5, err
res = [f"err {err:.2e}"]
for B, Tq, Tk in ((31, 2688, 2688), (31, 1344, 1344), (31, 2688, 1344), (31, 1344, 2688)):
    q, k, v = (torch.randn(B, 512, T, generator=g).cuda() for T in (Tq, Tk, Tk))
    o = torch.empty(B, 512, Tq, device="cuda")
    for _ in range(5):
        call(q, k, v, o, B, Tq, Tk)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    n = 20
    e0.record()
    for _ in range(n):
        call(q, k, v, o, B, Tq, Tk)
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / n
    res.append(f"{Tq}x{Tk} {ms:.3f} ms ({4 * B * H * Tq * Tk * 64 / ms / 1e9:.0f} TF)")
print(os.path.basename(os.environ.get("DEMUCS_AMD_LIB", "default")), " | ".join(res), flush=True)
