"""The float32 attention core on the split-bf16 matrix pipe (attention_x6.hip, C entry `mi_attention_split`: Q / 8, K, V and the
probabilities as three exact bf16 terms, six bf16 MFMA products, fp32 accumulate), which the float32 htdemucs engine takes by
default.

  * against the float64 softmax: the cases of the native kernel's test, the model's self- and cross-attention shapes, ragged
    Tq and Tk; no worse than twice the native fp32 kernel's error on the same inputs;
  * bit-exact determinism and plane isolation: a plane inside a batch of 31 equals the plane alone, and NaN in one plane's K or
    V leaves every other plane's output unchanged;
  * the engine's route: split by default, native with MI_X6=0 or mi_set_split_bf16(0), bit-identical between those two.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from demucs_amd import _lib
from gpu_helpers import maxerr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H = 8
TF, TT = 2688, 1344           # htdemucs tokens per segment: frequency branch (8 x 336), time branch


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return _lib.load()


def stream():
    return torch.cuda.current_stream().cuda_stream


def rnd(*shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g, dtype=torch.float64) * scale


def run(lib, q, k, v, B, Tq, Tk, q_bs, kv_bs, split=True):
    """q / k / v: device float32 views with token-contiguous rows, batch strides in elements; returns o (B, 512, Tq)."""
    o = torch.empty(B, 512, Tq, device="cuda")
    if split:
        _lib.check(lib.mi_attention_split(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), B, H, Tq, Tk, q_bs, kv_bs, 512 * Tq,
                                          stream()), "mi_attention_split")
    else:
        _lib.check(lib.mi_attention(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), B, H, Tq, Tk, q_bs, kv_bs, 512 * Tq, 0,
                                    stream()), "mi_attention")
    torch.cuda.synchronize()
    return o


def reference(q, k, v, Tq, Tk):
    """float64 softmax(QK^T/8)V of (B, 512, T) float32 tensors, on the GPU one item at a time -> (B, 512, Tq) on the CPU."""
    out = []
    for b in range(q.shape[0]):
        Q = q[b].double().view(H, 64, Tq).transpose(1, 2)
        K = k[b].double().view(H, 64, Tk).transpose(1, 2)
        V = v[b].double().view(H, 64, Tk).transpose(1, 2)
        out.append((torch.softmax(Q @ K.transpose(-1, -2) / 8.0, dim=-1) @ V).transpose(1, 2).reshape(512, Tq).cpu())
    return torch.stack(out)


def packed(B, Tq, Tk, seed, cross, spike=None):
    """Q / K / V as the projections write them: self-attention one (B, 1536, T) tensor, cross-attention q (B, 512, Tq) and
    kv (B, 1024, Tk).  Returns device views q, k, v and the batch strides."""
    q, k, v = rnd(B, 512, Tq, seed=seed), rnd(B, 512, Tk, seed=seed + 1), rnd(B, 512, Tk, seed=seed + 2)
    if spike is not None:
        k[:, :, spike] *= 6.0                   # a spiked key: scores up to |s| ~ 30 and a large running-max jump mid-stream
    if cross:
        qd = q.float().cuda()
        kv = torch.cat([k, v], 1).float().cuda()
        return qd, kv[:, :512], kv[:, 512:], 512 * Tq, 1024 * Tk
    assert Tq == Tk
    qkv = torch.cat([q, k, v], 1).float().cuda()
    return qkv[:, :512], qkv[:, 512:1024], qkv[:, 1024:], 1536 * Tq, 1536 * Tk


CASES = {
    "native_test_case": (2, 200, 320, True, 170),
    "self_freq": (1, TF, TF, False, None),
    "self_time": (1, TT, TT, False, None),
    "cross_freq_from_time": (1, TF, TT, True, None),
    "cross_time_from_freq": (1, TT, TF, True, None),
    "ragged_tk": (2, 256, 100, True, 37),        # Tk not a multiple of 64 (second 32-key sub-tile partly masked)
    "ragged_tk_short": (2, 130, 36, True, None),  # one ragged tile whose second sub-tile holds no key
    "ragged_tq": (2, 300, 256, True, None),      # Tq not a multiple of 128
}


@pytest.mark.parametrize("case", list(CASES))
def test_split_attention_matches_softmax(lib, case):
    B, Tq, Tk, cross, spike = CASES[case]
    q, k, v, q_bs, kv_bs = packed(B, Tq, Tk, seed=40, cross=cross, spike=spike)
    want = reference(q, k, v, Tq, Tk)
    err = maxerr(run(lib, q, k, v, B, Tq, Tk, q_bs, kv_bs), want)
    err_native = maxerr(run(lib, q, k, v, B, Tq, Tk, q_bs, kv_bs, split=False), want)
    print(f"{case}: split {err:.3e}, native fp32 {err_native:.3e}")
    assert err < 2e-5
    assert err <= 2 * err_native


def test_split_attention_deterministic_and_planes_isolated(lib):
    B, Tq, Tk = 31, 200, 320
    q, k, v, q_bs, kv_bs = packed(B, Tq, Tk, seed=60, cross=True)
    o = run(lib, q, k, v, B, Tq, Tk, q_bs, kv_bs)
    assert torch.equal(o, run(lib, q, k, v, B, Tq, Tk, q_bs, kv_bs))
    for b in (0, 17, 30):                       # the item alone (B = 1): same bits
        o1 = run(lib, q[b:b + 1], k[b:b + 1], v[b:b + 1], 1, Tq, Tk, q_bs, kv_bs)
        assert torch.equal(o1[0], o[b])
    # NaN in one plane's K, then in one plane's V: every other plane bit-identical, the poisoned plane non-finite
    for which in ("k", "v"):
        qq, kk, vv, _, _ = packed(B, Tq, Tk, seed=60, cross=True)
        bad, head = 12, 5
        (kk if which == "k" else vv)[bad, head * 64 + 9, 77] = float("nan")
        op = run(lib, qq, kk, vv, B, Tq, Tk, q_bs, kv_bs)
        ov, pv = o.view(B, H, 64, Tq), op.view(B, H, 64, Tq)
        keep = torch.ones(B, H, dtype=torch.bool)
        keep[bad, head] = False
        assert torch.equal(pv[keep], ov[keep]), which
        assert not torch.isfinite(pv[bad, head]).all(), which


# ---- the engine's route --------------------------------------------------------------------------
_ENGINE = r"""
import sys
import numpy as np
import torch
from demucs_amd import _lib
from demucs_amd.htdemucs import HTDemucs
from demucs_amd.synth import synth_mix
from demucs_amd.weights import HTDemucsConfig, synthetic_state_dict
if sys.argv[2] == "switch":
    _lib.load().mi_set_split_bf16(0)
cfg = HTDemucsConfig()
m = HTDemucs(cfg.sources, max_batch=1)
m.load_state_dict(synthetic_state_dict(cfg, 0))
m.to("cuda").eval()
mix = torch.from_numpy(synth_mix(3, cfg.segment_length, "tones"))[None].cuda()
m(mix)
m.profile_begin()
out = m(mix)
rows = m.profile_end()
np.save(sys.argv[1] + ".npy", out.cpu().numpy())
with open(sys.argv[1] + ".txt", "w") as f:
    for r in rows:
        f.write(f"{r['name']} {r['launches']}\n")
"""


def _engine_run(tmp_path, tag, env_extra, mode="default"):
    env = {k: v for k, v in os.environ.items() if k != "MI_X6"}
    env.update(env_extra, PYTHONPATH=ROOT)
    out = str(tmp_path / tag)
    r = subprocess.run([sys.executable, "-c", _ENGINE, out, mode], env=env, capture_output=True, text=True, cwd=ROOT, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    rows = {}
    for line in open(out + ".txt"):
        name, n = line.rsplit(" ", 1)
        rows[name] = int(n)
    return np.load(out + ".npy"), rows


def test_engine_attention_route(tmp_path):
    """float32 htdemucs forward, one fresh process each: by default the 10 attention launches (5 layers x 2 branches) run the
    split kernel; MI_X6=0 and mi_set_split_bf16(0) run the native fp32 kernel, bit-identical to each other; split and native
    forwards stay within the engine's 1e-4 parity target of each other."""
    y_def, rows_def = _engine_run(tmp_path, "default", {})
    assert rows_def.get("attention_x6_kernel") == 10 and "attention_kernel" not in rows_def, rows_def
    y_off, rows_off = _engine_run(tmp_path, "mi_x6_0", {"MI_X6": "0"})
    assert rows_off.get("attention_kernel") == 10 and "attention_x6_kernel" not in rows_off, rows_off
    y_sw, rows_sw = _engine_run(tmp_path, "switch", {}, mode="switch")
    assert rows_sw.get("attention_kernel") == 10 and "attention_x6_kernel" not in rows_sw, rows_sw
    assert np.array_equal(y_sw, y_off)
    d = np.abs(y_def.astype(np.float64) - y_off).max()
    print(f"split vs native fp32 forward: max-abs {d:.3e}")
    assert 0 < d < 1e-4
