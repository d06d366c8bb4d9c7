"""`apply_model_stream` / `Separator.separate_stream` on the MI355X: a track pushed block by block gives `apply_model`'s stems on
the whole track, bit for bit, with the same use of `random` (demucs_amd/stream.py), and `mi_stream_emit` alone equals the torch
operations `_apply_shifts` / `_apply_bag` run on the GPU."""
import ctypes as C
import functools
import random

import numpy as np
import pytest
import torch

from demucs_amd import _lib
from demucs_amd.api import Separator
from demucs_amd.apply import BagOfModels, apply_model, apply_model_stream
from demucs_amd.hdemucs import HDemucs
from demucs_amd.hdemucs_weights import HDemucsConfig, synthetic_hdemucs_state_dict
from demucs_amd.htdemucs import HTDemucs
from demucs_amd.stream import emit_scales
from demucs_amd.synth import synth_mix
from demucs_amd.weights import HTDemucsConfig, synthetic_state_dict

pytestmark = pytest.mark.gpu
SR = 44100
BAG_W = [[1.0, 0.3, 0.5, 2.0], [0.25, 1.0, 1.5, 0.0]]


@functools.lru_cache(maxsize=None)
def _ht_state(seed=0):
    return synthetic_state_dict(HTDemucsConfig(), seed)


@functools.lru_cache(maxsize=None)
def _h_state(channels=48, seed=1):
    return synthetic_hdemucs_state_dict(HDemucsConfig(channels=channels), seed)


def ht(mode="f32", max_batch=4, seed=0):
    m = HTDemucs(HTDemucsConfig().sources, max_batch=max_batch, compute_dtype=mode)
    m.load_state_dict(_ht_state(seed))
    return m.to("cuda").eval()


def hd(mode="f32", max_batch=3, segment=None, channels=48):
    m = HDemucs(HDemucsConfig().sources, max_batch=max_batch, compute_dtype=mode, channels=channels)
    m.load_state_dict(_h_state(channels))
    if segment is not None:
        m.segment = segment
    return m.to("cuda").eval()


def track(n, seed=0, device="cpu"):
    return torch.from_numpy(synth_mix(seed, n, "tones" if seed % 2 else "noise")).to(device)


def schedule(kind, length, seed=0):
    if kind == "one":
        return [length]
    if kind == "1s":
        return [SR] * (length // SR + 1)
    rng = np.random.default_rng(seed)
    out, total = [], 0
    while total < length:
        b = int(rng.choice([0, 1, int(rng.integers(1, 20 * SR))]))
        out.append(b)
        total += b
    return out


def streamed(model, mix, blocks, seed=7, **kw):
    random.seed(seed)
    st = apply_model_stream(model, **kw)
    outs, pos = [], 0
    for b in blocks:
        blk = mix[:, pos:pos + b]
        pos += blk.shape[1]
        o = st.push(blk)
        assert o.device == mix.device and o.shape[-1] == st.emitted - sum(x.shape[-1] for x in outs)
        assert st.emitted >= pos - st.latency
        outs.append(o)
    outs.append(st.finish())
    return torch.cat(outs, -1)


def check_stream(model, mix, blocks, seed=7, **kw):
    kw.setdefault("device", "cuda")
    ref_kw = {k: v for k, v in kw.items() if k != "length"}
    random.seed(seed)
    want = apply_model(model, mix[None], **ref_kw)[0]
    state = random.getstate()
    got = streamed(model, mix, blocks, seed=seed, **kw)
    assert random.getstate() == state
    assert got.shape == want.shape and got.device == want.device
    assert torch.equal(got, want), f"max diff {(got - want).abs().max().item():.3e}"


# ---- 1. HTDemucs, three block schedules ------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("kind,where", [("1s", "cpu"), ("random", "cuda"), ("one", "cuda")])
def test_htdemucs_stream_equals_apply_model(mode, kind, where):
    L = 40 * SR + 123
    check_stream(ht(mode), track(L, seed=3, device=where), schedule(kind, L, seed=len(mode)), shifts=1)


def test_bag_with_shifts_and_length_equals_apply_model():
    L = 23 * SR + 5
    bag = BagOfModels([ht("f32", seed=0), ht("f32", seed=1)], BAG_W)
    check_stream(bag, track(L, seed=4), schedule("random", L, seed=9), shifts=2, length=L)


def test_overlap_power_and_segment_override():
    L = 17 * SR + 11
    check_stream(ht("f32"), track(L, seed=5, device="cuda"), schedule("random", L, seed=3), shifts=1, overlap=0.1,
                 transition_power=2.0, segment=5)


# ---- 2. HDemucs ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["f32", "f16"])
def test_hdemucs_stream_equals_apply_model(mode):
    L = 9 * SR + 777                    # segment 3 s: a few full chunks, then tails
    check_stream(hd(mode, segment=3), track(L, seed=6, device="cuda"), schedule("random", L, seed=5),
                 shifts=1)


def test_demucs_unittest_width_stream():
    L = 7 * SR + 3
    m = hd("f32", max_batch=2, channels=4, segment=2)
    check_stream(m, track(L, seed=8), [SR] * 8, shifts=0)


# ---- 3. mi_stream_emit alone -----------------------------------------------------------------------------------------------
def _ola_finish(acc, offs, lens, SL, weight):
    lib = _lib.load()
    t_offs = torch.tensor(offs, dtype=torch.int64).cuda()
    t_lens = torch.tensor(lens, dtype=torch.int32).cuda()
    _lib.check(lib.mi_ola_finish(acc.data_ptr(), acc.shape[1], acc.shape[0], 0, t_offs.data_ptr(), t_lens.data_ptr(), len(offs),
                                 SL, weight.data_ptr(), C.c_void_p(_lib.current_stream_ptr())), "mi_ola_finish")


def assert_same_bits(got, want, what=""):
    """Equal bit patterns, NaN positions included (a NaN's payload is not compared)."""
    a = torch.where(torch.isnan(got), float("nan"), got).view(torch.int32)
    b = torch.where(torch.isnan(want), float("nan"), want).view(torch.int32)
    bad = (a != b).nonzero()
    if len(bad):
        idx = [tuple(i) for i in bad[:4].tolist()]
        pairs = [(float(got[i]), float(want[i]), hex(int(a[i]) & 0xffffffff), hex(int(b[i]) & 0xffffffff)) for i in idx]
        raise AssertionError(f"{what}: {len(bad)} of {got.numel()} differ, e.g. {list(zip(idx, pairs))}")


EMIT_SL = 3000
# stride 0.75 SL is the two-fold overlap of overlap=0.25; SL // 4 is four-fold, where the float32 sum of weights depends on its order
EMIT_CASES = [pytest.param(m, s, 2250, id=f"{m}-{s}") for m, s in [(1, 0), (1, 1), (1, 3), (2, 2), (3, 1), (4, 3), (2, 0)]]
EMIT_CASES += [pytest.param(m, s, EMIT_SL // 4, id=f"{m}-{s}-fourfold") for m, s in [(1, 0), (2, 2)]]


@pytest.mark.parametrize("members,shifts,stride", EMIT_CASES)
def test_emit_kernel_equals_the_torch_operations(members, shifts, stride):
    lib = _lib.load()
    g = torch.Generator().manual_seed(members * 10 + shifts)
    S, Ch, SL, L = 4, 2, EMIT_SL, 10000
    rows = S * Ch
    weights = (torch.cat([torch.arange(1, SL // 2 + 1), torch.arange(SL - SL // 2, 0, -1)]) / (SL // 2)).float().cuda()
    bag = [[float(x) for x in torch.rand(S, generator=g) * 2] for _ in range(members)] if members > 1 else None
    passes, segs, accs, want = [], [], [], None
    max_shift = 500
    base = 0
    member_out = []
    t0, t1 = 1234, 8765
    for e in range(members):
        out = None
        for _ in range(max(1, shifts)):
            d = int(torch.randint(0, max_shift + 1, (1,), generator=g)) if shifts else 0       # max_shift - shift
            plen = L + d
            acc = torch.randn(rows, plen, generator=g) * 3
            acc[torch.rand(rows, plen, generator=g) < 0.01] = float("nan")
            acc[torch.rand(rows, plen, generator=g) < 0.01] = float("inf")
            acc[torch.rand(rows, plen, generator=g) < 0.01] = -float("inf")
            acc = acc.cuda()
            offs = list(range(0, plen, stride))
            lens = [min(plen - o, SL) for o in offs]
            s_lo = len(segs) // 2
            for o, n in zip(offs, lens):
                segs += [o, n]
            passes += [base, plen, d + t0, s_lo, len(segs) // 2, 0, SL, e]
            base += rows * plen
            accs.append(acc.reshape(-1).clone())
            res = acc.clone()
            _ola_finish(res, offs, lens, SL, weights)
            piece = res.view(S, Ch, plen)[..., d:]
            out = piece.clone() if out is None else out.add_(piece)
        if shifts:
            out /= shifts
        member_out.append(out)
    if bag is None:
        want = member_out[0]
    else:
        totals = [0.0] * S
        for out, ws in zip(member_out, bag):
            for k, w in enumerate(ws):
                out[k, :, :] *= w
                totals[k] += w
            want = out if want is None else want.add_(out)
        for k in range(S):
            want[k, :, :] /= totals[k]
    stats = torch.tensor([0.25, 1.75], dtype=torch.float32).cuda()
    want_aff = want.clone().contiguous()
    _lib.check(lib.mi_track_affine(want_aff.data_ptr(), want_aff.numel(), stats.data_ptr(), 1, C.c_void_p(_lib.current_stream_ptr())),
               "mi_track_affine")
    acc_all = torch.cat(accs)
    t_passes = torch.tensor(passes, dtype=torch.int64).cuda()
    t_segs = torch.tensor(segs, dtype=torch.int64).cuda()
    scales = torch.tensor(emit_scales(shifts, members, bag, S), dtype=torch.float32).cuda()
    for name, aff, ref in [("plain", None, want), ("affine", stats, want_aff)]:
        got = torch.empty(S, Ch, t1 - t0, device="cuda")
        _lib.check(lib.mi_stream_emit(acc_all.data_ptr(), acc_all.numel(), S, Ch, t_passes.data_ptr(), len(passes) // 8,
                                      t_segs.data_ptr(), len(segs) // 2, weights.data_ptr(), weights.numel(), scales.data_ptr(),
                                      members, shifts, int(bag is not None), aff.data_ptr() if aff is not None else None,
                                      t1 - t0, got.data_ptr(), got.numel(), C.c_void_p(_lib.current_stream_ptr())),
                   "mi_stream_emit")
        assert_same_bits(got, ref[..., t0:t1], name)


# ---- 4. Separator.separate_stream --------------------------------------------------------------------------------------------
def _stats_for(wav):
    """The track's own (mean, std) in the form separate_stream takes: mi_mono_stats gives mean and s = std + 1e-8 in float32;
    any float32 x with float32(x + 1e-8) == s makes the same normaliser."""
    lib = _lib.load()
    dev = wav.cuda().contiguous()
    scratch = torch.empty(lib.mi_mono_stats_scratch_bytes(), dtype=torch.uint8, device="cuda")
    stats = torch.empty(2, dtype=torch.float32, device="cuda")
    _lib.check(lib.mi_mono_stats(dev.data_ptr(), dev.shape[0], dev.shape[1], scratch.data_ptr(), stats.data_ptr(),
                                 C.c_void_p(_lib.current_stream_ptr())), "mi_mono_stats")
    mean, s = (np.float32(v) for v in stats.cpu().tolist())
    x = np.float32(s - np.float32(1e-8))
    for cand in (x, np.nextafter(x, np.float32(0)), np.nextafter(x, np.float32(np.inf)), s):
        if np.float32(cand + np.float32(1e-8)) == s:
            return float(mean), float(cand)
    raise AssertionError("no std maps onto the normaliser")


def test_separate_stream_equals_separate_tensor():
    L = 21 * SR + 17
    wav = track(L, seed=12) * 0.3
    sep = Separator(ht("f32"), device="cuda", shifts=1)
    random.seed(3)
    _, want = sep.separate_tensor(wav.clone())
    mean, std = _stats_for(wav)
    random.seed(3)
    ss = sep.separate_stream(mean, std)
    outs = [ss.push(wav[:, i:i + 3 * SR]) for i in range(0, L, 3 * SR)] + [ss.finish()]
    for k in want:
        got = torch.cat([o[k] for o in outs], -1)
        assert torch.equal(got, want[k]), k
    with pytest.raises(ValueError, match="sample rate"):
        sep.separate_stream(sr=48000)


# ---- 5. two interleaved streams on one model -----------------------------------------------------------------------------------
def test_interleaved_streams_are_isolated():
    m = ht("f32")
    a, b = track(19 * SR + 3, seed=13, device="cuda"), track(14 * SR + 9, seed=14, device="cuda")
    random.seed(1)
    alone_a = streamed(m, a, [SR] * 20, seed=1, shifts=0)
    alone_b = streamed(m, b, [SR] * 15, seed=1, shifts=0)
    random.seed(1)
    sa, sb = apply_model_stream(m, shifts=0), apply_model_stream(m, shifts=0)
    oa, ob = [], []
    for i in range(20):
        oa.append(sa.push(a[:, i * SR:(i + 1) * SR]))
        ob.append(sb.push(b[:, i * SR:(i + 1) * SR]))
    oa.append(sa.finish())
    ob.append(sb.finish())
    assert torch.equal(torch.cat(oa, -1), alone_a) and torch.equal(torch.cat(ob, -1), alone_b)


# ---- 6. bounded device memory ----------------------------------------------------------------------------------------------------
def test_device_memory_does_not_grow_with_the_stream():
    m = ht("f32")
    st = apply_model_stream(m, shifts=1, device="cuda")
    block = track(SR, seed=15)
    peaks = {}
    torch.cuda.synchronize()
    for sec in range(8 * 60):
        st.push(block)
        if sec == 30:
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
        if sec + 1 in (2 * 60, 8 * 60):
            torch.cuda.synchronize()
            peaks[sec + 1] = torch.cuda.max_memory_allocated()
    st.finish()
    stems = 8 * 60 * SR * 4 * 2 * 4
    assert abs(peaks[8 * 60] - peaks[2 * 60]) < 1 << 20, peaks
    assert peaks[8 * 60] < stems, peaks
    assert st.device_bytes() < stems // 10
