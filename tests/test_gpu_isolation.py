"""Isolation of batch items and of successive forwards, with non-finite input as the probe.

The reference normalises every item by its own mean and std (demucs/htdemucs.py and demucs/hdemucs.py forward), so a NaN or Inf
in item k makes every output of item k NaN and leaves the other items untouched; successive forwards of one model are
independent.  The engine shares its workspace between layers, items and calls (the DConv hidden tensor, operand images, statistic
and Gram accumulators), and finite leftovers times zero weights add exactly 0 -- a NaN leftover does not.  So a poisoned item or an
earlier poisoned forward must leave every other result BIT-identical (the suite already relies on forwards being bit-reproducible:
test_gpu_hdemucs.py test_tail_chunk_overlap_is_bit_identical_and_stable)."""
import functools

import pytest
import torch

from demucs_amd import apply as P
from demucs_amd.hdemucs import HDemucs
from demucs_amd.hdemucs_weights import HDemucsConfig, synthetic_hdemucs_state_dict
from demucs_amd.htdemucs import HTDemucs
from demucs_amd.synth import synth_mix
from demucs_amd.weights import HTDemucsConfig, synthetic_state_dict

pytestmark = pytest.mark.gpu
MODES = ["f32", "bf16", "f16"]
SR = 44100
HT_TAPS = ["x0", "xt0", "enc0", "tenc0", "enc1", "tenc1", "enc2", "tenc2", "enc3", "tenc3", "tr_f", "tr_t", "yspec", "ytime"]
H_TAPS = ["enc0", "tenc0", "enc1", "tenc1", "enc2", "tenc2", "enc3", "tenc3", "tenc4", "enc4", "enc5", "dec0+skip", "dec1+skip",
          "tdec0+skip", "dec2+skip", "tdec1+skip", "dec3+skip", "tdec2+skip", "dec4+skip", "tdec3+skip", "dec5", "tdec4"]
POISONS = {"all_nan": lambda x: x.fill_(float("nan")),
           "nan_sample": lambda x: x[1, x.shape[-1] // 2].fill_(float("nan")),
           "inf_sample": lambda x: x[0, x.shape[-1] // 3].fill_(float("inf"))}


@functools.lru_cache(maxsize=None)
def _ht_state():
    return synthetic_state_dict(HTDemucsConfig(), 0)


@functools.lru_cache(maxsize=None)
def _h_state():
    return synthetic_hdemucs_state_dict(HDemucsConfig(), 1)


def ht_engine(mode, max_batch=3):
    m = HTDemucs(HTDemucsConfig().sources, max_batch=max_batch, compute_dtype=mode)
    m.load_state_dict(_ht_state())
    return m.to("cuda").eval()


def h_engine(mode, max_batch=3):
    m = HDemucs(HDemucsConfig().sources, max_batch=max_batch, compute_dtype=mode)
    m.load_state_dict(_h_state())
    return m.to("cuda").eval()


def mixes(B, L, seed):
    return torch.stack([torch.from_numpy(synth_mix(seed + i, L, "noise" if i % 2 else "tones")) for i in range(B)]).cuda()


def _same(a, b):
    """bit-identical, NaN at the same places counting as equal (taps include never-stored pitch padding)"""
    return torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(torch.nan_to_num(a), torch.nan_to_num(b))


def first_bad_tap(m, taps, run_a, run_b, j):
    """Name of the first internal stage where item j of forward run_a() and of forward run_b() differ."""
    B = None
    snap = {}
    for run, key in ((run_a, "a"), (run_b, "b")):
        out = run()
        B = out.shape[0]
        for t in taps:
            try:
                snap[key, t] = m.tap(t, B)[j].clone()
            except Exception:       # a tap the engine did not register for this geometry
                snap[key, t] = None
    for t in taps:
        a, b = snap["a", t], snap["b", t]
        if a is not None and b is not None and not _same(a, b):
            return t
    return "none of the taps (output stage)"


def check_batch_isolation(m, taps, clean, run):
    """clean (B, 2, L): every poison at every item position k leaves items j != k bit-identical and makes item k all NaN."""
    want = run(clean).clone()
    assert bool(torch.isfinite(want).all()), "clean batch gives non-finite output"
    fails = []
    for pname, poison in POISONS.items():
        for k in range(clean.shape[0]):
            x = clean.clone()
            poison(x[k])
            got = run(x)
            if not bool(torch.isnan(got[k]).all()):
                fails.append(f"{pname} k={k}: item {k} has {int((~torch.isnan(got[k])).sum())} non-NaN outputs")
            for j in range(clean.shape[0]):
                if j != k and not torch.equal(got[j], want[j]):
                    stage = first_bad_tap(m, taps, lambda: run(clean), lambda: run(x), j)
                    n = int((got[j] != want[j]).sum() + torch.isnan(got[j]).sum())
                    fails.append(f"{pname} k={k}: item {j} differs from the clean batch in {n} samples; first stage: {stage}")
    assert not fails, "\n".join(fails)


# ---- 1. batch-item isolation -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_htdemucs_batch_items_are_isolated(mode):
    m = ht_engine(mode)
    clean = mixes(3, m.segment_length, 100)
    check_batch_isolation(m, HT_TAPS, clean, m)


@pytest.mark.parametrize("L", [5 * SR + 3, 10 * SR], ids=["5s_odd", "10s"])
@pytest.mark.parametrize("mode", MODES)
def test_hdemucs_batch_items_are_isolated(mode, L):
    m = h_engine(mode)
    clean = mixes(3, L, 110)
    check_batch_isolation(m, H_TAPS, clean, m)
    m.check()


# ---- 2. forward-to-forward isolation on one handle --------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_htdemucs_forward_after_nan_forward(mode):
    m = ht_engine(mode)
    SL = m.segment_length
    x1, x2 = mixes(1, SL, 120), mixes(2, SL, 121)
    ref1 = m(x1).clone()
    m(torch.full((3, 2, SL), float("nan"), device="cuda"))
    assert torch.equal(m(x1), ref1), "B=1 after an all-NaN B=3 forward differs from the B=1 before it"
    got2 = m(x2).clone()
    fresh = ht_engine(mode)
    want2 = fresh(x2)
    assert torch.equal(got2, want2), f"B=2 after an all-NaN forward differs from a fresh handle in {int((got2 != want2).sum())} samples"


@pytest.mark.parametrize("mode", MODES)
def test_hdemucs_forward_after_nan_forward(mode):
    """Length and B change between the forwards; HDemucs.check() after the NaN forward: a NaN hidden state still carries its step
    tag (common.h lstm_cell ORs the tag into the bits after the arithmetic), so the persistent BLSTM must not time out on it."""
    m = h_engine(mode)
    short, odd, long_ = mixes(1, 2561, 130), mixes(2, 5 * SR + 3, 131), mixes(2, 44 * SR, 132)
    a = m(short).clone()
    m(torch.full((3, 2, 44 * SR), float("nan"), device="cuda"))
    m.check()
    assert torch.equal(m(short), a), "short chunk after a NaN 44 s B=3 forward differs from the same chunk before it"
    for x, name in ((odd, "5 s + 3 samples, B=2"), (long_, "44 s, B=2")):
        got = m(x).clone()
        fresh = h_engine(mode)
        want = fresh(x)
        fresh.check()
        del fresh
        assert torch.equal(got, want), f"{name} after a NaN forward differs from a fresh handle in {int((got != want).sum())} samples"
    m.check()


# ---- 3. the same through apply_model ------------------------------------------------------------------------------------------
def _apply_isolation(make, mix, **kw):
    m = make()
    clean = P.apply_model(m, mix, shifts=0, overlap=0.25, **kw).clone()
    poisoned = mix.clone()
    poisoned[0, 1, mix.shape[-1] // 2] = float("nan")
    got = P.apply_model(m, poisoned, shifts=0, overlap=0.25, **kw)
    assert torch.isnan(got[0]).any(), "the NaN of track 0 reached none of its stems"
    assert torch.equal(got[1], clean[1]), f"track 1 changed by a NaN in track 0 in {int((got[1] != clean[1]).sum())} samples"
    again = P.apply_model(m, mix, shifts=0, overlap=0.25, **kw)
    want = P.apply_model(make(), mix, shifts=0, overlap=0.25, **kw)
    assert torch.equal(again, want), "clean call after a NaN call differs from a fresh model's result"
    assert torch.equal(again, clean)
    return m


def test_htdemucs_apply_model_tracks_are_isolated():
    L = 10 * SR + 17                                # more than one 7.8 s segment: the split / overlap-add route
    _apply_isolation(lambda: ht_engine("f32"), mixes(2, L, 140))


@pytest.mark.parametrize("listener", [False, True], ids=["tails_on_side_engine", "track0_tail_on_main_engine"])
def test_hdemucs_apply_model_tracks_are_isolated(listener):
    """segment override 4 s: 3 full chunks per track and a 0.6 s tail chunk (demucs_amd/apply.py ragged_split_accumulate).  A
    track's tail runs on the single-item side engine unless the track has a listener: with a callback, the first track (the
    poisoned one) runs its tail on the main engine and the second still runs its tail on the side engine."""
    L = int(2.4 * 4 * SR) + 777
    kw = dict(segment=4)
    if listener:
        kw["callback"] = lambda d: None
    m = _apply_isolation(lambda: h_engine("f16"), mixes(2, L, 150), **kw)
    assert (m._device, True) in m._handles                       # track 1's tail ran on the side engine
    m.check()
