"""nSDR scoring on the MI355X through the Python face: `audio.new_sdr`, `audio.SdrStream`, `Separator.evaluate_blocks` and
`Separator.score_tensor`.  The sums are `mi_sdr`'s bit for bit for every partition of the two tracks and every interleaving of
the two kinds of push, so an evaluation pass on top of `separate_blocks` gives the score of `separate_tensor`'s stems exactly
without the stems leaving the device.  The bound against the oracle is test_gpu_score.py's."""
import ctypes as C
import functools
import random

import numpy as np
import pytest
import torch

from demucs_amd import _lib, audio
from demucs_amd.api import Separator
from demucs_amd.audio import SdrStream, TrackScore
from oracle import apply_oracle as A
from test_gpu_analyse import offline
from test_gpu_ingest import byte_chunks, to_i16
from test_gpu_stream import ht, track

pytestmark = pytest.mark.gpu
SR = 44100
BOUND_DB = 1e-8
STATE = 4 * 2 * audio.SDR_SLOTS * 8          # mi_sdr_state_bytes(4)


def kernel_sums(ref, est):
    """`mi_sdr` through the C ABI on (B, S, C, L) device tensors: (B, S, 2) float64 on the host."""
    lib = _lib.load()
    B, S, ch, L = ref.shape
    state = torch.empty(lib.mi_sdr_state_bytes(S), dtype=torch.uint8, device="cuda")
    scratch = torch.empty(lib.mi_sdr_scratch_bytes(S), dtype=torch.uint8, device="cuda")
    sums = torch.empty(B, S, 2, dtype=torch.float64, device="cuda")
    _lib.check(lib.mi_sdr(ref.data_ptr(), est.data_ptr(), B, S, ch, L, state.data_ptr(), scratch.data_ptr(), sums.data_ptr(),
                          C.c_void_p(_lib.current_stream_ptr())), "mi_sdr")
    return sums.cpu()


def same_bits(a, b) -> bool:
    a, b = (np.ascontiguousarray(np.asarray(v, dtype=np.float64)) for v in (a, b))
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


@functools.lru_cache(maxsize=None)
def tracks(S=4, ch=2, L=3001, B=2, seed=0):
    g = torch.Generator().manual_seed(seed)
    ref = torch.randn(B, S, ch, L, generator=g)
    return ref, ref + 0.2 * torch.randn(B, S, ch, L, generator=g)


def whole_score(ref, est) -> TrackScore:
    """The `TrackScore` of one (S, C, L) pair by `new_sdr`'s route."""
    return TrackScore.from_sums(audio.sdr_sums(ref[None], est[None])[0], ref.shape[-1])


# ---- new_sdr ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", ["cpu", "cuda"])
def test_new_sdr_equals_the_kernel_and_the_oracle(where):
    ref, est = (t.to(where) for t in tracks())
    got = audio.new_sdr(ref, est)
    assert got.shape == (2, 4) and got.dtype == torch.float64 and got.device.type == where
    sums = kernel_sums(ref.cuda(), est.cuda())
    want = 10 * torch.log10((sums[..., 0] + 1e-7) / (sums[..., 1] + 1e-7))
    assert same_bits(got.cpu().numpy(), want.numpy())
    oracle = A.new_sdr(ref.cpu().double(), est.cpu().double())
    err = (got.cpu() - oracle).abs().max().item()
    print(f"new_sdr on {where}: max |score - oracle| {err:.3e} dB")
    assert err <= BOUND_DB
    assert same_bits(audio.new_sdr(ref.double(), est.double()).cpu().numpy(), got.cpu().numpy())    # float32 values either way
    empty = audio.new_sdr(ref[..., :0], est[..., :0])
    assert empty.shape == (2, 4) and (empty == 0).all() and empty.device.type == where


# ---- SdrStream -------------------------------------------------------------------------------------------------------------------------
def test_every_interleaving_gives_the_whole_track_score():
    ref, est = (t[0] for t in tracks(L=audio.SDR_SLOTS + 3001, B=1))
    L = ref.shape[-1]
    want = whole_score(ref.cuda(), est.cuda())
    assert same_bits(want.nsdr, audio.new_sdr(ref[None], est[None])[0].numpy())

    def cut(t, sizes):
        out, pos = [], 0
        for n in sizes:
            out.append(t[..., pos:pos + n])
            pos += n
        assert pos >= L
        return out

    a, b = [1, 999, 50000, 0, 1, L], [7, 30000, 30000, 256, L]
    orders = {
        "references far ahead": [("r", x) for x in cut(ref, a)] + [("e", x.cuda()) for x in cut(est, b)],
        "estimates ahead": [("e", x) for x in cut(est.cuda(), b)] + [("r", x) for x in cut(ref.cuda(), a)],
        "alternating, uneven": [p for pairs in zip((("r", x) for x in cut(ref, a[:5] + [1, L])),
                                                   (("e", x) for x in cut(est, [3] + b + [L]))) for p in pairs],
    }
    for name, pushes in orders.items():
        st = SdrStream(4, 2)
        for kind, block in pushes:
            (st.push_references if kind == "r" else st.push_estimates)(block)
            assert st.scored == min(st.references_pushed, st.estimates_pushed)
        assert st.references_pushed == st.estimates_pushed == L, name
        assert st.device_bytes() == STATE
        got = st.finish()
        assert got == want and got.length == L, (name, got, want)
        assert same_bits(got.num, want.num) and same_bits(got.den, want.den) and same_bits(got.nsdr, want.nsdr)


def test_scores_mid_stream_device_bytes_and_a_length_mismatch():
    ref, est = (t[0].cuda() for t in tracks(L=5000, B=1))
    st = SdrStream(4, 2)
    assert st.device_bytes() == 0 and st.scores() == TrackScore([0.0] * 4, [0.0] * 4, [0.0] * 4, 0)
    st.push_references(ref[..., :3000])
    assert st.scored == 0 and st.device_bytes() == 3000 * 4 * 2 * 4            # no state yet: nothing was scored
    st.push_estimates(est[..., :1200])
    assert st.scored == 1200 and st.device_bytes() == STATE + 1800 * 4 * 2 * 4
    mid = st.scores()
    assert mid == whole_score(ref[..., :1200].contiguous(), est[..., :1200].contiguous())
    assert same_bits(mid.nsdr, audio.new_sdr(ref[None, ..., :1200], est[None, ..., :1200])[0].cpu().numpy())
    assert st.scores() == mid                                                    # the state is only read
    st.push_estimates(est[..., 1200:3000])
    assert st.scored == 3000 and st.device_bytes() == STATE                     # the lagging side caught up
    st.push_estimates(est[..., 3000:])
    assert st.device_bytes() == STATE + 2000 * 4 * 2 * 4
    with pytest.raises(ValueError, match="references ended after 3000 samples and the estimates after 5000"):
        st.finish()
    assert not st.finished
    st.push_references(ref[..., 3000:])
    assert st.finish() == whole_score(ref, est) and st.device_bytes() == STATE
    with pytest.raises(RuntimeError, match="twice"):
        st.finish()


def test_pcm_references_that_end_mid_frame():
    """Per-source int16 chunks of 4097 and 1 bytes: none is a multiple of the 4-byte frame."""
    ref, est = (t[0] for t in tracks(L=20011, B=1, seed=3))
    frames, floats = zip(*(to_i16(r * 0.2) for r in ref))
    data = [q.numpy().tobytes() + b"\x7f\x01\x02" for q in frames]               # an incomplete last frame: dropped
    want = whole_score(torch.stack(floats).cuda(), est.cuda())
    st = SdrStream(4, 2, pcm="i16", src_channels=2)
    st.push_estimates(est[..., :777])
    tails = set()
    for i in range(0, len(data[0]), 4097):
        st.push_references([d[i:i + 4096] for d in data])
        st.push_references([d[i + 4096:i + 4097] for d in data])
        tails.add(st.trailing_bytes)
    st.push_estimates(est[..., 777:])
    assert st.trailing_bytes == 3 and tails == {0, 1, 2, 3}
    assert st.finish() == want


# ---- Separator.evaluate_blocks / score_tensor ----------------------------------------------------------------------------------------
def synthetic_references(wav, S=4, seed=1):
    """(S, C, L) stems that sum to the mix: a split of it with fixed gains plus noise that cancels."""
    g = torch.Generator().manual_seed(seed)
    noise = 0.05 * torch.randn(S, *wav.shape, generator=g)
    noise -= noise.mean(0, keepdim=True)
    gains = torch.tensor([0.4, 0.3, 0.2, 0.1])[:S, None, None]
    return (gains * wav[None] + noise).contiguous()


def blocks_of(t, size):
    return [t[..., i:i + size] for i in range(0, t.shape[-1], size)]


def check_evaluate_blocks(sep, wav, refs, seed):
    """float blocks, i16 mix blocks and i16 reference chunks against the whole-track score; returns it."""
    L = wav.shape[-1]
    stems, state = offline(sep, wav, seed)
    want = whole_score(refs.cuda(), torch.stack(list(stems.values())).cuda())
    assert same_bits(want.nsdr, audio.new_sdr(refs[None], torch.stack(list(stems.values()))[None])[0].numpy())
    random.seed(seed)
    blocks = list(sep.separate_blocks(lambda: iter(blocks_of(wav, SR + 7))))
    assert random.getstate() == state and sum(b["drums"].shape[-1] for b in blocks) == L
    reads = []

    def source():
        reads.append("mix")
        return iter(blocks_of(wav, SR + 7))

    def references():
        reads.append("refs")
        return iter(blocks_of(refs, 30011))

    random.seed(seed)
    got = sep.evaluate_blocks(source, references)
    assert random.getstate() == state
    assert sorted(reads) == ["mix", "mix", "refs"], reads                        # the mix is read twice, the references once
    assert got == want and got.length == L, (got, want)
    return want, state


def test_evaluate_blocks_equals_the_whole_track_score():
    L = 3 * SR + 5
    sep = Separator("demucs_unittest", device="cuda", shifts=1)
    assert sep.model.sources == ["drums", "bass", "other", "vocals"]
    q, wav = to_i16(track(L, seed=15) * 0.9)                                     # the floats an int16 feed stands for
    rq, rfloats = zip(*(to_i16(r) for r in synthetic_references(wav)))
    refs = torch.stack(rfloats)
    want, state = check_evaluate_blocks(sep, wav, refs, 21)
    assert np.isfinite(want.nsdr).all() and (want.den > 0).all()

    # i16 PCM mix blocks that end anywhere
    random.seed(21)
    got = sep.evaluate_blocks(lambda: iter(byte_chunks(q.numpy().tobytes(), seed=2, typical=2 * SR)),
                              lambda: iter(blocks_of(refs.cuda(), 50000)), pcm="i16")
    assert random.getstate() == state and got == want

    # per-source i16 reference chunks that end mid-frame
    data = [r.numpy().tobytes() for r in rq]
    random.seed(21)
    got = sep.evaluate_blocks(lambda: iter(blocks_of(wav.cuda(), 2 * SR + 1)),
                              lambda: ([d[i:i + 65537] for d in data] for i in range(0, len(data[0]), 65537)), ref_pcm="i16")
    assert random.getstate() == state and got == want

    # score_tensor: the same score, separate_tensor's stems
    stems, _ = offline(sep, wav, 21)
    for where in ("cpu", "cuda"):
        random.seed(21)
        score, out = sep.score_tensor(wav.to(where), refs)
        assert random.getstate() == state and score == want
        assert list(out) == list(stems)
        for k in stems:
            assert out[k].device.type == where and torch.equal(out[k].cpu(), stems[k]), k
    with pytest.raises(ValueError, match="are not the stems'"):
        sep.score_tensor(wav, refs[..., :-1])


def test_htdemucs_evaluate_blocks_equals_the_whole_track_score():
    L = 9 * SR + 17
    wav = track(L, seed=13) * 0.3
    check_evaluate_blocks(Separator(ht("f32"), device="cuda", shifts=1), wav, synthetic_references(wav), 3)
