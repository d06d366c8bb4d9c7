"""`apply_model_many` / `Separator.separate_tensors` on the MI355X: many tracks of different lengths in shared batched forwards
(demucs_amd/packed.py), bit for bit the sequential loop of `apply_model` / `separate_tensor`, with the same use of `random`."""
import ctypes as C
import functools
import random

import pytest
import torch

from demucs_amd import _lib
from demucs_amd import packed as K
from demucs_amd.api import Separator
from demucs_amd.apply import BagOfModels, apply_model, apply_model_many
from demucs_amd.hdemucs import HDemucs
from demucs_amd.hdemucs_weights import HDemucsConfig, synthetic_hdemucs_state_dict
from demucs_amd.htdemucs import HTDemucs
from demucs_amd.synth import synth_mix
from demucs_amd.weights import HTDemucsConfig, synthetic_state_dict

pytestmark = pytest.mark.gpu
SR = 44100
SL = HTDemucsConfig().segment_length


@functools.lru_cache(maxsize=None)
def _ht_state(seed=0):
    return synthetic_state_dict(HTDemucsConfig(), seed)


@functools.lru_cache(maxsize=None)
def _h_state():
    return synthetic_hdemucs_state_dict(HDemucsConfig(), 1)


def ht(mode="f32", max_batch=4, seed=0):
    m = HTDemucs(HTDemucsConfig().sources, max_batch=max_batch, compute_dtype=mode)
    m.load_state_dict(_ht_state(seed))
    return m.to("cuda").eval()


def hd(mode="f16", max_batch=3, segment=None):
    m = HDemucs(HDemucsConfig().sources, max_batch=max_batch, compute_dtype=mode)
    m.load_state_dict(_h_state())
    if segment is not None:
        m.segment = segment
    return m.to("cuda").eval()


def tracks(lengths, seed=0, device="cpu"):
    return [torch.from_numpy(synth_mix(seed + i, n, "tones" if i % 2 else "noise")).to(device) for i, n in enumerate(lengths)]


def check_many(model, mixes, seed=7, **kw):
    kw.setdefault("device", "cuda")             # host inputs: the engine still runs on the GPU, as with apply_model
    copies = [m.clone() for m in mixes]
    random.seed(seed)
    want = [apply_model(model, m[None], **kw)[0] for m in mixes]
    state = random.getstate()
    random.seed(seed)
    got = apply_model_many(model, mixes, **kw)
    assert random.getstate() == state
    assert len(got) == len(mixes)
    for i, (g, w, m, c) in enumerate(zip(got, want, mixes, copies)):
        assert g.device == m.device and g.shape == w.shape
        assert torch.equal(g, w), f"track {i} (length {m.shape[-1]}): max diff {(g - w).abs().max().item():.3e}"
        assert torch.equal(m, c), "an input was mutated"


# ---- 1. batch invariance: the premise of bit identity --------------------------------------------------------------------
@pytest.mark.parametrize("engine,mode", [("ht", "f32"), ("ht", "bf16"), ("ht", "f16"), ("hd", "f32"), ("hd", "f16")])
def test_every_item_of_a_full_batch_equals_its_own_single_forward(engine, mode):
    B = 4
    if engine == "ht":
        m = ht(mode, max_batch=B)
        segs = torch.stack(tracks([SL] * B, seed=20, device="cuda"))
        fwd = lambda x: m.forward_segments(x.contiguous())           # noqa: E731
    else:
        m = hd(mode, max_batch=B)
        segs = torch.stack(tracks([10 * SR + 3] * B, seed=30, device="cuda"))
        fwd = lambda x: m(x.contiguous())                            # noqa: E731
    single = [fwd(segs[i:i + 1])[0].clone() for i in range(B)]
    for rot in range(B):                     # every segment at every batch position
        order = [(i + rot) % B for i in range(B)]
        out = fwd(segs[order])
        for pos, i in enumerate(order):
            assert torch.equal(out[pos], single[i]), f"{engine} {mode}: segment {i} at batch position {pos} of {B}"


# ---- 2. apply_model_many == the sequential loop ------------------------------------------------------------------------
RAGGED = [SR, SL, SL + 1, 30 * SR + 11, 47 * SR, 70 * SR - 5]


@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("shifts,overlap,tp", [(0, 0.25, 1.0), (1, 0.25, 1.0), (2, 0.5, 2.0)])
def test_htdemucs_many_equals_loop(where, shifts, overlap, tp):
    m = ht("f32", max_batch=8)
    check_many(m, tracks(RAGGED, device="cpu" if where == "host" else "cuda"), shifts=shifts, overlap=overlap,
               transition_power=tp)


@pytest.mark.parametrize("mode", ["bf16", "f16"])
def test_htdemucs_half_modes_many_equals_loop(mode):
    check_many(ht(mode, max_batch=8), tracks(RAGGED, seed=3), shifts=1)


def test_segment_override_many_equals_loop():
    check_many(ht("f32", max_batch=8), tracks([SR, 5 * SR, 5 * SR + 1, 23 * SR], seed=5, device="cuda"), shifts=1, segment=5)


def test_one_hot_bag_many_equals_loop():
    members = [ht("f32", max_batch=6, seed=s) for s in range(4)]
    bag = BagOfModels(members, weights=[[1.0 if k == i else 0.0 for k in range(4)] for i in range(4)])
    check_many(bag, tracks([SR, 12 * SR + 1, 31 * SR], seed=9), shifts=1)
    check_many(BagOfModels(members[:2], weights=[[1.0, 0.5, 0.0, 2.0], [0.25, 1.0, 1.5, 2.0]]),
               tracks([SL + 1, 20 * SR], seed=4, device="cuda"), shifts=0)


@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("shifts", [0, 1])
def test_hdemucs_f16_many_equals_loop(where, shifts):
    # 10 s chunks: the two 25 s tracks have equal tails (without shifts), the others differ; 8 s is a lone short chunk
    m = hd("f16", max_batch=3, segment=10)
    check_many(m, tracks([25 * SR, 25 * SR, 31 * SR + 7, 8 * SR], seed=11, device="cpu" if where == "host" else "cuda"),
               shifts=shifts)


# ---- 3. the packed route needs fewer forwards ------------------------------------------------------------------------
def test_forward_count_matches_the_plan(monkeypatch):
    m = ht("f32", max_batch=8)
    mixes = tracks(RAGGED, seed=2, device="cuda")
    lib = _lib.load()
    real = lib.mi_model_forward
    calls = []

    def counting(*args):
        calls.append(args[3])
        return real(*args)

    monkeypatch.setattr(lib, "mi_model_forward", counting)
    random.seed(1)
    for x in mixes:
        apply_model(m, x[None], shifts=1)
    sequential = len(calls)
    calls.clear()
    random.seed(1)
    apply_model_many(m, mixes, shifts=1)
    random.seed(1)
    p = K.plan(m, [x.shape[-1] for x in mixes], shifts=1)
    assert len(calls) == p.n_forwards < sequential
    assert all(b <= 8 for b in calls)


# ---- 4. Separator.separate_tensors ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("sr", [None, 32000])
def test_separate_tensors_equals_separate_tensor_loop(sr):
    sep = Separator(ht("f32", max_batch=8), device="cuda", shifts=1)
    wavs = [3.0 * w + 0.2 for w in tracks([2 * SR, 9 * SR + 5, 26 * SR], seed=13)]
    random.seed(4)
    want = [sep.separate_tensor(w.clone(), sr) for w in wavs]
    state = random.getstate()
    random.seed(4)
    got = sep.separate_tensors([w.clone() for w in wavs], sr)
    assert random.getstate() == state
    for (gw, gs), (ww, ws) in zip(got, want):
        assert torch.equal(gw, ww)
        assert list(gs) == list(ws)
        for k in ws:
            assert torch.equal(gs[k], ws[k])


# ---- 5. the packed kernels against the one-track entries -------------------------------------------------------------
def _stream():
    return C.c_void_p(_lib.current_stream_ptr())


def test_packed_kernels_equal_the_one_track_entries_and_isolate_tracks():
    lib = _lib.load()
    g = torch.Generator().manual_seed(0)
    ch, rows, valid, W = 2, 8, 3000, 2500
    lengths = [7001, 2999, 12000]
    src = [torch.randn(ch, n, generator=g).cuda() for n in lengths]
    packed = torch.cat([s.reshape(-1) for s in src])
    src_offs = [0, ch * lengths[0], ch * (lengths[0] + lengths[1])]
    acc_lens = [n + 500 for n in lengths]
    acc_base = [0, rows * acc_lens[0], rows * (acc_lens[0] + acc_lens[1])]
    weight = torch.rand(W, generator=g).cuda() + 0.1
    # items: per track, ascending offsets, random lens / trims; consecutive per accumulator
    items, per_track = [], []
    for t, n in enumerate(lengths):
        offs = sorted(torch.randint(-300, acc_lens[t] - 10, (7,), generator=g).unique().tolist())
        mine = []
        for o in offs:
            ln = int(torch.randint(1, W + 1, (1,), generator=g))
            tr = int(torch.randint(0, valid - ln + 1, (1,), generator=g))
            st = int(torch.randint(-400, n + 400, (1,), generator=g))
            mine.append((st, o, ln, tr))
            items += [src_offs[t], n, st, acc_base[t], acc_lens[t], o, ln, tr]
        per_track.append(mine)
    B = sum(len(x) for x in per_track)
    t_items = torch.tensor(items, dtype=torch.int64).cuda()
    # gather
    seg = torch.full((B, ch, valid), 7.0, device="cuda")
    _lib.check(lib.mi_segments_gather_packed(packed.data_ptr(), packed.numel(), ch, t_items.data_ptr(), B, valid, seg.data_ptr(),
                                             seg.numel(), _stream()), "gather_packed")
    i = 0
    for t, mine in enumerate(per_track):
        starts = torch.tensor([x[0] for x in mine], dtype=torch.int64).cuda()
        ref = torch.empty(len(mine), ch, valid, device="cuda")
        _lib.check(lib.mi_segments_gather(src[t].data_ptr(), lengths[t], ch, starts.data_ptr(), len(mine), valid, ref.data_ptr(),
                                          ref.numel(), _stream()), "gather")
        assert torch.equal(seg[i:i + len(mine)], ref)
        i += len(mine)

    def run_packed(mo):
        acc = torch.randn(sum(rows * a for a in acc_lens), generator=torch.Generator().manual_seed(1)).cuda()
        tiles, i0 = [], 0
        for t, mine in enumerate(per_track):
            lo = max(0, min(x[1] for x in mine))
            hi = min(acc_lens[t], max(x[1] + x[2] for x in mine))
            tiles += [v for pos in range(lo, hi, K.TILE_SPAN) for v in (acc_base[t], acc_lens[t], pos, i0, i0 + len(mine), 0, W)]
            i0 += len(mine)
        t_tiles = torch.tensor(tiles, dtype=torch.int64).cuda()
        _lib.check(lib.mi_ola_accumulate_packed(acc.data_ptr(), acc.numel(), rows, mo.data_ptr(), valid, mo.numel(),
                                                t_items.data_ptr(), B, t_tiles.data_ptr(), len(tiles) // K.TILE_COLS,
                                                weight.data_ptr(), W, _stream()), "ola_packed")
        ftiles, segs = [], []
        for t, mine in enumerate(per_track):
            s0 = len(segs) // 2
            for x in sorted(mine, key=lambda x: x[1]):
                segs += [x[1], x[2]]
            ftiles += [v for pos in range(0, acc_lens[t], K.TILE_SPAN) for v in (acc_base[t], acc_lens[t], pos, s0, len(segs) // 2,
                                                                                   0, W)]
        t_ft, t_segs = torch.tensor(ftiles, dtype=torch.int64).cuda(), torch.tensor(segs, dtype=torch.int64).cuda()
        _lib.check(lib.mi_ola_finish_packed(acc.data_ptr(), acc.numel(), rows, t_ft.data_ptr(), len(ftiles) // K.TILE_COLS,
                                            t_segs.data_ptr(), len(segs) // 2, weight.data_ptr(), W, _stream()), "finish_packed")
        return acc

    def run_single(mo):
        acc = torch.randn(sum(rows * a for a in acc_lens), generator=torch.Generator().manual_seed(1)).cuda()
        i0 = 0
        for t, mine in enumerate(per_track):
            view = acc[acc_base[t]:acc_base[t] + rows * acc_lens[t]]
            offs = torch.tensor([x[1] for x in mine], dtype=torch.int64).cuda()
            lens = torch.tensor([x[2] for x in mine], dtype=torch.int32).cuda()
            trims = torch.tensor([x[3] for x in mine], dtype=torch.int32).cuda()
            part = mo[i0:i0 + len(mine)].contiguous()
            lo = max(0, min(x[1] for x in mine))
            hi = min(acc_lens[t], max(x[1] + x[2] for x in mine))
            _lib.check(lib.mi_ola_accumulate(view.data_ptr(), acc_lens[t], rows, part.data_ptr(), valid, part.numel(), offs.data_ptr(),
                                             lens.data_ptr(), trims.data_ptr(), len(mine), lo, hi, weight.data_ptr(), W, _stream()),
                       "ola")
            _lib.check(lib.mi_ola_finish(view.data_ptr(), acc_lens[t], rows, 0, offs.data_ptr(), lens.data_ptr(), len(mine), W,
                                         weight.data_ptr(), _stream()), "finish")
            torch.cuda.synchronize()
            i0 += len(mine)
        return acc

    mo = torch.randn(B, rows, valid, generator=g).cuda()
    got, want = run_packed(mo), run_single(mo)
    assert torch.equal(torch.isnan(got), torch.isnan(want))
    assert torch.equal(torch.nan_to_num(got), torch.nan_to_num(want))
    # a NaN in track 1's model output never reaches another track's accumulator
    poisoned = mo.clone()
    n0 = len(per_track[0])
    poisoned[n0:n0 + len(per_track[1])] = float("nan")
    bad = run_packed(poisoned)
    for t in (0, 2):
        sl = slice(acc_base[t], acc_base[t] + rows * acc_lens[t])
        assert torch.equal(torch.nan_to_num(bad[sl], nan=123.0), torch.nan_to_num(got[sl], nan=123.0))


# ---- review follow-ups: the shapes the packed route runs, the side engine, device inputs of the Separator --------------
@pytest.mark.parametrize("mode", ["f32", "bf16", "f16"])
def test_batch_invariance_at_max_batch_32(mode):
    """The packed route runs forwards of up to max_batch items: no kernel may choose its tiling or split by B."""
    B = 32
    m = ht(mode, max_batch=B)
    segs = torch.stack(tracks([SL] * B, seed=40, device="cuda"))
    single = [m.forward_segments(segs[i:i + 1].contiguous())[0].clone() for i in range(B)]
    for rot in (0, 1, 13, 31):
        order = [(i + rot) % B for i in range(B)]
        out = m.forward_segments(segs[order].contiguous())
        for pos, i in enumerate(order):
            assert torch.equal(out[pos], single[i]), f"{mode}: segment {i} at batch position {pos} of {B}"
    for n in (5, 17):               # partial batches on the same handle
        out = m.forward_segments(segs[:n].contiguous())
        for i in range(n):
            assert torch.equal(out[i], single[i]), f"{mode}: segment {i} of a batch of {n}"


@pytest.mark.parametrize("mode", ["f32", "f16"])
def test_hdemucs_side_engine_equals_main_engine_while_both_run(mode):
    """A tail chunk on the single-item side engine, launched on the side stream while the main engine runs a batched
    forward (what both the single-track route and the packed route do), equals the main engine's own B = 1 forward."""
    m = hd(mode, max_batch=3, segment=10)
    full = torch.stack(tracks([10 * SR] * 3, seed=50, device="cuda"))
    tails = [x[None] for x in tracks([3 * SR + 7, SR + 1], seed=60, device="cuda")]
    want_full = m(full).clone()
    want_tails = [m(t).clone() for t in tails]
    main, side = torch.cuda.current_stream(), m.side_stream()
    for _ in range(3):
        side.wait_stream(main)
        with torch.cuda.stream(side):
            got_tails = [m(t, aux=True) for t in tails]
        got_full = m(full)
        main.wait_stream(side)
        m.check()
        assert torch.equal(got_full, want_full)
        for g, w in zip(got_tails, want_tails):
            assert torch.equal(g, w)


def test_hdemucs_packed_tails_use_the_side_engine():
    m = hd("f16", max_batch=3, segment=10)
    mixes = tracks([25 * SR, 31 * SR + 7, 17 * SR + 3], seed=12, device="cuda")
    check_many(m, mixes, shifts=0)
    assert (torch.device("cuda", torch.cuda.current_device()), True) in m._handles     # the tails ran on the side engine


def test_device_results_do_not_share_the_run_buffer():
    m = ht("f32", max_batch=8)
    out = apply_model_many(m, tracks([SR, 3 * SR], seed=8, device="cuda"), shifts=0)
    assert out[0].untyped_storage().data_ptr() != out[1].untyped_storage().data_ptr()
    assert out[0].untyped_storage().nbytes() == out[0].numel() * 4


@pytest.mark.parametrize("case", ["distinct", "same_tensor_twice", "views_of_one_buffer"])
def test_separate_tensors_device_inputs_equal_the_loop(case):
    """Device inputs are normalised in place: the result and the caller's tensors afterwards must match the loop's, also
    when list entries share storage."""
    sep = Separator(ht("f32", max_batch=8), device="cuda", shifts=1)
    base = [3.0 * w + 0.2 for w in tracks([4 * SR, 4 * SR, 9 * SR + 5], seed=21, device="cuda")]

    def make():
        if case == "distinct":
            return [w.clone() for w in base]
        if case == "same_tensor_twice":
            a = base[0].clone()
            return [a, a, base[2].clone()]
        buf = torch.stack(base[:2]).clone()
        return [buf[0], buf[1], base[2].clone()]

    mine, theirs = make(), make()
    random.seed(6)
    want = [sep.separate_tensor(w, None) for w in theirs]
    state = random.getstate()
    random.seed(6)
    got = sep.separate_tensors(mine, None)
    assert random.getstate() == state
    for a, b in zip(mine, theirs):
        assert torch.equal(a, b)                   # the caller's tensors end where the loop leaves them
    for (gw, gs), (ww, ws) in zip(got, want):
        assert torch.equal(gw, ww)
        for k in ws:
            assert torch.equal(gs[k], ws[k])
