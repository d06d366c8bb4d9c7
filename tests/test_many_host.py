"""Host side of `apply_model_many` (demucs_amd/packed.py): the sequential fallback, the planner's RNG calls and the ordering
of its unit, forward and tile tables.  No GPU: the engines are only constructed, never run."""
import math
import random
from fractions import Fraction

import pytest
import torch

from demucs_amd import packed as K
from demucs_amd.apply import BagOfModels, _segment_plan, apply_model, apply_model_many
from demucs_amd.hdemucs import HDemucs
from demucs_amd.hdemucs_weights import HDemucsConfig
from demucs_amd.htdemucs import HTDemucs
from demucs_amd.weights import HTDemucsConfig

SR = 44100


class Toy:
    """Deterministic, non-linear CPU stand-in with a per-forward RNG draw, like the reference's HTDemucs."""
    sources = ["a", "b", "c"]
    samplerate = 100
    audio_channels = 2
    segment = Fraction(4, 1)
    segment_length = 400

    def __init__(self, gain=1.0):
        self.gain = gain

    def valid_length(self, length):
        if length > 400:
            raise ValueError(f"Given length {length} is longer than training length 400")
        return 400

    def to(self, device):
        return self

    def eval(self):
        return self

    def parameters(self):
        yield torch.empty(0)

    def __call__(self, mix):
        random.randrange(1)
        ramp = torch.linspace(0.5, 1.5, mix.shape[-1])
        return torch.stack([torch.tanh(self.gain * (k + 1) * mix * ramp) + 0.01 * k for k in range(3)], 1)


def _tracks(lengths, seed=0):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(2, n, generator=g) for n in lengths]


@pytest.mark.parametrize("shifts", [0, 2])
@pytest.mark.parametrize("bag", [False, True])
def test_many_equals_the_sequential_loop_on_the_host(shifts, bag):
    model = BagOfModels([Toy(1.0), Toy(0.7)], weights=[[1.0, 0.5, 0.0], [0.25, 1.0, 2.0]]) if bag else Toy()
    mixes = _tracks([37, 400, 401, 1234, 90])          # shorter than a segment, exactly one, one + 1 sample, several
    copies = [m.clone() for m in mixes]
    kw = dict(shifts=shifts, overlap=0.25, transition_power=2.0)
    random.seed(11)
    want = [apply_model(model, m[None], **kw)[0] for m in mixes]
    state = random.getstate()
    random.seed(11)
    got = apply_model_many(model, mixes, **kw)
    assert random.getstate() == state
    assert len(got) == len(want)
    for g, w, m, c in zip(got, want, mixes, copies):
        assert g.shape == (3, 2, m.shape[-1])
        assert torch.equal(g, w)
        assert torch.equal(m, c)                       # inputs are never mutated
    assert apply_model_many(model, []) == []


def _ht(max_batch=4, segment=None):
    m = HTDemucs(HTDemucsConfig().sources, max_batch=max_batch)
    if segment is not None:
        m.segment = segment
    return m


def _h(max_batch=3, segment=None):
    m = HDemucs(HDemucsConfig().sources, max_batch=max_batch)
    if segment is not None:
        m.segment = segment
    return m


class _Recorder:
    def __init__(self, seed):
        self.rng, self.calls = random.Random(seed), []

    def randint(self, a, b):
        v = self.rng.randint(a, b)
        self.calls.append(("randint", (a, b), v))
        return v

    def randrange(self, n):
        v = self.rng.randrange(n)
        self.calls.append(("randrange", (n,), v))
        return v


def _expected_draws(members, lengths, shifts, overlap, segment, seed):
    """The sequential loop's RNG calls, restated: track, bag member, shift pass; randint per pass, then randrange(1) per
    segment forward on the HTDemucs route (apply.device_split_accumulate), none on the HDemucs route."""
    rec = _Recorder(seed)
    for n in lengths:
        for sub in members:
            max_shift = int(0.5 * sub.samplerate)
            for _ in range(max(1, shifts)):
                plen = n
                if shifts:
                    plen = n + max_shift - rec.randint(0, max_shift)
                if isinstance(sub, HTDemucs):
                    for _ in _segment_plan(sub, plen, overlap, segment)[3]:
                        rec.randrange(1)
    return rec.calls


@pytest.mark.parametrize("case", ["ht", "ht_bag_shift2", "h_shift1", "mixed_bag"])
def test_planner_draws_the_sequential_loops_rng_calls(case):
    lengths = [SR, 5 * SR + 17, 31 * SR, 1, 343980, 343981]
    shifts, overlap, segment = {"ht": (0, 0.25, None), "ht_bag_shift2": (2, 0.5, None), "h_shift1": (1, 0.25, None),
                                "mixed_bag": (1, 0.25, None)}[case]
    if case == "ht":
        model, members = _ht(), None
    elif case == "ht_bag_shift2":
        members = [_ht(), _ht(3)]
        model = BagOfModels(members, weights=[[1, 0, 0, 0], [0, 1, 1, 1]])
    elif case == "h_shift1":
        model, members, lengths = _h(), None, [20 * SR, 44 * SR, 100 * SR + 3]
    else:
        members = [_ht(), _h()]
        model = BagOfModels(members)
        lengths = [20 * SR, 50 * SR]
    members = members or [model]
    p = K.plan(model, lengths, shifts=shifts, overlap=overlap, segment=segment, rng=_Recorder(5))
    assert p.draws == _expected_draws(members, lengths, shifts, overlap, segment, 5)
    # the module-level default uses Python's global random exactly the same way
    random.seed(5)
    K.plan(model, lengths, shifts=shifts, overlap=overlap, segment=segment)
    after = random.getstate()
    random.seed(5)
    for name, args, _ in p.draws:
        getattr(random, name)(*args)
    assert random.getstate() == after


def _check_order(p):
    """Every accumulator receives its segments in ascending offset order, each unit exactly once, within max_batch."""
    seen = []
    last = {}
    for fw in p.forwards:
        sub = p.members[fw.member]
        assert 1 <= len(fw.units) <= sub.max_batch
        if isinstance(sub, HDemucs):
            assert len({p.units[u].n for u in fw.units}) == 1 and p.units[fw.units[0]].n == fw.valid
        for u in fw.units:
            unit = p.units[u]
            assert unit.off > last.get(unit.pass_idx, -1)
            last[unit.pass_idx] = unit.off
            seen.append(u)
    assert sorted(seen) == list(range(len(p.units)))
    return seen


def _check_tables(p):
    lengths = [max(ps.length for ps in p.passes if ps.track == t) for t in range(1 + max(ps.track for ps in p.passes))]
    src = [0] * len(lengths)
    w_offs = [0] * len(p.members)
    for fw in p.forwards:
        items, tiles = K.forward_tables(p, fw, src, lengths, w_offs)
        assert len(items) == K.ITEM_COLS * len(fw.units)
        covered = set()
        for t in range(0, len(tiles), K.TILE_COLS):
            base, alen, pos, lo, hi, _, wl = tiles[t:t + K.TILE_COLS]
            assert 0 <= lo < hi <= len(fw.units) and hi - lo <= 256 and wl == p.segment_lengths[fw.member]
            offs = []
            for i in range(lo, hi):
                it = items[i * K.ITEM_COLS:(i + 1) * K.ITEM_COLS]
                assert it[3] == base and it[4] == alen          # one accumulator per tile
                offs.append(it[5])
                if it[5] < pos + K.TILE_SPAN and it[5] + it[6] > pos:
                    covered.update((base, q) for q in range(max(pos, it[5]), min(pos + K.TILE_SPAN, it[5] + it[6], alen)))
            assert offs == sorted(offs) and len(set(offs)) == len(offs)
        # every position any item writes lies in some tile
        for u in fw.units:
            unit, ps = p.units[u], p.passes[p.units[u].pass_idx]
            for q in (max(0, unit.off), min(ps.length, unit.off + unit.n) - 1):
                assert (ps.acc_base, q) in covered
    tiles, segs = K.finish_tables(p, w_offs)
    for t in range(0, len(tiles), K.TILE_COLS):
        base, alen, pos, lo, hi, _, _ = tiles[t:t + K.TILE_COLS]
        offs = segs[2 * lo:2 * hi:2]
        assert offs == sorted(offs) and 0 <= pos < alen


@pytest.mark.parametrize("shifts", [0, 2])
def test_htdemucs_tables_keep_ascending_order_and_pack_the_ragged_list(shifts):
    lengths = [int(s * SR) for s in (5, 40, 12.5, 7, 33, 1)] + [343980, 343981]
    p = K.plan(_ht(max_batch=8), lengths, shifts=shifts, overlap=0.25, rng=random.Random(1))
    _check_order(p)
    _check_tables(p)
    sequential = sum(math.ceil(len(ps.offsets) / 8) for ps in p.passes)
    assert p.n_forwards == math.ceil(len(p.units) / 8) < sequential


@pytest.mark.parametrize("overlap", [0.25, 0.5])
@pytest.mark.parametrize("shifts", [0, 1])
def test_hdemucs_tails_come_after_their_pass_full_chunks(overlap, shifts):
    lengths = [60 * SR, 70 * SR + 5, 96 * SR, 96 * SR, 45 * SR, 120 * SR + 1]      # equal tails and different tails
    p = K.plan(_h(max_batch=5, segment=44), lengths, shifts=shifts, overlap=overlap, rng=random.Random(3))
    order = _check_order(p)
    pos = {u: i for i, u in enumerate(order)}
    for pi, ps in enumerate(p.passes):
        mine = [u for u, unit in enumerate(p.units) if unit.pass_idx == pi]
        full = [pos[u] for u in mine if p.units[u].n == p.segment_lengths[0]]
        tails = [pos[u] for u in mine if p.units[u].n < p.segment_lengths[0]]
        assert tails and (not full or max(full) < min(tails))
    _check_tables(p)
    if not shifts:              # the two 96 s tracks have equal tails: they share a forward
        tail_forwards = [fw for fw in p.forwards if fw.valid < p.segment_lengths[0]]
        assert any(len(fw.units) > 1 for fw in tail_forwards)
