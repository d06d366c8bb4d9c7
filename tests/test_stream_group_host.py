"""Host logic of `demucs_amd.stream.StreamGroup` on CPU with the stand-in models of test_apply_host.py (plain-torch route): every
per-push output of a group equals what a solo `ModelStream` of that stream returns, `random` ends in the same state, each stream
keeps its latency bound, and every refusal leaves the group as it was."""
import random

import pytest
import torch

from demucs_amd.apply import BagOfModels, apply_model_stream, apply_model_stream_group
from test_apply_host import RaggedToy, ToyModel

SEG = 400


def make_script(n_streams, seed, lengths=None):
    """A random schedule of calls [("open", i) | ("push", {i: n}) | ("finish", [i, ...])] over n_streams tracks: staggered opens,
    zero-length blocks, random finish order and groupings.  Returns (script, lengths)."""
    g = random.Random(seed)
    lengths = lengths or [g.choice([1, 37, SEG - 1, SEG + 1, 1000, 2345]) for _ in range(n_streams)]
    pos = [0] * n_streams
    state = ["new"] * n_streams
    script = []
    while any(s != "done" for s in state):
        new = [i for i in range(n_streams) if state[i] == "new"]
        if new and (g.random() < 0.3 or all(s != "open" for s in state)):
            i = new[0]
            script.append(("open", i))
            state[i] = "open"
            continue
        live = [i for i in range(n_streams) if state[i] == "open"]
        full = [i for i in live if pos[i] >= lengths[i]]
        if full and g.random() < 0.4:
            g.shuffle(full)
            keys = full[:g.randint(1, len(full))]
            script.append(("finish", keys))
            for i in keys:
                state[i] = "done"
            continue
        pick = [i for i in live if g.random() < 0.7] or live[:1]
        g.shuffle(pick)
        blocks = {}
        for i in pick:
            b = min(lengths[i] - pos[i], g.choice([0, 1, g.randint(1, 50), g.randint(1, 700)]))
            blocks[i] = b
            pos[i] += b
        script.append(("push", blocks))
    return script, lengths


def run_script(make, script, lengths, kw, grouped, seed=5, length_kw=False):
    """Runs the script through one group (grouped=True) or one solo ModelStream per track; returns (per-call outputs, state)."""
    mixes = [torch.randn(2, n, generator=torch.Generator().manual_seed(100 + i)) for i, n in enumerate(lengths)]
    random.seed(seed)
    model = make()
    group = apply_model_stream_group(model, **kw) if grouped else None
    keys, pos, outs = {}, [0] * len(lengths), []
    for op, arg in script:
        if op == "open":
            length = lengths[arg] if length_kw else None
            keys[arg] = group.open(length=length) if grouped else apply_model_stream(model, length=length, **kw)
        elif op == "push":
            blocks = {}
            for i, b in arg.items():
                blocks[i] = mixes[i][:, pos[i]:pos[i] + b]
                pos[i] += b
            if grouped:
                got = group.push({keys[i]: blk for i, blk in blocks.items()})
                assert list(got) == [keys[i] for i in blocks]
                res = {i: got[keys[i]] for i in blocks}
                for i in blocks:
                    assert group.pushed(keys[i]) == pos[i]
                    assert group.emitted(keys[i]) >= pos[i] - group.latency
            else:
                res = {i: keys[i].push(blk) for i, blk in blocks.items()}
            outs.append(res)
        else:
            if grouped:
                got = group.finish([keys[i] for i in arg])
                outs.append({i: got[keys[i]] for i in arg})
                assert not set(keys[i] for i in arg) & set(group.open_keys)
            else:
                outs.append({i: keys[i].finish() for i in arg})
    return outs, random.getstate()


def check_group(make, n_streams, seed, length_kw=False, **kw):
    script, lengths = make_script(n_streams, seed)
    want, want_state = run_script(make, script, lengths, kw, grouped=False, length_kw=length_kw)
    got, got_state = run_script(make, script, lengths, kw, grouped=True, length_kw=length_kw)
    assert len(got) == len(want)
    for call, (g, w) in enumerate(zip(got, want)):
        assert list(g) == list(w), call
        for i in w:
            assert g[i].shape == w[i].shape and torch.equal(g[i], w[i]), (call, i)
    assert got_state == want_state


@pytest.mark.parametrize("n_streams", [1, 2, 3, 6])
@pytest.mark.parametrize("shifts", [0, 1])
def test_group_equals_solo_streams(n_streams, shifts):
    for seed in range(3):
        check_group(ToyModel, n_streams, seed * 10 + n_streams, shifts=shifts)
        check_group(RaggedToy, n_streams, seed * 10 + n_streams + 1, shifts=shifts)


@pytest.mark.parametrize("n_streams", [2, 5])
def test_two_shift_passes_with_length(n_streams):
    check_group(ToyModel, n_streams, 41, length_kw=True, shifts=2)
    check_group(RaggedToy, n_streams, 42, shifts=2)


def test_weighted_bag():
    w = [[1.0, 0.0, 0.5], [0.3, 1.0, 1.5]]
    check_group(lambda: BagOfModels([ToyModel(1.0), ToyModel(0.7)], w), 4, 51, length_kw=True, shifts=1)
    check_group(lambda: BagOfModels([ToyModel(1.0), ToyModel(0.7)], w), 3, 52, shifts=0)
    check_group(lambda: BagOfModels([RaggedToy(), RaggedToy()], w), 4, 53, shifts=2)


def test_late_open_and_untouched_streams():
    """A stream opened after others have run long, and streams missing from a push keep their state."""
    script = [("open", 0), ("open", 1)] + [("push", {0: 300, 1: 300})] * 6 + [("push", {0: 500})] * 4 + \
        [("open", 2)] + [("push", {2: 250, 1: 100, 0: 10})] * 8 + [("finish", [1, 2, 0])]
    lengths = [3910, 2600, 2000]
    for shifts in (0, 1):
        want, ws = run_script(ToyModel, script, lengths, dict(shifts=shifts), grouped=False)
        got, gs = run_script(ToyModel, script, lengths, dict(shifts=shifts), grouped=True)
        assert gs == ws
        for g, w in zip(got, want):
            for i in w:
                assert torch.equal(g[i], w[i])


class Refusing(ToyModel):
    def __call__(self, mix):
        raise AssertionError("the model must not be called")


@pytest.mark.parametrize("kw,match", [
    (dict(split=False), "split"),
    (dict(callback=lambda d: None), "callback"),
    (dict(progress=True), "progress"),
])
def test_group_refuses_what_a_stream_refuses(kw, match):
    state = random.getstate()
    with pytest.raises(ValueError, match=match) as solo:
        apply_model_stream(Refusing(), **kw)
    with pytest.raises(ValueError, match=match) as grp:
        apply_model_stream_group(Refusing(), **kw)
    assert str(grp.value) == str(solo.value)
    assert random.getstate() == state


def snapshot(g):
    return [(k, g.pushed(k), g.emitted(k)) for k in g.open_keys], random.getstate()


def test_refusals_leave_the_group_unchanged():
    g = apply_model_stream_group(ToyModel(), shifts=1)
    a, b = g.open(), g.open(length=30)
    g.push({a: torch.randn(2, 450), b: torch.randn(2, 20)})
    with pytest.raises(ValueError, match="length"):
        g.open(length=-1)
    before = snapshot(g)
    bad_calls = [
        lambda: g.push({a: torch.randn(2, 50), 99: torch.randn(2, 5)}),                  # unknown key
        lambda: g.push({a: torch.randn(2, 50), b: torch.randn(1, 5)}),                   # channel count
        lambda: g.push({a: torch.randn(2, 50), b: torch.randn(2, 11)}),                  # past the declared length
        lambda: g.push({a: torch.randn(2, 50), b: torch.randn(2)}),                      # not (channels, n)
        lambda: g.finish([a, b]),                                                         # b short of its length
        lambda: g.finish([a, a]),                                                         # listed twice
        lambda: g.finish([a, 1234]),                                                      # unknown key
    ]
    for call in bad_calls:
        with pytest.raises(ValueError):
            call()
        assert snapshot(g) == before
    c = g.open()
    with pytest.raises(ValueError, match="before any sample"):
        g.finish([a, c])
    assert snapshot(g)[0][:2] == before[0]
    g.finish([a])
    for call in (lambda: g.push({a: torch.randn(2, 5)}), lambda: g.finish([a]), lambda: g.emitted(a)):
        with pytest.raises(ValueError, match="unknown or finished"):
            call()
    with pytest.raises(ValueError, match="length"):
        g2 = apply_model_stream_group(BagOfModels([Refusing(), Refusing()]), shifts=1)
        g2.open()                                        # a per-segment draw before a later shift offset: length= needed


def test_nan_block_stays_in_its_stream():
    lengths = [1300, 1300, 1300]
    mixes = [torch.randn(2, n, generator=torch.Generator().manual_seed(i)) for i, n in enumerate(lengths)]
    bad = mixes[1].clone()
    bad[:, 500:520] = float("nan")
    bad[:, 800] = float("inf")

    def run(tracks):
        random.seed(0)
        g = apply_model_stream_group(ToyModel(), shifts=1)
        ks = [g.open() for _ in tracks]
        outs = [[] for _ in tracks]
        for p in range(0, 1300, 130):
            got = g.push({k: t[:, p:p + 130] for k, t in zip(ks, tracks)})
            for i, k in enumerate(ks):
                outs[i].append(got[k])
        fin = g.finish(ks)
        return [torch.cat(o + [fin[k]], -1) for o, k in zip(outs, ks)]

    clean, dirty = run(mixes), run([mixes[0], bad, mixes[2]])
    assert torch.equal(clean[0], dirty[0]) and torch.equal(clean[2], dirty[2])
    assert not torch.isfinite(dirty[1]).all()


def test_separator_stream_group_on_host():
    from demucs_amd.api import Separator
    sep = Separator(ToyModel(), device="cpu", shifts=0)
    sg = sep.separate_stream_group()
    with pytest.raises(ValueError, match="mean and std"):
        sg.open(mean=0.1)
    wav = torch.randn(2, 900, generator=torch.Generator().manual_seed(3))
    random.seed(2)
    ss = sep.separate_stream(0.05, 0.9)
    want = [ss.push(wav[:, i:i + 200]) for i in range(0, 900, 200)] + [ss.finish()]
    random.seed(2)
    k = sg.open(0.05, 0.9)
    got = [sg.push({k: wav[:, i:i + 200]})[k] for i in range(0, 900, 200)] + [sg.finish([k])[k]]
    for g_, w_ in zip(got, want):
        assert list(g_) == ToyModel.sources
        for s in w_:
            assert torch.equal(g_[s], w_[s])
