"""The nn.Module-like surface `HTDemucs` and `HDemucs` share (demucs_amd/_engine_model.py), without a GPU: what
`load_state_dict` accepts and refuses, what `state_dict` returns, and that nothing runs off the GPU."""
import functools

import numpy as np
import pytest
import torch

from demucs_amd._lib import EngineError
from demucs_amd.hdemucs import HDemucs
from demucs_amd.hdemucs_weights import HDemucsConfig, synthetic_hdemucs_state_dict
from demucs_amd.htdemucs import HTDemucs
from demucs_amd.weights import HTDemucsConfig, synthetic_state_dict

KINDS = ["htdemucs", "hdemucs"]


def make(kind):
    if kind == "htdemucs":
        return HTDemucs(HTDemucsConfig().sources, max_batch=1)
    return HDemucs(HDemucsConfig().sources, max_batch=1, channels=4)


@functools.lru_cache(maxsize=None)
def state(kind):
    """A full synthetic state of the class's schema; shared between the tests and never written to."""
    if kind == "htdemucs":
        return synthetic_state_dict(HTDemucsConfig(), 0)
    return synthetic_hdemucs_state_dict(HDemucsConfig(channels=4), 3)


@pytest.mark.parametrize("kind", KINDS)
def test_load_state_dict_names_missing_and_unexpected_keys(kind):
    m = make(kind)
    first = next(iter(m._schema))
    with pytest.raises(RuntimeError, match="missing") as e:
        m.load_state_dict({})
    assert first in str(e.value)                            # the first missing keys are named
    extra = dict(state(kind), made_up_key=np.zeros(1, np.float32))
    with pytest.raises(RuntimeError, match=r"missing \[\], unexpected \['made_up_key'\]"):
        m.load_state_dict(extra)
    with pytest.raises(RuntimeError, match="no weights"):   # neither refusal left a half-loaded state behind
        m.state_dict()
    m.load_state_dict(extra, strict=False)                  # the extra key is dropped
    assert list(m.state_dict()) == list(m._schema)


@pytest.mark.parametrize("kind", KINDS)
def test_load_state_dict_refuses_a_wrong_shape_by_name(kind):
    m = make(kind)
    key, shape = next((k, s) for k, s in m._schema.items() if len(s) >= 2)
    bad = dict(state(kind))
    bad[key] = np.zeros(tuple(shape) + (2,), np.float32)
    with pytest.raises(RuntimeError, match="size mismatch for " + key.replace(".", r"\.")) as e:
        m.load_state_dict(bad)
    assert str(tuple(shape)) in str(e.value) and str(tuple(shape) + (2,)) in str(e.value)


@pytest.mark.parametrize("kind", KINDS)
def test_module_surface_without_weights_or_gpu(kind):
    m = make(kind)
    name = type(m).__name__
    with pytest.raises(RuntimeError, match=name + " has no weights"):
        m.state_dict()
    with pytest.raises(NotImplementedError, match=name):
        m.train(True)
    with pytest.raises(NotImplementedError):
        m.train()
    assert m.eval() is m and m.train(False) is m and m.training is False
    assert m.to("cpu") is m
    assert [p.device.type for p in m.parameters()] == ["cpu"]
    length = m.segment_length if kind == "htdemucs" else 4096
    mix = torch.zeros(1, 2, length)
    with pytest.raises(RuntimeError, match="no weights") as e:          # no weights: said before the device is looked at
        m(mix)
    assert not isinstance(e.value, EngineError)
    m.load_state_dict(state(kind))
    with pytest.raises(EngineError, match=name + " only runs on a GPU device"):
        m(mix)
    with pytest.raises(ValueError, match="compute_dtype"):
        type(m)(m.sources, compute_dtype="f64")


def test_hdemucs_state_round_trips_as_float32():
    sd = state("hdemucs")
    m = make("hdemucs").load_state_dict(sd)
    got = m.state_dict()
    assert list(got) == list(sd) == list(m._schema)
    for k, v in sd.items():
        assert got[k].dtype == torch.float32 and tuple(got[k].shape) == v.shape
        assert np.array_equal(got[k].numpy(), v), k
    got[next(iter(got))].zero_()                                       # state_dict hands out copies
    assert np.array_equal(m.state_dict()[next(iter(sd))].numpy(), next(iter(sd.values())))
    # a float16 checkpoint (states.py stores half precision) comes back as the float32 values of its halves, tensors or arrays
    half = {k: (torch.from_numpy(v).half() if i % 2 else v.astype(np.float16)) for i, (k, v) in enumerate(sd.items())}
    got = make("hdemucs").load_state_dict(half).state_dict()
    for k, v in sd.items():
        assert got[k].dtype == torch.float32
        assert np.array_equal(got[k].numpy(), v.astype(np.float16).astype(np.float32)), k
