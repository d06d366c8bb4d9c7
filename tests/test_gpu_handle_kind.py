"""The C interface's handles are typed: an entry of one engine refuses a handle of the other with MI_EINVAL before it reads the
handle's state or enqueues anything, the refusal leaves both engines as they were (their next forwards are bit-identical to
the ones before), and the profiler entries serve both kinds."""
import ctypes as C

import pytest
import torch

from demucs_amd import _lib
from demucs_amd.hdemucs import HDemucs
from demucs_amd.hdemucs_weights import HDemucsConfig, synthetic_hdemucs_state_dict
from demucs_amd.htdemucs import HTDemucs
from demucs_amd.synth import synth_mix
from demucs_amd.weights import HTDemucsConfig, synthetic_state_dict

pytestmark = pytest.mark.gpu
MI_EINVAL = -1
H_LEN = 20000           # HDemucs chunk: 20 STFT frames


class Engines:
    def __init__(self):
        cfg = HTDemucsConfig()
        self.ht = HTDemucs(cfg.sources, max_batch=1)
        self.ht.load_state_dict(synthetic_state_dict(cfg, 0))
        self.ht.to("cuda").eval()
        self.hd = HDemucs(HDemucsConfig().sources, max_batch=1, channels=4)
        self.hd.load_state_dict(synthetic_hdemucs_state_dict(HDemucsConfig(channels=4), 1))
        self.hd.to("cuda").eval()
        self.ht_mix = torch.from_numpy(synth_mix(1, cfg.segment_length, "tones"))[None].cuda()
        self.hd_mix = torch.from_numpy(synth_mix(2, H_LEN, "noise"))[None].cuda()
        self.ht_out = self.ht(self.ht_mix).clone()
        self.hd_out = self.hd(self.hd_mix).clone()
        torch.cuda.synchronize()
        self.ht_handle = C.c_void_p(self.ht._ensure_handle())
        self.hd_handle = C.c_void_p(self.hd._handles[(self.hd._device, False)][0])


@pytest.fixture(scope="module")
def eng():
    return Engines()


def _refused(status, entry):
    msg = _lib.load().mi_last_error().decode()
    assert status == MI_EINVAL, (entry, status, msg)
    assert msg.startswith(entry + ":") and " htdemucs " in msg and " hdemucs " in msg, msg      # the entry and both kinds
    return msg


def test_entries_refuse_the_other_engines_handle_and_leave_both_intact(eng):
    lib, st = _lib.load(), C.c_void_p(_lib.current_stream_ptr())
    n = C.c_int64(-7)
    S = len(eng.ht.sources)
    # mi_model_* on the hdemucs handle
    out = torch.full((1, S, 2, eng.ht.segment_length), 3.0, device="cuda")
    msg = _refused(lib.mi_model_forward(eng.hd_handle, eng.ht_mix.data_ptr(), out.data_ptr(), 1, st), "mi_model_forward")
    assert "belongs to the hdemucs engine" in msg and "one of the htdemucs engine" in msg, msg
    _refused(lib.mi_model_tap(eng.hd_handle, b"x0", None, 1, C.byref(n), None), "mi_model_tap")
    assert lib.mi_model_device_bytes(eng.hd_handle) == 0
    assert lib.mi_last_error().decode().startswith("mi_model_device_bytes:")
    # mi_hmodel_* on the htdemucs handle
    hout = torch.full((1, S, 2, H_LEN), 3.0, device="cuda")
    msg = _refused(lib.mi_hmodel_forward(eng.ht_handle, eng.hd_mix.data_ptr(), hout.data_ptr(), 1, H_LEN, st), "mi_hmodel_forward")
    assert "belongs to the htdemucs engine" in msg and "one of the hdemucs engine" in msg, msg
    _refused(lib.mi_hmodel_tap(eng.ht_handle, b"enc0", None, 1, C.byref(n), None), "mi_hmodel_tap")
    _refused(lib.mi_hmodel_status(eng.ht_handle, st), "mi_hmodel_status")
    assert lib.mi_hmodel_device_bytes(eng.ht_handle) == 0
    torch.cuda.synchronize()
    assert n.value == -7                                        # no tap answered
    assert bool((out == 3.0).all()) and bool((hout == 3.0).all())      # nothing was enqueued on the callers' buffers
    # the right entries still answer, and the forwards give what they gave before, bit for bit
    assert lib.mi_model_device_bytes(eng.ht_handle) == eng.ht.device_bytes() > 0
    assert lib.mi_hmodel_device_bytes(eng.hd_handle) == eng.hd.device_bytes() > 0
    eng.hd.check()
    assert torch.equal(eng.ht(eng.ht_mix), eng.ht_out)
    assert torch.equal(eng.hd(eng.hd_mix), eng.hd_out)
    assert eng.ht.tap("x0", 1).shape[0] == 1 and eng.hd.tap("enc0", 1).shape[0] == 1


def test_profiler_entries_serve_both_kinds(eng):
    for m, mix, want, row in ((eng.ht, eng.ht_mix, eng.ht_out, "attention"), (eng.hd, eng.hd_mix, eng.hd_out, "lstm")):
        m.profile_begin()
        out = m(mix)
        rows = m.profile_end()
        assert torch.equal(out, want)
        assert rows and all(r["launches"] > 0 and r["name"] for r in rows), rows
        assert any(r["name"].startswith("conv_gemm") for r in rows), rows       # the shared conv launcher's rows
        assert any(row in r["name"] for r in rows), rows                        # ... and a row only this engine books
