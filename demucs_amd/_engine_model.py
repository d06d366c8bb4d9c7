"""What the host-side model objects (`HTDemucs`, `HDemucs`) share: the nn.Module-like surface `apply_model` uses, the weights
as the engine reads them, and the handle-level calls that are the same for both engines.

A subclass sets `_schema` (key -> shape), `_state = None`, `_device = None`, `compute_dtype`, `training = False` in its
constructor and provides `_release()`, which destroys its engine handles.
"""
from __future__ import annotations

import ctypes as C
from collections import OrderedDict
from typing import Dict

import numpy as np
import torch

from . import _lib


class EngineModel:
    #: compute modes of the engine (mi_config.dtype): operand type of the matrix-core GEMMs and of attention;
    #: accumulation, statistics, norms, softmax and the STFT / iSTFT are float32 in every mode
    COMPUTE_DTYPES = {"f32": 0, "bf16": 1, "f16": 2}

    @classmethod
    def _check_compute_dtype(cls, compute_dtype: str) -> str:
        if compute_dtype not in cls.COMPUTE_DTYPES:
            raise ValueError(f"compute_dtype must be one of {sorted(cls.COMPUTE_DTYPES)}, got {compute_dtype!r}")
        return compute_dtype

    # ---- nn.Module-like surface ---------------------------------------------------------------
    def load_state_dict(self, state: Dict[str, "np.ndarray | torch.Tensor"], strict: bool = True):
        """Accepts the reference checkpoint's `state` (float32 or float16, states.py:83-107)."""
        missing = [k for k in self._schema if k not in state]
        unexpected = [k for k in state if k not in self._schema]
        if strict and (missing or unexpected):
            raise RuntimeError(f"Error(s) in loading state_dict: missing {missing[:4]}..., unexpected {unexpected[:4]}..."
                               if len(missing) + len(unexpected) > 8 else
                               f"Error(s) in loading state_dict: missing {missing}, unexpected {unexpected}")
        new: "OrderedDict[str, np.ndarray]" = OrderedDict()
        for k, shape in self._schema.items():
            v = state[k]
            if isinstance(v, torch.Tensor):
                v = v.detach().to("cpu", torch.float32).numpy()
            v = np.ascontiguousarray(v, dtype=np.float32)
            if tuple(v.shape) != tuple(shape):
                raise RuntimeError(f"size mismatch for {k}: checkpoint {tuple(v.shape)} vs model {tuple(shape)}")
            new[k] = v
        self._state = new
        self._release()
        return self

    def state_dict(self) -> "OrderedDict[str, torch.Tensor]":
        self._require_weights()
        return OrderedDict((k, torch.from_numpy(v.copy())) for k, v in self._state.items())

    def eval(self):
        self.training = False
        return self

    def train(self, mode: bool = True):
        if mode:
            raise NotImplementedError(f"demucs_amd.{type(self).__name__} is inference-only")
        return self

    def parameters(self):
        """A single placeholder tensor on the model's device (apply.py:213 asks for the device)."""
        yield torch.empty(0, device=self._device or torch.device("cpu"))

    def to(self, device):
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        # Engine handles are cached per device: `apply_model` moves every sub-model of a bag to the compute device and
        # back to its "home" on each call (apply.py:213-218); re-packing 42 M weights each time would dominate.
        # `release()` frees them explicitly.
        self._device = device
        return self

    def __del__(self):
        try:
            self._release()
        except Exception:
            pass

    # ---- what creating an engine handle needs ---------------------------------------------------
    def _require_weights(self) -> None:
        if self._state is None:
            raise RuntimeError(f"{type(self).__name__} has no weights: call load_state_dict first")

    def _require_runnable(self) -> None:
        self._require_weights()
        if self._device is None or self._device.type != "cuda":
            raise _lib.EngineError(f"demucs_amd.{type(self).__name__} only runs on a GPU device (MI355X); call .to('cuda'). "
                                   "There is no CPU implementation in this package.")

    def _tensor_descs(self):
        """The weights as the `mi_tensor_desc` array of mi_model_create / mi_hmodel_create (points into `self._state`)."""
        descs = (_lib.MiTensorDesc * len(self._state))()
        for d, (k, v) in zip(descs, self._state.items()):
            d.name = k.encode()
            d.data = v.ctypes.data
            d.numel = v.size
        return descs

    # ---- calls that are the same on a handle of either engine ------------------------------------
    def _profile_end(self, handle: int):
        """[{name, launches, ms, flops, bytes}] per kernel class since mi_profile_begin on `handle` (synchronises)."""
        rows = (_lib.MiProfileRow * 128)()
        n = C.c_int32()
        with torch.cuda.device(self._device):
            _lib.check(_lib.load().mi_profile_end(C.c_void_p(handle), rows, 128, C.byref(n), C.c_void_p(_lib.current_stream_ptr())),
                       "mi_profile_end")
        return [dict(name=r.name.decode(), launches=r.launches, ms=r.ms, flops=r.flops, bytes=r.bytes) for r in rows[:n.value]]

    def _tap(self, entry: str, handle: int, name: str, batch: int) -> torch.Tensor:
        """Copy of an internal activation of the last forward on `handle`, shape (batch, numel); `entry`: the engine's tap entry."""
        fn, h, n = getattr(_lib.load(), entry), C.c_void_p(handle), C.c_int64()
        _lib.check(fn(h, name.encode(), None, batch, C.byref(n), None), entry)
        out = torch.empty(batch, n.value, device=self._device, dtype=torch.float32)
        with torch.cuda.device(self._device):
            _lib.check(fn(h, name.encode(), out.data_ptr(), batch, C.byref(n), C.c_void_p(_lib.current_stream_ptr())), entry)
        return out
