"""Host-side `HTDemucs`: the object `apply_model` drives, backed by the gfx950 engine.

Mirrors the interface the reference's `apply_model` / `Separator` use on a model
(reference: demucs/htdemucs.py:27-133,511-660, demucs/apply.py:233-236,262-264,304-317):
attributes `.sources .samplerate .audio_channels .segment`, `valid_length`, `to`, `eval`,
`load_state_dict` / `state_dict` with the reference's key schema, and `__call__(mix)` mapping
float32 `(B, 2, n <= segment)` on a GPU device to `(B, S, 2, n)`.

The forward is one `mi_model_forward` call into libdemucs_amd.so; there is no PyTorch
implementation of the network in this package and no CPU path.
"""
from __future__ import annotations

import ctypes as C
import random
from fractions import Fraction
from typing import Dict, List, Optional

import torch

from . import _lib
from ._engine_model import EngineModel
from .weights import HTDemucsConfig, check_reference_keyword, htdemucs_schema

__all__ = ["HTDemucs"]


class HTDemucs(EngineModel):
    def __init__(self, sources: List[str], segment=Fraction(39, 5), max_batch: int = 8, compute_dtype: str = "f32", **kwargs):
        cfg = HTDemucsConfig(sources=list(sources), segment=Fraction(segment) if not isinstance(segment, Fraction) else segment)
        for k, v in kwargs.items():            # accept the reference's keyword names, reject other architectures
            if hasattr(cfg, k):
                setattr(cfg, k, v)
            elif not check_reference_keyword(k, v, cfg.depth):    # raises when the value selects another architecture
                raise ValueError(f"unsupported HTDemucs argument {k!r}")
        cfg.validate()
        self.cfg = cfg
        self.sources = list(sources)
        self.samplerate = cfg.samplerate
        self.audio_channels = cfg.audio_channels
        self.segment = cfg.segment
        self.use_train_segment = True
        self.max_batch = int(max_batch)
        self.compute_dtype = self._check_compute_dtype(compute_dtype)
        self._schema = htdemucs_schema(cfg)
        self._state = None                               # key -> float32 array, set by load_state_dict
        self._handles: Dict[torch.device, int] = {}      # engine handle per GPU the model has been used on
        self._device: Optional[torch.device] = None
        self.training = False

    def valid_length(self, length: int) -> int:
        """reference: demucs/htdemucs.py:511-525"""
        training_length = int(self.segment * self.samplerate)
        if training_length < length:
            raise ValueError(f"Given length {length} is longer than training length {training_length}")
        return training_length

    @property
    def segment_length(self) -> int:
        return int(self.segment * self.samplerate)

    # ---- engine handle ------------------------------------------------------------------------
    def _release(self):
        handles, self._handles = self._handles, {}
        for dev, h in handles.items():
            with torch.cuda.device(dev):
                _lib.load().mi_model_destroy(C.c_void_p(h))

    def release(self):
        """Free the packed weights (and, with the last handle of its kind, the shared workspace) on every GPU."""
        self._release()

    def _ensure_handle(self) -> int:
        if self._device in self._handles:
            return self._handles[self._device]
        self._require_runnable()
        descs = self._tensor_descs()
        cfg = _lib.MiConfig(len(self.sources), self.segment_length, self.max_batch, self.COMPUTE_DTYPES[self.compute_dtype])
        h = C.c_void_p()
        with torch.cuda.device(self._device):
            _lib.check(_lib.load().mi_model_create(C.byref(cfg), descs, len(descs), C.byref(h)), "mi_model_create")
        self._handles[self._device] = h.value
        return h.value

    def set_compute_dtype(self, compute_dtype: str):
        if self._check_compute_dtype(compute_dtype) != self.compute_dtype:
            self.compute_dtype = compute_dtype
            self._release()

    def set_max_batch(self, max_batch: int):
        if max_batch != self.max_batch:
            self.max_batch = int(max_batch)
            self._release()

    def device_bytes(self) -> int:
        return int(_lib.load().mi_model_device_bytes(C.c_void_p(self._ensure_handle())))

    def profile_begin(self) -> None:
        _lib.check(_lib.load().mi_profile_begin(C.c_void_p(self._ensure_handle())), "mi_profile_begin")

    def profile_end(self):
        """[{name, launches, ms, flops, bytes}] per kernel class since profile_begin (synchronises)."""
        return self._profile_end(self._ensure_handle())

    def tap(self, name: str, batch: int) -> torch.Tensor:
        """Copy of an internal activation of the last forward (parity tests), shape (batch, numel)."""
        return self._tap("mi_model_tap", self._ensure_handle(), name, batch)

    # ---- forward --------------------------------------------------------------------------------
    def forward_segments(self, mix: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """mix (B, 2, segment_length) float32 on the model device -> (B, S, 2, segment_length).
        No RNG side effect (see __call__)."""
        SL = self.segment_length
        if mix.dim() != 3 or mix.shape[1] != self.audio_channels or mix.shape[2] != SL:
            raise ValueError(f"expected (B, {self.audio_channels}, {SL}), got {tuple(mix.shape)}")
        if mix.dtype != torch.float32:
            raise TypeError("mix must be float32")
        handle = self._ensure_handle()
        if mix.device != self._device:
            raise _lib.EngineError(f"mix is on {mix.device} but the model is on {self._device}")
        mix = mix.contiguous()
        B = mix.shape[0]
        if out is None:
            out = torch.empty(B, len(self.sources), self.audio_channels, SL, device=mix.device, dtype=torch.float32)
        lib = _lib.load()
        with torch.cuda.device(self._device):
            for b0 in range(0, B, self.max_batch):
                nb = min(self.max_batch, B - b0)
                _lib.check(lib.mi_model_forward(C.c_void_p(handle), mix[b0:b0 + nb].data_ptr(), out[b0:b0 + nb].data_ptr(),
                                                nb, C.c_void_p(_lib.current_stream_ptr())), "mi_model_forward")
        return out

    def forward_core(self, mag: Optional[torch.Tensor], mix: torch.Tensor):
        """HTDemucs.forward_core (htdemucs.py:662-759): (spec_out (B,S,4,2048,T), time_out (B,S,2,L)).
        `mag` (B,4,2048,T) is the caller's `_magnitude(_spec(mix))` and feeds the frequency branch as given (the
        fork's ONNX / web tools compute it with their own STFT); None = the engine's own STFT of `mix`."""
        SL = self.segment_length
        if mix.dim() != 3 or mix.shape[1] != self.audio_channels or mix.shape[2] != SL or mix.dtype != torch.float32:
            raise ValueError(f"expected float32 (B, {self.audio_channels}, {SL}), got {tuple(mix.shape)} {mix.dtype}")
        B, S, T = mix.shape[0], len(self.sources), -(-SL // 1024)
        if mag is not None:
            if tuple(mag.shape) != (B, 4, 2048, T) or mag.dtype != torch.float32:
                raise ValueError(f"mag must be float32 (B, 4, 2048, {T}), got {tuple(mag.shape)} {mag.dtype}")
            if mag.device != mix.device:
                raise ValueError("mag and mix must live on the same device")
            mag = mag.contiguous()
        handle = self._ensure_handle()
        if mix.device != self._device:
            raise _lib.EngineError(f"mix is on {mix.device} but the model is on {self._device}")
        mix = mix.contiguous()
        spec = torch.empty(B, S, 4, 2048, T, device=mix.device, dtype=torch.float32)
        tout = torch.empty(B, S, self.audio_channels, SL, device=mix.device, dtype=torch.float32)
        lib = _lib.load()
        with torch.cuda.device(self._device):
            for b0 in range(0, B, self.max_batch):
                nb = min(self.max_batch, B - b0)
                _lib.check(lib.mi_model_forward_core(C.c_void_p(handle), mix[b0:b0 + nb].data_ptr(),
                                                     mag[b0:b0 + nb].data_ptr() if mag is not None else None,
                                                     spec[b0:b0 + nb].data_ptr(), tout[b0:b0 + nb].data_ptr(), nb,
                                                     C.c_void_p(_lib.current_stream_ptr())), "mi_model_forward_core")
        return spec, tout

    def __call__(self, mix: torch.Tensor) -> torch.Tensor:
        """HTDemucs.forward in eval mode (htdemucs.py:527-660): shorter inputs are right-padded with
        zeros to the training length and the output cropped back."""
        random.randrange(1)      # the reference draws its sin-embedding shift from Python's global
        #                          RNG on every forward (transformer.py:680); keep `shifts` offsets in step
        length = mix.shape[-1]
        SL = self.segment_length
        if length > SL:
            raise ValueError(f"Given length {length} is longer than training length {SL}")
        if length < SL:
            mix = torch.nn.functional.pad(mix, (0, SL - length))
        out = self.forward_segments(mix)
        return out[..., :length] if length < SL else out

    forward = __call__
