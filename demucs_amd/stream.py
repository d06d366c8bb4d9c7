"""Streaming scheduler: separate a track that arrives block by block (`apply_model_stream`).

The result contract is the offline call on the whole track: `torch.cat([*pushes, finish], -1)` equals
`apply_model(model, full[None], shifts=..., split=True, overlap=..., transition_power=..., segment=...)[0]` bit for bit, for
every partition of the input into blocks, and `random` ends in the same state.  Four facts make that possible:

  * Every pass (bag member x shift pass) reads the track zero-extended on both sides: `_apply_shifts` pads with zeros and
    `TensorChunk.padded` fills with real neighbours, so a segment's input window is fixed once the input has reached the
    window's end.  A full segment (`n == segment_length`) runs as soon as that happens; a tail segment (`n < segment_length`)
    only at `finish()`, because its `n` and its padding depend on where the track ends.
  * Each accumulator receives its segments in ascending offset order (the float32 summation order of `ola.hip`), and a
    forward's item does not depend on its batch position or on B (tests/test_gpu_many.py), so segments that become ready
    together may share forwards across passes of one model.
  * Position q of a pass is final once every segment with offset <= q has run: later segments start after q.  A push emits
    the track positions below `min over passes of (origin + next offset)`, capped at the pushed total P.  The next offset of
    a pass is the first whose window ends after P, so P - emitted is at most `latency` = max over members of
    `valid - (valid - segment_length) // 2`, minus one, and some push reaches it: `segment_length - 1` samples for the engines,
    whose leaf pads a full segment by nothing (HTDemucs' valid length is its segment length, HDemucs does not pad).  The shift origin does not enter:
    a pass's track position is never ahead of its chunk position.
  * Python's `random` is used in the reference's order.  A later member's or shift pass's `randint` comes after the earlier
    passes' per-segment `randrange(1)` draws, whose number depends on the track length.  With `length=` the stream makes every
    RNG call of the run at construction, as `packed.plan()` does; without it, a run is accepted only if no per-segment draw
    comes before a later `randint` (one model with `shifts <= 1`, or models that draw nothing per segment), the offsets are
    drawn at construction and the engine's per-segment draws are made as segments are dispatched.

Device state does not grow with the stream: an input window from the earliest next segment window on (plus the block being
pushed), one accumulator span per pass covering only what is not yet emitted, and the forward buffers.  One `mi_stream_emit`
launch per push turns the finished spans of every pass into final stems: `out /= sum_weight`, the shift average, the bag
average and optionally the Separator's inverse affine, each a separately rounded float32 operation in the device path's order.

Models that are not the engine's take a plain-torch route with the same scheduler (`apply_model`'s generic route).
"""
from __future__ import annotations

import ctypes as C
import random
from typing import List, Optional

import numpy as np
import torch
from torch.nn import functional as F

from . import _lib
from .hdemucs import HDemucs, MIN_LENGTH as _HDEMUCS_MIN_LENGTH
from .htdemucs import HTDemucs

__all__ = ["apply_model_stream", "ModelStream", "EMIT_PASS_COLS"]

# column layout of mi_stream_emit's pass table (include/demucs_amd.h, MI_EMIT_*)
EMIT_PASS_COLS = 8
TILE_COLS, TILE_SPAN = 7, 1024                 # packed tile table (MI_PACK_*)


def apply_model_stream(model, shifts: int = 1, overlap: float = 0.25, transition_power: float = 1.0, segment=None,
                       device=None, length: Optional[int] = None, split: bool = True, progress: bool = False,
                       callback=None) -> "ModelStream":
    """Start a stream; see the module docstring.  `st.push(block)` takes (channels, n) float32 on the host or a device and
    returns the newly final stems (S, channels, m); `st.finish()` returns the rest.  `device` defaults to the first block's."""
    return ModelStream(model, shifts=shifts, overlap=overlap, transition_power=transition_power, segment=segment, device=device,
                       length=length, split=split, progress=progress, callback=callback)


class _Member:
    def __init__(self, model, overlap, segment, transition_power):
        from .apply import _leaf_valid_length, _segment_plan
        from .distributed import rng_draws_per_forward
        self.model = model
        self.kind = "ht" if isinstance(model, HTDemucs) else "h" if isinstance(model, HDemucs) else "generic"
        _, self.SL, self.stride, _ = _segment_plan(model, 1, overlap, segment)
        if self.stride <= 0:
            raise ValueError(f"overlap {overlap} leaves no stride for a segment of {self.SL} samples")
        if self.kind == "ht":
            self.V = _leaf_valid_length(model, self.SL, segment)
        elif self.kind == "h":
            self.V = self.SL
        else:
            self.V = self.valid(self.SL)
        self.padl = (self.V - self.SL) // 2           # left padding of a full segment's window
        # left padding of any segment's window (a tail is padded more); a generic model's valid length must not grow as n shrinks
        self.reach = 0 if self.kind == "h" else max(self.padl, (self.V - 1) // 2)
        self.draws = rng_draws_per_forward(model)
        self.max_shift = int(0.5 * model.samplerate)
        self.rows = len(model.sources) * model.audio_channels
        self.transition_power = transition_power

    def valid(self, n: int) -> int:
        """Window length of a segment of n samples (apply._apply_leaf)."""
        if self.kind == "ht":
            return self.V
        if self.kind == "h":
            return n
        return self.model.valid_length(n) if hasattr(self.model, "valid_length") else n


class _Pass:
    def __init__(self, member: int, shift: Optional[int], origin: int):
        self.member, self.shift, self.origin = member, shift, origin       # chunk position q is track position origin + q
        self.k = 0                                                          # index of the next segment to dispatch
        self.a0 = 0                                                         # chunk position of accumulator sample 0
        self.hi = 0                                                         # end of the accumulated span (chunk positions)


class ModelStream:
    """One stream.  Attributes: `emitted` (samples returned so far), `pushed`, `latency` (see the module docstring)."""

    def __init__(self, model, shifts=1, overlap=0.25, transition_power=1.0, segment=None, device=None, length=None,
                 split=True, progress=False, callback=None, affine=None):
        from .apply import BagOfModels
        from . import distributed
        if not split:
            raise ValueError("apply_model_stream: split=False needs the whole track (one forward over it)")
        if callback is not None or progress:
            raise ValueError("apply_model_stream: callbacks and progress bars are not supported on a stream")
        if distributed.sharding_active():
            raise ValueError("apply_model_stream: multi-GPU sharding is not supported on a stream")
        assert transition_power >= 1, "transition_power < 1 leads to weird behavior."
        if length is not None and int(length) < 0:
            raise ValueError(f"length must be >= 0, got {length}")
        if isinstance(model, BagOfModels):
            models, self.bag_weights = list(model.models), [list(w) for w in model.weights]
        else:
            models, self.bag_weights = [model], None
        self.members = [_Member(m, overlap, segment, transition_power) for m in models]
        self.sources = list(models[0].sources)
        self.audio_channels = models[0].audio_channels
        self.samplerate = models[0].samplerate
        self.shifts = int(shifts)
        self.length = None if length is None else int(length)
        self.device = None if device is None else torch.device(device)
        self.latency = max(m.V - m.padl for m in self.members) - 1
        self.pushed = 0
        self.emitted = 0
        self.finished = False
        self._exec = None
        self._out_device = None
        # Separator.separate_stream: blocks are normalised `(x - mean) / s` and stems restored `x * s + mean`, s = std + 1e-8
        self.affine = None
        if affine is not None:
            mean, std = (float(v) for v in affine)
            self.affine = (float(np.float32(mean)), float(np.float32(std) + np.float32(1e-8)))

        n_passes = max(1, self.shifts)
        drawing = [m.draws > 0 for m in self.members for _ in range(n_passes)]
        if self.length is None and self.shifts and any(drawing[:-1]):
            raise ValueError("apply_model_stream: this run draws from `random` per segment before a later shift offset, and how "
                             "many draws depends on the track length: pass length= (the total number of samples)")
        # every RNG call that can be made now, in the reference's order (member, shift pass, segments)
        self.predrawn = self.length is not None
        self.passes: List[_Pass] = []
        for e, m in enumerate(self.members):
            for _ in range(n_passes):
                if self.shifts:
                    shift = random.randint(0, m.max_shift)
                    origin = shift - m.max_shift
                else:
                    shift, origin = None, 0
                self.passes.append(_Pass(e, shift, origin))
                if self.predrawn and m.draws:
                    plen = self.length - origin
                    for _ in range(m.draws * len(range(0, plen, m.stride))):
                        random.randrange(1)

    # ---- scheduling (device independent) ------------------------------------------------------------------------------
    def _ready(self, final: bool):
        """Dispatch list [(pass index, offset, n)]: pass by pass, offsets ascending.  Advances each pass's next segment."""
        out = []
        P = self.pushed
        for pi, ps in enumerate(self.passes):
            m = self.members[ps.member]
            while True:
                o = ps.k * m.stride
                if final:
                    plen = P - ps.origin
                    if o >= plen:
                        break
                    n = min(plen - o, m.SL)
                elif ps.origin + o - m.padl + m.V <= P:
                    n = m.SL
                else:
                    break
                out.append((pi, o, n))
                ps.k += 1
        return out

    def _emit_limit(self) -> int:
        if self.finished:
            return self.pushed
        lim = min(ps.origin + ps.k * self.members[ps.member].stride for ps in self.passes)
        return max(self.emitted, min(self.pushed, lim))

    def _keep_from(self) -> int:
        """First track position a segment still to be dispatched can read."""
        lo = min(ps.origin + ps.k * self.members[ps.member].stride - self.members[ps.member].reach for ps in self.passes)
        return max(0, min(self.pushed, lo))

    def _segments_covering(self, ps: _Pass, q0: int, q1: int):
        """(offset, n) of the pass's segments that touch chunk positions [q0, q1), ascending (all of them dispatched)."""
        m = self.members[ps.member]
        j0 = max(0, -(-(q0 - m.SL + 1) // m.stride))
        j1 = (q1 - 1) // m.stride
        plen = self.pushed - ps.origin if self.finished else None
        segs = []
        for j in range(j0, min(j1, ps.k - 1) + 1):
            o = j * m.stride
            segs.append((o, m.SL if plen is None else min(plen - o, m.SL)))
        return segs

    def _dispatch_draw(self, m: _Member, count: int) -> None:
        """The engine's per-segment `randrange(1)` (apply.device_split_accumulate), when not drawn at construction."""
        if not self.predrawn and m.kind == "ht":
            for _ in range(count):
                random.randrange(1)

    # ---- public --------------------------------------------------------------------------------------------------------
    def push(self, block: torch.Tensor) -> torch.Tensor:
        if self.finished:
            raise RuntimeError("push after finish()")
        if block.dim() != 2 or block.shape[0] != self.audio_channels:
            raise ValueError(f"expected a ({self.audio_channels}, n) block, got {tuple(block.shape)}: a stream converts no "
                             "channel layout")
        if self.length is not None and self.pushed + block.shape[1] > self.length:
            raise ValueError(f"pushed {self.pushed + block.shape[1]} samples, more than the declared length {self.length}")
        self._start(block.device)
        self._out_device = block.device
        return self._exec.push(block)

    def finish(self) -> torch.Tensor:
        if self.finished:
            raise RuntimeError("finish() called twice")
        if self.length is not None and self.pushed != self.length:
            raise ValueError(f"the stream ended after {self.pushed} samples, but length={self.length} was declared")
        if self.pushed == 0:
            raise ValueError("the stream ended before any sample was pushed")
        self._start(self._out_device)
        return self._exec.finish()

    def device_bytes(self) -> int:
        """Bytes of device memory the stream itself holds (input window, accumulators, forward buffers); the models' weights and
        workspaces are counted by `model.device_bytes()`."""
        return 0 if self._exec is None else self._exec.device_bytes()

    def _start(self, block_device) -> None:
        if self._exec is not None:
            return
        device = self.device if self.device is not None else torch.device(block_device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        self.device = device
        engine = [m.kind != "generic" for m in self.members]
        if all(engine):
            if device.type != "cuda":
                raise ValueError("apply_model_stream: HTDemucs / HDemucs engines run on a GPU device")
            self._exec = _EngineExec(self)
        else:
            self._exec = _TorchExec(self)

    def _result(self, out: torch.Tensor) -> torch.Tensor:
        dev = self._out_device
        if dev is None or out.device == torch.device(dev):
            return out
        return out.to(dev)


# ------------------------------------------------------------------------------------------------------------------------
# plain-torch route (models that are not the engine's): apply._apply_split / _apply_leaf / _apply_shifts / _apply_bag ops
# ------------------------------------------------------------------------------------------------------------------------
class _TorchExec:
    def __init__(self, st: ModelStream):
        from .apply import _model_device, _transition_weight
        self.st = st
        dev = st.device
        self.homes = []
        for m in st.members:
            self.homes.append(_model_device(m.model))
            m.model.to(dev)
            m.model.eval()
        self.weights = [_transition_weight(m.SL, m.transition_power, dev) for m in st.members]
        C_, S = st.audio_channels, len(st.sources)
        self.win = torch.zeros(C_, 0, device=dev)
        self.win0 = 0
        self.acc = [torch.zeros(S, C_, 0, device=dev) for _ in st.passes]
        self.sw = [torch.zeros(0, device=dev) for _ in st.passes]

    def device_bytes(self) -> int:
        if self.st.device.type != "cuda":
            return 0
        return sum(t.numel() * t.element_size() for t in [self.win, *self.acc, *self.sw])

    def _append(self, block):
        st = self.st
        keep = st._keep_from()
        blk = block.to(device=st.device, dtype=torch.float32)
        if st.affine is not None:
            mean, s = (torch.tensor(v, dtype=torch.float32, device=st.device) for v in st.affine)
            blk = (blk - mean) / s
        self.win = torch.cat([self.win[:, keep - self.win0:], blk], 1)
        self.win0 = keep
        st.pushed += block.shape[1]

    def _window(self, start: int, V: int) -> torch.Tensor:
        lo, hi = start - self.win0, start - self.win0 + V
        a, b = max(0, lo), min(self.win.shape[1], hi)
        return F.pad(self.win[:, a:max(a, b)], (a - lo, hi - max(a, b)))[None]

    def _run(self, units):
        from .apply import center_trim
        st = self.st
        for pi, o, n in units:
            ps = st.passes[pi]
            m = st.members[ps.member]
            V = m.valid(n)
            padded = self._window(ps.origin + o - (V - n) // 2, V)
            state = random.getstate() if st.predrawn else None        # the run's draws were made at construction
            with torch.no_grad():
                out = m.model(padded)
            if state is not None:
                random.setstate(state)
            chunk_out = center_trim(out, n)[0]
            end = o + n - ps.a0
            if end > self.acc[pi].shape[-1]:
                grow = end - self.acc[pi].shape[-1]
                self.acc[pi] = torch.cat([self.acc[pi], self.acc[pi].new_zeros(*self.acc[pi].shape[:-1], grow)], -1)
                self.sw[pi] = torch.cat([self.sw[pi], self.sw[pi].new_zeros(grow)])
            # positions before a0 lie before the track (a shift pass's lead-in) and are never emitted: only the rest is added
            j = max(0, ps.a0 - o)
            if j >= n:
                continue
            w = self.weights[ps.member]
            self.acc[pi][..., o + j - ps.a0:end] += (w[j:n] * chunk_out[..., j:]).to(self.acc[pi].device)
            self.sw[pi][o + j - ps.a0:end] += w[j:n].to(self.sw[pi].device)

    def _emit(self, t1: int) -> torch.Tensor:
        st = self.st
        t0 = st.emitted
        member_out = []
        for e, m in enumerate(st.members):
            out = None
            for pi, ps in enumerate(st.passes):
                if ps.member != e:
                    continue
                q0, q1 = t0 - ps.origin - ps.a0, t1 - ps.origin - ps.a0
                piece = self.acc[pi][..., q0:q1] / self.sw[pi][q0:q1]
                out = piece.clone() if out is None else out.add_(piece)
            if st.shifts:
                out /= st.shifts
            member_out.append(out)
        if st.bag_weights is None:
            res = member_out[0]
        else:
            totals = [0.0] * len(st.sources)
            res = None
            for out, sub_weights in zip(member_out, st.bag_weights):
                for k, w in enumerate(sub_weights):
                    out[k, :, :] *= w
                    totals[k] += w
                res = out if res is None else res.add_(out)
            for k in range(res.shape[0]):
                res[k, :, :] /= totals[k]
        if st.affine is not None:
            mean, s = (torch.tensor(v, dtype=torch.float32, device=res.device) for v in st.affine)
            res = res * s + mean
        # drop what is emitted
        for pi, ps in enumerate(st.passes):
            cut = max(0, t1 - ps.origin - ps.a0)
            self.acc[pi] = self.acc[pi][..., cut:].clone()
            self.sw[pi] = self.sw[pi][cut:].clone()
            ps.a0 += cut
        st.emitted = t1
        return st._result(res)

    def push(self, block):
        st = self.st
        self._append(block)
        self._run(st._ready(final=False))
        return self._emit(st._emit_limit())

    def finish(self):
        st = self.st
        st.finished = True
        self._run(st._ready(final=True))
        res = self._emit(st.pushed)
        for m, home in zip(st.members, self.homes):
            if home is not None and st.bag_weights is not None:
                m.model.to(home)
        return res


# ------------------------------------------------------------------------------------------------------------------------
# engine route: packed gather / overlap-add kernels, one mi_stream_emit launch per push
# ------------------------------------------------------------------------------------------------------------------------
def _upload(values, dtype, dev) -> torch.Tensor:
    return torch.tensor(values, dtype=dtype).to(dev)


def emit_scales(shifts: int, n_members: int, bag_weights, n_sources: int) -> List[float]:
    """mi_stream_emit's float table: per member [1 / shifts, w[m][0..S-1]], then [1 / totals[k]].  Each is the float32 factor
    torch's CUDA kernels apply for a host scalar: `x *= w` multiplies by float32(w), and `x /= s` multiplies by the float32
    rounding of the reciprocal taken in double, 1 / s (checked on torch 2.10 for ROCm: not 1.0f / float32(s), not a division).
    The bag's totals are summed in double on the host first, as apply._apply_bag does."""
    inv_shifts = float(np.float32(1.0 / shifts)) if shifts else 1.0
    vals = []
    totals = [0.0] * n_sources
    for e in range(n_members):
        ws = bag_weights[e] if bag_weights is not None else [1.0] * n_sources
        vals.append(inv_shifts)
        for k, w in enumerate(ws):
            vals.append(float(np.float32(w)))
            totals[k] += w
    vals += [float(np.float32(1.0 / t)) if t else float("inf") for t in totals]
    return vals


class _EngineExec:
    def __init__(self, st: ModelStream):
        from .apply import _model_device, _transition_weight
        self.st = st
        dev = st.device
        self.lib = _lib.load()
        self.homes = []
        for m in st.members:
            self.homes.append(_model_device(m.model))
            m.model.to(dev)
            m.model.eval()
        with torch.cuda.device(dev):
            ramps = [_transition_weight(m.SL, m.transition_power, dev).to(torch.float32) for m in st.members]
            self.w_offs = [sum(r.numel() for r in ramps[:e]) for e in range(len(ramps))]
            self.weights = torch.cat(ramps).contiguous()
            self.scales = _upload(emit_scales(st.shifts, len(st.members), st.bag_weights, len(st.sources)), torch.float32, dev)
            # (2,) float32 [mean, std + 1e-8] of the Separator's affine (mi_track_affine's stats)
            self.stats = None if st.affine is None else _upload(list(st.affine), torch.float32, dev)
            self.win = torch.zeros(st.audio_channels, 0, device=dev)
            self.acc = torch.zeros(0, device=dev)
        self.win0 = 0
        self.bases = [0] * len(st.passes)
        self.bufs = {}

    def device_bytes(self) -> int:
        n = self.win.numel() + self.acc.numel() + sum(t.numel() for b in self.bufs.values() for t in set(b))
        return 4 * n

    def _stream(self):
        return C.c_void_p(_lib.current_stream_ptr())

    def _append(self, block):
        st = self.st
        keep = st._keep_from()
        blk = block.to(device=st.device, dtype=torch.float32, copy=self.stats is not None).contiguous()
        if self.stats is not None and blk.numel():
            _lib.check(self.lib.mi_track_affine(blk.data_ptr(), blk.numel(), self.stats.data_ptr(), 0, self._stream()),
                       "mi_track_affine")
        self.win = torch.cat([self.win[:, keep - self.win0:], blk], 1).contiguous()
        self.win0 = keep
        st.pushed += block.shape[1]

    def _relayout(self, units):
        """One buffer for every pass's span [emitted - origin, hi): the emitted prefix dropped, room for `units` added."""
        st = self.st
        rows = [st.members[ps.member].rows for ps in st.passes]
        new_hi = [ps.hi for ps in st.passes]
        for pi, o, n in units:
            new_hi[pi] = max(new_hi[pi], o + n)
        spans = []
        for pi, ps in enumerate(st.passes):
            a0 = st.emitted - ps.origin
            spans.append((a0, max(a0, new_hi[pi])))
        same = all(a0 == ps.a0 and hi == ps.hi for (a0, hi), ps in zip(spans, st.passes))
        if same:
            return
        bases, total = [], 0
        for (a0, hi), r in zip(spans, rows):
            bases.append(total)
            total += r * (hi - a0)
        acc = torch.zeros(total, device=st.device, dtype=torch.float32)
        for pi, ps in enumerate(st.passes):
            a0, hi = spans[pi]
            live = ps.hi - a0
            if live > 0:
                old = self.acc[self.bases[pi]:self.bases[pi] + rows[pi] * (ps.hi - ps.a0)].view(rows[pi], ps.hi - ps.a0)
                acc[bases[pi]:bases[pi] + rows[pi] * (hi - a0)].view(rows[pi], hi - a0)[:, :live] = old[:, a0 - ps.a0:]
            ps.a0, ps.hi = a0, hi
        self.acc, self.bases = acc, bases

    def _tables(self, fw_units, valid):
        st = self.st
        items, tiles, groups = [], [], []
        W = self.win.shape[1]
        for k, (pi, o, n) in enumerate(fw_units):
            ps = st.passes[pi]
            m = st.members[ps.member]
            trim = (valid - n) // 2 if m.kind == "ht" else 0
            items += [0, W, ps.origin + o - trim - self.win0, self.bases[pi], ps.hi - ps.a0, o - ps.a0, n, trim]
            if groups and groups[-1][0] == pi:
                groups[-1][2] = k + 1
            else:
                groups.append([pi, k, k + 1])
        for pi, i0, i1 in groups:
            ps = st.passes[pi]
            us = fw_units[i0:i1]
            acc_len = ps.hi - ps.a0
            lo = max(0, min(o - ps.a0 for _, o, _ in us))
            hi = min(acc_len, max(o + n - ps.a0 for _, o, n in us))
            e = ps.member
            for pos in range(lo, hi, TILE_SPAN):
                tiles += [self.bases[pi], acc_len, pos, i0, i1, self.w_offs[e], st.members[e].SL]
        return items, tiles

    def _forward(self, e: int, fw_units, valid: int, keep: list):
        st = self.st
        m = st.members[e]
        sub = m.model
        dev = st.device
        nb = len(fw_units)
        channels = st.audio_channels
        items, tiles = self._tables(fw_units, valid)
        table = _upload(items + tiles, torch.int64, dev)
        keep.append(table)

        def gather(seg):
            _lib.check(self.lib.mi_segments_gather_packed(self.win.data_ptr(), self.win.numel(), channels, C.c_void_p(table.data_ptr()),
                                                          nb, valid, seg.data_ptr(), seg.numel(), self._stream()),
                       "mi_segments_gather_packed")

        if m.kind == "ht":
            SL = sub.segment_length
            if e not in self.bufs:
                B = sub.max_batch
                seg_buf = torch.zeros(B, channels, SL, device=dev, dtype=torch.float32)
                cut_buf = torch.empty(B, channels, valid, device=dev, dtype=torch.float32) if valid < SL else seg_buf
                self.bufs[e] = (seg_buf, cut_buf, torch.empty(B, len(sub.sources), channels, SL, device=dev, dtype=torch.float32))
            seg_buf, cut_buf, out_buf = self.bufs[e]
            gather(cut_buf[:nb])
            if valid < SL:
                seg_buf[:nb, :, :valid] = cut_buf[:nb]          # right zero padding, as HTDemucs.forward
            out = out_buf[:nb]
            sub.forward_segments(seg_buf[:nb], out)
            out_valid = SL
            self.st._dispatch_draw(m, nb)
        else:
            seg = torch.empty(nb, channels, valid, device=dev, dtype=torch.float32)
            gather(seg)
            side = nb == 1 and valid < m.SL and valid >= _HDEMUCS_MIN_LENGTH     # a lone tail: the single-item side engine
            out = sub(seg, aux=True) if side else sub(seg)
            out_valid = valid
            keep.append(out)
        if tiles:
            t_items = table.data_ptr()
            _lib.check(self.lib.mi_ola_accumulate_packed(self.acc.data_ptr(), self.acc.numel(), m.rows, out.data_ptr(), out_valid,
                                                         out.numel(), C.c_void_p(t_items), nb, C.c_void_p(t_items + 8 * len(items)),
                                                         len(tiles) // TILE_COLS, self.weights.data_ptr(), self.weights.numel(),
                                                         self._stream()), "mi_ola_accumulate_packed")

    def _run(self, units, keep):
        st = self.st
        for e, m in enumerate(st.members):
            mine = [u for u in units if st.passes[u[0]].member == e]
            if not mine:
                continue
            B = m.model.max_batch
            if m.kind == "ht":
                for i in range(0, len(mine), B):
                    self._forward(e, mine[i:i + B], m.V, keep)
                continue
            # HDemucs: one chunk length per forward; lengths never grow along a pass, so descending length order keeps every
            # accumulator's segments ascending (full chunks first, then each tail length on its own)
            for n in sorted({u[2] for u in mine}, reverse=True):
                same = [u for u in mine if u[2] == n]
                for i in range(0, len(same), B):
                    self._forward(e, same[i:i + B], n, keep)

    def _emit(self, t1: int, keep) -> torch.Tensor:
        st = self.st
        t0 = st.emitted
        S, channels = len(st.sources), st.audio_channels
        out = torch.empty(S, channels, t1 - t0, device=st.device, dtype=torch.float32)
        if t1 > t0:
            passes, segs = [], []
            for pi, ps in enumerate(st.passes):
                q0, q1 = t0 - ps.origin, t1 - ps.origin
                s_lo = len(segs) // 2
                for o, n in st._segments_covering(ps, q0, q1):
                    segs += [o - ps.a0, n]
                e = ps.member
                passes += [self.bases[pi], ps.hi - ps.a0, q0 - ps.a0, s_lo, len(segs) // 2, self.w_offs[e], st.members[e].SL, e]
            t_passes = _upload(passes, torch.int64, st.device)
            t_segs = _upload(segs or [0, 0], torch.int64, st.device)
            keep += [t_passes, t_segs]
            _lib.check(self.lib.mi_stream_emit(self.acc.data_ptr(), self.acc.numel(), S, channels, t_passes.data_ptr(),
                                               len(st.passes), t_segs.data_ptr(), len(segs) // 2, self.weights.data_ptr(),
                                               self.weights.numel(), self.scales.data_ptr(), len(st.members), st.shifts,
                                               int(st.bag_weights is not None),
                                               self.stats.data_ptr() if self.stats is not None else None,
                                               t1 - t0, out.data_ptr(), out.numel(), self._stream()), "mi_stream_emit")
        st.emitted = t1
        return out

    def _host(self, out: torch.Tensor) -> torch.Tensor:
        dev = self.st._out_device
        if dev is None or torch.device(dev).type != "cpu":
            return self.st._result(out)
        host = torch.empty(out.shape, dtype=torch.float32, pin_memory=True)
        host.copy_(out, non_blocking=True)
        torch.cuda.current_stream(self.st.device).synchronize()
        return host

    def push(self, block):
        st = self.st
        keep = []
        with torch.cuda.device(st.device):
            self._append(block)
            units = st._ready(final=False)
            self._relayout(units)
            self._run(units, keep)
            out = self._emit(st._emit_limit(), keep)
            return self._host(out)

    def finish(self):
        st = self.st
        keep = []
        with torch.cuda.device(st.device):
            st.finished = True
            units = st._ready(final=True)
            self._relayout(units)
            self._run(units, keep)
            out = self._emit(st.pushed, keep)
            for m in st.members:
                if m.kind == "h":
                    m.model.check()          # a time-out of the LAST forward's recurrence would otherwise pass unnoticed
            for m, home in zip(st.members, self.homes):
                if home is not None and st.bag_weights is not None:
                    m.model.to(home)
            return self._host(out)
