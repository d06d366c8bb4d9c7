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
import weakref
from typing import List, Optional

import numpy as np
import torch
from torch.nn import functional as F

from . import _lib
from .hdemucs import HDemucs, MIN_LENGTH as _HDEMUCS_MIN_LENGTH
from .htdemucs import HTDemucs

__all__ = ["apply_model_stream", "apply_model_stream_group", "ModelStream", "StreamGroup", "Delivery", "EMIT_PASS_COLS"]

# column layout of mi_stream_emit's pass table (include/demucs_amd.h, MI_EMIT_*)
EMIT_PASS_COLS = 8
TILE_COLS, TILE_SPAN = 7, 1024                 # packed tile table (MI_PACK_*)


class Delivery:
    """How a stream hands its stems over (`audio.deliver`'s arguments): with one, `push` / `finish` return `{name: (m, channels)
    frames}` -- every source, or with `stem` the `--two-stems` outputs -- after `prevent_clip(·, clip)`, as int16 PCM ("i16") or
    float32 ("f32") with the channels interleaved per frame, instead of the float32 (S, channels, m) stems.

    `samplerate=R` delivers at R Hz instead of the model's M: the frames are those of `prevent_clip(resample_frac(v, M, R), clip)`
    per output value v, i.e. `audio.deliver(..., samplerate=(M, R))` on the whole track, bit for bit for every partition of the
    input.  A resampler frame is final once the stream has emitted its last tap, so after `emitted` model-rate samples
    `ConvertPlan(M, R).ready(emitted)` frames have been returned (`stream.delivered`), at most `stream.output_hold` fewer than
    floor(new * emitted / old); `finish()` returns the rest, floor(new * L / old) in all.  None, or the model's own rate, changes
    nothing.

    `clip="rescale"` (the reference's default, `v / max(1.01 * peak, 1)` with the whole output's peak) takes two passes over the
    same stream.  `peaks="measure"` is the first: `push` returns `{}` (no frames are made and nothing is copied to the host), the
    device keeps `max |value|` per output (4 bytes each), and `finish()` returns them as an `audio.TrackPeaks`.
    `peaks=<TrackPeaks>` is the second: the frames are divided by those peaks.  The forwards are deterministic, so with the same
    input, the same arguments and `random` in the same state both passes see the same values, the peaks are the whole track's and
    the frames equal `audio.deliver(..., clip="rescale")` on it bit for bit (`Separator.separate_blocks` does all of this).  A
    `TrackPeaks` made by hand (an upper bound of a live feed's peak) gives a fixed gain of the same shape in one pass.

    `mix={output name: {"mix" | source name: gain}}` delivers gain-weighted remixes instead of the reference's outputs: vocals
    lowered by 12 dB rather than removed (`{"practice": {"mix": 1, "vocals": 10 ** -0.6 - 1}}`), drums raised, or `{"minus_vocals":
    {"mix": 1, "vocals": -1}}`, the reference's "minus" residual.  The frames equal `audio.deliver_mix(origin, stems, mix, ...)` on
    the whole track bit for bit, `origin` being the mix as `Separator.separate_tensor` hands back a device mix.  "mix" is the
    stream's own input: its window still holds every position that is being emitted, so no copy is kept for it.  `mix` goes with
    `stem=None`, the default `other_method` and the model's sample rate only.

    The gains are `mix`'s until a change takes effect.  `changes={output name: [(at, ramp, {"mix" | source name: gain}), ...]}` is
    a schedule known when the stream opens (`audio.mix_changes`): from delivered frame `at` the output's gains move to the named
    ones over `ramp` frames, linearly and in float32 (`ramp=0`: a step; all gains 0: a fade to silence).  `change_mix` on the open
    stream appends further changes.  Either way the frames equal `audio.deliver_mix(..., changes=)` on the whole track bit for bit.
    A stream with changes does not deliver with `clip="rescale"`: a `TrackPeaks` carries no schedule."""

    def __init__(self, stem=None, other_method: str = "add", clip="clamp", fmt: str = "i16", samplerate=None, peaks=None, mix=None,
                 changes=None):
        from .audio import TrackPeaks, clip_code, deliver_layout, mix_changes, mix_gains
        if other_method not in ("add", "minus", "none"):
            raise ValueError(f"Invalid other_method {other_method}")
        if mix is not None:
            if stem is not None or other_method != "add":
                raise ValueError("mix= names every output by its gains: it goes with stem=None and the default other_method, got "
                                 f"stem={stem!r}, other_method={other_method!r}")
            if samplerate is not None:
                raise ValueError(f"mix= delivers at the model's sample rate only, got samplerate={samplerate!r}: resample the "
                                 "remixed frames, or deliver the stems at that rate and remix them")
            named = mix_gains(mix)                              # what can be refused before the sources are known
            mix = {name: dict(gains) for name, gains in mix.items()}
            changes = mix_changes(changes, named) or None       # ordered; the terms are checked once the sources are known
        elif changes:
            raise ValueError(f"changes= moves the gains of mix= outputs: it goes with mix=, got changes={changes!r} without it")
        self.mix, self.changes = mix, changes or None
        self.stem, self.other_method, self.clip, self.fmt = stem, other_method, clip, fmt
        if samplerate is not None and (int(samplerate) != samplerate or samplerate <= 0):
            raise ValueError(f"the delivered sample rate must be a positive integer, got {samplerate}")
        self.samplerate = None if samplerate is None else int(samplerate)
        self.clip_code = clip_code(clip)
        deliver_layout([], 0, 1, fmt)                       # refuses an unknown format
        if peaks is not None:
            if not (isinstance(peaks, TrackPeaks) or (isinstance(peaks, str) and peaks == "measure")):
                raise ValueError(f"peaks must be 'measure', an audio.TrackPeaks or None, got {peaks!r}")
            if clip != "rescale":
                raise ValueError(f"peaks={'measure' if isinstance(peaks, str) else 'TrackPeaks(...)'!r} belongs to clip='rescale': "
                                 f"clip={clip!r} divides by no peak")
        self.peaks = peaks

    @property
    def measures(self) -> bool:
        """A measuring pass: no frames, `finish()` returns the `audio.TrackPeaks`."""
        return isinstance(self.peaks, str)

    def with_peaks(self, peaks) -> "Delivery":
        """The same delivery with other `peaks` (what a measuring pass found, for the delivering pass)."""
        return Delivery(self.stem, self.other_method, self.clip, self.fmt, self.samplerate, peaks, self.mix, self.changes)

    def __repr__(self):
        tail = "" if self.peaks is None else f", peaks={self.peaks!r}"
        tail += "" if self.mix is None else f", mix={self.mix!r}"
        tail += "" if self.changes is None else f", changes={self.changes!r}"
        return (f"Delivery(stem={self.stem!r}, other_method={self.other_method!r}, clip={self.clip!r}, fmt={self.fmt!r}, "
                f"samplerate={self.samplerate!r}{tail})")

    def outputs(self, sources) -> list:
        """[(name, KIND, SEL)] in the reference's save order (`audio.delivery_outputs`)."""
        from .audio import delivery_outputs, mix_gains, mix_outputs
        if self.mix is not None:
            return mix_outputs(mix_gains(self.mix, sources))
        return delivery_outputs(sources, self.stem, self.other_method)

    def rate_plan(self, model_rate: int, channels: int):
        """The `audio.ConvertPlan(model_rate, samplerate)` of a stream that resamples its frames, None when it delivers at the
        model's rate; refuses a rate pair the delivery kernel cannot take."""
        from .audio import delivery_rate_plan
        return delivery_rate_plan(model_rate, self.samplerate, channels)

    def for_stream(self, sources, engine: bool, model_rate=None, channels: int = 2) -> list:
        """The refusals of a delivering stream (no device work, no RNG call) and its outputs."""
        if self.clip == "rescale" and self.changes is not None:
            raise ValueError("a stream with gain changes (changes=) does not deliver with clip='rescale': the peaks of a track "
                             "belong to one schedule of gains and audio.TrackPeaks carries none; use 'clamp', 'tanh' or None, or "
                             "audio.deliver_mix(..., clip='rescale', changes=) on the whole track")
        if self.clip == "rescale" and self.peaks is None:
            raise ValueError("a stream cannot deliver with clip='rescale': the divisor is the whole track's peak per output; use "
                             "'clamp', 'tanh' or None, or measure the peaks in a pass of their own (peaks='measure', then "
                             "peaks=<the TrackPeaks it returned>)")
        if self.stem is not None and self.other_method == "minus":
            raise ValueError("a stream does not deliver other_method='minus'; use 'add' or 'none', or name the residual by its "
                             "gains: mix={'minus_STEM': {'mix': 1, STEM: -1}}")
        outs = self.outputs(sources)
        self.schedule(sources)              # refuses a change that names an unknown term
        if not engine:
            raise ValueError("a delivering stream runs on the GPU engines (HTDemucs / HDemucs on a cuda device); there is no CPU "
                             "implementation of the delivery kernels in this package")
        if model_rate is not None:
            self.rate_plan(model_rate, channels)
        if self.peaks is not None and not self.measures:
            self._check_peaks(outs, model_rate, self.gains(sources))
        return outs

    def gains(self, sources):
        """`mix` resolved against `sources` (`audio.mix_gains`: [(name, (g_mix, g_0 .. g_{S-1}))]), None without `mix`."""
        from .audio import mix_gains
        return None if self.mix is None else mix_gains(self.mix, sources)

    def schedule(self, sources) -> dict:
        """`changes` resolved against `sources` (`audio.mix_changes`: {output: [(at, ramp, (g_mix, g_0 .. g_{S-1}))]}), {} without."""
        from .audio import mix_changes
        return {} if self.changes is None else mix_changes(self.changes, self.gains(sources), sources)

    def _check_peaks(self, outs, model_rate, gains=None) -> None:
        """Refuses a `TrackPeaks` that was measured for other outputs or at another rate than this stream delivers."""
        from .audio import mix_identity
        pk = self.peaks
        names = [name for name, _, _ in outs]
        own_mix = None if gains is None else mix_identity(gains)
        if pk.mix != own_mix:
            raise ValueError(f"the peaks were measured for mix={pk.mix!r}, this stream delivers mix={own_mix!r}: other gains have "
                             "other peaks")
        if list(pk.names) != names:
            raise ValueError(f"the peaks were measured for the outputs {list(pk.names)}, this stream delivers {names}")
        if pk.stem != self.stem or (self.stem is not None and pk.other_method != self.other_method):
            raise ValueError(f"the peaks were measured for stem={pk.stem!r}, other_method={pk.other_method!r}, this stream delivers "
                             f"stem={self.stem!r}, other_method={self.other_method!r}")

        def rate(r):
            return None if r is None or (model_rate is not None and int(r) == int(model_rate)) else int(r)

        if rate(pk.samplerate) != rate(self.samplerate):
            own = "the model's rate"
            raise ValueError(f"the peaks were measured at {pk.samplerate or own} (Hz), this stream delivers at "
                             f"{self.samplerate or own}: a resampled output has another peak")


def _deliver_rows(outputs, dl: Delivery, src: int, n: int, offs, slot0: int = 0) -> list:
    """mi_deliver_pcm's rows (MI_DELIVER_*) for one stream's outputs on a push: `n` frames of the stems at device address `src`.
    Output i of a rescaling stream names peak slot `slot0 + i`; a measuring stream's rows are mi_deliver_peaks_update's, which
    reads no destination (`offs` None)."""
    from .audio import _FORMATS
    rows = []
    for i, (_, kind, sel) in enumerate(outputs):
        rows += [src, 0, n, kind, sel, dl.clip_code, slot0 + i if dl.peaks is not None else 0, _FORMATS[dl.fmt][0],
                 0 if offs is None else offs[i]]
    return rows


def _mix_rows(st: "ModelStream", src: int, n: int, t0: int, win: int, win0: int, pitch: int, offs, slot0: int = 0) -> list:
    """mi_deliver_mix_pcm's rows (MI_MIX_*) for one stream's remixes on a push: `n` frames from track position `t0` of the stems at
    device address `src`.  The mix is read from the stream's input window, (channels, pitch) floats at device address `win` whose
    column 0 is track position `win0`: the window is trimmed to `_keep_from()` taken before the call dispatched, which no emit
    point is behind, so it still holds [t0, t0 + n).  A stream with an affine keeps it normalised; the row carries (mean, s)."""
    from .audio import mix_rows
    origin = 0
    if any(g[0] != 0 for _, g in st.gains):
        assert win0 <= t0, f"the window starts at {win0}, past the emit point {t0}"
        origin = win + 4 * (t0 - win0)
    return mix_rows(st.gains, src, n, origin, pitch, st.affine, st.deliver.clip_code, slot0, st.deliver.fmt, offs)


def _auto_rows(st: "ModelStream", src: int, n: int, t0: int, win: int, win0: int, pitch: int, offs, slot0: int = 0):
    """`_mix_rows`' sibling for a stream whose gains change (`st.schedule`): `(rows, changes)` for `audio.auto_table`, one entry per
    remix.  The rows are `_mix_rows`' with the gains in force before the changes that reach into [t0, t0 + n), `changes` those
    changes (`audio.auto_span`): a call passes no change that lies wholly behind or ahead of it.  Changes that are behind leave the
    schedule for good and their gains become the output's base.  The mix is named when any of the call's gains reads it."""
    from .audio import auto_span, mix_rows
    base, changes = [], []
    for i, (name, _) in enumerate(st.gains):
        gains, listed, done = auto_span(st.auto_base[i], st.schedule[i], t0, n)
        st.auto_base[i] = gains
        del st.schedule[i][:done]
        base.append((name, gains))
        changes.append(listed)
    origin = 0
    if any(g[0] != 0 for _, g in base) or any(g[0] != 0 for listed in changes for _, _, g in listed):
        assert win0 <= t0, f"the window starts at {win0}, past the emit point {t0}"
        origin = win + 4 * (t0 - win0)
    return mix_rows(base, src, n, origin, pitch, st.affine, st.deliver.clip_code, slot0, st.deliver.fmt, offs), changes


def _packed_slots(slots) -> list:
    """int32 peak slots as int64 table entries (two a word, little-endian), so they ride in a call's one table upload."""
    arr = np.zeros(2 * -(-len(slots) // 2), dtype=np.int32)
    arr[:len(slots)] = slots
    return arr.view(np.int64).tolist()


def _track_peaks(st: "ModelStream", bits: torch.Tensor):
    """The `audio.TrackPeaks` of a finished measuring stream from its slots' bits (int32 on the host)."""
    from .audio import TrackPeaks, mix_identity
    dl = st.deliver
    return TrackPeaks([name for name, _, _ in st.outputs], [int(b) & 0xFFFFFFFF for b in bits.tolist()],
                      samplerate=None if st.rate is None else dl.samplerate, stem=dl.stem, other_method=dl.other_method,
                      length=st.emitted, mix=None if st.gains is None else mix_identity(st.gains))


class _Rate:
    """The resampler of one stream that delivers at another rate: its `audio.ConvertPlan(M, R)` and where its carried values
    live -- (outputs, 2 sides, channels, plan.carry) floats from `off` of a history buffer; `side` is the one to read, whose first
    value is model-rate position `h0`."""

    def __init__(self, plan, n_outputs: int, channels: int):
        self.plan, self.n_outputs, self.channels = plan, n_outputs, channels
        self.size = n_outputs * 2 * channels * plan.carry
        self.off = None
        self.side = self.h0 = 0

    def rows(self, outputs, dl: Delivery, src: int, n_in: int, t0: int, final: bool, bank_off: int, offs) -> list:
        """mi_deliver_resample_pcm's rows (MI_RATE_*) for the stream's outputs on a call that emits `n_in` model-rate samples after
        `t0`; flips the history side."""
        from .audio import _FORMATS
        plan = self.plan
        out0, n_out, nxt = plan.step(t0, n_in, final)
        side = self.channels * plan.carry
        rows = []
        for o, ((_, kind, sel), off) in enumerate(zip(outputs, offs)):
            base = self.off + o * 2 * side
            rows += [src if n_in else 0, n_in, t0, kind, sel, dl.clip_code, _FORMATS[dl.fmt][0], plan.old, plan.new, plan.width,
                     bank_off, out0, n_out, t0 + n_in if final else -1, plan.carry, base + self.side * side,
                     base + (1 - self.side) * side, self.h0, nxt, off]
        if not final:
            self.side, self.h0 = 1 - self.side, nxt
        return rows


def apply_model_stream(model, shifts: int = 1, overlap: float = 0.25, transition_power: float = 1.0, segment=None,
                       device=None, length: Optional[int] = None, split: bool = True, progress: bool = False,
                       callback=None, deliver: Optional[Delivery] = None, pcm: Optional[str] = None,
                       channels: Optional[int] = None) -> "ModelStream":
    """Start a stream; see the module docstring.  `st.push(block)` takes (channels, n) float32 on the host or a device and
    returns the newly final stems (S, channels, m); `st.finish()` returns the rest.  `device` defaults to the first block's.
    With `deliver=Delivery(...)` both return `{name: (m, channels) frames}` instead (one more launch per push, `mi_deliver_pcm`
    on the emitted span; host blocks get the frames by one D2H of their bytes and no float stems leave the device).  With
    `Delivery(samplerate=R)` the frames are at R Hz (`mi_deliver_resample_pcm` in that launch's place).  With
    `Delivery(clip="rescale", peaks="measure")` `push` returns `{}` and `finish()` the `audio.TrackPeaks` (see `Delivery`).

    With `pcm=` ("i16", "i24" or "f32"; `channels=` source channels, the model's by default, or 1 to feed every row) a block is
    wire PCM instead: little-endian frames with the channels interleaved, as a bytes-like object or a 1-D uint8 tensor that may
    end anywhere, or as an (n, channels) int16 / float32 tensor.  The bytes go to the device as they are and `mi_pcm_planar`
    de-interleaves, converts (`v / 32768`, `v / 8388608`: exact) and normalises them there, so the stems are those of the float
    stream fed the same values, bit for bit.  The incomplete last frame of a host chunk waits on the host for the next push
    (`audio.PcmFeed`); `finish()` drops it and `trailing_bytes` counts it.  `length`, `pushed` and `latency` count frames."""
    return ModelStream(model, shifts=shifts, overlap=overlap, transition_power=transition_power, segment=segment, device=device,
                       length=length, split=split, progress=progress, callback=callback, deliver=deliver, pcm=pcm,
                       channels=channels)


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
    """One stream.  Attributes: `emitted` (samples returned so far), `pushed`, `latency` (see the module docstring); with a
    `Delivery(samplerate=R)` also `delivered` (frames at R returned so far) and `output_hold`:
    floor(new * emitted / old) - delivered <= output_hold, and some push reaches it."""

    def __init__(self, model, shifts=1, overlap=0.25, transition_power=1.0, segment=None, device=None, length=None,
                 split=True, progress=False, callback=None, affine=None, deliver=None, pcm=None, channels=None, stats=None):
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
        self.deliver, self.outputs, self.rate = deliver, None, None
        self.delivered = self.output_hold = 0
        self.measure = deliver is not None and deliver.measures      # push returns {}, finish() the audio.TrackPeaks
        self.gains = None                  # a remixing delivery's gains per output (`Delivery.gains`)
        self.peak_off = None               # first of the stream's peak slots in its executor's buffer (a rescaling delivery)
        # gain changes (`Delivery(changes=)`, `change_mix`): per output the changes not yet behind the emit point, the gains in
        # force before them and the end of the last ramp; None until the first change, and the stream's launches are the fixed
        # gains' until then
        self.schedule = self.auto_base = self.auto_end = None
        if deliver is not None:
            engine = all(m.kind != "generic" for m in self.members) and (self.device is None or self.device.type == "cuda")
            self.outputs = deliver.for_stream(self.sources, engine, self.samplerate, self.audio_channels)
            self.gains = deliver.gains(self.sources)
            for name, rows in deliver.schedule(self.sources).items():
                for row in rows:
                    self._add_change([n for n, _ in self.gains].index(name), row)
            plan = deliver.rate_plan(self.samplerate, self.audio_channels)
            if plan is not None:
                self.rate = _Rate(plan, len(self.outputs), self.audio_channels)
                self.output_hold = plan.hold
        # wire PCM blocks (`audio.PcmFeed`): refused here, before any RNG call
        self.feed = None
        if pcm is not None:
            from .audio import PcmFeed, check_pcm, check_stream_channels
            check_pcm(pcm, all(m.kind != "generic" for m in self.members) and (self.device is None or self.device.type == "cuda"))
            self.feed = PcmFeed(pcm, self.audio_channels if channels is None else channels)
            check_stream_channels(self.feed.src_channels, self.audio_channels)
        elif channels is not None and channels != self.audio_channels:
            raise ValueError(f"expected {self.audio_channels} channels, got {channels}: a stream of float blocks converts no "
                             "channel layout")
        # Separator.separate_stream: blocks are normalised `(x - mean) / s` and stems restored `x * s + mean`, s = std + 1e-8;
        # `stats` (an `audio.TrackStats`: what the statistics kernels computed) names mean and s as they are
        self.affine = None
        if stats is not None:
            if affine is not None:
                raise ValueError("give stats, or mean and std, not both: stats already holds the normaliser s = std + 1e-8")
            self.affine = (float(stats.mean), float(stats.s))
        elif affine is not None:
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

    # ---- gain changes ---------------------------------------------------------------------------------------------------
    def _add_change(self, i: int, change) -> None:
        if self.schedule is None:
            self.schedule = [[] for _ in self.gains]
            self.auto_base = [tuple(g) for _, g in self.gains]
            self.auto_end = [0] * len(self.gains)
        self.schedule[i].append(change)
        self.auto_end[i] = change[0] + change[1]

    def change_mix(self, mix, at=None, ramp=0) -> None:
        """Moves the gains of the outputs named in `mix` (`{output name: {"mix" | source name: gain}}`, a term that is not named
        going to 0) to the given ones: from delivered frame `at` (model-rate frames, as `emitted` counts them) over `ramp` frames,
        as a change of `Delivery(changes=)` does.  `at=None` is the earliest position that contradicts nothing: the later of
        `emitted` and the end of the output's last ramp.  What has been delivered stays as it is, so an `at` before `emitted`, or
        before the end of the output's last ramp, is refused, and so is a stream without `Delivery(mix=)`.  Nothing runs on the
        device here; from its first change on the stream's frames come from `mi_deliver_mix_auto_pcm`."""
        from .audio import mix_changes
        if self.gains is None:
            raise ValueError("change_mix: the stream delivers no remix; open it with Delivery(mix=...)")
        if self.finished:
            raise ValueError("change_mix: the stream is finished")
        if self.deliver.clip == "rescale":
            raise ValueError("change_mix: a stream that delivers with clip='rescale' divides by peaks measured for fixed gains; "
                             "audio.TrackPeaks carries no schedule")
        if not isinstance(mix, dict) or not mix:
            raise ValueError(f"change_mix: a non-empty {{output name: {{'mix' | source name: gain}}}} is expected, got {mix!r}")
        names = [name for name, _ in self.gains]
        planned = []
        for name, gains in mix.items():
            end = self.auto_end[names.index(name)] if self.schedule is not None and name in names else 0
            a = max(self.emitted, end) if at is None else at
            change = mix_changes({name: [(a, ramp, gains)]}, self.gains, self.sources)[name][0]
            if a < self.emitted:
                raise ValueError(f"change_mix: at={a} lies before the {self.emitted} frames that were delivered already")
            if a < end:
                raise ValueError(f"change_mix: at={a} lies before {end}, where the last ramp of output {name!r} ends")
            planned.append((names.index(name), change))
        for i, change in planned:           # all of them, or none
            self._add_change(i, change)

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
    @property
    def trailing_bytes(self) -> int:
        """Bytes of an incomplete last frame of a PCM stream: carried to the next push, dropped by `finish()`."""
        return 0 if self.feed is None else self.feed.trailing_bytes

    def push(self, block: torch.Tensor) -> torch.Tensor:
        if self.finished:
            raise RuntimeError("push after finish()")
        if self.feed is not None:
            blk = self.feed.accept(block)
            if self.length is not None and self.pushed + blk.n > self.length:
                raise ValueError(f"pushed {self.pushed + blk.n} samples, more than the declared length {self.length}")
            self._start(blk.device)
            self.feed.commit(blk)
            self._out_device = blk.device
            return self._exec.push(blk)
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
        self.rate_hist = None              # a resampling delivery's carried values (`_Rate`)
        self.peaks = self.slots = None     # a rescaling delivery's peak bits (measured here, or given) and its rows' slots

    def device_bytes(self) -> int:
        n = self.win.numel() + self.acc.numel() + sum(t.numel() for b in self.bufs.values() for t in set(b))
        n += 0 if self.peaks is None else self.peaks.numel() + self.slots.numel()
        return 4 * (n + (0 if self.rate_hist is None else self.rate_hist.numel()))

    def _stream(self):
        return C.c_void_p(_lib.current_stream_ptr())

    def _append(self, block, alive):
        st = self.st
        keep = st._keep_from()
        if st.feed is not None:             # wire PCM: the bytes as they came, then de-interleave / convert / normalise on the device
            from .audio import _pcm_planar
            if block.n:
                blk = _pcm_planar(block.on_device(st.device, alive), block.fmt, block.src_channels, block.n, st.audio_channels,
                                  self.stats)
            else:
                blk = torch.empty(st.audio_channels, 0, device=st.device)
        else:
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
        dl, rt, frames = st.deliver, st.rate, None
        # a resampling delivery returns the frames whose last tap is emitted; its finish() has a tail even when nothing is emitted
        n_frames = t1 - t0 if rt is None else rt.plan.step(t0, t1 - t0, st.finished)[1]
        if t1 > t0 or (rt is not None and n_frames > 0):
            passes, segs = [], []
            for pi, ps in enumerate(st.passes if t1 > t0 else []):
                q0, q1 = t0 - ps.origin, t1 - ps.origin
                s_lo = len(segs) // 2
                for o, n in st._segments_covering(ps, q0, q1):
                    segs += [o - ps.a0, n]
                e = ps.member
                passes += [self.bases[pi], ps.hi - ps.a0, q0 - ps.a0, s_lo, len(segs) // 2, self.w_offs[e], st.members[e].SL, e]
            if dl is not None:              # the delivery rows ride behind the pass table, in its upload
                from .audio import _BankArena, deliver_layout, rate_groups, rate_lds_floats
                offs, total = deliver_layout(st.outputs, n_frames, channels, dl.fmt)
                d_at = len(passes)
                if dl.peaks is not None and self.peaks is None:
                    # a measuring pass's running peaks, zero at the start of the track; a rescaling delivery's peaks as given
                    n_pk = len(st.outputs)
                    self.peaks = torch.zeros(n_pk, dtype=torch.int32, device=st.device) if st.measure else \
                        _upload(list(dl.peaks.bits), torch.int32, st.device)
                    self.slots, st.peak_off = torch.arange(n_pk, dtype=torch.int32, device=st.device), 0
                auto_len = None                 # a stream whose gains change: MI_AUTO_* rows, their changes behind them
                if st.schedule is not None:
                    from .audio import auto_table
                    rows, changes = _auto_rows(st, out.data_ptr(), t1 - t0, t0, self.win.data_ptr(), self.win0, self.win.shape[1],
                                               offs)
                    rows = auto_table(rows, [t0] * len(changes), changes)
                    passes, auto_len = passes + rows, len(rows)
                elif st.gains is not None:
                    passes = passes + _mix_rows(st, out.data_ptr(), t1 - t0, t0, self.win.data_ptr(), self.win0, self.win.shape[1],
                                                None if st.measure else offs)
                elif rt is None:
                    passes = passes + _deliver_rows(st.outputs, dl, out.data_ptr(), t1 - t0, None if st.measure else offs)
                else:
                    arena = _BankArena.get(st.device)
                    if self.rate_hist is None:
                        self.rate_hist, rt.off = torch.zeros(rt.size, device=st.device, dtype=torch.float32), 0
                    passes = passes + rt.rows(st.outputs, dl, out.data_ptr(), t1 - t0, t0, st.finished, arena.offset(rt.plan), offs)
                    total = max(total, 16)                     # a call that only carries values still names a destination
                if not st.measure:          # a measuring pass makes no frames
                    frames = (torch.empty(total, dtype=torch.uint8, device=st.device), offs)
            t_passes = _upload(passes, torch.int64, st.device)
            keep.append(t_passes)
            if t1 > t0:
                t_segs = _upload(segs or [0, 0], torch.int64, st.device)
                keep.append(t_segs)
                _lib.check(self.lib.mi_stream_emit(self.acc.data_ptr(), self.acc.numel(), S, channels, t_passes.data_ptr(),
                                                   len(st.passes), t_segs.data_ptr(), len(segs) // 2, self.weights.data_ptr(),
                                                   self.weights.numel(), self.scales.data_ptr(), len(st.members), st.shifts,
                                                   int(st.bag_weights is not None),
                                                   self.stats.data_ptr() if self.stats is not None else None,
                                                   t1 - t0, out.data_ptr(), out.numel(), self._stream()), "mi_stream_emit")
            pk = (self.peaks.data_ptr(), self.peaks.numel()) if dl is not None and dl.peaks is not None else (None, 0)
            rows_at = C.c_void_p(t_passes.data_ptr() + 8 * d_at) if dl is not None else None
            mixed = "_mix" if st.gains is not None else ""      # remixes: the entries that read MI_MIX_* rows
            if dl is not None and rt is None and st.measure:
                keep.append(out)
                name = f"mi_deliver{mixed}_peaks_update"
                _lib.check(getattr(self.lib, name)(rows_at, len(st.outputs), t1 - t0, S, channels, *pk, self._stream()), name)
            elif dl is not None and rt is None and auto_len is not None:
                keep.append(out)
                _lib.check(self.lib.mi_deliver_mix_auto_pcm(rows_at, auto_len, len(st.outputs), t1 - t0, S, channels, *pk,
                                                            frames[0].data_ptr(), frames[0].numel(), self._stream()),
                           "mi_deliver_mix_auto_pcm")
            elif dl is not None and rt is None:
                keep.append(out)
                name = f"mi_deliver{mixed}_pcm"
                _lib.check(getattr(self.lib, name)(rows_at, len(st.outputs), t1 - t0, S, channels, *pk, frames[0].data_ptr(),
                                                   frames[0].numel(), self._stream()), name)
            elif dl is not None:
                keep.append(out)
                bank, hist = arena.buf, self.rate_hist
                rate_args = (rows_at, len(st.outputs), rate_groups(rt.plan, channels, n_frames), S, channels, bank.data_ptr(),
                             bank.numel(), hist.data_ptr() if hist.numel() else None, hist.numel(), rate_lds_floats(rt.plan, channels))
                if st.measure:
                    _lib.check(self.lib.mi_deliver_resample_peaks(*rate_args, self.slots.data_ptr(), *pk, self._stream()),
                               "mi_deliver_resample_peaks")
                elif dl.peaks is not None:
                    _lib.check(self.lib.mi_deliver_resample_pcm_peaks(*rate_args, frames[0].data_ptr(), frames[0].numel(),
                                                                      self.slots.data_ptr(), *pk, self._stream()),
                               "mi_deliver_resample_pcm_peaks")
                else:
                    _lib.check(self.lib.mi_deliver_resample_pcm(*rate_args, frames[0].data_ptr(), frames[0].numel(), self._stream()),
                               "mi_deliver_resample_pcm")
                st.delivered += n_frames
        st.emitted = t1
        return out if dl is None else (frames, n_frames)

    def _host(self, out):
        if self.st.measure:                 # nothing was made and nothing leaves the device; finish() reads the peaks
            if not self.st.finished:
                return {}
            return _track_peaks(self.st, self.peaks.cpu())      # ONE D2H, 4 bytes per output
        if self.st.deliver is not None:
            return self._frames(*out)
        dev = self.st._out_device
        if dev is None or torch.device(dev).type != "cpu":
            return self.st._result(out)
        host = torch.empty(out.shape, dtype=out.dtype, pin_memory=True)
        host.copy_(out, non_blocking=True)
        torch.cuda.current_stream(self.st.device).synchronize()
        return host

    def _frames(self, frames, n: int) -> dict:
        """`{name: (n, channels) frames}` of a delivering stream, on the pushed block's device (host: ONE D2H of the bytes)."""
        from .audio import _FORMATS, deliver_views
        st = self.st
        to = st._out_device if st._out_device is not None else st.device
        if frames is None:
            dtype = _FORMATS[st.deliver.fmt][1]
            return {name: torch.empty(0, st.audio_channels, dtype=dtype, device=to) for name, _, _ in st.outputs}
        buf, offs = frames
        buf = self._host_bytes(buf) if torch.device(to).type == "cpu" else st._result(buf)
        return deliver_views(buf, st.outputs, offs, n, st.audio_channels, st.deliver.fmt)

    def _host_bytes(self, buf: torch.Tensor) -> torch.Tensor:
        host = torch.empty(buf.shape, dtype=buf.dtype, pin_memory=True)
        host.copy_(buf, non_blocking=True)
        torch.cuda.current_stream(self.st.device).synchronize()
        return host

    def push(self, block):
        st = self.st
        keep = []
        with torch.cuda.device(st.device):
            self._append(block, keep)
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


# ------------------------------------------------------------------------------------------------------------------------
# stream groups: many streams, one unit of work per push
# ------------------------------------------------------------------------------------------------------------------------
STREAMS_EMIT_COLS, APPEND_COLS, COMPACT_COLS = 7, 6, 4     # include/demucs_amd.h: MI_STREAMS_EMIT_*, MI_APPEND_*, MI_COMPACT_*
DELIVER_COLS = 9                                            # MI_DELIVER_COLS
ITEM_COLS = 8                                               # MI_PACK_ITEM_COLS


def apply_model_stream_group(model, shifts: int = 1, overlap: float = 0.25, transition_power: float = 1.0, segment=None,
                             device=None, split: bool = True, progress: bool = False, callback=None) -> "StreamGroup":
    """Many streams of one model (see `StreamGroup`).  `device` defaults to the first pushed block's."""
    return StreamGroup(model, shifts=shifts, overlap=overlap, transition_power=transition_power, segment=segment, device=device,
                       split=split, progress=progress, callback=callback)


class StreamGroup:
    """Streams of one model that are pushed and finished together.  Each stream is a `ModelStream` whose own scheduler
    (`_ready`, `_emit_limit`, `_keep_from`, `_segments_covering`, its RNG rules) decides what runs and what is final; the group
    only pools the ready segments of all streams of a call into shared forwards.  A forward's item does not depend on its batch
    position or on B, and every accumulator still receives its segments in ascending offset order, so `push({k: block, ...})`
    returns for every key exactly what that stream's own `push(block)` would, in the mapping's order, with the same use of
    `random`.

    On the engines a call is a fixed amount of device work whatever the number of streams: one H2D of the call's int64 table
    together with its host blocks, one `mi_streams_append`, the pooled forwards (each a gather, the forward and an overlap-add
    driven by that table), one `mi_streams_emit` and one D2H of the host-bound stems, plus one `mi_streams_compact` when a
    stream outgrows its room in the state buffer (every stream's window and accumulators).  Streams opened with `deliver=` add one
    `mi_deliver_pcm` for all of them behind the emit (and one `mi_deliver_mix_pcm` for all that deliver remixes, `Delivery(mix=)`,
    which read the mix from their windows in the state buffer, and one `mi_deliver_mix_auto_pcm` for all of those whose gains
    change, `Delivery(changes=)` / `change_mix`); their host-bound frames leave in one D2H of the byte buffer, and
    their float stems never do.  Those whose `Delivery` names another sample rate share one `mi_deliver_resample_pcm` instead (so a
    call has at most one launch more, whatever the number of streams), their frames in the same byte buffer and their carried
    values in the group's history buffer.  Streams that deliver with `clip="rescale"` keep their peaks (measured by the stream, or given to it) in
    the group's peaks buffer: a rescaling row names its slot there, the resampled rows then share one
    `mi_deliver_resample_pcm_peaks`, and measuring streams (`peaks="measure"`: no frames, `finish` returns their `TrackPeaks`) add
    one `mi_deliver_peaks_update` for all of them at the model's rate and one `mi_deliver_resample_peaks` for all at other rates,
    only on calls that have such rows.  Streams opened with `convert=`
    take blocks at another sample rate or channel count: one `mi_streams_convert_append` per call runs the streaming
    `convert_audio` (demucs_amd/audio.py, `ConvertPlan`) for all of them into their windows, and what the converter has made
    final is what the stream's scheduler sees as pushed.
    Other models run the same scheduler one segment at a time on the plain-torch route."""

    def __init__(self, model, shifts=1, overlap=0.25, transition_power=1.0, segment=None, device=None, split=True,
                 progress=False, callback=None):
        # shifts=0 draws nothing: the refusals and the members' geometry without any RNG call
        probe = ModelStream(model, shifts=0, overlap=overlap, transition_power=transition_power, segment=segment, split=split,
                            progress=progress, callback=callback)
        self.model = model
        self._kw = dict(shifts=shifts, overlap=overlap, transition_power=transition_power, segment=segment)
        self.members, self.bag_weights = probe.members, probe.bag_weights
        self.sources, self.audio_channels, self.samplerate = probe.sources, probe.audio_channels, probe.samplerate
        self.latency = probe.latency
        self.device = None if device is None else torch.device(device)
        self._streams = {}
        self._next = 0
        self._exec = None

    # ---- public --------------------------------------------------------------------------------------------------------
    def open(self, length: Optional[int] = None, affine=None, convert=None, deliver: Optional[Delivery] = None,
             pcm: Optional[str] = None, channels: Optional[int] = None, stats=None):
        """A new stream; makes the RNG calls `ModelStream(..., length=length)` makes.  Returns its key.

        `deliver=Delivery(...)`: the stream's results are `{name: (m, channels) frames}` (see `Delivery`), each stream of a group
        with its own; one `mi_deliver_pcm` launch per call serves all of them, its rows in the call's table.

        `convert=(audio.ConvertPlan, source channels)`: the stream's blocks are (source channels, n) at the plan's input rate and
        pass through the streaming `convert_audio` into its window (one `mi_streams_convert_append` for all such streams of a
        call); `length` then counts input samples, and the RNG calls are those of the converted length.

        `pcm=` ("i16", "i24", "f32"): the stream's blocks are interleaved wire PCM (`apply_model_stream`'s rule; `channels=` source
        channels unless `convert=` names them).  A call with such a stream uses `mi_streams_append_pcm` /
        `mi_streams_convert_append_pcm` for all its streams, the float ones as planar rows: still one append launch, one
        convert-append launch and one H2D, in which a host block travels as its raw bytes.

        `stats=` (an `audio.TrackStats`) in place of `affine=`: the stream's affine is its `(mean, s)` as they are, and `length`
        defaults to its `input_length`."""
        if stats is not None:
            if affine is not None:
                raise ValueError("give stats, or mean and std, not both: stats already holds the normaliser s = std + 1e-8")
            if length is None:
                length = stats.input_length
        feed = None
        if pcm is not None:                 # refused here, before any RNG call
            from .audio import PcmFeed, check_pcm, check_stream_channels
            check_pcm(pcm, all(m.kind != "generic" for m in self.members) and (self.device is None or self.device.type == "cuda"))
            if convert is not None and channels is not None and int(channels) != int(convert[1]):
                raise ValueError(f"channels={channels} contradicts convert=, which names {convert[1]} source channels")
            feed = PcmFeed(pcm, convert[1] if convert is not None else self.audio_channels if channels is None else channels)
            check_stream_channels(feed.src_channels, self.audio_channels)
        elif convert is None and channels is not None and channels != self.audio_channels:
            raise ValueError(f"expected {self.audio_channels} channels, got {channels}: a stream of float blocks converts no "
                             "channel layout")
        if deliver is not None:             # refused here, before any RNG call
            deliver.for_stream(self.sources, all(m.kind != "generic" for m in self.members) and
                               (self.device is None or self.device.type == "cuda"), self.samplerate, self.audio_channels)
        conv = None
        if convert is not None:
            from .audio import check_stream_channels
            plan, src_channels = convert
            check_stream_channels(int(src_channels), self.audio_channels)
            if any(m.kind == "generic" for m in self.members) or (self.device is not None and self.device.type != "cuda"):
                raise ValueError("a converting stream runs on the GPU engines (HTDemucs / HDemucs on a cuda device); there is no "
                                 "CPU resampler in this package")
            if length is not None and int(length) < 0:
                raise ValueError(f"length must be >= 0, got {length}")
            conv = _Conv(plan, int(src_channels), None if length is None else int(length))
            length = None if length is None else plan.final_count(int(length))
        st = ModelStream(self.model, device=self.device, length=length, affine=affine, deliver=deliver, stats=stats, **self._kw)
        st.convert = conv
        st.feed = feed
        key = self._next
        self._next += 1
        self._streams[key] = st
        return key

    @property
    def open_keys(self) -> list:
        return list(self._streams)

    def emitted(self, key) -> int:
        return self._stream(key).emitted

    def delivered(self, key) -> int:
        """Frames a stream with `Delivery(samplerate=R)` has returned so far (at R)."""
        return self._stream(key).delivered

    def pushed(self, key) -> int:
        return self._stream(key).pushed

    def change_mix(self, key, mix, at=None, ramp=0) -> None:
        """`ModelStream.change_mix` for stream `key`: its gains move to `mix`'s from delivered frame `at` over `ramp` frames."""
        self._stream(key).change_mix(mix, at=at, ramp=ramp)

    def trailing_bytes(self, key) -> int:
        """Bytes of an incomplete last frame of a PCM stream, carried to its next push."""
        return self._stream(key).trailing_bytes

    def device_bytes(self) -> int:
        """Bytes of device memory the group itself holds (state buffer, stats, forward buffers)."""
        return 0 if self._exec is None else self._exec.device_bytes()

    def push(self, blocks) -> dict:
        """`{key: (channels, n) block}` -> `{key: (S, channels, m) newly final stems}` (a delivering stream: `{name: (m, channels)
        frames}`), the streams taken in the mapping's order."""
        items = list(blocks.items())
        accepted = {}
        for key, block in items:
            st = self._stream(key)
            cv = getattr(st, "convert", None)
            if st.feed is not None:
                blk = accepted[key] = st.feed.accept(block)
                at, length = (cv.pushed, cv.length) if cv is not None else (st.pushed, st.length)
                if length is not None and at + blk.n > length:
                    raise ValueError(f"pushed {at + blk.n} samples, more than the declared length {length}")
                continue
            if cv is not None:
                if not isinstance(block, torch.Tensor) or block.dim() != 2 or block.shape[0] != cv.src_channels:
                    shape = tuple(block.shape) if isinstance(block, torch.Tensor) else type(block).__name__
                    raise ValueError(f"expected a ({cv.src_channels}, n) block, got {shape}")
                if cv.length is not None and cv.pushed + block.shape[1] > cv.length:
                    raise ValueError(f"pushed {cv.pushed + block.shape[1]} samples, more than the declared length {cv.length}")
                continue
            if not isinstance(block, torch.Tensor) or block.dim() != 2 or block.shape[0] != self.audio_channels:
                shape = tuple(block.shape) if isinstance(block, torch.Tensor) else type(block).__name__
                raise ValueError(f"expected a ({self.audio_channels}, n) block, got {shape}: a stream converts no channel layout")
            if st.length is not None and st.pushed + block.shape[1] > st.length:
                raise ValueError(f"pushed {st.pushed + block.shape[1]} samples, more than the declared length {st.length}")
        if not items:
            return {}
        self._start(accepted.get(items[0][0], items[0][1]).device)
        for key, blk in accepted.items():
            self._streams[key].feed.commit(blk)
        return self._exec.push([(k, self._streams[k], accepted.get(k, b)) for k, b in items])

    def finish(self, keys) -> dict:
        """Ends the streams `keys` (in that order) and returns `{key: remaining stems}`."""
        keys = list(keys)
        if len(set(keys)) != len(keys):
            raise ValueError("finish: a stream key is listed twice")
        for key in keys:
            st = self._stream(key)
            cv = getattr(st, "convert", None)
            if cv is not None:
                if cv.length is not None and cv.pushed != cv.length:
                    raise ValueError(f"the stream ended after {cv.pushed} samples, but length={cv.length} was declared")
                if cv.plan.final_count(cv.pushed) == 0:
                    raise ValueError("the stream ended before any sample was pushed")
                continue
            if st.length is not None and st.pushed != st.length:
                raise ValueError(f"the stream ended after {st.pushed} samples, but length={st.length} was declared")
            if st.pushed == 0:
                raise ValueError("the stream ended before any sample was pushed")
        if not keys:
            return {}
        if self._exec is None:                     # converting streams whose pushes were all empty
            raise ValueError("the stream ended before any sample was pushed")
        out = self._exec.finish([(k, self._streams[k]) for k in keys])
        for key in keys:
            del self._streams[key]
        return out

    # ---- internals -----------------------------------------------------------------------------------------------------
    def _stream(self, key) -> ModelStream:
        try:
            return self._streams[key]
        except (KeyError, TypeError):
            raise ValueError(f"unknown or finished stream key {key!r}") from None

    def _start(self, block_device) -> None:
        if self._exec is not None:
            return
        device = self.device if self.device is not None else torch.device(block_device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        if all(m.kind != "generic" for m in self.members):
            if device.type != "cuda":
                raise ValueError("apply_model_stream: HTDemucs / HDemucs engines run on a GPU device")
            self.device = device
            self._exec = _GroupEngineExec(self)
        else:
            self.device = device
            self._exec = _GroupTorchExec(self)


class _GroupTorchExec:
    """Models that are not the engine's: every stream's segments, one at a time, through its own `_TorchExec`."""

    def __init__(self, g: StreamGroup):
        self.g = weakref.proxy(g)          # no cycle: a dropped group frees its device memory at once
        self.execs = {}

    def device_bytes(self) -> int:
        return sum(ex.device_bytes() for ex in self.execs.values())

    def _exec(self, key, st: ModelStream) -> _TorchExec:
        if key not in self.execs:
            st.device = self.g.device
            self.execs[key] = _TorchExec(st)
        return self.execs[key]

    def push(self, items) -> dict:
        for key, st, block in items:
            self._exec(key, st)._append(block)
            st._out_device = block.device
        for key, st, _ in items:
            self.execs[key]._run(st._ready(final=False))
        return {key: self.execs[key]._emit(st._emit_limit()) for key, st, _ in items}

    def finish(self, items) -> dict:
        return {key: self.execs.pop(key).finish() for key, _ in items}


class _Conv:
    """The converter of one stream of a group: its `audio.ConvertPlan`, the input samples pushed, and where its carried input
    lives in the group's history buffer (two sides of (channels, plan.carry) floats from `off`; `side` is the one to read, whose
    first sample is input `h0`)."""

    def __init__(self, plan, src_channels: int, length):
        self.plan, self.src_channels, self.length = plan, src_channels, length
        self.pushed = 0
        self.off = None
        self.side = self.h0 = 0


class _Slot:
    """A stream's room in the group's state buffer: its window (channels, w_cap) at w_base, column 0 = track position w0, and
    per pass an accumulator (rows, cap) at base, column 0 = the pass's `a0`.  Columns past what was written hold zeros."""

    def __init__(self, st: ModelStream):
        self.st = st
        self.w_base = self.w_cap = self.w0 = 0
        self.a_base = [0] * len(st.passes)
        self.a_cap = [0] * len(st.passes)
        self.stats = -1
        self.placed = False


class _Staging:
    """The host blocks of one call, behind its table in the pinned upload: [(table index of the row's source column, byte offset,
    block)].  A wire PCM block travels as its raw bytes from a 16-byte boundary (the ingest kernels' widest load), a float block as
    float32."""

    def __init__(self):
        self.items, self.end = [], 0

    def add(self, pos: int, block) -> None:
        from .audio import PcmBlock
        wire = isinstance(block, PcmBlock)
        align = 16 if wire else 4
        self.end = -(-self.end // align) * align
        self.items.append((pos, self.end, block))
        self.end += block.nbytes if wire else 4 * block.numel()


class _GroupEngineExec:
    def __init__(self, g: StreamGroup):
        from .apply import _transition_weight
        self.g = weakref.proxy(g)          # no cycle: a dropped group frees its device memory at once
        dev = g.device
        self.lib = _lib.load()
        for m in g.members:
            m.model.to(dev)
            m.model.eval()
        with torch.cuda.device(dev):
            ramps = [_transition_weight(m.SL, m.transition_power, dev).to(torch.float32) for m in g.members]
            self.w_offs = [sum(r.numel() for r in ramps[:e]) for e in range(len(ramps))]
            self.weights = torch.cat(ramps).contiguous()
            self.scales = _upload(emit_scales(g._kw["shifts"], len(g.members), g.bag_weights, len(g.sources)), torch.float32, dev)
            self.state = torch.zeros(0, device=dev)
            self.stats = torch.zeros(2, device=dev)
        self.n_stats, self.stats_vals = 0, []
        self.slots = {}
        self.dead = False
        self.bufs = {}
        self.pad = max(m.V for m in g.members)
        # converting streams and streams that deliver at another rate: every stream's carried samples in one buffer (doubled when
        # an opened stream finds no room; regions of finished streams are reused), so its size follows the number of open streams
        # and never a stream's duration
        self.hist = None
        self.hist_used = 0
        self.hist_free = {}
        self.last_upload = (0, 0)          # bytes of the last call's table and of its whole pinned upload
        # rescaling deliveries: every stream's peak slots (one uint32 bit pattern per output) in one buffer, managed as the
        # history regions are: a measuring stream's are zeroed when it opens, a delivering stream's hold the peaks it was given
        self.peaks = None
        self.peaks_used = 0
        self.peaks_free = {}

    def device_bytes(self) -> int:
        n = self.state.numel() + self.stats.numel() + sum(t.numel() for b in self.bufs.values() for t in set(b))
        n += 0 if self.peaks is None else self.peaks.numel()
        return 4 * (n + (0 if self.hist is None else self.hist.numel()))

    def _peak_region(self, st: ModelStream) -> None:
        """Slots for the peaks of `st`'s outputs in the peaks buffer, filled at the stream's first call."""
        n = len(st.outputs)
        if st.peak_off is not None:
            return
        if self.peaks_free.get(n):
            st.peak_off = self.peaks_free[n].pop()
        else:
            have = 0 if self.peaks is None else self.peaks.numel()
            if self.peaks_used + n > have:
                grown = torch.zeros(max(2 * have, self.peaks_used + n, 64), device=self.g.device, dtype=torch.int32)
                if have:
                    grown[:have] = self.peaks
                self.peaks = grown
            st.peak_off = self.peaks_used
            self.peaks_used += n
        region = self.peaks[st.peak_off:st.peak_off + n]
        if st.measure:
            region.zero_()
        else:
            region.copy_(torch.tensor(list(st.deliver.peaks.bits), dtype=torch.int32))

    def _hist_region(self, cv, size=None) -> None:
        """Room for `cv`'s carried samples (a `_Conv`'s input, a `_Rate`'s values) in the history buffer."""
        size = 2 * self.g.audio_channels * cv.plan.carry if size is None else size
        if cv.off is not None or size == 0:
            return
        if self.hist_free.get(size):
            cv.off = self.hist_free[size].pop()
            return
        have = 0 if self.hist is None else self.hist.numel()
        if self.hist_used + size > have:
            grown = torch.zeros(max(2 * have, self.hist_used + size, 4096), device=self.g.device, dtype=torch.float32)
            if have:
                grown[:have] = self.hist
            self.hist = grown
        cv.off = self.hist_used
        self.hist_used += size

    def _stream(self):
        return C.c_void_p(_lib.current_stream_ptr())

    # ---- layout --------------------------------------------------------------------------------------------------------
    def _fits(self, slot: _Slot, w_end: int, new_hi) -> bool:
        if not slot.placed or w_end - slot.w0 > slot.w_cap:
            return False
        return all(h - ps.a0 <= cap for h, ps, cap in zip(new_hi, slot.st.passes, slot.a_cap))

    def _compact(self, before, keep_w, new_hi, w_end, table: list):
        """Lay every live slot out anew in a fresh state buffer: windows from `keep_w` on, accumulators from the emitted
        position on, each with room for at least as much again (rooms never shrink, so a steady stream stops moving them).
        Appends the copy rows to `table`; returns (new buffer, first row, rows, longest row)."""
        g = self.g
        C_ = g.audio_channels
        rows, total, longest = [], 0, 1
        stats_vals = []
        for key, slot in self.slots.items():
            st = slot.st
            w0 = keep_w[key]
            live_w = before[key] - w0 if slot.placed else 0
            w_cap = max(slot.w_cap, 2 * (w_end[key] - w0) + self.pad)
            for c in range(C_):
                src = slot.w_base + c * slot.w_cap + (w0 - slot.w0)
                rows.append((src if live_w > 0 else 0, total + c * w_cap, max(0, live_w), w_cap))
            slot.w_base, slot.w_cap, slot.w0 = total, w_cap, w0
            total += C_ * w_cap
            longest = max(longest, w_cap)
            for pi, ps in enumerate(st.passes):
                m = st.members[ps.member]
                a0 = st.emitted - ps.origin
                hi = max(ps.hi, new_hi[key][pi])
                live = ps.hi - a0 if slot.placed else 0
                cap = max(slot.a_cap[pi], 2 * max(0, hi - a0) + m.SL)
                for r in range(m.rows):
                    src = slot.a_base[pi] + r * slot.a_cap[pi] + (a0 - ps.a0)
                    rows.append((src if live > 0 else 0, total + r * cap, max(0, live), cap))
                slot.a_base[pi], slot.a_cap[pi] = total, cap
                ps.a0 = a0
                total += m.rows * cap
                longest = max(longest, cap)
            if st.affine is not None:
                slot.stats = len(stats_vals) // 2
                stats_vals += list(st.affine)
            else:
                slot.stats = -1
            slot.placed = True
        first = len(table) // COMPACT_COLS
        for r in rows:
            table += r
        self.dead = False
        self.n_stats = len(stats_vals) // 2
        if stats_vals != self.stats_vals:
            self.stats_vals = stats_vals
            self.stats = _upload(stats_vals or [0.0, 0.0], torch.float32, g.device)
        return torch.empty(total, device=g.device, dtype=torch.float32), first, len(rows), longest

    # ---- forwards ------------------------------------------------------------------------------------------------------
    def _plan(self, units):
        """Pool the ready units of all streams into forwards [(member, valid, [(key, pass index, offset, n)])]: per member,
        HTDemucs in stream / pass / offset order, up to max_batch per forward; HDemucs one chunk length per forward, longest
        first (lengths never grow along a pass, so every accumulator still receives its segments in ascending order)."""
        g = self.g
        plan = []
        for e, m in enumerate(g.members):
            mine = [(key, pi, o, n) for key, us in units for pi, o, n in us if self.slots[key].st.passes[pi].member == e]
            for key, us in units:
                st = self.slots[key].st
                st._dispatch_draw(st.members[e], sum(1 for pi, _, _ in us if st.passes[pi].member == e))
            if not mine:
                continue
            B = m.model.max_batch
            if m.kind == "ht":
                plan += [(e, m.V, mine[i:i + B]) for i in range(0, len(mine), B)]
                continue
            for n in sorted({u[3] for u in mine}, reverse=True):
                same = [u for u in mine if u[3] == n]
                plan += [(e, n, same[i:i + B]) for i in range(0, len(same), B)]
        return plan

    def _forward_tables(self, e, valid, fw, table: list):
        g = self.g
        m = g.members[e]
        items, tiles, groups = [], [], []
        for k, (key, pi, o, n) in enumerate(fw):
            slot = self.slots[key]
            ps = slot.st.passes[pi]
            trim = (valid - n) // 2 if m.kind == "ht" else 0
            items += [slot.w_base, slot.w_cap, ps.origin + o - trim - slot.w0, slot.a_base[pi], slot.a_cap[pi], o - ps.a0, n, trim]
            if groups and groups[-1][0] == (key, pi):
                groups[-1][2] = k + 1
            else:
                groups.append([(key, pi), k, k + 1])
        for (key, pi), i0, i1 in groups:
            slot = self.slots[key]
            ps = slot.st.passes[pi]
            us = fw[i0:i1]
            lo = max(0, min(o - ps.a0 for _, _, o, _ in us))
            hi = min(slot.a_cap[pi], max(o + n - ps.a0 for _, _, o, n in us))
            for pos in range(lo, hi, TILE_SPAN):
                tiles += [slot.a_base[pi], slot.a_cap[pi], pos, i0, i1, self.w_offs[e], m.SL]
        at = len(table)
        table += items + tiles
        return at, len(tiles) // TILE_COLS

    def _forward(self, e, valid, fw, t_items, n_tiles, keep):
        g = self.g
        m = g.members[e]
        sub = m.model
        dev = g.device
        nb = len(fw)
        channels = g.audio_channels

        def gather(seg):
            _lib.check(self.lib.mi_segments_gather_packed(self.state.data_ptr(), self.state.numel(), channels, C.c_void_p(t_items),
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
        else:
            seg = torch.empty(nb, channels, valid, device=dev, dtype=torch.float32)
            gather(seg)
            side = nb == 1 and valid < m.SL and valid >= _HDEMUCS_MIN_LENGTH     # a lone tail: the single-item side engine
            out = sub(seg, aux=True) if side else sub(seg)
            out_valid = valid
            keep.append(out)
        if n_tiles:
            _lib.check(self.lib.mi_ola_accumulate_packed(self.state.data_ptr(), self.state.numel(), m.rows, out.data_ptr(), out_valid,
                                                         out.numel(), C.c_void_p(t_items), nb, C.c_void_p(t_items + 8 * ITEM_COLS * nb),
                                                         n_tiles, self.weights.data_ptr(), self.weights.numel(), self._stream()),
                       "mi_ola_accumulate_packed")

    # ---- one call --------------------------------------------------------------------------------------------------------
    def _step(self, work, final: bool) -> dict:
        """work: [(key, stream, block or None)] in call order."""
        g = self.g
        dev = g.device
        S, C_ = len(g.sources), g.audio_channels
        keep = []
        with torch.cuda.device(dev):
            # 1. the streams' own scheduling: windows to keep, new samples, ready segments, what becomes final
            for key, st, _ in work:
                if key not in self.slots:
                    self.slots[key] = _Slot(st)
                    st.device = dev
            # the first window position a pending segment can read, before this call dispatches any (as ModelStream's append)
            before = {key: slot.st.pushed for key, slot in self.slots.items()}
            keep_w = {key: slot.st._keep_from() for key, slot in self.slots.items()}
            units, blocks, jobs = [], [], []
            for key, st, block in work:
                cv = getattr(st, "convert", None)
                if cv is not None:
                    # the converter decides how many samples at the model's rate this call adds to the window
                    n_in = 0 if block is None else block.shape[1]
                    out0, n_out, nxt = cv.plan.step(cv.pushed, n_in, block is None)
                    jobs.append((self.slots[key], cv, block, n_in, out0, n_out, nxt))
                    st.pushed += n_out
                    cv.pushed += n_in
                    if block is not None:
                        st._out_device = block.device
                    else:
                        st.finished = True
                elif block is not None:
                    st.pushed += block.shape[1]
                    st._out_device = block.device
                    blocks.append((key, self.slots[key], block))
                else:
                    st.finished = True
            for key, st, _ in work:
                units.append((key, st._ready(final=final)))
            w_end = {key: slot.st.pushed for key, slot in self.slots.items()}
            new_hi = {key: [ps.hi for ps in slot.st.passes] for key, slot in self.slots.items()}
            for key, us in units:
                for pi, o, n in us:
                    new_hi[key][pi] = max(new_hi[key][pi], o + n)
            # 2. one int64 table for the whole call: compaction rows, append rows, every forward's items and tiles, the emit
            table = []
            compact = None
            if self.dead or not all(self._fits(s, w_end[k], new_hi[k]) for k, s in self.slots.items()):
                compact = self._compact(before, keep_w, new_hi, w_end, table)
            for key, us in units:
                slot = self.slots[key]
                for pi, o, n in us:
                    ps = slot.st.passes[pi]
                    ps.hi = max(ps.hi, o + n)
            staged = _Staging()
            append = self._append_rows(blocks, table, keep, staged)
            convert = self._convert_rows(jobs, table, keep, staged)
            plan = [(e, valid, fw, *self._forward_tables(e, valid, fw, table)) for e, valid, fw in self._plan(units)]
            emit = self._emit_rows(work, table, self.state if compact is None else compact[0])
            base = self._upload(table, staged, keep)
            # 3. device work
            if compact is not None:
                state, first, n_rows, longest = compact
                # nothing to copy from an empty buffer: any live pointer, capacity 0
                old, old_cap = (self.state, self.state.numel()) if self.state.numel() else (self.weights, 0)
                for r0 in range(0, n_rows, 65535):
                    nr = min(65535, n_rows - r0)
                    _lib.check(self.lib.mi_streams_compact(state.data_ptr(), state.numel(), old.data_ptr(), old_cap,
                                                           C.c_void_p(base + 8 * COMPACT_COLS * (first + r0)), nr, longest,
                                                           self._stream()), "mi_streams_compact")
                self.state = state
            if append is not None and append[3]:        # a wire PCM block among them: the entry with a format per row
                at, n_rows, _, max_bytes = append
                _lib.check(self.lib.mi_streams_append_pcm(self.state.data_ptr(), self.state.numel(), C_, C.c_void_p(base + 8 * at),
                                                          n_rows, max_bytes, self.stats.data_ptr(), self.n_stats, self._stream()),
                           "mi_streams_append_pcm")
            elif append is not None:
                at, n_rows, longest, _ = append
                _lib.check(self.lib.mi_streams_append(self.state.data_ptr(), self.state.numel(), C_, C.c_void_p(base + 8 * at), n_rows,
                                                      longest, self.stats.data_ptr(), self.n_stats, self._stream()),
                           "mi_streams_append")
            if convert is not None:
                from .audio import _BankArena
                at, n_rows, groups, lds_floats, wire = convert
                bank, hist = _BankArena.get(dev).buf, self.hist
                entry, name = self.lib.mi_streams_convert_append, "mi_streams_convert_append"
                if wire:
                    entry, name = self.lib.mi_streams_convert_append_pcm, "mi_streams_convert_append_pcm"
                _lib.check(entry(self.state.data_ptr(), self.state.numel(), C_, C.c_void_p(base + 8 * at),
                                 n_rows, groups, bank.data_ptr() if bank.numel() else None, bank.numel(),
                                 hist.data_ptr() if hist is not None else None,
                                 0 if hist is None else hist.numel(), self.stats.data_ptr(), self.n_stats,
                                 lds_floats, self._stream()), name)
            for e, valid, fw, at, n_tiles in plan:
                self._forward(e, valid, fw, base + 8 * at, n_tiles, keep)
            outs = self._emit(emit, base)
            if final:
                for m in g.members:
                    if m.kind == "h":
                        m.model.check()      # a time-out of the LAST forward's recurrence would otherwise pass unnoticed
                for key, st, _ in work:
                    cv = getattr(st, "convert", None)
                    if cv is not None and cv.off is not None:
                        self.hist_free.setdefault(2 * C_ * cv.plan.carry, []).append(cv.off)
                        cv.off = None
                    if st.rate is not None and st.rate.off is not None:
                        self.hist_free.setdefault(st.rate.size, []).append(st.rate.off)
                        st.rate.off = None
                    if st.peak_off is not None:
                        self.peaks_free.setdefault(len(st.outputs), []).append(st.peak_off)
                        st.peak_off = None
                    del self.slots[key]
                    self.dead = True
                if not self.slots:
                    self.state = torch.zeros(0, device=dev)
            return outs

    def _append_rows(self, blocks, table, keep, staged):
        """mi_streams_append's rows, or mi_streams_append_pcm's (MI_APPEND_PCM_*: a format and a source channel count more per
        row, the float blocks as planar rows) when a block of the call is wire PCM.  Device blocks are read where they are; a host
        block joins `staged`, and its source is named once the call's upload buffer exists (`_upload`).  Returns (first row, rows,
        longest block, largest source in bytes if the rows are the PCM entry's else 0) or None."""
        from .audio import PCM_PLANAR, PcmBlock
        g = self.g
        C_ = g.audio_channels
        live = [(key, slot, b) for key, slot, b in blocks if b.shape[1] > 0]
        if not live:
            return None
        wire = any(isinstance(b, PcmBlock) for _, _, b in live)
        at = len(table)
        longest, max_bytes = 1, 0
        for key, slot, b in live:
            n = b.shape[1]
            pcm = isinstance(b, PcmBlock)
            if b.device.type == "cpu":
                staged.add(len(table), b)
                src = 0
            else:
                d = b.on_device(g.device, keep) if pcm else b.to(device=g.device, dtype=torch.float32).contiguous()
                keep.append(d)
                src = d.data_ptr()
            table += [src, n, slot.w_base, slot.w_cap, slot.st.pushed - n - slot.w0, slot.stats]
            if wire:
                table += [b.code, b.src_channels] if pcm else [PCM_PLANAR, C_]
                max_bytes = max(max_bytes, b.nbytes if pcm else 4 * C_ * n)
            longest = max(longest, n)
        return at, len(live), longest, max_bytes

    def _convert_rows(self, jobs, table, keep, staged):
        """mi_streams_convert_append's rows (MI_CVT_*) for the converting streams of the call with a block or final outputs; host
        blocks join `staged`.  Flips every such stream's history side.  Returns (first index, rows, workgroups per row, LDS
        floats) or None."""
        from .audio import CVT_COLS, CVT_PCM_COLS, PCM_PLANAR, PcmBlock, _BankArena
        g = self.g
        C_ = g.audio_channels
        live = [j for j in jobs if j[3] > 0 or j[5] > 0]
        if not live:
            return None
        # a wire PCM block among them: mi_streams_convert_append_pcm's rows (one column more, the block's format) for all
        wire = any(isinstance(j[2], PcmBlock) for j in live)
        arena = _BankArena.get(g.device)
        at = len(table)
        groups, lds_floats = 1, 1
        for slot, cv, b, n_in, out0, n_out, nxt in live:
            plan, final = cv.plan, b is None
            pcm = isinstance(b, PcmBlock)
            self._hist_region(cv)
            src = 0
            if n_in and b.device.type == "cpu":
                staged.add(len(table), b)
            elif n_in:
                d = b.on_device(g.device, keep) if pcm else b.to(device=g.device, dtype=torch.float32).contiguous()
                keep.append(d)
                src = d.data_ptr()
            side = C_ * plan.carry
            base = cv.off or 0
            table += [src, cv.src_channels, n_in, cv.pushed - n_in, plan.carry, base + cv.side * side, base + (1 - cv.side) * side,
                      cv.h0, nxt, out0, n_out, cv.pushed if final else -1, plan.old, plan.new, plan.width, arena.offset(plan),
                      slot.w_base, slot.w_cap, slot.st.pushed - n_out - slot.w0, slot.stats]
            if wire:
                table.append(b.code if pcm else PCM_PLANAR)
            if not final and not plan.copy:
                cv.side, cv.h0 = 1 - cv.side, nxt
            groups = max(groups, plan.groups(n_out))
            lds_floats = max(lds_floats, plan.lds_floats())
        assert (len(table) - at) == (CVT_PCM_COLS if wire else CVT_COLS) * len(live)
        return at, len(live), groups, lds_floats, wire

    def _upload(self, table, staged, keep) -> int:
        """The call's int64 table and its host blocks (`_Staging`: float32, or a wire PCM block's raw bytes) in one pinned
        buffer, down in ONE H2D.  Returns the table's device address."""
        from .audio import PcmBlock
        T = max(1, len(table))
        f_at = -(-8 * T // 16) * 16
        nbytes = f_at + staged.end
        dev_buf = torch.empty(nbytes, dtype=torch.uint8, device=self.g.device)
        base = dev_buf.data_ptr()
        for pos, off, _ in staged.items:
            table[pos] = base + f_at + off
        host = torch.empty(nbytes, dtype=torch.uint8, pin_memory=True)
        raw = host.numpy()
        np.frombuffer(raw, dtype=np.int64, count=T)[:] = table or [0]
        for _, off, b in staged.items:
            if isinstance(b, PcmBlock):
                b.stage(raw[f_at + off:f_at + off + b.nbytes])
            else:
                host[f_at + off:f_at + off + 4 * b.numel()].view(torch.float32).view(b.shape).copy_(b)
        self.last_upload = (8 * T, nbytes)
        dev_buf.copy_(host, non_blocking=True)
        keep += [host, dev_buf]
        return base

    def _emit_rows(self, work, table, state):
        """mi_streams_emit's tables for every stream of the call with new final samples; host-bound stems first.  Behind them the
        rows of the delivering streams: mi_deliver_pcm's, then mi_deliver_resample_pcm's for those that deliver at another rate,
        last mi_deliver_mix_pcm's for those that deliver remixes, which read the mix from their windows in `state` (the state
        buffer as the emit will find it, after this call's compaction), and mi_deliver_mix_auto_pcm's table (`audio.auto_table`)
        for the remixing streams whose gains change."""
        g = self.g
        from .audio import MIX_COLS, RATE_COLS, _BankArena, auto_table, deliver_layout, rate_groups, rate_lds_floats
        S, C_ = len(g.sources), g.audio_channels
        spans = []
        for key, st, _ in work:
            t0, t1 = st.emitted, st._emit_limit()
            dev = st._out_device
            spans.append((key, st, t0, t1, dev is not None and torch.device(dev).type == "cpu"))
        # float stems that go to the host first; a delivering stream's stay on the device, so they sort with the device-bound
        spans.sort(key=lambda s: not (s[4] and s[1].deliver is None))
        streams, passes, segs = [], [], []
        off, host_n, longest = 0, 0, 1
        layout = {}
        for key, st, t0, t1, to_host in spans:
            n = t1 - t0
            layout[key] = (off, n)
            if n > 0:
                slot = self.slots[key]
                p_lo, s_lo = len(passes) // 8, len(segs) // 2
                for pi, ps in enumerate(st.passes):
                    q0, q1 = t0 - ps.origin, t1 - ps.origin
                    g_lo = len(segs) // 2
                    for o, sn in st._segments_covering(ps, q0, q1):
                        segs += [o - ps.a0, sn]
                    e = ps.member
                    passes += [slot.a_base[pi], slot.a_cap[pi], q0 - ps.a0, g_lo, len(segs) // 2, self.w_offs[e], g.members[e].SL, e]
                streams += [p_lo, len(passes) // 8, s_lo, len(segs) // 2, slot.stats, off, n]
                longest = max(longest, n)
            off += S * C_ * n
            if to_host and st.deliver is None:
                host_n = off
            st.emitted = t1
        at = len(table)
        table += streams + passes + (segs or [0, 0])
        # the float stems of the call (allocated here: a delivery row names its stream's) and the delivered frames, one byte
        # buffer with the host-bound streams first
        out = torch.empty(off, device=g.device, dtype=torch.float32) if off else None
        d_rows, d_layout, d_off, d_host, d_longest = [], {}, 0, 0, 1
        r_rows, r_groups, r_lds, d_count = [], 1, 1, {}
        # rescaling deliveries: the peak slot of every resampled row (-1: the row does not rescale), and the measuring streams'
        # rows, which make no frames: mi_deliver_peaks_update's at the model's rate, mi_deliver_resample_peaks' at another
        r_slots, r_rescales = [], False
        m_rows, m_longest, mr_rows, mr_slots, mr_groups, mr_lds = [], 1, [], [], 1, 1
        # remixing deliveries: all of a call's in one launch more, the measuring ones among them in one of their own
        x_rows, x_longest, xm_rows, xm_longest = [], 1, [], 1
        # those among them whose gains change: one launch for all of them too, their changes behind their rows
        a_rows, a_t0s, a_changes, a_longest = [], [], [], 1
        for key, st, t0, _, to_host in sorted(spans, key=lambda s: not s[4]):
            f_off, n = layout[key]
            rt, dl = st.rate, st.deliver
            if dl is None:
                continue
            if dl.peaks is not None:
                self._peak_region(st)
            if n == 0 and rt is None:
                continue
            src = out.data_ptr() + 4 * f_off if n else 0
            if rt is not None:
                # the frames whose last tap is emitted; a finishing stream has a tail even when it emits nothing
                n_out = rt.plan.step(t0, n, st.finished)[1]
                if n == 0 and n_out == 0:
                    continue
                self._hist_region(rt, rt.size)
                bank_off = _BankArena.get(g.device).offset(rt.plan)
                st.delivered += n_out
                if st.measure:
                    mr_rows += rt.rows(st.outputs, dl, src, n, t0, st.finished, bank_off, [0] * len(st.outputs))
                    mr_slots += range(st.peak_off, st.peak_off + len(st.outputs))
                    mr_groups = max(mr_groups, rate_groups(rt.plan, C_, n_out))
                    mr_lds = max(mr_lds, rate_lds_floats(rt.plan, C_))
                    continue
                offs, d_off = deliver_layout(st.outputs, n_out, C_, dl.fmt, d_off)
                r_rows += rt.rows(st.outputs, dl, src, n, t0, st.finished, bank_off, offs)
                r_slots += range(st.peak_off, st.peak_off + len(st.outputs)) if dl.peaks is not None else [-1] * len(st.outputs)
                r_rescales = r_rescales or dl.peaks is not None
                r_groups = max(r_groups, rate_groups(rt.plan, C_, n_out))
                r_lds = max(r_lds, rate_lds_floats(rt.plan, C_))
                d_layout[key], d_count[key] = offs, n_out
            elif st.measure and st.gains is not None:
                slot = self.slots[key]
                xm_rows += _mix_rows(st, src, n, t0, state.data_ptr() + 4 * slot.w_base, slot.w0, slot.w_cap, None, st.peak_off)
                xm_longest = max(xm_longest, n)
                continue
            elif st.measure:
                m_rows += _deliver_rows(st.outputs, dl, src, n, None, st.peak_off)
                m_longest = max(m_longest, n)
                continue
            elif st.schedule is not None:
                slot = self.slots[key]
                offs, d_off = deliver_layout(st.outputs, n, C_, dl.fmt, d_off)
                rows, changes = _auto_rows(st, src, n, t0, state.data_ptr() + 4 * slot.w_base, slot.w0, slot.w_cap, offs,
                                           st.peak_off or 0)
                a_rows += rows
                a_t0s += [t0] * len(changes)
                a_changes += changes
                d_layout[key], d_count[key] = offs, n
                a_longest = max(a_longest, n)
            elif st.gains is not None:
                slot = self.slots[key]
                offs, d_off = deliver_layout(st.outputs, n, C_, dl.fmt, d_off)
                x_rows += _mix_rows(st, src, n, t0, state.data_ptr() + 4 * slot.w_base, slot.w0, slot.w_cap, offs, st.peak_off or 0)
                d_layout[key], d_count[key] = offs, n
                x_longest = max(x_longest, n)
            else:
                offs, d_off = deliver_layout(st.outputs, n, C_, dl.fmt, d_off)
                d_rows += _deliver_rows(st.outputs, dl, src, n, offs, st.peak_off or 0)
                d_layout[key], d_count[key] = offs, n
                d_longest = max(d_longest, n)
            if to_host:
                d_host = d_off
        d_at = len(table)
        table += d_rows
        r_at = len(table)
        table += r_rows
        rs_at = len(table)
        table += _packed_slots(r_slots) if r_rescales else []
        m_at = len(table)
        table += m_rows
        mr_at = len(table)
        table += mr_rows
        mrs_at = len(table)
        table += _packed_slots(mr_slots)
        x_at = len(table)
        table += x_rows
        xm_at = len(table)
        table += xm_rows
        a_at = len(table)
        a_table = auto_table(a_rows, a_t0s, a_changes)
        table += a_table
        return dict(at=at, n_streams=len(streams) // STREAMS_EMIT_COLS, n_passes=len(passes) // 8, n_segs=len(segs) // 2,
                    x_at=x_at, x_rows=len(x_rows) // MIX_COLS, x_longest=x_longest, xm_at=xm_at, xm_rows=len(xm_rows) // MIX_COLS,
                    xm_longest=xm_longest, a_at=a_at, a_rows=len(a_t0s), a_len=len(a_table), a_longest=a_longest,
                    total=off, host_n=host_n, longest=longest, layout=layout, order=[k for k, _, _ in work],
                    streams={k: st for k, st, _ in work}, out=out, d_at=d_at, d_rows=len(d_rows) // DELIVER_COLS, d_total=d_off,
                    d_host=d_host, d_longest=d_longest, d_layout=d_layout, d_count=d_count, r_at=r_at,
                    r_rows=len(r_rows) // RATE_COLS, r_groups=r_groups, r_lds=r_lds, r_rescales=r_rescales, rs_at=rs_at,
                    m_at=m_at, m_rows=len(m_rows) // DELIVER_COLS, m_longest=m_longest, mr_at=mr_at,
                    mr_rows=len(mr_rows) // RATE_COLS, mr_groups=mr_groups, mr_lds=mr_lds, mrs_at=mrs_at)

    def _emit(self, emit, base) -> dict:
        g = self.g
        dev = g.device
        S, C_ = len(g.sources), g.audio_channels
        out = emit["out"]
        if emit["n_streams"]:
            at = base + 8 * emit["at"]
            t_streams = at
            t_passes = t_streams + 8 * STREAMS_EMIT_COLS * emit["n_streams"]
            t_segs = t_passes + 8 * EMIT_PASS_COLS * emit["n_passes"]
            _lib.check(self.lib.mi_streams_emit(self.state.data_ptr(), self.state.numel(), S, C_, C.c_void_p(t_streams),
                                                emit["n_streams"], emit["longest"], C.c_void_p(t_passes), emit["n_passes"],
                                                C.c_void_p(t_segs), emit["n_segs"], self.weights.data_ptr(), self.weights.numel(),
                                                self.scales.data_ptr(), len(g.members), g._kw["shifts"],
                                                int(g.bag_weights is not None), self.stats.data_ptr(), self.n_stats, out.data_ptr(),
                                                out.numel(), self._stream()), "mi_streams_emit")
        frames = None
        if emit["d_rows"] or emit["r_rows"] or emit["x_rows"] or emit["a_rows"]:
            # at least 16 bytes: a call on which resampling streams only carry values still names a destination
            frames = torch.empty(max(emit["d_total"], 16), dtype=torch.uint8, device=dev)
        pk = (None, 0) if self.peaks is None else (self.peaks.data_ptr(), self.peaks.numel())
        if emit["d_rows"]:
            _lib.check(self.lib.mi_deliver_pcm(C.c_void_p(base + 8 * emit["d_at"]), emit["d_rows"], emit["d_longest"], S, C_, *pk,
                                               frames.data_ptr(), frames.numel(), self._stream()), "mi_deliver_pcm")
        if emit["r_rows"] or emit["mr_rows"]:
            from .audio import _BankArena
            bank, hist = _BankArena.get(dev).buf, self.hist
        if emit["r_rows"]:
            rate_args = (C.c_void_p(base + 8 * emit["r_at"]), emit["r_rows"], emit["r_groups"], S, C_, bank.data_ptr(), bank.numel(),
                         hist.data_ptr(), hist.numel(), emit["r_lds"], frames.data_ptr(), frames.numel())
            if emit["r_rescales"]:          # a row among them divides by its peak: the entry that reads the slots
                _lib.check(self.lib.mi_deliver_resample_pcm_peaks(*rate_args, C.c_void_p(base + 8 * emit["rs_at"]), *pk,
                                                                  self._stream()), "mi_deliver_resample_pcm_peaks")
            else:
                _lib.check(self.lib.mi_deliver_resample_pcm(*rate_args, self._stream()), "mi_deliver_resample_pcm")
        # the measuring streams: one launch for those at the model's rate, one for those at another, and only when there are any
        if emit["m_rows"]:
            _lib.check(self.lib.mi_deliver_peaks_update(C.c_void_p(base + 8 * emit["m_at"]), emit["m_rows"], emit["m_longest"], S, C_,
                                                        *pk, self._stream()), "mi_deliver_peaks_update")
        if emit["mr_rows"]:
            _lib.check(self.lib.mi_deliver_resample_peaks(C.c_void_p(base + 8 * emit["mr_at"]), emit["mr_rows"], emit["mr_groups"], S,
                                                          C_, bank.data_ptr(), bank.numel(), hist.data_ptr(), hist.numel(),
                                                          emit["mr_lds"], C.c_void_p(base + 8 * emit["mrs_at"]), *pk, self._stream()),
                       "mi_deliver_resample_peaks")
        # the remixing streams: one launch for all that deliver, one for all that measure
        if emit["x_rows"]:
            _lib.check(self.lib.mi_deliver_mix_pcm(C.c_void_p(base + 8 * emit["x_at"]), emit["x_rows"], emit["x_longest"], S, C_, *pk,
                                                   frames.data_ptr(), frames.numel(), self._stream()), "mi_deliver_mix_pcm")
        if emit["a_rows"]:                  # and one for all whose gains change
            _lib.check(self.lib.mi_deliver_mix_auto_pcm(C.c_void_p(base + 8 * emit["a_at"]), emit["a_len"], emit["a_rows"],
                                                        emit["a_longest"], S, C_, *pk, frames.data_ptr(), frames.numel(),
                                                        self._stream()), "mi_deliver_mix_auto_pcm")
        if emit["xm_rows"]:
            _lib.check(self.lib.mi_deliver_mix_peaks_update(C.c_void_p(base + 8 * emit["xm_at"]), emit["xm_rows"], emit["xm_longest"],
                                                            S, C_, *pk, self._stream()), "mi_deliver_mix_peaks_update")
        host = host_frames = None
        if emit["host_n"]:
            host = torch.empty(emit["host_n"], dtype=torch.float32, pin_memory=True)
            host.copy_(out[:emit["host_n"]], non_blocking=True)
        if emit["d_host"]:
            host_frames = torch.empty(emit["d_host"], dtype=torch.uint8, pin_memory=True)
            host_frames.copy_(frames[:emit["d_host"]], non_blocking=True)
        if host is not None or host_frames is not None:
            torch.cuda.current_stream(dev).synchronize()
        res = {}
        for key in emit["order"]:
            off, n = emit["layout"][key]
            st = emit["streams"][key]
            to = st._out_device
            if st.measure:                  # no frames; a finishing stream's peaks come back by ONE D2H of 4 bytes per output
                res[key] = _track_peaks(st, self.peaks[st.peak_off:st.peak_off + len(st.outputs)].cpu()) if st.finished else {}
            elif st.deliver is not None:
                res[key] = self._frames(st, emit["d_count"].get(key, 0), emit["d_layout"].get(key), frames, host_frames,
                                        emit["d_host"])
            elif n == 0:
                res[key] = torch.empty(S, C_, 0, dtype=torch.float32, device=to)
            elif host is not None and off < emit["host_n"]:
                res[key] = host[off:off + S * C_ * n].view(S, C_, n)
            else:
                res[key] = st._result(out[off:off + S * C_ * n].view(S, C_, n))
        return res

    def _frames(self, st: ModelStream, n: int, offs, frames, host_frames, d_host: int) -> dict:
        """`{name: (n, channels) frames}` of a delivering stream, on its last block's device."""
        from .audio import _FORMATS, deliver_views
        C_ = self.g.audio_channels
        to = st._out_device if st._out_device is not None else self.g.device
        if offs is None:
            dtype = _FORMATS[st.deliver.fmt][1]
            return {name: torch.empty(0, C_, dtype=dtype, device=to) for name, _, _ in st.outputs}
        if host_frames is not None and offs[0] < d_host:
            return deliver_views(host_frames, st.outputs, offs, n, C_, st.deliver.fmt)
        views = deliver_views(frames, st.outputs, offs, n, C_, st.deliver.fmt)
        return {name: st._result(v) for name, v in views.items()}

    def push(self, items) -> dict:
        return self._step(items, final=False)

    def finish(self, items) -> dict:
        return self._step([(k, st, None) for k, st in items], final=True)
