"""`Separator`: the tensor-level face of the reference's public API (reference: demucs/api.py:53-319).

Only what sits on the tensor -> tensor path is provided: construction around an already built
model (the model zoo download of `demucs/pretrained.py` needs the network and is out of scope),
`update_parameter`, `separate_tensor` (api.py:241-291), the `samplerate / audio_channels / model`
properties and `list_models` for a local folder (api.py:322-347).  Audio file loading and the stem writers are not part of this path.

`separate_tensor` is a device path: ONE host -> device copy of the raw `wav`, the resampler kernel when `sr`
differs (`convert_audio`, demucs_amd/audio.py), the mono mean / unbiased std by a device reduction
(`mi_mono_stats`; the two scalars never visit the host), `(x - mean) / (std + 1e-8)` in place on the device
copy (`mi_track_affine`), `apply_model` on device-resident tensors, `x * std + mean` in place on the stems,
ONE device -> host copy of the stems into a pinned tensor.  The caller's host `wav` is never touched (the
reference normalises it in place and restores it, which leaves rounding differences of ~1e-7 behind); a device
`wav` is normalised and restored in place exactly as the reference does.
"""
from __future__ import annotations

import ctypes as C
from pathlib import Path
from typing import Callable, Dict, List, Optional, Sequence, Tuple, Union

import torch

from . import _lib
from .audio import ConvertingStatsStream, MonoStatsStream, TrackLoudness, TrackPeaks, TrackScore, TrackStats, TrackTruePeaks, convert_audio
from .apply import BagOfModels, _is_engine, _to_host, apply_model, apply_model_many
from .stream import Delivery, ModelStream, StreamGroup

__all__ = ["Separator", "SeparatorStream", "Delivery", "TrackStats", "TrackPeaks", "TrackScore", "TrackLoudness", "TrackTruePeaks",
           "LoadModelError", "list_models"]


class LoadModelError(Exception):
    pass


def _with(d: Optional[dict], **subs) -> dict:
    out = dict(d) if d is not None else {}
    out.update(subs)
    return out


def _shared_device_storage(wavs) -> bool:
    """True when two GPU tensors of `wavs` are backed by the same storage."""
    seen = set()
    for w in wavs:
        if w.device.type != "cuda":
            continue
        key = (w.device, w.untyped_storage().data_ptr())
        if key in seen:
            return True
        seen.add(key)
    return False


class Separator:
    def __init__(self, model, repo=None, device="cuda", shifts: int = 1, overlap: float = 0.25, split: bool = True,
                 segment: Optional[int] = None, jobs: int = 0, progress: bool = False,
                 callback: Optional[Callable[[dict], None]] = None, callback_arg: Optional[dict] = None):
        if isinstance(model, str):
            # api.py:99-104: `Separator(model=name, repo=folder)`; offline only "demucs_unittest" and local folders resolve
            from .pretrained import get_model
            from .states import ModelLoadingError
            try:
                model = get_model(model, repo)
            except ModelLoadingError as exc:
                raise LoadModelError(str(exc)) from exc
        self._model = model
        self._audio_channels = model.audio_channels
        self._samplerate = model.samplerate
        self.update_parameter(device=device, shifts=shifts, overlap=overlap, split=split, segment=segment, jobs=jobs,
                              progress=progress, callback=callback, callback_arg=callback_arg)

    def update_parameter(self, device=None, shifts=None, overlap=None, split=None, segment=-1, jobs=None, progress=None,
                         callback=-1, callback_arg=-1):
        """api.py:124-201: only the given parameters change (segment / callback use a sentinel because
        None is a legal value)."""
        if device is not None: self._device = device
        if shifts is not None: self._shifts = shifts
        if overlap is not None: self._overlap = overlap
        if split is not None: self._split = split
        if segment != -1:
            if segment is not None and segment <= 0:
                raise ValueError("segment must be greater than 0")       # api.py:166-170
            self._segment = segment
        if jobs is not None: self._jobs = jobs
        if progress is not None: self._progress = progress
        if callback != -1: self._callback = callback
        if callback_arg != -1: self._callback_arg = callback_arg

    def separate_tensor(self, wav: torch.Tensor, sr: Optional[int] = None) -> Tuple[torch.Tensor, Dict[str, torch.Tensor]]:
        """api.py:241-291.  `wav` (channels, length) float32 is normalised IN PLACE by the mono
        mean / std for the duration of the call and restored before returning."""
        if _is_engine(self._model) and torch.device(self._device).type == "cuda":
            return self._separate_on_device(wav, sr)
        if sr is not None and sr != self._samplerate:
            wav = convert_audio(wav, sr, self._samplerate, self._audio_channels, device=self._device)
        ref = wav.mean(0)
        wav -= ref.mean()
        wav /= ref.std() + 1e-8
        out = apply_model(self._model, wav[None], segment=self._segment, shifts=self._shifts, split=self._split,
                          overlap=self._overlap, device=self._device, num_workers=self._jobs, callback=self._callback,
                          callback_arg=_with(self._callback_arg, audio_length=wav.shape[1]), progress=self._progress)
        if out is None:
            raise KeyboardInterrupt
        out = out.to(wav.device)
        out *= ref.std() + 1e-8
        out += ref.mean()
        wav *= ref.std() + 1e-8
        wav += ref.mean()
        return wav, dict(zip(self._model.sources, out[0]))

    def separate_tensors(self, wavs: Sequence[torch.Tensor], sr: Optional[int] = None
                         ) -> List[Tuple[torch.Tensor, Dict[str, torch.Tensor]]]:
        """`separate_tensor` for many tracks of possibly different lengths: the result equals
        `[self.separate_tensor(w, sr) for w in wavs]`, bit for bit.  Each track gets its own mono statistics and
        normalisation; on the engine the segments of all tracks share batched forwards (`apply_model_many`).  With a
        `callback` or `progress` (whose events follow the reference's per-track order), `split=False`, multi-GPU sharding,
        a model that is not an engine or a non-GPU device, the tracks run one after another.  So do device tracks that share
        storage (`[w, w]`, views of one buffer): a device track is normalised in place, and the packed route normalises every
        track before the first forward, where the loop restores each before the next is read."""
        from . import distributed
        wavs = list(wavs)
        if (not wavs or self._callback is not None or self._progress or not self._split or distributed.sharding_active()
                or not _is_engine(self._model) or torch.device(self._device).type != "cuda"
                or any(w.device != wavs[0].device for w in wavs) or _shared_device_storage(wavs)):
            return [self.separate_tensor(w, sr) for w in wavs]
        device = self._device_index()
        with torch.cuda.device(device):
            states = [self._normalise_on_device(w, sr, device) for w in wavs]
            outs = apply_model_many(self._model, [st[0] for st in states], segment=self._segment, shifts=self._shifts,
                                    split=self._split, overlap=self._overlap, device=device)
            return [self._restore_on_device(st, out[None], device) for st, out in zip(states, outs)]

    def separate_stream(self, mean: Optional[float] = None, std: Optional[float] = None, sr: Optional[int] = None,
                        length: Optional[int] = None, convert: bool = False, channels: Optional[int] = None,
                        deliver: Optional[Delivery] = None, pcm: Optional[str] = None,
                        stats: Optional[TrackStats] = None) -> "SeparatorStream":
        """`separate_tensor` for a track that arrives block by block (demucs_amd/stream.py): `push(block)` takes (channels, n)
        float32 and returns `{source: (channels, m)}` of the newly final samples, `finish()` the rest.

        `separate_tensor` normalises by the whole track's mono mean and std, which a stream cannot know in advance.  Pass
        them (from an earlier analysis pass, or `mi_mono_stats` on a prefix): blocks become `(x - mean) / s` and stems
        `x * s + mean`, s = float32(std) + 1e-8 in float32, and with the track's own statistics the concatenated stems equal
        `separate_tensor`'s bit for bit.  Without them nothing is normalised, which differs from `separate_tensor`.  `length`
        is `apply_model_stream`'s.

        Without `convert=True` the input must already be at the model's sample rate and channel count.  With it, blocks are
        (`channels` or the model's, n) at `sr` and pass through `convert_audio` on the device first (`audio.ConvertStream`:
        mono to the model's channels or the first channels, then the resampler), so the concatenated stems equal
        `separate_tensor(wav, sr)`'s bit for bit; `mean` / `std` are those of the CONVERTED track, `length` counts input samples
        at `sr`, stems come back at the model's rate, and `input_latency` bounds the lag in input samples.

        With `deliver=Delivery(...)` (demucs_amd/stream.py) `push` / `finish` return what the reference would write to its files
        for those samples instead: `{name: (m, channels) frames}` in the order of its save loop, after `prevent_clip` and as
        int16 PCM or float32 with interleaved channels -- `audio.deliver`'s chain on the stems above, by one more launch per
        push.  A stream refuses the spelling other_method="minus" (the residual is `Delivery(mix={"minus_STEM": {"mix": 1,
        STEM: -1}})`, below) and clip="rescale" without peaks: the divisor is the whole output's peak.  `Delivery(clip="rescale", peaks="measure")` is a pass that finds those peaks: `push` returns
        `{}`, nothing is copied to the host, and `finish()` returns an `audio.TrackPeaks`; a second stream over the same input, with
        the same arguments, `random` in the same state and `Delivery(clip="rescale", peaks=<that TrackPeaks>)`, delivers the
        frames of `audio.deliver(..., clip="rescale")` bit for bit (`separate_blocks` runs both).

        `Delivery(..., samplerate=R)` returns the frames at R Hz instead of the model's rate M, resampled on the device:
        `audio.deliver(..., samplerate=(M, R))` on the whole track, bit for bit.  A push returns the resampler frames whose last
        tap the stream has emitted (`delivered` counts them, at most `output_hold` behind floor(new * emitted / old)), `finish()`
        the rest, floor(new * L / old) in all for L samples at M.  With `convert=True` and `samplerate=sr` a feed gets its stems back
        at its own rate; the length then is floor(new' * floor(new * N / old) / old') for N input samples (sr -> M reduces to
        old:new, M -> sr to old':new'), which can be a sample or two short of N: nothing is padded.

        `Delivery(mix={output: {"mix" | source: gain}})` returns gain-weighted remixes of the stems and of the input mix instead
        (vocals lowered rather than removed, `mix - vocals`): `audio.deliver_mix(origin, stems, mix, ...)` on the whole track bit
        for bit, `origin` being the mix as `separate_tensor` hands back a device mix.  The stream reads the mix from its own input
        window (`mi_deliver_mix_pcm` in the delivery launch's place), so nothing is kept for it.  `Delivery(mix=, changes=)` and
        the stream's `change_mix(mix, at=None, ramp=0)` move those gains along the track by steps and linear ramps
        (`audio.deliver_mix(..., changes=)` bit for bit; `mi_deliver_mix_auto_pcm` from the first change on).

        With `pcm=` ("i16", "i24" or "f32") a block is what a socket, a capture device or a WAV file read in pieces delivers:
        little-endian frames with the channels interleaved, as a bytes-like object or a 1-D uint8 tensor that may end anywhere
        (the incomplete last frame waits for the next push; `finish()` drops it, `trailing_bytes` counts it; a device block must
        be whole frames), or an (n, channels) int16 / float32 tensor.  The bytes cross to the device as they are and are
        de-interleaved, converted (`v / 32768`, `v / 8388608`: both exact) and normalised there, so the stems are those of the float
        stream fed the same values, bit for bit.  `length`, `pushed_input`, `latency` and `input_latency` count frames.  With
        `Delivery(fmt="i16")` a stream is then a transcoding loop without host arithmetic: wire frames in, wire frames out.

        `stats=` takes the `audio.TrackStats` that `analyse_stream` returned for the same input in place of `mean` and `std`: the
        affine is its `(mean, s)` as the statistics kernel wrote them, with no further `+ 1e-8`, and `length` defaults to its
        `input_length`.  With the track's own statistics the stems equal `separate_tensor`'s bit for bit."""
        self._check_stream_input(sr, channels, convert, pcm)
        if (mean is None) != (std is None):
            raise ValueError("separate_stream: give both mean and std, or neither")
        if stats is not None:
            if mean is not None:
                raise ValueError("separate_stream: give stats, or mean and std, not both: stats already holds the normaliser "
                                 "s = std + 1e-8")
            if not isinstance(stats, TrackStats):
                raise ValueError(f"separate_stream: stats must be an audio.TrackStats, got {type(stats).__name__}")
            if length is None:
                length = stats.input_length
        plan = self._convert_plan(sr, channels) if convert else None
        if plan is not None and length is not None:
            if int(length) < 0:
                raise ValueError(f"length must be >= 0, got {length}")
            in_length, length = int(length), plan.final_count(int(length))
        st = ModelStream(self._model, shifts=self._shifts, overlap=self._overlap, segment=self._segment, split=self._split,
                         device=self._device, length=length, progress=self._progress, callback=self._callback,
                         affine=None if mean is None else (mean, std), deliver=deliver, pcm=pcm if plan is None else None,
                         stats=stats)
        if plan is None:
            return SeparatorStream(st, self._model.sources)
        return ConvertingSeparatorStream(st, self._model.sources, plan, channels or self._audio_channels,
                                         in_length if length is not None else None, self._device_index, pcm=pcm)

    def _check_stream_input(self, sr: Optional[int], channels: Optional[int], convert: bool, pcm: Optional[str]) -> None:
        """The refusals `separate_stream` and `analyse_stream` share ahead of `_convert_plan` (no device work, no RNG call)."""
        if pcm is not None:                 # refused before any RNG call
            from .audio import check_pcm
            check_pcm(pcm, _is_engine(self._model) and torch.device(self._device).type == "cuda")
        if not convert:
            if channels is not None and channels != self._audio_channels:
                raise ValueError(f"separate_stream: {channels} input channels are not the model's {self._audio_channels}; pass "
                                 "convert=True to convert the channel layout on the stream")
            if sr is not None and sr != self._samplerate:
                raise ValueError(f"separate_stream: input sample rate {sr} is not the model's {self._samplerate}; a stream does not "
                                 "resample unless convert=True")

    def analyse_stream(self, sr: Optional[int] = None, channels: Optional[int] = None, convert: bool = False,
                       pcm: Optional[str] = None):
        """The analysis pass in front of `separate_stream`: a stream whose `push(block)` takes the blocks `separate_stream` takes
        for the same arguments (and refuses what it refuses) and whose `finish()` returns the `audio.TrackStats` of the track --
        the `(mean, s)` that `separate_tensor(wav, sr)` computes internally, with the same bits, for every partition of the
        input.  Device memory is bounded: 4 MiB of carried sums (`audio.MonoStatsStream`), plus the converter's carried samples
        when `convert=True` puts an `audio.ConvertStream` in front.  Read the input twice: once into this stream, once into
        `separate_stream(stats=...)` with the same `sr`, `channels`, `convert` and `pcm`."""
        self._check_stream_input(sr, channels, convert, pcm)
        plan = self._convert_plan(sr, channels) if convert else None
        if plan is None:
            return MonoStatsStream(self._audio_channels, device=self._device, pcm=pcm,
                                   src_channels=None if pcm is None else self._audio_channels)
        return ConvertingStatsStream(plan, self._audio_channels, channels or self._audio_channels, self._device_index(), pcm=pcm)

    def separate_blocks(self, source, sr: Optional[int] = None, channels: Optional[int] = None, pcm: Optional[str] = None,
                        deliver: Optional[Delivery] = None):
        """`separate_tensor(wav, sr)` for a track that never exists whole on the host or the device, read twice: `source()` returns
        a fresh iterator over the track's blocks each time it is called (`separate_stream`'s blocks for `sr`, `channels` and
        `pcm`, converted on the device when they are not the model's).  Pass 1 pushes them through `analyse_stream`, pass 2 through
        `separate_stream(stats=..., length=...)`; this generator yields what every `push` and then `finish` of pass 2 return.
        Concatenated, the stems equal `separate_tensor`'s bit for bit, with `random` left in the same state; with `deliver=` the
        frames equal `audio.deliver`'s on those stems, under a delivering stream's refusals (raised before pass 1).

        `deliver=Delivery(clip="rescale", peaks="measure")` reads the track a third time: between the two passes above a measuring
        `separate_stream` runs the same forwards and keeps only `max |value|` per output on the device (`audio.TrackPeaks`); the
        state of `random` is saved before it and restored after it, so pass 3 draws the same shift offsets, sees the same values
        and divides by the whole track's peaks: the frames are `audio.deliver(..., clip="rescale")`'s bit for bit, and `random`
        ends where `separate_tensor` leaves it.  Nothing but the 4 bytes per output leaves the device in the measuring pass."""
        import random
        if deliver is not None:
            deliver.for_stream(self._model.sources, _is_engine(self._model) and torch.device(self._device).type == "cuda",
                               self._samplerate, self._audio_channels)
        an = self.analyse_stream(sr=sr, channels=channels, convert=True, pcm=pcm)
        for block in source():
            an.push(block)
        stats = an.finish()
        if deliver is not None and deliver.measures:
            state = random.getstate()
            st = self.separate_stream(stats=stats, sr=sr, channels=channels, convert=True, pcm=pcm, deliver=deliver,
                                      length=stats.input_length)
            for block in source():
                st.push(block)
            deliver = deliver.with_peaks(st.finish())
            random.setstate(state)
        st = self.separate_stream(stats=stats, sr=sr, channels=channels, convert=True, pcm=pcm, deliver=deliver,
                                  length=stats.input_length)
        for block in source():
            yield st.push(block)
        yield st.finish()

    def _check_scoring(self, what: str) -> None:
        """The refusals of the scoring entries (no device work, no RNG call): the score kernels have no CPU implementation."""
        if not _is_engine(self._model) or torch.device(self._device).type != "cuda":
            raise ValueError(f"{what} runs on the GPU engines (HTDemucs / HDemucs on a cuda device); score host stems with "
                             "audio.new_sdr instead")
        if not 1 <= len(self._model.sources) <= 8:
            raise ValueError(f"{what}: 1 to 8 sources, the model has {len(self._model.sources)}")

    def evaluate_blocks(self, source, references, sr: Optional[int] = None, channels: Optional[int] = None,
                        pcm: Optional[str] = None, ref_pcm: Optional[str] = None) -> TrackScore:
        """`separate_blocks` with the stems scored instead of returned: the `new_sdr` score (demucs/evaluate.py:30-43, what
        `eval_track(..., compute_sdr=False)` computes) of a track that never exists whole on the host or the device, against
        reference stems that arrive block by block.  `source` is `separate_blocks`' argument; `references()` returns an iterator
        over blocks of the reference stems for the same track, at the model's sample rate and channel count: (sources, channels,
        n) floating tensors in the model's source order, or with `ref_pcm=` lists of one interleaved PCM chunk per source
        (`audio.SdrStream`).  Their block sizes need not match the mix's.  Every span pass 2 emits and every reference block goes
        into an `audio.SdrStream`; references are read only as far as the stems have come, so the surplus the stream holds stays
        below a block of either kind.  Returns the `audio.TrackScore`, with the bits of
        `audio.new_sdr(refs[None], stems[None])[0]` for `stems` = `separate_tensor(wav, sr)`'s stacked in source order, and
        `random` left as `separate_blocks` leaves it.

        Host mix blocks are uploaded here (PCM bytes as they are, an incomplete frame carried to the next block), so the stream
        emits device stems, the kernel reads them where they lie and no float stem visits the host.

        Normalisation: the reference's `evaluate` normalises the mix by `ref.std()`, a `Separator` by `ref.std() + 1e-8`; this
        method is the `Separator`'s chain (`separate_tensor`'s stems), so on a silent track the two differ."""
        from .audio import PcmFeed, SdrStream
        self._check_scoring("evaluate_blocks")
        if ref_pcm is not None:
            from .audio import check_pcm
            check_pcm(ref_pcm)
        self._check_stream_input(sr, channels, True, pcm)
        self._convert_plan(sr, channels)
        device = self._device_index()
        src_channels = channels or self._audio_channels

        def on_device():
            feed = PcmFeed(pcm, src_channels) if pcm is not None else None
            for block in source():
                if feed is not None:
                    blk = feed.accept(block)
                    feed.commit(blk)
                    with torch.cuda.device(device):
                        yield blk.on_device(device, [])[:blk.nbytes]
                elif isinstance(block, torch.Tensor):
                    yield block.to(device)
                else:
                    yield block                            # refused by the stream, with its message

        score = SdrStream(len(self._model.sources), self._audio_channels, device=device, pcm=ref_pcm,
                          src_channels=None if ref_pcm is None else self._audio_channels)
        refs = iter(references())
        for out in self.separate_blocks(on_device, sr=sr, channels=channels, pcm=pcm):
            score.push_estimates(_stacked(list(out.values())))
            while score.references_pushed < score.estimates_pushed:
                block = next(refs, None)
                if block is None:
                    break
                score.push_references(block)
        for block in refs:
            score.push_references(block)
        return score.finish()

    def score_tensor(self, wav: torch.Tensor, references: torch.Tensor, sr: Optional[int] = None):
        """The whole-track counterpart of `evaluate_blocks`: `separate_tensor(wav, sr)` followed by `audio.new_sdr` against
        `references` (sources, channels, length) on the device.  A host `wav` is uploaded first, so the stems are scored where the
        engine leaves them and cross to the host once, as `separate_tensor` returns them.  Returns `(TrackScore, stems)`."""
        from .audio import sdr_sums
        self._check_scoring("score_tensor")
        if references.dim() != 3 or tuple(references.shape[:2]) != (len(self._model.sources), self._audio_channels):
            raise ValueError(f"score_tensor: references must be ({len(self._model.sources)}, {self._audio_channels}, length), got "
                             f"{tuple(references.shape)}")
        device = self._device_index()
        host_in = wav.device.type == "cpu"
        with torch.cuda.device(device):
            _, stems = self.separate_tensor(wav.to(device) if host_in else wav, sr)
            est = _stacked(list(stems.values()))
            if references.dim() != 3 or references.shape != est.shape:
                raise ValueError(f"score_tensor: references {tuple(references.shape)} are not the stems' {tuple(est.shape)}")
            score = TrackScore.from_sums(sdr_sums(references[None], est[None])[0], est.shape[-1])
            if host_in:
                stems = dict(zip(stems, _to_host(est[None], device)[0]))
        return score, stems

    def _check_loudness(self, what: str, mix):
        """The refusals of the loudness entries (no device work, no RNG call) and the remixes they measure: `mix` as
        `audio.deliver_mix` takes it; None is every source by itself and the mix as output "mix"."""
        from .audio import _check_loudness_format, mix_gains
        if not _is_engine(self._model) or torch.device(self._device).type != "cuda":
            raise ValueError(f"{what} runs on the GPU engines (HTDemucs / HDemucs on a cuda device); there is no CPU meter in this "
                             "package")
        sources = list(self._model.sources)
        if not 1 <= len(sources) <= 8:
            raise ValueError(f"{what}: 1 to 8 sources, the model has {len(sources)}")
        _check_loudness_format(self._samplerate, self._audio_channels)
        if mix is None:
            mix = {**{name: {name: 1.0} for name in sources}, "mix": {"mix": 1.0}}
        return mix, any(g[0] != 0 for _, g in mix_gains(mix, sources))

    def loudness_tensor(self, wav: torch.Tensor, mix=None, sr: Optional[int] = None
                        ) -> Tuple[TrackLoudness, torch.Tensor, Dict[str, torch.Tensor]]:
        """`separate_tensor(wav, sr)` followed by `audio.loudness` where the stems lie: ITU-R BS.1770-4 loudness of the
        gain-weighted remixes `mix` (`audio.deliver_mix`'s `{output: {"mix" | source: gain}}`; None: every source by itself and
        the mix) without a float stem crossing to the host for it.  Returns `(TrackLoudness, origin, stems)`, `origin` and `stems`
        as `separate_tensor` returns them -- a host `wav` is uploaded first and the stems cross to the host once -- and the
        `TrackLoudness` that of `audio.loudness(origin, stems, mix)` on exactly those: for a host `wav` the mix as given (or as
        converted from `sr`), for a device `wav` the mix as `separate_tensor` leaves it after normalising and restoring it in
        place."""
        from .audio import loudness
        mix, _ = self._check_loudness("loudness_tensor", mix)
        return self._meter_tensor(wav, mix, sr, [loudness])

    def loudness_blocks(self, source, mix=None, sr: Optional[int] = None, channels: Optional[int] = None,
                        pcm: Optional[str] = None) -> TrackLoudness:
        """`separate_blocks` with the loudness of remixes measured instead of stems returned: the `audio.TrackLoudness` of a track
        that never exists whole on the host or the device, with the bits of `loudness_tensor(wav, mix, sr)` for a host `wav`.
        `source` is `separate_blocks`' argument, read twice (the analysis pass, the separating pass); host blocks are uploaded
        here, so the stream emits device stems and every emitted span goes into an `audio.LoudnessStream` where it lies.  When an
        output has a gain on "mix" the blocks of the second pass also go through `audio.convert_audio_stream` (straight through
        when they already are what the model takes), which has `convert_audio`'s bits; the model-rate mix waits in a queue until
        the stems of its positions arrive, at most one segment plus one block of it.

        The state of `random` is saved on entry and restored on exit, as the measuring pass of `separate_blocks` does: a following
        `separate_blocks(source, deliver=Delivery(mix=result.normalised(-14), clip="clamp"))` draws the same shift offsets and
        delivers the remixes that were measured, each at -14 LUFS."""
        from .audio import LoudnessStream
        mix, mixed = self._check_loudness("loudness_blocks", mix)
        return self._meter_blocks(source, mix, mixed, sr, channels, pcm, [LoudnessStream])[0]

    def _check_levels(self, what: str, mix):
        """`_check_loudness` and the true-peak meter's own refusal."""
        from .audio import _check_true_peak_format
        checked = self._check_loudness(what, mix)
        _check_true_peak_format(self._samplerate, self._audio_channels)
        return checked

    def levels_tensor(self, wav: torch.Tensor, mix=None, sr: Optional[int] = None
                      ) -> Tuple[TrackLoudness, TrackTruePeaks, torch.Tensor, Dict[str, torch.Tensor]]:
        """`loudness_tensor` with the second meter of EBU R 128 beside the first: one separation, then `audio.loudness` and
        `audio.true_peak` (BS.1770-4 Annex 2) where the stems lie.  Returns `(TrackLoudness, TrackTruePeaks, origin, stems)`;
        `loudness.normalised(-14, true_peaks=peaks)` is the `mix` that delivers every remix at -14 LUFS or, where its peaks do
        not allow that, at -1 dBTP."""
        from .audio import loudness, true_peak
        mix, _ = self._check_levels("levels_tensor", mix)
        return self._meter_tensor(wav, mix, sr, [loudness, true_peak])

    def levels_blocks(self, source, mix=None, sr: Optional[int] = None, channels: Optional[int] = None,
                      pcm: Optional[str] = None) -> Tuple[TrackLoudness, TrackTruePeaks]:
        """`loudness_blocks` with both meters fed by one separating pass: `(TrackLoudness, TrackTruePeaks)` with the bits of
        `levels_tensor(wav, mix, sr)` for a host `wav`.  Every emitted span goes into an `audio.LoudnessStream` and an
        `audio.TruePeakStream` where it lies; the state of `random` is restored on exit as `loudness_blocks` restores it."""
        from .audio import LoudnessStream, TruePeakStream
        mix, mixed = self._check_levels("levels_blocks", mix)
        loud, peaks = self._meter_blocks(source, mix, mixed, sr, channels, pcm, [LoudnessStream, TruePeakStream])
        return loud, peaks

    def _meter_tensor(self, wav: torch.Tensor, mix, sr: Optional[int], meters):
        """`separate_tensor(wav, sr)` followed by every whole-track meter of `meters` (`audio.loudness`'s arguments) on the same
        mix and stems: `(*results, origin, stems)`, `origin` and `stems` as `loudness_tensor` documents them."""
        device = self._device_index()
        host_in = wav.device.type == "cpu"
        with torch.cuda.device(device):
            dev = wav.to(device) if host_in else wav
            converted = sr is not None and sr != self._samplerate
            if converted:
                dev = convert_audio(dev, sr, self._samplerate, self._audio_channels, device=device)
            raw = dev.clone() if host_in else None               # the forward normalises its input in place
            origin, stems = self.separate_tensor(dev, None)
            measured = [meter(raw if host_in else origin, stems, mix, self._samplerate) for meter in meters]
            if host_in:
                stems = dict(zip(stems, _to_host(_stacked(list(stems.values()))[None], device)[0]))
                origin = _to_host(raw, device) if converted else wav
        return (*measured, origin, stems)

    def _meter_blocks(self, source, mix, mixed: bool, sr: Optional[int], channels: Optional[int], pcm: Optional[str], meters) -> list:
        """The two passes of `loudness_blocks` with every emitted span pushed into each of the stream meters that `meters`
        constructs (`audio.LoudnessStream`'s arguments and interface); returns what their `finish()` return, in order."""
        import random
        from .audio import ConvertStream, PcmFeed
        self._check_stream_input(sr, channels, True, pcm)
        plan = self._convert_plan(sr, channels)
        device = self._device_index()
        src_channels = channels or self._audio_channels

        def on_device():
            feed = PcmFeed(pcm, src_channels) if pcm is not None else None
            for block in source():
                if feed is not None:
                    blk = feed.accept(block)
                    feed.commit(blk)
                    with torch.cuda.device(device):
                        yield blk.on_device(device, [])[:blk.nbytes]
                elif isinstance(block, torch.Tensor):
                    yield block.to(device)
                else:
                    yield block                            # refused by the stream, with its message

        state = random.getstate()
        try:
            an = self.analyse_stream(sr=sr, channels=channels, convert=True, pcm=pcm)
            for block in on_device():
                an.push(block)
            stats = an.finish()
            st = self.separate_stream(stats=stats, sr=sr, channels=channels, convert=True, pcm=pcm, length=stats.input_length)
            streams = [meter(self._model.sources, self._audio_channels, self._samplerate, mix, device=device) for meter in meters]
            convert = None
            if mixed and (plan is not None or pcm is not None):
                convert = ConvertStream(sr or self._samplerate, self._samplerate, self._audio_channels, device=device, plan=plan,
                                        pcm=pcm, src_channels=src_channels if pcm is not None else None)
            queue = []

            def measure(out):
                stems = _stacked(list(out.values()))
                need, parts = stems.shape[-1], []
                while mixed and need:
                    head = queue[0]
                    k = min(need, head.shape[1])
                    parts.append(head[:, :k])
                    if k == head.shape[1]:
                        queue.pop(0)
                    else:
                        queue[0] = head[:, k:]
                    need -= k
                origin = None if not mixed else parts[0] if len(parts) == 1 else torch.cat(parts, 1) if parts else \
                    stems.new_empty(self._audio_channels, 0)
                for meter in streams:
                    meter.push(stems, origin)

            for block in on_device():
                if mixed:
                    queue.append(block if convert is None else convert.push(block, on_device=True))
                measure(st.push(block))
            if convert is not None:
                queue.append(convert.finish(on_device=True))
            measure(st.finish())
            return [meter.finish() for meter in streams]
        finally:
            random.setstate(state)

    def _convert_plan(self, sr: Optional[int], channels: Optional[int]):
        """The refusals of a converting stream (before any device work or RNG call) and its `audio.ConvertPlan`; None when the
        input is already what the model takes."""
        from .audio import ConvertPlan, check_stream_channels
        sr = self._samplerate if sr is None else sr
        src_channels = self._audio_channels if channels is None else channels
        if int(sr) != sr or sr <= 0:
            raise ValueError(f"separate_stream: the sample rate must be a positive integer, got {sr}")
        check_stream_channels(int(src_channels), self._audio_channels)
        if int(sr) == self._samplerate and src_channels == self._audio_channels:
            return None
        if not _is_engine(self._model) or torch.device(self._device).type != "cuda":
            raise ValueError("separate_stream: convert=True runs on the GPU engines (HTDemucs / HDemucs on a cuda device); there is "
                             "no CPU resampler in this package")
        return ConvertPlan(int(sr), self._samplerate)

    def separate_stream_group(self) -> "SeparatorStreamGroup":
        """Many `separate_stream`s of this separator's model at once (demucs_amd/stream.py, `StreamGroup`): `open(mean, std,
        length, sr, channels)` starts a stream with `separate_stream`'s normalisation rule and returns its key,
        `push({key: block})` and `finish(keys)` return `{key: {source: (channels, m)}}`.  A stream opened with an `sr` or a
        channel count that is not the model's converts on the device as `separate_stream(convert=True)` does, each stream with
        its own rate; the others must already be at the model's sample rate and channel count."""
        g = StreamGroup(self._model, shifts=self._shifts, overlap=self._overlap, segment=self._segment, split=self._split,
                        device=self._device, progress=self._progress, callback=self._callback)
        return SeparatorStreamGroup(g, self._model.sources, self)

    def _device_index(self) -> torch.device:
        device = torch.device(self._device)
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        return device

    def _separate_on_device(self, wav: torch.Tensor, sr: Optional[int]):
        """The engine's `separate_tensor` (module docstring): everything between the one H2D and the one D2H runs on the GPU."""
        device = self._device_index()
        with torch.cuda.device(device):
            st = self._normalise_on_device(wav, sr, device)
            dev, length = st[0], st[0].shape[1]
            out = apply_model(self._model, dev[None], segment=self._segment, shifts=self._shifts, split=self._split,
                              overlap=self._overlap, device=device, num_workers=self._jobs, callback=self._callback,
                              callback_arg=_with(self._callback_arg, audio_length=length), progress=self._progress)
            if out is None:
                raise KeyboardInterrupt
            return self._restore_on_device(st, out, device)

    def _normalise_on_device(self, wav: torch.Tensor, sr: Optional[int], device: torch.device):
        """One H2D of a host `wav`, the resampler when `sr` differs, then `(x - mean) / (std + 1e-8)` on the device copy.
        Returns (normalised track, stats, wav as handed back, restore copy or None, host_in)."""
        lib = _lib.load()
        host_in = wav.device.type == "cpu"
        stream = lambda: C.c_void_p(_lib.current_stream_ptr())          # noqa: E731
        dev = wav.to(device=device, dtype=torch.float32, non_blocking=True) if host_in else wav
        if sr is not None and sr != self._samplerate:
            dev = convert_audio(dev, sr, self._samplerate, self._audio_channels, device=device)
            if host_in:
                wav = None                    # the reference returns the converted tensor: handed back from the device below
        if not dev.is_contiguous() or dev.dtype != torch.float32:
            dev = dev.contiguous().float()
        channels, length = dev.shape
        scratch = torch.empty(lib.mi_mono_stats_scratch_bytes(), dtype=torch.uint8, device=device)
        stats = torch.empty(2, dtype=torch.float32, device=device)
        _lib.check(lib.mi_mono_stats(dev.data_ptr(), channels, length, scratch.data_ptr(), stats.data_ptr(), stream()),
                   "mi_mono_stats")
        restore = dev.clone() if (host_in and wav is None) else None       # resampled host input: returned un-normalised
        _lib.check(lib.mi_track_affine(dev.data_ptr(), dev.numel(), stats.data_ptr(), 0, stream()), "mi_track_affine")
        return dev, stats, wav, restore, host_in

    def _restore_on_device(self, st, out: torch.Tensor, device: torch.device):
        """`x * std + mean` on the (1, S, channels, length) stems (and on a device `wav`), ONE D2H for a host input."""
        lib = _lib.load()
        dev, stats, wav, restore, host_in = st
        stream = lambda: C.c_void_p(_lib.current_stream_ptr())          # noqa: E731
        out = out.contiguous()
        _lib.check(lib.mi_track_affine(out.data_ptr(), out.numel(), stats.data_ptr(), 1, stream()), "mi_track_affine")
        if host_in:
            stems = _to_host(out, device)
            if wav is None:
                wav = _to_host(restore, device)
        else:
            _lib.check(lib.mi_track_affine(dev.data_ptr(), dev.numel(), stats.data_ptr(), 1, stream()), "mi_track_affine")
            stems, wav = out, dev
        return wav, dict(zip(self._model.sources, stems[0]))

    @property
    def samplerate(self):
        return self._samplerate

    @property
    def audio_channels(self):
        return self._audio_channels

    @property
    def model(self):
        return self._model


def _named(sources, out) -> Dict[str, torch.Tensor]:
    """A stream's stems by source name; a delivering stream's result already is `{name: frames}`, a measuring stream's `{}` or
    its `audio.TrackPeaks`."""
    return out if isinstance(out, (dict, TrackPeaks)) else dict(zip(sources, out))


def _stacked(stems) -> torch.Tensor:
    """The per-source (channels, n) stems as one (sources, channels, n) tensor: the block they were cut from, without a copy, when
    they still lie one behind the other in it (what a stream and `separate_tensor` return), else their stack."""
    first = stems[0]
    if first.numel() and first.is_contiguous() and all(
            t.shape == first.shape and t.dtype == first.dtype and t.device == first.device and t.is_contiguous()
            and t.untyped_storage().data_ptr() == first.untyped_storage().data_ptr()
            and t.data_ptr() == first.data_ptr() + i * first.numel() * first.element_size() for i, t in enumerate(stems)):
        return first.as_strided((len(stems), *first.shape), (first.numel(), *first.stride()))
    return torch.stack(list(stems))


class SeparatorStream:
    """What `Separator.separate_stream` returns: the stream's stems as `{source: (channels, m)}`."""

    def __init__(self, stream, sources):
        self.stream, self.sources = stream, list(sources)

    def push(self, block: torch.Tensor) -> Dict[str, torch.Tensor]:
        return _named(self.sources, self.stream.push(block))

    def finish(self) -> Dict[str, torch.Tensor]:
        return _named(self.sources, self.stream.finish())

    def change_mix(self, mix, at=None, ramp=0) -> None:
        """Moves the gains of a `Delivery(mix=)` stream's outputs named in `mix` to the given ones from delivered frame `at` (None:
        as soon as nothing delivered is contradicted) over `ramp` frames; see `ModelStream.change_mix`."""
        self.stream.change_mix(mix, at=at, ramp=ramp)

    @property
    def emitted(self) -> int:
        return self.stream.emitted

    @property
    def latency(self) -> int:
        return self.stream.latency

    @property
    def trailing_bytes(self) -> int:
        """Bytes of an incomplete last frame of a `pcm=` stream: carried to the next push, dropped by `finish()`."""
        return self.stream.trailing_bytes

    @property
    def delivered(self) -> int:
        """Frames returned so far by a stream that delivers at another sample rate (`Delivery(samplerate=R)`), at R."""
        return self.stream.delivered

    @property
    def output_hold(self) -> int:
        """Bound of floor(new * emitted / old) - delivered for such a stream; some push reaches it."""
        return self.stream.output_hold


class ConvertingSeparatorStream(SeparatorStream):
    """`Separator.separate_stream(convert=True)`: an `audio.ConvertStream` on the device in front of the model's stream.
    `emitted` and `latency` count samples at the model's rate, `pushed_input` and `input_latency` input samples:
    after every push `pushed_input - ceil(emitted * old / new) <= input_latency = width + old - 1 + floor(latency * old / new)`
    (old / new the rates divided by their gcd): the converter holds back at most `width + old - 1` input samples and the model's
    stream `latency` of its own; a push that meets both bounds at once reaches it."""

    def __init__(self, stream, sources, plan, src_channels, in_length, device_index, pcm=None):
        super().__init__(stream, sources)
        self.plan, self.src_channels, self.in_length = plan, int(src_channels), in_length
        self.pcm, self.feed = pcm, None
        if pcm is not None:
            from .audio import PcmFeed
            self.feed = PcmFeed(pcm, self.src_channels)
        self.input_latency = plan.width + plan.old - 1 + stream.latency * plan.old // plan.new
        self.pushed_input = 0
        self._device_index = device_index
        self._cv = None

    def push(self, block: torch.Tensor) -> Dict[str, torch.Tensor]:
        if self.stream.finished:
            raise RuntimeError("push after finish()")
        if self.feed is not None:
            block = self.feed.accept(block)                # whole frames of wire PCM; the converter reads them as they are
        elif not isinstance(block, torch.Tensor) or block.dim() != 2 or block.shape[0] != self.src_channels:
            shape = tuple(block.shape) if isinstance(block, torch.Tensor) else type(block).__name__
            raise ValueError(f"expected a ({self.src_channels}, n) block, got {shape}")
        if self.in_length is not None and self.pushed_input + block.shape[1] > self.in_length:
            raise ValueError(f"pushed {self.pushed_input + block.shape[1]} samples, more than the declared length {self.in_length}")
        if self.feed is not None:
            self.feed.commit(block)
        if self._cv is None:
            from .audio import ConvertStream
            self._cv = ConvertStream(None, None, self.stream.audio_channels, device=self._device_index(), plan=self.plan,
                                     pcm=self.pcm, src_channels=self.src_channels if self.pcm is not None else None)
        y = self._cv.push(block, on_device=True)
        self.pushed_input = self._cv.pushed
        return self._stems(self.stream.push(y), block.device)

    def finish(self) -> Dict[str, torch.Tensor]:
        if self.stream.finished:
            raise RuntimeError("finish() called twice")
        if self.in_length is not None and self.pushed_input != self.in_length:
            raise ValueError(f"the stream ended after {self.pushed_input} samples, but length={self.in_length} was declared")
        if self._cv is None or self.pushed_input == 0:
            raise ValueError("the stream ended before any sample was pushed")
        to = self._cv._out_device
        y = self._cv.finish(on_device=True)
        parts = [self.stream.push(y)] if y.shape[1] else []
        parts.append(self.stream.finish())
        if isinstance(parts[-1], TrackPeaks):               # a measuring stream: every push gave {}
            return parts[-1]
        if isinstance(parts[0], dict):                      # delivered frames: (m, channels) per name
            return self._stems({k: torch.cat([p[k] for p in parts], 0) for k in parts[0]}, to)
        return self._stems(parts[0] if len(parts) == 1 else torch.cat(parts, -1), to)

    @property
    def trailing_bytes(self) -> int:
        return 0 if self.feed is None else self.feed.trailing_bytes

    def _stems(self, out, to) -> Dict[str, torch.Tensor]:
        host = to is not None and torch.device(to).type == "cpu"
        if isinstance(out, dict):
            return out if to is None else {k: v.to(to) for k, v in out.items()}
        if host:
            out = _to_host(out, out.device)
        return dict(zip(self.sources, out))

    def device_bytes(self) -> int:
        return self.stream.device_bytes() + (0 if self._cv is None else self._cv.device_bytes())


class SeparatorStreamGroup:
    """What `Separator.separate_stream_group` returns: every stream's stems as `{key: {source: (channels, m)}}`."""

    def __init__(self, group, sources, separator=None):
        self.group, self.sources, self.separator = group, list(sources), separator

    def open(self, mean: Optional[float] = None, std: Optional[float] = None, length: Optional[int] = None,
             sr: Optional[int] = None, channels: Optional[int] = None, deliver: Optional[Delivery] = None,
             pcm: Optional[str] = None, stats: Optional[TrackStats] = None):
        """`length`, `sr` and `channels` describe the stream's INPUT, as for `separate_stream(convert=True)`; `deliver` and `pcm`
        are `separate_stream`'s, each stream with its own: a group may mix float, int16, int24 and float32 PCM feeds, and a call
        stays one append launch, one convert-append launch and one H2D.  `stats=` (an `audio.TrackStats`, from `analyse_stream`)
        replaces `mean` and `std` as in `separate_stream`; `length` then defaults to its `input_length`."""
        if pcm is not None:
            from .audio import check_pcm
            check_pcm(pcm, _is_engine(self.separator.model) and torch.device(self.separator._device).type == "cuda")
        if (mean is None) != (std is None):
            raise ValueError("separate_stream_group: give both mean and std, or neither")
        if stats is not None and mean is not None:
            raise ValueError("separate_stream_group: give stats, or mean and std, not both: stats already holds the normaliser "
                             "s = std + 1e-8")
        convert = None
        if sr is not None or channels is not None:
            plan = self.separator._convert_plan(sr, channels)
            if plan is not None:
                convert = (plan, int(channels or self.separator.audio_channels))
        return self.group.open(length=length, affine=None if mean is None else (mean, std), convert=convert, deliver=deliver,
                               pcm=pcm, channels=None if convert is not None else channels, stats=stats)

    def trailing_bytes(self, key) -> int:
        return self.group.trailing_bytes(key)

    def push(self, blocks) -> Dict[object, Dict[str, torch.Tensor]]:
        return {k: _named(self.sources, v) for k, v in self.group.push(blocks).items()}

    def finish(self, keys) -> Dict[object, Dict[str, torch.Tensor]]:
        return {k: _named(self.sources, v) for k, v in self.group.finish(keys).items()}

    def emitted(self, key) -> int:
        return self.group.emitted(key)

    def change_mix(self, key, mix, at=None, ramp=0) -> None:
        """`SeparatorStream.change_mix` for stream `key`."""
        self.group.change_mix(key, mix, at=at, ramp=ramp)

    def delivered(self, key) -> int:
        return self.group.delivered(key)

    @property
    def latency(self) -> int:
        return self.group.latency

    @property
    def open_keys(self) -> list:
        return self.group.open_keys


def list_models(repo: Optional[Union[str, Path]] = None) -> Dict[str, Dict[str, Union[str, Path]]]:
    """api.py:322-347: `{"single": {signature: package path}, "bag": {name: yaml path}}` of a local model folder.  Without `repo`
    the reference lists its remote zoo (`remote/files.txt` + the bag YAMLs it ships); offline only `demucs_unittest`, the one
    model that needs no download (pretrained.py:27-29), can be named."""
    if repo is None:
        return {"single": {"demucs_unittest": "built in (HDemucs(channels=4), pretrained.py:27-29)"}, "bag": {}}
    from .states import LocalRepo
    repo = Path(repo)
    if not repo.is_dir():
        raise LoadModelError(f"{repo} must exist and be a directory.")
    local = LocalRepo(repo)
    return {"single": dict(local._models), "bag": dict(local._bags)}
