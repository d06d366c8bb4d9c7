"""`demucs.audio.convert_audio` for the MI355X engine (demucs/audio.py:137-172): channel conversion on the
host tensor, fractional sinc resampling (`julius.resample_frac`) as a HIP kernel.

julius is a pinned dependency of the reference (requirements.txt: julius>=0.2.3) that is neither vendored in
/root/reference nor installable here, so its algorithm is restated from the published source (julius/resample.py,
ResampleFrac: zeros=24, rolloff=0.945, cos^2-windowed sinc bank of new_sr phases, replicate padding, stride old_sr):
PARITY UNPINNED — checked against `oracle/resample_oracle.py` (the same restatement with torch conv1d) and against
analytic properties (identity at equal rates, sine amplitude / frequency preservation), not against julius itself.
"""
import ctypes as C
import math
from functools import lru_cache

import torch

from . import _lib

ZEROS = 24
ROLLOFF = 0.945


def convert_audio_channels(wav: torch.Tensor, channels: int = 2) -> torch.Tensor:
    """demucs/audio.py:137-166."""
    *shape, src_channels, length = wav.shape
    if src_channels == channels:
        pass
    elif channels == 1:
        wav = wav.mean(dim=-2, keepdim=True)
    elif src_channels == 1:
        wav = wav.expand(*shape, channels, length)
    elif src_channels >= channels:
        wav = wav[..., :channels, :]
    else:
        raise ValueError('The audio file has less channels than requested but is not mono.')
    return wav


@lru_cache(maxsize=16)
def sinc_bank(old_sr: int, new_sr: int, zeros: int = ZEROS, rolloff: float = ROLLOFF):
    """(width, kernels (new_sr, 2*width + old_sr) float32) of julius.ResampleFrac._init_kernels for REDUCED rates."""
    sr = min(new_sr, old_sr) * rolloff
    width = math.ceil(zeros * old_sr / sr)
    idx = torch.arange(-width, width + old_sr).float()
    kernels = []
    for i in range(new_sr):
        t = (-i / new_sr + idx / old_sr) * sr
        t = t.clamp_(-zeros, zeros)
        t *= math.pi
        window = torch.cos(t / zeros / 2) ** 2
        kernel = torch.where(t == 0, torch.tensor(1.0), torch.sin(t) / t) * window
        kernel.div_(kernel.sum())
        kernels.append(kernel)
    return width, torch.stack(kernels).contiguous()


def resample_frac(x: torch.Tensor, old_sr: int, new_sr: int, device="cuda") -> torch.Tensor:
    """`julius.resample_frac(x, old_sr, new_sr)` (default output length floor(new_sr * L / old_sr)) computed on `device`
    by the HIP kernel; the result comes back on x.device.  There is no CPU implementation in this package."""
    gcd = math.gcd(int(old_sr), int(new_sr))
    old, new = int(old_sr) // gcd, int(new_sr) // gcd
    if old == new:
        return x
    dev = torch.device(device)
    if dev.type != "cuda":
        raise _lib.EngineError("demucs_amd.audio.resample_frac only runs on a GPU device (MI355X)")
    width, bank = sinc_bank(old, new)
    shape, length = x.shape, x.shape[-1]
    out_len = int(math.floor(new * length / old))
    xs = x.reshape(-1, length).to(dev, torch.float32).contiguous()
    y = torch.empty(xs.shape[0], out_len, device=dev, dtype=torch.float32)
    if out_len > 0:
        table = bank.to(dev)
        with torch.cuda.device(dev):
            _lib.check(_lib.load().mi_resample_frac(xs.data_ptr(), xs.shape[0], length, table.data_ptr(), old, new, width, y.data_ptr(),
                                                    out_len, C.c_void_p(_lib.current_stream_ptr())), "mi_resample_frac")
    return y.reshape(list(shape[:-1]) + [out_len]).to(x.device)


def convert_audio(wav: torch.Tensor, from_samplerate: int, to_samplerate: int, channels: int, device="cuda") -> torch.Tensor:
    """demucs/audio.py:169-172."""
    wav = convert_audio_channels(wav, channels)
    return resample_frac(wav, from_samplerate, to_samplerate, device)


# ---- convert_audio for a stream: the same float32 chain per output, whatever the partition of the input ------------------
CVT_COLS = 20                      # include/demucs_amd.h: MI_CVT_*
CVT_LDS_FLOATS = 16384             # MI_CVT_LDS_FLOATS: the kernel's LDS staging area (64 KiB)
CVT_FRAMES, CVT_SUBRUNS, CVT_COPY_SPAN = 8, 4, 1024


def check_stream_channels(src_channels: int, channels: int) -> None:
    """`convert_audio_channels`' cases that a stream takes: the three per-sample ones."""
    if src_channels < 1:
        raise ValueError(f"a block needs at least one channel, got {src_channels}")
    if src_channels == channels or src_channels == 1:
        return
    if channels == 1:
        raise ValueError("a stream does not down-mix to mono (the mean over channels): convert the input before pushing it")
    if src_channels < channels:
        raise ValueError('The audio file has less channels than requested but is not mono.')


# ---- wire PCM in: what a socket, a capture device or a WAV file read in pieces delivers (demucs_amd/csrc/ingest.hip) ------------
PCM_PLANAR = 0                                  # include/demucs_amd.h: MI_PCM_PLANAR, a planar float32 row of a PCM table
# name -> (MI_PCM_* code, bytes per sample, dtype of an (n, channels) tensor block or None); little-endian, channels interleaved
PCM_FORMATS = {"i16": (1, 2, torch.int16), "i24": (2, 3, None), "f32": (3, 4, torch.float32)}
APPEND_PCM_COLS, CVT_PCM_COLS = 8, 21           # MI_APPEND_PCM_COLS, MI_CVT_PCM_COLS


def check_pcm(pcm, engine: bool = True) -> None:
    """The refusals of a PCM stream that need no block (no device work, no RNG call)."""
    if pcm not in PCM_FORMATS:
        raise ValueError(f"Invalid PCM format {pcm!r}: 'i16', 'i24' or 'f32'")
    if not engine:
        raise ValueError("a PCM stream runs on the GPU engines (HTDemucs / HDemucs on a cuda device); there is no CPU "
                         "implementation of the ingest kernels in this package")


class PcmBlock:
    """The whole frames of one push of a PCM stream: `n` frames of `src_channels` channels, as host byte pieces (the carried
    bytes, then the block's) or as one uint8 device tensor.  `shape` is the planar block's, so a scheduler counts it as one."""

    def __init__(self, fmt: str, src_channels: int, n: int, pieces=None, dev=None, carry: bytes = b""):
        self.fmt, self.src_channels, self.n, self.pieces, self.dev, self.carry = fmt, src_channels, n, pieces, dev, carry
        self.code, self.width, _ = PCM_FORMATS[fmt]
        self.shape = (src_channels, n)
        self.nbytes = n * src_channels * self.width
        self.device = torch.device("cpu") if dev is None else dev.device

    def stage(self, host) -> None:
        """The host pieces into `host`, a numpy uint8 view of `nbytes` bytes of a pinned buffer."""
        at = 0
        for p in self.pieces:
            host[at:at + len(p)] = p
            at += len(p)

    def on_device(self, dev, keep: list) -> torch.Tensor:
        """The frames as a uint8 tensor on `dev`: a device block where it is, a host block by one H2D from a pinned copy."""
        if self.dev is not None:
            return self.dev if self.dev.device == torch.device(dev) else self.dev.to(dev)
        host = torch.empty(max(1, self.nbytes), dtype=torch.uint8, pin_memory=True)
        self.stage(host.numpy()[:self.nbytes])
        raw = torch.empty(max(1, self.nbytes), dtype=torch.uint8, device=dev)
        raw.copy_(host, non_blocking=True)
        keep += [host, raw]
        return raw


class PcmFeed:
    """The host side of a PCM stream (no device work): it cuts a byte stream that stops wherever the transport stopped into whole
    frames.  The incomplete trailing frame of a host chunk, at most `frame_bytes - 1` bytes, is carried and goes in front of the
    next; `trailing_bytes` counts the carried bytes, which a finished stream drops as a decoder does.  `accept` validates a block
    and changes nothing; `commit` makes its carry the feed's."""

    def __init__(self, fmt: str, src_channels: int):
        check_pcm(fmt)
        if int(src_channels) != src_channels or src_channels < 1:
            raise ValueError(f"a block needs at least one channel, got {src_channels}")
        self.fmt, self.src_channels = fmt, int(src_channels)
        self.frame_bytes = self.src_channels * PCM_FORMATS[fmt][1]
        self.carry = b""

    @property
    def trailing_bytes(self) -> int:
        return len(self.carry)

    def _refuse(self, block):
        dtype = PCM_FORMATS[self.fmt][2]
        typed = "" if dtype is None else f", or an (n, {self.src_channels}) {dtype} tensor"
        got = f"{tuple(block.shape)} {block.dtype}" if isinstance(block, torch.Tensor) else type(block).__name__
        return ValueError(f"expected a block of {self.fmt!r} PCM: bytes, bytearray, memoryview or a 1-D torch.uint8 tensor{typed}; "
                          f"got {got}")

    def accept(self, block) -> PcmBlock:
        import numpy as np
        frame, width = self.frame_bytes, PCM_FORMATS[self.fmt][1]
        if isinstance(block, torch.Tensor):
            if block.dim() == 2 and block.dtype == PCM_FORMATS[self.fmt][2] and block.shape[1] == self.src_channels:
                raw = block.contiguous().view(torch.uint8).reshape(-1)
            elif block.dim() == 1 and block.dtype == torch.uint8:
                raw = block.contiguous()
            else:
                raise self._refuse(block)
            if raw.device.type != "cpu":
                if self.carry:
                    raise ValueError(f"a device block cannot follow an incomplete host frame ({len(self.carry)} bytes are carried)")
                if raw.numel() % frame:
                    raise ValueError(f"a device block must be whole frames of {frame} bytes, got {raw.numel()} bytes")
                if width != 3 and raw.numel() and raw.data_ptr() % width:
                    raise ValueError(f"a device block of {self.fmt!r} PCM must be aligned to its {width}-byte samples")
                return PcmBlock(self.fmt, self.src_channels, raw.numel() // frame, dev=raw)
            data = raw.numpy()
        else:
            try:
                data = np.frombuffer(block, dtype=np.uint8)
            except (TypeError, ValueError, BufferError):
                raise self._refuse(block) from None
        have = len(self.carry)
        whole = (have + len(data)) // frame * frame
        if whole == 0:
            return PcmBlock(self.fmt, self.src_channels, 0, pieces=[], carry=self.carry + data.tobytes())
        pieces = ([np.frombuffer(self.carry, dtype=np.uint8)] if have else []) + [data[:whole - have]]
        return PcmBlock(self.fmt, self.src_channels, whole // frame, pieces=pieces, carry=data[whole - have:].tobytes())

    def commit(self, blk: PcmBlock) -> None:
        self.carry = blk.carry


def _pcm_planar(raw: torch.Tensor, fmt: str, src_channels: int, n: int, channels: int, stats=None) -> torch.Tensor:
    """mi_pcm_planar on the uint8 device tensor `raw`: (channels, n) float32 on its device."""
    out = torch.empty(channels, n, device=raw.device, dtype=torch.float32)
    if n:
        with torch.cuda.device(raw.device):
            _lib.check(_lib.load().mi_pcm_planar(raw.data_ptr(), PCM_FORMATS[fmt][0], src_channels, n, channels,
                                                 stats.data_ptr() if stats is not None else None, out.data_ptr(),
                                                 C.c_void_p(_lib.current_stream_ptr())), "mi_pcm_planar")
    return out


def pcm_to_tensor(data, fmt: str, channels: int, device="cuda") -> torch.Tensor:
    """A whole buffer of interleaved PCM (`PCM_FORMATS`; bytes-like, a 1-D uint8 tensor or an (n, channels) int16 / float32 tensor,
    on the host or a device) as the (channels, n) float32 tensor `Separator.separate_tensor` takes, on `device`: one H2D of the
    bytes as they are and one `mi_pcm_planar`, no host pass over the samples.  int16 v becomes v / 32768, int24 v / 8388608, both
    exact; float32 keeps its bits.  An incomplete last frame is dropped."""
    dev = torch.device(device)
    if dev.type != "cuda":
        raise _lib.EngineError("demucs_amd.audio.pcm_to_tensor only runs on a GPU device (MI355X)")
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    blk = PcmFeed(fmt, channels).accept(data)
    if blk.n == 0:
        return torch.empty(blk.src_channels, 0, device=dev)
    keep = []
    with torch.cuda.device(dev):
        return _pcm_planar(blk.on_device(dev, keep), fmt, blk.src_channels, blk.n, blk.src_channels)


_WAVE_SUBFORMAT_TAIL = bytes.fromhex("000000001000800000aa00389b71")


def wav_info(head):
    """`wav_header`'s inverse: from the first bytes of a RIFF / WAVE file, `(fmt, channels, samplerate, frames or None,
    data_offset)` -- the `PCM_FORMATS` name of its samples, and where they start -- or None while `head` does not yet reach the
    samples.  Takes format tags 1 (PCM: 16 or 24 bits) and 3 (IEEE float: 32 bits), WAVE_FORMAT_EXTENSIBLE with either as its
    sub-format, any chunks before `data`, and the 0xFFFFFFFF sizes of a stream of unknown length (frames None); anything else
    (RIFX, 8-bit, int32, ADPCM, ...) is a ValueError."""
    import struct
    b = bytes(head)
    if b[:4] != b"RIFF"[:len(b[:4])]:
        raise ValueError(f"wav_info: not a little-endian RIFF file (it starts with {b[:4]!r})")
    if b[8:12] != b"WAVE"[:len(b[8:12])]:
        raise ValueError(f"wav_info: not a WAVE file (form type {b[8:12]!r})")
    pos, found = 12, None
    while pos + 8 <= len(b):
        tag, size = b[pos:pos + 4], struct.unpack_from("<I", b, pos + 4)[0]
        if tag == b"data":
            if found is None:
                raise ValueError("wav_info: the data chunk comes before the fmt chunk")
            fmt, channels, rate, align = found
            return fmt, channels, rate, None if size == 0xFFFFFFFF else size // align, pos + 8
        if tag == b"fmt ":
            if size < 16:
                raise ValueError(f"wav_info: a fmt chunk of {size} bytes")
            if pos + 8 + size > len(b):
                return None
            code, channels, rate, _, align, bits = struct.unpack_from("<HHIIHH", b, pos + 8)
            if code == 0xFFFE:
                if size < 40 or b[pos + 34:pos + 48] != _WAVE_SUBFORMAT_TAIL:
                    raise ValueError("wav_info: WAVE_FORMAT_EXTENSIBLE with a sub-format that is neither PCM nor IEEE float")
                code = struct.unpack_from("<H", b, pos + 32)[0]
            fmt = {(1, 16): "i16", (1, 24): "i24", (3, 32): "f32"}.get((code, bits))
            if fmt is None:
                raise ValueError(f"wav_info: format tag {code} with {bits} bits per sample is not supported (16 / 24-bit PCM and "
                                 "32-bit float are)")
            if channels < 1 or rate < 1 or align != channels * bits // 8:
                raise ValueError(f"wav_info: {channels} channels at {rate} Hz with a block align of {align} bytes")
            found = (fmt, channels, rate, align)
        pos += 8 + size + (size & 1)
    return None


class ConvertPlan:
    """The arithmetic of a streaming `resample_frac` (no device work).  For old / new = the rates divided by their gcd, `width`
    and klen = 2 * width + old as `sinc_bank` builds them, output n * new + i reads inputs clamp(n * old - width + k), k < klen.
    Frame n (its `new` outputs) is final iff its last tap is pushed: n * old + width + old <= P."""

    def __init__(self, from_samplerate: int, to_samplerate: int, zeros: int = ZEROS, rolloff: float = ROLLOFF):
        from_samplerate, to_samplerate = int(from_samplerate), int(to_samplerate)
        if from_samplerate <= 0 or to_samplerate <= 0:
            raise ValueError(f"sample rates must be positive, got {from_samplerate} -> {to_samplerate}")
        gcd = math.gcd(from_samplerate, to_samplerate)
        self.old, self.new = from_samplerate // gcd, to_samplerate // gcd
        self.copy = self.old == self.new                                   # equal rates: no filter, nothing is held back
        self.width = 0 if self.copy else math.ceil(zeros * self.old / (min(self.new, self.old) * rolloff))   # sinc_bank's
        self.klen = 2 * self.width + self.old
        if not self.copy and CVT_FRAMES * self.old + 2 * self.width > CVT_LDS_FLOATS:
            raise ValueError(f"the rate pair {from_samplerate} -> {to_samplerate} reduces to {self.old}:{self.new}: a frame of "
                             f"{self.old} input samples is too long for the stream kernel; resample the whole track instead")
        # floor(new * P / old) - ready(P) is largest one sample before a frame completes: P = width + old - 1 (+ a multiple of old)
        self.hold = 0 if self.copy else self.new * (self.width + self.old - 1) // self.old
        self.carry = 0 if self.copy else self.klen - 1                    # most input samples kept between two pushes

    def ready(self, pushed: int) -> int:
        """Outputs that are final after `pushed` input samples."""
        if self.copy:
            return pushed
        return self.new * max(0, (pushed - self.width - self.old) // self.old + 1)

    def final_count(self, total: int) -> int:
        """The whole track's output length (`resample_frac`'s default)."""
        return self.new * total // self.old

    def carry_start(self, pushed: int) -> int:
        """First input sample the first frame that is not ready reads (the left clamp keeps sample 0 while it is needed)."""
        if self.copy:
            return pushed
        return max(0, self.ready(pushed) // self.new * self.old - self.width)

    def subruns(self) -> int:
        """8-frame runs a workgroup of the kernel takes (convert_stream.hip)."""
        return min(CVT_SUBRUNS, (CVT_LDS_FLOATS - 2 * self.width) // (CVT_FRAMES * self.old))

    def groups(self, n_out: int) -> int:
        """Workgroups per row for `n_out` outputs."""
        if self.copy:
            return max(1, -(-n_out // CVT_COPY_SPAN))
        return max(1, -(-(-(-n_out // self.new)) // (CVT_FRAMES * self.subruns())))

    def lds_floats(self) -> int:
        return 1 if self.copy else CVT_FRAMES * self.subruns() * self.old + 2 * self.width

    def step(self, pushed: int, n_in: int, final: bool):
        """One call: (first output, outputs to write, carried start for the next call or -1 when final)."""
        total = pushed + n_in
        out0 = self.ready(pushed)
        if final:
            return out0, self.final_count(total) - out0, -1
        return out0, self.ready(total) - out0, self.carry_start(total)


class _BankArena:
    """Every rate pair's transposed kernel bank ([klen][new]: a tap's coefficients of all phases side by side) in one device
    buffer per device, built once per pair.  Offsets never move; a grown buffer is a new tensor (calls in flight keep theirs)."""
    _arenas = {}

    def __init__(self, dev):
        self.dev, self.buf, self.offs = dev, torch.zeros(0, device=dev), {}

    @classmethod
    def get(cls, dev) -> "_BankArena":
        dev = torch.device(dev)
        if dev not in cls._arenas:
            cls._arenas[dev] = cls(dev)
        return cls._arenas[dev]

    def offset(self, plan: ConvertPlan) -> int:
        key = (plan.old, plan.new)
        if plan.copy:
            return 0
        if key not in self.offs:
            width, bank = sinc_bank(plan.old, plan.new)
            assert width == plan.width and bank.shape == (plan.new, plan.klen)
            self.offs[key] = self.buf.numel()
            self.buf = torch.cat([self.buf, bank.t().contiguous().reshape(-1).to(self.dev)])
        return self.offs[key]


def convert_audio_stream(from_samplerate: int, to_samplerate: int, channels: int, device="cuda", affine=None, pcm=None,
                         src_channels=None) -> "ConvertStream":
    """`convert_audio` for a track that arrives block by block: `torch.cat([*pushes, finish], -1)` equals
    `convert_audio(full, from_samplerate, to_samplerate, channels)` bit for bit for every partition of the input.
    `pcm=` ("i16", "i24", "f32") with `src_channels=` takes the blocks as interleaved wire PCM instead (see `ConvertStream`)."""
    return ConvertStream(from_samplerate, to_samplerate, channels, device=device, affine=affine, pcm=pcm, src_channels=src_channels)


class ConvertStream:
    """`push(block)` takes (source channels, n) float32 on the host or a device and returns the (channels, m) outputs that became
    final, on the block's device; `finish()` returns the rest.  `pushed` counts input samples, `emitted` output samples;
    `floor(new * pushed / old) - emitted <= hold`, and some push reaches it.  The source channel count is the first block's.
    `affine=(mean, s)` writes `(y - mean) / s` instead (mi_track_affine inverse = 0 on the converted samples).
    Device state: two sides of (channels, klen - 1) carried input samples, whatever the stream's duration.

    With `pcm=` and `src_channels=` a block is interleaved little-endian PCM of that format (`PCM_FORMATS`): a bytes-like object
    or a 1-D uint8 tensor that may end anywhere (a `PcmFeed` carries the incomplete frame to the next push; a device block must be
    whole frames), or an (n, src_channels) int16 / float32 tensor.  `mi_streams_convert_append_pcm` reads the frames where the
    float entry reads planar floats, so the outputs are those of the float stream on `v / 32768`, bit for bit; `pushed` counts
    frames and `trailing_bytes` the bytes of an incomplete last frame, which `finish()` drops."""

    def __init__(self, from_samplerate, to_samplerate, channels: int, device="cuda", affine=None, plan=None, pcm=None,
                 src_channels=None):
        self.plan = plan if plan is not None else ConvertPlan(from_samplerate, to_samplerate)
        self.channels = int(channels)
        if self.channels < 1:
            raise ValueError(f"channels must be >= 1, got {channels}")
        dev = torch.device(device)
        if dev.type != "cuda":
            raise _lib.EngineError("demucs_amd.audio.convert_audio_stream only runs on a GPU device (MI355X)")
        self.device = dev
        self.hold = self.plan.hold
        self.pushed = self.emitted = 0
        self.src_channels = None
        self.feed = None
        if pcm is not None:
            if src_channels is None:
                raise ValueError("a PCM stream needs src_channels=: the frames do not say how many channels they hold")
            self.feed = PcmFeed(pcm, src_channels)
            check_stream_channels(self.feed.src_channels, self.channels)
            self.src_channels = self.feed.src_channels
        self.finished = False
        self.affine = None if affine is None else tuple(float(v) for v in affine)
        self._hist = self._stats = None
        self._side = 0
        self._h0 = 0
        self._out_device = None

    def device_bytes(self) -> int:
        return sum(4 * t.numel() for t in (self._hist, self._stats) if t is not None)

    def _call(self, block, final: bool, on_device: bool = False) -> torch.Tensor:
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        plan, dev, ch = self.plan, self.device, self.channels
        n_in = 0 if block is None else block.shape[1]
        out0, n_out, nxt = plan.step(self.pushed, n_in, final)
        with torch.cuda.device(dev):
            out = torch.empty(ch, n_out, device=dev, dtype=torch.float32)
            if n_in or n_out:
                if self._hist is None and not plan.copy:
                    self._hist = torch.zeros(2, ch, plan.carry, device=dev)
                if self._stats is None and self.affine is not None:
                    self._stats = torch.tensor(self.affine, dtype=torch.float32).to(dev)
                keep = []
                wire = isinstance(block, PcmBlock)
                if wire:
                    src = block.on_device(dev, keep) if n_in else None
                else:
                    src = block.to(device=dev, dtype=torch.float32).contiguous() if n_in else None
                arena = _BankArena.get(dev)
                bank_off = arena.offset(plan)
                bank, hist, stats = arena.buf, self._hist, self._stats
                h_len = plan.carry
                side = ch * h_len
                row = [src.data_ptr() if n_in else 0, self.src_channels or 1, n_in, self.pushed, h_len, self._side * side,
                       (1 - self._side) * side, self._h0, nxt, out0, n_out, self.pushed + n_in if final else -1, plan.old, plan.new,
                       plan.width, bank_off, 0, n_out, 0, 0 if stats is not None else -1]
                lib = _lib.load()
                entry, name = lib.mi_streams_convert_append, "mi_streams_convert_append"
                if self.feed is not None:                  # the final call of a PCM stream has no block: any format
                    row.append(PCM_FORMATS[self.feed.fmt][0])
                    entry, name = lib.mi_streams_convert_append_pcm, "mi_streams_convert_append_pcm"
                table = torch.tensor(row, dtype=torch.int64).to(dev)
                win = out if n_out else table              # nothing is written when n_out == 0: any live pointer
                _lib.check(entry(
                    win.data_ptr(), max(1, out.numel()), ch, table.data_ptr(), 1, plan.groups(n_out),
                    bank.data_ptr() if bank.numel() else None, bank.numel(), hist.data_ptr() if hist is not None else None,
                    0 if hist is None else hist.numel(), stats.data_ptr() if stats is not None else None, int(stats is not None),
                    plan.lds_floats(), C.c_void_p(_lib.current_stream_ptr())), name)
                if not final and not plan.copy:
                    self._side, self._h0 = 1 - self._side, nxt
        self.pushed += n_in
        self.emitted += n_out
        to = None if on_device else self._out_device
        return out if to is None or out.device == torch.device(to) else out.to(to)

    def push(self, block: torch.Tensor, on_device: bool = False) -> torch.Tensor:
        """`on_device=True` leaves the output on the stream's device whatever the block's."""
        if self.finished:
            raise RuntimeError("push after finish()")
        if self.feed is not None:
            blk = block
            if not isinstance(block, PcmBlock):            # a caller with a feed of its own hands over whole frames
                blk = self.feed.accept(block)
                self.feed.commit(blk)
            self._out_device = blk.device
            return self._call(blk, final=False, on_device=on_device)
        if not isinstance(block, torch.Tensor) or block.dim() != 2:
            raise ValueError(f"expected a (channels, n) block, got {tuple(getattr(block, 'shape', ()))}")
        if self.src_channels is None:
            check_stream_channels(block.shape[0], self.channels)
            self.src_channels = block.shape[0]
        elif block.shape[0] != self.src_channels:
            raise ValueError(f"expected a ({self.src_channels}, n) block, got {tuple(block.shape)}")
        self._out_device = block.device
        return self._call(block, final=False, on_device=on_device)

    def finish(self, on_device: bool = False) -> torch.Tensor:
        if self.finished:
            raise RuntimeError("finish() called twice")
        self.finished = True
        return self._call(None, final=True, on_device=on_device)

    @property
    def trailing_bytes(self) -> int:
        """Bytes of an incomplete last frame of a PCM stream: carried to the next push, dropped by `finish()`."""
        return 0 if self.feed is None else self.feed.trailing_bytes


# ---- track statistics for a stream: mi_mono_stats block by block (demucs_amd/csrc/stats_stream.hip) -----------------------
class TrackStats:
    """The normaliser of `Separator.separate_tensor` for one track, as `mi_mono_stats` computes it: `mean` and `s`, the float32
    mono mean and `std + 1e-8` (the 1e-8 already added; NaN for a track of one sample, as torch's unbiased std), of `length`
    samples at the model's rate.  `input_length` counts the frames pushed when a converter sat in front of the analysis, else it
    equals `length`.  Immutable; `separate_stream(stats=...)` takes it as it is."""
    __slots__ = ("mean", "s", "length", "input_length")

    def __init__(self, mean, s, length, input_length=None):
        import numpy as np
        vals = []
        for name, v in (("mean", mean), ("s", s)):
            if isinstance(v, (bool, str, bytes)) or not isinstance(v, (int, float, np.floating, np.integer)):
                raise ValueError(f"TrackStats: {name} must be a real number, got {v!r}")
            v = float(v)
            with np.errstate(over="ignore"):
                r = float(np.float32(v))
            if r != v and not (math.isnan(r) and math.isnan(v)):
                raise ValueError(f"TrackStats: {name} must be a float32 value as mi_mono_stats writes it, got {v!r}")
            vals.append(v)
        lens = []
        for name, v in (("length", length), ("input_length", length if input_length is None else input_length)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 1:
                raise ValueError(f"TrackStats: {name} must be a positive integer, got {v!r}")
            lens.append(int(v))
        for name, v in zip(self.__slots__, vals + lens):
            object.__setattr__(self, name, v)

    def __setattr__(self, name, value):
        raise AttributeError("TrackStats is immutable")

    def __delattr__(self, name):
        raise AttributeError("TrackStats is immutable")

    def _key(self):
        return (*(("nan",) if math.isnan(v) else (v,) for v in (self.mean, self.s)), self.length, self.input_length)

    def __eq__(self, other):
        return isinstance(other, TrackStats) and self._key() == other._key()

    def __hash__(self):
        return hash(self._key())

    def __repr__(self):
        return f"TrackStats(mean={self.mean!r}, s={self.s!r}, length={self.length}, input_length={self.input_length})"


class MonoStatsStream:
    """`mi_mono_stats` for a track that arrives block by block: `push(block)` adds a block, `finish()` returns the `TrackStats`
    of everything pushed, with the bits `mi_mono_stats` gives for the whole (channels, length) track, for every partition.
    A block is planar (channels, n) float32 on the host or a device; with `pcm=` and `src_channels=` interleaved wire PCM as
    `ConvertStream` takes it (a bytes-like object or a 1-D uint8 tensor that may end anywhere, a `PcmFeed` carrying the incomplete
    frame; an (n, src_channels) int16 / float32 tensor; or a `PcmBlock`), read by the kernel where it lies with `mi_pcm_planar`'s
    channel map.  A push is one H2D for a host block and one `mi_mono_stats_update` launch.  `pushed` counts samples per channel
    (frames), `trailing_bytes` the bytes of an incomplete last frame, which `finish()` drops.  Device state: 4 MiB of per-thread
    sums (`mi_mono_stats_state_bytes`), whatever the track's duration."""

    def __init__(self, channels: int, device="cuda", pcm=None, src_channels=None):
        self.channels = int(channels)
        if self.channels < 1:
            raise ValueError(f"channels must be >= 1, got {channels}")
        self.feed = None
        if pcm is not None:
            if src_channels is None:
                raise ValueError("a PCM stream needs src_channels=: the frames do not say how many channels they hold")
            self.feed = PcmFeed(pcm, src_channels)
            check_stream_channels(self.feed.src_channels, self.channels)
        dev = torch.device(device)
        if dev.type != "cuda":
            raise _lib.EngineError("demucs_amd.audio.MonoStatsStream only runs on a GPU device (MI355X)")
        self.device = dev
        self.pushed = 0
        self.finished = False
        self._state = self._scratch = self._stats = None

    def device_bytes(self) -> int:
        return sum(t.numel() * t.element_size() for t in (self._state, self._scratch, self._stats) if t is not None)

    @property
    def trailing_bytes(self) -> int:
        return 0 if self.feed is None else self.feed.trailing_bytes

    def _on(self):
        """The device as a context, its index resolved at the first device work."""
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        return torch.cuda.device(self.device)

    def _update(self, src: torch.Tensor, code: int, src_channels: int, n: int) -> None:
        lib = _lib.load()
        if self._state is None:
            self._state = torch.zeros(lib.mi_mono_stats_state_bytes(), dtype=torch.uint8, device=self.device)
        _lib.check(lib.mi_mono_stats_update(src.data_ptr(), code, src_channels, n, self.channels, self.pushed, self._state.data_ptr(),
                                            C.c_void_p(_lib.current_stream_ptr())), "mi_mono_stats_update")
        self.pushed += n

    def push(self, block) -> None:
        if self.finished:
            raise RuntimeError("push after finish()")
        if self.feed is not None or isinstance(block, PcmBlock):
            blk = block
            if not isinstance(block, PcmBlock):            # a caller with a feed of its own hands over whole frames
                blk = self.feed.accept(block)
                self.feed.commit(blk)
            else:
                check_stream_channels(blk.src_channels, self.channels)
            if blk.n:
                keep = []
                with self._on():
                    self._update(blk.on_device(self.device, keep), blk.code, blk.src_channels, blk.n)
            return
        if not isinstance(block, torch.Tensor) or block.dim() != 2 or block.shape[0] != self.channels:
            shape = tuple(block.shape) if isinstance(block, torch.Tensor) else type(block).__name__
            raise ValueError(f"expected a ({self.channels}, n) block, got {shape}")
        if block.shape[1]:
            with self._on():
                src = block.to(device=self.device, dtype=torch.float32).contiguous()
                self._update(src, PCM_PLANAR, self.channels, block.shape[1])

    def finish(self) -> TrackStats:
        if self.finished:
            raise RuntimeError("finish() called twice")
        if self.pushed == 0:
            raise ValueError("the stream ended before any sample was pushed")
        self.finished = True
        lib = _lib.load()
        with torch.cuda.device(self.device):
            self._scratch = torch.empty(lib.mi_mono_stats_scratch_bytes(), dtype=torch.uint8, device=self.device)
            self._stats = torch.empty(2, dtype=torch.float32, device=self.device)
            _lib.check(lib.mi_mono_stats_finish(self._state.data_ptr(), self.pushed, self._scratch.data_ptr(), self._stats.data_ptr(),
                                                C.c_void_p(_lib.current_stream_ptr())), "mi_mono_stats_finish")
            mean, s = self._stats.cpu().tolist()
        return TrackStats(mean, s, self.pushed)


class ConvertingStatsStream:
    """`Separator.analyse_stream` for an input at another sample rate or channel count: a `ConvertStream` on the device whose
    outputs feed a `MonoStatsStream`, so the statistics are those of `convert_audio(...)` of the whole track.  `pushed` counts
    input frames; `finish()` fills `TrackStats.input_length` with it."""

    def __init__(self, plan, channels: int, src_channels: int, device, pcm=None):
        self.convert = ConvertStream(None, None, channels, device=device, plan=plan, pcm=pcm,
                                     src_channels=src_channels if pcm is not None else None)
        self.stats = MonoStatsStream(channels, device=device)
        self.src_channels = int(src_channels)

    @property
    def pushed(self) -> int:
        return self.convert.pushed

    @property
    def finished(self) -> bool:
        return self.stats.finished

    @property
    def trailing_bytes(self) -> int:
        return self.convert.trailing_bytes

    def device_bytes(self) -> int:
        return self.convert.device_bytes() + self.stats.device_bytes()

    def push(self, block) -> None:
        if self.stats.finished:
            raise RuntimeError("push after finish()")
        if self.convert.feed is None and (not isinstance(block, torch.Tensor) or block.dim() != 2 or
                                          block.shape[0] != self.src_channels):
            shape = tuple(block.shape) if isinstance(block, torch.Tensor) else type(block).__name__
            raise ValueError(f"expected a ({self.src_channels}, n) block, got {shape}")
        self.stats.push(self.convert.push(block, on_device=True))

    def finish(self) -> TrackStats:
        if self.stats.finished:
            raise RuntimeError("finish() called twice")
        if self.convert.pushed == 0:
            raise ValueError("the stream ended before any sample was pushed")
        self.stats.push(self.convert.finish(on_device=True))
        st = self.stats.finish()
        return TrackStats(st.mean, st.s, st.length, self.convert.pushed)


# ---- after the separation: what demucs.separate does with the stems before any encoder sees them ----------------------
_CLIP_MODES = {"rescale": 1, "clamp": 2, "tanh": 3}


def _engine_device(*tensors) -> torch.device:
    """The GPU the kernels run on: the device of the first device tensor, else the current GPU (host tensors -- what
    `Separator.separate_tensor(host wav)` returns -- are staged through it).  There is no CPU implementation."""
    for t in tensors:
        if t is not None and t.device.type == "cuda":
            return t.device
    if not torch.cuda.is_available():
        raise _lib.EngineError("demucs_amd.audio: prevent_clip / two_stems run on the GPU (MI355X) and none is available; "
                               "there is no CPU implementation in this package.")
    return torch.device("cuda", torch.cuda.current_device())


def _stage(t: torch.Tensor, dev: torch.device, what: str) -> torch.Tensor:
    """`t` as a contiguous float32 tensor on `dev` (the reference accepts any floating tensor on any device)."""
    if not t.dtype.is_floating_point:
        raise TypeError(f"{what}: a floating-point tensor is expected, got {t.dtype}")
    return t.to(device=dev, dtype=torch.float32).contiguous()


def prevent_clip(wav: torch.Tensor, mode="rescale") -> torch.Tensor:
    """demucs/audio.py:218-234 as a device kernel (`mi_prevent_clip`: the peak of "rescale" is reduced on the device and
    never visits the host).  Device stems (an engine separation with `split=True` and a device mix) are processed where
    they live; host stems (what `Separator.separate_tensor(host wav)` returns) are staged H2D / D2H around the kernel;
    other floating dtypes are computed in float32 and cast back.  NaN samples propagate like torch's `abs().max()`."""
    if mode is None or mode == "none":
        return wav
    assert wav.dtype.is_floating_point, "too late for clipping"
    if mode not in _CLIP_MODES:
        raise ValueError(f"Invalid mode {mode}")
    dev = _engine_device(wav)
    x = _stage(wav, dev, "prevent_clip")
    y = torch.empty_like(x)
    if x.numel():
        with torch.cuda.device(dev):
            peak = torch.empty(1, dtype=torch.int32, device=dev)
            _lib.check(_lib.load().mi_prevent_clip(x.data_ptr(), x.numel(), _CLIP_MODES[mode], peak.data_ptr(), y.data_ptr(),
                                                   C.c_void_p(_lib.current_stream_ptr())), "mi_prevent_clip")
    return y.to(device=wav.device, dtype=wav.dtype)            # like the reference: same device and dtype as the input


def two_stems(origin: torch.Tensor, stems: dict, stem: str, other_method: str = "add") -> dict:
    """`--two-stems STEM` of demucs/separate.py:189-218 as a tensor function on the stems' device (`mi_two_stems`): returns
    {STEM: ..., "no_STEM": 0 + the other stems in dict order} for other_method="add", {"minus_STEM": origin - STEM, STEM: ...}
    for "minus", {STEM: ...} for "none"."""
    if stem not in stems:
        raise KeyError(f"stem {stem!r} is not in the separated sources {list(stems)}")
    if other_method not in ("add", "minus", "none"):
        raise ValueError(f"Invalid other_method {other_method}")
    names = list(stems)
    out = {}
    if other_method in ("add", "minus"):
        if len(names) > 8:
            raise ValueError("two_stems: at most 8 stems")
        dev = _engine_device(*stems.values())
        tensors = [_stage(stems[k], dev, "two_stems") for k in names]
        n = tensors[0].numel()
        assert all(t.numel() == n for t in tensors)
        y = torch.empty_like(tensors[0])
        minus = other_method == "minus"
        org = _stage(origin, dev, "two_stems") if minus else None
        assert org is None or org.numel() == n
        ptrs = (C.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])
        with torch.cuda.device(y.device):
            _lib.check(_lib.load().mi_two_stems(ptrs, len(tensors), names.index(stem), org.data_ptr() if minus else None, int(minus), n,
                                                y.data_ptr(), C.c_void_p(_lib.current_stream_ptr())), "mi_two_stems")
        y = y.to(device=stems[stem].device, dtype=stems[stem].dtype)
        if minus:
            out["minus_" + stem] = y
    out[stem] = stems[stem]
    if other_method == "add":
        out["no_" + stem] = y
    return out


# ---- delivery: every output of the reference's save loop, clipped, converted and interleaved by one kernel pair -----------
DELIVER_COLS = 9                                  # include/demucs_amd.h: MI_DELIVER_*
DELIVER_STEM, DELIVER_ADD, DELIVER_MINUS = 0, 1, 2
_FORMATS = {"i16": (0, torch.int16, 2), "f32": (1, torch.float32, 4)}       # MI_DELIVER_I16 / _F32, dtype, bytes per sample


def clip_code(clip) -> int:
    """`prevent_clip`'s mode as mi_deliver_pcm's CLIP column (0: none)."""
    if clip is None or clip == "none":
        return 0
    if clip not in _CLIP_MODES:
        raise ValueError(f"Invalid mode {clip}")
    return _CLIP_MODES[clip]


def delivery_outputs(sources, stem=None, other_method="add") -> list:
    """[(name, KIND, SEL)] in the order demucs/separate.py:178-218 saves its files: every source without `stem`; with it
    "minus_STEM" (other_method "minus"), STEM, "no_STEM" ("add")."""
    sources = list(sources)
    if other_method not in ("add", "minus", "none"):
        raise ValueError(f"Invalid other_method {other_method}")
    if stem is None:
        return [(name, DELIVER_STEM, k) for k, name in enumerate(sources)]
    if stem not in sources:
        raise ValueError(f"stem {stem!r} is not in the separated sources {sources}")
    sel = sources.index(stem)
    outs = [("minus_" + stem, DELIVER_MINUS, sel)] if other_method == "minus" else []
    outs.append((stem, DELIVER_STEM, sel))
    if other_method == "add":
        outs.append(("no_" + stem, DELIVER_ADD, sel))
    return outs


def deliver_layout(outputs, frames: int, channels: int, fmt: str, at: int = 0):
    """Byte offsets of `outputs`' (frames, channels) blocks from `at` on, each on a 16-byte boundary (the kernel's widest store),
    and the end of the last."""
    if fmt not in _FORMATS:
        raise ValueError(f"Invalid format {fmt!r}: 'i16' or 'f32'")
    size = frames * channels * _FORMATS[fmt][2]
    offs = []
    for _ in outputs:
        at = -(-at // 16) * 16
        offs.append(at)
        at += size
    return offs, at


def deliver_views(buf: torch.Tensor, outputs, offs, frames: int, channels: int, fmt: str) -> dict:
    """{name: (frames, channels) int16 / float32 view} of the byte buffer `buf` mi_deliver_pcm filled."""
    _, dtype, width = _FORMATS[fmt]
    size = frames * channels * width
    return {name: buf[off:off + size].view(dtype).view(frames, channels) for (name, _, _), off in zip(outputs, offs)}


class TrackPeaks:
    """What a measuring pass over a stream found (`Delivery(clip="rescale", peaks="measure")`): per output of the reference's save
    loop the peak that `prevent_clip(·, "rescale")` divides by, so that a second pass of the same stream can deliver with it.

    `names` are the outputs in the reference's save order (`delivery_outputs` for `stem` / `other_method`), `bits` one uint32 per
    output: the bit pattern of the float32 `max |value|` as `mi_deliver_peaks` writes it (a NaN sample gives a NaN pattern),
    `samplerate` the rate of the delivered frames the peaks were measured at (None: the model's), `length` the model-rate samples
    measured.  Constructible by hand: a caller who knows an upper bound of a live feed's peak passes its bits and gets the fixed,
    reference-shaped gain `v / max(1.01 * peak, 1)`.  Peaks of gain-weighted remixes (`Delivery(mix=...)`) carry the remixes'
    identity in `mix`: `((output name, (g_mix, g_0 .. g_{S-1})), ...)`, the float32 gains per source as `mix_gains` resolves them
    (None: the outputs are the reference's).  Immutable."""
    __slots__ = ("names", "bits", "samplerate", "stem", "other_method", "length", "mix")

    def __init__(self, names, bits, samplerate=None, stem=None, other_method: str = "add", length: int = 1, mix=None):
        import numpy as np
        if isinstance(names, (str, bytes)) or not all(isinstance(n, str) for n in names):
            raise ValueError(f"TrackPeaks: names must be a sequence of output names, got {names!r}")
        names = tuple(names)
        if other_method not in ("add", "minus", "none"):
            raise ValueError(f"Invalid other_method {other_method}")
        if stem is not None and not isinstance(stem, str):
            raise ValueError(f"TrackPeaks: stem must be a source name or None, got {stem!r}")
        if mix is not None:
            if stem is not None:
                raise ValueError(f"TrackPeaks: mix belongs to stem=None, got stem={stem!r}")
            try:
                mix = tuple((str(name), tuple(float(np.float32(g)) for g in gains)) for name, gains in mix)
            except (TypeError, ValueError):
                raise ValueError(f"TrackPeaks: mix must be ((output name, (g_mix, g_0, ...)), ...) as audio.mix_gains returns it, "
                                 f"got {mix!r}") from None
            if tuple(name for name, _ in mix) != names or len({len(g) for _, g in mix}) > 1 or \
                    not all(len(g) >= 2 and all(np.isfinite(v) for v in g) for _, g in mix):
                raise ValueError(f"TrackPeaks: mix must name the outputs {list(names)} in order, each with finite gains for the mix "
                                 f"and every source, got {mix!r}")
        if stem is None:
            if not names or len(set(names)) != len(names):
                raise ValueError(f"TrackPeaks: names must be the separated sources, each once, got {list(names)}")
        else:
            # the sources other than `stem` do not enter a two-stems output's name
            want = tuple(name for name, _, _ in delivery_outputs([stem], stem, other_method))
            if names != want:
                raise ValueError(f"TrackPeaks: the outputs of stem={stem!r}, other_method={other_method!r} are {list(want)} in the "
                                 f"reference's save order, got {list(names)}")
        if isinstance(bits, (str, bytes)) or not hasattr(bits, "__len__"):
            raise ValueError(f"TrackPeaks: bits must be a sequence of uint32 bit patterns, got {bits!r}")
        if len(bits) != len(names):
            raise ValueError(f"TrackPeaks: {len(names)} outputs need {len(names)} peaks, got {len(bits)}")
        vals = []
        for v in bits:
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 0 <= int(v) <= 0xFFFFFFFF:
                raise ValueError(f"TrackPeaks: a peak is the uint32 bit pattern of a float32 (see TrackPeaks.from_values), got {v!r}")
            if int(v) & 0x80000000:
                raise ValueError(f"TrackPeaks: a peak is max |value|, whose sign bit is clear, got {int(v):#010x}")
            vals.append(int(v))
        if samplerate is not None and (isinstance(samplerate, bool) or not isinstance(samplerate, (int, np.integer)) or samplerate <= 0):
            raise ValueError(f"TrackPeaks: samplerate must be a positive integer or None, got {samplerate!r}")
        if isinstance(length, bool) or not isinstance(length, (int, np.integer)) or length < 1:
            raise ValueError(f"TrackPeaks: length must be a positive integer, got {length!r}")
        for name, v in zip(self.__slots__, (names, tuple(vals), None if samplerate is None else int(samplerate), stem, other_method,
                                            int(length), mix)):
            object.__setattr__(self, name, v)

    @classmethod
    def from_values(cls, names, peaks, **kw) -> "TrackPeaks":
        """From float peaks (each rounded to float32, its magnitude taken)."""
        import numpy as np
        return cls(names, [int(np.abs(np.float32(p)).view(np.uint32)) for p in peaks], **kw)

    def __setattr__(self, name, value):
        raise AttributeError("TrackPeaks is immutable")

    def __delattr__(self, name):
        raise AttributeError("TrackPeaks is immutable")

    def peak(self, name: str):
        """The float32 `max |value|` of output `name`."""
        import numpy as np
        return np.uint32(self.bits[self.names.index(name)]).view(np.float32)

    def divisor(self, name: str):
        """float32(peak * float32(1.01)): `clip_divisor` of post_ops.h; the frames are `v / divisor` when it exceeds 1 or is NaN."""
        import numpy as np
        with np.errstate(over="ignore", invalid="ignore"):
            return np.float32(self.peak(name) * np.float32(1.01))

    def _key(self):
        return tuple(getattr(self, k) for k in self.__slots__)

    def __eq__(self, other):
        return isinstance(other, TrackPeaks) and self._key() == other._key()

    def __hash__(self):
        return hash(self._key())

    def __repr__(self):
        return (f"TrackPeaks(names={list(self.names)}, bits={[hex(b) for b in self.bits]}, samplerate={self.samplerate}, "
                f"stem={self.stem!r}, other_method={self.other_method!r}, length={self.length}"
                + ("" if self.mix is None else f", mix={self.mix!r}") + ")")


def _stems_block(tensors, dev: torch.device) -> torch.Tensor:
    """The stems as one contiguous float32 (S, channels, n) tensor on `dev`: read in place when they already are the rows of one
    (what `Separator.separate_tensor` returns for a device mix), else stacked once (host stems: stacked, then one H2D)."""
    first = tensors[0]
    step = first.numel() * 4
    if (first.device == dev and step and
            all(t.dtype == torch.float32 and t.device == dev and t.is_contiguous() and t.shape == first.shape and
                t.untyped_storage().data_ptr() == first.untyped_storage().data_ptr() and
                t.data_ptr() == first.data_ptr() + k * step for k, t in enumerate(tensors))):
        return torch.as_strided(first, (len(tensors), *first.shape), (first.numel(), *first.stride()))
    return torch.stack([t.to(torch.float32) for t in tensors]).to(dev).contiguous()


# ---- delivery at another sample rate (mi_deliver_resample_pcm, demucs_amd/csrc/deliver_resample.hip) -------------------------
RATE_COLS = 20                     # include/demucs_amd.h: MI_RATE_*
RATE_LDS_FLOATS = 16384            # MI_RATE_LDS_FLOATS: the kernel's LDS staging area (64 KiB), shared by all channels
RATE_FRAMES, RATE_SUBRUNS = 8, 4


def rate_subruns(plan: ConvertPlan, channels: int) -> int:
    """8-frame runs a workgroup of the kernel takes: what the staging area holds for all channels (deliver_resample.hip)."""
    return min(RATE_SUBRUNS, (RATE_LDS_FLOATS // channels - 2 * plan.width) // (RATE_FRAMES * plan.old))


def rate_groups(plan: ConvertPlan, channels: int, n_out: int) -> int:
    """Workgroups per row for `n_out` output frames."""
    return max(1, -(-(-(-n_out // plan.new)) // (RATE_FRAMES * rate_subruns(plan, channels))))


def rate_lds_floats(plan: ConvertPlan, channels: int) -> int:
    return channels * (RATE_FRAMES * rate_subruns(plan, channels) * plan.old + 2 * plan.width)


def delivery_rate_plan(model_rate: int, samplerate, channels: int):
    """The `ConvertPlan(model_rate, samplerate)` of a stream that delivers at `samplerate`, None when that is the model's rate (or
    None): the refusals of such a stream, without any device work."""
    if samplerate is None:
        return None
    if int(samplerate) != samplerate or samplerate <= 0:
        raise ValueError(f"the delivered sample rate must be a positive integer, got {samplerate}")
    if int(samplerate) == int(model_rate):
        return None
    try:
        plan = ConvertPlan(int(model_rate), int(samplerate))
    except ValueError as exc:
        raise ValueError(f"a stream cannot deliver at {samplerate} Hz from the model's {model_rate} Hz: {exc}") from None
    if rate_subruns(plan, channels) < 1:
        raise ValueError(f"a stream cannot deliver at {samplerate} Hz from the model's {model_rate} Hz: the rate pair {model_rate} -> "
                         f"{samplerate} reduces to {plan.old}:{plan.new}, and a frame of {plan.old} samples of {channels} channels is "
                         "too long for the delivery kernel; deliver at the model's rate and resample the whole track instead")
    return plan


def _deliver_resampled(origin, stems: dict, stem, other_method, clip, fmt, rates) -> dict:
    """`deliver` at another sample rate, for a whole track: per output the `two_stems` value, `resample_frac`, then the delivery
    kernels on the resampled values as plain rows (the peak of "rescale" is that of the resampled value)."""
    old_rate, new_rate = (int(r) for r in rates)
    names = list(stems)
    outputs = delivery_outputs(names, stem, other_method)
    code = clip_code(clip)
    if fmt not in _FORMATS:
        raise ValueError(f"Invalid format {fmt!r}: 'i16' or 'f32'")
    for t in stems.values():
        if not t.dtype.is_floating_point:
            raise TypeError(f"deliver: a floating-point tensor is expected, got {t.dtype}")
        if t.dim() != 2 or t.shape != stems[names[0]].shape:
            raise ValueError(f"deliver: every stem is (channels, n), got {[tuple(x.shape) for x in stems.values()]}")
    values = dict(stems) if stem is None else two_stems(origin, stems, stem, other_method)
    assert list(values) == [name for name, _, _ in outputs]
    first = next(iter(values.values()))
    home = first.device
    dev = _engine_device(*values.values())
    with torch.cuda.device(dev):
        block = torch.stack([_stage(v, dev, "deliver") for v in values.values()])
        block = resample_frac(block, old_rate, new_rate, device=dev).contiguous()
        _, channels, n = block.shape
        if n == 0 or channels == 0:
            return {name: torch.empty(n, channels, dtype=_FORMATS[fmt][1], device=home) for name in values}
        plain = [(name, DELIVER_STEM, i) for i, name in enumerate(values)]
        offs, total = deliver_layout(plain, n, channels, fmt)
        rows = []
        for (_, kind, sel), off in zip(plain, offs):
            rows += [block.data_ptr(), 0, n, kind, sel, code, sel, _FORMATS[fmt][0], off]
        table = torch.tensor(rows, dtype=torch.int64).to(dev)
        buf = torch.empty(total, dtype=torch.uint8, device=dev)
        lib, stream = _lib.load(), C.c_void_p(_lib.current_stream_ptr())
        peaks = None
        if code == _CLIP_MODES["rescale"]:
            peaks = torch.empty(len(plain), dtype=torch.int32, device=dev)
            _lib.check(lib.mi_deliver_peaks(table.data_ptr(), len(plain), n, len(plain), channels, peaks.data_ptr(), len(plain), total,
                                            stream), "mi_deliver_peaks")
        _lib.check(lib.mi_deliver_pcm(table.data_ptr(), len(plain), n, len(plain), channels,
                                      peaks.data_ptr() if peaks is not None else None, 0 if peaks is None else len(plain),
                                      buf.data_ptr(), total, stream), "mi_deliver_pcm")
        if home.type == "cpu":
            host = torch.empty(total, dtype=torch.uint8, pin_memory=True)
            host.copy_(buf, non_blocking=True)
            torch.cuda.current_stream(dev).synchronize()
            buf = host
        elif home != dev:
            buf = buf.to(home)
    return deliver_views(buf, plain, offs, n, channels, fmt)


def deliver(origin: torch.Tensor, stems: dict, stem=None, other_method: str = "add", clip="rescale", fmt: str = "i16",
            samplerate=None) -> dict:
    """What demucs/separate.py:178-218 hands to its encoders, for one separated track: `{name: (n, channels) frames}` in the
    order of the reference's save loop -- every source, or with `stem` the `--two-stems` outputs `two_stems` names -- each after
    `prevent_clip(·, clip)` (the peak of "rescale" is per output, as `save_audio` is called per output) and `i16_pcm` (fmt "i16")
    or as float32 ("f32"), channels interleaved per frame.  All outputs of the track take ONE `mi_deliver_peaks` launch (only
    for "rescale") and ONE `mi_deliver_pcm` launch; host stems come back on the host by one D2H of the byte buffer.

    `samplerate=(M, R)` delivers at R what was separated at M: per output `resample_frac(value, M, R)` between the two-stems value
    and `prevent_clip`, i.e. `save_audio(julius.resample_frac(v, M, R), path, samplerate=R, clip=clip)`; the frames number
    floor(R' * n / M') (the rates divided by their gcd).  It is the whole-track counterpart of `Delivery(samplerate=R)` on a
    stream, and takes `two_stems`' and `resample_frac`'s launches before the two above."""
    if samplerate is not None and int(samplerate[0]) != int(samplerate[1]):
        return _deliver_resampled(origin, stems, stem, other_method, clip, fmt, samplerate)
    names = list(stems)
    outputs = delivery_outputs(names, stem, other_method)
    code = clip_code(clip)
    if fmt not in _FORMATS:
        raise ValueError(f"Invalid format {fmt!r}: 'i16' or 'f32'")
    tensors = [stems[k] for k in names]
    for t in tensors:
        if not t.dtype.is_floating_point:
            raise TypeError(f"deliver: a floating-point tensor is expected, got {t.dtype}")
        if t.dim() != 2 or t.shape != tensors[0].shape:
            raise ValueError(f"deliver: every stem is (channels, n), got {[tuple(x.shape) for x in tensors]}")
    channels, n = tensors[0].shape
    home = tensors[0].device
    dtype = _FORMATS[fmt][1]
    if n == 0 or channels == 0:
        return {name: torch.empty(n, channels, dtype=dtype, device=home) for name, _, _ in outputs}
    dev = _engine_device(*tensors)
    minus = any(kind == DELIVER_MINUS for _, kind, _ in outputs)
    with torch.cuda.device(dev):
        block = _stems_block(tensors, dev)
        org = _stage(origin, dev, "deliver") if minus else None
        if org is not None and org.shape != (channels, n):
            raise ValueError(f"deliver: the mix is {tuple(org.shape)}, the stems are {(channels, n)}")
        offs, total = deliver_layout(outputs, n, channels, fmt)
        rows = []
        for i, ((_, kind, sel), off) in enumerate(zip(outputs, offs)):
            rows += [block.data_ptr(), org.data_ptr() if kind == DELIVER_MINUS else 0, n, kind, sel, code, i, _FORMATS[fmt][0], off]
        table = torch.tensor(rows, dtype=torch.int64).to(dev)
        buf = torch.empty(total, dtype=torch.uint8, device=dev)
        lib, stream = _lib.load(), C.c_void_p(_lib.current_stream_ptr())
        peaks = None
        if code == _CLIP_MODES["rescale"]:
            peaks = torch.empty(len(outputs), dtype=torch.int32, device=dev)
            _lib.check(lib.mi_deliver_peaks(table.data_ptr(), len(outputs), n, len(names), channels, peaks.data_ptr(), len(outputs),
                                            total, stream), "mi_deliver_peaks")
        _lib.check(lib.mi_deliver_pcm(table.data_ptr(), len(outputs), n, len(names), channels,
                                      peaks.data_ptr() if peaks is not None else None, 0 if peaks is None else len(outputs),
                                      buf.data_ptr(), total, stream), "mi_deliver_pcm")
        if home.type == "cpu":
            host = torch.empty(total, dtype=torch.uint8, pin_memory=True)
            host.copy_(buf, non_blocking=True)
            torch.cuda.current_stream(dev).synchronize()
            buf = host
        elif home != dev:
            buf = buf.to(home)
    return deliver_views(buf, outputs, offs, n, channels, fmt)


# ---- gain-weighted remixes of the stems and the mix (mi_deliver_mix_*, demucs_amd/csrc/deliver_mix.hip) --------------------------
MIX_COLS = 15                      # include/demucs_amd.h: MI_MIX_*
MIX_GAINS_AT, MIX_CLIP_AT, MIX_MAX_SOURCES = 6, 11, 8      # the nine gains take the five words before CLIP


def mix_gains(mix, sources=None) -> list:
    """`mix` -- `{output name: {"mix" | source name: gain}}` -- checked, its gains rounded to float32 once, outputs in dict order.
    With `sources` it is resolved against them: `[(name, (g_mix, g_0 .. g_{S-1}))]`, a term that is not named having gain 0;
    without, what can be checked before the sources are known is, and `[(name, {key: gain})]` comes back.  Raises ValueError for
    an empty `mix`, an unknown source, a source literally named "mix", a non-finite gain, an output whose gains are all 0, or more
    than 8 sources."""
    import numpy as np
    if not isinstance(mix, dict) or not mix:
        raise ValueError(f"mix: a non-empty {{output name: {{'mix' | source name: gain}}}} is expected, got {mix!r}")
    if sources is not None:
        sources = list(sources)
        if len(sources) > MIX_MAX_SOURCES:
            raise ValueError(f"mix: at most {MIX_MAX_SOURCES} sources, got {len(sources)}")
        if "mix" in sources:
            raise ValueError("mix: a source is named 'mix', the name of the input mix in a remix; rename the source")
    out = []
    for name, gains in mix.items():
        if not isinstance(name, str):
            raise ValueError(f"mix: an output name is a string, got {name!r}")
        if not isinstance(gains, dict):
            raise ValueError(f"mix: output {name!r} needs {{'mix' | source name: gain}}, got {gains!r}")
        vals = {}
        for key, g in gains.items():
            if sources is not None and key != "mix" and key not in sources:
                raise ValueError(f"mix: output {name!r} names {key!r}, which is neither 'mix' nor one of the separated sources {sources}")
            if isinstance(g, (bool, str, bytes)) or not isinstance(key, str):
                raise ValueError(f"mix: output {name!r} needs {{'mix' | source name: gain}}, got {key!r}: {g!r}")
            try:
                with np.errstate(over="ignore"):
                    v = np.float32(g)
            except (TypeError, ValueError):
                raise ValueError(f"mix: the gain of {key!r} in output {name!r} must be a number, got {g!r}") from None
            if not np.isfinite(v):
                raise ValueError(f"mix: the gain of {key!r} in output {name!r} must be finite in float32, got {g!r}")
            vals[key] = float(v)
        if not any(v != 0 for v in vals.values()):
            raise ValueError(f"mix: every gain of output {name!r} is 0; it would be silence")
        out.append((name, vals))
    if sources is None:
        return out
    return [(name, tuple(vals.get(k, 0.0) for k in ["mix"] + sources)) for name, vals in out]


def mix_outputs(gains) -> list:
    """[(name, None, index)] of resolved remixes, the shape `deliver_layout` and `deliver_views` take."""
    return [(name, None, i) for i, (name, _) in enumerate(gains)]


def mix_identity(gains) -> tuple:
    """Resolved remixes as `TrackPeaks.mix` keeps them."""
    return tuple((name, tuple(g)) for name, g in gains)


def mix_rows(gains, src: int, n: int, origin: int, pitch: int, affine, clip: int, slot0: int, fmt: str, offs) -> list:
    """mi_deliver_mix_pcm's rows (MI_MIX_*) for resolved remixes of `n` frames of the stems at device address `src`.  `origin` is
    the device address of the mix's frame 0 (channel rows `pitch` floats apart; 0: no remix reads it), `affine` (mean, s) when it is
    stored normalised.  Remix i names peak slot `slot0 + i`; `offs` None: rows without a destination (mi_deliver_mix_peaks_update)."""
    import numpy as np
    aff = 0 if affine is None else int(np.array(affine, dtype=np.float32).view(np.int64)[0])
    rows = []
    for i, (_, g) in enumerate(gains):
        packed = np.zeros(2 * (MIX_CLIP_AT - MIX_GAINS_AT), dtype=np.float32)
        packed[:len(g)] = g
        rows += [src, n, origin, pitch, aff, int(affine is not None), *packed.view(np.int64).tolist(), clip, slot0 + i,
                 _FORMATS[fmt][0], 0 if offs is None else offs[i]]
    return rows


# ---- remixes whose gains change along the track (mi_deliver_mix_auto_*, demucs_amd/csrc/deliver_mix_auto.hip) ---------------------
AUTO_COLS, AUTO_CHG_COLS = 18, 7   # include/demucs_amd.h: MI_AUTO_* (MI_MIX_*'s columns, then T0, CHG_OFF, CHG_N), MI_AUTO_CHG_*
AUTO_GAIN_MAX = 2.0 ** 64          # of a change's gains: the difference of two cannot overflow float32


def mix_changes(changes, gains, sources=None) -> dict:
    """`changes` -- `{output name: [(at, ramp, {"mix" | source name: gain}), ...]}` -- checked and ordered by `at` against `gains`
    (what `mix_gains` returned, in either form: its output names are what a change may name).  From track position `at` (model-rate
    frames) the output's gains move to the named ones over `ramp` frames (`0`: a step; a term that is not named has gain 0, and all
    of them may be 0: a fade to silence); frame `at` still has the old gains, frame `at + ramp` is the first with the new ones.
    With `sources` the gains are resolved as `mix_gains` resolves them: `{name: [(at, ramp, (g_mix, g_0 .. g_{S-1}))]}`; without,
    `{name: [(at, ramp, {key: gain})]}`.  Outputs without a change are left out, so None and `{}` give `{}`.  Raises ValueError for
    an unknown output or term, a gain that is not finite or above 2**64 in magnitude, a negative or fractional `at` or `ramp`, and
    changes of one output that overlap (`at[i] < at[i-1] + ramp[i-1]`)."""
    import numpy as np
    if changes is None:
        return {}
    if not isinstance(changes, dict):
        raise ValueError(f"changes: {{output name: [(at, ramp, {{'mix' | source name: gain}}), ...]}} is expected, got {changes!r}")
    names = [name for name, _ in gains]
    if sources is not None:
        sources = list(sources)
    out = {}
    for name, items in changes.items():
        if name not in names:
            raise ValueError(f"changes: {name!r} is none of the outputs {names}")
        if not isinstance(items, (list, tuple)):
            raise ValueError(f"changes: output {name!r} needs a list of (at, ramp, gains), got {items!r}")
        rows = []
        for item in items:
            if not isinstance(item, (list, tuple)) or len(item) != 3 or not isinstance(item[2], dict):
                raise ValueError(f"changes: output {name!r} needs (at, ramp, {{'mix' | source name: gain}}), got {item!r}")
            at, ramp, g = item
            for what, v in (("at", at), ("ramp", ramp)):
                if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or v != v or int(v) != v or v < 0 \
                        or v >= 2 ** 61:
                    raise ValueError(f"changes: `{what}` of output {name!r} is a frame count >= 0, got {v!r}")
            vals = {}
            for key, x in g.items():
                if not isinstance(key, str) or (sources is not None and key != "mix" and key not in sources):
                    raise ValueError(f"changes: output {name!r} names {key!r}, which is neither 'mix' nor one of the separated "
                                     f"sources {sources}")
                if isinstance(x, (bool, str, bytes)):
                    raise ValueError(f"changes: the gain of {key!r} in output {name!r} must be a number, got {x!r}")
                try:
                    with np.errstate(over="ignore"):
                        v = np.float32(x)
                except (TypeError, ValueError):
                    raise ValueError(f"changes: the gain of {key!r} in output {name!r} must be a number, got {x!r}") from None
                if not np.isfinite(v) or abs(float(v)) > AUTO_GAIN_MAX:
                    raise ValueError(f"changes: the gain of {key!r} in output {name!r} must be finite and at most 2**64 in magnitude, "
                                     f"got {x!r}")
                vals[key] = float(v)
            rows.append((int(at), int(ramp), vals if sources is None else tuple(vals.get(k, 0.0) for k in ["mix"] + sources)))
        rows.sort(key=lambda r: r[0])                       # stable: changes at one position keep the order they were given in
        for prev, cur in zip(rows, rows[1:]):
            if cur[0] < prev[0] + prev[1]:
                raise ValueError(f"changes: output {name!r} has a change at {cur[0]} before the ramp from {prev[0]} ends at "
                                 f"{prev[0] + prev[1]}; changes of one output do not overlap")
        if rows:
            out[name] = rows
    return out


def auto_span(base, schedule, t0: int, n: int):
    """What a call that delivers track positions [t0, t0 + n) needs of one output's ordered `schedule` [(at, ramp, gains)] whose
    gains before it are `base`: `(gains in force before the listed changes, the listed changes, how many are behind)`.  A change is
    behind once its ramp has ended at or before t0 (frame at + ramp has the new gains exactly), and those form a prefix; listed are
    the ones after them that begin before t0 + n."""
    done = 0
    while done < len(schedule) and schedule[done][0] + schedule[done][1] <= t0:
        base = schedule[done][2]
        done += 1
    end = done
    while end < len(schedule) and schedule[end][0] < t0 + n:
        end += 1
    return tuple(base), list(schedule[done:end]), done


def auto_table(rows, t0s, changes) -> list:
    """mi_deliver_mix_auto_pcm's table (MI_AUTO_*) from `mix_rows`' words `rows` (their gains being each remix's base gains), the
    track position `t0s[i]` of remix i's frame 0 and its changes `changes[i]` [(at, ramp, resolved gains)]: the rows first, the
    changes of all of them behind, each row naming where its own begin."""
    import numpy as np
    n = len(rows) // MIX_COLS
    head, tail = [], []
    for i in range(n):
        head += rows[i * MIX_COLS:(i + 1) * MIX_COLS] + [t0s[i], n * AUTO_COLS + len(tail), len(changes[i])]
        for at, ramp, g in changes[i]:
            packed = np.zeros(2 * (MIX_CLIP_AT - MIX_GAINS_AT), dtype=np.float32)
            packed[:len(g)] = g
            tail += [at, ramp, *packed.view(np.int64).tolist()]
    return head + tail


def deliver_mix(origin: torch.Tensor, stems: dict, mix: dict, clip="rescale", fmt: str = "i16", changes=None) -> dict:
    """Gain-weighted remixes of one separated track, what a user of the reference writes after `separate_tensor` as
    `save_audio(sum(g * x for ...), path, clip=clip)`: `{name: (n, channels) frames}` in `mix`'s order, `mix` being `{output
    name: {"mix" | source name: gain}}` ("mix" is `origin`).  Per sample `acc = 0`, then `acc = acc + g * x` for the mix first and
    the sources in the stems' order, every product and sum rounded to float32 and a term with gain 0 left out (never read: a NaN
    in a muted stem stays out); then `prevent_clip(·, clip)` with the peak per output, `i16_pcm` ("i16") or float32 ("f32"), the
    channels interleaved.  `{"mix": 1, STEM: -1}` is the reference's "minus" output, gains of 1 on all sources but one its "add".
    All remixes of the track take ONE `mi_deliver_mix_peaks` launch (only for "rescale") and ONE `mi_deliver_mix_pcm` launch;
    host stems come back on the host by one D2H of the byte buffer.

    `changes` (`mix_changes`: `{output: [(at, ramp, {term: gain}), ...]}`) moves an output's gains along the track: they are
    `mix`'s until a change, and from frame `at` move to the change's over `ramp` frames, `g = P + (G - P) * (float32(k) /
    float32(ramp))` at frame `at + k`, each operation rounded to float32; a term is left out at exactly the samples where its gain
    is 0.  The launches are then `mi_deliver_mix_auto_peaks` / `mi_deliver_mix_auto_pcm`, still one each; None or `{}` is the call
    without it."""
    names = list(stems)
    gains = mix_gains(mix, names)
    schedule = mix_changes(changes, gains, names)
    outputs = mix_outputs(gains)
    code = clip_code(clip)
    if fmt not in _FORMATS:
        raise ValueError(f"Invalid format {fmt!r}: 'i16' or 'f32'")
    tensors = [stems[k] for k in names]
    for t in tensors:
        if not t.dtype.is_floating_point:
            raise TypeError(f"deliver_mix: a floating-point tensor is expected, got {t.dtype}")
        if t.dim() != 2 or t.shape != tensors[0].shape:
            raise ValueError(f"deliver_mix: every stem is (channels, n), got {[tuple(x.shape) for x in tensors]}")
    channels, n = tensors[0].shape
    home = tensors[0].device
    if n == 0 or channels == 0:
        return {name: torch.empty(n, channels, dtype=_FORMATS[fmt][1], device=home) for name, _ in gains}
    dev = _engine_device(*tensors)
    with torch.cuda.device(dev):
        block = _stems_block(tensors, dev)
        mixed = any(g[0] != 0 for _, g in gains) or any(g[0] != 0 for rows in schedule.values() for _, _, g in rows)
        org = _stage(origin, dev, "deliver_mix") if mixed else None
        if org is not None and org.shape != (channels, n):
            raise ValueError(f"deliver_mix: the mix is {tuple(org.shape)}, the stems are {(channels, n)}")
        offs, total = deliver_layout(outputs, n, channels, fmt)
        rows = mix_rows(gains, block.data_ptr(), n, 0 if org is None else org.data_ptr(), n, None, code, 0, fmt, offs)
        auto, head = "", ()
        if schedule:                        # MI_AUTO_* rows with their changes behind them; the entries take the table's length
            rows = auto_table(rows, [0] * len(gains), [schedule.get(name, []) for name, _ in gains])
            auto, head = "_auto", (len(rows),)
        table = torch.tensor(rows, dtype=torch.int64).to(dev)
        buf = torch.empty(total, dtype=torch.uint8, device=dev)
        lib, stream = _lib.load(), C.c_void_p(_lib.current_stream_ptr())
        peaks = None
        if code == _CLIP_MODES["rescale"]:
            peaks = torch.empty(len(outputs), dtype=torch.int32, device=dev)
            name = f"mi_deliver_mix{auto}_peaks"
            _lib.check(getattr(lib, name)(table.data_ptr(), *head, len(outputs), n, len(names), channels, peaks.data_ptr(),
                                          len(outputs), total, stream), name)
        name = f"mi_deliver_mix{auto}_pcm"
        _lib.check(getattr(lib, name)(table.data_ptr(), *head, len(outputs), n, len(names), channels,
                                      peaks.data_ptr() if peaks is not None else None, 0 if peaks is None else len(outputs),
                                      buf.data_ptr(), total, stream), name)
        if home.type == "cpu":
            host = torch.empty(total, dtype=torch.uint8, pin_memory=True)
            host.copy_(buf, non_blocking=True)
            torch.cuda.current_stream(dev).synchronize()
            buf = host
        elif home != dev:
            buf = buf.to(home)
    return deliver_views(buf, outputs, offs, n, channels, fmt)


def wav_header(frames, samplerate: int, channels: int, fmt: str = "i16") -> bytes:
    """The RIFF / WAVE header in front of `deliver`'s frames: 44 bytes of PCM header for "i16"; format tag 3 (IEEE float) with
    the `fact` chunk that format needs for "f32".  `frames=None` writes 0xFFFFFFFF sizes, for a live stream of unknown length."""
    import struct
    if fmt not in _FORMATS:
        raise ValueError(f"Invalid format {fmt!r}: 'i16' or 'f32'")
    samplerate, channels = int(samplerate), int(channels)
    if samplerate <= 0 or not 1 <= channels <= 65535:
        raise ValueError(f"wav_header: sample rate {samplerate} and {channels} channels do not fit a WAVE header")
    width = _FORMATS[fmt][2]
    align = channels * width
    head = 58 if fmt == "f32" else 44
    if frames is None:
        data = riff = count = 0xFFFFFFFF
    else:
        count = int(frames)
        data = count * align
        riff = head - 8 + data
        if count < 0 or riff > 0xFFFFFFFF:
            raise ValueError(f"wav_header: {frames} frames do not fit a WAVE file's 32-bit sizes")
    if fmt == "i16":
        return (b"RIFF" + struct.pack("<I", riff) + b"WAVEfmt " +
                struct.pack("<IHHIIHH", 16, 1, channels, samplerate, samplerate * align, align, 16) +
                b"data" + struct.pack("<I", data))
    return (b"RIFF" + struct.pack("<I", riff) + b"WAVEfmt " +
            struct.pack("<IHHIIHHH", 18, 3, channels, samplerate, samplerate * align, align, 32, 0) +
            b"fact" + struct.pack("<II", 4, count) + b"data" + struct.pack("<I", data))


# ---- evaluation: the nSDR of stems against reference stems (demucs/evaluate.py:30-43; demucs_amd/csrc/score.hip) -----------------
SDR_SLOTS = 131072                 # demucs_amd/csrc/sdr_sums.h: kSdrSlots, position p of a track belongs to slot p % SDR_SLOTS
SDR_MAX_SOURCES = 8
SDR_DELTA = 1e-7                   # evaluate.py:37


def _check_n_sources(n_sources, what: str) -> int:
    if isinstance(n_sources, bool) or int(n_sources) != n_sources or not 1 <= n_sources <= SDR_MAX_SOURCES:
        raise ValueError(f"{what}: 1 to {SDR_MAX_SOURCES} sources, got {n_sources!r}")
    return int(n_sources)


def _sdr_scores(sums: torch.Tensor) -> torch.Tensor:
    """evaluate.py:40-42 in float64 on the host: (..., 2) raw (num, den) -> 10 log10((num + 1e-7) / (den + 1e-7))."""
    sums = sums.to(device="cpu", dtype=torch.float64)
    return 10 * torch.log10((sums[..., 0] + SDR_DELTA) / (sums[..., 1] + SDR_DELTA))


def sdr_sums(references: torch.Tensor, estimates: torch.Tensor) -> torch.Tensor:
    """The raw float64 (B, S, 2) sums (num, den) of `new_sdr` as `mi_sdr` leaves them, on the engine device."""
    if references.dim() != 4 or estimates.dim() != 4:
        raise ValueError("new_sdr: (batch, sources, channels, length) tensors are expected")
    if references.shape != estimates.shape:
        raise ValueError(f"new_sdr: references {tuple(references.shape)} and estimates {tuple(estimates.shape)} differ in shape")
    B, S, ch, L = references.shape
    _check_n_sources(S, "new_sdr")
    if ch < 1:
        raise ValueError("new_sdr: at least one channel")
    dev = _engine_device(references, estimates)
    ref, est = _stage(references, dev, "new_sdr"), _stage(estimates, dev, "new_sdr")
    sums = torch.zeros(B, S, 2, dtype=torch.float64, device=dev)
    if B:
        lib = _lib.load()
        with torch.cuda.device(dev):
            state = torch.empty(lib.mi_sdr_state_bytes(S), dtype=torch.uint8, device=dev)
            scratch = torch.empty(lib.mi_sdr_scratch_bytes(S), dtype=torch.uint8, device=dev)
            _lib.check(lib.mi_sdr(ref.data_ptr(), est.data_ptr(), B, S, ch, L, state.data_ptr(), scratch.data_ptr(), sums.data_ptr(),
                                  C.c_void_p(_lib.current_stream_ptr())), "mi_sdr")
    return sums


def new_sdr(references: torch.Tensor, estimates: torch.Tensor) -> torch.Tensor:
    """demucs/evaluate.py:30-43, the SDR of the MDX challenge definition: two (batch, sources, channels, length) floating
    tensors -> float64 (batch, sources) scores `10 log10((sum ref^2 + 1e-7) / (sum (ref - est)^2 + 1e-7))`.  The two sums are
    float64 reductions of the float32 samples on the engine device (`mi_sdr`, in the fixed order of demucs_amd/csrc/sdr_sums.h: the
    same bits as an `SdrStream` fed the tracks in pieces); the logarithm is taken on the 2 x sources returned doubles on the host.
    Host tensors are staged H2D as `prevent_clip` stages them, other floating dtypes are scored as float32; the result comes back on
    the references' device.  NaN and Inf samples reach the score as in the reference; length 0 gives 0."""
    return _sdr_scores(sdr_sums(references, estimates)).to(references.device)


class TrackScore:
    """The `new_sdr` score of one track: per source `nsdr` (dB), and the raw sums `num` = sum ref^2 and `den` = sum (ref - est)^2 it
    comes from (before the 1e-7), as read-only float64 arrays, with the `length` scored in samples per channel.  Immutable; equal
    when every bit is (every NaN counting as one value)."""
    __slots__ = ("nsdr", "num", "den", "length")

    def __init__(self, nsdr, num, den, length):
        import numpy as np
        arrays = []
        for name, v in (("nsdr", nsdr), ("num", num), ("den", den)):
            a = np.array(v, dtype=np.float64)
            if a.ndim != 1 or not 1 <= a.size <= SDR_MAX_SOURCES:
                raise ValueError(f"TrackScore: {name} must hold one value per source (1 to {SDR_MAX_SOURCES}), got shape {a.shape}")
            a.setflags(write=False)
            arrays.append(a)
        if len({a.size for a in arrays}) != 1:
            raise ValueError("TrackScore: nsdr, num and den must have one length")
        if isinstance(length, bool) or not isinstance(length, (int, np.integer)) or length < 0:
            raise ValueError(f"TrackScore: length must be a non-negative integer, got {length!r}")
        for name, v in zip(self.__slots__, arrays + [int(length)]):
            object.__setattr__(self, name, v)

    def __setattr__(self, name, value):
        raise AttributeError("TrackScore is immutable")

    def __delattr__(self, name):
        raise AttributeError("TrackScore is immutable")

    def _key(self):
        return (*(tuple("nan" if math.isnan(v) else float(v).hex() for v in a) for a in (self.nsdr, self.num, self.den)), self.length)

    def __eq__(self, other):
        return isinstance(other, TrackScore) and self._key() == other._key()

    def __hash__(self):
        return hash(self._key())

    def __repr__(self):
        return (f"TrackScore(nsdr={self.nsdr.tolist()!r}, num={self.num.tolist()!r}, den={self.den.tolist()!r}, "
                f"length={self.length})")

    @classmethod
    def from_sums(cls, sums: torch.Tensor, length: int) -> "TrackScore":
        """From the (sources, 2) raw sums of `mi_sdr` / `mi_sdr_finish`."""
        sums = sums.to(device="cpu", dtype=torch.float64)
        return cls(_sdr_scores(sums).numpy(), sums[:, 0].numpy(), sums[:, 1].numpy(), length)


class SdrStream:
    """`new_sdr` for a track whose references and estimates arrive block by block, each at its own pace: `push_references(block)`
    and `push_estimates(block)` are independent, and the stream scores the positions both sides have reached
    (`mi_sdr_update`, demucs_amd/csrc/score.hip).  `finish()` returns the `TrackScore`, whose bits depend on the two tracks alone:
    not on the block sizes, nor on the interleaving of the two kinds of push, and they are those of `new_sdr` on the whole tracks.

    A block is (n_sources, channels, n) floating, on the host (one H2D) or a device; a device block is read where it lies (a slice
    of a longer tensor keeps its stride) and is held, not copied, until its last sample is scored, so the caller must not write
    to it before then.  With `pcm=` and `src_channels=` a references block is instead a list of `n_sources` chunks of interleaved
    wire PCM (`PCM_FORMATS`), one per source as MusDB keeps its stems in separate files, each as `ConvertStream` takes them: a
    chunk may end inside a frame (one `PcmFeed` per source carries the rest), but the chunks of one push must complete the same
    number of frames.  The kernel decodes them where they lie under `mi_pcm_planar`'s rules.

    Device memory: the state (`mi_sdr_state_bytes`: 2 MiB per source) plus the surplus of whichever side is ahead -- references
    normally lead the estimates by a stream's `latency` -- which is as large as the caller lets the two drift; `device_bytes()`
    reports both.  A partly scored block stays allocated until it is used up.  `scores()` reads the state at any time."""

    def __init__(self, n_sources: int, channels: int, device="cuda", pcm=None, src_channels=None):
        self.n_sources = _check_n_sources(n_sources, "SdrStream")
        self.channels = int(channels)
        if self.channels < 1:
            raise ValueError(f"channels must be >= 1, got {channels}")
        self.feeds = None
        if pcm is not None:
            if src_channels is None:
                raise ValueError("a PCM stream needs src_channels=: the frames do not say how many channels they hold")
            self.feeds = [PcmFeed(pcm, src_channels) for _ in range(self.n_sources)]
            check_stream_channels(self.feeds[0].src_channels, self.channels)
        dev = torch.device(device)
        if dev.type != "cuda":
            raise _lib.EngineError("demucs_amd.audio.SdrStream only runs on a GPU device (MI355X)")
        self.device = dev
        self.references_pushed = self.estimates_pushed = self.scored = 0
        self.finished = False
        self._state = None
        self._refs, self._ests = [], []           # blocks not yet used up: [rows or per-source chunks, row stride, n, frames used]

    # ---- bookkeeping ------------------------------------------------------------------------------------------------------------
    def _frame_bytes(self, pcm: bool) -> int:
        if pcm:
            return self.n_sources * self.feeds[0].frame_bytes
        return self.n_sources * self.channels * 4

    def device_bytes(self) -> int:
        """The state plus the samples pushed and not yet scored."""
        held = sum((n - used) * self._frame_bytes(isinstance(rows, list)) for rows, _, n, used in self._refs + self._ests)
        return held + (0 if self._state is None else self._state.numel())

    @property
    def trailing_bytes(self) -> int:
        """Bytes of an incomplete last frame of the PCM references, per source: carried to the next push, dropped by `finish()`."""
        return 0 if self.feeds is None else self.feeds[0].trailing_bytes

    def _on(self):
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        return torch.cuda.device(self.device)

    def _rows(self, block, what: str):
        S, ch = self.n_sources, self.channels
        if not isinstance(block, torch.Tensor) or block.dim() != 3 or tuple(block.shape[:2]) != (S, ch):
            shape = tuple(block.shape) if isinstance(block, torch.Tensor) else type(block).__name__
            raise ValueError(f"{what}: expected a ({S}, {ch}, n) block, got {shape}")
        if not block.dtype.is_floating_point:
            raise TypeError(f"{what}: a floating-point tensor is expected, got {block.dtype}")
        n = block.shape[2]
        if n == 0:
            return None
        with self._on():
            t = block.to(device=self.device, dtype=torch.float32)
            stride = t.stride(1) if ch > 1 else t.stride(0) if S > 1 else n
            if not ((n == 1 or t.stride(2) == 1) and stride >= n and (ch == 1 or S == 1 or t.stride(0) == ch * stride)):
                t, stride = t.contiguous(), n
        return [t, stride, n, 0]

    def _drain(self) -> None:
        """Scores what both sides hold: one `mi_sdr_update` per overlap of a references block with an estimates block."""
        lib = _lib.load()
        while self._refs and self._ests:
            r, e = self._refs[0], self._ests[0]
            n = min(r[2] - r[3], e[2] - e[3])
            with self._on():
                if self._state is None:
                    self._state = torch.zeros(lib.mi_sdr_state_bytes(self.n_sources), dtype=torch.uint8, device=self.device)
                if isinstance(r[0], list):
                    feed = self.feeds[0]
                    ptrs = (C.c_void_p * self.n_sources)(*[t.data_ptr() + r[3] * feed.frame_bytes for t in r[0]])
                    code, src_ch = PCM_FORMATS[feed.fmt][0], feed.src_channels
                else:
                    ptrs = (C.c_void_p * 1)(r[0].data_ptr() + 4 * r[3])
                    code, src_ch = PCM_PLANAR, self.channels
                _lib.check(lib.mi_sdr_update(ptrs, code, src_ch, r[1], e[0].data_ptr() + 4 * e[3], e[1], self.n_sources, self.channels, n,
                                             self.scored, self._state.data_ptr(), C.c_void_p(_lib.current_stream_ptr())),
                           "mi_sdr_update")
            self.scored += n
            for queue in (self._refs, self._ests):
                queue[0][3] += n
                if queue[0][3] == queue[0][2]:
                    queue.pop(0)

    # ---- public -----------------------------------------------------------------------------------------------------------------
    def push_references(self, block) -> None:
        if self.finished:
            raise RuntimeError("push after finish()")
        if self.feeds is None:
            seg = self._rows(block, "push_references")
        else:
            if not isinstance(block, (list, tuple)) or len(block) != self.n_sources:
                got = len(block) if isinstance(block, (list, tuple)) else type(block).__name__
                raise ValueError(f"push_references: expected a list of {self.n_sources} PCM chunks, one per source, got {got}")
            blks = [feed.accept(chunk) for feed, chunk in zip(self.feeds, block)]
            if len({b.n for b in blks}) != 1:
                raise ValueError(f"push_references: the chunks of one push must complete the same number of frames, got "
                                 f"{[b.n for b in blks]}")
            for feed, b in zip(self.feeds, blks):
                feed.commit(b)
            seg = None
            if blks[0].n:
                keep = []
                with self._on():
                    seg = [[b.on_device(self.device, keep) for b in blks], 0, blks[0].n, 0]
        if seg is not None:
            self.references_pushed += seg[2]
            self._refs.append(seg)
            self._drain()

    def push_estimates(self, block) -> None:
        if self.finished:
            raise RuntimeError("push after finish()")
        seg = self._rows(block, "push_estimates")
        if seg is not None:
            self.estimates_pushed += seg[2]
            self._ests.append(seg)
            self._drain()

    def scores(self) -> TrackScore:
        """The `TrackScore` of the `scored` positions both sides have reached so far; the state is only read."""
        lib = _lib.load()
        with self._on():
            sums = torch.zeros(self.n_sources, 2, dtype=torch.float64, device=self.device)
            if self._state is not None:
                scratch = torch.empty(lib.mi_sdr_scratch_bytes(self.n_sources), dtype=torch.uint8, device=self.device)
                _lib.check(lib.mi_sdr_finish(self._state.data_ptr(), self.n_sources, scratch.data_ptr(), sums.data_ptr(),
                                             C.c_void_p(_lib.current_stream_ptr())), "mi_sdr_finish")
            return TrackScore.from_sums(sums, self.scored)

    def finish(self) -> TrackScore:
        if self.finished:
            raise RuntimeError("finish() called twice")
        if self.references_pushed != self.estimates_pushed:
            raise ValueError(f"the references ended after {self.references_pushed} samples and the estimates after "
                             f"{self.estimates_pushed}: a score needs both tracks whole")
        if self.scored == 0:
            raise ValueError("the stream ended before any sample was pushed")
        self.finished = True
        return self.scores()


def summarise_scores(tracks, sources) -> dict:
    """The aggregation of demucs/evaluate.py:157-173 for the `nsdr` metric, on the host.  `tracks` maps a track's name to its
    scores: a `TrackScore` whose entries follow `sources`, or a `{source: score}` mapping whose scores are numbers or one-source
    `TrackScore`s (an `SdrStream` per source).  Per source the per-track values -- `nanmedian` of a track's one value is that
    value -- give `nsdr_<source>` (their mean) and `nsdr_med_<source>` (their median); `nsdr` and `nsdr_med` average those over
    the sources.  A NaN score makes the figures it enters NaN, as numpy's mean and median do in the reference."""
    import numpy as np
    sources = list(sources)
    if not tracks or not sources:
        raise ValueError("summarise_scores: at least one track and one source")

    def value(entry, source, idx):
        if isinstance(entry, TrackScore):
            if len(entry.nsdr) != len(sources):
                raise ValueError(f"summarise_scores: a TrackScore of {len(entry.nsdr)} sources for {len(sources)} names")
            return float(entry.nsdr[idx])
        v = entry[source]
        if isinstance(v, TrackScore):
            if len(v.nsdr) != 1:
                raise ValueError(f"summarise_scores: the score of {source!r} must be one source's, got {len(v.nsdr)}")
            return float(v.nsdr[0])
        return float(v)

    result, avg, avg_of_medians = {}, 0.0, 0.0
    for idx, source in enumerate(sources):
        medians = np.array([value(tracks[name], source, idx) for name in tracks], dtype=np.float64)
        mean, median = float(np.mean(medians)), float(np.median(medians))
        result["nsdr_" + source] = mean
        result["nsdr_med_" + source] = median
        avg += mean / len(sources)
        avg_of_medians += median / len(sources)
    result["nsdr"] = avg
    result["nsdr_med"] = avg_of_medians
    return result


# ---- loudness of remixes: ITU-R BS.1770-4 / EBU R 128 (mi_loudness_update, demucs_amd/csrc/loudness.hip) -------------------------
LOUD_COLS = 22                     # include/demucs_amd.h: MI_LOUD_* (MI_MIX_*'s columns up to the gains, then its own)
LOUD_CHUNK = 1 << 20               # samples per push of the whole-track call: bounds its work area
LOUD_ABSOLUTE_GATE = -70.0         # LUFS
LOUD_RELATIVE_GATE = -10.0         # LU below the loudness of the blocks over the absolute gate


def _check_loudness_format(samplerate, channels) -> None:
    if isinstance(samplerate, bool) or int(samplerate) != samplerate or samplerate <= 0:
        raise ValueError(f"loudness: the sample rate must be a positive integer, got {samplerate!r}")
    if int(samplerate) % 10:
        raise ValueError(f"loudness: the sample rate {samplerate} is no multiple of 10: a 100 ms sub-block is no whole number of samples")
    if isinstance(channels, bool) or int(channels) != channels or not 1 <= channels <= 2:
        raise ValueError(f"loudness: 1 or 2 channels (both weighted 1), got {channels!r}; the surround weights are not implemented")


def k_weighting(samplerate):
    """The K-weighting of BS.1770-4 at `samplerate` as a float64 array `[stage][b | a][3]`: the shelf, then the high-pass, each
    `y[n] = b0 x[n] + b1 x[n-1] + b2 x[n-2] - a1 y[n-1] - a2 y[n-2]` with `a0 = 1`.  At 48 000 Hz these are the recommendation's
    tabulated coefficients (to 9e-16); at other rates the same analogue prototypes through the bilinear transform."""
    import numpy as np
    fs = float(samplerate)
    if not fs > 0:
        raise ValueError(f"loudness: the sample rate must be positive, got {samplerate!r}")
    f0, gain, q = 1681.974450955533, 3.999843853973347, 0.7071752369554196
    k = math.tan(math.pi * f0 / fs)
    vh = 10.0 ** (gain / 20.0)
    vb = vh ** 0.4996667741545416
    a0 = 1.0 + k / q + k * k
    shelf = [[(vh + vb * k / q + k * k) / a0, 2.0 * (k * k - vh) / a0, (vh - vb * k / q + k * k) / a0],
             [1.0, 2.0 * (k * k - 1.0) / a0, (1.0 - k / q + k * k) / a0]]
    f0, q = 38.13547087602444, 0.5003270373238773
    k = math.tan(math.pi * f0 / fs)
    d = 1.0 + k / q + k * k
    high = [[1.0, -2.0, 1.0], [1.0, 2.0 * (k * k - 1.0) / d, (1.0 - k / q + k * k) / d]]
    return np.array([shelf, high], dtype=np.float64)


def loudness_warmup(samplerate) -> int:
    """Samples a sub-block's recursion runs from zero state before its first counted sample (loudness.hip): by then the
    high-pass's response to everything earlier is below float64 rounding."""
    return 16384 * -(-int(samplerate) // 48000)


def _block_powers(energies, hop: int):
    """P[j] of the 400 ms gating blocks (75 % overlap) from (channels, Hn) sub-block energies; empty below 4 sub-blocks."""
    import numpy as np
    e = np.asarray(energies, dtype=np.float64)
    if e.shape[-1] < 4:
        return np.zeros(0, dtype=np.float64)
    return (e[:, :-3] + e[:, 1:-2] + e[:, 2:-1] + e[:, 3:]).sum(0) / (4.0 * hop)


def _lufs(power):
    import numpy as np
    with np.errstate(divide="ignore", invalid="ignore"):
        return -0.691 + 10.0 * np.log10(power)


def gated_loudness(energies, hop: int) -> float:
    """Integrated loudness (LUFS) from (channels, Hn) sub-block energies of `hop` samples: BS.1770-4's absolute gate at -70 LUFS
    and relative gate 10 LU below the loudness of what passed it.  -inf when no block passes or there are fewer than 4
    sub-blocks; NaN when an energy is NaN."""
    import numpy as np
    e = np.asarray(energies, dtype=np.float64)
    if np.isnan(e).any():
        return float("nan")
    power = _block_powers(e, hop)
    l = _lufs(power)
    keep = l > LOUD_ABSOLUTE_GATE
    if not keep.any():
        return float("-inf")
    keep &= l > _lufs(power[keep].mean()) + LOUD_RELATIVE_GATE
    if not keep.any():
        return float("-inf")
    return float(_lufs(power[keep].mean()))


class TrackLoudness:
    """What a loudness pass over a track found (`audio.loudness`, `LoudnessStream`, `Separator.loudness_blocks`): per output the
    K-weighted energies of its 100 ms sub-blocks, from which every BS.1770-4 figure of the track follows on the host.

    `names` are the outputs, `sources` the separated sources their gains refer to, `mix` the outputs' identity `((output name,
    (g_mix, g_0 .. g_{S-1})), ...)` as `mix_gains` resolves it (`TrackPeaks.mix`'s form), `samplerate`, `channels` and `length`
    those of the measured frames, `energies` a read-only float64 array (outputs, channels, length // (samplerate // 10)).
    Immutable."""
    __slots__ = ("names", "sources", "samplerate", "channels", "length", "energies", "mix")

    def __init__(self, names, sources, samplerate, channels, length, energies, mix):
        import numpy as np
        for what, v in (("names", names), ("sources", sources)):
            if isinstance(v, (str, bytes)) or not all(isinstance(n, str) for n in v) or len(set(v)) != len(tuple(v)) or not len(v):
                raise ValueError(f"TrackLoudness: {what} must be a sequence of names, each once, got {v!r}")
        names, sources = tuple(names), tuple(sources)
        _check_loudness_format(samplerate, channels)
        if isinstance(length, bool) or not isinstance(length, (int, np.integer)) or length < 0:
            raise ValueError(f"TrackLoudness: length must be a non-negative integer, got {length!r}")
        try:
            mix = tuple((str(name), tuple(float(np.float32(g)) for g in gains)) for name, gains in mix)
        except (TypeError, ValueError):
            raise ValueError(f"TrackLoudness: mix must be ((output name, (g_mix, g_0, ...)), ...) as audio.mix_gains returns it, got "
                             f"{mix!r}") from None
        if tuple(name for name, _ in mix) != names or \
                not all(len(g) == 1 + len(sources) and all(np.isfinite(v) for v in g) for _, g in mix):
            raise ValueError(f"TrackLoudness: mix must name the outputs {list(names)} in order, each with finite gains for the mix and "
                             f"the {len(sources)} sources, got {mix!r}")
        e = np.array(energies, dtype=np.float64)
        want = (len(names), int(channels), int(length) // (int(samplerate) // 10))
        if e.shape != want:
            raise ValueError(f"TrackLoudness: the energies of {length} samples are {want} (outputs, channels, sub-blocks), got {e.shape}")
        e.setflags(write=False)
        for name, v in zip(self.__slots__, (names, sources, int(samplerate), int(channels), int(length), e, mix)):
            object.__setattr__(self, name, v)

    def __setattr__(self, name, value):
        raise AttributeError("TrackLoudness is immutable")

    def __delattr__(self, name):
        raise AttributeError("TrackLoudness is immutable")

    @property
    def hop(self) -> int:
        """Samples of a sub-block: 100 ms."""
        return self.samplerate // 10

    def _row(self, name: str):
        if name not in self.names:
            raise KeyError(f"output {name!r} is not among the measured outputs {list(self.names)}")
        return self.energies[self.names.index(name)]

    def integrated(self, name: str) -> float:
        """Integrated (gated) loudness of output `name` in LUFS; -inf for silence or less than 400 ms, NaN for a NaN sample."""
        return gated_loudness(self._row(name), self.hop)

    def momentary(self, name: str):
        """The loudness of every 400 ms gating block of output `name` (a block every 100 ms), in LUFS, ungated."""
        return _lufs(_block_powers(self._row(name), self.hop))

    def gain(self, name: str, target: float) -> float:
        """The linear gain that brings output `name` to `target` LUFS."""
        have = self.integrated(name)
        if not math.isfinite(have) or not math.isfinite(float(target)):
            raise ValueError(f"TrackLoudness: output {name!r} measures {have} LUFS; no gain brings that to {target} LUFS")
        return 10.0 ** ((float(target) - have) / 20.0)

    def normalised(self, target: float = -14.0, true_peaks=None, ceiling: float = -1.0) -> dict:
        """The measured remixes with every gain scaled so that each output reads `target` LUFS: `{output: {"mix" | source:
        gain}}`, what `deliver_mix` and `Delivery(mix=)` take.  With `true_peaks`, the `TrackTruePeaks` of the same remixes of
        the same track, an output whose peak that scale would lift over `ceiling` dBTP gets `true_peaks.gain_limit(name,
        ceiling)` instead and stays below the target loudness: R 128's other half."""
        if true_peaks is not None:
            if not isinstance(true_peaks, TrackTruePeaks):
                raise ValueError(f"TrackLoudness: true_peaks must be a TrackTruePeaks, got {type(true_peaks).__name__}")
            for what in ("names", "sources", "mix", "samplerate", "channels", "length"):
                if getattr(true_peaks, what) != getattr(self, what):
                    raise ValueError(f"TrackLoudness: the true peaks were measured with {what}={getattr(true_peaks, what)!r}, the "
                                     f"loudness with {getattr(self, what)!r}")
        terms = ("mix",) + self.sources
        out = {}
        for name, gains in self.mix:
            k = self.gain(name, target)
            if true_peaks is not None:
                k = min(k, true_peaks.gain_limit(name, ceiling))
            out[name] = {t: g * k for t, g in zip(terms, gains) if g != 0}
        return out

    def _key(self):
        return (self.names, self.sources, self.samplerate, self.channels, self.length, self.energies.tobytes(), self.mix)

    def __eq__(self, other):
        return isinstance(other, TrackLoudness) and self._key() == other._key()

    def __hash__(self):
        return hash(self._key())

    def __repr__(self):
        return (f"TrackLoudness(names={list(self.names)}, sources={list(self.sources)}, samplerate={self.samplerate}, "
                f"channels={self.channels}, length={self.length}, integrated={[self.integrated(n) for n in self.names]})")


def loud_rows(gains, src: int, src_pitch: int, n: int, origin: int, pitch: int, affine, before: int, hist_len: int, side: int,
              hist_start: int, hist_next: int, channels: int, e_pitch: int, work_pitch: int) -> list:
    """mi_loudness_update's rows (MI_LOUD_*) for resolved remixes of `n` frames from track position `before`.  Output i keeps its
    history at `(side, i)` of a (2, outputs, channels, hist_len) buffer, its energies at row i of (outputs, channels, e_pitch) and
    works in row i of (outputs, channels, work_pitch)."""
    import numpy as np
    aff = 0 if affine is None else int(np.array(affine, dtype=np.float32).view(np.int64)[0])
    per = channels * hist_len
    rows = []
    for i, (_, g) in enumerate(gains):
        packed = np.zeros(2 * (MIX_CLIP_AT - MIX_GAINS_AT), dtype=np.float32)
        packed[:len(g)] = g
        rows += [src, n, origin, pitch, aff, int(affine is not None), *packed.view(np.int64).tolist(), src_pitch, before, hist_len,
                 (side * len(gains) + i) * per, ((1 - side) * len(gains) + i) * per, hist_start, hist_next,
                 i * channels * e_pitch, e_pitch, i * channels * work_pitch, work_pitch]
    return rows


class LoudnessStream:
    """BS.1770-4 loudness of gain-weighted remixes of a track that arrives block by block, measured where the stems lie.
    `push(stems_block, origin=None)` takes the next `n >= 0` samples as a device float32 (sources, channels, n) and the mix of the
    same positions as (channels, n) (required when an output has a gain on "mix"; `affine=(mean, s)` when it is stored normalised,
    as a stream's window is); `finish()` returns the `TrackLoudness`.  `mix` is `deliver_mix`'s; None measures every source by
    itself.  The measured values are `deliver_mix(..., clip=None, fmt="f32")`'s, and the energies have the same bits for every
    partition of the track into pushes.

    Every push is ONE `mi_loudness_update` call for all outputs; nothing visits the host before `finish()`, which copies the
    energies once.  Device state: two sides of (outputs, channels, warm-up + hop) carried values, and the energies, 8 bytes per
    output, channel and 100 ms; a push also uses a work area of (outputs, channels, carried + n) floats for its duration."""

    def __init__(self, sources, channels: int, samplerate: int, mix=None, device="cuda"):
        self.sources = list(sources)
        _check_loudness_format(samplerate, channels)
        if not self.sources:
            raise ValueError("loudness: at least one source")
        if mix is None:
            mix = {name: {name: 1.0} for name in self.sources}
        self.gains = mix_gains(mix, self.sources)
        self.channels, self.samplerate = int(channels), int(samplerate)
        self.hop, self.warm = self.samplerate // 10, loudness_warmup(samplerate)
        self.mixed = any(g[0] != 0 for _, g in self.gains)
        dev = torch.device(device)
        if dev.type != "cuda":
            raise _lib.EngineError("demucs_amd.audio.LoudnessStream only runs on a GPU device (MI355X)")
        self.device = dev
        self.pushed = 0
        self.finished = False
        self._coef = k_weighting(self.samplerate)
        self._hist = self._energies = None
        self._side = self._h0 = 0

    @property
    def device_bytes(self) -> int:
        return sum(t.numel() * t.element_size() for t in (self._hist, self._energies) if t is not None)

    def _rows_of(self, t: torch.Tensor):
        """`t` as float32 on the stream's device with unit stride along time and evenly pitched rows, read in place when it
        already is (a span of a whole track's stems): (tensor, pitch)."""
        t = t.to(device=self.device, dtype=torch.float32)
        n = t.shape[-1]
        pitch = t.stride(-2)
        if t.stride(-1) != 1 or pitch < n or (t.dim() == 3 and t.stride(0) != self.channels * pitch):
            t, pitch = t.contiguous(), n
        return t, pitch

    def push(self, stems_block: torch.Tensor, origin=None, affine=None) -> None:
        if self.finished:
            raise RuntimeError("push after finish()")
        S, ch, R = len(self.sources), self.channels, len(self.gains)
        if not isinstance(stems_block, torch.Tensor) or stems_block.dim() != 3 or tuple(stems_block.shape[:2]) != (S, ch) or \
                not stems_block.dtype.is_floating_point:
            raise ValueError(f"loudness: expected a floating ({S}, {ch}, n) block of stems, got "
                             f"{tuple(getattr(stems_block, 'shape', ()))}")
        n = stems_block.shape[2]
        if self.mixed:
            if origin is None:
                raise ValueError("loudness: an output has a gain on 'mix'; push the mix of the same positions as origin=")
            if not isinstance(origin, torch.Tensor) or tuple(origin.shape) != (ch, n) or not origin.dtype.is_floating_point:
                raise ValueError(f"loudness: the mix is {tuple(getattr(origin, 'shape', ()))}, the stems are {(ch, n)}")
        if n == 0:
            return
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        dev, hop, warm = self.device, self.hop, self.warm
        with torch.cuda.device(dev):
            block, src_pitch = self._rows_of(stems_block)
            org, pitch = self._rows_of(origin) if self.mixed else (None, 0)
            hist_len = warm + hop
            if self._hist is None:
                self._hist = torch.zeros(2, R, ch, hist_len, device=dev)
            end = self.pushed + n
            done = end // hop
            if self._energies is None or self._energies.shape[2] < done:
                grown = torch.zeros(R, ch, max(done, 600, 0 if self._energies is None else 2 * self._energies.shape[2]),
                                    dtype=torch.float64, device=dev)
                if self._energies is not None:
                    grown[:, :, :self._energies.shape[2]] = self._energies
                self._energies = grown
            kept = self.pushed - self._h0
            nxt = max(0, done * hop - warm)
            work = torch.empty(R * ch * (kept + n), dtype=torch.float32, device=dev)
            rows = loud_rows(self.gains, block.data_ptr(), src_pitch, n, 0 if org is None else org.data_ptr(), pitch, affine,
                             self.pushed, hist_len, self._side, self._h0, nxt, ch, self._energies.shape[2], kept + n)
            table = torch.tensor(rows, dtype=torch.int64).to(dev)
            coef = (C.c_double * 10)(*[*self._coef[0, 0], *self._coef[0, 1, 1:], *self._coef[1, 0], *self._coef[1, 1, 1:]])
            _lib.check(_lib.load().mi_loudness_update(
                table.data_ptr(), R, kept + n, done - self.pushed // hop, S, ch, coef, hop, warm, self._hist.data_ptr(),
                self._hist.numel(), self._energies.data_ptr(), self._energies.numel(), work.data_ptr(), work.numel(),
                C.c_void_p(_lib.current_stream_ptr())), "mi_loudness_update")
        self._side, self._h0, self.pushed = 1 - self._side, nxt, end

    def finish(self) -> TrackLoudness:
        if self.finished:
            raise RuntimeError("finish() called twice")
        self.finished = True
        import numpy as np
        done = self.pushed // self.hop
        if done:
            energies = self._energies[:, :, :done].cpu().numpy()
        else:
            energies = np.zeros((len(self.gains), self.channels, 0), dtype=np.float64)
        return TrackLoudness([name for name, _ in self.gains], self.sources, self.samplerate, self.channels, self.pushed, energies,
                             mix_identity(self.gains))


def loudness(origin, stems: dict, mix=None, samplerate: int = 44100) -> TrackLoudness:
    """ITU-R BS.1770-4 / EBU R 128 loudness of gain-weighted remixes of one separated track, measured on the stems' device: the
    `TrackLoudness` of the frames `deliver_mix(origin, stems, mix, clip=None, fmt="f32")` returns, none of which is produced.
    `stems` is `{name: (channels, n)}` as `deliver_mix` takes it, `mix` its `{output: {"mix" | source: gain}}`; None measures
    every source by itself, and the mix as output "mix" when `origin` is given.  The track goes through a `LoudnessStream` in
    pushes of `LOUD_CHUNK` samples read in place, so the memory used beside the stems stays bounded."""
    names = list(stems)
    if mix is None:
        mix = {name: {name: 1.0} for name in names}
        if origin is not None:
            mix["mix"] = {"mix": 1.0}
    tensors = [stems[k] for k in names]
    for t in tensors:
        if not t.dtype.is_floating_point:
            raise TypeError(f"loudness: a floating-point tensor is expected, got {t.dtype}")
        if t.dim() != 2 or t.shape != tensors[0].shape:
            raise ValueError(f"loudness: every stem is (channels, n), got {[tuple(x.shape) for x in tensors]}")
    if not tensors:
        raise ValueError("loudness: at least one source")
    channels, n = tensors[0].shape
    _check_loudness_format(samplerate, channels)
    gains = mix_gains(mix, names)
    mixed = any(g[0] != 0 for _, g in gains)
    if mixed and origin is None:
        raise ValueError("loudness: an output has a gain on 'mix'; pass the mix as origin")
    if mixed and tuple(origin.shape) != (channels, n):
        raise ValueError(f"loudness: the mix is {tuple(origin.shape)}, the stems are {(channels, n)}")
    dev = _engine_device(*tensors)
    stream = LoudnessStream(names, channels, samplerate, mix, device=dev)
    with torch.cuda.device(dev):
        block = _stems_block(tensors, dev)
        org = _stage(origin, dev, "loudness") if mixed else None
        for a in range(0, n, LOUD_CHUNK):
            b = min(n, a + LOUD_CHUNK)
            stream.push(block[:, :, a:b], None if org is None else org[:, a:b])
    return stream.finish()


# ---- true peak of remixes: ITU-R BS.1770-4 Annex 2 (mi_true_peak_update, demucs_amd/csrc/true_peak.hip) ---------------------------
TP_COLS = 20                       # include/demucs_amd.h: MI_TP_* (MI_MIX_*'s columns up to the gains, then its own)
TP_MAX_PHASES = 8                  # MI_TP_MAX_PHASES
TP_MAX_TAPS = 32                   # MI_TP_MAX_TAPS
# Annex 2's order-48, 4-phase FIR interpolator: phases 0 and 1; phase 2 is phase 1 reversed and phase 3 phase 0 reversed.  Every
# coefficient is a multiple of 2^-13, hence exact in float32
_TP_PHASE0 = (0.0017089843750, 0.0109863281250, -0.0196533203125, 0.0332031250000, -0.0594482421875, 0.1373291015625,
              0.9721679687500, -0.1022949218750, 0.0476074218750, -0.0266113281250, 0.0148925781250, -0.0083007812500)
_TP_PHASE1 = (-0.0291748046875, 0.0292968750000, -0.0517578125000, 0.0891113281250, -0.1665039062500, 0.4650878906250,
              0.7797851562500, -0.2003173828125, 0.1015625000000, -0.0582275390625, 0.0330810546875, -0.0189208984375)


def _check_true_peak_format(samplerate, channels) -> None:
    if isinstance(samplerate, bool) or int(samplerate) != samplerate or samplerate <= 0:
        raise ValueError(f"true peak: the sample rate must be a positive integer, got {samplerate!r}")
    if samplerate >= 96000:
        raise ValueError(f"true peak: Annex 2's 4-times oversampling is for sample rates below 96 kHz, got {samplerate}; the 2-times "
                         "bank of higher rates is not implemented")
    if isinstance(channels, bool) or int(channels) != channels or channels < 1:
        raise ValueError(f"true peak: at least one channel, got {channels!r}")


def true_peak_bank(samplerate):
    """The polyphase bank of BS.1770-4 Annex 2's 4-times oversampling filter as a float32 array (4 phases, 12 taps), for sample
    rates below 96 kHz; other rates are refused.  Output `4 n + p` of the oversampled signal is `sum_k bank[p][k] * x[n - k]`."""
    import numpy as np
    _check_true_peak_format(samplerate, 1)
    return np.array([_TP_PHASE0, _TP_PHASE1, _TP_PHASE1[::-1], _TP_PHASE0[::-1]], dtype=np.float32)


def _peak_value(bits: int):
    import numpy as np
    return float(np.uint32(bits).view(np.float32))


class TrackTruePeaks:
    """What a true-peak pass over a track found (`audio.true_peak`, `TruePeakStream`, `Separator.levels_blocks`): per output the
    bit patterns of two float32 maxima, `bits` of the 4-times oversampled signal of BS.1770-4 Annex 2 and `sample_bits` of the
    samples themselves (a NaN sample gives a NaN pattern).  The oversampled estimate can lie below the sample peak, so a limit
    uses the larger of the two.

    `names`, `sources`, `samplerate`, `channels`, `length` and `mix` are `TrackLoudness`'s.  Immutable."""
    __slots__ = ("names", "sources", "samplerate", "channels", "length", "bits", "sample_bits", "mix")

    def __init__(self, names, sources, samplerate, channels, length, bits, sample_bits, mix):
        import numpy as np
        for what, v in (("names", names), ("sources", sources)):
            if isinstance(v, (str, bytes)) or not all(isinstance(n, str) for n in v) or len(set(v)) != len(tuple(v)) or not len(v):
                raise ValueError(f"TrackTruePeaks: {what} must be a sequence of names, each once, got {v!r}")
        names, sources = tuple(names), tuple(sources)
        _check_true_peak_format(samplerate, channels)
        if isinstance(length, bool) or not isinstance(length, (int, np.integer)) or length < 0:
            raise ValueError(f"TrackTruePeaks: length must be a non-negative integer, got {length!r}")
        try:
            mix = tuple((str(name), tuple(float(np.float32(g)) for g in gains)) for name, gains in mix)
        except (TypeError, ValueError):
            raise ValueError(f"TrackTruePeaks: mix must be ((output name, (g_mix, g_0, ...)), ...) as audio.mix_gains returns it, got "
                             f"{mix!r}") from None
        if tuple(name for name, _ in mix) != names or \
                not all(len(g) == 1 + len(sources) and all(np.isfinite(v) for v in g) for _, g in mix):
            raise ValueError(f"TrackTruePeaks: mix must name the outputs {list(names)} in order, each with finite gains for the mix "
                             f"and the {len(sources)} sources, got {mix!r}")
        both = []
        for what, seq in (("bits", bits), ("sample_bits", sample_bits)):
            if isinstance(seq, (str, bytes)) or not hasattr(seq, "__len__") or len(seq) != len(names):
                raise ValueError(f"TrackTruePeaks: {what} must hold one uint32 bit pattern for each of the {len(names)} outputs, got "
                                 f"{seq!r}")
            vals = []
            for v in seq:
                if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 0 <= int(v) <= 0x7FFFFFFF:
                    raise ValueError(f"TrackTruePeaks: a peak is the uint32 bit pattern of a float32 max |value|, whose sign bit is "
                                     f"clear, got {v!r}")
                vals.append(int(v))
            both.append(tuple(vals))
        for name, v in zip(self.__slots__, (names, sources, int(samplerate), int(channels), int(length), both[0], both[1], mix)):
            object.__setattr__(self, name, v)

    def __setattr__(self, name, value):
        raise AttributeError("TrackTruePeaks is immutable")

    def __delattr__(self, name):
        raise AttributeError("TrackTruePeaks is immutable")

    def _at(self, name: str) -> int:
        if name not in self.names:
            raise KeyError(f"output {name!r} is not among the measured outputs {list(self.names)}")
        return self.names.index(name)

    def true_peak(self, name: str) -> float:
        """The largest magnitude of output `name`'s 4-times oversampled signal (linear; Annex 2's estimate of the true peak)."""
        return _peak_value(self.bits[self._at(name)])

    def sample_peak(self, name: str) -> float:
        """The largest magnitude among output `name`'s samples (linear)."""
        return _peak_value(self.sample_bits[self._at(name)])

    def dbtp(self, name: str) -> float:
        """`true_peak(name)` in dBTP: -inf for silence, NaN for a NaN sample."""
        v = self.true_peak(name)
        if v != v:
            return float("nan")
        return 20.0 * math.log10(v) if v > 0 else float("-inf")

    def gain_limit(self, name: str, ceiling: float = -1.0) -> float:
        """The largest linear scale that keeps `max(true_peak, sample_peak)` of output `name` at or below `ceiling` dBTP; inf for
        silence.  A NaN peak has no such scale and raises."""
        over, sample = self.true_peak(name), self.sample_peak(name)
        if over != over or sample != sample or not math.isfinite(float(ceiling)):
            raise ValueError(f"TrackTruePeaks: output {name!r} has the peaks {over} / {sample}; no gain keeps that below "
                             f"{ceiling} dBTP")
        peak = max(over, sample)
        return 10.0 ** (float(ceiling) / 20.0) / peak if peak > 0 else float("inf")

    def _key(self):
        return tuple(getattr(self, k) for k in self.__slots__)

    def __eq__(self, other):
        return isinstance(other, TrackTruePeaks) and self._key() == other._key()

    def __hash__(self):
        return hash(self._key())

    def __repr__(self):
        return (f"TrackTruePeaks(names={list(self.names)}, sources={list(self.sources)}, samplerate={self.samplerate}, "
                f"channels={self.channels}, length={self.length}, dbtp={[self.dbtp(n) for n in self.names]})")


def true_peak_rows(gains, src: int, src_pitch: int, n: int, origin: int, pitch: int, affine, before: int, tail: int, hist_len: int,
                   side: int, hist_start: int, hist_next: int, channels: int) -> list:
    """mi_true_peak_update's rows (MI_TP_*) for resolved remixes of `n` frames from track position `before`.  Output i keeps its
    history at `(side, i)` of a (2, outputs, channels, hist_len) buffer and its two maxima in slot i."""
    import numpy as np
    aff = 0 if affine is None else int(np.array(affine, dtype=np.float32).view(np.int64)[0])
    per = channels * hist_len
    rows = []
    for i, (_, g) in enumerate(gains):
        packed = np.zeros(2 * (MIX_CLIP_AT - MIX_GAINS_AT), dtype=np.float32)
        packed[:len(g)] = g
        rows += [src, n, origin, pitch, aff, int(affine is not None), *packed.view(np.int64).tolist(), src_pitch, before, tail,
                 hist_len, (side * len(gains) + i) * per, ((1 - side) * len(gains) + i) * per, hist_start, hist_next, i]
    return rows


def _true_peak_call(table, rows: int, max_n: int, n_sources: int, channels: int, bank, hist, peaks) -> None:
    _lib.check(_lib.load().mi_true_peak_update(
        table.data_ptr(), rows, max_n, n_sources, channels, bank.data_ptr(), bank.shape[0], bank.shape[1],
        0 if hist is None else hist.data_ptr(), 0 if hist is None else hist.numel(), peaks.data_ptr(), peaks.numel() // 2,
        C.c_void_p(_lib.current_stream_ptr())), "mi_true_peak_update")


class TruePeakStream:
    """BS.1770-4 Annex 2 true peak (and sample peak) of gain-weighted remixes of a track that arrives block by block, measured
    where the stems lie.  The interface is `LoudnessStream`'s: `push(stems_block, origin=None, affine=None)` takes the next
    `n >= 0` samples as a device float32 (sources, channels, n) and the mix of the same positions, `finish()` returns the
    `TrackTruePeaks`.  The measured values are `deliver_mix(..., clip=None, fmt="f32")`'s, and the peaks have the same bits for
    every partition of the track into pushes.

    Every push is ONE `mi_true_peak_update` call for all outputs, reading a span of a larger tensor in place; `finish()` issues
    the one call for the positions past the end and copies 8 bytes per output.  Device state: two sides of (outputs, channels,
    taps - 1) carried values, and the slots."""

    def __init__(self, sources, channels: int, samplerate: int, mix=None, device="cuda"):
        self.sources = list(sources)
        _check_true_peak_format(samplerate, channels)
        if not self.sources:
            raise ValueError("true peak: at least one source")
        if mix is None:
            mix = {name: {name: 1.0} for name in self.sources}
        self.gains = mix_gains(mix, self.sources)
        self.channels, self.samplerate = int(channels), int(samplerate)
        self.bank = true_peak_bank(self.samplerate)
        self.mixed = any(g[0] != 0 for _, g in self.gains)
        dev = torch.device(device)
        if dev.type != "cuda":
            raise _lib.EngineError("demucs_amd.audio.TruePeakStream only runs on a GPU device (MI355X)")
        self.device = dev
        self.pushed = 0
        self.finished = False
        self._hist = self._peaks = self._bank = None
        self._side = self._h0 = 0

    @property
    def device_bytes(self) -> int:
        return sum(t.numel() * t.element_size() for t in (self._hist, self._peaks, self._bank) if t is not None)

    _rows_of = LoudnessStream._rows_of

    def _state(self):
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        if self._peaks is None:
            with torch.cuda.device(self.device):
                self._hist = torch.zeros(2, len(self.gains), self.channels, self.bank.shape[1] - 1, device=self.device)
                self._peaks = torch.zeros(2 * len(self.gains), dtype=torch.int32, device=self.device)
                self._bank = torch.from_numpy(self.bank).to(self.device)

    def push(self, stems_block: torch.Tensor, origin=None, affine=None) -> None:
        if self.finished:
            raise RuntimeError("push after finish()")
        S, ch, R = len(self.sources), self.channels, len(self.gains)
        if not isinstance(stems_block, torch.Tensor) or stems_block.dim() != 3 or tuple(stems_block.shape[:2]) != (S, ch) or \
                not stems_block.dtype.is_floating_point:
            raise ValueError(f"true peak: expected a floating ({S}, {ch}, n) block of stems, got "
                             f"{tuple(getattr(stems_block, 'shape', ()))}")
        n = stems_block.shape[2]
        if self.mixed:
            if origin is None:
                raise ValueError("true peak: an output has a gain on 'mix'; push the mix of the same positions as origin=")
            if not isinstance(origin, torch.Tensor) or tuple(origin.shape) != (ch, n) or not origin.dtype.is_floating_point:
                raise ValueError(f"true peak: the mix is {tuple(getattr(origin, 'shape', ()))}, the stems are {(ch, n)}")
        if n == 0:
            return
        self._state()
        keep = self.bank.shape[1] - 1
        with torch.cuda.device(self.device):
            block, src_pitch = self._rows_of(stems_block)
            org, pitch = self._rows_of(origin) if self.mixed else (None, 0)
            end = self.pushed + n
            nxt = max(0, end - keep)
            rows = true_peak_rows(self.gains, block.data_ptr(), src_pitch, n, 0 if org is None else org.data_ptr(), pitch, affine,
                                  self.pushed, 0, keep, self._side, self._h0, nxt, ch)
            table = torch.tensor(rows, dtype=torch.int64).to(self.device)
            _true_peak_call(table, R, n, S, ch, self._bank, self._hist, self._peaks)
        self._side, self._h0, self.pushed = 1 - self._side, nxt, end

    def finish(self) -> TrackTruePeaks:
        if self.finished:
            raise RuntimeError("finish() called twice")
        self.finished = True
        R = len(self.gains)
        bits = [0] * (2 * R)
        if self.pushed:
            keep = self.bank.shape[1] - 1
            with torch.cuda.device(self.device):
                # the positions past the end: no new sample, the history alone
                rows = true_peak_rows(self.gains, 0, 0, 0, 0, 0, None, self.pushed, keep, keep, self._side, self._h0, -1, self.channels)
                table = torch.tensor(rows, dtype=torch.int64).to(self.device)
                _true_peak_call(table, R, keep, len(self.sources), self.channels, self._bank, self._hist, self._peaks)
                bits = [v & 0xFFFFFFFF for v in self._peaks.cpu().tolist()]
        return TrackTruePeaks([name for name, _ in self.gains], self.sources, self.samplerate, self.channels, self.pushed, bits[0::2],
                              bits[1::2], mix_identity(self.gains))


def true_peak(origin, stems: dict, mix=None, samplerate: int = 44100) -> TrackTruePeaks:
    """BS.1770-4 Annex 2 true peaks of gain-weighted remixes of one separated track, measured on the stems' device in ONE
    `mi_true_peak_update` call: the `TrackTruePeaks` of the frames `deliver_mix(origin, stems, mix, clip=None, fmt="f32")`
    returns, none of which is produced.  The arguments and their defaults are `audio.loudness`'s."""
    names = list(stems)
    if mix is None:
        mix = {name: {name: 1.0} for name in names}
        if origin is not None:
            mix["mix"] = {"mix": 1.0}
    tensors = [stems[k] for k in names]
    for t in tensors:
        if not t.dtype.is_floating_point:
            raise TypeError(f"true peak: a floating-point tensor is expected, got {t.dtype}")
        if t.dim() != 2 or t.shape != tensors[0].shape:
            raise ValueError(f"true peak: every stem is (channels, n), got {[tuple(x.shape) for x in tensors]}")
    if not tensors:
        raise ValueError("true peak: at least one source")
    channels, n = tensors[0].shape
    _check_true_peak_format(samplerate, channels)
    gains = mix_gains(mix, names)
    mixed = any(g[0] != 0 for _, g in gains)
    if mixed and origin is None:
        raise ValueError("true peak: an output has a gain on 'mix'; pass the mix as origin")
    if mixed and tuple(origin.shape) != (channels, n):
        raise ValueError(f"true peak: the mix is {tuple(origin.shape)}, the stems are {(channels, n)}")
    dev = _engine_device(*tensors)
    R = len(gains)
    bits = [0] * (2 * R)
    if n:
        bank = true_peak_bank(samplerate)
        with torch.cuda.device(dev):
            block = _stems_block(tensors, dev)
            org = _stage(origin, dev, "true peak").contiguous() if mixed else None
            tail = bank.shape[1] - 1
            rows = true_peak_rows(gains, block.data_ptr(), n, n, 0 if org is None else org.data_ptr(), n if mixed else 0, None, 0, tail,
                                  0, 0, 0, -1, channels)
            table = torch.tensor(rows, dtype=torch.int64).to(dev)
            peaks = torch.zeros(2 * R, dtype=torch.int32, device=dev)
            _true_peak_call(table, R, n + tail, len(names), channels, torch.from_numpy(bank).to(dev), None, peaks)
            bits = [v & 0xFFFFFFFF for v in peaks.cpu().tolist()]
    return TrackTruePeaks([name for name, _ in gains], names, samplerate, channels, n, bits[0::2], bits[1::2], mix_identity(gains))
