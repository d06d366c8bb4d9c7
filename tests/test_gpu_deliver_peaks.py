"""`clip="rescale"` on a stream, the kernels alone (demucs_amd/csrc/deliver.hip, deliver_resample.hip): `mi_deliver_peaks_update`,
`mi_deliver_resample_peaks` and `mi_deliver_resample_pcm_peaks` against the CPU definition in float32 -- `peak = value.abs().max()`,
frames `i16_pcm(value / max(1.01 * peak, 1))` or the float, `value` the two-stems value of tests/test_gpu_deliver_rate.py and at
another rate `audio.resample_frac` of it.  Every comparison is on the bits.  Guard words surround every buffer a kernel writes."""
import ctypes as C

import numpy as np
import pytest
import torch

from demucs_amd import _lib, audio
from test_gpu_deliver_rate import ADD, GUARD, SR, STEM, i16_pcm, kernel_length, same, stream_ptr, value_of

pytestmark = pytest.mark.gpu
RESCALE = 1
SENTINEL = 0x11111111                    # guard slots of a peaks buffer
NAN_BITS = 0x7FC00000


def bits_of(v: torch.Tensor) -> int:
    """The uint32 bit pattern of a float32 scalar tensor."""
    return int(v.reshape(1).to(torch.float32).view(torch.int32)) & 0xFFFFFFFF


def cpu_peak_bits(value: torch.Tensor) -> int:
    return bits_of(value.abs().max())


def same_peak(got: int, want: int) -> bool:
    """Equal bits; a NaN peak is any NaN pattern (it orders above +inf)."""
    return got == want or (got > 0x7F800000 and want > 0x7F800000)


def peaks_buffer(n_peaks, values=None):
    """n_peaks slots between two guards of GUARD sentinel words; returns (buffer, address of slot 0)."""
    buf = torch.full((GUARD + n_peaks + GUARD,), SENTINEL, dtype=torch.int32, device="cuda")
    buf[GUARD:GUARD + n_peaks] = 0 if values is None else torch.tensor(values, dtype=torch.int64).to(torch.int32).cuda()
    return buf, buf.data_ptr() + 4 * GUARD


def read_peaks(buf, n_peaks):
    host = buf.cpu()
    assert bool((host[:GUARD] == SENTINEL).all()) and bool((host[GUARD + n_peaks:] == SENTINEL).all())
    return [int(v) & 0xFFFFFFFF for v in host[GUARD:GUARD + n_peaks]]


def whole_track_peak_bits(value: torch.Tensor) -> int:
    """`mi_deliver_peaks` (the whole-track entry, memset included) on value (C, n)."""
    v = value.contiguous().cuda()
    C_, n = v.shape
    table = torch.tensor([v.data_ptr(), 0, n, STEM, 0, RESCALE, 0, 0, 0], dtype=torch.int64).cuda()
    peak = torch.full((1,), 0x55, dtype=torch.int32, device="cuda")
    _lib.check(_lib.load().mi_deliver_peaks(table.data_ptr(), 1, n, 1, C_, peak.data_ptr(), 1, 1 << 40, stream_ptr()), "mi_deliver_peaks")
    return int(peak.cpu()) & 0xFFFFFFFF


# ---- 1. mi_deliver_peaks_update ---------------------------------------------------------------------------------------------------
S1, C1, N1 = 3, 2, 2 * 1024 + 7
PARTITIONS_1 = [[N1], [1, N1 - 1], [1023, 1025, 7], [1023, 0, 1025, 0, 7]]
# (kind, sel, slot): slot 1 is a guard between two rows' slots
ROWS_1 = [(STEM, 1, 0), (ADD, 1, 2), (ADD, 0, 3)]


def update(x, partition, rows=ROWS_1, n_peaks=4, start=None):
    """Feed x (S, C, n) through mi_deliver_peaks_update block by block; FMT and DST_OFF hold values mi_deliver_pcm would refuse."""
    lib = _lib.load()
    S, C_, n = x.shape
    buf, peaks = peaks_buffer(n_peaks, start if start is not None else [0, SENTINEL, 0, 0][:n_peaks])
    pos = 0
    assert sum(partition) == n
    for b in partition:
        src = x[:, :, pos:pos + b].contiguous().cuda()
        table = torch.tensor([v for kind, sel, slot in rows for v in (src.data_ptr() if b else 0, 0, b, kind, sel, RESCALE, slot, 99, -3)],
                             dtype=torch.int64).cuda()
        _lib.check(lib.mi_deliver_peaks_update(table.data_ptr(), len(rows), max(b, 1), S, C_, C.c_void_p(peaks), n_peaks, stream_ptr()),
                   "mi_deliver_peaks_update")
        torch.cuda.synchronize()
        pos += b
    return read_peaks(buf, n_peaks)


def quiet(seed):
    return torch.rand(S1, C1, N1, generator=torch.Generator().manual_seed(seed)) * 0.5 - 0.25


def planted_cases():
    cases = {}
    x = quiet(1); x[1, 0, 0] = -3.0; cases["sample 0"] = x
    x = quiet(2); x[1, 1, N1 - 1] = 3.0; cases["the last sample"] = x
    x = quiet(3); x[1, 0, 1022] = 3.0; cases["the last sample of a block that is not the last"] = x
    x = quiet(4); x[:, 0, :] = 0.0; x[1, 1, 1500] = -2.5; cases["channel 1 only"] = x
    x = quiet(5); x[1, 0, 5] = 7.0; cases["a stem the sum leaves out"] = x
    cases["all zero"] = torch.zeros(S1, C1, N1)
    x = quiet(6); x[1, 0, 100] = float("nan"); cases["one NaN"] = x
    return cases


def test_update_equals_the_whole_track_peak_for_every_partition():
    for tag, x in planted_cases().items():
        want = [cpu_peak_bits(value_of(x, kind, sel)) for kind, sel, _ in ROWS_1]
        whole = [whole_track_peak_bits(value_of(x, kind, sel)) for kind, sel, _ in ROWS_1]
        for a, b in zip(want, whole):
            assert same_peak(b, a), tag
        for partition in PARTITIONS_1:
            got = update(x, partition)
            assert got[1] == SENTINEL, (tag, partition)                       # the slot between two rows' slots
            for (kind, sel, slot), w, wh in zip(ROWS_1, want, whole):
                assert same_peak(got[slot], w) and same_peak(got[slot], wh), (tag, partition, kind, sel, hex(got[slot]), hex(w))
        if tag == "a stem the sum leaves out":
            seven = bits_of(torch.tensor(7.0))
            assert want[0] == seven and want[1] != seven and want[1] < bits_of(torch.tensor(1.0)) and want[2] > bits_of(torch.tensor(6.0))
        if tag == "all zero":
            assert want == [0, 0, 0]
        if tag == "one NaN":
            assert want[0] > 0x7F800000 and want[2] > 0x7F800000 and want[1] < 0x7F800000   # the row that leaves stem 1 out is clean
        if tag == "channel 1 only":
            assert want[0] == bits_of(torch.tensor(2.5))


def test_update_carries_the_running_maximum_and_skips_bad_rows():
    x = quiet(7)
    big = bits_of(torch.tensor(5.0))
    # a slot that already holds more keeps it; the memset of mi_deliver_peaks is not there
    got = update(x, [N1], start=[big, SENTINEL, 0, big])
    assert got[0] == big and got[3] == big and got[2] == cpu_peak_bits(value_of(x, ADD, 1))
    # rows with a slot outside [0, n_peaks), another clip mode, a bad kind or selection: nothing is written
    lib = _lib.load()
    src = x.contiguous().cuda()
    buf, peaks = peaks_buffer(2)
    bad = [[src.data_ptr(), 0, N1, STEM, 1, RESCALE, -1, 0, 0], [src.data_ptr(), 0, N1, STEM, 1, RESCALE, 2, 0, 0],
           [src.data_ptr(), 0, N1, STEM, 1, 2, 0, 0, 0], [src.data_ptr(), 0, N1, STEM, 1, 0, 0, 0, 0],
           [src.data_ptr(), 0, N1, 3, 1, RESCALE, 0, 0, 0], [src.data_ptr(), 0, N1, STEM, S1, RESCALE, 0, 0, 0],
           [src.data_ptr(), 0, N1, 2, 1, RESCALE, 0, 0, 0],                   # "minus" without an origin
           [0, 0, N1, STEM, 1, RESCALE, 0, 0, 0], [src.data_ptr(), 0, -5, STEM, 1, RESCALE, 0, 0, 0]]
    table = torch.tensor([v for r in bad for v in r], dtype=torch.int64).cuda()
    _lib.check(lib.mi_deliver_peaks_update(table.data_ptr(), len(bad), N1, S1, C1, C.c_void_p(peaks), 2, stream_ptr()),
               "mi_deliver_peaks_update")
    torch.cuda.synchronize()
    assert read_peaks(buf, 2) == [0, 0]


# ---- 2. and 3. the resampling entries -------------------------------------------------------------------------------------------------
def run_rate(mode, x, plan, specs, blocks, final_with_block, slots=None, peaks=None, snapshots=False):
    """Feed x (S, C, L) block by block as a stream's emitted stems through one of the three entries ("pcm": the shipped
    mi_deliver_resample_pcm, "pcm_peaks", "measure"); every spec (kind, sel, clip, fmt) is one row of each launch with its own
    history and, for the delivering entries, its own destination region for the whole track (a call writes its frames behind the
    last call's).  All blocks and all tables go to the device once.  Returns (frames per spec or None, history regions per spec at
    the end, [history after every launch] if snapshots, [peaks after every launch] if snapshots and measuring)."""
    lib = _lib.load()
    S, C_, L = x.shape
    dev = torch.device("cuda", torch.cuda.current_device())
    arena = audio._BankArena.get(dev)
    bank_off = arena.offset(plan)
    bank = arena.buf
    side = C_ * plan.carry
    hist = torch.full((GUARD + len(specs) * 2 * side + GUARD,), 7.5, device="cuda")
    calls = [(b, False) for b in blocks]
    if final_with_block:
        calls[-1] = (calls[-1][0], True)
    else:
        calls.append((0, True))
    assert sum(b for b, _ in calls) == L
    total_out = plan.final_count(L)
    # destinations: per spec the whole track's frames, 16-byte aligned (every third at 4 mod 16), guards between them
    regions, at = [], GUARD
    for i, (_, _, _, fmt) in enumerate(specs):
        at = -(-at // 16) * 16 + (4 if i % 3 == 1 else 0)
        regions.append(at)
        at += total_out * C_ * (4 if fmt else 2) + GUARD
    dst = torch.full((at,), 0xA5, dtype=torch.uint8, device="cuda")
    # every block, as the (S, C, n_in) tensor a stream emits, one behind the other
    flat, pos = [], 0
    for n_in, _ in calls:
        flat.append(x[:, :, pos:pos + n_in].reshape(-1))
        pos += n_in
    sizes = np.cumsum([0] + [t.numel() for t in flat])
    src_all = torch.cat(flat).cuda()
    # the rows of a launch from a template: the columns that change per call are filled in for all specs at once.  A measuring
    # row holds an FMT and a DST_OFF the delivering entries would refuse: they are not read
    n_specs = len(specs)
    tmpl = np.zeros((n_specs, audio.RATE_COLS), dtype=np.int64)
    tmpl[:, 3:7] = [(kind, sel, clip, 77 if mode == "measure" else fmt) for kind, sel, clip, fmt in specs]
    tmpl[:, 7:11] = (plan.old, plan.new, plan.width, bank_off)
    tmpl[:, 14] = plan.carry
    bases = GUARD + np.arange(n_specs, dtype=np.int64) * 2 * side
    frame = np.array([C_ * (4 if fmt else 2) for _, _, _, fmt in specs], dtype=np.int64)
    region0 = np.array(regions, dtype=np.int64)
    tables, launches, sd, h0, pos = [], [], 0, 0, 0
    for k, (n_in, final) in enumerate(calls):
        out0, n_out, nxt = plan.step(pos, n_in, final)
        if n_in or n_out:
            launches.append((len(tables) * n_specs * audio.RATE_COLS, audio.rate_groups(plan, C_, n_out)))
            r = tmpl.copy()
            r[:, 0:3] = (src_all.data_ptr() + 4 * int(sizes[k]) if n_in else 0, n_in, pos)
            r[:, 11:14] = (out0, n_out, pos + n_in if final else -1)
            r[:, 15], r[:, 16] = bases + sd * side, bases + (1 - sd) * side
            r[:, 17:19] = (h0, nxt)
            r[:, 19] = -2 if mode == "measure" else region0 + out0 * frame
            tables.append(r)
            if not final:
                sd, h0 = 1 - sd, nxt
        pos += n_in
    table = torch.from_numpy(np.concatenate(tables).reshape(-1)).cuda()
    n_peaks = 0 if peaks is None else peaks[0].numel() - 2 * GUARD
    slots_dev = torch.tensor(slots if slots is not None else [0] * len(specs), dtype=torch.int32).cuda()
    lds = audio.rate_lds_floats(plan, C_)
    hist_snaps, peak_snaps = [], []
    for at_row, groups in launches:
        common = (C.c_void_p(table.data_ptr() + 8 * at_row), len(specs), groups, S, C_, bank.data_ptr(), bank.numel(), hist.data_ptr(),
                  hist.numel(), lds)
        if mode == "pcm":
            _lib.check(lib.mi_deliver_resample_pcm(*common, dst.data_ptr(), dst.numel(), stream_ptr()), "mi_deliver_resample_pcm")
        elif mode == "pcm_peaks":
            _lib.check(lib.mi_deliver_resample_pcm_peaks(*common, dst.data_ptr(), dst.numel(), slots_dev.data_ptr(), C.c_void_p(peaks[1]),
                                                         n_peaks, stream_ptr()), "mi_deliver_resample_pcm_peaks")
        else:
            _lib.check(lib.mi_deliver_resample_peaks(*common, slots_dev.data_ptr(), C.c_void_p(peaks[1]), n_peaks, stream_ptr()),
                       "mi_deliver_resample_peaks")
        if snapshots:
            hist_snaps.append(hist.clone())
            if mode == "measure":
                peak_snaps.append(peaks[0].clone())
    torch.cuda.synchronize()
    h = hist.cpu()
    assert bool((h[:GUARD] == 7.5).all()) and bool((h[-GUARD:] == 7.5).all())
    host = dst.cpu()
    frames = None
    if mode == "measure":
        assert bool((host == 0xA5).all())                                      # a measuring launch has no destination
    else:
        used = torch.zeros(host.numel(), dtype=torch.bool)
        frames = []
        for i, (_, _, _, fmt) in enumerate(specs):
            size = total_out * C_ * (4 if fmt else 2)
            used[regions[i]:regions[i] + size] = True
            frames.append(host[regions[i]:regions[i] + size].clone().view(torch.float32 if fmt else torch.int16).view(total_out, C_))
        frames = (frames, host, used)
    regions_h = [h[GUARD + i * 2 * side:GUARD + (i + 1) * 2 * side] for i in range(len(specs))]
    return frames, regions_h, hist_snaps, peak_snaps


def partitions_for(plan, L):
    """(tag, blocks, final call carries a block): one block; blocks of 1 sample; blocks of old - 1 samples; a final call without
    input."""
    ones = [1] * L
    short = [plan.old - 1] * (L // (plan.old - 1))
    short += [L - sum(short)] if L - sum(short) else []
    return [("one block", [L], True), ("blocks of 1 sample", ones, True), ("blocks of old - 1", short, True),
            ("blocks of old - 1, then a final call with no input", short, False), ("one block, then the tail", [L], False)]


RATES = [(48000, (147, 160), 2), (16000, (441, 160), 2), (48000, (147, 160), 1)]      # the last: the route of channels != 2


def planted_rate_signals(S, C_, L, plan):
    g = torch.Generator().manual_seed(L)
    out = {"noise": torch.rand(S, C_, L, generator=g) * 3 - 1.5}
    x = torch.rand(S, C_, L, generator=g) * 0.2 - 0.1
    x[1, C_ - 1, L - 1] = 5.0                                                  # the peak frame is one of the final call's
    out["a spike in the last input sample"] = x
    x = torch.rand(S, C_, L, generator=g) * 0.2 - 0.1
    x[1, 0, L // 2 - 1] = -5.0                                                 # with [L // 2, rest]: the taps straddle two calls
    out["a spike at the end of a block"] = x
    ramp = (torch.arange(1, L + 1, dtype=torch.float32) / L)
    x = ramp[None, None, :] * (1.0 + 0.1 * torch.arange(S)[:, None, None] + 0.01 * torch.arange(C_)[None, :, None])
    out["growing toward the end"] = x * (1 - 2 * (torch.arange(S)[:, None, None] % 2))     # odd stems negative
    return out


@pytest.mark.parametrize("rate,pair,C_", RATES)
def test_resample_peaks_equal_the_whole_track_peak_for_every_partition(rate, pair, C_):
    S = 4
    plan = audio.delivery_rate_plan(SR, rate, C_)
    assert (plan.old, plan.new) == pair
    L = kernel_length(plan, C_)
    specs = [(STEM, 1, RESCALE, 0), (ADD, 1, RESCALE, 0), (ADD, 0, RESCALE, 0), (STEM, 1, RESCALE, 0), (STEM, 1, RESCALE, 0)]
    slots = [0, 2, 3, -1, 4]                                                   # slot 1 stays a guard; -1 and 4 = n_peaks are refused
    for tag, x in planted_rate_signals(S, C_, L, plan).items():
        values = [audio.resample_frac(value_of(x, kind, sel), SR, rate) for kind, sel, _, _ in specs[:3]]
        want = [cpu_peak_bits(v) for v in values]
        whole = [whole_track_peak_bits(v) for v in values]
        assert want == whole, tag
        parts = partitions_for(plan, L)
        if tag == "a spike at the end of a block":
            parts = [("two halves", [L // 2, L - L // 2], True), ("two halves and a tail", [L // 2, L - L // 2], False)] + parts[:1]
        elif tag != "noise" or C_ != 2:
            parts = [p for p in parts if p[0] != "blocks of 1 sample"]           # the 1-sample partition runs on the stereo noise
        for ptag, blocks, with_block in parts:
            peaks = peaks_buffer(4, [0, SENTINEL, 0, 0])
            _, regions, _, _ = run_rate("measure", x, plan, specs, blocks, with_block, slots=slots, peaks=peaks)
            got = read_peaks(peaks[0], 4)
            assert got[1] == SENTINEL
            assert [got[0], got[2], got[3]] == want, (tag, ptag, [hex(v) for v in got], [hex(v) for v in want])
            # the rows with a slot outside [0, n_peaks) were skipped whole: their history keeps its fill
            assert bool((regions[3] == 7.5).all()) and bool((regions[4] == 7.5).all()), (tag, ptag)


def test_resample_peaks_carry_the_history_as_the_delivering_kernel_does():
    """After every launch both history sides equal what mi_deliver_resample_pcm leaves for the same calls with clip = 0, and the
    running peak is the peak of the frames delivered so far: on a signal that grows toward the end of every block a frame computed
    early, or a lane past n_out, would raise it."""
    S, C_, rate = 4, 2, 48000
    plan = audio.delivery_rate_plan(SR, rate, C_)
    L = kernel_length(plan, C_)
    x = planted_rate_signals(S, C_, L, plan)["growing toward the end"]
    kinds = [(STEM, 1), (ADD, 1), (ADD, 0)]
    blocks = partitions_for(plan, L)[3][1]
    peaks = peaks_buffer(3)
    _, _, hist_m, peak_m = run_rate("measure", x, plan, [(k, s, RESCALE, 0) for k, s in kinds], blocks, False, slots=[0, 1, 2],
                                    peaks=peaks, snapshots=True)
    _, _, hist_p, _ = run_rate("pcm", x, plan, [(k, s, 0, 1) for k, s in kinds], blocks, False, snapshots=True)
    assert len(hist_m) == len(hist_p) > 50
    assert torch.equal(torch.stack(hist_m), torch.stack(hist_p))
    values = [audio.resample_frac(value_of(x, k, s), SR, rate) for k, s in kinds]
    running = torch.stack([v.abs().max(0).values.cummax(0).values for v in values])          # (3, frames)
    got = torch.stack(peak_m).cpu()[:, GUARD:GUARD + 3]
    pos, k = 0, 0
    for n_in, final in [(b, False) for b in blocks] + [(0, True)]:
        out0, n_out, _ = plan.step(pos, n_in, final)
        pos += n_in
        if not (n_in or n_out):
            continue
        done = out0 + n_out
        want = [bits_of(running[i, done - 1]) if done else 0 for i in range(3)]
        assert [int(v) & 0xFFFFFFFF for v in got[k]] == want, (k, pos)
        k += 1
    assert k == len(peak_m) and done == plan.final_count(L)
    assert float(running[0, -1]) > float(running[0, running.shape[1] // 2]) > 0            # it did grow


def boundary_peaks():
    """Peaks p around 1 / 1.01, found by a search on the CPU: float32(1.01f * p) below 1, exactly 1, and the next float above 1."""
    m = np.float32(1.01)
    one, above = np.float32(1.0), np.nextafter(np.float32(1.0), np.float32(2.0))
    p = np.float32(1.0) / m
    for _ in range(64):
        p = np.nextafter(p, np.float32(0.0))
    found = {}
    for _ in range(160):
        d = np.float32(p * m)
        for name, target in (("one", one), ("above", above)):
            if d == target and name not in found:
                found[name] = p
        if d < one:
            found["below"] = p                                                  # the largest such p seen last
        p = np.nextafter(p, np.float32(2.0))
    assert set(found) == {"below", "one", "above"}
    assert np.float32(found["below"] * m) < one
    return found


def cpu_rescaled_frames(v, peak_bits, fmt):
    """`i16_pcm(v / max(1.01 * peak, 1))` or the float (audio.py:226, 178), v (C, n) on the CPU; the peak as a float32 tensor."""
    peak = torch.tensor([peak_bits], dtype=torch.int64).to(torch.int32).view(torch.float32)[0]
    w = v / max(1.01 * peak, 1)
    return (i16_pcm(w) if fmt == 0 else w).t().contiguous()


@pytest.mark.parametrize("rate,pair,C_", RATES)
def test_resample_pcm_peaks_divide_by_the_given_peak(rate, pair, C_):
    S = 4
    plan = audio.delivery_rate_plan(SR, rate, C_)
    L = kernel_length(plan, C_)
    x = torch.rand(S, C_, L, generator=torch.Generator().manual_seed(rate)) * 3 - 1.5
    found = boundary_peaks()
    peak_bits = [int(np.float32(found[k]).view(np.uint32)) for k in ("below", "one", "above")] + [NAN_BITS, bits_of(torch.tensor(1.7))]
    n_peaks = len(peak_bits)
    specs, slots = [], []
    for slot in range(n_peaks):
        for kind, sel in ((STEM, 1), (ADD, 2)):
            for fmt in (0, 1):
                specs.append((kind, sel, RESCALE, fmt))
                slots.append(slot)
    plain = [(STEM, 1, 0, 0), (ADD, 2, 2, 1), (STEM, 0, 3, 0), (ADD, 0, 0, 1), (STEM, 3, 2, 0), (ADD, 3, 3, 1)]
    refused = [(STEM, 1, RESCALE, 0), (ADD, 2, RESCALE, 1)]                     # slots n_peaks and -1
    all_specs = specs + plain + refused
    all_slots = slots + [-7] * len(plain) + [n_peaks, -1]                      # a row of another clip mode reads no slot
    values = {(kind, sel): audio.resample_frac(value_of(x, kind, sel), SR, rate) for kind, sel, _, _ in all_specs}
    want = [cpu_rescaled_frames(values[kind, sel], peak_bits[slot], fmt) for (kind, sel, _, fmt), slot in zip(specs, slots)]
    # the four cases do what they are named for
    v = values[STEM, 1]
    assert torch.equal(cpu_rescaled_frames(v, peak_bits[0], 1), v.t()) and torch.equal(cpu_rescaled_frames(v, peak_bits[1], 1), v.t())
    assert not torch.equal(cpu_rescaled_frames(v, peak_bits[2], 1), v.t())
    assert bool(torch.isnan(cpu_rescaled_frames(v, NAN_BITS, 1)).all()) and bool((cpu_rescaled_frames(v, NAN_BITS, 0) == 0).all())
    for ptag, blocks, with_block in partitions_for(plan, L):
        if ptag == "blocks of 1 sample" and (rate, C_) != (48000, 2):
            continue                                                            # once: the longest loop of the file
        peaks = peaks_buffer(n_peaks, peak_bits)
        (got, host, used), regions, _, _ = run_rate("pcm_peaks", x, plan, all_specs, blocks, with_block, slots=all_slots, peaks=peaks)
        assert read_peaks(peaks[0], n_peaks) == peak_bits                       # only read
        for i, w in enumerate(want):
            assert got[i].dtype == w.dtype and same(got[i], w), (ptag, all_specs[i], all_slots[i])
        (base, host_b, _), regions_b, _, _ = run_rate("pcm", x, plan, plain, blocks, with_block)
        for j in range(len(plain)):
            assert torch.equal(got[len(specs) + j], base[j]), (ptag, plain[j])
            assert torch.equal(regions[len(specs) + j], regions_b[j])
        # the refused rows wrote neither frames nor history; nothing lies outside the rows' frames
        for j in (len(all_specs) - 2, len(all_specs) - 1):
            raw = got[j].view(torch.uint8) if got[j].numel() else got[j]
            assert bool((raw == 0xA5).all()) and bool((regions[j] == 7.5).all()), (ptag, j)
        assert bool((host[~used] == 0xA5).all())
