"""Packed scheduler: many tracks of different lengths in shared batched forwards (`apply_model_many`).

The result contract is the sequential loop `[apply_model(model, m[None], ...)[0] for m in mixes]`, bit for bit, with the same
use of Python's `random`.  Three facts make that possible:

  * `plan()` makes the loop's RNG calls up front, in its order -- track, then bag member, then shift pass:
    `randint(0, max_shift)` once per shift pass and, on the HTDemucs route, `randrange(1)` once per segment forward
    (`apply.device_split_accumulate`); the HDemucs route draws nothing.  After that, forwards may run in any order.
  * A forward's items do not depend on each other or on their batch position (tests/test_gpu_many.py checks this premise),
    so a segment's output is the same whichever forward carries it.
  * Every accumulator receives its segments in ascending offset order (the float32 summation order of `ola.hip`): units are
    listed in offset order per pass, HTDemucs forwards are consecutive slices of that list, and the HDemucs forwards go full
    chunks first, then the shorter tails by descending length (chunk lengths never grow along a pass).

Device side: all tracks live in one packed buffer (one host -> device copy for host inputs), all pass accumulators in
another; each forward needs ONE table upload, ONE gather launch and ONE overlap-add launch however many tracks it spans
(`mi_segments_gather_packed`, `mi_ola_accumulate_packed`), and one `mi_ola_finish_packed` launch finishes every
accumulator of the run.  Shift passes need no padded copy of the track: the gather's zero fill outside [0, length) is the
reference's padding.  HDemucs tail chunks without an equal-length partner run on the model's single-item side engine
under the main engine's batched forwards, as the single-track route runs each track's tail.  The shift and bag averages then run the same torch operations, in the same order, as
`apply._apply_shifts` and `apply._apply_bag`.
"""
from __future__ import annotations

import ctypes as C
import random
from dataclasses import dataclass, field
from typing import Any, List, Optional, Sequence

import torch

from . import _lib
from .hdemucs import HDemucs, MIN_LENGTH as _HDEMUCS_MIN_LENGTH, tail_overlap_enabled
from .htdemucs import HTDemucs

# column layout of the device tables (include/demucs_amd.h, MI_PACK_*)
ITEM_COLS, TILE_COLS, TILE_SPAN = 8, 7, 1024


@dataclass
class Pass:
    """One (track, bag member, shift pass): an accumulator (rows, length) at float offset `acc_base`, whose position 0 is
    track sample `origin` (the shift trick's window start; 0 without shifts)."""
    track: int
    member: int
    shift: Optional[int]            # drawn shift offset, None without shifts
    origin: int
    length: int
    offsets: List[int]
    lens: List[int]
    acc_base: int = 0


@dataclass
class Unit:
    """One segment forward item: pass `pass_idx`, accumulator position `off`, `n` samples from output sample `trim` on;
    its input window starts at track sample `start`."""
    pass_idx: int
    off: int
    n: int
    trim: int
    start: int


@dataclass
class Forward:
    member: int
    valid: int                      # gathered window length (HTDemucs: the leaf's padded length; HDemucs: the chunk length)
    units: List[int]


@dataclass
class Plan:
    members: List[Any]
    bag_weights: Optional[List[List[float]]]
    shifts: int
    segment_lengths: List[int]      # per member
    valid_lengths: List[Optional[int]]
    passes: List[Pass] = field(default_factory=list)
    units: List[Unit] = field(default_factory=list)
    forwards: List[Forward] = field(default_factory=list)
    draws: List[tuple] = field(default_factory=list)        # (name, args, value) of every RNG call, in call order
    acc_floats: int = 0                                     # size of the accumulator buffer

    @property
    def n_forwards(self) -> int:
        return len(self.forwards)


def plan(model, lengths: Sequence[int], shifts: int = 1, overlap: float = 0.25, segment=None, rng=random) -> Plan:
    """Build the unit and forward lists for tracks of `lengths`, making the sequential loop's RNG calls on `rng` in its
    order.  `model` is an engine or a `BagOfModels` of engines; nothing here touches a device."""
    from .apply import BagOfModels, _leaf_valid_length, _segment_plan
    if isinstance(model, BagOfModels):
        members, bag_weights = list(model.models), [list(w) for w in model.weights]
    else:
        members, bag_weights = [model], None
    seg_lens, valids = [], []
    for sub in members:
        if not isinstance(sub, (HTDemucs, HDemucs)):
            raise TypeError(f"the packed scheduler needs HTDemucs / HDemucs engines, got {type(sub).__name__}")
        _, segment_length, _, _ = _segment_plan(sub, 1, overlap, segment)
        seg_lens.append(segment_length)
        valids.append(_leaf_valid_length(sub, segment_length, segment) if isinstance(sub, HTDemucs) else None)
    p = Plan(members, bag_weights, shifts, seg_lens, valids)

    def draw(name, *args):
        value = getattr(rng, name)(*args)
        p.draws.append((name, args, value))
        return value

    acc_base = 0
    for t, length in enumerate(lengths):
        for e, sub in enumerate(members):
            rows = len(sub.sources) * sub.audio_channels
            max_shift = int(0.5 * sub.samplerate)
            for s in range(max(1, shifts)):
                if shifts:
                    shift = draw("randint", 0, max_shift)
                    origin, plen = shift - max_shift, length + max_shift - shift
                else:
                    shift, origin, plen = None, 0, length
                _, segment_length, _, offsets = _segment_plan(sub, plen, overlap, segment)
                lens = [min(plen - o, segment_length) for o in offsets]
                pi = len(p.passes)
                p.passes.append(Pass(t, e, shift, origin, plen, list(offsets), lens, acc_base))
                acc_base += rows * plen
                valid = valids[e]
                for o, n in zip(offsets, lens):
                    trim = (valid - n) // 2 if valid is not None else 0
                    p.units.append(Unit(pi, o, n, trim, origin + o - trim))
                    if valid is not None:
                        draw("randrange", 1)          # transformer.py:680, once per segment forward of a track
    p.acc_floats = acc_base

    for e, sub in enumerate(members):
        mine = [u for u, unit in enumerate(p.units) if p.passes[unit.pass_idx].member == e]
        B = sub.max_batch
        if isinstance(sub, HTDemucs):
            for i in range(0, len(mine), B):
                p.forwards.append(Forward(e, valids[e], mine[i:i + B]))
            continue
        # HDemucs: one chunk length per forward.  Lengths never grow along a pass, so descending length order keeps every
        # accumulator's segments ascending; the full chunks come first, then each tail length on its own
        for n in sorted({p.units[u].n for u in mine}, reverse=True):
            same = [u for u in mine if p.units[u].n == n]
            for i in range(0, len(same), B):
                p.forwards.append(Forward(e, n, same[i:i + B]))
    return p


def forward_tables(p: Plan, fw: Forward, src_offs: Sequence[int], lengths: Sequence[int], w_offs: Sequence[int]):
    """(items, tiles) of one forward as flat int64 lists (MI_PACK_* layout).  Items of one accumulator are consecutive and
    ascending in offset; each accumulator's span is cut into TILE_SPAN-position tiles over its item range."""
    items, tiles = [], []
    w_len = p.segment_lengths[fw.member]
    groups = []                                      # [pass_idx, first item, end item]
    for k, u in enumerate(fw.units):
        unit = p.units[u]
        ps = p.passes[unit.pass_idx]
        items += [src_offs[ps.track], lengths[ps.track], unit.start, ps.acc_base, ps.length, unit.off, unit.n, unit.trim]
        if groups and groups[-1][0] == unit.pass_idx:
            groups[-1][2] = k + 1
        else:
            groups.append([unit.pass_idx, k, k + 1])
    for pi, i0, i1 in groups:
        ps = p.passes[pi]
        us = [p.units[u] for u in fw.units[i0:i1]]
        lo = max(0, min(u.off for u in us))
        hi = min(ps.length, max(u.off + u.n for u in us))
        for pos in range(lo, hi, TILE_SPAN):
            tiles += [ps.acc_base, ps.length, pos, i0, i1, w_offs[fw.member], w_len]
    return items, tiles


def finish_tables(p: Plan, w_offs: Sequence[int]):
    """(tiles, segs) of the finish launch for every accumulator of the plan."""
    tiles, segs = [], []
    for ps in p.passes:
        s0 = len(segs) // 2
        for o, n in zip(ps.offsets, ps.lens):
            segs += [o, n]
        s1 = len(segs) // 2
        for pos in range(0, ps.length, TILE_SPAN):
            tiles += [ps.acc_base, ps.length, pos, s0, s1, w_offs[ps.member], p.segment_lengths[ps.member]]
    return tiles, segs


def _side_tail(p: Plan, fw: Forward) -> bool:
    """An HDemucs forward of ONE tail chunk: it may run on the member's single-item side engine (same result, bit for bit)."""
    sub = p.members[fw.member]
    return (isinstance(sub, HDemucs) and len(fw.units) == 1 and fw.valid < p.segment_lengths[fw.member]
            and fw.valid >= _HDEMUCS_MIN_LENGTH)


def _upload(values, dev) -> torch.Tensor:
    # built on the host, ONE copy (apply._i64)
    return torch.tensor(values, dtype=torch.int64).to(dev)


def run(model, mixes: Sequence[torch.Tensor], device: torch.device, shifts: int, overlap: float, transition_power: float,
        segment) -> List[torch.Tensor]:
    """The packed route of `apply.apply_model_many`: `mixes` all on the host or all on `device` (a GPU)."""
    from .apply import _transition_weight
    assert transition_power >= 1, "transition_power < 1 leads to weird behavior."
    lengths = [int(m.shape[-1]) for m in mixes]
    p = plan(model, lengths, shifts=shifts, overlap=overlap, segment=segment)
    lib = _lib.load()
    host_in = mixes[0].device.type == "cpu"
    channels = int(mixes[0].shape[0])
    with torch.cuda.device(device):
        stream = lambda: C.c_void_p(_lib.current_stream_ptr())          # noqa: E731
        homes = []
        for sub in p.members:
            try:
                homes.append(next(iter(sub.parameters())).device)
            except (AttributeError, StopIteration, TypeError):
                homes.append(None)
            sub.to(device)
            sub.eval()
        # all tracks resident in HBM as one packed buffer, (channels, length_i) at float offset src_offs[i]
        src_offs, total = [], 0
        for n in lengths:
            src_offs.append(total)
            total += channels * n
        if host_in:
            staged = torch.empty(total, dtype=torch.float32, pin_memory=True)
            for m, o, n in zip(mixes, src_offs, lengths):
                staged[o:o + channels * n].view(channels, n).copy_(m)
            tracks = staged.to(device, non_blocking=True)
        else:
            tracks = torch.cat([m.to(torch.float32).reshape(-1) for m in mixes])
        ramps = [_transition_weight(sl, transition_power, device).to(torch.float32) for sl in p.segment_lengths]
        w_offs = [sum(r.numel() for r in ramps[:e]) for e in range(len(ramps))]
        weights = torch.cat(ramps).contiguous()
        acc = torch.zeros(p.acc_floats, device=device, dtype=torch.float32)
        # the finish tables go up first: a host -> device copy issued behind the forwards would wait for them to drain
        fin_tiles, fin_segs = finish_tables(p, w_offs)
        t_fin_tiles, t_fin_segs = _upload(fin_tiles, device), _upload(fin_segs, device)
        bufs = {}
        keep = []                                     # every table stays referenced until the run's launches are enqueued

        def gather(fw, seg):
            """One table upload (items + tiles) and the gather of `fw`'s windows into `seg`, on the current stream."""
            items, tiles = forward_tables(p, fw, src_offs, lengths, w_offs)
            table = _upload(items + tiles, device)
            keep.append(table)
            _lib.check(lib.mi_segments_gather_packed(tracks.data_ptr(), tracks.numel(), channels, C.c_void_p(table.data_ptr()),
                                                     len(fw.units), fw.valid, seg.data_ptr(), seg.numel(), stream()),
                       "mi_segments_gather_packed")
            return table, len(items), len(tiles)

        def overlap_add(fw, tab, out, out_valid):
            table, n_items, n_tiles = tab
            if n_tiles:
                rows = len(p.members[fw.member].sources) * channels
                t_items = table.data_ptr()
                _lib.check(lib.mi_ola_accumulate_packed(acc.data_ptr(), acc.numel(), rows, out.data_ptr(), out_valid, out.numel(),
                                                        C.c_void_p(t_items), len(fw.units), C.c_void_p(t_items + 8 * n_items),
                                                        n_tiles // TILE_COLS, weights.data_ptr(), weights.numel(), stream()),
                           "mi_ola_accumulate_packed")

        # HDemucs tails that have no equal-length partner run on the member's single-item side engine and stream, under the
        # batched forwards of the main engine (as apply.ragged_split_accumulate does per track); their overlap-adds still go
        # on the main stream in plan order, after every full chunk's
        main = torch.cuda.current_stream(device)
        side = {}                                     # forward index -> (table, out)
        if tail_overlap_enabled():
            for e, sub in enumerate(p.members):
                mine = [i for i, fw in enumerate(p.forwards) if fw.member == e and _side_tail(p, fw)]
                if not mine or len(mine) == sum(fw.member == e for fw in p.forwards):
                    continue
                st = sub.side_stream()
                st.wait_stream(main)                  # the packed tracks and whatever produced them
                with torch.cuda.stream(st):
                    for i in mine:
                        fw = p.forwards[i]
                        seg = torch.empty(1, channels, fw.valid, device=device, dtype=torch.float32)
                        tab = gather(fw, seg)
                        side[i] = (tab, sub(seg, aux=True), st)
        waited = set()
        for i, fw in enumerate(p.forwards):
            sub = p.members[fw.member]
            S = len(sub.sources)
            nb = len(fw.units)
            if i in side:
                tab, out, st = side[i]
                if fw.member not in waited:
                    main.wait_stream(st)
                    waited.add(fw.member)
                for t in (tab[0], out):
                    t.record_stream(main)             # allocated under the side stream, consumed on this one
                overlap_add(fw, tab, out, fw.valid)
                continue
            if isinstance(sub, HTDemucs):
                SL = sub.segment_length
                if fw.member not in bufs:
                    B = sub.max_batch
                    seg_buf = torch.zeros(B, channels, SL, device=device, dtype=torch.float32)
                    cut_buf = (torch.empty(B, channels, fw.valid, device=device, dtype=torch.float32) if fw.valid < SL
                               else seg_buf)
                    bufs[fw.member] = (seg_buf, cut_buf, torch.empty(B, S, channels, SL, device=device, dtype=torch.float32))
                seg_buf, cut_buf, out_buf = bufs[fw.member]
                tab = gather(fw, cut_buf[:nb])
                if fw.valid < SL:
                    seg_buf[:nb, :, :fw.valid] = cut_buf[:nb]          # right zero padding, as HTDemucs.forward
                out = out_buf[:nb]
                sub.forward_segments(seg_buf[:nb], out)
                overlap_add(fw, tab, out, SL)
            else:
                seg = torch.empty(nb, channels, fw.valid, device=device, dtype=torch.float32)
                tab = gather(fw, seg)
                overlap_add(fw, tab, sub(seg), fw.valid)
        _lib.check(lib.mi_ola_finish_packed(acc.data_ptr(), acc.numel(), len(p.members[0].sources) * channels,
                                            t_fin_tiles.data_ptr(), len(fin_tiles) // TILE_COLS, t_fin_segs.data_ptr(),
                                            len(fin_segs) // 2, weights.data_ptr(), weights.numel(), stream()),
                   "mi_ola_finish_packed")
        for sub in p.members:
            if isinstance(sub, HDemucs):
                sub.check()          # a time-out of the LAST forward's recurrence would otherwise pass unnoticed
        results = _assemble(p, acc, channels)
        # results without a shift pass are views of the run's accumulator buffer: give each its own storage, as the loop
        # does, so that keeping one result does not keep every track's accumulators resident
        if not host_in:
            results = [r.clone() if r.untyped_storage().data_ptr() == acc.untyped_storage().data_ptr() else r for r in results]
        for sub, home in zip(p.members, homes):
            if home is not None and p.bag_weights is not None:
                sub.to(home)                          # apply._apply_bag puts every member back where it was
        if not host_in:
            return results
        hosts = []
        for r in results:
            h = torch.empty(r.shape, dtype=torch.float32, pin_memory=True)
            h.copy_(r, non_blocking=True)
            hosts.append(h)
        torch.cuda.current_stream(device).synchronize()
        return hosts


def _assemble(p: Plan, acc: torch.Tensor, channels: int) -> List[torch.Tensor]:
    """Per track: the shift average (`apply._apply_shifts`), then the bag average (`apply._apply_bag`), with the same torch
    operations in the same order."""
    by_track: dict = {}
    for ps in p.passes:
        by_track.setdefault(ps.track, {}).setdefault(ps.member, []).append(ps)
    results = []
    for t in range(len(by_track)):
        member_out = []
        for e, sub in enumerate(p.members):
            S = len(sub.sources)
            out = None
            for ps in by_track[t][e]:
                res = acc[ps.acc_base:ps.acc_base + S * channels * ps.length].view(S, channels, ps.length)
                if ps.shift is None:
                    out = res
                    continue
                max_shift = int(0.5 * sub.samplerate)
                piece = res[..., max_shift - ps.shift:]
                out = piece.clone() if out is None else out.add_(piece)
            if p.shifts:
                out /= p.shifts
            member_out.append(out)
        if p.bag_weights is None:
            results.append(member_out[0])
            continue
        totals = [0.0] * len(p.members[0].sources)
        estimates = None
        for out, sub_weights in zip(member_out, p.bag_weights):
            for k, w in enumerate(sub_weights):
                out[k, :, :] *= w
                totals[k] += w
            estimates = out if estimates is None else estimates.add_(out)
        for k in range(estimates.shape[0]):
            estimates[k, :, :] /= totals[k]
        results.append(estimates)
    return results
