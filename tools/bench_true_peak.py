"""The true-peak pass (`mi_true_peak_update`, demucs_amd/csrc/true_peak.hip) beside `mi_deliver_mix_peaks_update`
(demucs_amd/csrc/deliver_mix.hip) over the same rows: that entry does the same loads and the same reduction without the filter, so
it is the floor.

A `--minutes` 4-stem stereo track (seeded noise) and its mix lie on the device; five outputs are measured, the default `mix` of
`Separator.levels_tensor`: the four stems and the mix.  Timed by device events around `--reps` back-to-back calls, `--rounds`
alternating pairs after a warm-up:

  whole    ONE `mi_true_peak_update` call over the whole track with Annex 2's 4 x 12 bank (the instance with its window in
           registers);
  generic  the same with the bank padded by a zero tap to 4 x 13, which takes the generic loop (13 / 12 of the arithmetic): what
           the unrolled window buys;
  push     one stream push of `--stride` samples (a segment stride of HTDemucs) in the middle of the track, the carried values in
           front of it;
  peaks    `mi_deliver_mix_peaks_update` on the whole track's rows.

Prints ONE JSON line and writes it to --out.

    python tools/bench_true_peak.py --out profiles/true_peak_bench.json
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from demucs_amd import _lib, audio  # noqa: E402

SR = 44100
SOURCES = ["drums", "bass", "other", "vocals"]
MIX = {**{k: {k: 1.0} for k in SOURCES}, "mix": {"mix": 1.0}}


def spread(values, digits=4):
    return {"all": [round(v, digits) for v in values], "median": round(statistics.median(values), digits),
            "min": round(min(values), digits), "max": round(max(values), digits)}


def timed(fn, reps):
    """ms per call of `reps` back-to-back calls, by device events."""
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--minutes", type=float, default=3.0)
    ap.add_argument("--stride", type=int, default=257985, help="samples of the timed stream push (HTDemucs: 0.75 of a 7.8 s segment)")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "true_peak_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_true_peak.py measures on the GPU and none is available")
    lib = _lib.load()
    S, ch, L = len(SOURCES), 2, int(args.minutes * 60 * SR)
    gains = audio.mix_gains(MIX, SOURCES)
    R = len(gains)
    g = torch.Generator(device="cuda").manual_seed(1)
    stems = 0.2 * torch.randn(S, ch, L, device="cuda", generator=g)
    origin = stems.sum(0)
    annex = audio.true_peak_bank(SR)
    padded = np.concatenate([annex, np.zeros((annex.shape[0], 1), dtype=np.float32)], 1)
    stream = lambda: C.c_void_p(_lib.current_stream_ptr())          # noqa: E731

    def true_peak_call(bank, before, n, tail, carried):
        """One mi_true_peak_update over samples [before, before + n) of the track, read in place."""
        keep = bank.shape[1] - 1
        dev_bank = torch.from_numpy(np.ascontiguousarray(bank)).cuda()
        hist = torch.randn(2, R, ch, keep, device="cuda", generator=g) if carried else None
        slots = torch.zeros(2 * R, dtype=torch.int32, device="cuda")
        rows = audio.true_peak_rows(gains, stems.data_ptr() + 4 * before, L, n, origin.data_ptr() + 4 * before, L, None, before, tail,
                                    keep if carried else 0, 0, before - keep if carried else 0,
                                    before + n - keep if carried else -1, ch)
        table = torch.tensor(rows, dtype=torch.int64).cuda()

        def call():
            if not carried:
                slots.zero_()                                       # a track starts from empty slots: every early maximum is an atomic
            _lib.check(lib.mi_true_peak_update(table.data_ptr(), R, n + tail, S, ch, dev_bank.data_ptr(), bank.shape[0], bank.shape[1],
                                               0 if hist is None else hist.data_ptr(), 0 if hist is None else hist.numel(),
                                               slots.data_ptr(), R, stream()), "mi_true_peak_update")
        return call, slots

    whole, slots_whole = true_peak_call(annex, 0, L, annex.shape[1] - 1, False)
    generic, slots_generic = true_peak_call(padded, 0, L, padded.shape[1] - 1, False)
    before = L // 2
    push, _ = true_peak_call(annex, before, min(args.stride, L - before), 0, True)
    peak_rows = audio.mix_rows(gains, stems.data_ptr(), L, origin.data_ptr(), L, None, audio.clip_code("rescale"), 0, "i16", None)
    peak_table = torch.tensor(peak_rows, dtype=torch.int64).cuda()
    slots_peaks = torch.zeros(R, dtype=torch.int32, device="cuda")

    def peaks():
        _lib.check(lib.mi_deliver_mix_peaks_update(peak_table.data_ptr(), R, L, S, ch, slots_peaks.data_ptr(), R, stream()),
                   "mi_deliver_mix_peaks_update")

    routes = {"whole": whole, "peaks": peaks, "generic": generic, "push": push}
    for fn in routes.values():
        timed(fn, 3)
    ms = {name: [] for name in routes}
    for r in range(args.rounds):
        for name in (list(routes) if r % 2 == 0 else list(routes)[::-1]):
            ms[name].append(timed(routes[name], args.reps))
    med = {name: statistics.median(v) for name, v in ms.items()}
    # the slots against the library's own route and the floor's: the same bits
    measured = audio.true_peak(origin, dict(zip(SOURCES, stems)), MIX, SR)
    got = [v & 0xFFFFFFFF for v in slots_whole.cpu().tolist()]
    same = tuple(got[0::2]) == measured.bits and tuple(got[1::2]) == measured.sample_bits
    same_sample = got[1::2] == [v & 0xFFFFFFFF for v in slots_peaks.cpu().tolist()]
    same_generic = got == [v & 0xFFFFFFFF for v in slots_generic.cpu().tolist()]

    terms = sum(sum(1 for v in row if v != 0) for _, row in gains)           # values read per sample and channel, all outputs
    read_bytes = terms * ch * L * 4
    ops = 2 * annex.size * R * ch * L                                        # rounded multiplies and adds of the chains
    result = {
        "what": "mi_true_peak_update on a 4-stem stereo track resident on the device, five outputs (the stems and the mix): the whole "
                "track in one call with the 4 x 12 bank (unrolled window) and with a 4 x 13 bank (generic loop), one stream push of a "
                "segment stride, and mi_deliver_mix_peaks_update over the same rows; device events around back-to-back calls, "
                "alternating order",
        "device": torch.cuda.get_device_name(0), "minutes": args.minutes, "length": L, "outputs": R, "channels": ch,
        "stride": args.stride, "reps": args.reps, "rounds": args.rounds,
        "whole_ms": spread(ms["whole"]), "generic_ms": spread(ms["generic"]), "push_ms": spread(ms["push"]),
        "peaks_ms": spread(ms["peaks"]),
        "whole_over_peaks": round(med["whole"] / med["peaks"], 2), "generic_over_whole": round(med["generic"] / med["whole"], 2),
        "values_read_bytes": read_bytes, "peaks_tb_per_s": round(read_bytes / (med["peaks"] * 1e-3) / 1e12, 3),
        "whole_tb_per_s": round(read_bytes / (med["whole"] * 1e-3) / 1e12, 3),
        "chain_ops": ops, "whole_fp32_tops": round(ops / (med["whole"] * 1e-3) / 1e12, 2),
        "dbtp": [round(measured.dbtp(n), 3) for n in measured.names],
        "whole_equals_library_route": bool(same), "sample_slots_equal_deliver_mix_peaks": bool(same_sample),
        "generic_equals_unrolled": bool(same_generic),
    }
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
