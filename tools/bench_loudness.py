"""The loudness pass (`mi_loudness_update`, demucs_amd/csrc/loudness.hip) beside the streaming pass over the same data that the
project already ships, `mi_deliver_mix_peaks_update` (demucs_amd/csrc/deliver_mix.hip).

A `--minutes` 4-stem stereo track (seeded noise) and its mix lie on the device; five outputs are measured: the four stems and
`mix - vocals`.  Three things are timed by device events around `--reps` back-to-back calls, `--rounds` times in alternating
order after a warm-up:

  whole    ONE `mi_loudness_update` call over the whole track (both launches);
  push     one stream push of `--stride` samples (a segment stride of HTDemucs) in the middle of the track, the carried values
           in front of it;
  peaks    `mi_deliver_mix_peaks_update` on the whole track's rows.

`whole` and `push` are also timed with the recursion launch left out (max_blocks = 0), which splits each time between the two
launches.

Beside the times: the float64 FMAs the recursions issue (11 per step: five per biquad and the square; a sub-block's window is
warm-up + hop steps) and the bytes the passes read, so that each time can be set against a rate of the machine.
Prints ONE JSON line and writes it to --out.

    python tools/bench_loudness.py --out profiles/loudness_bench.json
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

import torch  # noqa: E402

from demucs_amd import _lib, audio  # noqa: E402

SR = 44100
SOURCES = ["drums", "bass", "other", "vocals"]
MIX = {**{k: {k: 1.0} for k in SOURCES}, "karaoke": {"mix": 1.0, "vocals": -1.0}}


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
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "loudness_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_loudness.py measures on the GPU and none is available")
    lib = _lib.load()
    S, ch, L = len(SOURCES), 2, int(args.minutes * 60 * SR)
    hop, warm = SR // 10, audio.loudness_warmup(SR)
    gains = audio.mix_gains(MIX, SOURCES)
    R = len(gains)
    g = torch.Generator(device="cuda").manual_seed(1)
    stems = 0.2 * torch.randn(S, ch, L, device="cuda", generator=g)
    origin = stems.sum(0)
    k = audio.k_weighting(SR)
    coef = (C.c_double * 10)(*k[0, 0], *k[0, 1, 1:], *k[1, 0], *k[1, 1, 1:])
    hist_len = warm + hop
    hist = torch.randn(2, R, ch, hist_len, device="cuda", generator=g)
    stream = lambda: C.c_void_p(_lib.current_stream_ptr())          # noqa: E731

    def loudness_call(before, n, hist_start):
        """One mi_loudness_update over samples [before, before + n) of the track, read in place."""
        kept, done = before - hist_start, (before + n) // hop
        nxt = max(0, done * hop - warm)
        energies = torch.zeros(R, ch, done, dtype=torch.float64, device="cuda")
        work = torch.empty(R * ch * (kept + n), dtype=torch.float32, device="cuda")
        rows = audio.loud_rows(gains, stems.data_ptr() + 4 * before, L, n, origin.data_ptr() + 4 * before, L, None, before, hist_len, 0,
                               hist_start, nxt, ch, done, kept + n)
        table = torch.tensor(rows, dtype=torch.int64).cuda()
        blocks = done - before // hop

        def call(blocks=blocks):
            _lib.check(lib.mi_loudness_update(table.data_ptr(), R, kept + n, blocks, S, ch, coef, hop, warm, hist.data_ptr(),
                                              hist.numel(), energies.data_ptr(), energies.numel(), work.data_ptr(), work.numel(),
                                              stream()), "mi_loudness_update")
        return call, energies, blocks

    whole, e_whole, blocks_whole = loudness_call(0, L, 0)
    before = L // 2
    push, e_push, blocks_push = loudness_call(before, min(args.stride, L - before), max(0, before // hop * hop - warm))
    peak_rows = audio.mix_rows(gains, stems.data_ptr(), L, origin.data_ptr(), L, None, audio.clip_code("rescale"), 0, "i16", None)
    peak_table = torch.tensor(peak_rows, dtype=torch.int64).cuda()
    slots = torch.zeros(R, dtype=torch.int32, device="cuda")

    def peaks():
        _lib.check(lib.mi_deliver_mix_peaks_update(peak_table.data_ptr(), R, L, S, ch, slots.data_ptr(), R, stream()),
                   "mi_deliver_mix_peaks_update")

    # max_blocks = 0 leaves the recursion launch out: the first launch alone
    routes = {"whole": whole, "push": push, "peaks": peaks, "whole_values": lambda: whole(0), "push_values": lambda: push(0)}
    for fn in routes.values():
        timed(fn, 3)
    ms = {name: [] for name in routes}
    for r in range(args.rounds):
        for name in (list(routes) if r % 2 == 0 else list(routes)[::-1]):
            ms[name].append(timed(routes[name], args.reps))
    med = {name: statistics.median(v) for name, v in ms.items()}
    # the whole-track energies against the library's own streamed route: the same bytes
    same = audio.loudness(origin, dict(zip(SOURCES, stems)), MIX, SR).energies.tobytes() == e_whole.cpu().numpy().tobytes()

    terms = sum(sum(1 for v in row if v != 0) for _, row in gains)           # values read per sample and channel, all outputs
    read_bytes = terms * ch * L * 4
    fma = lambda blocks: 11 * R * ch * blocks * (warm + hop)                 # noqa: E731  (upper bound: the first windows are shorter)
    result = {
        "what": "mi_loudness_update (values + history launch, recursion launch) on a 4-stem stereo track resident on the device, five "
                "outputs (the stems and mix - vocals): the whole track in one call, one stream push of a segment stride, and "
                "mi_deliver_mix_peaks_update over the same rows; device events around back-to-back calls, alternating order",
        "device": torch.cuda.get_device_name(0), "minutes": args.minutes, "length": L, "outputs": R, "channels": ch, "hop": hop,
        "warm": warm, "stride": args.stride, "reps": args.reps, "rounds": args.rounds,
        "whole_ms": spread(ms["whole"]), "push_ms": spread(ms["push"]), "peaks_ms": spread(ms["peaks"]),
        "whole_values_launch_ms": spread(ms["whole_values"]), "push_values_launch_ms": spread(ms["push_values"]),
        "whole_sub_blocks": R * ch * blocks_whole, "push_sub_blocks": R * ch * blocks_push,
        "whole_waves": R * ch * -(-blocks_whole // 64), "push_waves": R * ch * -(-blocks_push // 64),
        "steps_per_sub_block": warm + hop,
        "whole_fp64_fma": fma(blocks_whole), "whole_fp64_tflops": round(2 * fma(blocks_whole) / (med["whole"] * 1e-3) / 1e12, 3),
        "push_fp64_tflops": round(2 * fma(blocks_push) / (med["push"] * 1e-3) / 1e12, 3),
        "ns_per_step_whole": round((med["whole"] - med["whole_values"]) * 1e6 / (warm + hop), 2),
        "ns_per_step_push": round((med["push"] - med["push_values"]) * 1e6 / (warm + hop), 2),
        "values_read_bytes": read_bytes, "peaks_tb_per_s": round(read_bytes / (med["peaks"] * 1e-3) / 1e12, 3),
        "whole_over_peaks": round(med["whole"] / med["peaks"], 2),
        "whole_equals_streamed_bytes": bool(same),
    }
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
