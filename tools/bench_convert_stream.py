"""`mi_streams_convert_append` (the streaming `convert_audio` kernel, demucs_amd/csrc/convert_stream.hip) given a whole track as ONE
block, against `mi_resample_frac` (demucs_amd/csrc/resample.hip) on the same input.

A `--seconds` stereo track of seeded noise at `--sr` on the device; both kernels write (2, floor(new * L / old)) float32 and the
results are compared bit for bit first.  Then `--reps` rounds, each timing both kernels with device events over `--iters`
back-to-back launches after a warm-up, in alternating order (a, b, b, a, ...).  Reported: each kernel's median and min / max over
the rounds in milliseconds per launch, and the ratio of the medians.  Prints ONE JSON line (and writes it to --out when given).

    python tools/bench_convert_stream.py --out profiles/convert_stream_kernel.json
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=180.0)
    ap.add_argument("--sr", type=int, default=48000)
    ap.add_argument("--to", type=int, default=44100)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lib = _lib.load()
    plan = audio.ConvertPlan(args.sr, args.to)
    L = int(args.seconds * args.sr)
    x = torch.randn(2, L, generator=torch.Generator().manual_seed(0)).cuda()
    n_out = plan.final_count(L)
    width, bank = audio.sinc_bank(plan.old, plan.new)
    table_old = bank.cuda()
    bank_t = bank.t().contiguous().reshape(-1).cuda()
    y_old, y_new = torch.empty(2, n_out, device="cuda"), torch.empty(2, n_out, device="cuda")
    row = [x.data_ptr(), 2, L, 0, 0, 0, 0, 0, -1, 0, n_out, L, plan.old, plan.new, plan.width, 0, 0, n_out, 0, -1]
    table = torch.tensor(row, dtype=torch.int64).cuda()
    stream = lambda: C.c_void_p(_lib.current_stream_ptr())          # noqa: E731

    def old():
        _lib.check(lib.mi_resample_frac(x.data_ptr(), 2, L, table_old.data_ptr(), plan.old, plan.new, width, y_old.data_ptr(), n_out,
                                        stream()), "mi_resample_frac")

    def new():
        _lib.check(lib.mi_streams_convert_append(y_new.data_ptr(), y_new.numel(), 2, table.data_ptr(), 1, plan.groups(n_out),
                                                 bank_t.data_ptr(), bank_t.numel(), None, 0, None, 0, plan.lds_floats(), stream()),
                   "mi_streams_convert_append")

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(args.iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / args.iters

    old()
    new()
    torch.cuda.synchronize()
    same = bool((y_old.view(torch.int32) == y_new.view(torch.int32)).all())
    for _ in range(3):
        timed(old)
        timed(new)
    t = {"old": [], "new": []}
    for r in range(args.reps):
        for name in (("old", "new") if r % 2 == 0 else ("new", "old")):
            t[name].append(timed(old if name == "old" else new))
    moved = 4.0 * (x.numel() + y_old.numel())

    def stat(v):
        med = statistics.median(v)
        return {"ms_median": round(med, 4), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4),
                "GB_per_s_at_median": round(moved / med / 1e6, 1)}

    result = {"what": "mi_streams_convert_append on a whole track as one block vs mi_resample_frac, device events",
              "device": torch.cuda.get_device_name(0), "seconds": args.seconds, "from_sr": args.sr, "to_sr": args.to,
              "reps": args.reps, "iters": args.iters, "same_bits": same, "mi_resample_frac": stat(t["old"]),
              "mi_streams_convert_append": stat(t["new"]),
              "old_over_new": round(statistics.median(t["old"]) / statistics.median(t["new"]), 3)}
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    assert same, "the two kernels disagree"


if __name__ == "__main__":
    main()
