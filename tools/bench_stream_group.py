"""Many concurrent streams (`apply_model_stream_group`, demucs_amd/stream.py) against the same streams as solo `ModelStream`s.

Seeded synthetic audio on the host (`demucs_amd.synth`), synthetic weights, htdemucs f32 and bf16, shifts=1, max_batch=8.  For
N in {1, 8, 32, 64} streams of `--seconds` each, pushed from the host in 0.1 s or 1 s blocks, with starts in lockstep or staggered
(stream i opens i * 0.37 s into the run, modulo 6 s), one round per block time pushes every live stream's next block and then
finishes the streams that have reached their end.  The group does a round as one `push` (and one `finish`); the solo run as N
`push` calls (and `finish` calls).  Every call's wall time (host clock) ends in a device synchronise.  Reported per case and
per side: aggregate real-time factor (audio seconds of all streams / wall seconds, finishes included), median and p99 wall time
of a round's pushes, the number of forwards and their mean batch size (counted at `mi_model_forward`).  The group and the solo
run alternate in one process (group, solo, group, solo) after one warm-up of each; each side reports its faster run.
`--sr RATE` pushes the same audio duration as stereo blocks at RATE: the group's streams are opened converting
(`SeparatorStreamGroup.open(sr=RATE)`, one `mi_streams_convert_append` per round) and the solo side is
`Separator.separate_stream(sr=RATE, convert=True)`.
Prints ONE JSON line (and writes it to --out when given).

    python tools/bench_stream_group.py --out profiles/stream_group_bench.json
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

from demucs_amd import _lib  # noqa: E402
from demucs_amd.apply import apply_model_stream, apply_model_stream_group  # noqa: E402
from demucs_amd.htdemucs import HTDemucs  # noqa: E402
from demucs_amd.synth import synth_mix  # noqa: E402
from demucs_amd.weights import HTDemucsConfig, synthetic_state_dict  # noqa: E402

SR = 44100


def model(mode: str) -> HTDemucs:
    m = HTDemucs(HTDemucsConfig().sources, max_batch=8, compute_dtype=mode)
    m.load_state_dict(synthetic_state_dict(HTDemucsConfig(), 0))
    return m.to("cuda").eval()


def rounds(n_streams: int, length: int, block: int, staggered: bool, sr: int = SR):
    """[(opens, pushes {i: (pos, n)}, finishes)] per round."""
    start = [int(((i * 0.37) % 6.0) * sr) // block if staggered else 0 for i in range(n_streams)]
    n_blocks = -(-length // block)
    out = []
    for r in range(max(start) + n_blocks):
        opens = [i for i in range(n_streams) if start[i] == r]
        pushes = {i: ((r - start[i]) * block, min(block, length - (r - start[i]) * block))
                  for i in range(n_streams) if start[i] <= r < start[i] + n_blocks}
        ends = [i for i in range(n_streams) if r == start[i] + n_blocks - 1]
        out.append((opens, pushes, ends))
    return out


class ForwardCounter:
    def __init__(self):
        self.lib = _lib.load()
        self.real = self.lib.mi_model_forward
        self.batches = []

    def __enter__(self):
        def counting(*args):
            self.batches.append(args[3])
            return self.real(*args)
        self.lib.mi_model_forward = counting
        return self

    def __exit__(self, *exc):
        self.lib.mi_model_forward = self.real


def run(m, audio, plan, grouped: bool, sr: int = SR):
    times = []
    sep = None
    if sr != SR:
        from demucs_amd.api import Separator
        sep = Separator(m, device="cuda", shifts=1)
    with ForwardCounter() as fc:
        torch.cuda.synchronize()
        t_all = time.perf_counter()
        if grouped:
            g = apply_model_stream_group(m, shifts=1, device="cuda") if sep is None else sep.separate_stream_group()
            keys = {}
            for opens, pushes, ends in plan:
                for i in opens:
                    keys[i] = g.open() if sep is None else g.open(sr=sr)
                t0 = time.perf_counter()
                g.push({keys[i]: audio[:, p:p + n] for i, (p, n) in pushes.items()})
                torch.cuda.synchronize()
                times.append(time.perf_counter() - t0)
                if ends:
                    g.finish([keys[i] for i in ends])
        else:
            streams = {}
            for opens, pushes, ends in plan:
                for i in opens:
                    streams[i] = apply_model_stream(m, shifts=1, device="cuda") if sep is None else \
                        sep.separate_stream(sr=sr, convert=True)
                t0 = time.perf_counter()
                for i, (p, n) in pushes.items():
                    streams[i].push(audio[:, p:p + n])
                torch.cuda.synchronize()
                times.append(time.perf_counter() - t0)
                for i in ends:
                    streams.pop(i).finish()
        torch.cuda.synchronize()
        wall = time.perf_counter() - t_all
    times.sort()
    return {
        "wall_s": round(wall, 3),
        "push_ms_median": round(1e3 * statistics.median(times), 3),
        "push_ms_p99": round(1e3 * times[min(len(times) - 1, int(0.99 * len(times)))], 3),
        "forwards": len(fc.batches),
        "mean_batch": round(sum(fc.batches) / max(1, len(fc.batches)), 2),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=60.0, help="length of every stream")
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--streams", default="1,8,32,64")
    ap.add_argument("--blocks", default="0.1,1")
    ap.add_argument("--modes", default="f32,bf16")
    ap.add_argument("--sr", type=int, default=SR, help="sample rate of the pushed blocks (converted on the streams when not 44100)")
    ap.add_argument("--starts", default="lockstep,staggered")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sr = args.sr
    length = int(args.seconds * sr)
    audio = torch.from_numpy(synth_mix(1, length, "tones"))
    result = {"what": "apply_model_stream_group vs solo apply_model_stream, htdemucs, shifts=1, max_batch=8, host blocks",
              "device": torch.cuda.get_device_name(0), "stream_seconds": args.seconds, "input_sr": sr, "reps": args.reps, "runs": {}}
    for mode in args.modes.split(","):
        m = model(mode)
        warm = rounds(2, 10 * sr, sr, False, sr)
        run(m, audio, warm, True, sr)
        run(m, audio, warm, False, sr)
        for n_streams in (int(x) for x in args.streams.split(",")):
            for block_s in (float(x) for x in args.blocks.split(",")):
                for staggered in [x == "staggered" for x in args.starts.split(",")]:
                    plan = rounds(n_streams, length, int(block_s * sr), staggered, sr)
                    grps, solos = [], []
                    for _ in range(args.reps):
                        grps.append(run(m, audio, plan, True, sr))
                        solos.append(run(m, audio, plan, False, sr))
                    grp = min(grps, key=lambda r: r["wall_s"])
                    solo = min(solos, key=lambda r: r["wall_s"])
                    audio_s = n_streams * args.seconds
                    grp["realtime_factor"] = round(audio_s / grp["wall_s"], 1)
                    solo["realtime_factor"] = round(audio_s / solo["wall_s"], 1)
                    name = f"{mode}_n{n_streams}_block{block_s:g}s_{'staggered' if staggered else 'lockstep'}"
                    result["runs"][name] = {"group": grp, "solo": solo,
                                            "group_over_solo_rtf": round(grp["realtime_factor"] / solo["realtime_factor"], 2)}
                    print(name, result["runs"][name], file=sys.stderr, flush=True)
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
