"""Delivered frames against float stems on a stream group (`SeparatorStreamGroup.open(deliver=)`, demucs_amd/stream.py).

The method of tools/bench_stream_group.py: seeded synthetic audio on the host, synthetic weights, htdemucs, shifts=1, max_batch=8,
N streams of `--seconds` each pushed in lockstep from the host in `--block`-second blocks, one group `push` per round, every
round's wall time (host clock) ending in a device synchronise.  Two routes over the same rounds:

  float      no `deliver`: every push returns `{source: (channels, m) float32}` on the host, 4 sources x 2 channels x 4 B per sample;
  delivered  `Delivery("vocals")` (the karaoke pair `vocals` + `no_vocals`, clip "clamp", int16 interleaved): 2 x 2 x 2 B per sample.

The routes alternate in one process (float, delivered, float, delivered, ...) after one warm-up of each, `--pairs` times.  Reported
per route: host-bound bytes per round and per sample (the `nbytes` of what `push` returned), every pair's aggregate real-time
factor (audio seconds of all streams / wall seconds, the finish included), its median, and the spread (max - min) of the float
route's own pairs, the yardstick for "not slower": delivered_median >= float_median - float_spread.
Prints ONE JSON line (and writes it to --out when given).

    python tools/bench_deliver.py --out profiles/deliver_bench.json

With `--out-sr R` the pair is instead the delivered route at the model's rate (`Delivery("vocals")`, the run of record) and the
same route at R Hz (`Delivery("vocals", samplerate=R)`: `mi_deliver_resample_pcm` in `mi_deliver_pcm`'s place), by the same
method; `rate_over_model` is the ratio of their median real-time factors.  No speed is claimed for it.

    python tools/bench_deliver.py --out-sr 48000 --out profiles/deliver_rate_bench.json
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

from demucs_amd.api import Delivery, Separator  # noqa: E402
from demucs_amd.htdemucs import HTDemucs  # noqa: E402
from demucs_amd.synth import synth_mix  # noqa: E402
from demucs_amd.weights import HTDemucsConfig, synthetic_state_dict  # noqa: E402

SR = 44100


def model(mode: str) -> HTDemucs:
    m = HTDemucs(HTDemucsConfig().sources, max_batch=8, compute_dtype=mode)
    m.load_state_dict(synthetic_state_dict(HTDemucsConfig(), 0))
    return m.to("cuda").eval()


def run(sep: Separator, audio: torch.Tensor, n_streams: int, block: int, deliver):
    length = audio.shape[1]
    times, nbytes, samples = [], 0, 0
    torch.cuda.synchronize()
    t_all = time.perf_counter()
    g = sep.separate_stream_group()
    keys = [g.open(0.0, 1.0, deliver=deliver) for _ in range(n_streams)]
    for p in range(0, length, block):
        t0 = time.perf_counter()
        out = g.push({k: audio[:, p:p + block] for k in keys})
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
        for frames in out.values():
            first = next(iter(frames.values()))
            samples += first.shape[0] if deliver is not None else first.shape[-1]
            nbytes += sum(v.nbytes for v in frames.values())
    g.finish(keys)
    torch.cuda.synchronize()
    wall = time.perf_counter() - t_all
    times.sort()
    return {"wall_s": wall, "push_ms_median": 1e3 * statistics.median(times),
            "host_bytes_per_round": nbytes / max(1, len(times)), "host_bytes_per_sample": nbytes / max(1, samples)}


def summary(runs, audio_s: float) -> dict:
    rtf = [audio_s / r["wall_s"] for r in runs]
    return {"realtime_factor_pairs": [round(x, 1) for x in rtf], "realtime_factor_median": round(statistics.median(rtf), 1),
            "realtime_factor_spread": round(max(rtf) - min(rtf), 1),
            "push_ms_median": round(statistics.median(r["push_ms_median"] for r in runs), 3),
            "host_bytes_per_round": round(runs[0]["host_bytes_per_round"]), "host_bytes_per_sample": runs[0]["host_bytes_per_sample"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=30.0, help="length of every stream")
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--streams", default="8,32")
    ap.add_argument("--block", type=float, default=1.0)
    ap.add_argument("--modes", default="f32,bf16")
    ap.add_argument("--out", default=None)
    ap.add_argument("--out-sr", type=int, default=None, help="compare delivery at the model's rate with delivery at this rate")
    args = ap.parse_args()
    if args.out_sr is not None:
        return rate_main(args)
    length = int(args.seconds * SR)
    audio = torch.from_numpy(synth_mix(1, length, "tones"))
    karaoke = Delivery("vocals")
    result = {"what": "stream group, htdemucs, shifts=1, max_batch=8, lockstep host blocks: float stems vs Delivery('vocals') int16",
              "device": torch.cuda.get_device_name(0), "stream_seconds": args.seconds, "block_seconds": args.block,
              "pairs": args.pairs, "runs": {}}
    for mode in args.modes.split(","):
        sep = Separator(model(mode), device="cuda", shifts=1)
        warm = audio[:, :10 * SR]
        run(sep, warm, 2, SR, None)
        run(sep, warm, 2, SR, karaoke)
        for n_streams in (int(x) for x in args.streams.split(",")):
            floats, delivered = [], []
            for _ in range(args.pairs):
                floats.append(run(sep, audio, n_streams, int(args.block * SR), None))
                delivered.append(run(sep, audio, n_streams, int(args.block * SR), karaoke))
            f, d = summary(floats, n_streams * args.seconds), summary(delivered, n_streams * args.seconds)
            name = f"{mode}_n{n_streams}"
            result["runs"][name] = {"float": f, "delivered": d,
                                    "not_slower": d["realtime_factor_median"] >= f["realtime_factor_median"] - f["realtime_factor_spread"]}
            print(name, result["runs"][name], file=sys.stderr, flush=True)
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


def rate_main(args):
    length = int(args.seconds * SR)
    audio = torch.from_numpy(synth_mix(1, length, "tones"))
    at_model, at_rate = Delivery("vocals"), Delivery("vocals", samplerate=args.out_sr)
    result = {"what": f"stream group, htdemucs, shifts=1, max_batch=8, lockstep host blocks: Delivery('vocals') int16 at the model's "
                      f"{SR} Hz vs at {args.out_sr} Hz",
              "device": torch.cuda.get_device_name(0), "stream_seconds": args.seconds, "block_seconds": args.block,
              "pairs": args.pairs, "out_sr": args.out_sr, "runs": {}}
    for mode in args.modes.split(","):
        sep = Separator(model(mode), device="cuda", shifts=1)
        warm = audio[:, :10 * SR]
        run(sep, warm, 2, SR, at_model)
        run(sep, warm, 2, SR, at_rate)
        for n_streams in (int(x) for x in args.streams.split(",")):
            plain, rated = [], []
            for _ in range(args.pairs):
                plain.append(run(sep, audio, n_streams, int(args.block * SR), at_model))
                rated.append(run(sep, audio, n_streams, int(args.block * SR), at_rate))
            a, b = summary(plain, n_streams * args.seconds), summary(rated, n_streams * args.seconds)
            name = f"{mode}_n{n_streams}"
            result["runs"][name] = {"model_rate": a, "out_rate": b,
                                    "rate_over_model": round(b["realtime_factor_median"] / a["realtime_factor_median"], 3)}
            print(name, result["runs"][name], file=sys.stderr, flush=True)
    line = json.dumps(result)
    print(line)
    out = args.out or os.path.join(ROOT, "profiles", "deliver_rate_bench.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
