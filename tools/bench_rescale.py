"""What `clip="rescale"` costs on a stream: one long synthetic track through `Separator.separate_blocks`, three ways.

  clamp     `Delivery(clip="clamp")`: two passes over the source (analysis, separation); int16 frames to the host.
  rescale   `Delivery(clip="rescale", peaks="measure")`: three passes (analysis, a measuring separation that keeps 4 bytes per
            output on the device, the delivering separation); the same int16 frames to the host.
  floats    no `deliver=`: two passes, the float32 stems of every push to the host, then `audio.deliver(clip="rescale")` on the whole
            track -- the only way to the reference's default files without the measuring pass.

A `--minutes` stereo feed (seeded synthetic audio, `--unique` seconds of it repeated) is pushed from the host in `--block` second
float blocks; a run is timed with a host clock from the first read of the source to the last frame on the host.  After one warm-up
of each the three run `--rounds` times in rotating order; `rescale` and `floats` are compared bit for bit.  The bytes copied to
the host are counted from the tensors returned.  Prints ONE JSON line and writes it to --out.

    python tools/bench_rescale.py --out profiles/rescale_bench.json
"""
from __future__ import annotations

import argparse
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

from demucs_amd import audio  # noqa: E402
from demucs_amd.api import Delivery, Separator  # noqa: E402
from demucs_amd.htdemucs import HTDemucs  # noqa: E402
from demucs_amd.synth import synth_mix  # noqa: E402
from demucs_amd.weights import HTDemucsConfig, synthetic_state_dict  # noqa: E402

SR = 44100


def delivered(sep, source, deliver, seed):
    """(ms, {name: frames}, bytes to the host) of `separate_blocks(source, deliver=deliver)`, the frames joined on the host."""
    random.seed(seed)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    parts = list(sep.separate_blocks(source, deliver=deliver))
    frames = {k: torch.cat([p[k] for p in parts], 0) for k in parts[0]}
    ms = (time.perf_counter() - t0) * 1e3
    n_bytes = sum(v.numel() * v.element_size() for p in parts for v in p.values())
    return ms, frames, n_bytes + (4 * len(frames) if deliver.measures else 0)


def through_floats(sep, source, whole, stem, seed):
    """(ms, frames, bytes to the host): float stems of every push to the host, then `audio.deliver(clip="rescale")`."""
    random.seed(seed)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    parts = list(sep.separate_blocks(source))
    stems = {k: torch.cat([p[k] for p in parts], -1) for k in parts[0]}
    n_bytes = sum(v.numel() * v.element_size() for v in stems.values())
    del parts
    frames = audio.deliver(whole, stems, stem=stem, clip="rescale")
    ms = (time.perf_counter() - t0) * 1e3
    return ms, frames, n_bytes + sum(v.numel() * v.element_size() for v in frames.values())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--minutes", type=float, default=60.0)
    ap.add_argument("--block", type=float, default=10.0, help="seconds per push")
    ap.add_argument("--unique", type=int, default=60, help="seconds of distinct audio, repeated to the feed's length")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--batch", type=int, default=32, help="segments per batched forward")
    ap.add_argument("--stem", default=None, help="two-stems delivery of this source (default: every source)")
    ap.add_argument("--gain", type=float, default=1.0, help="scales the feed (the stems follow it)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rescale_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_rescale.py measures on the GPU and none is available")
    cfg = HTDemucsConfig()
    model = HTDemucs(cfg.sources, max_batch=args.batch)
    model.load_state_dict(synthetic_state_dict(cfg, 0))
    model.to("cuda").eval()
    sep = Separator(model, device="cuda", shifts=1)
    n = int(args.block * SR)
    n_blocks = int(round(args.minutes * 60 / args.block))
    unique = max(1, min(n_blocks, int(round(args.unique / args.block))))
    floats = torch.from_numpy(synth_mix(1, unique * n, "tones")) * args.gain
    blocks = [floats[:, k * n:(k + 1) * n].contiguous() for k in range(unique)]

    def source():
        return (blocks[k % unique] for k in range(n_blocks))

    whole = torch.cat([blocks[k % unique] for k in range(n_blocks)], 1)        # the mix: only "minus" reads it, the call wants it
    routes = {
        "clamp": lambda: delivered(sep, source, Delivery(args.stem, clip="clamp"), 7),
        "rescale": lambda: delivered(sep, source, Delivery(args.stem, clip="rescale", peaks="measure"), 7),
        "floats": lambda: through_floats(sep, source, whole, args.stem, 7),
    }
    short = n_blocks

    def warm():
        nonlocal n_blocks
        n_blocks = min(short, max(2, int(60 / args.block)))                   # a minute of it: code objects, allocator pools
        for run in routes.values():
            run()
        n_blocks = short

    warm()
    times = {k: [] for k in routes}
    to_host, equal = {}, True
    order = list(routes)
    for r in range(args.rounds):
        got = {}
        for kind in order[r % 3:] + order[:r % 3]:
            ms, frames, n_bytes = routes[kind]()
            times[kind].append(ms)
            to_host[kind] = n_bytes
            got[kind] = frames
        equal = equal and all(torch.equal(got["rescale"][k], got["floats"][k]) for k in got["floats"])
        del got
    med = {k: statistics.median(v) for k, v in times.items()}
    seconds = n_blocks * n / SR
    result = {
        "what": "one synthetic stereo track through Separator.separate_blocks from host float blocks, HTDemucs float32 engine with "
                "random-init weights, shifts=1: Delivery(clip='clamp') (two passes), Delivery(clip='rescale', peaks='measure') "
                "(three passes), and float stems to the host followed by audio.deliver(clip='rescale'); host clock from the first "
                "read of the source to the last frame on the host, rotating order after one warm-up of each",
        "device": torch.cuda.get_device_name(0), "track_minutes": round(seconds / 60, 3), "block_seconds": args.block,
        "pushes_per_pass": n_blocks, "rounds": args.rounds, "stem": args.stem, "max_batch": args.batch,
        "ms": {k: [round(x, 1) for x in v] for k, v in times.items()}, "ms_median": {k: round(v, 1) for k, v in med.items()},
        "track_seconds_per_second": {k: round(seconds / (v * 1e-3), 1) for k, v in med.items()},
        "rescale_over_clamp": round(med["rescale"] / med["clamp"], 3), "rescale_over_floats": round(med["rescale"] / med["floats"], 3),
        "bytes_to_host": to_host, "rescale_equals_floats_bit_for_bit": bool(equal),
    }
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    if not equal:
        raise SystemExit("the three-pass frames differ from audio.deliver's on the float stems")


if __name__ == "__main__":
    main()
