"""Streaming separation (`apply_model_stream`, demucs_amd/stream.py): real-time factor and per-push wall time.

Seeded synthetic audio on the host (`demucs_amd.synth`), synthetic weights, htdemucs f32 and bf16, shifts=1, max_batch=8.  For
0.1 / 1 / 10 s blocks a `--seconds` stream is pushed from the host; every push returns host stems, so each push's wall time
(host clock) ends in a device synchronise.  Real-time factor = audio seconds / wall seconds over the whole stream, `finish()`
included; one warm-up stream runs first.  Then a 20-minute stream of 1 s blocks reports the peak `torch.cuda.max_memory_allocated`
(after the first minute, and at the end) against the size of the whole track's stems.
`--sr RATE` pushes the same audio duration as stereo blocks at RATE through the converting stream
(`Separator.separate_stream(sr=RATE, convert=True)`: the streaming `convert_audio` in front of the same model stream).
Prints ONE JSON line (and writes it to --out when given).

    python tools/bench_stream.py --out profiles/stream_bench.json
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

from demucs_amd.apply import apply_model_stream  # noqa: E402
from demucs_amd.htdemucs import HTDemucs  # noqa: E402
from demucs_amd.synth import synth_mix  # noqa: E402
from demucs_amd.weights import HTDemucsConfig, synthetic_state_dict  # noqa: E402

SR = 44100


def model(mode: str) -> HTDemucs:
    m = HTDemucs(HTDemucsConfig().sources, max_batch=8, compute_dtype=mode)
    m.load_state_dict(synthetic_state_dict(HTDemucsConfig(), 0))
    return m.to("cuda").eval()


def open_stream(m, sr: int):
    if sr == SR:
        return apply_model_stream(m, shifts=1, device="cuda")
    from demucs_amd.api import Separator
    return Separator(m, device="cuda", shifts=1).separate_stream(sr=sr, convert=True)


def run_stream(m, audio: torch.Tensor, block: int, sr: int = SR):
    from demucs_amd import _lib
    lib = _lib.load()
    real, calls = lib.mi_model_forward, [0]

    def counting(*args):
        calls[0] += 1
        return real(*args)

    lib.mi_model_forward = counting
    try:
        st = open_stream(m, sr)
        times, forwards = [], []
        t_all = time.perf_counter()
        for pos in range(0, audio.shape[1], block):
            before = calls[0]
            t0 = time.perf_counter()
            st.push(audio[:, pos:pos + block])
            times.append(time.perf_counter() - t0)
            forwards.append(calls[0] > before)
        st.finish()
        wall = time.perf_counter() - t_all
    finally:
        lib.mi_model_forward = real
    run_stream.forwards = forwards
    return wall, times


def _median_ms(values):
    return round(1e3 * statistics.median(values), 3) if values else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=120.0)
    ap.add_argument("--memory-minutes", type=float, default=20.0)
    ap.add_argument("--sr", type=int, default=SR, help="sample rate of the pushed blocks (converted on the stream when not 44100)")
    ap.add_argument("--blocks", default="0.1,1,10")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sr = args.sr
    audio = torch.from_numpy(synth_mix(1, int(args.seconds * sr), "tones"))
    result = {"what": "apply_model_stream htdemucs, shifts=1, host blocks", "device": torch.cuda.get_device_name(0),
              "stream_seconds": args.seconds, "input_sr": sr, "runs": {}}
    for mode in ("f32", "bf16"):
        m = model(mode)
        run_stream(m, audio[:, :20 * sr], sr, sr)               # warm-up: handles, workspaces, allocator
        for block_s in (float(x) for x in args.blocks.split(",")):
            wall, times = run_stream(m, audio, int(block_s * sr), sr)
            result["runs"][f"{mode}_block{block_s:g}s"] = {
                "realtime_factor": round(args.seconds / wall, 1),
                "push_ms_median": round(1e3 * statistics.median(times), 3),
                "push_ms_max": round(1e3 * max(times), 3),
                "push_ms_median_with_forward": _median_ms([t for t, f in zip(times, run_stream.forwards) if f]),
                "push_ms_median_without_forward": _median_ms([t for t, f in zip(times, run_stream.forwards) if not f]),
                "pushes": len(times),
            }
            print(mode, block_s, result["runs"][f"{mode}_block{block_s:g}s"], file=sys.stderr)
    # bounded memory: a long stream of 1 s blocks
    m = model("f32")
    st = open_stream(m, sr)
    block = torch.from_numpy(synth_mix(2, sr, "noise"))
    n = int(args.memory_minutes * 60)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    peak_1min = None
    for sec in range(n):
        st.push(block)
        if sec + 1 == 60:
            torch.cuda.synchronize()
            peak_1min = torch.cuda.max_memory_allocated()
    st.finish()
    torch.cuda.synchronize()
    result["memory"] = {
        "minutes": args.memory_minutes,
        "peak_allocated_after_1min_MiB": round(peak_1min / 2 ** 20, 2) if peak_1min is not None else None,
        "peak_allocated_end_MiB": round(torch.cuda.max_memory_allocated() / 2 ** 20, 2),
        "whole_track_stems_MiB": round(n * SR * 4 * 2 * 4 / 2 ** 20, 1),
        "stream_device_bytes_end": st.device_bytes(),
    }
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
