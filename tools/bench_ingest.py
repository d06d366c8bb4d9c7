"""Wire PCM into a stream (`apply_model_stream(pcm="i16")`, demucs_amd/csrc/ingest.hip) against the float push: per-push time and
the bytes a push sends to the device.

Seeded synthetic audio on the host (`demucs_amd.synth`), synthetic weights, htdemucs f32, shifts=1, max_batch=8, as
`tools/bench_stream.py`.  A `--seconds` stereo stream is pushed from the host in 0.1 s and 1 s blocks, once as planar float32
blocks and once as the same samples' interleaved int16 bytes, `--rounds` times in alternating order (float first, then int16
first, ...), one warm-up stream first.  A push is timed with device events around it (every push returns host stems, so it ends
in a device synchronise) and reported as the median over the stream's pushes, per round, with and without a forward.  The bytes
are not a measurement: a solo float push stages 8 n bytes for n stereo frames and an int16 push 4 n; the group-of-one figures are
the sizes of the pinned upload (`_GroupEngineExec.last_upload`: the call's table, then the block).
Prints ONE JSON line (and writes it to --out when given).

    python tools/bench_ingest.py --out profiles/ingest_bench.json
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

from demucs_amd import _lib  # noqa: E402
from demucs_amd.apply import apply_model_stream  # noqa: E402
from demucs_amd.htdemucs import HTDemucs  # noqa: E402
from demucs_amd.stream import StreamGroup  # noqa: E402
from demucs_amd.synth import synth_mix  # noqa: E402
from demucs_amd.weights import HTDemucsConfig, synthetic_state_dict  # noqa: E402

SR = 44100


def model() -> HTDemucs:
    m = HTDemucs(HTDemucsConfig().sources, max_batch=8, compute_dtype="f32")
    m.load_state_dict(synthetic_state_dict(HTDemucsConfig(), 0))
    return m.to("cuda").eval()


def blocks_of(floats: torch.Tensor, frames: torch.Tensor, kind: str, block: int):
    if kind == "f32":
        return [floats[:, pos:pos + block] for pos in range(0, floats.shape[1], block)]
    data = frames.numpy().tobytes()
    return [data[4 * pos:4 * (pos + block)] for pos in range(0, frames.shape[0], block)]


def run_stream(m, blocks, kind: str):
    """ms per push by device events, and which pushes ran a forward."""
    lib = _lib.load()
    real, calls = lib.mi_model_forward, [0]

    def counting(*args):
        calls[0] += 1
        return real(*args)

    lib.mi_model_forward = counting
    try:
        st = apply_model_stream(m, shifts=1, device="cuda", pcm="i16" if kind == "i16" else None)
        events, forwards = [], []
        for b in blocks:
            before = calls[0]
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            st.push(b)
            t1.record()
            events.append((t0, t1))
            forwards.append(calls[0] > before)
        st.finish()
        torch.cuda.synchronize()
    finally:
        lib.mi_model_forward = real
    return [a.elapsed_time(b) for a, b in events], forwards


def upload_bytes(m, block_f32, block_i16):
    """(table bytes, pinned upload bytes) of a group-of-one push, float and int16."""
    out = {}
    for kind, block in (("f32", block_f32), ("i16", block_i16)):
        g = StreamGroup(m, shifts=1, device="cuda")
        key = g.open(pcm="i16" if kind == "i16" else None)
        g.push({key: block})
        table, total = g._exec.last_upload
        out[kind] = {"table_bytes": table, "upload_bytes": total}
        g.push({key: block})
        g.finish([key])
    return out


def med(values):
    return round(statistics.median(values), 4) if values else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=60.0)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--blocks", default="0.1,1")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    floats = torch.from_numpy(synth_mix(1, int(args.seconds * SR), "tones"))
    frames = (floats * 32767.0).round().clamp(-32768, 32767).to(torch.int16).t().contiguous()
    floats = (frames.to(torch.float32) / 32768.0).t().contiguous()           # the values the int16 frames stand for
    m = model()
    result = {"what": "apply_model_stream htdemucs f32, shifts=1, host blocks: int16 PCM push against the float push, device events, "
                      "alternating order", "device": torch.cuda.get_device_name(0), "stream_seconds": args.seconds,
              "rounds": args.rounds, "runs": {}}
    run_stream(m, blocks_of(floats[:, :20 * SR], frames[:20 * SR], "f32", SR), "f32")       # warm-up: handles, workspaces, allocator
    run_stream(m, blocks_of(floats[:, :20 * SR], frames[:20 * SR], "i16", SR), "i16")
    for block_s in (float(x) for x in args.blocks.split(",")):
        n = int(block_s * SR)
        per = {"f32": [], "i16": []}
        for r in range(args.rounds):
            for kind in (("f32", "i16") if r % 2 == 0 else ("i16", "f32")):
                times, forwards = run_stream(m, blocks_of(floats, frames, kind, n), kind)
                per[kind].append({"push_ms_median": med(times),
                                  "push_ms_median_without_forward": med([t for t, f in zip(times, forwards) if not f]),
                                  "push_ms_median_with_forward": med([t for t, f in zip(times, forwards) if f]),
                                  "pushes": len(times)})
        entry = {"frames_per_push": n, "h2d_bytes_per_push": {"f32": 8 * n, "i16": 4 * n},
                 "group_of_one": upload_bytes(m, floats[:, :n].contiguous(), frames[:n].numpy().tobytes())}
        for kind in ("f32", "i16"):
            entry[kind] = {"rounds": per[kind],
                           "push_ms_median": med([p["push_ms_median"] for p in per[kind]]),
                           "push_ms_median_without_forward": med([p["push_ms_median_without_forward"] for p in per[kind]
                                                                  if p["push_ms_median_without_forward"] is not None])}
        result["runs"][f"block{block_s:g}s"] = entry
        print(block_s, {k: entry[k]["push_ms_median"] for k in ("f32", "i16")}, file=sys.stderr)
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
