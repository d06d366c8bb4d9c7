"""The analysis pass of a stream (`audio.MonoStatsStream`, demucs_amd/csrc/stats_stream.hip) against one `mi_mono_stats` call on
the same track.

A `--minutes` stereo int16 feed (seeded synthetic audio, `--unique` seconds of it repeated) is pushed from the host in `--block`
second blocks of wire bytes: per push one pinned staging copy, one H2D and one `mi_mono_stats_update` launch; `finish()` ends in
a device synchronise, so the pass is timed with a host clock around all of it.  The one-shot figure is `mi_mono_stats` on the
whole track, already planar float32 on the device (what `separate_tensor` has after its one H2D), by device events; it leaves out
the copy that puts the track there, which the stream exists to avoid.  Both run `--rounds` times in alternating order after one
warm-up each, and the two results are compared bit for bit.  No model is involved.
Prints ONE JSON line and writes it to --out.

    python tools/bench_analyse.py --out profiles/analyse_bench.json
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from demucs_amd import _lib, audio  # noqa: E402
from demucs_amd.synth import synth_mix  # noqa: E402

SR = 44100


def analysis_pass(blocks, n_blocks: int):
    """(ms of the whole pass, TrackStats): `n_blocks` pushes of the host byte blocks in turn, then finish()."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    st = audio.MonoStatsStream(2, pcm="i16", src_channels=2)
    for k in range(n_blocks):
        st.push(blocks[k % len(blocks)])
    stats = st.finish()
    return (time.perf_counter() - t0) * 1e3, stats


def one_shot(track: torch.Tensor):
    """(ms of mi_mono_stats by device events, (mean, s))."""
    lib = _lib.load()
    scratch = torch.empty(lib.mi_mono_stats_scratch_bytes(), dtype=torch.uint8, device="cuda")
    stats = torch.empty(2, dtype=torch.float32, device="cuda")
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    _lib.check(lib.mi_mono_stats(track.data_ptr(), track.shape[0], track.shape[1], scratch.data_ptr(), stats.data_ptr(),
                                 C.c_void_p(_lib.current_stream_ptr())), "mi_mono_stats")
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1), tuple(stats.cpu().tolist())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--minutes", type=float, default=60.0)
    ap.add_argument("--block", type=float, default=1.0, help="seconds per push")
    ap.add_argument("--unique", type=int, default=60, help="seconds of distinct audio, repeated to the feed's length")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "analyse_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_analyse.py measures on the GPU and none is available")
    n = int(args.block * SR)
    n_blocks = int(round(args.minutes * 60 / args.block))
    unique = max(1, min(n_blocks, int(round(args.unique / args.block))))
    floats = torch.from_numpy(synth_mix(1, unique * n, "tones"))
    frames = (floats * 32767.0).round().clamp(-32768, 32767).to(torch.int16).t().contiguous()
    blocks = [frames[k * n:(k + 1) * n].numpy().tobytes() for k in range(unique)]
    # the same track whole, planar float32 on the device: the distinct part decoded once, then repeated there
    part = audio.pcm_to_tensor(frames.numpy().tobytes(), "i16", 2)
    reps, rest = divmod(n_blocks, unique)
    track = torch.cat([part.repeat(1, reps), part[:, :rest * n]], 1).contiguous()
    assert track.shape == (2, n_blocks * n)

    analysis_pass(blocks, min(n_blocks, 200))            # warm-up: code objects, pinned and device allocator pools
    one_shot(track)
    passes, shots, equal = [], [], True
    for r in range(args.rounds):
        for kind in (("stream", "one") if r % 2 == 0 else ("one", "stream")):
            if kind == "stream":
                ms, stats = analysis_pass(blocks, n_blocks)
                passes.append(ms)
            else:
                ms, want = one_shot(track)
                shots.append(ms)
        got = np.array([stats.mean, stats.s], np.float32).view(np.uint32)
        equal = equal and stats.length == track.shape[1] and np.array_equal(got, np.array(want, np.float32).view(np.uint32))
    pass_ms = statistics.median(passes)
    result = {
        "what": "analysis pass of a stereo int16 feed pushed from the host in blocks (MonoStatsStream: staging copy, H2D and one "
                "mi_mono_stats_update per push, host clock around the pass and its final synchronise) against one mi_mono_stats on "
                "the whole planar float32 track resident on the device (device events, no copy); alternating order",
        "device": torch.cuda.get_device_name(0), "feed_minutes": args.minutes, "block_seconds": args.block, "pushes": n_blocks,
        "frames_per_push": n, "h2d_bytes_per_push": 4 * n, "track_bytes_on_device_one_shot": track.numel() * 4,
        "stream_state_bytes": _lib.load().mi_mono_stats_state_bytes(), "rounds": args.rounds,
        "analysis_pass_ms": [round(v, 3) for v in passes], "analysis_pass_ms_median": round(pass_ms, 3),
        "per_push_us_median_round": round(pass_ms * 1e3 / n_blocks, 2),
        "feed_seconds_per_second": round(args.minutes * 60 / (pass_ms * 1e-3), 1),
        "one_shot_ms": [round(v, 4) for v in shots], "one_shot_ms_median": round(statistics.median(shots), 4),
        "bits_equal": bool(equal),
    }
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    if not equal:
        raise SystemExit("the streamed statistics differ from mi_mono_stats")


if __name__ == "__main__":
    main()
