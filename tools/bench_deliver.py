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

With `--mix-kernel` the pair is two launches on the same device data, `--seconds` (180 for the run of record) of 4 stereo float32
stems: `mi_deliver_pcm` with the four MI_DELIVER_ADD rows (every "no_STEM" output, clip "clamp", int16), and
`mi_deliver_mix_pcm` with the four rows of add-equivalent gains (1 on every stem but one, no mix), which write the same bytes.
Runs of `--reps` launches between two device events alternate (add, mix, add, mix, ...) `--pairs` times after a warm-up of each;
reported per entry: microseconds per launch of every run, their median and spread, and the bytes moved per second at the median.

    python tools/bench_deliver.py --mix-kernel --seconds 180 --out profiles/deliver_mix_kernel.json

With `--auto-kernel` the launches are `mi_deliver_mix_pcm` and `mi_deliver_mix_auto_pcm` on the same four remix rows (the mix and
two stems each, clip "clamp", int16) of the same device data, by the same method.  The automated rows carry ONE ramp each, to the
row's own gains, so both entries read the same terms and must write the same bytes, while every frame inside the ramp takes the
per-frame path: leg `auto` with a ramp of `--ramp-seconds` in the middle of the track (the blocks outside it run on uniform gains),
leg `auto_ramping` with a ramp over the whole track (every block on the per-frame path: the worst case).

    python tools/bench_deliver.py --auto-kernel --seconds 180 --out profiles/deliver_mix_auto_kernel.json
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
    ap.add_argument("--mix-kernel", action="store_true", help="time mi_deliver_mix_pcm against mi_deliver_pcm's ADD rows")
    ap.add_argument("--auto-kernel", action="store_true", help="time mi_deliver_mix_auto_pcm against mi_deliver_mix_pcm on the same rows")
    ap.add_argument("--ramp-seconds", type=float, default=10.0, help="length of each row's ramp in the `auto` leg of --auto-kernel")
    ap.add_argument("--reps", type=int, default=20, help="launches per timed run of --mix-kernel / --auto-kernel")
    args = ap.parse_args()
    if args.mix_kernel:
        return mix_kernel_main(args)
    if args.auto_kernel:
        return auto_kernel_main(args)
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


def mix_kernel_main(args):
    import ctypes as C

    from demucs_amd import _lib, audio
    S, channels, n = 4, 2, int(args.seconds * SR)
    dev = torch.device("cuda", 0)
    stems = (torch.rand(S, channels, n, device=dev) * 2 - 1) * 0.4
    outputs = [(f"no_{k}", audio.DELIVER_ADD, k) for k in range(S)]
    offs, total = audio.deliver_layout(outputs, n, channels, "i16")
    clamp = audio.clip_code("clamp")
    add_rows = []
    for (_, kind, sel), off in zip(outputs, offs):
        add_rows += [stems.data_ptr(), 0, n, kind, sel, clamp, 0, 0, off]
    gains = [(name, (0.0,) + tuple(0.0 if k == sel else 1.0 for k in range(S))) for name, _, sel in outputs]
    mix_rows = audio.mix_rows(gains, stems.data_ptr(), n, 0, 0, None, clamp, 0, "i16", offs)
    tables = {"add": torch.tensor(add_rows, dtype=torch.int64).to(dev), "mix": torch.tensor(mix_rows, dtype=torch.int64).to(dev)}
    bufs = {k: torch.zeros(total, dtype=torch.uint8, device=dev) for k in tables}
    lib = _lib.load()
    entries = {"add": (lib.mi_deliver_pcm, "mi_deliver_pcm"), "mix": (lib.mi_deliver_mix_pcm, "mi_deliver_mix_pcm")}

    def timed(which: str, reps: int) -> float:
        entry, name = entries[which]
        stream = C.c_void_p(_lib.current_stream_ptr())
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(reps):
            _lib.check(entry(tables[which].data_ptr(), S, n, S, channels, None, 0, bufs[which].data_ptr(), total, stream), name)
        t1.record()
        t1.synchronize()
        return 1e3 * t0.elapsed_time(t1) / reps                          # microseconds per launch

    for which in entries:
        timed(which, 3)
    assert torch.equal(bufs["add"], bufs["mix"]), "the two entries must write the same bytes"
    runs = {"add": [], "mix": []}
    for _ in range(args.pairs):
        for which in ("add", "mix"):
            runs[which].append(timed(which, args.reps))
    moved = (S - 1) * S * channels * n * 4 + S * channels * n * 2           # bytes read and written by a launch
    result = {"what": f"{args.seconds:g} s of {S} stereo stems: mi_deliver_pcm's {S} ADD rows vs mi_deliver_mix_pcm with add-equivalent "
                      "gains, clamp, int16; alternating runs",
              "device": torch.cuda.get_device_name(0), "reps": args.reps, "pairs": args.pairs, "bytes_per_launch": moved}
    for which, us in runs.items():
        med = statistics.median(us)
        result[which] = {"us_per_launch_runs": [round(x, 1) for x in us], "us_median": round(med, 1),
                         "us_spread": round(max(us) - min(us), 1), "gb_per_s": round(moved / med / 1e3, 1)}
    result["mix_over_add"] = round(result["mix"]["us_median"] / result["add"]["us_median"], 3)
    result["within_add_spread"] = result["mix"]["us_median"] <= result["add"]["us_median"] + result["add"]["us_spread"]
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


def auto_kernel_main(args):
    import ctypes as C

    from demucs_amd import _lib, audio
    S, channels, n = 4, 2, int(args.seconds * SR)
    dev = torch.device("cuda", 0)
    stems = (torch.rand(S, channels, n, device=dev) * 2 - 1) * 0.4
    origin = (torch.rand(channels, n, device=dev) * 2 - 1) * 0.4
    # the mix and two stems per remix: "STEM lowered", as a practice feed asks for
    gains = [(f"practice_{k}", (1.0,) + tuple(-0.75 if j == k else 0.5 if j == (k + 1) % S else 0.0 for j in range(S))) for k in range(S)]
    offs, total = audio.deliver_layout(audio.mix_outputs(gains), n, channels, "i16")
    clamp = audio.clip_code("clamp")
    rows = audio.mix_rows(gains, stems.data_ptr(), n, origin.data_ptr(), n, None, clamp, 0, "i16", offs)
    ramp = min(n, int(args.ramp_seconds * SR))
    words = {"mix": rows,
             "auto": audio.auto_table(rows, [0] * S, [[((n - ramp) // 2 + 1000 * k, ramp - 1000 * S, g)] for k, (_, g) in enumerate(gains)]),
             "auto_ramping": audio.auto_table(rows, [0] * S, [[(-1 - k, n + 2 + k, g)] for k, (_, g) in enumerate(gains)])}
    tables = {k: torch.tensor(v, dtype=torch.int64).to(dev) for k, v in words.items()}
    bufs = {k: torch.zeros(total, dtype=torch.uint8, device=dev) for k in tables}
    lib = _lib.load()

    def timed(which: str, reps: int) -> float:
        stream = C.c_void_p(_lib.current_stream_ptr())
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(reps):
            if which == "mix":
                _lib.check(lib.mi_deliver_mix_pcm(tables[which].data_ptr(), S, n, S, channels, None, 0, bufs[which].data_ptr(), total,
                                                  stream), "mi_deliver_mix_pcm")
            else:
                _lib.check(lib.mi_deliver_mix_auto_pcm(tables[which].data_ptr(), len(words[which]), S, n, S, channels, None, 0,
                                                       bufs[which].data_ptr(), total, stream), "mi_deliver_mix_auto_pcm")
        t1.record()
        t1.synchronize()
        return 1e3 * t0.elapsed_time(t1) / reps                          # microseconds per launch

    for which in tables:
        timed(which, 3)
    for which in ("auto", "auto_ramping"):
        assert torch.equal(bufs["mix"], bufs[which]), f"{which}: a ramp to the row's own gains must write the fixed gains' bytes"
    assert int(bufs["mix"].count_nonzero()) > total // 2
    runs = {k: [] for k in tables}
    for _ in range(args.pairs):
        for which in tables:
            runs[which].append(timed(which, args.reps))
    moved = S * 3 * channels * n * 4 + S * channels * n * 2                 # bytes read (three terms a row) and written by a launch
    result = {"what": f"{args.seconds:g} s of {S} stereo stems and the mix: mi_deliver_mix_pcm vs mi_deliver_mix_auto_pcm on the same "
                      f"{S} rows of three terms, clamp, int16; one ramp per automated row ({ramp / SR:g} s, or the whole track); "
                      "alternating runs",
              "device": torch.cuda.get_device_name(0), "reps": args.reps, "pairs": args.pairs, "bytes_per_launch": moved}
    for which, us in runs.items():
        med = statistics.median(us)
        result[which] = {"us_per_launch_runs": [round(x, 1) for x in us], "us_median": round(med, 1),
                         "us_spread": round(max(us) - min(us), 1), "gb_per_s": round(moved / med / 1e3, 1)}
    for which in ("auto", "auto_ramping"):
        result[f"{which}_over_mix"] = round(result[which]["us_median"] / result["mix"]["us_median"], 3)
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
