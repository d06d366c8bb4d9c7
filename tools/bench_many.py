"""Many tracks of different lengths: the sequential `apply_model` loop against `apply_model_many` (demucs_amd/packed.py).

Seeded synthetic clips (`demucs_amd.synth`) on the host, synthetic weights.  Each timing is a host clock around work that ends
in a device synchronise; the figure is the median of `--runs` runs after one warm-up run of each route.  Workloads:
  (a) 64 clips of 5-40 s, htdemucs f32 and bf16, max_batch=32, shifts=0;
  (b) the same clips, shifts=1;
  (c) 8 tracks of 60-120 s, hdemucs_mmi f16, max_batch=5, segment=44 (BagOfModels, as remote/hdemucs_mmi.yaml).
Also the f32 and bf16 forward times at B = 1 and B = 32 (HIP events), which bound what packing can gain.
Prints ONE JSON line (and writes it to --out when given).

    python tools/bench_many.py --out profiles/many_tracks_bench.json
"""
from __future__ import annotations

import argparse
import json
import os
import random
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

from demucs_amd import packed as K  # noqa: E402
from demucs_amd.apply import BagOfModels, apply_model, apply_model_many  # noqa: E402
from demucs_amd.synth import synth_mix  # noqa: E402

SR = 44100


def clips(n, lo_s, hi_s, seed):
    rng = random.Random(seed)
    lengths = [int(rng.uniform(lo_s, hi_s) * SR) for _ in range(n)]
    return [torch.from_numpy(synth_mix(seed * 1000 + i, L, "tones" if i % 2 else "noise")) for i, L in enumerate(lengths)]


def timed(fn, dev, runs):
    fn()
    torch.cuda.synchronize(dev)
    times = []
    for _ in range(runs):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize(dev)
        times.append(time.perf_counter() - t0)
    return sorted(times)[len(times) // 2]


def compare(model, mixes, dev, runs, **kw):
    seq = timed(lambda: [apply_model(model, m[None], device=dev, **kw)[0] for m in mixes], dev, runs)
    many = timed(lambda: apply_model_many(model, mixes, device=dev, **kw), dev, runs)
    random.seed(0)
    p = K.plan(model, [m.shape[-1] for m in mixes], shifts=kw.get("shifts", 1))
    audio = sum(m.shape[-1] for m in mixes) / SR
    members = model.models if isinstance(model, BagOfModels) else [model]
    seq_fw = sum(sequential_forwards(members[ps.member], ps) for ps in p.passes)
    return {"tracks": len(mixes), "audio_s": round(audio, 1), "sequential_s": round(seq, 4), "many_s": round(many, 4),
            "speedup": round(seq / many, 3), "segments": len(p.units), "packed_forwards": p.n_forwards,
            "sequential_forwards": seq_fw}


def sequential_forwards(sub, ps) -> int:
    """Forwards the sequential loop spends on one pass: HTDemucs batches the pass's segments by `max_batch`; HDemucs batches
    runs of equal chunk length (apply.ragged_split_accumulate), so every tail length is a forward of its own."""
    if not hasattr(sub, "side_stream"):
        return -(-len(ps.offsets) // sub.max_batch)
    n, i = 0, 0
    while i < len(ps.lens):
        j = i + 1
        while j < len(ps.lens) and j - i < sub.max_batch and ps.lens[j] == ps.lens[i]:
            j += 1
        n, i = n + 1, j
    return n


def forward_ms(model, dev, B, reps=5):
    x = torch.randn(B, 2, model.segment_length, device=dev)
    model.forward_segments(x)
    torch.cuda.synchronize(dev)
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        model.forward_segments(x)
    t1.record()
    t1.synchronize()
    return round(t0.elapsed_time(t1) / reps, 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--workloads", default="a,b,c")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from demucs_amd.hdemucs import HDemucs
    from demucs_amd.hdemucs_weights import HDemucsConfig, synthetic_hdemucs_state_dict
    from demucs_amd.htdemucs import HTDemucs
    from demucs_amd.weights import HTDemucsConfig, synthetic_state_dict
    dev = torch.device("cuda", 0)
    todo = set(args.workloads.split(","))
    result = {"tool": "tools/bench_many.py", "timing": f"host clock to a device synchronise, median of {args.runs} after a warm-up",
              "device": torch.cuda.get_device_name(dev)}
    mixes = clips(64, 5, 40, 1)
    if todo & {"a", "b"}:
        cfg = HTDemucsConfig()
        sd = synthetic_state_dict(cfg, 0)
        for dt in ("f32", "bf16"):
            m = HTDemucs(cfg.sources, max_batch=32, compute_dtype=dt)
            m.load_state_dict(sd)
            m.to(dev).eval()
            result[f"forward_ms_{dt}"] = {"B1": forward_ms(m, dev, 1), "B32": forward_ms(m, dev, 32)}
            for w, shifts in (("a", 0), ("b", 1)):
                if w in todo:
                    result[f"{w}_htdemucs_{dt}"] = compare(m, mixes, dev, args.runs, shifts=shifts, overlap=0.25)
                    print(json.dumps({w + "_" + dt: result[f"{w}_htdemucs_{dt}"]}), file=sys.stderr, flush=True)
            m.release()
            del m
    if "c" in todo:
        hcfg = HDemucsConfig()
        hm = HDemucs(hcfg.sources, max_batch=5, compute_dtype="f16")
        hm.load_state_dict(synthetic_hdemucs_state_dict(hcfg, 0))
        hm.to(dev).eval()
        hbag = BagOfModels([hm], segment=44)
        long = clips(8, 60, 120, 2)
        result["c_hdemucs_mmi_f16"] = compare(hbag, long, dev, args.runs, shifts=0, overlap=0.25)
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
