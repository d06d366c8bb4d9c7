"""nSDR scoring on the device (`mi_sdr`, demucs_amd/csrc/score.hip) against the host route it replaces: copy the stems to the host,
then the float64 formula of demucs/evaluate.py:30-43 on the CPU.

Part 1, the kernel.  A `--minutes` 4-stem stereo pair of references and estimates (seeded noise) lies on the device.  `mi_sdr` is
timed by device events (its memset, update and two finish launches) and gives bytes per second over the 2 x S x C x L x 4 bytes it
reads; the host route is timed in its two pieces: the D2H copy of the stems into a pinned tensor (`_to_host`, what
`separate_tensor` does for a host input) and into a pageable one (`.cpu()`), and `new_sdr` on `.double()` host tensors with
`--threads` CPU threads, as `eval_track` does.

Part 2, end to end.  One HTDemucs (synthetic weights, float32 mode) and one `--minutes` track in `--block` second host blocks, with
host reference blocks: `Separator.evaluate_blocks` against `separate_blocks` + concatenation on the host + the CPU formula, and
`separate_blocks` alone with its stems left on the device, all by a host clock around a final synchronise; `random` is seeded
per round, so every route of a round draws the same shift and the two scores can be compared.

Every pair runs `--rounds` times in alternating order after one warm-up each; every value is listed, with its median.
Prints ONE JSON line and writes it to --out.

    python tools/bench_score.py --out profiles/score_bench.json
"""
from __future__ import annotations

import argparse
import ctypes as C
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

from demucs_amd import _lib, audio  # noqa: E402
from demucs_amd.api import Separator  # noqa: E402
from demucs_amd.apply import _to_host  # noqa: E402
from demucs_amd.htdemucs import HTDemucs  # noqa: E402
from demucs_amd.synth import synth_mix  # noqa: E402
from demucs_amd.weights import HTDemucsConfig, synthetic_state_dict  # noqa: E402

SR = 44100


def host_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def device_sdr(ref, est, bufs):
    """(ms of mi_sdr by device events, (1, S, 2) sums on the device)."""
    state, scratch, sums = bufs
    _, S, ch, L = ref.shape
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    _lib.check(_lib.load().mi_sdr(ref.data_ptr(), est.data_ptr(), 1, S, ch, L, state.data_ptr(), scratch.data_ptr(), sums.data_ptr(),
                                  C.c_void_p(_lib.current_stream_ptr())), "mi_sdr")
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1), sums


def cpu_formula(ref, est):
    """evaluate.py:30-43 on float64 host tensors, as eval_track calls it."""
    ref, est = ref.double(), est.double()
    num = torch.sum(torch.square(ref), dim=(2, 3)) + 1e-7
    den = torch.sum(torch.square(ref - est), dim=(2, 3)) + 1e-7
    return 10 * torch.log10(num / den)


def spread(values, digits=3):
    return {"all": [round(v, digits) for v in values], "median": round(statistics.median(values), digits),
            "min": round(min(values), digits), "max": round(max(values), digits)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--minutes", type=float, default=3.0)
    ap.add_argument("--block", type=float, default=10.0, help="seconds per block of the end-to-end part")
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "score_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_score.py measures on the GPU and none is available")
    torch.set_num_threads(args.threads)
    lib = _lib.load()
    S, ch, L = 4, 2, int(args.minutes * 60 * SR)

    # ---- part 1: the kernel against D2H + the CPU formula ----------------------------------------------------------------------------
    g = torch.Generator(device="cuda").manual_seed(1)
    ref = torch.randn(1, S, ch, L, device="cuda", generator=g)
    est = ref + 0.3 * torch.randn(1, S, ch, L, device="cuda", generator=g)
    bufs = (torch.empty(lib.mi_sdr_state_bytes(S), dtype=torch.uint8, device="cuda"),
            torch.empty(lib.mi_sdr_scratch_bytes(S), dtype=torch.uint8, device="cuda"),
            torch.empty(1, S, 2, dtype=torch.float64, device="cuda"))
    ref_host = ref.cpu()
    device_sdr(ref, est, bufs)
    cpu_formula(ref_host, _to_host(est, est.device))
    est.cpu()
    kernel, pinned, pageable, formula = [], [], [], []
    for r in range(args.rounds):
        for kind in (("gpu", "cpu") if r % 2 == 0 else ("cpu", "gpu")):
            if kind == "gpu":
                ms, sums = device_sdr(ref, est, bufs)
                kernel.append(ms)
            else:
                ms, est_host = host_ms(lambda: _to_host(est, est.device))
                pinned.append(ms)
                pageable.append(host_ms(est.cpu)[0])
                ms, want = host_ms(lambda: cpu_formula(ref_host, est_host))
                formula.append(ms)
    got = audio._sdr_scores(sums)
    kernel_err = (got - want).abs().max().item()
    read_bytes = 2 * S * ch * L * 4
    kernel_ms = statistics.median(kernel)

    # ---- part 2: evaluate_blocks against separate_blocks + D2H + the CPU formula ------------------------------------------------------
    model = HTDemucs(HTDemucsConfig().sources, max_batch=4, compute_dtype="f32")
    model.load_state_dict(synthetic_state_dict(HTDemucsConfig(), 0))
    model = model.to("cuda").eval()
    sep = Separator(model, device="cuda", shifts=1)
    wav = torch.from_numpy(synth_mix(1, L, "tones"))
    gains = torch.tensor([0.4, 0.3, 0.2, 0.1])[:, None, None]
    refs = (gains * wav[None]).contiguous()
    n = int(args.block * SR)
    mix_blocks = [wav[:, i:i + n] for i in range(0, L, n)]
    ref_blocks = [refs[..., i:i + n] for i in range(0, L, n)]
    wav_dev = wav.cuda()
    dev_blocks = [b.cuda() for b in mix_blocks]

    def gpu_route():
        return sep.evaluate_blocks(lambda: iter(mix_blocks), lambda: iter(ref_blocks))

    def host_route():
        outs = list(sep.separate_blocks(lambda: iter(mix_blocks)))               # host blocks: the stems come back on the host
        stems = torch.stack([torch.cat([o[k] for o in outs], -1) for k in model.sources])
        return cpu_formula(refs[None], stems[None])[0]

    def separation_only():
        return [None for _ in sep.separate_blocks(lambda: iter(dev_blocks))]

    def whole_track():
        return sep.separate_tensor(wav_dev)

    for fn in (gpu_route, host_route, separation_only, whole_track):
        fn()
    e2e = {"evaluate_blocks": [], "separate_blocks_d2h_cpu_formula": [], "separate_blocks_alone": [], "separate_tensor_device": []}
    routes = list(zip(e2e, (gpu_route, host_route, separation_only, whole_track)))
    for r in range(args.rounds):
        for name, fn in (routes if r % 2 == 0 else routes[::-1]):
            random.seed(r)                                   # shifts=1 draws the shift from `random`: the same one for every route
            ms, out = host_ms(fn)
            e2e[name].append(ms)
            if name == "evaluate_blocks":
                score = out
            elif name.startswith("separate_blocks_d2h"):
                host_scores = out
    e2e_err = float((torch.tensor(score.nsdr) - host_scores).abs().max())
    med = {k: statistics.median(v) for k, v in e2e.items()}
    host_scoring_ms = statistics.median(pinned) + statistics.median(formula)

    result = {
        "what": "nSDR scoring of a 4-stem stereo pair resident on the device by mi_sdr (device events) against the host route: D2H of "
                "the stems (pinned and pageable) and new_sdr on .double() host tensors; then Separator.evaluate_blocks against "
                "separate_blocks + concatenation + the CPU formula on one HTDemucs (float32 mode, synthetic weights) and one track of "
                "host blocks with host reference blocks (host clock around a final synchronise); alternating order",
        "device": torch.cuda.get_device_name(0), "minutes": args.minutes, "sources": S, "channels": ch, "length": L,
        "cpu_threads": args.threads, "rounds": args.rounds, "block_seconds": args.block,
        "stems_bytes": S * ch * L * 4, "mi_sdr_read_bytes": read_bytes, "mi_sdr_state_bytes": lib.mi_sdr_state_bytes(S),
        "mi_sdr_ms": spread(kernel, 4), "mi_sdr_tb_per_s": round(read_bytes / (kernel_ms * 1e-3) / 1e12, 3),
        "mi_sdr_fraction_of_8_tb_per_s": round(read_bytes / (kernel_ms * 1e-3) / 8e12, 3),
        "d2h_stems_pinned_ms": spread(pinned), "d2h_stems_pageable_ms": spread(pageable), "cpu_float64_formula_ms": spread(formula),
        "host_scoring_ms_median": round(host_scoring_ms, 3),
        "host_scoring_over_mi_sdr": round(host_scoring_ms / kernel_ms, 1),
        "max_abs_db_kernel_vs_cpu": kernel_err,
        "end_to_end_ms": {k: spread(v) for k, v in e2e.items()},
        "host_scoring_over_separate_tensor": round(host_scoring_ms / med["separate_tensor_device"], 3),
        "evaluate_blocks_over_host_route": round(med["evaluate_blocks"] / med["separate_blocks_d2h_cpu_formula"], 3),
        "gpu_route_faster_end_to_end": bool(med["evaluate_blocks"] < med["separate_blocks_d2h_cpu_formula"]),
        "max_abs_db_evaluate_blocks_vs_host_route": e2e_err,
    }
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
