"""Generate tests/golden/*.npz from the IMPORTED REFERENCE (build container only).

    python tools/make_golden.py            # writes tests/golden/

The reference (read-only at /root/reference) is imported with stand-ins for its non-hot-path
dependencies (tools/ref_import.py), given this repo's deterministic synthetic weights through
`load_state_dict`, and run on CPU in float32 and float64.  Only DATA is stored: input recipes
(seeds), and for every tap a strided sample plus sum / sum-of-squares.  No reference source is
copied.  The fixtures pin `oracle/` (tests/test_oracle_golden.py) and, on the GPU box, the HIP
path (tests/test_gpu_*.py) without /root/reference being present.
"""
import os
import random
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from demucs_amd.weights import HTDemucsConfig, synthetic_state_dict       # noqa: E402
from demucs_amd.synth import synth_mix                                    # noqa: E402
from ref_import import import_reference, build_reference_htdemucs         # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
SL = 343980


def sample(t: torch.Tensor, n_max: int = 2048):
    """strided sample + moments of a tensor (float64 moments)."""
    flat = t.detach().reshape(-1)
    stride = max(1, flat.numel() // n_max)
    d = flat.double()
    return dict(shape=np.array(t.shape), stride=np.array(stride), sample=flat[::stride].cpu().numpy().copy(),
                sum=np.array(d.sum().item()), sumsq=np.array((d * d).sum().item()))


def pack(prefix: str, s: dict, store: dict):
    for k, v in s.items():
        store[f"{prefix}/{k}"] = v


def segment_fixture(name: str, cfg: HTDemucsConfig, wseed: int, mix: np.ndarray):
    """One-segment forward of the reference with per-stage taps (forward hooks)."""
    store = {"meta/wseed": np.array(wseed), "meta/n_sources": np.array(len(cfg.sources))}
    sd = synthetic_state_dict(cfg, wseed)
    for tag, dtype in (("f32", torch.float32), ("f64", torch.float64)):
        model = build_reference_htdemucs(cfg, sd, dtype)
        taps = {}
        hooks = []

        def mk(nm, pick=None):
            def hook(mod, inp, out):
                taps[nm] = out if pick is None else out[pick]
            return hook
        for i in range(4):
            hooks.append(model.encoder[i].register_forward_hook(mk(f"enc{i}" if i else "enc0_preemb")))
            hooks.append(model.tencoder[i].register_forward_hook(mk(f"tenc{i}")))
            hooks.append(model.decoder[i].register_forward_hook(mk(f"dec{i}", 0)))
            hooks.append(model.tdecoder[i].register_forward_hook(mk(f"tdec{i}", 0)))
        for idx in range(5):
            hooks.append(model.crosstransformer.layers[idx].register_forward_hook(mk(f"tr{idx}_f")))
            hooks.append(model.crosstransformer.layers_t[idx].register_forward_hook(mk(f"tr{idx}_t")))
        hooks.append(model.channel_downsampler.register_forward_hook(mk("bott_f")))
        hooks.append(model.channel_downsampler_t.register_forward_hook(mk("bott_t")))
        x = torch.from_numpy(mix).to(dtype)[None]
        t0 = time.time()
        with torch.no_grad():
            out = model(x)
            xp = torch.nn.functional.pad(x, (0, SL - x.shape[-1]))       # htdemucs.py:535-537
            z = model._magnitude(model._spec(xp))
        print(f"  {name} {tag}: {time.time() - t0:.1f}s  out rms {out.pow(2).mean().sqrt():.4f}")
        for h in hooks:
            h.remove()
        taps["stft"] = z
        # transformer layer taps are (B, tokens, C) in the reference; store channel-first
        for k in list(taps):
            if k.startswith("tr"):
                taps[k] = taps[k].transpose(1, 2)
        taps["bott_f"] = taps["bott_f"].reshape(1, 384, 8, -1)
        taps["out"] = out
        for k, v in taps.items():
            pack(f"{tag}/{k}", sample(v, 16384 if k == "out" else 2048), store)
    np.savez_compressed(os.path.join(OUT, name + ".npz"), **store)


def apply_fixture(name: str, cfg: HTDemucsConfig, wseeds, bag_weights, mix: np.ndarray, rseed=None, **kw):
    """Track-level `apply_model` of the reference (float32 model; float64 model for truth)."""
    ref_apply, _ = import_reference()
    store = {"meta/wseeds": np.array(wseeds), "meta/length": np.array(mix.shape[-1])}
    for k, v in kw.items():
        store[f"meta/kw_{k}"] = np.array(v)
    if rseed is not None:
        store["meta/rseed"] = np.array(rseed)
    if bag_weights is not None:
        store["meta/bag_weights"] = np.array(bag_weights)
    for tag, dtype in (("f32", torch.float32), ("f64", torch.float64)):
        models = [build_reference_htdemucs(cfg, synthetic_state_dict(cfg, s), dtype) for s in wseeds]
        model = models[0] if bag_weights is None else ref_apply.BagOfModels(models, bag_weights)
        events = []
        if rseed is not None:
            random.seed(rseed)
        x = torch.from_numpy(mix).to(dtype)[None]
        x0 = x.clone()
        t0 = time.time()
        out = ref_apply.apply_model(model, x, callback=lambda d: events.append(dict(d)), **kw)
        assert torch.equal(x, x0), "apply_model must not mutate mix"
        print(f"  {name} {tag}: {time.time() - t0:.1f}s  {len(events)} events, out rms {out.pow(2).mean().sqrt():.4f}")
        pack(f"{tag}/out", sample(out, 16384), store)
        if tag == "f32":
            keys = ["model_idx_in_bag", "shift_idx", "segment_offset", "models", "state"]
            store["events"] = np.array([[str(e[k]) for k in keys] for e in events])
    np.savez_compressed(os.path.join(OUT, name + ".npz"), **store)


def separator_fixture(name: str, cfg: HTDemucsConfig, wseed: int, wav: np.ndarray, rseed: int, **params):
    """`demucs.api.Separator.separate_tensor` of the reference (api.py:241-291) around a reference HTDemucs carrying
    our synthetic weights.  The zoo loader (`get_model`: a network fetch) is bypassed by handing the instance its
    model directly; everything `separate_tensor` itself does -- in-place normalise by the mono mean / std, apply_model,
    de-normalise, restore `wav` -- is the reference's code.  sr = the model's rate (no resampling: julius is absent)."""
    import_reference()
    import demucs.api as ref_api
    store = {"meta/wseed": np.array(wseed), "meta/length": np.array(wav.shape[-1]), "meta/rseed": np.array(rseed)}
    for k, v in params.items():
        store[f"meta/kw_{k}"] = np.array(v)
    for tag, dtype in (("f32", torch.float32), ("f64", torch.float64)):
        sep = ref_api.Separator.__new__(ref_api.Separator)
        sep._model = build_reference_htdemucs(cfg, synthetic_state_dict(cfg, wseed), dtype)
        sep._audio_channels, sep._samplerate = sep._model.audio_channels, sep._model.samplerate
        events = []
        sep.update_parameter(device="cpu", jobs=0, progress=False, callback=lambda d: events.append(dict(d)),
                             callback_arg={"tag": "fixture"}, **params)
        x = torch.from_numpy(wav).to(dtype)
        x0 = x.clone()
        random.seed(rseed)
        t0 = time.time()
        got_wav, stems = sep.separate_tensor(x, sr=sep.samplerate)
        assert got_wav is x, "separate_tensor returns the caller's tensor"
        print(f"  {name} {tag}: {time.time() - t0:.1f}s  {len(events)} events, restore err {(x - x0).abs().max():.2e}")
        assert list(stems) == list(cfg.sources)
        pack(f"{tag}/out", sample(torch.stack([stems[k] for k in cfg.sources]), 16384), store)
        pack(f"{tag}/wav", sample(x, 4096), store)
        store[f"{tag}/restore_err"] = np.array((x - x0).abs().max().item())
        if tag == "f32":
            keys = ["model_idx_in_bag", "shift_idx", "segment_offset", "models", "state", "audio_length", "tag"]
            store["events"] = np.array([[str(e[k]) for k in keys] for e in events])
    np.savez_compressed(os.path.join(OUT, name + ".npz"), **store)


def autocast_fixture(name: str, cfg: HTDemucsConfig, wseed: int, mix: np.ndarray):
    """Noise floor for the engine's reduced-precision modes: the reference's own float32 model run under
    `torch.autocast("cpu", dtype=bfloat16 / float16)` (conv / linear / attention matmuls in the low-precision type,
    normalisations and the STFT in float32 by autocast's op lists), beside its float64 run of the same input."""
    store = {"meta/wseed": np.array(wseed), "meta/n_sources": np.array(len(cfg.sources))}
    sd = synthetic_state_dict(cfg, wseed)
    x = torch.from_numpy(mix)[None]
    runs = [("f64", torch.float64, None), ("bf16", torch.float32, torch.bfloat16), ("f16", torch.float32, torch.float16)]
    for tag, dtype, cast in runs:
        model = build_reference_htdemucs(cfg, sd, dtype)
        t0 = time.time()
        with torch.no_grad():
            if cast is None:
                out = model(x.to(dtype))
            else:
                with torch.autocast("cpu", dtype=cast):
                    out = model(x)
        out = out.double()
        print(f"  {name} {tag}: {time.time() - t0:.1f}s  out rms {out.pow(2).mean().sqrt():.4f}")
        if tag == "f64":
            truth = out
        else:
            err = out - truth
            store[f"{tag}/max_abs"] = np.array(err.abs().max().item())
            store[f"{tag}/sdr_db"] = np.array((10 * torch.log10((truth.pow(2).sum((2, 3)) + 1e-7) / (err.pow(2).sum((2, 3)) + 1e-7))).min().item())
            print(f"    vs f64: max-abs {store[tag + '/max_abs']:.3e}  min SDR {store[tag + '/sdr_db']:.1f} dB")
        pack(f"{tag}/out", sample(out, 16384), store)
    np.savez_compressed(os.path.join(OUT, name + ".npz"), **store)


def hsegment_fixture(name: str, hcfg, wseed: int, mix: np.ndarray):
    """One forward of the reference `HDemucs` (hdemucs_mmi architecture) with per-layer taps."""
    import_reference()
    from demucs.hdemucs import HDemucs as RefHDemucs
    from demucs_amd.hdemucs_weights import hdemucs_schema, synthetic_hdemucs_state_dict
    store = {"meta/wseed": np.array(wseed), "meta/n_sources": np.array(len(hcfg.sources)), "meta/length": np.array(mix.shape[-1])}
    sd = synthetic_hdemucs_state_dict(hcfg, wseed)
    for tag, dtype in (("f32", torch.float32), ("f64", torch.float64)):
        model = RefHDemucs(sources=list(hcfg.sources), channels=hcfg.channels)
        ref_schema = [(k, tuple(v.shape)) for k, v in model.state_dict().items()]
        assert ref_schema == list(hdemucs_schema(hcfg).items()), "hdemucs_schema differs from the reference's state_dict"
        model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()}, strict=True)
        model = model.eval().to(dtype)
        taps, hooks = {}, []

        def mk(nm, pick=None):
            def hook(mod, inp, out):
                taps[nm] = out if pick is None else out[pick]
            return hook
        for i in range(6):
            hooks.append(model.encoder[i].register_forward_hook(mk(f"enc{i}" if i else "enc0_preemb")))
            hooks.append(model.decoder[i].register_forward_hook(mk(f"dec{i}", 0)))
        for i in range(5):
            hooks.append(model.tencoder[i].register_forward_hook(mk(f"tenc{i}")))
            hooks.append(model.tdecoder[i].register_forward_hook(mk(f"tdec{i}", 0)))
        x = torch.from_numpy(mix).to(dtype)[None]
        t0 = time.time()
        with torch.no_grad():
            out = model(x)
        print(f"  {name} {tag}: {time.time() - t0:.1f}s  out rms {out.pow(2).mean().sqrt():.4f}  "
              + " ".join(f"{k}:{v.pow(2).mean().sqrt():.2f}" for k, v in taps.items() if k.startswith("enc") or k.startswith("dec")))
        for h in hooks:
            h.remove()
        taps["out"] = out
        for k, v in taps.items():
            pack(f"{tag}/{k}", sample(v, 16384 if k == "out" else 2048), store)
    np.savez_compressed(os.path.join(OUT, name + ".npz"), **store)


def happly_fixture(name: str, hcfg, wseed: int, mix: np.ndarray, **kw):
    """Track-level `apply_model` of the reference around its HDemucs (no valid_length: every chunk runs at its own length)."""
    ref_apply, _ = import_reference()
    from demucs.hdemucs import HDemucs as RefHDemucs
    from demucs_amd.hdemucs_weights import synthetic_hdemucs_state_dict
    store = {"meta/wseed": np.array(wseed), "meta/length": np.array(mix.shape[-1])}
    for k, v in kw.items():
        store[f"meta/kw_{k}"] = np.array(v)
    sd = synthetic_hdemucs_state_dict(hcfg, wseed)
    for tag, dtype in (("f32", torch.float32), ("f64", torch.float64)):
        model = RefHDemucs(sources=list(hcfg.sources))
        model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()}, strict=True)
        model = model.eval().to(dtype)
        events = []
        x = torch.from_numpy(mix).to(dtype)[None]
        t0 = time.time()
        out = ref_apply.apply_model(model, x, callback=lambda d: events.append(dict(d)), **kw)
        print(f"  {name} {tag}: {time.time() - t0:.1f}s  {len(events)} events, out rms {out.pow(2).mean().sqrt():.4f}")
        pack(f"{tag}/out", sample(out, 16384), store)
        if tag == "f32":
            keys = ["model_idx_in_bag", "shift_idx", "segment_offset", "models", "state"]
            store["events"] = np.array([[str(e[k]) for k in keys] for e in events])
    np.savez_compressed(os.path.join(OUT, name + ".npz"), **store)



def hautocast_fixture(name: str, hcfg, wseed: int, mix: np.ndarray):
    """`autocast_fixture` for the reference HDemucs: its float32 model under `torch.autocast("cpu", bf16 / fp16)` beside its
    float64 run -- the noise floor the engine's reduced-precision hdemucs modes are scored against (BASELINE configs[4])."""
    import_reference()
    from demucs.hdemucs import HDemucs as RefHDemucs
    from demucs_amd.hdemucs_weights import synthetic_hdemucs_state_dict
    store = {"meta/wseed": np.array(wseed), "meta/n_sources": np.array(len(hcfg.sources)), "meta/length": np.array(mix.shape[-1])}
    sd = synthetic_hdemucs_state_dict(hcfg, wseed)
    x = torch.from_numpy(mix)[None]
    for tag, dtype, cast in (("f64", torch.float64, None), ("bf16", torch.float32, torch.bfloat16), ("f16", torch.float32, torch.float16)):
        model = RefHDemucs(sources=list(hcfg.sources))
        model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()}, strict=True)
        model = model.eval().to(dtype)
        t0 = time.time()
        with torch.no_grad():
            if cast is None:
                out = model(x.to(dtype))
            else:
                with torch.autocast("cpu", dtype=cast):
                    out = model(x)
        out = out.double()
        print(f"  {name} {tag}: {time.time() - t0:.1f}s  out rms {out.pow(2).mean().sqrt():.4f}")
        if tag == "f64":
            truth = out
        else:
            err = out - truth
            store[f"{tag}/max_abs"] = np.array(err.abs().max().item())
            store[f"{tag}/sdr_db"] = np.array((10 * torch.log10((truth.pow(2).sum((2, 3)) + 1e-7) / (err.pow(2).sum((2, 3)) + 1e-7))).min().item())
            print(f"    vs f64: max-abs {store[tag + '/max_abs']:.3e}  min SDR {store[tag + '/sdr_db']:.1f} dB")
        pack(f"{tag}/out", sample(out, 16384), store)
    np.savez_compressed(os.path.join(OUT, name + ".npz"), **store)


PACKAGE_PERIOD = 509          # weights repeat with this period (a prime): the package deflates ~200:1 (see periodic_uniform)


def _reference_config(section: str) -> dict:
    """Every keyword of one model section of the reference's conf/config.yaml (htdemucs: lines 195-271, hdemucs: 126-165)."""
    import yaml
    with open("/root/reference/conf/config.yaml") as f:
        raw = dict(yaml.safe_load(f)[section])

    def number(v):          # PyYAML reads `1e-3` (no dot) as a string; the reference's loader (omegaconf) reads a float
        try:
            return float(v) if isinstance(v, str) else v
        except ValueError:
            return v
    return {k: number(v) for k, v in raw.items()}


def package_fixture(name: str, kind: str, wseed: int, mix: np.ndarray):
    """A checkpoint PACKAGE written by the reference's own code: the reference model is built with EVERY
    keyword of its conf/config.yaml section passed explicitly (plus what demucs/train.py:38-60 adds and, for htdemucs, the
    released-model overrides of grids/mmi.py), `demucs.states.serialize_model` (klass, args / kwargs from
    `_init_args_kwargs`, `get_state(half=True)`) assembles it and `torch.save` writes it.  The zip members are then
    re-stored deflated (same member bytes; `torch.load` reads either) so that the 84 / 167 MB file takes ~1 MB here.  Beside
    it: forward samples of that reference model after `set_state` from the package (the half-rounded weights)."""
    import zipfile
    from fractions import Fraction
    import_reference()
    import demucs.states as ref_states
    ref_states.OmegaConf = type("OmegaConf", (), {"to_container": staticmethod(lambda a, resolve=True: dict(a))})   # omegaconf is absent
    if kind == "htdemucs":
        from demucs.htdemucs import HTDemucs as Klass
        cfg = HTDemucsConfig()
        kwargs = _reference_config("htdemucs")
        kwargs.update(dconv_mode=3, bottom_channels=512, t_dropout=0.02)                     # demucs/grids/mmi.py:15-30
        kwargs.update(sources=list(cfg.sources), audio_channels=2, samplerate=44100, segment=Fraction(39, 5))
        sd = synthetic_state_dict(cfg, wseed, period=PACKAGE_PERIOD)
    else:
        from demucs.hdemucs import HDemucs as Klass
        from demucs_amd.hdemucs_weights import HDemucsConfig, synthetic_hdemucs_state_dict
        cfg = HDemucsConfig()
        kwargs = _reference_config("hdemucs")
        kwargs.update(sources=list(cfg.sources), audio_channels=2, samplerate=44100, segment=40)   # train.py: 4 * dset.segment
        sd = synthetic_hdemucs_state_dict(cfg, wseed, period=PACKAGE_PERIOD)
    model = Klass(**kwargs)
    model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()}, strict=True)
    package = ref_states.serialize_model(model, {"fixture": name, "epochs": 0}, quantizer=None, half=True)
    assert package["args"] == () and set(package["kwargs"]) == set(kwargs)
    raw = os.path.join(OUT, name + ".raw.th")
    torch.save(package, raw)
    with zipfile.ZipFile(raw) as zin, zipfile.ZipFile(os.path.join(OUT, name + ".th"), "w", zipfile.ZIP_DEFLATED, compresslevel=9) as zout:
        for info in zin.infolist():
            zout.writestr(info.filename, zin.read(info.filename))
    raw_size = os.path.getsize(raw)
    os.remove(raw)
    store = {"meta/wseed": np.array(wseed), "meta/period": np.array(PACKAGE_PERIOD), "meta/length": np.array(mix.shape[-1]),
             "meta/kwargs": np.array(sorted(kwargs)), "meta/n_tensors": np.array(len(package["state"]))}
    print(f"  {name}: {len(kwargs)} keywords, {len(package['state'])} tensors, {raw_size / 1e6:.0f} MB -> "
          f"{os.path.getsize(os.path.join(OUT, name + '.th')) / 1e6:.2f} MB deflated")
    for tag, dtype in (("f32", torch.float32), ("f64", torch.float64)):
        # the reference's own loader on the fixture (its torch.load predates the weights_only default: the file written
        # a few lines up is opened here and handed over as the package dict)
        m = ref_states.load_model(torch.load(os.path.join(OUT, name + ".th"), map_location="cpu", weights_only=False)).eval().to(dtype)
        with torch.no_grad():
            out = m(torch.from_numpy(mix).to(dtype)[None])
        print(f"  {name} {tag}: out rms {out.pow(2).mean().sqrt():.4f}")
        pack(f"{tag}/out", sample(out, 16384), store)
    np.savez_compressed(os.path.join(OUT, name + ".npz"), **store)


def signature_fixture(name: str):
    """Names and defaults of the reference constructors' keywords (inspect.signature of HTDemucs / HDemucs `__init__`) as
    JSON: tests compare the engine's keyword tables (weights.py, hdemucs.py) with it mechanically."""
    import inspect
    import json
    from fractions import Fraction
    import_reference()
    from demucs.hdemucs import HDemucs
    from demucs.htdemucs import HTDemucs

    def plain(v):
        if v is inspect.Parameter.empty:
            return "<required>"
        if isinstance(v, Fraction):
            return {"Fraction": [v.numerator, v.denominator]}
        return v
    out = {}
    for klass in (HTDemucs, HDemucs):
        params = list(inspect.signature(klass.__init__).parameters.values())[1:]
        out[klass.__name__] = [[p.name, plain(p.default)] for p in params]
    out["config.yaml"] = {k: _reference_config(k) for k in ("htdemucs", "hdemucs")}
    with open(os.path.join(OUT, name + ".json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=False)
    print(f"  {name}: HTDemucs {len(out['HTDemucs'])} keywords, HDemucs {len(out['HDemucs'])}")


def embedding_fixture(name: str, d_model: int, height: int, width: int):
    """The float32 2-D sinusoidal embedding table the reference adds at the cross-transformer's input
    (create_2d_sin_embedding), exactly as the reference computed it on the machine that made the float64 fixtures.  Its
    float32 exp / sin / cos come from the host's vector math library, whose last bits depend on the CPU (MKL takes another
    code path on a non-Intel CPU); the transformer then amplifies them to ~1e-6 in the float64 taps.  The float64 oracle
    tests feed this table to the oracle, so that they pin the algorithm and not the host."""
    import_reference()
    from demucs.transformer import create_2d_sin_embedding
    with torch.no_grad():
        table = create_2d_sin_embedding(d_model, height, width)[0]          # (d_model, height, width) float32
    np.savez_compressed(os.path.join(OUT, name + ".npz"), **{"f32/table": table.numpy()})
    print(f"  {name}: {tuple(table.shape)} {table.dtype}")


def clip_fixture(name: str):
    """`demucs.audio.prevent_clip` in its three modes, and the `--two-stems` arithmetic of
    demucs/separate.py:189-218 obtained by RUNNING the reference's `separate.main` with its `Separator` and `save_audio`
    names swapped for stand-ins that hand over fixed stems and capture what would be written (no audio codec exists here)."""
    import tempfile
    import_reference()
    import demucs.audio as ref_audio
    import demucs.separate as ref_sep
    L = 6000
    names = ["drums", "bass", "other", "vocals"]
    stems = {k: torch.from_numpy(synth_mix(70 + i, L, "tones" if i % 2 else "noise")) * (0.4 + 0.5 * i) for i, k in enumerate(names)}
    origin = sum(stems.values()) + 0.01 * torch.from_numpy(synth_mix(79, L, "noise"))
    store = {"meta/length": np.array(L), "meta/sources": np.array(names), "origin": origin.numpy()}
    for k, v in stems.items():
        store[f"stem/{k}"] = v.numpy()
        for mode in ("rescale", "clamp", "tanh"):
            store[f"clip/{mode}/{k}"] = ref_audio.prevent_clip(v, mode).numpy()
    quiet = stems["drums"] * 0.1                     # below full scale: "rescale" divides by max(1.01 * peak, 1) = 1
    store["stem/quiet"] = quiet.numpy()
    store["clip/rescale/quiet"] = ref_audio.prevent_clip(quiet, "rescale").numpy()

    class FakeSeparator:
        samplerate, audio_channels = 44100, 2
        model = type("M", (), {"sources": names})()

        def __init__(self, *a, **k):
            pass

        def separate_audio_file(self, track):
            return origin.clone(), {k: v.clone() for k, v in stems.items()}
    saved = {}
    real = ref_sep.Separator, ref_sep.save_audio
    ref_sep.Separator = FakeSeparator
    ref_sep.save_audio = lambda wav, path, **kw: saved.__setitem__(os.path.basename(path), wav.clone())
    try:
        with tempfile.TemporaryDirectory() as tmp:
            track = os.path.join(tmp, "song.wav")
            open(track, "wb").close()
            for method in ("add", "minus", "none"):
                saved.clear()
                ref_sep.main(["--two-stems", "vocals", "--other-method", method, "-o", os.path.join(tmp, method), track])
                for fname, wav in saved.items():
                    store[f"two_stems/{method}/{fname.rsplit('.', 1)[0]}"] = wav.numpy()
                print(f"  {name} two-stems {method}: {sorted(saved)}")
    finally:
        ref_sep.Separator, ref_sep.save_audio = real
    np.savez_compressed(os.path.join(OUT, name + ".npz"), **store)


def main():
    global hautocast_fixture, package_fixture, signature_fixture, clip_fixture, embedding_fixture
    global segment_fixture, apply_fixture, separator_fixture, autocast_fixture, hsegment_fixture, happly_fixture
    only = set(sys.argv[1:])
    if only:                                   # regenerate just the named fixtures
        seg_all, app_all = segment_fixture, apply_fixture
        segment_fixture = lambda n, *a, **k: seg_all(n, *a, **k) if n in only else None    # noqa: E731
        apply_fixture = lambda n, *a, **k: app_all(n, *a, **k) if n in only else None      # noqa: E731
        ac_all = autocast_fixture
        autocast_fixture = lambda n, *a, **k: ac_all(n, *a, **k) if n in only else None     # noqa: E731
        hs_all, ha_all = hsegment_fixture, happly_fixture
        hsegment_fixture = lambda n, *a, **k: hs_all(n, *a, **k) if n in only else None     # noqa: E731
        happly_fixture = lambda n, *a, **k: ha_all(n, *a, **k) if n in only else None       # noqa: E731
        sep_all = separator_fixture
        separator_fixture = lambda n, *a, **k: sep_all(n, *a, **k) if n in only else None   # noqa: E731
        hac_all, pk_all, sg_all, cl_all = hautocast_fixture, package_fixture, signature_fixture, clip_fixture
        hautocast_fixture = lambda n, *a, **k: hac_all(n, *a, **k) if n in only else None   # noqa: E731
        package_fixture = lambda n, *a, **k: pk_all(n, *a, **k) if n in only else None      # noqa: E731
        signature_fixture = lambda n, *a, **k: sg_all(n, *a, **k) if n in only else None    # noqa: E731
        clip_fixture = lambda n, *a, **k: cl_all(n, *a, **k) if n in only else None         # noqa: E731
        em_all = embedding_fixture
        embedding_fixture = lambda n, *a, **k: em_all(n, *a, **k) if n in only else None    # noqa: E731
    os.makedirs(OUT, exist_ok=True)
    torch.manual_seed(0)
    cfg4 = HTDemucsConfig()
    cfg6 = HTDemucsConfig(sources=["drums", "bass", "other", "vocals", "guitar", "piano"])
    print("segment fixtures")
    segment_fixture("seg_noise_w0", cfg4, 0, synth_mix(123, SL, "noise"))
    segment_fixture("seg_tones_w1", cfg4, 1, synth_mix(7, SL, "tones"))
    segment_fixture("seg_short_w0", cfg4, 0, synth_mix(5, 100001, "tones"))      # right zero-pad path
    segment_fixture("seg6_noise_w2", cfg6, 2, synth_mix(11, SL, "noise"))
    print("apply fixtures")
    # BASELINE config 1: one 7.8 s segment, shifts=0 -> 2 forwards (offsets 0 and 257985)
    apply_fixture("apply_one_segment", cfg4, [0], None, synth_mix(1, SL, "noise"), shifts=0, split=True, overlap=0.25)
    apply_fixture("apply_2p3_segments", cfg4, [0], None, synth_mix(2, int(2.3 * SL), "tones"),
                  shifts=0, split=True, overlap=0.25)
    apply_fixture("apply_sl_plus_1", cfg4, [1], None, synth_mix(3, SL + 1, "noise"), shifts=0, split=True, overlap=0.25)
    apply_fixture("apply_shifts2", cfg4, [0], None, synth_mix(4, 300000, "tones"), rseed=0,
                  shifts=2, split=True, overlap=0.25)
    apply_fixture("apply_bag2_shift1", cfg4, [10, 11], [[1., 0., 0.5, 0.25], [0., 1., 0.5, 0.75]],
                  synth_mix(5, 400000, "noise"), rseed=3, shifts=1, split=True, overlap=0.25)
    # BASELINE config 3 in miniature: bag of 4 with the one-hot per-source weights of remote/htdemucs_ft.yaml, shifts=2
    apply_fixture("apply_bag4_onehot_shifts2", cfg4, [10, 11, 12, 13],
                  [[1., 0., 0., 0.], [0., 1., 0., 0.], [0., 0., 1., 0.], [0., 0., 0., 1.]],
                  synth_mix(9, 280000, "tones"), rseed=0, shifts=2, split=True, overlap=0.25)
    apply_fixture("apply_nosplit_short", cfg4, [0], None, synth_mix(6, 200000, "tones"), shifts=0, split=False)
    apply_fixture("apply_overlap10_tp2", cfg4, [1], None, synth_mix(8, int(1.5 * SL), "noise"),
                  shifts=0, split=True, overlap=0.1, transition_power=2.0)
    print("autocast (reduced-precision noise floor) fixtures")
    autocast_fixture("autocast_seg_tones_w1", cfg4, 1, synth_mix(7, SL, "tones"))
    autocast_fixture("autocast_seg6_noise_w2", cfg6, 2, synth_mix(11, SL, "noise"))
    print("hdemucs (hdemucs_mmi architecture) fixtures")
    from demucs_amd.hdemucs_weights import HDemucsConfig
    hcfg = HDemucsConfig()
    hsegment_fixture("hseg_tones_10s_w0", hcfg, 0, synth_mix(21, 441000, "tones"))        # T = 431 frames: two BLSTM chunks per row
    hsegment_fixture("hseg_noise_odd_w1", hcfg, 1, synth_mix(22, 233731, "noise"))        # odd length: every right-padding path
    # 449 833 samples, 4 s segments: chunks of 176 400 samples and a last one of 52 933 (T = 52 frames, odd length)
    hsegment_fixture("hseg_tiny_w0", hcfg, 0, synth_mix(24, 1500, "tones"))               # 2 frames: pad1d's zero-then-reflect rule
    happly_fixture("happly_10s_seg4", hcfg, 0, synth_mix(23, 449833, "tones"), shifts=0, split=True, overlap=0.25, segment=4)
    hsegment_fixture("hseg_10smp_w1", hcfg, 1, synth_mix(25, 10, "noise"))                # 10 samples: everything collapses to one position
    # stride 132 300: three full 4-second chunks and a TAIL CHUNK OF 10 SAMPLES (396 910 = 3 * 132 300 + 10)
    happly_fixture("happly_tail10", hcfg, 1, synth_mix(26, 396910, "noise"), shifts=0, split=True, overlap=0.25, segment=4)
    hautocast_fixture("hautocast_10s_w0", hcfg, 0, synth_mix(21, 441000, "tones"))
    # the reference's own offline model: pretrained.get_model("demucs_unittest") = HDemucs(channels=4, sources=SOURCES) (pretrained.py:27-29),
    # here with this repo's deterministic weights; 220 623 samples = 216 frames: the BLSTM runs in two overlapping chunks at layer 4
    hsegment_fixture("hseg_unittest_w3", HDemucsConfig(channels=4), 3, synth_mix(27, 220623, "tones"))
    print("checkpoint package / keyword / clip fixtures")
    package_fixture("pkg_htdemucs", "htdemucs", 5, synth_mix(31, 150000, "tones"))
    package_fixture("pkg_hdemucs", "hdemucs", 6, synth_mix(32, 88200, "noise"))
    signature_fixture("ref_signatures")
    clip_fixture("clip_two_stems")
    embedding_fixture("emb2d_512x8x336", 512, 8, 336)          # htdemucs: bottom channels 512, 8 bins x 336 frames at the transformer
    print("separator fixtures")
    # a loud, DC-shifted input so that the mono mean / std normalisation of api.py:267-269 is far from the identity
    separator_fixture("separator_shift1", cfg4, 3, 3.0 * synth_mix(12, int(1.3 * SL), "tones") + 0.2, rseed=11,
                      shifts=1, overlap=0.25, split=True, segment=None)


if __name__ == "__main__":
    main()
