"""Whole-segment parity of the HIP forward on a real MI355X against (a) the committed golden
fixtures of the reference and (b) the float64 CPU oracle at full resolution.

Tolerance: BASELINE.json's north_star states <= 1e-4 max-abs sample deviation from the CPU
reference; asserted below on the final output (scored against float64 truth), with the SDR of
demucs/evaluate.py:30-43 reported alongside.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from demucs_amd.htdemucs import HTDemucs
from demucs_amd.synth import synth_mix
from demucs_amd.weights import HTDemucsConfig, synthetic_state_dict
from oracle import apply_oracle as A
from oracle import htdemucs_oracle as O

pytestmark = pytest.mark.gpu
SL = 343980
TOL = 1e-4
CFG6 = HTDemucsConfig(sources=["drums", "bass", "other", "vocals", "guitar", "piano"])


def make_model(cfg, wseed, max_batch=2, compute_dtype="f32"):
    m = HTDemucs(cfg.sources, max_batch=max_batch, compute_dtype=compute_dtype)
    m.load_state_dict(synthetic_state_dict(cfg, wseed))
    return m.to("cuda").eval()


CASES = {
    "seg_noise_w0": (HTDemucsConfig(), 0, lambda: synth_mix(123, SL, "noise")),
    "seg_tones_w1": (HTDemucsConfig(), 1, lambda: synth_mix(7, SL, "tones")),
    "seg_short_w0": (HTDemucsConfig(), 0, lambda: synth_mix(5, 100001, "tones")),
    "seg6_noise_w2": (CFG6, 2, lambda: synth_mix(11, SL, "noise")),
}


@pytest.mark.parametrize("name", list(CASES))
def test_forward_matches_reference_golden(golden, name):
    cfg, wseed, mk = CASES[name]
    g = golden(name)
    model = make_model(cfg, wseed)
    mix = torch.from_numpy(mk())[None].cuda()
    out = model(mix)
    torch.cuda.synchronize()
    S = len(cfg.sources)
    shapes = {"enc0": (1, 48, 512, 336), "enc1": (1, 96, 128, 336), "enc2": (1, 192, 32, 336), "enc3": (1, 384, 8, 336),
              "tenc0": (1, 48, 85995), "tenc1": (1, 96, 21499), "tenc2": (1, 192, 5375), "tenc3": (1, 384, 1344),
              "dec3": (1, 4 * S, 2048, 336), "tdec3": (1, 2 * S, SL)}
    names = {"dec3": "yspec", "tdec3": "ytime"}
    worst = {}
    for tap, shape in shapes.items():
        t = model.tap(names.get(tap, tap), 1)
        if tap == "enc0":
            # the golden hook sees encoder.0 BEFORE the frequency embedding is added (htdemucs.py:577-582): take the
            # embedding 0.2 * (10 * weight).t() off the engine's tap and compare with `enc0_preemb`
            w = torch.from_numpy(synthetic_state_dict(cfg, wseed)["freq_emb.embedding.weight"]).cuda()      # (512, 48)
            t = t.reshape(shape) - (0.2 * (w * 10.0)).t()[None, :, :, None]
            worst[tap] = g.check("f64", "enc0_preemb", t, atol=2e-4, rtol=2e-4)
            continue
        if tap.startswith("tenc"):                           # time-branch rows carry a pitch rounded up to 4
            t = t.view(1, shape[1], -1)[..., :shape[2]]
        t = t.reshape(shape)
        worst[tap] = g.check("f64", tap, t, atol=2e-4, rtol=2e-4)
    # transformer output: our token order is (fr, t1), the reference's is (t1, fr)
    trf = model.tap("tr_f", 1).view(1, 512, 8, 336).permute(0, 1, 3, 2).reshape(1, 512, 2688)
    worst["tr4_f"] = g.check("f64", "tr4_f", trf, atol=2e-4, rtol=2e-4)
    worst["tr4_t"] = g.check("f64", "tr4_t", model.tap("tr_t", 1).view(1, 512, 1344), atol=2e-4, rtol=2e-4)
    worst["out"] = g.check("f64", "out", out, atol=TOL)
    print(name, {k: f"{v:.2e}" for k, v in worst.items()})


def test_forward_full_resolution_vs_float64_oracle():
    """Every sample of a batch of 2 different segments against the float64 oracle; also checks that
    batching is exact per item (statistics are per item)."""
    cfg = HTDemucsConfig()
    sd = synthetic_state_dict(cfg, 3)
    model = make_model(cfg, 3, max_batch=2)
    mix = torch.stack([torch.from_numpy(synth_mix(21, SL, "tones")), torch.from_numpy(synth_mix(22, SL, "noise"))])
    out = model(mix.cuda()).cpu()
    osd = O.to_torch_state(sd, torch.float64)
    with torch.no_grad():
        want = O.htdemucs_forward(osd, mix.double(), 4)
    err = (out.double() - want).abs().max().item()
    sdr = A.new_sdr(want.float(), out).min().item()
    print(f"full-resolution max-abs {err:.3e}  min SDR {sdr:.1f} dB  (out rms {want.pow(2).mean().sqrt():.3f})")
    assert err <= TOL
    assert sdr > 80.0
    single = model(mix[1:].cuda()).cpu()
    assert torch.equal(single[0], out[1]), "batched and single-item forwards must be bit-identical"


AUTOCAST = {"autocast_seg_tones_w1": (HTDemucsConfig(), 1, lambda: synth_mix(7, SL, "tones")),
            "autocast_seg6_noise_w2": (CFG6, 2, lambda: synth_mix(11, SL, "noise"))}


def _sample_sdr(want, got):
    return float(10 * np.log10((np.sum(want * want) + 1e-7) / (np.sum((got - want) ** 2) + 1e-7)))


@pytest.mark.parametrize("mode,floor_db", [("bf16", 28.0), ("f16", 44.0)])
@pytest.mark.parametrize("name", list(AUTOCAST))
def test_reduced_precision_modes_against_reference_autocast_floor(golden, name, mode, floor_db):
    """g1 / g2 (BASELINE configs[2] "bf16", configs[4] "fp16"): compute modes with bf16 / fp16 matrix-core operands and
    float32 everything else.  No 1e-4 bar applies to a reduced-precision mode (that is the float32 mode's); stated
    tolerance instead: SDR (evaluate.py:30-43 formula) against the reference's float64 output of at least `floor_db`
    AND at least that of the reference's OWN float32 model under `torch.autocast("cpu", dtype=...)` on the same input
    (fixture made by tools/make_golden.py), minus 1 dB of sampling slack.  Max-abs is reported beside it."""
    cfg, wseed, mk = AUTOCAST[name]
    g = golden(name)
    model = make_model(cfg, wseed, compute_dtype=mode)
    out = model(torch.from_numpy(mk())[None].cuda()).cpu()
    assert bool(torch.isfinite(out).all())
    stride = int(g.z["f64/out/stride"])
    got = out.reshape(-1)[::stride].double().numpy()
    want = g.z["f64/out/sample"].astype(np.float64)
    ref = g.z[f"{mode}/out/sample"].astype(np.float64)
    sdr, ref_sdr = _sample_sdr(want, got), _sample_sdr(want, ref)
    err, ref_err = float(np.abs(got - want).max()), float(np.abs(ref - want).max())
    print(f"{name} {mode}: engine max-abs {err:.3e} SDR {sdr:.1f} dB | reference under CPU autocast: max-abs {ref_err:.3e} SDR {ref_sdr:.1f} dB"
          f" (whole-tensor reference figures: max-abs {float(g.z[mode + '/max_abs']):.3e}, min SDR {float(g.z[mode + '/sdr_db']):.1f} dB)")
    assert sdr >= floor_db and sdr >= ref_sdr - 1.0, (sdr, ref_sdr)
    # the float32 mode of the same handle type is untouched by the switch
    m32 = make_model(cfg, wseed)
    out32 = m32(torch.from_numpy(mk())[None].cuda()).cpu()
    assert float(np.abs(out32.reshape(-1)[::stride].double().numpy() - want).max()) <= TOL


def test_forward_core_contract():
    """forward_core (htdemucs.py:662-759): spec_out / time_out before iSTFT, against the float64 oracle;
    iSTFT(spec_out) + time_out must reproduce the full forward."""
    import ctypes as C
    from demucs_amd import _lib
    cfg = HTDemucsConfig()
    sd = synthetic_state_dict(cfg, 5)
    model = make_model(cfg, 5, max_batch=1)
    mix = torch.from_numpy(synth_mix(61, SL, "tones"))[None]
    spec, tout = model.forward_core(None, mix.cuda())
    taps = {}
    with torch.no_grad():
        O.htdemucs_forward(O.to_torch_state(sd, torch.float64), mix.double(), 4, taps=taps)
    es = (spec.cpu().double() - taps["spec_out"]).abs().max().item()
    et = (tout.cpu().double() - taps["time_out"]).abs().max().item()
    assert es <= 2e-4 * taps["spec_out"].abs().max().item() and et <= 2e-4 * taps["time_out"].abs().max().item(), (es, et)
    wav = torch.empty(1, 4, 2, SL, device="cuda")
    _lib.check(_lib.load().mi_istft_cac(spec.data_ptr(), 1, 4, SL, wav.data_ptr(), C.c_void_p(_lib.current_stream_ptr())), "istft")
    full = model(mix.cuda())
    assert (wav + tout - full).abs().max().item() < 2e-5
    with pytest.raises(ValueError):
        model.forward_core(torch.zeros(1, 4, 2048, 10), mix.cuda())
    # a caller-supplied `mag` is what the frequency branch consumes (the fork's ONNX / web tools compute it with their
    # own STFT): the oracle's spectrogram reproduces the mag=None result, a different spectrogram changes spec_out only
    mag = taps["stft"].float().cuda()
    spec2, tout2 = model.forward_core(mag, mix.cuda())
    assert (spec2 - spec).abs().max().item() <= 2e-4 * spec.abs().max().item()
    assert (tout2 - tout).abs().max().item() <= 2e-4 * tout.abs().max().item()
    spec3, _ = model.forward_core(0.5 * mag + 0.01, mix.cuda())
    taps3 = {}
    with torch.no_grad():
        O.htdemucs_forward(O.to_torch_state(sd, torch.float64), mix.double(), 4, taps=taps3, mag_override=0.5 * taps["stft"] + 0.01)
    assert (spec3.cpu().double() - taps3["spec_out"]).abs().max().item() <= 2e-4 * taps3["spec_out"].abs().max().item()
    assert (spec3 - spec).abs().max().item() > 1e-3


def test_model_rejects_cpu_and_bad_shapes():
    cfg = HTDemucsConfig()
    m = HTDemucs(cfg.sources)
    m.load_state_dict(synthetic_state_dict(cfg, 0))
    with pytest.raises(RuntimeError):
        m.to("cpu")(torch.zeros(1, 2, SL))            # no CPU fallback: must fail loudly
    m.to("cuda")
    with pytest.raises(ValueError):
        m(torch.zeros(1, 2, SL + 1, device="cuda"))   # htdemucs.py:521-524
    with pytest.raises(ValueError):
        m.forward_segments(torch.zeros(1, 3, SL, device="cuda"))


@pytest.mark.skipif(os.environ.get("MI_X6") is not None or os.environ.get("MI_DCONV_ROW") is not None, reason="already inside the re-run")
def test_non_default_kernel_switches_keep_parity():
    """Non-default kernel routes, re-run together in ONE fresh process (the switches are read once, when the library is loaded;
    they touch disjoint layers):
      * MI_X6=1 (gemm_x6.hip: fp32 operands as three exact bf16 terms, six bf16 MFMA products, fp32 accumulate) on the
        transformer / 1x1 layers -- single process, as DESIGN.md section 8 requires for this mode;
      * MI_DCONV_ROW=lds (dconv_row.hip `dconv_rowlds_kernel`: the C = 48 frequency rows stay in LDS across both residual
        layers; slower than the per-wave kernel, kept selectable);
      * MI_NO_DMA_TAP=1 / MI_NO_DMA_ROWS=1: the float32 k x k, strided and transposed convs back on the table-driven gather of
        conv_gemm_kernel (round 3's route, which the LDS-DMA main loops replaced by default).
    The reference-golden and float64-oracle parity tests above must hold unchanged.  Then the half-mode switch groups, against
    the reduced-precision floors (below)."""
    env = dict(os.environ, MI_X6="1", MI_X6_MODE="1", MI_DCONV_ROW="lds", MI_NO_DMA_TAP="1", MI_NO_DMA_ROWS="1")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-m", "gpu", "-q", "-x", "-k",
                        "reference_golden or float64_oracle", "-p", "no:cacheprovider"], env=env, capture_output=True, text=True,
                       cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "passed" in r.stdout
    # The half-mode routes behind the image / statistics / schedule switches, one fresh process per group (the groups overlap in
    # the layers they touch): group A -- float32 projection inputs, float32 encoder conv inputs, norm_out's statistics by a
    # separate pass, one stream; group B -- float32 Q / K / V, table-driven decoder convs, time-branch DConv on the implicit-GEMM
    # route; group C -- float32 attention output and FFN hidden tensor.  Each must meet the floors the default routes meet.
    groups = {"A": dict(MI_NO_INPUT_IMAGE="1", MI_NO_ENC_IMAGE="1", MI_NO_LIN2_STATS="1", MI_ONE_STREAM="1"),
              "B": dict(MI_NO_QKV_HEADS="1", MI_NO_TAP_IMAGE="1", MI_NO_DCONV_TIME="1"),
              "C": dict(MI_NO_FFN_IMAGE="1")}
    for tag, extra in groups.items():
        r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-m", "gpu", "-q", "-x", "-k",
                            "autocast_floor and autocast_seg_tones_w1", "-p", "no:cacheprovider"], env=dict(os.environ, **extra),
                           capture_output=True, text=True, cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
        assert r.returncode == 0, f"group {tag}: " + r.stdout[-3000:] + r.stderr[-2000:]
        assert "2 passed" in r.stdout, f"group {tag}: " + r.stdout[-1000:]
