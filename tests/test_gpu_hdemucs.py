"""SURVEY 8 a25 on a real MI355X: the Hybrid Demucs v3 engine (`hdemucs_mmi` architecture: BLSTM, LocalState, GroupNorm(4),
merge layer, decoders from zeros, any input length) against the reference's outputs (tests/golden/hseg_*.npz,
happly_*.npz made by tools/make_golden.py from the imported `demucs.hdemucs.HDemucs`) and the float64 oracle.

Tolerance: the float32 bar of north_star (<= 1e-4 max-abs on the output, scored against the float64 reference run)."""
import numpy as np
import pytest
import torch

from demucs_amd import apply as P
from demucs_amd.hdemucs import HDemucs
from demucs_amd.hdemucs_weights import HDemucsConfig, synthetic_hdemucs_state_dict
from demucs_amd.synth import synth_mix

pytestmark = pytest.mark.gpu
TOL = 1e-4
HSEG = {"hseg_tones_10s_w0": (0, lambda: synth_mix(21, 441000, "tones")),
        "hseg_noise_odd_w1": (1, lambda: synth_mix(22, 233731, "noise")),
        "hseg_tiny_w0": (0, lambda: synth_mix(24, 1500, "tones")),
        "hseg_10smp_w1": (1, lambda: synth_mix(25, 10, "noise"))}


def engine(wseed, max_batch=1, compute_dtype="f32"):
    cfg = HDemucsConfig()
    m = HDemucs(cfg.sources, max_batch=max_batch, compute_dtype=compute_dtype)
    m.load_state_dict(synthetic_hdemucs_state_dict(cfg, wseed))
    return m.to("cuda").eval()


@pytest.mark.parametrize("name", list(HSEG))
def test_forward_matches_reference_golden(golden, name):
    wseed, mk = HSEG[name]
    g = golden(name)
    m = engine(wseed)
    mix = torch.from_numpy(mk())[None].cuda()
    out = m(mix)
    L = mix.shape[-1]
    T = -(-L // 1024)
    Tp = max(32, -(-T // 4) * 4)             # frame pitch of the frequency-branch tensors
    lt = [L]
    for _ in range(5):
        lt.append(-(-lt[-1] // 4))
    lp = [-(-v // 4) * 4 for v in lt]
    ch, fr = [48, 96, 192, 384], [512, 128, 32, 8]
    worst = {}
    for i in range(4):
        t = m.tap(f"enc{i}", 1).reshape(1, ch[i], fr[i], Tp)[..., :T]
        if i == 0:       # the golden hook sees encoder.0 before the frequency embedding is added
            w = torch.from_numpy(synthetic_hdemucs_state_dict(HDemucsConfig(), wseed)["freq_emb.embedding.weight"]).cuda()
            worst["enc0"] = g.check("f64", "enc0_preemb", t - (0.2 * (w * 10.0)).t()[None, :, :, None], atol=2e-4, rtol=2e-4)
        else:
            worst[f"enc{i}"] = g.check("f64", f"enc{i}", t, atol=2e-4, rtol=2e-4)
        tt = m.tap(f"tenc{i}", 1).view(1, ch[i], lp[i + 1])[..., :lt[i + 1]]
        worst[f"tenc{i}"] = g.check("f64", f"tenc{i}", tt, atol=2e-4, rtol=2e-4)
    worst["tenc4"] = g.check("f64", "tenc4", m.tap("tenc4", 1).view(1, 768, T), atol=2e-4, rtol=2e-4)
    worst["enc4"] = g.check("f64", "enc4", m.tap("enc4", 1).view(1, 768, 1, T), atol=2e-4, rtol=2e-4)
    worst["enc5"] = g.check("f64", "enc5", m.tap("enc5", 1).view(1, 1536, -(-T // 2)), atol=2e-4, rtol=2e-4)
    worst["dec5"] = g.check("f64", "dec5", m.tap("dec5", 1).view(1, 16, 2048, Tp)[..., :T], atol=2e-4, rtol=2e-4)
    worst["tdec4"] = g.check("f64", "tdec4", m.tap("tdec4", 1).view(1, 8, lp[0])[..., :L], atol=2e-4, rtol=2e-4)
    worst["out"] = g.check("f64", "out", out, atol=TOL)
    g.check("f32", "out", out, atol=TOL)
    print(name, {k: f"{v:.2e}" for k, v in worst.items()})


def test_full_resolution_vs_float64_oracle_and_batching():
    """Every sample of a batch of 2 against the float64 oracle (4.2 s: three BLSTM chunks at layer 4, none at layer 5);
    batched == single-item bit for bit."""
    from demucs_amd.hdemucs_weights import hdemucs_layer_plan
    from oracle import apply_oracle as A
    from oracle import hdemucs_oracle as HO
    cfg = HDemucsConfig()
    sd = synthetic_hdemucs_state_dict(cfg, 3)
    m = HDemucs(cfg.sources, max_batch=2)
    m.load_state_dict(sd)
    m.to("cuda")
    L = 185222
    mix = torch.stack([torch.from_numpy(synth_mix(31, L, "tones")), torch.from_numpy(synth_mix(32, L, "noise"))])
    out = m(mix.cuda()).cpu()
    osd = {k: torch.from_numpy(v.copy()).double() for k, v in sd.items()}
    with torch.no_grad():
        want = HO.hdemucs_forward(osd, mix.double(), hdemucs_layer_plan(cfg), 4)
    err = (out.double() - want).abs().max().item()
    sdr = A.new_sdr(want.float(), out).min().item()
    print(f"hdemucs full-resolution max-abs {err:.3e}  min SDR {sdr:.1f} dB  (out rms {want.pow(2).mean().sqrt():.3f})")
    assert err <= TOL and sdr > 80.0
    single = m(mix[1:].cuda()).cpu()
    assert torch.equal(single[0], out[1])


def test_many_sequences_span_several_lstm_tiles():
    """A batch of 7 items of 23.3 s: the BLSTM of encoder.4 sees 7 x 11 = 77 framed sequences (sequence tiles of 32, 32
    and 13 in `lstm_step_kernel`), encoder.5's 7 x 6 = 42 (32 + 10), and LocalState runs over 1 004 / 502 positions with
    a ragged last key tile -- the geometry of the 44-second production chunks, checked sample by sample against the
    float32 oracle (the 4-second cases above, against the float64 one, stay inside one tile)."""
    from demucs_amd.hdemucs_weights import hdemucs_layer_plan
    from oracle import hdemucs_oracle as HO
    cfg = HDemucsConfig()
    sd = synthetic_hdemucs_state_dict(cfg, 5)
    B, L = 7, 1027600
    m = HDemucs(cfg.sources, max_batch=B)
    m.load_state_dict(sd)
    m.to("cuda")
    mix = torch.stack([torch.from_numpy(synth_mix(60 + b, L, "tones" if b % 2 else "noise")) for b in range(B)])
    out = m(mix.cuda()).cpu()
    osd = {k: torch.from_numpy(v.copy()) for k, v in sd.items()}          # float32 oracle (its own error ~1e-5): half the CPU time
    # items are independent; the oracle (the slow side) scores three of them: item 1's 11 sequences cross the boundary of the LSTM
    # kernel's first two 16-sequence tiles, item 4's the third / fourth, item 6 fills the ragged last tile
    pick = [1, 4, 6]
    with torch.no_grad():
        want = HO.hdemucs_forward(osd, mix[pick], hdemucs_layer_plan(cfg), 4).double()
    err = (out[pick].double() - want).abs().amax(dim=(1, 2, 3))
    print(f"hdemucs 7 x 23.3 s: max-abs of items {pick} {[f'{e:.2e}' for e in err.tolist()]} (out rms {want.pow(2).mean().sqrt():.3f})")
    assert float(err.max()) <= TOL and bool(torch.isfinite(out).all())


@pytest.mark.parametrize("name,max_batch", [("happly_10s_seg4", 1), ("happly_10s_seg4", 2), ("happly_tail10", 3)])
def test_apply_model_matches_reference(golden, name, max_batch):
    """`apply_model` around the engine with a segment override: three chunks of 176 400 samples and a last one of 52 933
    (happly_tail10: a TAIL CHUNK OF 10 SAMPLES), each forwarded at its own length (the reference's HDemucs has no
    valid_length) -- equal-length chunks batched up to `max_batch` per forward, same events in the same order; host mix in,
    result on the host."""
    g = golden(name)
    m = engine(int(g.meta("wseed")), max_batch=max_batch)
    kw = {k[len("meta/kw_"):]: g.z[k].item() for k in g.z.files if k.startswith("meta/kw_")}
    L = int(g.meta("length"))
    mix = torch.from_numpy(synth_mix(23, L, "tones") if name == "happly_10s_seg4" else synth_mix(26, L, "noise"))[None]
    events = []
    out = P.apply_model(m, mix, device="cuda", callback=lambda d: events.append(dict(d)), **kw)
    assert out.device.type == "cpu" and out.shape == (1, 4, 2, L)
    e64 = g.check("f64", "out", out, atol=TOL)
    g.check("f32", "out", out, atol=TOL)
    keys = ["model_idx_in_bag", "shift_idx", "segment_offset", "models", "state"]
    got = np.array([[str(e[k]) for k in keys] for e in events])
    assert got.shape == g.z["events"].shape and (got == g.z["events"]).all()
    m.check()                     # mi_hmodel_status: no forward of this handle lost its recurrence to a time-out (apply_model asked too)
    print(f"hdemucs apply_model: max-abs vs reference f64 {e64:.2e}")


def test_bag_raises_segment_fp16_mode_and_errors():
    """remote/hdemucs_mmi.yaml: a bag of one model with `segment: 44` (BagOfModels raises the member's segment, apply.py:53-55);
    BASELINE configs[4]'s fp16 mode on a 50-second track (two chunks: 44 s and the rest); empty chunks are refused loudly."""
    from oracle import apply_oracle as A
    lo, hi = engine(0, compute_dtype="f16"), engine(0)
    bag = P.BagOfModels([lo], segment=44)
    assert lo.segment == 44
    L = 50 * 44100
    mix = torch.from_numpy(synth_mix(5, L, "noise"))[None].cuda()
    out = P.apply_model(bag, mix, shifts=0, overlap=0.25)
    assert out.shape == (1, 4, 2, L) and bool(torch.isfinite(out).all())
    ref = P.apply_model(P.BagOfModels([hi], segment=44), mix, shifts=0, overlap=0.25)
    sdrs = A.new_sdr(ref.cpu(), out.cpu())
    print(f"hdemucs fp16 mode, 50 s track, 44 s segments: per-source SDR vs the float32 mode {[round(float(v), 1) for v in sdrs.flatten()]} dB")
    assert float(sdrs.min()) >= 40.0
    with pytest.raises(ValueError):
        hi(torch.zeros(1, 2, 0, device="cuda"))
    with pytest.raises(RuntimeError):
        hi.to("cpu")(torch.zeros(1, 2, 40000))


@pytest.mark.parametrize("length", [1, 2, 3, 5, 33, 63, 64, 777, 2559, 2561, 5000, 31000])
def test_short_chunks_match_float64_oracle(length):
    """The reference's HDemucs takes ANY chunk length (no valid_length), down to a handful of samples: pad1d's
    zero-then-reflect rule (hdemucs.py:29-36) below 2 560 samples, a single STFT frame below 1 025, BLSTM without framing.
    The oracle is pinned on that path by the reference golden `hseg_tiny_w0` (tests/test_oracle_golden.py)."""
    from demucs_amd.hdemucs_weights import hdemucs_layer_plan
    from oracle import hdemucs_oracle as HO
    cfg = HDemucsConfig()
    sd = synthetic_hdemucs_state_dict(cfg, 2)
    m = HDemucs(cfg.sources, max_batch=1)
    m.load_state_dict(sd)
    m.to("cuda")
    mix = torch.from_numpy(synth_mix(40 + length % 7, length, "tones"))[None]
    out = m(mix.cuda()).cpu()
    osd = {k: torch.from_numpy(v.copy()).double() for k, v in sd.items()}
    with torch.no_grad():
        want = HO.hdemucs_forward(osd, mix.double(), hdemucs_layer_plan(cfg), 4)
    err = (out.double() - want).abs().max().item()
    print(f"hdemucs {length} samples: max-abs {err:.3e} (out rms {want.pow(2).mean().sqrt():.3f})")
    assert out.shape == (1, 4, 2, length) and err <= TOL


def test_tail_chunk_overlap_is_bit_identical_and_stable(monkeypatch):
    """Without listeners `apply_model` runs a track's shorter tail chunk on the side engine and a side stream while the full
    chunks' batched forward runs (demucs_amd/apply.py ragged_split_accumulate): the result must equal the sequential
    schedule's bit for bit -- float32 and fp16 modes, 12 repeats each (two kernel streams share the CUs here)."""
    L = int(2.4 * 4 * 44100) + 777                  # segment override 4 s: offsets 0, 3 s, 6 s, 9 s -> 3 full chunks + a 0.6 s tail
    mix = torch.from_numpy(synth_mix(77, L, "noise"))[None].cuda()
    for dtype in ("f32", "f16"):
        m = engine(1, max_batch=3, compute_dtype=dtype)
        monkeypatch.setenv("MI_NO_TAIL_OVERLAP", "1")
        want = P.apply_model(m, mix, shifts=0, overlap=0.25, segment=4)
        monkeypatch.delenv("MI_NO_TAIL_OVERLAP")
        for rep in range(12):
            got = P.apply_model(m, mix, shifts=0, overlap=0.25, segment=4)
            assert torch.equal(got, want), f"{dtype} repeat {rep}: overlapped tail differs, max {float((got - want).abs().max()):.3e}"
        assert (m._device, True) in m._handles           # the side engine really ran
        m.release()


def test_handle_outlives_many_distinct_lengths():
    """A long-lived handle sees a new input length with every track's tail chunk and every random shift: the per-length
    geometries (gather tables) are cached LRU (hmodel.hip kMaxGeos = 24), so 70 distinct lengths through ONE handle must
    neither fail nor grow the device footprint without bound, and a length that was evicted gives the same bits again."""
    m = engine(2)
    x = torch.from_numpy(synth_mix(9, 4000, "tones"))[None].cuda()
    first = m(x[..., :1100]).clone()
    sizes = []
    for i in range(70):
        n = 1101 + 17 * i
        out = m(x[..., :n])
        assert out.shape == (1, 4, 2, n)
        sizes.append(m.device_bytes())
    assert bool(torch.isfinite(out).all())
    assert sizes[-1] == sizes[30], "device footprint keeps growing with the number of distinct lengths"
    assert torch.equal(m(x[..., :1100]), first)          # evicted long ago, rebuilt: same result


def test_the_reference_unittest_model_width(golden):
    """`demucs_unittest`, the only model the reference ships offline and the one its own CI runs, is HDemucs(channels=4)
    (pretrained.py:27-29): the engine takes the layer widths from the weights (4 ... 128 channels; hidden 16 / 32 in the BLSTM,
    head dimension 4 / 8 in LocalState: generic kernels), checked against the reference's forward with this repo's weights
    (fixture `hseg_unittest_w3`: output and the deep layers' taps), in float32 and -- table routes only, the widths are no
    multiples of 8 -- in the fp16 mode."""
    g = golden("hseg_unittest_w3")
    cfg = HDemucsConfig(channels=4)
    sd = synthetic_hdemucs_state_dict(cfg, 3)
    mix = torch.from_numpy(synth_mix(27, 220623, "tones"))[None].cuda()
    L = mix.shape[-1]
    T = -(-L // 1024)
    m = HDemucs(cfg.sources, max_batch=2, channels=4)
    m.load_state_dict(sd)
    m.to("cuda")
    out = m(torch.cat([mix, mix]))
    assert torch.equal(out[0], out[1])
    err = g.check("f64", "out", out[:1], atol=TOL)
    g.check("f64", "enc4", m.tap("enc4", 1).view(1, 64, 1, T), atol=2e-4, rtol=2e-4)
    g.check("f64", "enc5", m.tap("enc5", 1).view(1, 128, -(-T // 2)), atol=2e-4, rtol=2e-4)
    g.check("f64", "tenc4", m.tap("tenc4", 1).view(1, 64, T), atol=2e-4, rtol=2e-4)
    print(f"demucs_unittest width: max-abs vs the reference's float64 forward {err:.2e}")
    mh = HDemucs(cfg.sources, max_batch=1, channels=4, compute_dtype="f16")
    mh.load_state_dict(sd)
    mh.to("cuda")
    lo = mh(mix)
    want = out[:1].double()
    sdr = 10 * torch.log10(want.pow(2).sum() / (lo.double() - want).pow(2).sum())
    print(f"demucs_unittest width, fp16 mode: SDR vs the float32 mode {float(sdr):.1f} dB")
    assert float(sdr) >= 38.0
    # the reference's `Separator("demucs_unittest")` plumbing (api.py:99-104, pretrained.py:64-65): resolves offline, separates a clip
    from demucs_amd.api import Separator
    from demucs_amd.pretrained import SOURCES, get_model
    sep = Separator("demucs_unittest", device="cuda", shifts=0, overlap=0.25)
    wav = mix[0].cpu().clone()
    back, stems = sep.separate_tensor(wav)
    assert list(stems) == SOURCES and all(v.shape == wav.shape and bool(torch.isfinite(v).all()) for v in stems.values())
    assert torch.equal(back, wav) and get_model("demucs_unittest").cfg.channels == 4


@pytest.mark.parametrize("mode,floor_db", [("f16", 38.0), ("bf16", 20.0)])
def test_reduced_precision_modes_against_the_reference_autocast_floor(golden, mode, floor_db):
    """BASELINE configs[4] (hdemucs fp16) scored against the REFERENCE, not against this engine's own float32 mode:
    tests/golden/hautocast_10s_w0.npz holds the reference's float64 output and the SDR its own float32 model reaches under
    `torch.autocast("cpu", fp16 / bf16)` on the same input.  The engine's mode must reach that floor - 1 dB (stated
    tolerance of the reduced-precision modes) and an absolute minimum."""
    g = golden("hautocast_10s_w0")
    m = engine(int(g.meta("wseed")), compute_dtype=mode)
    mix = torch.from_numpy(synth_mix(21, int(g.meta("length")), "tones"))[None].cuda()
    out = m(mix).cpu()
    p = "f64/out"
    stride = int(g.z[p + "/stride"])
    want = g.z[p + "/sample"].astype(np.float64)
    got = out.reshape(-1)[::stride].double().numpy()
    sdr = 10 * np.log10((want ** 2).sum() / ((got - want) ** 2).sum())
    ref_sdr = float(g.z[f"{mode}/sdr_db"])
    print(f"hdemucs {mode}: SDR vs the reference's float64 output {sdr:.1f} dB on the stored sample "
          f"(reference under CPU autocast: min per-source {ref_sdr:.1f} dB, max-abs {float(g.z[mode + '/max_abs']):.2e}); "
          f"max-abs {np.abs(got - want).max():.2e}")
    assert sdr >= max(floor_db, ref_sdr - 1.0)


def test_production_chunk_44s_against_float64_oracle():
    """One 44-second item (1 940 400 samples: T = 1 895 frames, 19 BLSTM frames per row at layer 4, 10 at layer 5) -- the
    chunk `hdemucs_mmi` really runs (remote/hdemucs_mmi.yaml segment: 44) -- sample by sample against the FLOAT64 oracle
    (itself pinned to the float64 reference to 2e-9 on the goldens).  Reported beside it, for scale, is the float32 ORACLE
    against the same float64 result (7.39e-5 on this input: the noise floor of any float32 evaluation of this network at this
    length; the engine measured 7.8e-5 - 8.1e-5), so the output says which side of a float32-vs-float32 difference carries what."""
    from demucs_amd.hdemucs_weights import hdemucs_layer_plan
    from oracle import hdemucs_oracle as HO
    cfg = HDemucsConfig()
    sd = synthetic_hdemucs_state_dict(cfg, 4)
    L = 44 * 44100
    m = HDemucs(cfg.sources, max_batch=1)
    m.load_state_dict(sd)
    m.segment = 44
    m.to("cuda")
    mix = torch.from_numpy(synth_mix(90, L, "tones"))[None]
    out = m(mix.cuda()).cpu()
    plan = hdemucs_layer_plan(cfg)
    with torch.no_grad():
        want = HO.hdemucs_forward({k: torch.from_numpy(v.copy()).double() for k, v in sd.items()}, mix.double(), plan, 4)
        want32 = HO.hdemucs_forward({k: torch.from_numpy(v.copy()).float() for k, v in sd.items()}, mix.float(), plan, 4)
    err = float((out.double() - want).abs().max())
    err32 = float((want32.double() - want).abs().max())
    print(f"hdemucs 44 s item: engine vs float64 oracle max-abs {err:.3e}; float32 oracle vs float64 oracle {err32:.3e}; engine vs "
          f"float32 oracle {float((out - want32).abs().max()):.3e} (out rms {want.pow(2).mean().sqrt():.3f})")
    assert err <= TOL and err32 <= TOL


# ------------------------------------------------------------------------------------------------
# Batches of short chunks.  The time branch's DConv blocks (encoder levels 0 - 3) take their GroupNorm statistics per ITEM from the
# k = 3 conv's epilogue, which reduces 32 consecutive columns at a time; level i's rows have a pitch of round_up(ceil(L / 4^(i+1)), 4)
# floats, so below L = 3 072 (and for 4 097 .. 5 120) three or more items of a batch share such a run at some level.
SHORT_LENGTHS = [40, 100, 777, 2561, 3000, 5000]


def short_batch(length):
    """four different items of `length` samples: kinds alternate, seeds differ"""
    return torch.stack([torch.from_numpy(synth_mix(100 + 7 * b + length % 13, length, "tones" if b % 2 == 0 else "noise")) for b in range(4)])


@pytest.fixture(scope="module")
def short_f32():
    """ONE float32 engine with max_batch = 4 for every length (a geometry change with B > 1 comes with it) and its batched
    outputs, each computed once"""
    m, outs = engine(2, max_batch=4), {}

    def run(length):
        if length not in outs:
            outs[length] = m(short_batch(length).cuda()).cpu()
        return outs[length]
    run.model = m
    yield run
    m.release()


@pytest.mark.parametrize("length", SHORT_LENGTHS)
def test_batches_of_short_chunks_match_float64_oracle(short_f32, length):
    """Every item of a batch of 4 short chunks against the float64 oracle at the suite's bar, and bit for bit equal to the
    single-item forward of that item on the same handle."""
    from demucs_amd.hdemucs_weights import hdemucs_layer_plan
    from oracle import hdemucs_oracle as HO
    cfg = HDemucsConfig()
    sd = synthetic_hdemucs_state_dict(cfg, 2)
    mix = short_batch(length)
    out = short_f32(length)
    assert out.shape == (4, 4, 2, length)
    osd = {k: torch.from_numpy(v.copy()).double() for k, v in sd.items()}
    with torch.no_grad():
        want = HO.hdemucs_forward(osd, mix.double(), hdemucs_layer_plan(cfg), 4)
    err = (out.double() - want).abs().amax(dim=(1, 2, 3))
    print(f"hdemucs 4 x {length} samples: max-abs per item {[f'{e:.2e}' for e in err.tolist()]} (out rms {want.pow(2).mean().sqrt():.3f})")
    singles = [short_f32.model(mix[b:b + 1].cuda()).cpu()[0] for b in range(4)]
    assert float(err.max()) <= TOL
    for b in range(4):
        assert torch.equal(singles[b], out[b]), f"item {b} of the batch differs from its single-item forward by {float((singles[b] - out[b]).abs().max()):.3e}"


@pytest.mark.parametrize("mode,floor_db", [("f16", 38.0), ("bf16", 20.0)])
def test_batches_of_short_chunks_half_modes(short_f32, mode, floor_db):
    """The same batches in the reduced-precision modes: batched == single-item bit for bit, finite, and at least the mode's SDR
    floor of this file against the float32 mode's output."""
    m = engine(2, max_batch=4, compute_dtype=mode)
    for length in SHORT_LENGTHS:
        mix = short_batch(length).cuda()
        out = m(mix).cpu()
        assert out.shape == (4, 4, 2, length) and bool(torch.isfinite(out).all())
        want = short_f32(length).double()
        noise = (out.double() - want).pow(2)
        sdr = 10 * torch.log10(want.pow(2).sum() / noise.sum())
        per_item = 10 * torch.log10(want.pow(2).sum((1, 2, 3)) / noise.sum((1, 2, 3)))
        print(f"hdemucs {mode} 4 x {length} samples: SDR vs the float32 mode {float(sdr):.1f} dB (per item {[round(float(v), 1) for v in per_item]})")
        for b in range(4):
            single = m(mix[b:b + 1]).cpu()[0]
            assert torch.equal(single, out[b]), f"{mode} {length}: item {b} of the batch differs from its single-item forward"
        assert float(per_item.min()) >= floor_db, (mode, length, per_item.tolist())
    m.release()


def test_apply_model_on_four_short_tracks_equals_one_at_a_time(short_f32):
    """`apply_model` on a (4, 2, 2561) mix on the engine with max_batch = 4: each track's result equals the one it gets alone,
    bit for bit, however the tracks' chunks were grouped into forwards."""
    m = short_f32.model
    mix = short_batch(2561).cuda()
    out = P.apply_model(m, mix, shifts=0)
    assert out.shape == (4, 4, 2, 2561) and bool(torch.isfinite(out).all())
    for b in range(4):
        alone = P.apply_model(m, mix[b:b + 1], shifts=0)
        assert torch.equal(alone[0], out[b]), f"track {b}: {float((alone[0] - out[b]).abs().max()):.3e}"
    m.check()
