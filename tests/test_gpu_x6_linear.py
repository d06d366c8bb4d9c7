"""The float32 transformer linears on the split-bf16 main loop (gemm_x6.hip: fp32 operands as three exact bf16 terms, six bf16
MFMA products, fp32 accumulate), which the float32 htdemucs engine takes by default.

  * every epilogue flag set the transformer uses (LN, LN|GELU, SCALE|RES, SCALE|RES|STATS) against float64;
  * the native LDS-DMA tile (gemm_conv.hip conv_gemm_dma_kernel) on each of its seven flag sets against float64 and, bit for
    bit, against the table-driven route;
  * the same products in the same k order on every tile the launch heuristics can pick: the 128-row tile, the 64-row
    small-batch tile reading the 128-row image, and a 64-row image, bit for bit; B = 1 against a batched call;
  * the engine default (split route), MI_X6=0 and the process-wide switch mi_set_split_bf16(0) (native fp32 kernels), which
    demucs_amd/distributed.py sets for ranks that share a GPU.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from demucs_amd import _lib
from gpu_helpers import EPI_LINEAR, FLAG_GELU, FLAG_RES, FLAG_SCALE, conv_call, ktab, maxerr, pack_vec, pack_w

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAG_LN, FLAG_STATS = 32, 256
ROUTE_X6, ROUTE_DMA = 4, 1          # mi_debug_last_conv_route: split-bf16 loop, native fp32 LDS-DMA linear tile
ROUTE_TABLE = 0                     # the register-staged native kernel behind the gather table


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return _lib.load()


def rnd(*shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g, dtype=torch.float64) * scale


def _linear(flags, B, Tn, K, seed, tile_m=128, x6=True, plain=1):
    """One transformer linear (M = 512) on tokens (B, K, Tn) -> (y, stats or None, float64 expectation)."""
    M = 512
    x = rnd(B, K, Tn, seed=seed)
    W, b = rnd(M, K, seed=seed + 1, scale=K ** -0.5), rnd(M, seed=seed + 2, scale=0.2)
    wt, bias, _, Mpad, _, Kpad, _ = pack_w(W, b, tile=tile_m)
    kw = dict(x6=x6, wt=wt, M=M, Mpad=Mpad, K=K, Kpad=Kpad, ktab=ktab(K, 1, 1, 1, 1, 0, 0, Tn, Tn, Kpad), x=x.float().cuda(),
              x_bstride=K * Tn, B=B, D1=1, D2=Tn, O1=1, O2=Tn, S1=1, S2=1, plain=plain, epi=EPI_LINEAR, flags=flags, bias=bias,
              y_bstride=M * Tn, y_cstride=Tn, tile_m=tile_m)
    acc = torch.einsum("mk,bkt->bmt", W, x)
    if flags & FLAG_LN:
        # the LayerNorm fold: W already carries diag(ln_w); the epilogue applies rstd * (W x - mean * c1) + b per token
        xf = x.float().double()
        mean, rstd = xf.mean(1), 1.0 / torch.sqrt(xf.var(1, unbiased=False) + 1e-5)
        c1 = W.float().double().sum(1)
        kw["pro_stats"] = torch.stack([mean, rstd], -1).reshape(B * Tn, 2).float().cuda().contiguous()
        kw["scale"] = pack_vec(c1, Mpad)
        stf = kw["pro_stats"].double().cpu().reshape(B, Tn, 2)
        want = stf[:, None, :, 1] * (acc - stf[:, None, :, 0] * c1.float().double()[None, :, None]) + b[None, :, None]
    else:
        want = acc + b[None, :, None]
    if flags & FLAG_GELU:
        want = torch.nn.functional.gelu(want)
    if flags & FLAG_SCALE:
        g = rnd(M, seed=seed + 3)
        kw["scale"] = pack_vec(g, Mpad)
        want = want * g[None, :, None]
    if flags & FLAG_RES:
        r = rnd(B, M, Tn, seed=seed + 4)
        kw["res"] = r.float().cuda()
        want = want + r
    stats = None
    if flags & FLAG_STATS:
        stats = torch.zeros(B, 32, 2, dtype=torch.float64, device="cuda")
        kw["stats"] = stats
    y = torch.empty(B, M, Tn, device="cuda")
    conv_call(y=y, **kw)
    return y, stats, want


FLAG_SETS = {"ln": FLAG_LN, "ln_gelu": FLAG_LN | FLAG_GELU, "scale_res": FLAG_SCALE | FLAG_RES,
             "scale_res_stats": FLAG_SCALE | FLAG_RES | FLAG_STATS}


@pytest.mark.parametrize("name", list(FLAG_SETS))
def test_x6_linear_epilogues_match_float64(lib, name):
    """qkv / q / kv projections (LN), lin1 (LN|GELU), out_proj (SCALE|RES), lin2 (SCALE|RES|STATS, K = 2048): float32-level
    error against float64 on the split route, no worse than three times the native fp32 kernels' error on the same layer."""
    flags = FLAG_SETS[name]
    K = 2048 if flags & FLAG_STATS else 512
    B, Tn = 2, 3300                      # 52 column tiles x 4 row tiles: the 128-row tile
    y, stats, want = _linear(flags, B, Tn, K, seed=100)
    assert lib.mi_debug_last_conv_route() == ROUTE_X6
    err = maxerr(y, want)
    y_nat, _, _ = _linear(flags, B, Tn, K, seed=100, x6=False)
    assert lib.mi_debug_last_conv_route() == ROUTE_DMA
    err_nat = maxerr(y_nat, want)
    print(f"{name}: split {err:.2e}, native fp32 {err_nat:.2e}")
    assert err < 3e-5 and err <= 3 * err_nat + 2e-6
    if stats is not None:
        got = stats.sum(1).cpu()
        ref = torch.stack([y.double().sum((1, 2)).cpu(), (y.double() ** 2).sum((1, 2)).cpu()], 1)
        assert ((got - ref).abs() / ref.abs().clamp_min(1.0)).max().item() < 2e-6, (got, ref)


@pytest.mark.parametrize("name", list(FLAG_SETS))
def test_x6_linear_64_and_128_row_tiles_bit_identical(lib, name):
    """The 128-row tile and a 64-row weight image: the same products in the same k order, equal bit for bit."""
    flags = FLAG_SETS[name]
    K = 2048 if flags & FLAG_STATS else 512
    y128, _, _ = _linear(flags, 2, 3300, K, seed=200)
    y64, _, _ = _linear(flags, 2, 3300, K, seed=200, tile_m=64)
    assert lib.mi_debug_last_conv_route() == ROUTE_X6
    assert torch.equal(y128, y64)


@pytest.mark.parametrize("name", list(FLAG_SETS))
def test_x6_linear_single_item_equals_batched(lib, name):
    """The first item of a batched call (128-row tile), run alone (B = 1: 26 x 4 tiles < 200 workgroups, so the 64-row small-batch
    tile reading the 128-row image), gives the same bits as in the batch."""
    flags = FLAG_SETS[name]
    K = 2048 if flags & FLAG_STATS else 512
    M, B, Tn = 512, 2, 3300
    x = rnd(B, K, Tn, seed=300)
    W, b = rnd(M, K, seed=301, scale=K ** -0.5), rnd(M, seed=302, scale=0.2)
    wt, bias, _, Mpad, _, Kpad, _ = pack_w(W, b, tile=128)
    st = torch.stack([x.mean(1), 1.0 / torch.sqrt(x.var(1, unbiased=False) + 1e-5)], -1).float()      # (B, Tn, 2)
    r = rnd(B, M, Tn, seed=303).float()
    sc = pack_vec(rnd(M, seed=304), Mpad)
    outs = []
    for nb in (B, 1):
        kw = dict(x6=True, wt=wt, M=M, Mpad=Mpad, K=K, Kpad=Kpad, ktab=ktab(K, 1, 1, 1, 1, 0, 0, Tn, Tn, Kpad),
                  x=x[:nb].float().cuda().contiguous(), x_bstride=K * Tn, B=nb, D1=1, D2=Tn, O1=1, O2=Tn, S1=1, S2=1, plain=1,
                  epi=EPI_LINEAR, flags=flags, bias=bias, y_bstride=M * Tn, y_cstride=Tn, tile_m=128, scale=sc,
                  res=r[:nb].cuda().contiguous(), pro_stats=st[:nb].reshape(nb * Tn, 2).cuda().contiguous())
        if flags & FLAG_STATS:
            kw["stats"] = torch.zeros(nb, 32, 2, dtype=torch.float64, device="cuda")
        y = torch.empty(nb, M, Tn, device="cuda")
        conv_call(y=y, **kw)
        assert lib.mi_debug_last_conv_route() == ROUTE_X6
        outs.append(y)
    assert torch.equal(outs[0][:1], outs[1])


@pytest.mark.parametrize("name", ["none", "gelu", "res"] + list(FLAG_SETS))
def test_native_dma_linear_tile_equals_the_table_route(lib, name):
    """Every LINEAR flag set conv_gemm_dma_kernel is compiled for (gemm_tile.h dispatch_epilogue), those the transformer does not
    use (none, GELU, RES) included, on the native LDS-DMA tile: against float64 at the file's tolerance and, bit for bit, against
    the same layer declared non-plain, which runs the register-staged kernel behind the gather table (same products, same k
    order).  M = 512 on 6 600 columns: 4 x 52 tiles (the 128-row tile; the last column tile has 72 columns), K = 80: five K
    steps, so the ring wraps."""
    flags = {"none": 0, "gelu": FLAG_GELU, "res": FLAG_RES, **FLAG_SETS}[name]
    y, _, want = _linear(flags, 2, 3300, 80, seed=500, x6=False)
    assert (lib.mi_debug_last_conv_route(), lib.mi_debug_last_conv_tile()) == (ROUTE_DMA, 128)
    assert maxerr(y, want) < 3e-5
    y_tab, _, _ = _linear(flags, 2, 3300, 80, seed=500, x6=False, plain=0)
    assert (lib.mi_debug_last_conv_route(), lib.mi_debug_last_conv_tile()) == (ROUTE_TABLE, 128)
    assert torch.equal(y, y_tab)


def test_split_switch_selects_native_route(lib):
    """mi_set_split_bf16(0) sends a layer WITH a split image to the native fp32 kernel, bit-identical to a call without one."""
    flags = FLAG_SCALE | FLAG_RES | FLAG_STATS
    y_nat, _, _ = _linear(flags, 2, 3300, 2048, seed=400, x6=False)
    old = lib.mi_set_split_bf16(0)
    try:
        y_off, _, _ = _linear(flags, 2, 3300, 2048, seed=400)
        assert lib.mi_debug_last_conv_route() == ROUTE_DMA
    finally:
        lib.mi_set_split_bf16(old)
    assert old == 1
    assert torch.equal(y_off, y_nat)
    _linear(flags, 2, 3300, 2048, seed=400)
    assert lib.mi_debug_last_conv_route() == ROUTE_X6


# ---- the engine's default ------------------------------------------------------------------------
_ENGINE = r"""
import sys
import numpy as np
import torch
from demucs_amd import _lib
from demucs_amd.synth import synth_mix
# argv: output prefix, "default" | "switch", compute mode (f32 | bf16 | f16), engine (htdemucs | hdemucs)
dtype = sys.argv[3] if len(sys.argv) > 3 else "f32"
engine = sys.argv[4] if len(sys.argv) > 4 else "htdemucs"
if sys.argv[2] == "switch":
    _lib.load().mi_set_split_bf16(0)
if engine == "hdemucs":
    from demucs_amd.hdemucs import HDemucs
    from demucs_amd.hdemucs_weights import HDemucsConfig, synthetic_hdemucs_state_dict
    cfg = HDemucsConfig(channels=48, segment=3)
    m = HDemucs(cfg.sources, max_batch=1, compute_dtype=dtype, channels=48, segment=3)
    m.load_state_dict(synthetic_hdemucs_state_dict(cfg, 0))
    length = 3 * cfg.samplerate
else:
    from demucs_amd.htdemucs import HTDemucs
    from demucs_amd.weights import HTDemucsConfig, synthetic_state_dict
    cfg = HTDemucsConfig()
    m = HTDemucs(cfg.sources, max_batch=1, compute_dtype=dtype)
    m.load_state_dict(synthetic_state_dict(cfg, 0))
    length = cfg.segment_length
m.to("cuda").eval()
mix = torch.from_numpy(synth_mix(3, length, "tones"))[None].cuda()
m(mix)
m.profile_begin()
out = m(mix)
rows = m.profile_end()
np.save(sys.argv[1] + ".npy", out.cpu().numpy())
with open(sys.argv[1] + ".txt", "w") as f:
    for r in rows:
        f.write(f"{r['name']} {r['launches']}\n")
"""


def _engine_run(tmp_path, tag, env_extra, mode="default", dtype="f32", engine="htdemucs"):
    env = {k: v for k, v in os.environ.items() if k != "MI_X6"}
    env.update(env_extra, PYTHONPATH=ROOT)
    out = str(tmp_path / tag)
    r = subprocess.run([sys.executable, "-c", _ENGINE, out, mode, dtype, engine], env=env, capture_output=True, text=True, cwd=ROOT, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    rows = {}
    for line in open(out + ".txt"):
        name, n = line.rsplit(" ", 1)
        rows[name] = int(n)
    return np.load(out + ".npy"), rows


def test_engine_default_route_and_switches(tmp_path):
    """float32 htdemucs forward, one fresh process each: by default all 44 transformer linears per forward (self layers: qkv,
    out, lin1, lin2; cross layers: q, kv, out, lin1, lin2; two branches) and nothing else run on the split loop; MI_X6=0 and
    mi_set_split_bf16(0) run them on the native fp32 kernels with bit-identical results; split and native forwards stay within
    the engine's 1e-4 parity target of each other."""
    y_def, rows_def = _engine_run(tmp_path, "default", {})
    x6 = {k: v for k, v in rows_def.items() if k.startswith("conv_gemm_x6")}
    assert x6 and all(k.startswith("conv_gemm_x6<linear,") for k in x6), rows_def
    assert sum(x6.values()) == 44, x6
    y_off, rows_off = _engine_run(tmp_path, "mi_x6_0", {"MI_X6": "0"})
    assert not any(k.startswith("conv_gemm_x6") for k in rows_off), rows_off
    y_sw, rows_sw = _engine_run(tmp_path, "switch", {}, mode="switch")
    assert not any(k.startswith("conv_gemm_x6") for k in rows_sw), rows_sw
    assert np.array_equal(y_sw, y_off)
    d = np.abs(y_def.astype(np.float64) - y_off).max()
    print(f"split vs native fp32 forward: max-abs {d:.3e}")
    assert 0 < d < 1e-4


def _share_worker(rank, world, port, out_path):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from demucs_amd import _lib as L
    from demucs_amd import distributed as D
    torch.cuda.init()
    lib = L.load()
    D._native_kernels_if_gpu_shared(torch.device("cuda"), None)
    on = lib.mi_set_split_bf16(1)
    dist.destroy_process_group()
    with open(f"{out_path}.{rank}", "w") as f:
        f.write(str(on))


def test_ranks_sharing_a_gpu_take_native_kernels(tmp_path):
    """Two ranks on the one GPU of the test box: the sharded scheduler's device exchange switches both engines to the native
    fp32 kernels (tests/test_gpu_distributed.py then runs exactly the kernels it ran before the split loop became default)."""
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    out = str(tmp_path / "flag")
    mp.spawn(_share_worker, args=(2, port, out), nprocs=2, join=True)
    assert [open(f"{out}.{r}").read() for r in range(2)] == ["0", "0"]
