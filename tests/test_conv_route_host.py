"""The conv route table without a GPU: tools/conv_route_table.hip links demucs_amd/csrc/conv_route.hip and switches.hip alone and
prints `name route tile plain` for each of its descriptors, or the message conv_validate refuses it with.  Built once, then run in
fresh processes: with no MI_* variable, with each switch conv_route reads, and with the split-bf16 loops off.

Expectations.  Float32 rows: what tests/test_gpu_conv_route.py (rows A - I) and tests/test_gpu_x6_tile192.py (the tile_m = 192 rows)
assert on the GPU; under a switch, the decision list of conv_route read top to bottom without the routes the switch removes.  Half
rows: the rules of the launchers as they stood in gemm_half.hip before the decision moved -- operand image with SCALE|RES[|STATS]:
the 3-stage kernel, 256 rows where Mpad % 256 == 0 else 128 (MI_IMG256=1: SCALE|RES alone on the 512-thread kernel where
Mpad % 256 == 0); LN|HEADS and LN|GELU|IMG: the 512-thread kernel; no image: the register-staged kernel, 256 rows for a plain
LINEAR layer of 128-row tiles with Mpad % 256 == 0 unless MI_HALF_TILE256=0 -- which are the kernel-name sets
tests/test_gpu_half_linear.py::test_switch_route sees (family = route, TM = 4 / <2, 2, 4, 2> = 256 rows)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "demucs_amd", "csrc")
TABLE, DMA, DMATAP, DMAROW, X6, HALF, TAP_HALF, TAP_X6, ROWS_X6, HALF_IMG, HALF_IMG256 = range(11)   # enum mi_conv_route

BIG, SMALL = 200 * 128, 60 * 128
HEADS_MSG, IMG_MSG = "MI_FLAG_HEADS needs", "MI_FLAG_IMG needs"

DEFAULT = {
    # tests/test_gpu_conv_route.py, with and without a split image
    "A+x6": (X6, 64, 1), "B+x6": (X6, 128, 1), "C+x6": (TAP_X6, 96, 0), "D+x6": (X6, 96, 0), "E+x6": (TAP_X6, 64, 0), "F+x6": (TAP_X6, 64, 0),
    "G+x6": (ROWS_X6, 64, 0), "H+x6": (ROWS_X6, 96, 0), "I+x6": (X6, 128, 0),
    "A": (TABLE, 64, 1), "B": (DMA, 128, 1), "C": (DMATAP, 96, 0), "D": (TABLE, 96, 0), "E": (DMATAP, 128, 0), "F": (DMATAP, 96, 0),
    "G": (DMAROW, 128, 0), "H": (DMAROW, 96, 0), "I": (TABLE, 128, 0),
    # tests/test_gpu_x6_tile192.py: filled -> 192, under-filled -> 96 (the threshold counts 192-row tiles)
    **{f"t192_{kind}_M{M}_N{N}": (route, tile, plain)
       for kind, route, plain in (("linear", X6, 1), ("tap", TAP_X6, 0), ("enc", ROWS_X6, 0))
       for M, N, tile in ((192, 200 * 128, 192), (192, 199 * 128, 96), (384, 100 * 128, 192), (384, 99 * 128, 96))},
    "t192_linear_M1536_N3000": (X6, 96, 1), "t192_linear_M1536_N3200": (X6, 192, 1), "t192_linear_M384_flags0": (X6, 96, 1),
    f"t192_linear_M384_N{BIG}_noimage": (DMA, 128, 1), f"t192_linear_M192_N{BIG}_noimage": (TABLE, 96, 1),
    f"t192_linear_M384_N{SMALL}_noimage": (TABLE, 64, 1), f"t192_tap_M384_N{BIG}_noimage": (DMATAP, 128, 0),
    f"t192_tap_M384_N{SMALL}_noimage": (DMATAP, 96, 0), f"t192_enc_M192_N{BIG}_noimage": (DMAROW, 96, 0),
    "t192_M256": "tile_m 192 needs", "t192_M96": "tile_m 192 needs", "t192_M192_Mpad384": "tile_m 192 needs",
    # the half rules at M = 120 (Mpad 128), 128, 256, 384, 512
    **{f"half_xh_{fam}_M{M}": (HALF_IMG, 256 if M % 256 == 0 else 128, 1) for fam in ("sr", "srs") for M in (120, 128, 256, 384, 512)},
    **{f"half_xh_heads_M{M}": HEADS_MSG for M in (120, 128, 256, 384)}, "half_xh_heads_M512": (HALF_IMG256, 256, 1),
    **{f"half_xh_ffn_M{M}": (HALF_IMG256, 256, 1) for M in (120, 128, 256, 384, 512)},
    **{f"half_reg_M{M}": (HALF, 256 if M % 256 == 0 else 128, 1) for M in (120, 128, 256, 384, 512)},
    "dconv_k3": (DMATAP, 32, 0), "half_encoder_M256": (HALF, 128, 0), "half_wtap_M128": (TAP_HALF, 128, 0),
    # test_refusals_launch_nothing: five refused by conv_validate, four by the launchers' operand checks (they have a route)
    "refuse_xh_gelu": "not instantiated for LINEAR flags 1", "refuse_ffn_M128": (HALF_IMG256, 256, 1), "refuse_ffn_K36": (HALF_IMG256, 256, 1),
    "refuse_heads_narrow_image": (HALF_IMG256, 256, 1), "refuse_heads_M256": HEADS_MSG, "refuse_heads_frame": HEADS_MSG,
    "refuse_heads_xh_off": (HALF_IMG256, 256, 1), "refuse_heads_yh_off": HEADS_MSG, "refuse_ffn_yh_off": IMG_MSG,
}

T192_IMAGE = [(kind, M, N) for kind in ("linear", "tap", "enc") for M, N in ((192, 200 * 128), (192, 199 * 128), (384, 100 * 128), (384, 99 * 128))]
# mi_set_split_bf16(0): every row with an image answers as the same layer without one (a tile_m = 192 layer: as tile_m = 0)
NOSPLIT = {**{f"{r}+x6": DEFAULT[r] for r in "ABCDEFGHI"},
           **{f"t192_{kind}_M{M}_N{N}": {("linear", 192): (TABLE, 96, 1), ("linear", 384): (DMA, 128, 1), ("tap", 192): (DMATAP, 96, 0),
                                          ("tap", 384): (DMATAP, 128, 0), ("enc", 192): (DMAROW, 96, 0), ("enc", 384): (DMAROW, 128, 0)}[(kind, M)]
              for kind, M, N in T192_IMAGE},
           "t192_linear_M1536_N3000": (DMA, 128, 1), "t192_linear_M1536_N3200": (DMA, 128, 1), "t192_linear_M384_flags0": (DMA, 128, 1)}

# what each switch changes, against DEFAULT
CHANGES = {
    "MI_IMG256=1": {"half_xh_sr_M256": (HALF_IMG256, 256, 1), "half_xh_sr_M512": (HALF_IMG256, 256, 1)},
    "MI_HALF_TILE256=0": {"half_reg_M256": (HALF, 128, 1), "half_reg_M512": (HALF, 128, 1)},
    # no small-batch tiles: every under-filled layer keeps its own tile, the 192-row layers the 192-row tile
    "MI_SMALL_TILE=0": {"A+x6": (X6, 128, 1), "E+x6": (TAP_X6, 128, 0), "F+x6": (TAP_X6, 128, 0), "G+x6": (ROWS_X6, 128, 0), "A": (DMA, 128, 1),
                        "F": (DMATAP, 128, 0), "t192_linear_M1536_N3000": (X6, 192, 1),
                        **{f"t192_{kind}_M{M}_N{N}": (DEFAULT[f"t192_{kind}_M{M}_N{N}"][0], 192, DEFAULT[f"t192_{kind}_M{M}_N{N}"][2])
                           for kind, M, N in T192_IMAGE if DEFAULT[f"t192_{kind}_M{M}_N{N}"][1] == 96},
                        f"t192_linear_M384_N{SMALL}_noimage": (DMA, 128, 1), f"t192_tap_M384_N{SMALL}_noimage": (DMATAP, 128, 0)},
    # the split loop for plain layers only: a non-plain layer with an image has no route but the table-driven gather (the native DMA
    # loaders take layers without an image), on the layer's own tile
    "MI_X6_MODE=1": {"C+x6": (TABLE, 96, 0), "D+x6": (TABLE, 96, 0), "E+x6": (TABLE, 128, 0), "F+x6": (TABLE, 128, 0), "G+x6": (TABLE, 128, 0),
                     "H+x6": (TABLE, 96, 0), "I+x6": (TABLE, 128, 0),
                     **{f"t192_{kind}_M{M}_N{N}": (TABLE, 96 if M == 192 else 128, 0) for kind, M, N in T192_IMAGE if kind != "linear"}},
    "MI_NO_DMA=1": {"B": (TABLE, 128, 1), f"t192_linear_M384_N{BIG}_noimage": (TABLE, 128, 1)},
    # no shifted-run taps: with an image the gather table in front of the split loop (no 64-row tile for a non-linear layer, no
    # 192-row tile for a GLU conv behind the table), without one the table-driven native kernel on the layer's tile
    "MI_NO_DMA_TAP=1": {"C+x6": (X6, 96, 0), "E+x6": (X6, 128, 0), "F+x6": (X6, 128, 0), "C": (TABLE, 96, 0), "E": (TABLE, 128, 0), "F": (TABLE, 128, 0),
                        **{f"t192_tap_M{M}_N{N}": (X6, 96, 0) for kind, M, N in T192_IMAGE if kind == "tap"},
                        f"t192_tap_M384_N{BIG}_noimage": (TABLE, 128, 0), f"t192_tap_M384_N{SMALL}_noimage": (TABLE, 128, 0), "dconv_k3": (TABLE, 32, 0)},
    "MI_NO_DMA_ROWS=1": {"G+x6": (X6, 128, 0), "H+x6": (X6, 96, 0), "G": (TABLE, 128, 0), "H": (TABLE, 96, 0),
                         **{f"t192_enc_M{M}_N{N}": (X6, 96, 0) for kind, M, N in T192_IMAGE if kind == "enc"},
                         f"t192_enc_M192_N{BIG}_noimage": (TABLE, 96, 0)},
    "MI_NO_DMA_DCONV=1": {"dconv_k3": (TABLE, 32, 0)},
}


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("conv_route") / "conv_route_table")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-std=c++17", "-O1", os.path.join(ROOT, "tools", "conv_route_table.hip"),
                        os.path.join(CSRC, "conv_route.hip"), os.path.join(CSRC, "switches.hip"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def rows(exe, env=None, *args):
    e = {k: v for k, v in os.environ.items() if not k.startswith("MI_")}
    e.update(env or {})
    r = subprocess.run([exe, *args], env=e, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr[-2000:]
    out = {}
    for line in r.stdout.splitlines():
        name, rest = line.split(" ", 1)
        assert name not in out, name
        out[name] = rest if rest.startswith("invalid:") else tuple(int(v) for v in rest.split())
    return out


def check(got, want):
    assert sorted(got) == sorted(want)
    bad = []
    for name, w in want.items():
        g = got[name]
        if not (g.startswith("invalid:") and w in g if isinstance(w, str) and isinstance(g, str) else g == w):
            bad.append((name, g, w))
    assert bad == [], bad


def test_default_table(table):
    check(rows(table), DEFAULT)


@pytest.mark.parametrize("switch", sorted(CHANGES))
def test_switch_changes_only_its_rows(table, switch):
    assert set(CHANGES[switch]) <= set(DEFAULT) and all(DEFAULT[k] != v for k, v in CHANGES[switch].items())
    check(rows(table, dict([switch.split("=")])), {**DEFAULT, **CHANGES[switch]})


def test_split_off(table):
    assert set(NOSPLIT) <= set(DEFAULT)
    check(rows(table, None, "nosplit"), {**DEFAULT, **NOSPLIT})
