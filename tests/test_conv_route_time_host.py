"""The route of the time branch's strided and transposed convs without a GPU: `tools/conv_route_table.hip time` prints `name
route tile plain` for tenc[1 .. 3].conv (M = 96: a 96-row layer; M = 192 / 384: 192-row layers on 96-row images) and
tdec[0 .. 2].convtr (M = 768 / 384 / 192: 192-row layers) of a 7.8 s segment and for a 128-row layer of each kind, each
under-filled and filled, with and without a split image, as the engine describes them -- `dma_time` set; the transposed convs'
columns 0 .. Lv on a pitch that is a multiple of 4.

Expectations, from conv_route read top to bottom: with an image route 11 on the 192-row tile when its workgroups fill the chip,
else on the 96-row tile of the same image (a 128-row layer: the 64-row tile that reads the 128-row image); without an image, with
mi_set_split_bf16(0) and under MI_X6_MODE=1 the table-driven native kernel on the layer's own tile; without the caller's promise or on
a pitch that is no multiple of 4 the gather table in front of the split loop (route 4), which has no 192-row tile for this epilogue.
The tool's output without the argument is what tests/test_conv_route_host.py compares."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "demucs_amd", "csrc")
TABLE, X6, TIME_X6 = 0, 4, 11     # enum mi_conv_route

OWN_TILE = {768: 128, 384: 128, 192: 96, 128: 128}
ENC_TILE = {96: 96, 192: 96, 384: 128, 128: 128}      # the layer's own tile
DEFAULT = {
    # a 96-row layer has no smaller tile; the 192-row layers: 96 rows under-filled, 192 filled; the 128-row layer: 64 / 128
    **{f"time_enc_M{M}_under+x6": (TIME_X6, 64 if M == 128 else 96, 0) for M in ENC_TILE},
    **{f"time_enc_M{M}_filled+x6": (TIME_X6, {96: 96, 128: 128}.get(M, 192), 0) for M in ENC_TILE},
    **{f"time_enc_M{M}_{fill}": (TABLE, tile, 0) for M, tile in ENC_TILE.items() for fill in ("under", "filled")},
    "time_enc_M384_nopromise+x6": (X6, 96, 0),
    **{f"time_tr_M{M}_under+x6": (TIME_X6, 64 if M == 128 else 96, 0) for M in OWN_TILE},
    **{f"time_tr_M{M}_filled+x6": (TIME_X6, 128 if M == 128 else 192, 0) for M in OWN_TILE},
    **{f"time_tr_M{M}_{fill}": (TABLE, tile, 0) for M, tile in OWN_TILE.items() for fill in ("under", "filled")},
    "time_tr_M768_nopromise+x6": (X6, 96, 0), "time_tr_M768_pitch1345+x6": (X6, 96, 0), "time_tr_M768_skip+x6": (TIME_X6, 192, 0),
}
WITH_IMAGE = [k for k in DEFAULT if k.endswith("+x6")]


def _own(name):
    return (ENC_TILE if name.startswith("time_enc") else OWN_TILE)[int(name.split("_")[2][1:])]


CHANGES = {
    "MI_SMALL_TILE=0": {**{f"time_tr_M{M}_under+x6": (TIME_X6, 128 if M == 128 else 192, 0) for M in OWN_TILE},
                        **{f"time_enc_M{M}_under+x6": (TIME_X6, 128 if M == 128 else 192, 0) for M in ENC_TILE if M != 96}},
    "MI_X6_MODE=1": {k: (TABLE, _own(k), 0) for k in WITH_IMAGE},
}
NOSPLIT = {k: (TABLE, _own(k), 0) for k in WITH_IMAGE}


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("conv_route_time") / "conv_route_table")
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


def test_default_time_rows(table):
    assert rows(table, None, "time") == DEFAULT


@pytest.mark.parametrize("switch", sorted(CHANGES))
def test_switch_changes_only_its_time_rows(table, switch):
    assert set(CHANGES[switch]) <= set(DEFAULT) and all(DEFAULT[k] != v for k, v in CHANGES[switch].items())
    assert rows(table, dict([switch.split("=")]), "time") == {**DEFAULT, **CHANGES[switch]}


def test_split_off_time_rows(table):
    assert rows(table, None, "time", "nosplit") == {**DEFAULT, **NOSPLIT}
    assert rows(table, None, "nosplit", "time") == {**DEFAULT, **NOSPLIT}


def test_other_rows_do_not_name_the_new_route(table):
    """without the argument the tool prints none of the time rows and no descriptor of the older tests takes route 11"""
    got = rows(table)
    assert not any(name.startswith("time_tr") for name in got)
    assert not any(isinstance(v, tuple) and v[0] == TIME_X6 for v in got.values())
