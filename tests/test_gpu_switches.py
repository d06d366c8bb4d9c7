"""The environment switches as the library parses them (mi_debug_switches), and the launch census: the profiler rows and launch
counts of one B = 1 forward per engine, compute mode and half-mode switch group, against tests/golden/launch_census.json
(recorded before the switches, the forward plans and the split scope were each given one place of decision)."""
import json
import os
import subprocess
import sys

import pytest

from test_gpu_x6_linear import _ENGINE

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_PRINT = r"""
import ctypes
from demucs_amd import _lib
lib = _lib.load()
n = lib.mi_debug_switches(None, 0)
buf = ctypes.create_string_buffer(n + 1)
assert lib.mi_debug_switches(buf, n + 1) == n
short = ctypes.create_string_buffer(8)
assert lib.mi_debug_switches(short, 8) == n and short.value == buf.value[:7]
print(buf.value.decode(), end="")
"""

DEFAULTS = {
    "MI_NO_DMA": "0", "MI_NO_DMA_TAP": "0", "MI_NO_DMA_ROWS": "0", "MI_NO_DMA_DCONV": "0", "MI_SMALL_TILE": "1", "MI_MGROUPS": "0",
    "MI_X6_MODE": "0", "MI_X6": "default", "MI_NO_TAP_IMAGE": "0", "MI_NO_ENC_IMAGE": "0", "MI_NO_DCONV_TIME": "0",
    "MI_NO_LIN2_STATS": "0", "MI_NO_FFN_IMAGE": "0", "MI_NO_QKV_HEADS": "0", "MI_NO_INPUT_IMAGE": "0", "MI_ONE_STREAM": "0",
    "MI_DEBUG_SYNC": "0", "MI_SIDE_PRIO": "normal", "MI_H_NO_DEEP_TAP": "0", "MI_H_NO_LAST_TAP": "0", "MI_H_ONE_STREAM": "0",
    "MI_LSTM_STEPS": "0", "MI_LSTM_WRITE_THROUGH": "0", "MI_LSTM_DEBUG": "0", "MI_TRANSPOSE_TILES": "0", "MI_ISTFT_SPLIT": "0",
    "MI_DCONV_ROW": "wave", "MI_IMG256": "0", "MI_HALF_TILE256": "1",
}
# every variable at a non-default value -> what the library must report
NON_DEFAULT_ENV = dict({name: "1" for name in DEFAULTS}, MI_X6="0", MI_SMALL_TILE="0", MI_HALF_TILE256="0", MI_LSTM_STEPS="1",
                       MI_DCONV_ROW="lds", MI_SIDE_PRIO="low", MI_TRANSPOSE_TILES="1")
FLIPPED = dict({name: "1" for name in DEFAULTS}, MI_X6="none", MI_SMALL_TILE="0", MI_HALF_TILE256="0", MI_DCONV_ROW="lds",
               MI_SIDE_PRIO="low", MI_TRANSPOSE_TILES="7")


def _clean_env(extra):
    env = {k: v for k, v in os.environ.items() if not k.startswith("MI_")}
    env.update(extra, PYTHONPATH=ROOT)
    return env


def _switches(extra):
    r = subprocess.run([sys.executable, "-c", _PRINT], env=_clean_env(extra), capture_output=True, text=True, cwd=ROOT, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    lines = r.stdout.splitlines()
    got = dict(line.split("=", 1) for line in lines)
    assert len(got) == len(lines), "a variable is printed twice"
    return got


def test_clean_environment_reports_every_default():
    assert _switches({}) == DEFAULTS


def test_every_switch_flips():
    got = _switches(NON_DEFAULT_ENV)
    assert got == FLIPPED
    assert all(got[name] != DEFAULTS[name] for name in DEFAULTS)


def test_parsing_corners():
    """MI_LSTM_STEPS needs a non-zero number, MI_X6 is tri-state, MI_X6_MODE recognises the value 1 only; the first letter decides
    MI_SIDE_PRIO and MI_DCONV_ROW; MI_TRANSPOSE_TILES above 1 is a mask."""
    got = _switches({"MI_LSTM_STEPS": "0", "MI_X6": "1", "MI_X6_MODE": "2"})
    assert got == dict(DEFAULTS, MI_X6="all")
    got = _switches({"MI_SIDE_PRIO": "high", "MI_DCONV_ROW": "wave", "MI_TRANSPOSE_TILES": "6", "MI_IMG256": "0", "MI_SMALL_TILE": "2"})
    assert got == dict(DEFAULTS, MI_SIDE_PRIO="high", MI_TRANSPOSE_TILES="6")


# ---- launch census ---------------------------------------------------------------------------------------------------
GROUP_A = {"MI_NO_INPUT_IMAGE": "1", "MI_NO_ENC_IMAGE": "1", "MI_NO_LIN2_STATS": "1", "MI_ONE_STREAM": "1"}
GROUP_B = {"MI_NO_QKV_HEADS": "1", "MI_NO_TAP_IMAGE": "1", "MI_NO_DCONV_TIME": "1"}
GROUP_C = {"MI_NO_FFN_IMAGE": "1"}
H_SWITCHES = {"MI_H_NO_DEEP_TAP": "1", "MI_H_NO_LAST_TAP": "1", "MI_H_ONE_STREAM": "1"}
CENSUS = {          # entry of launch_census.json -> (engine, compute mode, environment)
    "htdemucs_f32": ("htdemucs", "f32", {}), "htdemucs_bf16": ("htdemucs", "bf16", {}), "htdemucs_f16": ("htdemucs", "f16", {}),
    "hdemucs_f32": ("hdemucs", "f32", {}), "hdemucs_f16": ("hdemucs", "f16", {}),
    "htdemucs_bf16_group_a": ("htdemucs", "bf16", GROUP_A), "htdemucs_bf16_group_b": ("htdemucs", "bf16", GROUP_B),
    "htdemucs_bf16_group_c": ("htdemucs", "bf16", GROUP_C), "hdemucs_f16_h_switches": ("hdemucs", "f16", H_SWITCHES),
}


@pytest.fixture(scope="module")
def census():
    return json.load(open(os.path.join(ROOT, "tests", "golden", "launch_census.json")))


def test_census_file_lists_every_configuration(census):
    assert set(census) == set(CENSUS)


@pytest.mark.parametrize("tag", list(CENSUS))
def test_launch_census_unchanged(census, tmp_path, tag):
    """HTDemucs (one segment) / HDemucs (channels = 48, 3 s) at B = 1 with the profiler on: the sorted (row name, launches) list
    equals the recorded one, entry for entry."""
    engine, dtype, extra = CENSUS[tag]
    out = str(tmp_path / tag)
    r = subprocess.run([sys.executable, "-c", _ENGINE, out, "default", dtype, engine], env=_clean_env(extra), capture_output=True,
                       text=True, cwd=ROOT, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    rows = sorted([line.rsplit(" ", 1)[0], int(line.rsplit(" ", 1)[1])] for line in open(out + ".txt"))
    assert rows == census[tag]
