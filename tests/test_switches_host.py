"""The environment switches are read in ONE place (demucs_amd/csrc/switches.hip) and documented in one table:
the source holds no other environment read, no packing scope kept as mutable state, and table and reader name the same variables.
Text checks only: no GPU, no library."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "demucs_amd", "csrc")
READER = "switches.hip"


def _sources():
    return {os.path.basename(p): open(p).read() for p in sorted(glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.h")))}


def test_one_file_reads_the_environment():
    src = _sources()
    assert READER in src and "getenv(" in src[READER]
    others = [name for name, text in src.items() if name != READER and re.search(r"getenv\s*\(|\benviron\b|secure_getenv", text)]
    assert others == [], others


def test_no_static_initialised_from_the_environment():
    """No function keeps its own once-only copy of a switch: a `static const` initialised from the environment or from switches().
    The reader's own `static const Switches` (built by its one function) is the only static that holds switch values."""
    bad = []
    for name, text in _sources().items():
        for n, line in enumerate(text.splitlines(), 1):
            if re.search(r"\bstatic\s+const\b", line) and re.search(r"getenv|\bswitches\(\)", line):
                bad.append(f"{name}:{n}: {line.strip()}")
    assert bad == [], bad
    assert len(re.findall(r"\bstatic\s+const\s+Switches\b", _sources()[READER])) == 1


def test_conv_launchers_do_not_ask_the_switches():
    """Which conv kernel runs is conv_route's answer (conv_route.hip: host code only); the files that hold the kernels and their
    launchers take it and never look at a switch."""
    src = _sources()
    asking = [name for name in ("gemm_conv.hip", "gemm_x6.hip", "gemm_half.hip", "gemm_tap.hip") if "switches()" in src[name]]
    assert asking == [], asking
    assert "switches()" in src["conv_route.hip"]
    assert "__global__" not in src["conv_route.hip"] and "hipLaunchKernelGGL" not in src["conv_route.hip"]


def test_split_scope_is_not_mutable_state():
    hits = [name for name, text in _sources().items() if re.search(r"split_linears|split_taps|split_rows", text)]
    assert hits == [], hits


def test_switch_table_matches_the_reader():
    """The backticked MI_* variables in the first column of INTEGRATION.md's switch table are exactly the variables the reader's
    source names, plus MI_NO_TAIL_OVERLAP (read by Python)."""
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    lines = doc.splitlines()
    start = next(i for i, line in enumerate(lines) if line.startswith("| variable | values | effect | tested by |"))
    table = []
    for line in lines[start + 2:]:
        if not line.startswith("|"):
            break
        table.append(line)
    documented = [re.match(r"\|\s*`(MI_[A-Z0-9_]+)`\s*\|", line).group(1) for line in table]
    assert len(documented) == len(set(documented)), "a variable has two rows"
    assert all(len(line.strip().strip("|").split("|")) >= 4 for line in table)
    reader = open(os.path.join(CSRC, READER)).read()
    read = set(re.findall(r'(?:present|nonzero|getenv)\("(MI_[A-Z0-9_]+)"', reader))
    assert len(read) >= 29
    assert set(documented) == read | {"MI_NO_TAIL_OVERLAP"}, set(documented) ^ (read | {"MI_NO_TAIL_OVERLAP"})
    # mi_debug_switches prints one line per variable the reader parses
    printed = set(re.findall(r"(MI_[A-Z0-9_]+)=%", reader))
    assert printed == read, printed ^ read
    # the one Python-side switch has one reader too
    py = {p: open(p).read() for p in glob.glob(os.path.join(ROOT, "demucs_amd", "*.py"))}
    assert [os.path.basename(p) for p, text in py.items() if '"MI_NO_TAIL_OVERLAP"' in text] == ["hdemucs.py"]
    assert "MI_H_TWO_STREAMS" not in doc
