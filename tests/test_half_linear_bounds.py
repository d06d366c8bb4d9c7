"""The bound constants of test_gpu_half_linear.py against the cases that file runs: RESTATED must have one entry per (family,
operand type, K) of `family_cases()`, and each entry must still be the largest float32-restatement distance over the family's
cases.  Runs on the CPU.  The restatement's figures depend a little on the host's float32 matmul (kernel-level parity:
factors up to 2.4 have been seen between hosts for a single case of another file), so an entry may differ from this host's figure
by a factor of 2 either way before a stale table is reported: a changed case list or seed moves it by more or drops a key."""
import test_gpu_half_linear as t


def test_restated_table_matches_the_cases():
    flags_of = {v: k for k, v in t.FAMILY.items()}
    now = {}
    for mode in t.MODES:
        for fam, K, B, T, M in t.family_cases():
            o = t.operands(mode, K, B, T, M)
            key = (fam, mode, K)
            now[key] = max(now.get(key, 0.0), t.want_of(o, flags_of[fam])[1])
    assert set(now) == set(t.RESTATED), sorted(set(now) ^ set(t.RESTATED))
    off = {k: (t.RESTATED[k], v) for k, v in now.items() if not 0.5 <= v / t.RESTATED[k] <= 2.0}
    assert not off, off
