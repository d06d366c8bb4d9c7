"""The bound constants of test_gpu_tap_image.py against the cases that file runs: RESTATED must have one entry per (family,
operand type, K) of `family_cases()`, and each entry must still be the largest float32-restatement distance over the family's
cases.  Runs on the CPU.  The restatement's figures depend a little on the host's float32 convolution (kernel-level
parity), so an entry may differ from this host's figure by a factor of 2 either way before a stale table is reported: a changed
case list or seed moves it by more or drops a key.  Also the image helpers the GPU file builds its operands with."""
import torch

import test_gpu_tap_image as t
from gpu_helpers import image_of, image_to


def test_restated_table_matches_the_cases():
    now = {}
    for mode in t.MODES:
        for L, fam in t.family_cases(mode):
            key = (fam, mode, L.K)
            now[key] = max(now.get(key, 0.0), t.want_of(L, fam)[1])
    assert set(now) == set(t.RESTATED), sorted(set(now) ^ set(t.RESTATED))
    off = {k: (t.RESTATED[k], v) for k, v in now.items() if not 0.5 <= v / t.RESTATED[k] <= 2.0}
    assert not off, off


def test_operands_are_exact_in_both_types():
    for mode in t.MODES:
        for L, _ in t.family_cases(mode)[:-2]:           # the chain's consumers read computed values, rounded to ONE type
            for v in (L.x, L.W2d):
                assert torch.equal(v.bfloat16().double(), v) and torch.equal(v.half().double(), v), L.name


def test_image_layout_and_its_inverse():
    v = torch.arange(2 * 16 * 3 * 5, dtype=torch.float64).reshape(2, 16, 3, 5)
    img = image_of(v)
    assert img.shape == (2, 30, 8)
    for b, c, r, w in ((0, 0, 0, 0), (1, 9, 2, 4), (0, 15, 1, 3), (1, 8, 0, 0)):
        assert img[c // 8, b * 15 + r * 5 + w, c % 8] == v[b, c, r, w]
    slack = torch.cat([img, torch.full((2, 4, 8), -1.0, dtype=torch.float64)], 1)
    assert torch.equal(image_to(slack, 2, 3, 5), v)
