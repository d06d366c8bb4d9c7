"""Host logic of bench.py that needs no GPU: `--gpus N` without a torchrun environment starts its own ranks as a CHILD
`torch.distributed.run` (never an exec), relays rank 0's JSON line and returns the child's exit code."""
import os
import subprocess
import sys
import types

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def test_self_launch_builds_the_torchrun_child(monkeypatch, capsys):
    import bench
    seen = {}

    def fake_run(cmd, **kw):
        seen["cmd"], seen["kw"] = cmd, kw
        return types.SimpleNamespace(returncode=7, stdout='{"metric": "x"}\n')

    monkeypatch.setattr(subprocess, "run", fake_run)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "8", "--steps", "3", "--warmup", "1", "--spawn"])
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    with pytest.raises(SystemExit) as e:
        bench.main()
    assert e.value.code == 7                                   # the child's exit code is the parent's
    cmd = seen["cmd"]
    assert cmd[:3] == [sys.executable, "-m", "torch.distributed.run"]
    assert "--nproc-per-node" in cmd and cmd[cmd.index("--nproc-per-node") + 1] == "8"
    assert cmd[cmd.index("--master-addr") + 1] == "127.0.0.1"
    tail = cmd[cmd.index(os.path.join(ROOT, "bench.py")) + 1:]
    assert tail == ["--gpus", "8", "--steps", "3", "--warmup", "1"]          # --spawn is not handed down
    assert seen["kw"]["env"]["HSA_ENABLE_IPC_MODE_LEGACY"] == "0"            # dmabuf IPC for RCCL on this pool
    assert capsys.readouterr().out.strip() == '{"metric": "x"}'             # the JSON line is relayed


class _FirstDeviceCall(Exception):
    pass


def test_no_self_launch_under_torchrun(monkeypatch):
    """With WORLD_SIZE in the environment (the driver's torchrun form) the process is a rank: it must not spawn."""
    import torch
    import bench
    called = []

    def first_device_call(*a):
        raise _FirstDeviceCall
    monkeypatch.setattr(bench, "self_launch", lambda *a: called.append(a))
    # the rank is stopped at its first device call, with or without a GPU: on a GPU machine a real rank 0 of a world of 2
    # would go on to wait for its missing peer
    monkeypatch.setattr(torch.cuda, "set_device", first_device_call)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "2"])
    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.setenv("RANK", "0")
    monkeypatch.setenv("LOCAL_RANK", "0")
    with pytest.raises(_FirstDeviceCall):                      # the rank reaches its first device call ...
        bench.main()
    assert called == []                                        # ... but never tried to launch ranks of its own


def test_self_launch_hands_the_ranks_an_absolute_dump_dir(monkeypatch, tmp_path):
    """The ranks run in the repository root: a relative --dump-outputs DIR must still name the caller's directory."""
    import bench
    seen = {}

    def fake_run(cmd, **kw):
        seen["cmd"] = cmd
        return types.SimpleNamespace(returncode=0, stdout="")

    monkeypatch.setattr(subprocess, "run", fake_run)
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "2", "--steps", "3", "--dump-outputs", "dumps"])
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    with pytest.raises(SystemExit):
        bench.main()
    argv = seen["cmd"][seen["cmd"].index(os.path.join(ROOT, "bench.py")) + 1:]
    assert argv[-2:] == ["--dump-outputs", str(tmp_path / "dumps")]      # the last occurrence is the one argparse keeps


def test_steps_below_one_are_refused(monkeypatch):
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "0"])
    with pytest.raises(SystemExit) as e:
        bench.main()
    assert e.value.code == 2


def test_output_sample_is_fixed_bounded_and_exact():
    """--dump-outputs: the same positions on every call, float32 / float64 only, at most 64 MB for the 3-minute track."""
    import numpy as np
    import torch
    import bench
    length = bench.TRACK_SECONDS * bench.SR
    out = torch.randn(1, 4, 2, length, generator=torch.Generator().manual_seed(3))
    a, b = bench.output_sample(out), bench.output_sample(out.clone())
    assert sorted(a) == ["stems_sample", "stems_sum", "stems_sumsq", "stems_time_index"]
    for name in a:
        assert a[name].dtype in (np.float32, np.float64) and np.array_equal(a[name], b[name]), name
    assert sum(v.nbytes for v in a.values()) <= 64 << 20
    idx = a["stems_time_index"].astype(np.int64)
    assert idx.shape == (bench.DUMP_TIME_SAMPLES,) and (np.diff(idx) > 0).all() and idx[-1] < length
    assert np.array_equal(a["stems_sample"], out.numpy()[..., idx])
    want = out.double()
    assert np.allclose(a["stems_sum"], want.sum(-1).numpy(), rtol=0, atol=1e-9)
    assert np.allclose(a["stems_sumsq"], (want * want).sum(-1).numpy(), rtol=1e-12)
    short = bench.output_sample(out[..., :1000])                           # a track shorter than the sample: every position
    assert np.array_equal(short["stems_time_index"], np.arange(1000.0))
