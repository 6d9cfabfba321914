"""bench.py contract: the driver launches it via torch.distributed.run —
verify the exact multi-process invocation end-to-end on CPU (gloo)."""

import json
import os
import socket
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def test_bench_single_process_cpu(tmp_path):
    out = subprocess.run(
        [sys.executable, os.path.join(REPO, "bench.py"), "--cpu", "--full",
         "--steps", "1", "--warmup", "0", "--batch", "64", "--hidden", "32",
         "--train-steps-per-iter", "3", "--eval-batches", "2"],
        capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert out.returncode == 0, out.stderr[-2000:]
    line = out.stdout.strip().splitlines()[-1]
    d = json.loads(line)
    assert d["metric"] == "adanet_iterations_per_hour"
    assert d["n_gpus"] == 1 and d["steps"] == 1
    assert d["value"] > 0 and d["higher_is_better"] is True
    assert d["scaling"] == "weak"
    assert d["dtype"] == "fp32"  # --cpu debug mode; bf16 on GPU
    assert "final_ensemble_accuracy" in d["config"]
    assert 0.0 <= d["config"]["final_ensemble_accuracy"] <= 1.0


def _plain_cpu_run(tmp_path, dump_dir):
    out = subprocess.run(
        [sys.executable, os.path.join(REPO, "bench.py"), "--cpu",
         "--steps", "2", "--warmup", "1", "--batch", "64", "--hidden", "32",
         "--train-steps-per-iter", "3", "--eval-batches", "2",
         "--dump-outputs", str(dump_dir)],
        capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert out.returncode == 0, out.stderr[-2000:]
    return json.loads(out.stdout.strip().splitlines()[-1])


def test_bench_plain_run_and_dump_outputs(tmp_path):
    """A plain run (no --full) times exactly --steps iterations, skips the
    final-accuracy evaluation, and --dump-outputs writes the last
    iteration's arrays — identical from run to run."""
    import numpy as np

    d = _plain_cpu_run(tmp_path, tmp_path / "a")
    assert d["steps"] == 2 and d["warmup"] == 1
    assert d["config"]["final_ensemble_size"] == 3  # warmup + steps
    assert d["ms_per_step"] > 0
    assert abs(d["value"] - 3600.0 * 1000.0 / d["ms_per_step"]) < 1e-6 * d[
        "value"]
    assert "final_ensemble_accuracy" not in d["config"]

    _plain_cpu_run(tmp_path, tmp_path / "b")
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(os.listdir(tmp_path / "b"))
    assert "selected_indices.npy" in names
    assert any(n.startswith("member.t2_") for n in names)
    assert any(n.startswith("ensemble.") for n in names)
    total = 0
    for n in names:
        a = np.load(tmp_path / "a" / n)
        assert a.dtype in (np.float32, np.float64), n
        assert np.isfinite(a).all(), n
        np.testing.assert_array_equal(a, np.load(tmp_path / "b" / n))
        total += a.nbytes
    assert total <= 64 * 1024 * 1024
    assert len(np.load(tmp_path / "a" / "selected_indices.npy")) == 3


def test_bench_torchrun_two_ranks_cpu(tmp_path):
    """The driver's exact launch shape at N=2 (gloo stands in for RCCL)."""
    port = _free_port()
    out = subprocess.run(
        [sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
         "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
         "--master-port", str(port), os.path.join(REPO, "bench.py"),
         "--gpus", "2", "--cpu", "--steps", "1", "--warmup", "0",
         "--batch", "64", "--hidden", "32", "--train-steps-per-iter", "3",
         "--eval-batches", "2"],
        capture_output=True, text=True, timeout=900, cwd=str(tmp_path))
    assert out.returncode == 0, (out.stdout[-1000:], out.stderr[-2000:])
    # exactly one JSON line, from rank 0
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2
    assert d["config"]["candidates_per_iter"] == 4  # 2 per rank (weak)
    assert "round_robin2" in d["config"]["parallelism"]
    assert d["value"] > 0


def test_bench_torchrun_replication_cpu(tmp_path):
    """DP placement at N=2 over gloo: flat-bucket all-reduce path."""
    port = _free_port()
    out = subprocess.run(
        [sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
         "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
         "--master-port", str(port), os.path.join(REPO, "bench.py"),
         "--gpus", "2", "--cpu", "--steps", "1", "--warmup", "0",
         "--batch", "64", "--hidden", "32", "--train-steps-per-iter", "3",
         "--eval-batches", "2", "--placement", "replication"],
        capture_output=True, text=True, timeout=900, cwd=str(tmp_path))
    assert out.returncode == 0, (out.stdout[-1000:], out.stderr[-2000:])
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["config"]["parallelism"] == "dp2"
    assert d["value"] > 0


def test_bench_self_launches_torchrun(tmp_path):
    """A plain `python bench.py --gpus 2` (no torchrun env) must self-launch
    under torch.distributed.run and report n_gpus=2 — never silently measure
    one rank."""
    out = subprocess.run(
        [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "2",
         "--cpu", "--steps", "1", "--warmup", "0", "--batch", "64",
         "--hidden", "32", "--train-steps-per-iter", "3",
         "--eval-batches", "2"],
        capture_output=True, text=True, timeout=900, cwd=str(tmp_path))
    assert out.returncode == 0, (out.stdout[-1000:], out.stderr[-2000:])
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    assert json.loads(lines[0])["n_gpus"] == 2


def test_bench_world_size_mismatch_fails(tmp_path):
    """Under a torchrun env whose world size contradicts --gpus, bench.py
    must fail instead of reporting a wrong n_gpus."""
    port = _free_port()
    out = subprocess.run(
        [sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
         "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
         "--master-port", str(port), os.path.join(REPO, "bench.py"),
         "--gpus", "4", "--cpu", "--steps", "1", "--warmup", "0",
         "--batch", "64", "--hidden", "32", "--train-steps-per-iter", "3",
         "--eval-batches", "2"],
        capture_output=True, text=True, timeout=900, cwd=str(tmp_path))
    assert out.returncode != 0
