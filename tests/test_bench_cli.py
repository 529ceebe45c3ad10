"""bench.py as the round driver runs it at N > 1: ``python bench.py --gpus 2`` without a
launcher spawns the ranks itself (never measures W=1 under an N-GPU label) and rank 0
prints ONE JSON line with the whole-job value, the rank count the process group really has,
and the per-region breakdown (max/min over ranks, exposed exchange, bytes per peer). CPU /
gloo here; the same code path runs RCCL on an 8-GPU node."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_cli_w2_spawns_ranks_and_reports_regions(tmp_path):
    env = {k: v for k, v in os.environ.items()
           if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--scale", "2e-5",
           "--steps", "2", "--warmup", "1", "--window", "64", "--extra-steps", "1", "--full"]
    p = subprocess.run(cmd, cwd=tmp_path, env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["config"]["rccl_world_size"] == 2
    assert d["metric"] == "edges_per_s" and d["value"] > 0 and d["steps"] == 2
    assert d["executor"].startswith("fused") and d["dtype"] == "fp32"
    r = d["regions"]
    for k in ("ms_max_over_ranks", "ms_min_over_ranks", "compute_ms_max", "compute_ms_min",
              "exposed_exchange_ms_max", "max_bytes_per_peer_per_step", "bytes_sent_per_rank"):
        assert k in r, k
    assert len(r["bytes_sent_per_rank"]) == 2 and min(r["bytes_sent_per_rank"]) > 0
    assert any(k.startswith("exchange") for k in r["ms_max_over_ranks"])
    assert "structureless" in d  # measured or explicitly skipped, never a crash
    # the one-sided probe ran as a separate child job over the headline's plan (gloo here:
    # the torch exchange only, the heap needs device memory)
    sp = d["shmem_probe"]
    assert "failed" not in sp, sp
    assert sp["world"] == 2 and sp["torch_pg"]["exchange_ms_max"] > 0
    assert sp["rows_sent_max"] > 0 and sp["shmem"].startswith("unavailable")
    # the resolved configuration, whole
    assert d["run_config"]["fused"]["halo_stream"] in ("auto", "on", "off")
    assert d["run_config"]["model"]["dtype"] == "fp32"


def test_bench_cli_shmem_probe_failure_keeps_headline(tmp_path):
    """A probe child that dies (rank 1 aborts, as after a GPU fault) costs the probe only:
    the headline JSON line is printed with ``shmem_probe.failed`` naming the rank."""
    env = {k: v for k, v in os.environ.items()
           if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env["DGRAPH_SHMEM_PROBE_FAULT"] = "abort1"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--scale", "2e-5",
           "--steps", "1", "--warmup", "1", "--window", "64", "--full", "--no-extra",
           "--shmem-probe-timeout", "90"]
    p = subprocess.run(cmd, cwd=tmp_path, env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["value"] > 0 and d["n_gpus"] == 2
    failed = d["shmem_probe"]["failed"]
    assert any(f["rank"] == 1 and f["exit"] not in (0, None) for f in failed), failed


def test_bench_cli_plain_run_is_lean_and_dumps_outputs(tmp_path):
    """Without ``--full`` the line carries the headline only (no region breakdown, no
    secondary jobs); ``--dump-outputs`` writes the last timed step's loss, hit counts,
    updated weights and gradients as float .npy files."""
    import numpy as np

    env = {k: v for k, v in os.environ.items()
           if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    out = tmp_path / "dump"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--scale", "2e-5",
           "--steps", "1", "--warmup", "0", "--window", "64", "--dump-outputs", str(out)]
    p = subprocess.run(cmd, cwd=tmp_path, env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["metric"] == "edges_per_s" and d["unit"] == "edges/s" and d["higher_is_better"]
    assert d["steps"] == 1 and d["ms_per_step"] > 0 and d["dtype"] == "fp32"
    c = d["config"]
    assert d["value"] == pytest.approx(c["num_layers"] * c["E_msg"] / (d["ms_per_step"] / 1e3))
    for k in ("regions", "structureless", "bf16_stack", "train_rows_only", "xgmi_probe",
              "shmem_probe"):
        assert k not in d, k
    files = {f.name: np.load(f) for f in out.iterdir()}
    assert all(a.dtype in (np.float32, np.float64) for a in files.values())
    assert float(files["loss.npy"][0]) == d["final_loss"]
    assert files["correct_val_test.npy"].shape == (2,)
    params = [n for n in files if n.startswith("param_")]
    assert len(params) == 9 and sum(n.startswith("grad_") for n in files) == 9
    assert files["param_00_layers_0_w_self.npy"].shape == (128, 256)
    assert sum(a.nbytes for a in files.values()) <= 64 << 20


def test_bench_cli_refuses_mismatched_world(tmp_path):
    env = dict(os.environ, WORLD_SIZE="1")
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "4", "--scale", "2e-5",
           "--steps", "1", "--warmup", "0"]
    p = subprocess.run(cmd, cwd=tmp_path, env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode != 0 and not any(l.startswith("{") for l in p.stdout.splitlines())
