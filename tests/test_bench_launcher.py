"""bench.py's --gpus contract on the CPU (multi-process, gloo): `--gpus N` without torchrun spawns N
ranks itself, each seeing WORLD_SIZE=N; under torchrun a mismatching --gpus is refused."""
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _env():
    e = dict(os.environ, MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT"):
        e.pop(k, None)
    return e


def test_gpus_n_spawns_n_ranks():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--dry-run"],
                       capture_output=True, text=True, timeout=240, env=_env(), cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [json.loads(m) for m in re.findall(r"\{[^{}]*\}", r.stdout)]
    assert sorted(d["rank"] for d in lines) == [0, 1]
    assert all(d["world"] == 2 for d in lines)
    assert all(d["ranks_share_gpu"] for d in lines)  # no GPU here: both ranks share "one"


def test_gpus_mismatch_is_refused():
    env = _env()
    env.update(WORLD_SIZE="2", RANK="0", LOCAL_RANK="0")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "4", "--dry-run"],
                       capture_output=True, text=True, timeout=120, env=env, cwd=ROOT)
    assert r.returncode != 0 and "WORLD_SIZE=2" in (r.stderr + r.stdout)


def test_gpus_8_through_torchrun_dry_run():
    """the driver's 8-GPU scaling launch shape (torch.distributed.run, 8 ranks, 127.0.0.1) on the CPU:
    every rank joins the process group and reports WORLD_SIZE 8"""
    import socket

    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "8",
                        "--master-addr", "127.0.0.1", "--master-port", str(port),
                        os.path.join(ROOT, "bench.py"), "--gpus", "8", "--dry-run"],
                       capture_output=True, text=True, timeout=300, env=_env(), cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [json.loads(m) for m in re.findall(r"\{[^{}]*\}", r.stdout)]
    assert sorted(d["rank"] for d in lines) == list(range(8))
    assert all(d["world"] == 8 for d in lines)


def test_gpus_8_one_device_per_rank():
    """the 8-GPU node shape: with 8 devices visible every rank gets its own (share False -> RCCL
    process group, the XgmiComm / self-test path, the persistent kernels on), device = LOCAL_RANK"""
    env = _env()
    env["AIOS_BENCH_DEVICES"] = "8"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "8", "--dry-run"],
                       capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [json.loads(m) for m in re.findall(r"\{[^{}]*\}", r.stdout)]
    assert sorted(d["rank"] for d in lines) == list(range(8))
    assert not any(d["ranks_share_gpu"] for d in lines)
    assert sorted(d["device"] for d in lines) == list(range(8))


def test_dump_outputs_float32_npy_within_budget(tmp_path, monkeypatch):
    """--dump-outputs: one float32 .npy per array; an array past its share of the byte budget is
    written as the same seeded sample of its elements every time (two builds compare output for
    output)"""
    import numpy as np

    sys.path.insert(0, ROOT)
    import bench

    toks = np.arange(24, dtype=np.float32).reshape(2, 12)
    logits = np.random.default_rng(1).standard_normal((2, 5000)).astype(np.float32)
    bench.dump_outputs(str(tmp_path / "a"), {"tokens": toks, "logits": logits})
    assert sorted(os.listdir(tmp_path / "a")) == ["logits.npy", "tokens.npy"]
    assert np.array_equal(np.load(tmp_path / "a" / "logits.npy"), logits)
    assert np.load(tmp_path / "a" / "tokens.npy").dtype == np.float32
    monkeypatch.setattr(bench, "DUMP_BUDGET", 16384)
    for d in ("b", "c"):
        bench.dump_outputs(str(tmp_path / d), {"tokens": toks, "logits": logits})
    b, c = np.load(tmp_path / "b" / "logits.npy"), np.load(tmp_path / "c" / "logits.npy")
    assert np.array_equal(b, c) and b.dtype == np.float32 and 1000 < b.size < logits.size
    assert np.isin(b, logits).all()
    assert np.array_equal(np.load(tmp_path / "b" / "tokens.npy"), toks)  # within its share: whole
    assert sum(os.path.getsize(tmp_path / "b" / f) for f in os.listdir(tmp_path / "b")) <= 16384


def test_ranks_per_gpu_from_device_identity():
    """sharing is counted from the physical device identity, not device_count() (each
    rank may see only its own GPU)"""
    from aios_amd.parallel.tp import ranks_per_gpu

    assert ranks_per_gpu(8, [f"node/0000:{i:02x}:00.0" for i in range(8)]) == 1
    assert ranks_per_gpu(4, ["node/0000:05:00.0"] * 4) == 4
    assert ranks_per_gpu(4, ["n/a", "n/a", "n/b", "n/b"]) == 2
