"""The driver's bench.py contract (one JSON line with the documented fields) on the CPU plumbing path,
single rank and a 2-rank gloo run under torch.distributed.run; ``--dump-outputs`` and ``--full`` on the CPU
path and, marked ``gpu``, on the headline LeNet-5 workload."""
import json
import os
import socket
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = {"metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
        "vs_baseline", "dtype", "data", "config"}


def _json_lines(out: str):
    return [json.loads(l) for l in out.splitlines() if l.startswith("{")]


def _port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


@pytest.mark.timeout(300)
def test_bench_single_rank_json_line():
    env = dict(os.environ, PYTHONPATH=ROOT)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, "bench.py", "--model", "mlp_mnist", "--batch-per-gpu", "64", "--steps", "3",
                        "--warmup", "1"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=280)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = _json_lines(p.stdout)
    assert len(lines) == 1
    d = lines[0]
    assert KEYS <= set(d)
    assert d["n_gpus"] == 1 and d["steps"] == 3 and d["warmup"] == 1 and d["higher_is_better"] is True
    assert d["value"] > 0 and d["scaling"] == "weak"
    assert {"model", "global_batch", "per_gpu_batch", "parallelism"} <= set(d["config"])


def _bench(*args):
    env = dict(os.environ, PYTHONPATH=ROOT)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, "bench.py", *args], cwd=ROOT, env=env, capture_output=True, text=True,
                       timeout=280)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = _json_lines(p.stdout)
    assert len(lines) == 1
    return lines[0]


@pytest.mark.timeout(300)
def test_bench_dump_outputs_is_reproducible(tmp_path):
    """``--dump-outputs DIR``: the last timed step's outputs as float32 .npy files, identical between two runs
    with the same arguments, and different after a different number of timed steps (``--steps`` is real)."""
    import numpy as np

    args = ("--model", "mlp_mnist", "--batch-per-gpu", "64", "--warmup", "1")
    runs = {}
    for tag, steps in (("a", "3"), ("b", "3"), ("c", "4")):
        d = _bench(*args, "--steps", steps, "--dump-outputs", str(tmp_path / tag))
        assert d["steps"] == int(steps) and d["ms_per_step"] > 0
        files = sorted(os.listdir(tmp_path / tag))
        assert files == ["stats.npy", "weights.npy"] and sorted(d["dumped"]) == ["stats", "weights"]
        runs[tag] = {f: np.load(tmp_path / tag / f) for f in files}
        assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in runs[tag].values())
        assert sum(os.path.getsize(tmp_path / tag / f) for f in files) <= 64 << 20
    # the flat master holds the model's 7,960 parameters (plus its alignment padding)
    assert 7960 <= runs["a"]["weights.npy"].size < 7960 + 64 and runs["a"]["stats.npy"].shape == (2,)
    for f in ("stats.npy", "weights.npy"):
        np.testing.assert_array_equal(runs["a"][f], runs["b"][f])
    assert not np.array_equal(runs["a"]["weights.npy"], runs["c"]["weights.npy"])


def test_dump_outputs_samples_large_arrays(tmp_path, monkeypatch):
    """An array over its share of the byte budget is written as a fixed, seeded sample of its elements."""
    import numpy as np
    import torch

    sys.path.insert(0, ROOT)
    try:
        import bench
    finally:
        sys.path.remove(ROOT)
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 2 * 4096 + 4 * 2000)  # 2000 elements in all
    big, small = torch.arange(5000, dtype=torch.float64), torch.arange(6).reshape(2, 3)
    for tag in ("a", "b"):
        rec = bench.dump_outputs(str(tmp_path / tag), {"big": big, "small": small})
        assert rec == {"big": [1994], "small": [2, 3]}  # the small one whole, the rest of the budget sampled
    a, b = np.load(tmp_path / "a" / "big.npy"), np.load(tmp_path / "b" / "big.npy")
    assert a.dtype == np.float32 and np.array_equal(a, b)
    assert (np.diff(a) > 0).all() and a.min() >= 0 and a.max() < 5000  # distinct elements, in order
    np.testing.assert_array_equal(np.load(tmp_path / "a" / "small.npy"), small.float().numpy())
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")) <= bench.DUMP_MAX_BYTES


@pytest.mark.timeout(300)
def test_bench_full_option_keeps_the_result_line():
    """``--full`` is accepted everywhere; on the CPU plumbing path it adds nothing to the line."""
    d = _bench("--model", "mlp_mnist", "--batch-per-gpu", "64", "--steps", "2", "--warmup", "1", "--full")
    assert KEYS <= set(d) and d["steps"] == 2 and d["check"]["ok"] is True


_HEADLINE = ("--gpus", "1", "--batch-per-gpu", "256", "--steps", "4", "--warmup", "1")


@pytest.mark.gpu
@pytest.mark.timeout(120)
def test_bench_gpu_plain_run_is_lean_and_dumps_reproducibly(tmp_path):
    """The headline workload (LeNet-5 on the GPU): a plain run times its steps and nothing else, and two runs
    with ``--dump-outputs`` train on the same inputs, so their last steps agree bit for bit."""
    import numpy as np

    out = []
    for tag in ("a", "b"):
        d = _bench(*_HEADLINE, "--dump-outputs", str(tmp_path / tag))
        assert d["dtype"] == "bf16" and d["steps"] == 4 and d["ms_per_step"] > 0 and d["check"]["ok"] is True
        assert "gradient" not in d["check"] and "async" not in d and len(d["settle"]["runs"]) == 1
        out.append({f: np.load(tmp_path / tag / (f + ".npy")) for f in ("stats", "weights")})
        assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in out[-1].values())
    assert d["settle"]["runs"][0]["steps"] == 1024  # a fixed count of settle steps (4 per replay), not a time
    assert out[0]["weights"].size >= 61706 and 0 < out[0]["stats"][0] / 256 < 50.0
    for f in ("stats", "weights"):
        np.testing.assert_array_equal(out[0][f], out[1][f])


@pytest.mark.gpu
@pytest.mark.timeout(120)
def test_bench_gpu_full_run_adds_guard_and_async():
    """``--full`` keeps the correctness guard and the async comparison next to the same headline fields."""
    d = _bench(*_HEADLINE, "--full")
    assert KEYS <= set(d) and d["steps"] == 4 and d["ms_per_step"] > 0
    assert d["check"]["gradient"]["ok"] is True and d["check"]["ok"] is True
    assert d["async"]["steps"] == 4 and d["async"]["speedup_vs_sync"] > 0


@pytest.mark.timeout(300)
def test_bench_two_rank_gloo_json_line():
    env = dict(os.environ, PYTHONPATH=ROOT)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                        "--master-addr", "127.0.0.1", "--master-port", str(_port()), "bench.py", "--gpus", "2",
                        "--model", "mlp_mnist", "--batch-per-gpu", "64", "--steps", "3", "--warmup", "1"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=280)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = _json_lines(p.stdout)
    assert len(lines) == 1  # rank 0 only
    d = lines[0]
    assert d["n_gpus"] == 2 and d["config"]["global_batch"] == 128 and d["config"]["parallelism"] == "dp2"


@pytest.mark.timeout(300)
def test_bench_self_spawns_ranks_without_torchrun():
    """``bench.py --gpus N`` with WORLD_SIZE unset launches N ranks itself."""
    env = dict(os.environ, PYTHONPATH=ROOT)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, "bench.py", "--gpus", "2", "--model", "mlp_mnist", "--batch-per-gpu", "64",
                        "--steps", "3", "--warmup", "1"], cwd=ROOT, env=env, capture_output=True, text=True,
                       timeout=280)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = _json_lines(p.stdout)
    assert len(lines) == 1
    d = lines[0]
    assert d["n_gpus"] == 2 and d["world"] == 2 and d["backend"] == "gloo"
    assert d["config"]["global_batch"] == 128


@pytest.mark.timeout(120)
def test_bench_refuses_world_mismatch():
    """A process group whose size differs from --gpus is an error, never a mislabelled number."""
    env = dict(os.environ, PYTHONPATH=ROOT, RANK="0", WORLD_SIZE="1", LOCAL_RANK="0")
    p = subprocess.run([sys.executable, "bench.py", "--gpus", "2", "--model", "mlp_mnist", "--batch-per-gpu", "64",
                        "--steps", "1", "--warmup", "0"], cwd=ROOT, env=env, capture_output=True, text=True,
                       timeout=110)
    assert p.returncode != 0
    assert not _json_lines(p.stdout)
