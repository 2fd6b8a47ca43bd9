"""bench.py --gpus N: the launch contract (VERDICT r03 Missing #1).

* CPU: a --gpus that disagrees with an outer launcher's WORLD_SIZE is refused before anything
  touches a GPU (no line with a wrong n_gpus can be printed);
* GPU: ``bench.py --gpus 2`` with no launcher around it starts its two rank processes itself
  (children, torch.distributed.run on 127.0.0.1 -- the reference's Trainer(gpus=N,
  accelerator='ddp'), sl_pipeline.py:157-170) and relays rank 0's line; over gloo both ranks share
  the one GPU of the test box.
"""
import json
import os
import pathlib
import subprocess
import sys

import pytest

ROOT = pathlib.Path(__file__).resolve().parents[1]


def test_bench_refuses_world_size_mismatch():
    env = dict(os.environ, WORLD_SIZE="1", RANK="0", LOCAL_RANK="0")
    p = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "2", "--steps", "1"], env=env,
                       capture_output=True, text=True, timeout=300)
    assert p.returncode != 0
    assert "misreport n_gpus" in (p.stderr + p.stdout)
    assert '"metric"' not in p.stdout


def test_dump_outputs_float32_and_seeded_sample_under_budget(tmp_path):
    """bench.dump_outputs: float32 .npy per name; over the byte budget the large arrays are cut to a
    fixed (seeded) sample, the same elements in every call, small arrays whole."""
    import numpy as np
    import torch
    sys.path.insert(0, str(ROOT))
    import bench
    big = torch.arange(300_000, dtype=torch.float64).reshape(300, 1000)
    arrays = {"loss": torch.tensor(1.5, requires_grad=True), "big": big, "ints": np.arange(7)}
    a = bench.dump_outputs(tmp_path / "a", arrays, budget=400_000)
    b = bench.dump_outputs(tmp_path / "b", arrays, budget=400_000)
    files = sorted(p.name for p in (tmp_path / "a").iterdir())
    assert files == ["big.npy", "ints.npy", "loss.npy"]
    assert sum(p.stat().st_size for p in (tmp_path / "a").iterdir()) <= 400_000 + 3 * 128
    for k in arrays:
        la, lb = np.load(tmp_path / "a" / f"{k}.npy"), np.load(tmp_path / "b" / f"{k}.npy")
        assert la.dtype == (np.float64 if k == "big" else np.float32)
        assert np.array_equal(la, lb) and np.array_equal(la, a[k]) and np.array_equal(lb, b[k])
    s = np.load(tmp_path / "a" / "big.npy")
    assert 40_000 <= s.size < 50_000 and np.all(np.diff(s) > 0)      # a sorted subset of arange
    assert np.array_equal(np.load(tmp_path / "a" / "ints.npy"), np.arange(7, dtype=np.float32))
    whole = bench.dump_outputs(tmp_path / "c", {"big": big.float()})
    assert whole["big"].shape == (300, 1000) and whole["big"].dtype == np.float32


@pytest.mark.gpu
def test_bench_plain_run_is_lean_and_dumps_outputs(tmp_path):
    """A plain ``--gpus 1`` run prints the headline line without the --full measurements and
    --dump-outputs writes finite float32 arrays of the last step (loss, scalars, parameters)."""
    import numpy as np
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--dump-outputs", str(tmp_path / "out")],
                       env=env, capture_output=True, text=True, timeout=300, cwd=str(ROOT))
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout
    rec = json.loads(lines[0])
    assert rec["steps"] == 3 and rec["n_gpus"] == 1 and rec["dtype"] == "f32" and rec["higher_is_better"] is True
    assert rec["value"] > 0 and rec["unit"] == "images/s"
    assert abs(rec["value"] - 128 / (rec["ms_per_step"] * 1e-3)) <= 1e-3 * rec["value"]
    for k in ("roofline", "hot_path", "cpu_baseline", "lyapunov_only_step", "dopri5_train_step", "certify_T40",
              "large_batch_step"):
        assert rec[k] is None, k
    files = list((tmp_path / "out").glob("*.npy"))
    names = {f.stem for f in files}
    assert {"loss", "scalars"} <= names and any(n.startswith("param.") for n in names)
    assert sum(f.stat().st_size for f in files) <= 64 << 20
    for f in files:
        a = np.load(f)
        assert a.dtype == np.float32 and np.isfinite(a).all(), f.name


@pytest.mark.gpu
def test_bench_gpus2_launches_its_ranks():
    env = dict(os.environ, FIODE_BENCH_BACKEND="gloo")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1",
                        "--no-cpu-baseline", "--no-secondary", "--no-configs", "--prof-reps", "2"],
                       env=env, capture_output=True, text=True, timeout=600, cwd=str(ROOT))
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout
    rec = json.loads(lines[0])
    assert rec["n_gpus"] == 2
    assert rec["config"]["parallelism"] == "dp2"
    assert rec["config"]["global_batch"] == 256
    assert rec["process_group"] == {"backend": "gloo", "world_size": 2}
    assert rec["value"] > 0 and rec["device_status"]["status"] == 0
