"""The driver depends on bench.py's CLI and JSON-line contract — protect it."""

import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the child runs the CPU path: kernels off, and no device visible to it even
# where the machine has one
CPU_ONLY_ENV = {"MAML355_NO_HIP": "1", "HIP_VISIBLE_DEVICES": "-1",
                "CUDA_VISIBLE_DEVICES": "-1"}

REQUIRED_KEYS = {
    "metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step",
    "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config",
}


def test_bench_json_contract_cpu():
    env = dict(os.environ, **CPU_ONLY_ENV)
    out = subprocess.run(
        [sys.executable, os.path.join(REPO, "bench.py"), "--steps", "1",
         "--warmup", "0", "--tasks_per_gpu", "2", "--inner_steps", "1"],
        capture_output=True, text=True, timeout=600, cwd=REPO, env=env)
    assert out.returncode == 0, out.stderr[-2000:]
    line = [l for l in out.stdout.strip().splitlines() if l.startswith("{")][-1]
    d = json.loads(line)
    assert REQUIRED_KEYS.issubset(d.keys()), REQUIRED_KEYS - set(d.keys())
    assert d["metric"] == "meta-tasks/sec"
    assert d["value"] > 0
    assert d["higher_is_better"] is True
    assert d["scaling"] == "weak"
    assert d["data"] == "synthetic"
    assert d["config"]["global_batch"] == 2
    assert d["config"]["parallelism"] == "task-dp1"


def test_bench_dump_outputs_and_full_cpu(tmp_path):
    """--dump-outputs writes the last timed step's returns as float arrays,
    identical from run to run; --full is accepted and keeps the result line."""
    import numpy as np
    env = dict(os.environ, **CPU_ONLY_ENV)
    dumps = []
    for name, extra in (("a", []), ("b", ["--full"])):
        out_dir = tmp_path / name
        out = subprocess.run(
            [sys.executable, os.path.join(REPO, "bench.py"), "--steps", "2",
             "--warmup", "0", "--tasks_per_gpu", "2", "--inner_steps", "1",
             "--dump-outputs", str(out_dir)] + extra,
            capture_output=True, text=True, timeout=600, cwd=REPO, env=env)
        assert out.returncode == 0, out.stderr[-2000:]
        d = json.loads([l for l in out.stdout.strip().splitlines()
                        if l.startswith("{")][-1])
        assert REQUIRED_KEYS.issubset(d.keys())
        assert d["steps"] == 2 and d["ms_per_step"] > 0
        assert d["dtype"] == "fp32"
        files = sorted(p.name for p in out_dir.iterdir())
        assert files == ["accuracy.npy", "loss.npy", "per_task_logits.npy"]
        dumps.append({f: np.load(out_dir / f) for f in files})
    a, b = dumps
    assert a["per_task_logits.npy"].shape == (2, 5 * 15, 5)
    for f, arr in a.items():
        assert arr.dtype == np.float32
        assert np.isfinite(arr).all()
        np.testing.assert_array_equal(arr, b[f])
