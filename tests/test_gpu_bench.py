"""bench.py on the device: a plain run prints the headline line, --dump-outputs writes the last
timed step's embedding and eigenvalues, and the same arguments give the same outputs bit for bit
(each run a fresh process, as the benchmark is used)."""

import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent


def _bench(out_dir: Path) -> dict:
    cmd = [sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
           "--workload", "custom", "--taxa", "2000", "--trees", "50", "--dump-outputs", str(out_dir)]
    proc = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert proc.returncode == 0, proc.stderr[-2000:]
    return json.loads(proc.stdout.strip().splitlines()[-1])


@pytest.mark.gpu
def test_plain_bench_dumps_repeatable_outputs(tmp_path):
    lines = [_bench(tmp_path / f"run{i}") for i in range(2)]
    for line in lines:
        assert line["steps"] == 2 and line["ms_per_step"] > 0 and line["unit"] == "s"
        assert line["higher_is_better"] is False and line["dtype"].startswith("f64")
        assert abs(line["value"] * 1e3 - line["ms_per_step"]) < 1e-2
        for key in ("parity", "cpu_baseline", "seeds", "other_workloads", "recursion", "value_tables_resident"):
            assert key not in line, key
    for name, shape in (("embedding", (2000, 2)), ("eigenvalues", (3,))):
        a, b = (np.load(tmp_path / f"run{i}" / f"{name}.npy") for i in range(2))
        assert a.dtype == np.float64 and a.shape == shape and np.all(np.isfinite(a))
        assert np.array_equal(a, b), name
