"""bench.py's output contract (the driver parses its one JSON line): one short run of the headline
workload on the GPU with the optional legs off, checked for the keys and invariants the task's bench
contract names — metric / value / unit, ms_per_step consistent with value, the roofline block of the
write kernel (achieved <= peak, frac = achieved / peak) and the config's workload."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu


@pytest.mark.timeout(600)
def test_bench_json_line_contract(require_gpu, tmp_path):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "3", "--warmup", "1", "--no-cpu-baseline",
           "--no-north-star", "--no-npd", "--no-drop-in", "--no-general", "--dump-outputs", str(tmp_path / "dump")]
    res = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=540)
    assert res.returncode == 0, res.stderr[-2000:]
    lines = [ln for ln in res.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, res.stdout[-2000:]
    d = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config", "roofline"):
        assert k in d, k
    assert d["n_gpus"] == 1 and d["steps"] == 3 and d["warmup"] == 1 and d["higher_is_better"] is True
    assert d["dtype"] == "f64" and d["config"]["workload"] == "syc 32 5 p=2"
    # value = reference instances per second of whole full knits
    assert abs(d["value"] - d["config"]["instances_ref"] / (d["ms_per_step"] * 1e-3)) <= 1e-6 * d["value"]
    r = d["roofline"]
    assert r["bound"] == "hbm" and r["unit"] == "GB/s" and r["peak"] == 8000.0
    assert 0 < r["achieved"] <= r["peak"] and abs(r["frac"] - r["achieved"] / r["peak"]) <= 1e-9
    # the write kernel runs inside the step
    assert r["avg_launch_ms"] <= d["ms_per_step"]
    # a plain run holds none of the legs that take runs of their own (--full)
    for k in ("npd", "drop_in", "knit_general", "north_star_sweep", "sweep_full", "cpu_baseline"):
        assert k not in d, k
    # --dump-outputs: the last timed step's distribution (head block + seeded sample), float64, <= 64 MB
    import numpy as np

    files = sorted(os.listdir(tmp_path / "dump"))
    assert files == ["knit_out_head.npy", "knit_out_sample.npy"] == sorted(d["dump_outputs"]["entries"])
    arrays = {f: np.load(tmp_path / "dump" / f) for f in files}
    assert all(a.dtype == np.float64 and a.ndim == 1 for a in arrays.values())
    assert sum(a.nbytes for a in arrays.values()) <= 64 << 20
    assert all(a.size == d["dump_outputs"]["entries"][f] for f, a in arrays.items())
    # entries of a probability distribution over 2^32 outcomes (the knit is exact to ~1e-14)
    for a in arrays.values():
        assert np.isfinite(a).all() and a.min() >= -1e-13 and a.sum() <= 1 + 1e-10
    assert arrays["knit_out_sample.npy"].max() > 0

