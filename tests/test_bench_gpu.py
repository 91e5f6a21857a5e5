"""bench.py's contract with whoever runs it: a plain run prints one result line whose headline fields describe the K timed steps,
leaves the measurements beside the headline to `--full`, and `--dump-outputs DIR` writes what the last timed step returned."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_plain_bench_run_reports_its_steps_and_dumps_the_last_one(tmp_path):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    out = tmp_path / "outputs"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--dump-outputs", str(out)], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, lines
    line = json.loads(lines[0])
    assert line["metric"].startswith("PCG subproblems/sec") and line["unit"] == "PCG subproblems/s"
    assert line["higher_is_better"] is True and line["dtype"] == "f64"
    assert line["steps"] == 3 and line["warmup"] == 1
    assert line["ms_per_step"] > 0 and line["value"] * line["ms_per_step"] == pytest.approx(1e3, rel=1e-12)
    # what only --full measures is absent from a plain run
    assert line["cpu_baseline"] is None and line["roofline"]["dense_sample"] is None
    assert not {"matvec", "read_probe", "post_stream_us", "ic_variant"} & set(line)
    dumped = {name: np.load(out / (name + ".npy")) for name in ("w", "status", "iters", "n_hmul")}
    assert all(a.dtype == np.float64 for a in dumped.values())
    w = dumped["w"]
    assert w.shape == (line["config"]["n"],) and np.isfinite(w).all() and np.linalg.norm(w) > 0
    cfg = line["config"]
    from benlsip_jl_amd import CGStatus
    assert dumped["status"].tolist() == [float(CGStatus[cfg["cg_status"]])]
    assert dumped["iters"].tolist() == [float(cfg["cg_iters_per_subproblem"] + 1)]
    assert dumped["n_hmul"].tolist() == [float(cfg["hmul_per_subproblem"])]
