"""GPU: a plain `bench.py` run (no --full) and its --dump-outputs.

A plain run times its steps and prints the line; the baselines, the parity sample and the
per-stage runs belong to --full (tests/test_gpu_multiprocess.py runs that form). Here one small
plain run writes the last timed step's outputs, and they are checked against the host float64
oracle over the same seeded catalog and queries, regenerated in this process: the dump is what
the timed path returned, and the inputs depend on the arguments only.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import restatement as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")
FULL_ONLY = ("roofline_topk", "stage_ms_per_step", "stage_breakdown", "host_boundary",
             "cpu_baseline", "parity", "device_parity")


def test_plain_run_times_and_dumps(cuda_device, tmp_path):
    import bench
    n, b, steps = 40_000, 300, 3
    out_dir = tmp_path / "out"
    env = {k: v for k, v in os.environ.items()
           if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    p = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--config", "C2", "--n", str(n),
                        "--b", str(b), "--steps", str(steps), "--warmup", "1",
                        "--dump-outputs", str(out_dir)],
                       capture_output=True, text=True, timeout=120, env=env)
    assert p.returncode == 0, p.stderr[-4000:]
    (j,) = [json.loads(l) for l in p.stdout.splitlines() if l.startswith("{")]
    assert j["metric"] == bench.METRIC and j["unit"] == "queries/s" and j["higher_is_better"]
    assert j["dtype"] == "f64" and j["n_gpus"] == 1
    assert j["steps"] == steps and j["warmup"] == 1 and j["full"] is False
    assert j["ms_per_step"] > 0
    # value and ms_per_step are the same measurement (both rounded to 3 decimals)
    assert j["value"] == pytest.approx(b / (j["ms_per_step"] * 1e-3), rel=1e-2)
    # the roofline comes from the timed steps' own events: every step launched the kernel
    assert j["roofline"]["per_launch"]["launches"] >= steps
    assert not [key for key in FULL_ONLY if key in j], sorted(j)
    assert f"step {steps}/{steps} submitted" in p.stderr

    assert sorted(os.listdir(out_dir)) == ["rows.npy", "scores.npy"]
    s, r = np.load(out_dir / "scores.npy"), np.load(out_dir / "rows.npy")
    assert s.dtype == np.float64 and r.dtype == np.float64
    k = bench.CONFIGS["C2"]["k"]
    assert s.shape == (b, k) and r.shape == (b, k)
    cfg = dict(bench.CONFIGS["C2"], n=n, b=b)
    cat = bench.make_catalog_shard(cfg, 0, n, cuda_device).double().cpu().numpy()
    q = bench.make_queries(cfg, cuda_device).double().cpu().numpy()
    s_ref, r_ref = R.cosine_topk(q, cat, k)
    assert np.array_equal(r.astype(np.int64), r_ref)
    assert np.max(np.abs(s - s_ref)) <= 1e-12
