"""bench.py end to end on the GPU: a plain run prints the headline line and nothing of --full, and --dump-outputs writes
what the last timed step computed -- checked bit-exact against the CPU oracle on the same synthetic cloud."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from vtkcloudpoint_amd import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_bench(out_dir, *args):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--dump-outputs", str(out_dir)] + list(args), capture_output=True, text=True, timeout=300,
                       cwd=ROOT)
    assert p.returncode == 0, p.stderr[-2000:]
    line = json.loads(p.stdout.strip().splitlines()[-1])
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in line, k
    assert line["steps"] == 3 and line["warmup"] == 1 and line["ms_per_step"] > 0
    for k in ("beside_headline", "icp_1M_vs_100", "after_clustering", "monolithic_dbscan", "block_pipeline",
              "single_gpu_same_workload_ms"):
        assert k not in line, k  # --full only
    assert line["cpu_baseline"] is None
    return line, {f[:-4]: np.load(os.path.join(out_dir, f)) for f in os.listdir(out_dir)}


def test_single_dump_matches_oracle(tmp_path, oracle):
    n = 2_500_000  # above the dump's sample size: the per-point arrays are a seeded sample
    line, d = run_bench(tmp_path, "--points", str(n))
    c = synth.config_cloud(n, seed=4)
    o = oracle.dbscan(c["motor"], c["eps_l1"], c["min_pts"], oracle.L1_2D)
    idx = d["sample_index"].astype(np.int64)
    assert len(idx) == 2_000_000 and np.all(np.diff(idx) > 0) and idx[-1] < n
    assert d["labels"].dtype == np.float64 and d["is_key_point"].dtype == np.float32
    assert np.array_equal(d["labels"], o["labels"][idx]) and np.array_equal(d["is_key_point"], o["is_key"][idx])
    assert np.array_equal(d["is_classed"], o["classed"][idx])
    assert d["clusters"][0] == o["cf"] == line["config"]["clusters"] and d["dist_evals"][0] == o["evals"]
    assert sum(os.path.getsize(os.path.join(tmp_path, f)) for f in os.listdir(tmp_path)) <= 64 << 20


def test_blocks_dump_matches_oracle(tmp_path, oracle):
    n = 300_000
    line, d = run_bench(tmp_path, "--points", str(n), "--mode", "blocks")
    o = oracle.block_pipeline(synth.config_cloud(n, seed=4)["motor"], 0.07, 7, 200, 3)
    assert np.array_equal(d["sample_index"], np.arange(n, dtype=np.float64))
    assert np.array_equal(d["labels"], o["labels"])
    for k in ("cluster_amount", "kept", "del_sum", "evals"):
        assert d[k][0] == o[k], k
    assert line["config"]["clusters"] == o["cluster_amount"]
