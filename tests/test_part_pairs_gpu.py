"""The grid build's scatter pass with the pairing stash (csrc/gridbuild.hip: k_part_scatter_pairs) and without it
(k_part_scatter: VCP_PART_PAIRS=0, or more super-buckets than the stash has room for): every case once each way, results
bit-exact against the CPU oracle -- labels, is_core, is_classed, cf and evals; for the grouped case the block pipeline's
labels, block assignment, merge order and counters.  The switches are read once per process, so every run is a fresh
child process (tests/_part_pairs_worker.py).  The child runs with VCP_TRACE, and its launch trace has to show the scatter
kernel the run is about: a switch that did nothing would otherwise pass as two runs of the same kernel."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "_part_pairs_worker.py")
PAIRS, NO_PAIRS = "vcp-trace launch (k_part_scatter_pairs<GD, GROUPED>)", "vcp-trace launch (k_part_scatter<GD, GROUPED>)"


def run(case, pairs, stash=None, **extra):
    """stash: whether the pairing stash is expected to run (default: whenever the switch allows it)"""
    env = {k: v for k, v in os.environ.items() if k not in ("VCP_PART_PAIRS", "VCP_CPB_LOG2", "VCP_PART_CHUNKS",
                                                             "VCP_CELL_BUDGET", "VCP_BRUTE_MAX")}
    env["VCP_TRACE"] = "1"
    if not pairs:
        env["VCP_PART_PAIRS"] = "0"
    env.update(extra)
    p = subprocess.run([sys.executable, WORKER, case], env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, "%s, pairs %s:\n%s\n%s" % (case, pairs, p.stdout[-2000:], p.stderr[-4000:])
    assert p.stdout.strip().startswith("ok " + case)
    launched = set(p.stderr.splitlines())
    want, other = (PAIRS, NO_PAIRS) if (pairs if stash is None else stash) else (NO_PAIRS, PAIRS)
    assert want in launched and other not in launched, "%s, pairs %s: the trace does not show %s alone" % (case, pairs, want)


@pytest.mark.parametrize("pairs", [True, False], ids=["pairs", "no_pairs"])
def test_n_1_2_3_1023(pairs):
    """No pair, one pair, a pair and a leftover, one partial trip; both metrics."""
    run("tiny", pairs)


@pytest.mark.parametrize("pairs", [True, False], ids=["pairs", "no_pairs"])
def test_three_chunks_clumps_background_nonfinite_2d(pairs):
    """n = 2 * 8192 + 37: pairs inside a trip and across trips, runs of length one and of odd length, NaN and inf."""
    run("mixed2d", pairs)


@pytest.mark.parametrize("pairs", [True, False], ids=["pairs", "no_pairs"])
def test_three_chunks_clumps_background_nonfinite_3d(pairs):
    """The same shape through the 3-D build (L2_3D)."""
    run("mixed3d", pairs)


@pytest.mark.parametrize("pairs", [True, False], ids=["pairs", "no_pairs"])
def test_grouped_call_with_points_left_out(pairs):
    """Staged block pipeline on 20 k points in three shares against oracle.block_pipeline: lanes that take no slot
    inside the barriered loop."""
    run("grouped", pairs)


@pytest.mark.parametrize("pairs", [True, False], ids=["pairs", "no_pairs"])
def test_more_buckets_than_the_stash_holds(pairs):
    """250 k uniform points on 2740 x 2740 cells with VCP_CPB_LOG2=10: NS = 7332 super-buckets, between the stash
    capacity (6826 = 160 KB / 24 B) and MAXB = 8192, so k_part_scatter runs whatever VCP_PART_PAIRS says."""
    run("fallback", pairs, stash=False, VCP_CPB_LOG2="10")
