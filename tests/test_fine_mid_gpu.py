"""The grid build's fine pass for handed-on buckets of at most 8192 records (csrc/gridbuild.hip: k_part_fine_mid, two
workgroups per CU) and the output scatter with its loads in front (k_out_scatter): every case once with the new path and
once with VCP_FINE_MID=0 (every handed-on bucket through k_part_fine), results bit-exact against the CPU oracle --
labels, is_core, is_classed, cf and evals; for the grouped case the block pipeline's labels, block assignment, merge
order and counters.  The switch is read once per process, so every run is a fresh child (tests/_fine_mid_worker.py).

Which kernel took which bucket is read from the child's trace, never from the case's intent: the launch lines, the
decision line `gridfine mid_on= lds_m=` and the read-back `gridfine small= mid= big=`.  Where the worker lays
a cloud out bucket by bucket it prints the counts its layout should give, and the trace has to agree.

Shown once that these tests bite, on a scratch build with a value-only mutation: the parked indices of a thread's records
4 .. 7 read back pairwise swapped (`park[(k - 4) ^ 1]`; every parked word is the index of a record of the bucket, so
nothing stale goes out as a position).  With the path on, every_record_count_and_counter_fork, nonfinite_points,
is_classed_input, coarse_grid_csh_10, coarse_grid_csh_12, grouped_call, slab_call_with_d_ord and output_scatter_edges fail
(each holds a bucket of more than 4096 records); the 3-D case and all nine runs with VCP_FINE_MID=0 pass.  (The staged
part's bound off by one is not value-only: the record at the part's border then lands in the index array, or a stale
word is flushed as an index.)"""
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "_fine_mid_worker.py")
MID = "vcp-trace launch (k_part_fine_mid<GD, GROUPED>)"
OLD = "vcp-trace launch (k_part_fine<GD, GROUPED>)"
COUNTS = re.compile(r"gridfine small=(\d+) mid=(\d+) big=(\d+)")


def run(case, mid, two_d=True):
    """-> the (small, mid, big) bucket counts of every grid build of the run, from the trace"""
    env = {k: v for k, v in os.environ.items() if k not in ("VCP_FINE_MID", "VCP_PART_PAIRS", "VCP_CPB_LOG2",
                                                             "VCP_PART_CHUNKS", "VCP_CELL_BUDGET", "VCP_BRUTE_MAX")}
    env["VCP_TRACE"] = "1"
    if not mid:
        env["VCP_FINE_MID"] = "0"
    p = subprocess.run([sys.executable, WORKER, case], env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, "%s, mid %s:\n%s\n%s" % (case, mid, p.stdout[-2000:], p.stderr[-4000:])
    assert p.stdout.strip().splitlines()[-1].startswith("ok " + case)
    lines = p.stderr.splitlines()
    counts = [tuple(int(v) for v in m.groups()) for m in map(COUNTS.search, lines) if m]
    assert counts, "no grid build in the trace"
    assert OLD in lines
    on = mid and two_d
    assert (MID in lines) == on, "%s, mid %s: launch of k_part_fine_mid" % (case, mid)
    decided = [l for l in lines if "gridfine mid_on=" in l]
    assert decided and all(("mid_on=%d " % on) in l for l in decided), decided[:3]
    if not on:
        assert all(c[1] == 0 for c in counts), counts
    m = re.search(r"expect small=(\d+) mid=(\d+) big=(\d+)", p.stdout)
    if m:  # a laid-out cloud: one grid build, and it went as laid out
        assert counts == [tuple(int(v) for v in m.groups())], "%s, mid %s: %s, laid out for %s" % (case, mid, counts, m.group(0))
    return counts


BOTH = pytest.mark.parametrize("mid", [True, False], ids=["mid", "old"])


@BOTH
def test_every_record_count_and_counter_fork(mid):
    """16 buckets of 2^14 cells: 2048 | 2049 records, 129 populous words, 2048 in one part, 4096 | 4097, 8192 | 8193, 4096
    in one even / odd cell, 2 x 2048 in one counter word, an empty bucket, a cell across positions 2047 | 2048, a cell of
    five beside empty ones, one record, the grid's last bucket."""
    small, m, big = run("thresholds", mid)[0]
    assert (m >= 10 and big == 1) if mid else (m == 0 and big >= 11)


@BOTH
def test_nonfinite_points_leave_fewer_records(mid):
    run("nonfinite", mid)


@BOTH
def test_is_classed_input(mid):
    run("classed", mid)


@BOTH
def test_coarse_grid_csh_10(mid):
    small, m, big = run("coarse10", mid)[0]
    assert (m, big) == ((3, 1) if mid else (0, 4))


@BOTH
def test_coarse_grid_csh_12(mid):
    small, m, big = run("coarse12", mid)[0]
    assert (m, big) == ((4, 1) if mid else (0, 5))


@BOTH
def test_3d_build_keeps_the_old_path(mid):
    counts = run("3d", mid, two_d=False)
    assert sum(c[2] for c in counts) >= 1


@BOTH
def test_grouped_call(mid):
    counts = run("grouped", mid)
    assert sum(c[1] + c[2] for c in counts) >= 1, counts  # some bucket was handed on


@BOTH
def test_slab_call_with_d_ord(mid):
    counts = run("slab", mid)
    assert sum(c[1] + c[2] for c in counts) >= 1, counts


@BOTH
def test_output_scatter_edges(mid):
    run("scatter", mid)
