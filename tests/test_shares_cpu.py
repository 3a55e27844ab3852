"""The sharded block pipeline's driver (vtkcloudpoint_amd.distributed.sharded_pipeline_local) on shares that hold no block:
lattices whose last bucket -- the points in no block, on x == x_Min or y == y_Min -- holds more than n / world points, so
that the ranks behind it get the share [NS, NS).  The per-rank compute is the CPU stand-in (oracle.binding.StagedPipeline),
which reports such a share as the block range (nblocks, nblocks) with no point; the HIP library keeps the same contract
(tests/test_shares_gpu.py).  Every rank's result must equal the oracle's single-process pipeline."""
import numpy as np
import pytest

from vtkcloudpoint_amd import distributed as D

EPS, MIN_PTS = 0.25, 3
# (columns, rows, ptsInCell): lattices of step 0.25
LATTICES = [(3, 300, 12), (4, 200, 20), (2, 500, 10), (2, 40000, 4)]


def lattice(cols, rows, step=0.25):
    x, y = np.meshgrid(np.arange(cols), np.arange(rows))
    return np.ascontiguousarray(np.stack([x.ravel(), y.ravel()], 1).astype(np.float64) * step)


@pytest.mark.parametrize("cols,rows,pic", LATTICES)
def test_empty_trailing_shares_on_the_stand_in(oracle, cols, rows, pic):
    motor = lattice(cols, rows)
    o = oracle.block_pipeline(motor, EPS, MIN_PTS, pic, 3)
    nblocks = o["rows"] * o["cols"]
    n_empty = 0
    for world in (4, 8, 16):
        probe = oracle.StagedPipeline()
        probe.blocks_plan(motor.ctypes.data, len(motor), EPS, MIN_PTS, pic, 3)
        cuts = probe.blocks_plan_cuts(world)
        n_empty += cuts[world - 1] == nblocks + 1
        for noise in ("gather", "slabs"):
            res = D.sharded_pipeline_local([oracle.StagedPipeline() for _ in range(world)], motor.ctypes.data, len(motor),
                                           EPS, MIN_PTS, pic, 3, device="cpu", noise=noise)
            what = "%dx%d world %d %s" % (cols, rows, world, noise)
            for q, r in enumerate(res):
                assert np.array_equal(r["labels"].numpy(), o["labels"]), "%s rank %d: labels" % (what, q)
                for k in ("rows", "cols", "kept", "del_sum", "cluster_amount", "evals"):
                    assert r[k] == o[k], "%s rank %d: %s %r != %r" % (what, q, k, r[k], o[k])
                assert r["m"] == len(o["order"]), what
            ranges = [r["block_range"] for r in res]
            assert ranges[0][0] == 0 and ranges[-1][1] == nblocks, what
            assert all(lo <= hi for lo, hi in ranges) and all(a[1] == b[0] for a, b in zip(ranges, ranges[1:])), what
            if cuts[world - 1] == nblocks + 1:
                assert ranges[-1] == (nblocks, nblocks) and res[-1]["m_local"] == 0, what
    assert n_empty >= 2  # the last rank's share really was empty (at 8 and 16 ranks at least)
