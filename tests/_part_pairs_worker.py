"""Worker of tests/test_part_pairs_gpu.py: one case of the grid build's scatter pass (csrc/gridbuild.hip) against the
CPU oracle, in a process of its own because the switches that pick the kernel (VCP_PART_PAIRS, VCP_CPB_LOG2) are read
once per process.  usage: _part_pairs_worker.py CASE; exit status 0 = every comparison held."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

PCH_MIN, PT, MAXB = 8192, 1024, 8192  # csrc/gridbuild.hip
STASH_MAX = 160 * 1024 // 24         # super-buckets whose cursors + stash fit one CU's LDS
Q = 1024.0                            # coordinates on the 2^-10 lattice: exact ties at the threshold, nothing to re-test


def same(g, o, what):
    assert np.array_equal(g["labels"], o["labels"]), what + ": labels"
    assert np.array_equal(g["is_core"], o["is_key"]), what + ": is_core"
    assert np.array_equal(g["is_classed"], o["classed"]), what + ": is_classed"
    assert g["cf"] == o["cf"], what + ": cf %d != %d" % (g["cf"], o["cf"])
    assert g["evals"] == o["evals"], what + ": evals"


def mixed_cloud(dim, seed):
    """2 * 8192 + 37 points = three chunks, the last of 37.  Three clumps of 5000 points, each inside one grid row (a
    run of 35 cells along x in 2-D, of 4 in 3-D) and far more than eps from the others; 1421 background points over the whole grid (2-D: 700 x
    700 cells, 31 buckets of 2^14 cells; 3-D: 80^3 cells), i.e. about five per bucket and chunk; six points with a NaN or
    infinite coordinate.  Caller order is shuffled, so every trip of 1024 points brings each clump's bucket some 300
    records (pairs inside a trip) and the background's buckets one or none (pairs across trips, runs of length one, runs
    that start on an odd slot or end on an even one)."""
    rng = np.random.default_rng(seed)
    n = 2 * PCH_MIN + 37
    ext = 700.0 if dim == 2 else 80.0
    parts = []
    for k in range(3):
        c = np.empty((5000, dim))
        c[:, 0] = (0.1 + 0.4 * (k % 2) + rng.random(5000) * 0.05) * ext
        c[:, 1:] = (0.2 + 0.25 * (k + 1)) * ext + 0.3 + rng.random((5000, dim - 1)) * 0.5
        parts.append(c)
    bg = rng.random((n - 15000, dim)) * ext
    bg[0], bg[1] = 0.0, ext  # the bounding box
    parts.append(bg)
    c = np.round(np.concatenate(parts) * Q) / Q
    c = c[rng.permutation(n)]
    bad = rng.choice(n, 6, replace=False)
    c[bad[0]] = np.nan
    c[bad[1], 0] = np.inf
    c[bad[2], 1] = -np.inf
    c[bad[3], dim - 1] = np.nan
    c[bad[4], 0] = -np.inf
    c[bad[5], dim - 1] = np.inf
    return c


def case_tiny(ctx, O, N):
    rng = np.random.default_rng(11)
    for n in (1, 2, 3, 1023):
        for metric, dim in ((N.L1_2D, 2), (N.L2_3D, 3)):
            c = np.round(rng.random((n, dim)) * 8.0 * Q) / Q
            for mp in (1, 3):
                same(ctx.dbscan(c, 0.5, mp, metric), O.dbscan(c, 0.5, mp, metric, literal=True),
                     "n=%d metric=%d minPts=%d" % (n, metric, mp))


def case_mixed2d(ctx, O, N):
    c = mixed_cloud(2, 5)
    same(ctx.dbscan(c, 1.0, 5, N.L1_2D), O.dbscan(c, 1.0, 5, N.L1_2D), "mixed 2-D")


def case_mixed3d(ctx, O, N):
    c = mixed_cloud(3, 6)
    same(ctx.dbscan(c, 1.0, 5, N.L2_3D), O.dbscan(c, 1.0, 5, N.L2_3D), "mixed 3-D")


def case_grouped(ctx, O, N):
    """Staged block pipeline, three shares: every vcp_blocks_cluster_dev call is one grouped launch of the grid engine
    that leaves the other shares' points (and those of the blocks small enough for the all-pairs kernel) out."""
    import torch
    from vtkcloudpoint_amd import synth
    motor = synth.config_cloud(20_000, seed=31)["motor"]
    eps, mp, pic = 0.1, 10, 1500
    o = O.block_pipeline(motor, eps, mp, pic, 3)
    sizes = np.bincount(o["block_of"][o["block_of"] >= 0])
    assert (sizes > 1024).sum() >= 3, "the cloud has to give the engine blocks in more than one share"
    info = ctx.blocks_begin(motor, eps, mp, pic, 3)
    assert info["rows"] == o["rows"] and info["cols"] == o["cols"] and info["m"] == len(o["order"])
    m, n = info["m"], len(motor)
    local = torch.zeros(m, dtype=torch.int32, device="cuda")
    evals = 0
    for r in range(3):
        lo, hi, _, _ = ctx.blocks_share(r, 3)
        evals += ctx.blocks_cluster_dev(lo, hi, local.data_ptr())
    labels = torch.zeros(n, dtype=torch.int32, device="cuda")
    block_of = torch.zeros(n, dtype=torch.int32, device="cuda")
    order = torch.zeros(m, dtype=torch.int64, device="cuda")
    out = ctx.blocks_finish_dev(local.data_ptr(), evals, labels.data_ptr(), block_of.data_ptr(), order.data_ptr())
    assert np.array_equal(labels.cpu().numpy(), o["labels"]), "grouped: labels"
    assert np.array_equal(block_of.cpu().numpy(), o["block_of"]), "grouped: block_of"
    assert np.array_equal(order.cpu().numpy(), o["order"]), "grouped: order"
    for k in ("kept", "del_sum", "cluster_amount", "evals"):
        assert out[k] == o[k], "grouped: %s %r != %r" % (k, out[k], o[k])


def case_fallback(ctx, O, N):
    """250 k uniform points on 2740 x 2740 cells with VCP_CPB_LOG2=10: 7 507 600 cells / 2^10 = 7332 buckets, more than
    the 6826 whose stash fits the LDS and fewer than MAXB, so the scatter pass runs without the stash either way."""
    assert os.environ.get("VCP_CPB_LOG2") == "10"
    rng = np.random.default_rng(9)
    n, eps, D = 250_000, 1.0, 2740
    ext = (D - 0.5) * eps * 1.0007  # cell edge = eps * (1 + 6.5e-4) on this extent: D - 0.37 edges, D cells per axis
    c = np.round(rng.random((n, 2)) * ext * Q) / Q
    c[0], c[1] = 0.0, np.round(ext * Q) / Q
    ns = (D * D + 1 + 1023) >> 10
    assert STASH_MAX < ns <= MAXB and D * D <= 32 * n, ns
    same(ctx.dbscan(c, eps, 3, N.L1_2D), O.dbscan(c, eps, 3, N.L1_2D), "fallback")


CASES = {"tiny": case_tiny, "mixed2d": case_mixed2d, "mixed3d": case_mixed3d, "grouped": case_grouped,
         "fallback": case_fallback}


def main():
    from oracle import binding as O
    from vtkcloudpoint_amd import _native as N
    O.build()
    ctx = N.Context(0)
    try:
        CASES[sys.argv[1]](ctx, O, N)
    finally:
        ctx.close()
    print("ok", sys.argv[1], "VCP_PART_PAIRS=%s" % os.environ.get("VCP_PART_PAIRS", "(unset)"))


if __name__ == "__main__":
    main()
