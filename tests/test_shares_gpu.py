"""The sharded block pipeline (vcp_blocks_plan_dev / plan_cuts / build_dev / cluster_dev / finish_local / zero / zcoords /
pairs, driven by distributed.sharded_pipeline_local and by vcp_dbscan_blocks_multi) on the shares where something unusual
happens, against the CPU oracle's single-process pipeline (or the single-device vcp_dbscan_blocks):
  - empty trailing shares: the last super-bucket (the points in no block) holds more than n / world points, and the ranks
    behind it get [NS, NS);
  - empty middle shares: one block holds most of the cloud;
  - coarse super-buckets (fsh > 0, more than 2^15 blocks): shares that start inside the super-bucket list;
  - fewer points than ranks, the keyed partition, and 4 / 8 / 16 contexts of vcp_multi.
Every case asserts that its degenerate condition really occurred, read from the product's own plan."""
import numpy as np
import pytest
import torch

from vtkcloudpoint_amd import _native as N
from vtkcloudpoint_amd import distributed as D
from vtkcloudpoint_amd import synth

pytestmark = pytest.mark.gpu

EPS, MIN_PTS = 0.25, 3
# (columns, rows, ptsInCell) of a lattice of step 0.25 -> the worlds at which the last rank's share is empty
LATTICES = {(3, 300, 12): (4, 8, 16), (4, 200, 20): (8, 16), (2, 500, 10): (4, 8, 16), (2, 40000, 4): (4, 8, 16)}
KEYS = ("rows", "cols", "kept", "del_sum", "cluster_amount", "evals")


def lattice(cols, rows, step=0.25):
    x, y = np.meshgrid(np.arange(cols), np.arange(rows))
    return np.ascontiguousarray(np.stack([x.ravel(), y.ravel()], 1).astype(np.float64) * step)


def disk_in_background():
    """20 k points in a disk of radius 0.01 inside 2 k uniform points: one block holds 90 % of the cloud."""
    rng = np.random.default_rng(5)
    bg = rng.random((2000, 2)) * 10
    ang, rad = rng.random(20000) * 2 * np.pi, 0.01 * np.sqrt(rng.random(20000))
    disk = np.stack([5.3 + rad * np.cos(ang), 5.3 + rad * np.sin(ang)], 1)
    return np.ascontiguousarray(np.concatenate([bg, disk]))


@pytest.fixture(scope="module")
def ranks():
    ctxs = [N.Context(0) for _ in range(16)]
    yield ctxs
    for c in ctxs:
        c.close()


_ORACLE = {}


def _oracle(oracle, name, motor, eps, mp, pic, key=None):
    """one oracle run per cloud (its noise pass is quadratic in the zero list), reused across worlds and noise modes"""
    if name not in _ORACLE:
        _ORACLE[name] = oracle.block_pipeline(motor, eps, mp, pic, 3, key_xy=key)
    return _ORACLE[name]


def _plan(ctx, d, n, eps, mp, pic, world, dk=None):
    """the product's own partition: (nblocks, nsuper, cuts)"""
    info = ctx.blocks_plan(d.data_ptr(), n, eps, mp, pic, 3, None if dk is None else dk.data_ptr())
    return info["nblocks"], info["nsuper"], ctx.blocks_plan_cuts(world)


def _sharded(ctxs, d, n, eps, mp, pic, noise, dk=None):
    torch.cuda.synchronize()
    res = D.sharded_pipeline_local(ctxs, d.data_ptr(), n, eps, mp, pic, 3, device="cuda", noise=noise,
                                   d_key=None if dk is None else dk.data_ptr())
    torch.cuda.synchronize()
    return res


def _check(res, ref, nblocks, what):
    for q, r in enumerate(res):
        assert np.array_equal(r["labels"].cpu().numpy(), ref["labels"]), "%s rank %d: labels" % (what, q)
        for k in KEYS:
            assert r[k] == ref[k], "%s rank %d: %s %r != %r" % (what, q, k, r[k], ref[k])
        assert r["m"] == len(ref["order"]), "%s rank %d: m" % (what, q)
    ranges = [r["block_range"] for r in res]
    assert ranges[0][0] == 0 and ranges[-1][1] == nblocks, (what, ranges)
    assert all(lo <= hi for lo, hi in ranges), (what, ranges)
    assert all(a[1] == b[0] for a, b in zip(ranges, ranges[1:])), (what, ranges)
    return ranges


@pytest.mark.parametrize("cols,rows,pic", list(LATTICES))
def test_empty_trailing_shares(ranks, oracle, cols, rows, pic):
    motor = lattice(cols, rows)
    n = len(motor)
    d = torch.from_numpy(motor).cuda()
    o = _oracle(oracle, ("lattice", cols, rows), motor, EPS, MIN_PTS, pic)
    for world in LATTICES[(cols, rows, pic)]:
        nblocks, nsuper, cuts = _plan(ranks[0], d, n, EPS, MIN_PTS, pic, world)
        assert cuts[world - 1] == nsuper, (cols, rows, world, cuts)
        empty = sum(1 for r in range(world) if cuts[r] == cuts[r + 1] == nsuper)
        print("%dx%d pic %d world %d: nblocks %d nsuper %d, %d trailing shares empty" % (cols, rows, pic, world, nblocks,
                                                                                       nsuper, empty))
        for noise in ("gather", "slabs"):
            what = "%dx%d world %d %s" % (cols, rows, world, noise)
            res = _sharded(ranks[:world], d, n, EPS, MIN_PTS, pic, noise)
            ranges = _check(res, o, nblocks, what)
            assert ranges[-1] == (nblocks, nblocks) and res[-1]["m_local"] == 0, what


@pytest.mark.parametrize("world", [2, 3, 4])
def test_coarse_super_buckets_lattice(ranks, oracle, world):
    motor = lattice(2, 40000)
    n = len(motor)
    d = torch.from_numpy(motor).cuda()
    o = _oracle(oracle, ("lattice", 2, 40000), motor, EPS, MIN_PTS, 4)
    nblocks, nsuper, cuts = _plan(ranks[0], d, n, EPS, MIN_PTS, 4, world)
    assert nsuper < nblocks + 1 and 0 < cuts[1] < nsuper, (nblocks, nsuper, cuts)  # fsh > 0; rank 1 starts inside the list
    print("2x40000 world %d: nblocks %d nsuper %d (fsh > 0), cuts %s" % (world, nblocks, nsuper, cuts))
    res = _sharded(ranks[:world], d, n, EPS, MIN_PTS, 4, ("gather", "slabs")[world % 2])
    _check(res, o, nblocks, "2x40000 world %d" % world)


@pytest.fixture(scope="module")
def cloud_1m(vcp_ctx):
    """45 k blocks at ptsInCell 10 (fsh = 1) and the single-device result"""
    d = synth.config_cloud(1_000_000, seed=3)
    motor = np.ascontiguousarray(d["motor"])
    return motor, vcp_ctx.dbscan_blocks(motor, 0.07, 7, 10, 3)


@pytest.mark.parametrize("world", [3, 5, 8])
def test_coarse_super_buckets_1m(ranks, oracle, cloud_1m, world):
    motor, ref = cloud_1m
    n = len(motor)
    d = torch.from_numpy(motor).cuda()
    nblocks, nsuper, cuts = _plan(ranks[0], d, n, 0.07, 7, 10, world)
    assert nblocks >= 32768 and nsuper < nblocks + 1, (nblocks, nsuper)
    assert all(0 < cuts[r] < cuts[r + 1] for r in range(1, world)), cuts  # every share non-empty, all but one start inside
    print("1M world %d: nblocks %d nsuper %d (fsh > 0), cuts %s" % (world, nblocks, nsuper, cuts))
    if world == 5:  # the single-device call itself against the oracle, once
        o = _oracle(oracle, "1m", motor, 0.07, 7, 10)
        for k in ("labels", "block_of", "order") + KEYS:
            assert np.array_equal(ref[k], o[k]), k
    res = _sharded(ranks[:world], d, n, 0.07, 7, 10, ("gather", "slabs")[world % 2])
    _check(res, ref, nblocks, "1M world %d" % world)


@pytest.mark.parametrize("world", [4, 8])
def test_empty_middle_shares(ranks, oracle, world):
    motor = disk_in_background()
    n = len(motor)
    d = torch.from_numpy(motor).cuda()
    o = _oracle(oracle, "disk", motor, 0.002, 5, 20)
    nblocks, nsuper, cuts = _plan(ranks[0], d, n, 0.002, 5, 20, world)
    middle = [r for r in range(world) if cuts[r] == cuts[r + 1] < nsuper]
    assert middle, cuts
    print("disk world %d: nblocks %d nsuper %d, empty middle shares %s, cuts %s" % (world, nblocks, nsuper, middle, cuts))
    for noise in ("gather", "slabs"):
        res = _sharded(ranks[:world], d, n, 0.002, 5, 20, noise)
        ranges = _check(res, o, nblocks, "disk world %d %s" % (world, noise))
        for r in middle:
            assert ranges[r][0] == ranges[r][1] and res[r]["m_local"] == 0


# (points, ptsInCell, minPts): found with the oracle; the -3 and -4 ones raise there
TINY = [
    ([[0.25, 0.25], [0.0, 0.0], [0.0, 0.25], [1.0, 0.75], [1.25, 0.75], [0.75, 1.25], [1.0, 0.75]], 2, 2),
    ([[1.25, 0.0], [0.0, 1.0], [1.25, 0.25], [0.25, 1.25], [0.5, 0.25], [1.0, 0.25]], 2, 3),
    ([[0.25, 0.5], [1.0, 0.5], [0.0, 0.5], [0.75, 1.0], [1.0, 1.25], [0.25, 1.25], [0.0, 0.75]], 1, 1),   # -3
    ([[1.0, 0.5], [0.75, 0.75], [0.25, 1.25], [0.0, 0.25], [0.5, 0.75], [0.5, 0.0], [0.0, 0.0]], 3, 1),   # -4
]


def test_fewer_points_than_ranks(ranks, oracle):
    world = 8
    n_err = n_ok = 0
    for k, (pts, pic, mp) in enumerate(TINY):
        motor = np.ascontiguousarray(np.array(pts, np.float64))
        n = len(motor)
        assert n < world
        d = torch.from_numpy(motor).cuda()
        try:
            o = oracle.block_pipeline(motor, 0.3, mp, pic, 3)
        except oracle.OracleError as e:
            n_err += 1
            with pytest.raises((N.VcpError, IndexError)) as ge:
                _sharded(ranks[:world], d, n, 0.3, mp, pic, "gather")
            if isinstance(ge.value, N.VcpError):
                assert ge.value.code == e.code, "case %d error code" % k
            else:  # found by the driver from the ranks' flags: the C#'s clusForMerge[-1] (VCP_ERR_INDEX)
                assert e.code == -4, "case %d" % k
            print("tiny %d: %d points at world %d, error %d as the oracle" % (k, n, world, e.code))
            continue
        n_ok += 1
        nblocks, nsuper, cuts = _plan(ranks[0], d, n, 0.3, mp, pic, world)
        empty = [r for r in range(world) if cuts[r] == cuts[r + 1]]
        assert empty, cuts
        print("tiny %d: %d points at world %d, empty shares %s" % (k, n, world, empty))
        for noise in ("gather", "slabs"):
            _check(_sharded(ranks[:world], d, n, 0.3, mp, pic, noise), o, nblocks, "tiny %d %s" % (k, noise))
    assert n_err >= 2 and n_ok >= 2


@pytest.mark.parametrize("world", [4, 16])
def test_keyed_partition_empty_shares(ranks, oracle, world):
    """getClusterFromList: the partition reads (X, Y) = a lattice whose last bucket is heavy, the clustering reads motor."""
    key = lattice(3, 300)
    motor = np.ascontiguousarray(key + np.random.default_rng(8).normal(0.0, 0.05, key.shape))
    n = len(motor)
    dm, dk = torch.from_numpy(motor).cuda(), torch.from_numpy(key).cuda()
    o = _oracle(oracle, "keyed", motor, EPS, MIN_PTS, 12, key=key)
    nblocks, nsuper, cuts = _plan(ranks[0], dm, n, EPS, MIN_PTS, 12, world, dk)
    assert cuts[world - 1] == nsuper, cuts
    print("keyed 3x300 world %d: nblocks %d nsuper %d, cuts %s" % (world, nblocks, nsuper, cuts))
    for noise in ("gather", "slabs"):
        res = _sharded(ranks[:world], dm, n, EPS, MIN_PTS, 12, noise, dk)
        _check(res, o, nblocks, "keyed world %d %s" % (world, noise))
        assert res[0]["noise_active"] == res[0]["noise_points"]


@pytest.mark.parametrize("k", [4, 8, 16])
def test_multi_contexts_on_degenerate_shares(ranks, oracle, vcp_ctx, cloud_1m, k):
    """vcp_dbscan_blocks_multi with k contexts on the one GPU: the lattices (empty trailing shares) and the 1 M cloud
    (fsh > 0) give what the single-device call and the oracle give, order and block of every point included."""
    clouds = [(("lattice", c, r), lattice(c, r), EPS, MIN_PTS, pic, k in worlds) for (c, r, pic), worlds in LATTICES.items()]
    motor_1m, ref_1m = cloud_1m
    clouds.append(("1m", motor_1m, 0.07, 7, 10, False))
    mg = N.MultiContext([0] * k)
    try:
        assert mg.count() == k
        for name, motor, eps, mp, pic, degenerate in clouds:
            n = len(motor)
            d = torch.from_numpy(motor).cuda()
            nblocks, nsuper, cuts = _plan(ranks[0], d, n, eps, mp, pic, k)
            if degenerate:
                assert cuts[k - 1] == nsuper, (name, cuts)
            if name == "1m":
                assert nsuper < nblocks + 1, (nblocks, nsuper)
            print("multi %d %s: nblocks %d nsuper %d, empty trailing %s" % (k, name, nblocks, nsuper, cuts[k - 1] == nsuper))
            g = mg.dbscan_blocks(motor, eps, mp, pic, 3)
            refs = [ref_1m] if name == "1m" else [vcp_ctx.dbscan_blocks(motor, eps, mp, pic, 3),
                                                  _oracle(oracle, name, motor, eps, mp, pic)]
            for ref in refs:
                for key in ("labels", "block_of", "order") + KEYS:
                    assert np.array_equal(g[key], ref[key]), (name, k, key)
    finally:
        mg.close()
