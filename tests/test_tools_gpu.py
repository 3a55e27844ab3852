"""GPU parity for the Tools part of the path (centroids, centroid merge, dictionary refresh) and the
centroid<->truth matching, through the C-ABI, vs the CPU oracle."""
import numpy as np
import pytest

import centroid_ref as R
from vtkcloudpoint_amd import _native as N
from vtkcloudpoint_amd import synth

pytestmark = pytest.mark.gpu
RTOL = 1e-12  # fixed-order tree sum vs the C#'s sequential sum; beside it, bit for bit vs the tree's replay


def same(a, b):
    return np.array_equal(a, b, equal_nan=True)


def test_centroids_c1_and_1m(vcp_ctx, oracle):
    for d in (synth.config_c1(), synth.config_cloud(1_000_000)):
        o = oracle.dbscan(d["motor"], d["eps_l1"], d["min_pts"])
        K = o["cf"]
        c3, c2, cnt = vcp_ctx.centroids(d["xyz"], d["motor"], o["labels"], K)
        r3, r2, rc = oracle.centroids(d["xyz"], d["motor"], o["labels"], K)
        assert np.array_equal(cnt, rc)
        assert np.allclose(c3, r3, rtol=RTOL, atol=1e-12) and np.allclose(c2, r2, rtol=RTOL, atol=1e-12)
        t3, t2, tc = R.tree_centroids(d["xyz"], d["motor"], o["labels"], K)
        assert same(c3, t3) and same(c2, t2) and np.array_equal(cnt, tc)
        # run-to-run deterministic (fixed reduction tree)
        c3b, c2b, _ = vcp_ctx.centroids(d["xyz"], d["motor"], o["labels"], K)
        assert np.array_equal(c3, c3b) and np.array_equal(c2, c2b)


def test_centroids_edge_cases(vcp_ctx, oracle):
    rng = np.random.default_rng(5)
    n = 5000
    xyz = rng.random((n, 3))
    motor = rng.random((n, 2))
    lab = rng.integers(0, 8, n).astype(np.int32)
    lab[lab == 3] = 0  # cluster 3 empty -> NaN row, count 0 (Tools.cs:191 skips it)
    c3, c2, cnt = vcp_ctx.centroids(xyz, motor, lab, 9)
    r3, r2, rc = oracle.centroids(xyz, motor, lab, 9)
    assert np.array_equal(cnt, rc) and cnt[2] == 0 and cnt[8] == 0
    assert np.allclose(c3, r3, rtol=RTOL, equal_nan=True) and np.allclose(c2, r2, rtol=RTOL, equal_nan=True)
    t3, t2, _ = R.tree_centroids(xyz, motor, lab, 9)
    assert same(c3, t3) and same(c2, t2)
    # a giant cluster spanning many chunks (3 full ones and a part of a fourth) and all-noise input
    big = 3 * R.CH + 1000
    bxyz = rng.random((big, 3))
    c3, _, cnt = vcp_ctx.centroids(bxyz, None, np.ones(big, np.int32), 1)
    assert cnt[0] == big > 3 * R.CH and np.allclose(c3[0], bxyz.mean(0), rtol=1e-12)
    assert same(c3, R.tree_centroids(bxyz, None, np.ones(big, np.int32), 1)[0])
    lab[:] = 1
    c3, _, cnt = vcp_ctx.centroids(xyz, None, lab, 1)
    assert cnt[0] == n and np.allclose(c3[0], xyz.mean(0), rtol=1e-12)
    lab[:] = 0
    _, _, cnt = vcp_ctx.centroids(xyz, motor, lab, 4)
    assert cnt.sum() == 0
    # label beyond K -> the C# indexes clusList out of range
    lab[7] = 5
    with pytest.raises(N.VcpError) as e:
        vcp_ctx.centroids(xyz, motor, lab, 4)
    assert e.value.code == -4


def test_merge_and_refresh(vcp_ctx, oracle):
    d = synth.config_cloud(200_000, seed=9)
    o = oracle.dbscan(d["motor"], d["eps_l1"], d["min_pts"])
    K = o["cf"]
    r3, r2, rc = oracle.centroids(d["xyz"], d["motor"], o["labels"], K)
    ids = np.arange(1, K + 1, dtype=np.int32)
    for thr in (0.1, 0.5, 2.0):
        mo, co = oracle.merge_ids(r3[:, :2], ids, thr)
        mg, cg = vcp_ctx.merge_centroids(r3[:, :2], ids, thr)
        assert np.array_equal(mo, mg) and co == cg
        lo, ko, o3, o2, oc = oracle.refresh_by_dictionary(d["xyz"], d["motor"], o["labels"], K, mo)
        lg, kg, g3, g2, gc = vcp_ctx.refresh_by_dictionary(d["xyz"], d["motor"], o["labels"], K, mg)
        assert ko == kg and np.array_equal(lo, lg) and np.array_equal(oc, gc)
        assert np.allclose(o3, g3, rtol=RTOL, atol=1e-12) and np.allclose(o2, g2, rtol=RTOL, atol=1e-12)
        tl, tk, t3, t2, tc = R.tree_refresh(d["xyz"], d["motor"], o["labels"], K, mg)
        assert tk == kg and np.array_equal(tl, lg) and np.array_equal(tc, gc) and same(g3, t3) and same(g2, t2)
    assert co > 0  # the largest threshold really merges something


def test_match(vcp_ctx, oracle):
    rng = np.random.default_rng(11)
    K, T = 3000, 257
    truths = rng.random((T, 3)) * 100
    centers = rng.random((K, 3)) * 100
    # exact ties: duplicate truth points (lowest index must win) and centroids sitting on truths
    truths[100] = truths[7]
    centers[:50] = truths[:50]
    M = np.eye(4)
    M[:3, :3] = synth.rotation_about((0, 0, 1), 2.0)
    M[:3, 3] = (0.5, -0.25, 0.125)
    o = oracle.match(centers, truths, M, 5.0)
    g = vcp_ctx.match(centers, truths, M, 5.0)
    assert np.array_equal(o["matched_xyz"], g["matched_xyz"])
    assert np.array_equal(o["nearest"], g["nearest"])
    assert np.array_equal(o["nearest_dist"], g["nearest_dist"])  # correctly rounded sqrt on both sides
    assert np.array_equal(o["is_matched"], g["is_matched"]) and o["count"] == g["count"]
    with pytest.raises(N.VcpError) as e:
        vcp_ctx.match(centers, np.zeros((0, 3)), M, 5.0)
    assert e.value.code == -2


def test_match_long_truth_list_through_the_grid(vcp_ctx, oracle):
    """T > 512: the truths are binned (csrc/nngrid.hpp).  RecorrectMatchingPtsByDistance compares correctly rounded
    sqrt distances with strict `<` (FrmMain.cs:3588-3618, getDisP :829-835): ties AFTER the sqrt go to the lowest truth
    index too.  30 k x 30 k on a lattice (exact ties), duplicates, centroids far away, non-finite centroid."""
    rng = np.random.default_rng(12)
    K = T = 30_000
    truths = rng.integers(0, 80, size=(T, 3)).astype(np.float64) * 0.5
    centers = rng.integers(0, 160, size=(K, 3)).astype(np.float64) * 0.25
    truths[9000:9100] = truths[:100]
    centers[:100] += 500.0
    M = np.eye(4)
    o = oracle.match(centers, truths, M, 0.6)
    g = vcp_ctx.match(centers, truths, M, 0.6)
    for k in ("matched_xyz", "nearest", "nearest_dist", "is_matched"):
        assert np.array_equal(o[k], g[k]), k
    assert o["count"] == g["count"]
    # generic positions + a rigid transform; nearly equal distances that the sqrt merges
    truths = rng.random((T, 3)) * 200
    centers = truths[rng.permutation(T)] + rng.normal(0, 1e-9, (K, 3))
    centers[5] = np.nan
    centers[6] = np.inf
    M[:3, :3] = synth.rotation_about((0, 0, 1), 0.01)
    M[:3, 3] = (0.05, -0.025, 0.0125)
    o = oracle.match(centers, truths, M, 0.5)
    g = vcp_ctx.match(centers, truths, M, 0.5)
    assert np.array_equal(o["nearest"], g["nearest"]) and np.array_equal(o["is_matched"], g["is_matched"])
    assert np.array_equal(o["nearest_dist"], g["nearest_dist"], equal_nan=True) and o["count"] == g["count"]


def test_minimal_bounding_circles(vcp_ctx, oracle):
    """Tools.getCircles / Geometry.FindMinimalBoundingCircle: bit-exact vs the literal port."""
    # hand-checkable: the circumcircle of a square, and an obtuse triangle (circle on the longest side)
    xy = np.array([[0, 0], [2, 0], [2, 2], [0, 2], [1, 1], [0.5, 1.5], [10, 10], [14, 10], [11, 10.5], [12, 10.2]], float)
    lab = np.array([1, 1, 1, 1, 1, 1, 2, 2, 2, 2], np.int32)
    g = vcp_ctx.mcc(xy, lab, 2)
    assert g["valid"].tolist() == [1, 1] and np.allclose(g["centers"], [[1, 1], [12, 10]])
    assert np.allclose(g["radius"], [np.sqrt(2), 2.0]) and g["hull_n"][0] == 4
    for d in (synth.config_c1(), synth.config_cloud(300_000, seed=23)):
        o = oracle.block_pipeline(d["motor"], 0.1 if len(d["motor"]) > 20000 else 0.3, 10 if len(d["motor"]) > 20000 else 5, 200, 3)
        K = o["cluster_amount"]
        for coords in (d["motor"], d["xyz"][:, :2].copy()):  # the 2-D and the 3-D view (Tools.cs:394, is3D)
            ref = oracle.get_circles(coords, o["labels"], K, o["order"])
            got = vcp_ctx.mcc(coords, o["labels"], K, o["order"])
            assert np.array_equal(ref["valid"], got["valid"]) and np.array_equal(ref["hull_n"], got["hull_n"])
            assert np.array_equal(ref["centers"], got["centers"]) and np.array_equal(ref["radius"], got["radius"])
            assert ref["valid"].sum() > 0
    # clusters of <= 3 points are skipped (Tools.cs:400); labels beyond K index clusList out of range
    g = vcp_ctx.mcc(xy[:3], np.array([1, 1, 1], np.int32), 1)
    assert g["valid"].tolist() == [0]
    with pytest.raises(N.VcpError) as e:
        vcp_ctx.mcc(xy, lab + 5, 2)
    assert e.value.code == -4


def test_truth_guided_assignment(vcp_ctx, oracle):
    """MainForm.refreshClusList: nearest truth within the radius, last one wins ties."""
    rng = np.random.default_rng(8)
    d = synth.config_cloud(500_000, seed=31)
    T = 300
    txy = rng.random((T, 2)) * d["motor_extent"]
    txy[50] = txy[10]                      # duplicated truth: equal distances -> the later one (50) wins
    tids = np.arange(1, T + 1, dtype=np.int32)
    tids[7] = 0                            # a truth with clusterId 0 behaves like "none"
    for radius in (2.0, 20.0):
        o_ids, o_out = oracle.assign_truths(d["motor"], txy, tids, radius)
        g_ids, g_out = vcp_ctx.assign_truths(d["motor"], txy, tids, radius)
        assert np.array_equal(o_ids, g_ids) and o_out == g_out
    assert (g_ids == 51).any() and not (g_ids == 11).any()
    ids, out = vcp_ctx.assign_truths(d["motor"][:10], np.zeros((0, 2)), np.zeros(0, np.int32), 1.0)
    assert out == 10 and not ids.any()


def test_truth_grid_equals_brute_force(vcp_ctx, oracle):
    """The grid over the truths (radius-sized cells) against the oracle's literal LINQ query: lattice coordinates
    give many exactly equal distances (the LAST truth in list order must win), duplicate truths, truths with NaN /
    inf coordinates, raw points far outside the truths' bounding box, and radii for which the grid does not apply
    (0, negative, inf, NaN -> brute-force kernel)."""
    rng = np.random.default_rng(77)
    n, T = 60_000, 900
    motor = rng.integers(-40, 240, size=(n, 2)).astype(np.float64) * 0.25
    motor[::501] = np.nan
    txy = rng.integers(0, 160, size=(T, 2)).astype(np.float64) * 0.25
    txy[100:130] = txy[0:30]                      # duplicates: the later one wins
    txy[5] = (np.nan, 1.0)
    txy[6] = (np.inf, 2.0)
    tids = rng.integers(0, 50, size=T).astype(np.int32)
    for radius in (0.75, 1.0, 2.5, 13.0, 1e6, 0.0, -1.0, float("inf"), float("nan")):
        o_ids, o_out = oracle.assign_truths(motor, txy, tids, radius)
        g_ids, g_out = vcp_ctx.assign_truths(motor, txy, tids, radius)
        assert np.array_equal(o_ids, g_ids) and o_out == g_out, radius
    # a single truth, and truths on one vertical line (zero extent in x)
    line = np.c_[np.full(40, 3.0), np.arange(40) * 0.5]
    for t in (txy[:1], line):
        ti = np.arange(1, len(t) + 1, dtype=np.int32)
        o_ids, o_out = oracle.assign_truths(motor, t, ti, 1.25)
        g_ids, g_out = vcp_ctx.assign_truths(motor, t, ti, 1.25)
        assert np.array_equal(o_ids, g_ids) and o_out == g_out


def test_truth_grid_subnormal_radius_on_a_box_of_no_extent(vcp_ctx, oracle):
    """Found by tests/fuzz_queries.py (assign_truths, seed 9, case 80): every truth at one place and a radius of
    5e-324, the double above the distance 0 of a raw point that sits on them.  The cell edge stays subnormal (a box of
    no extent needs no doubling), its reciprocal is +inf, and (p - x0) * inv_h = 0 * inf = NaN put that point outside
    the grid: id 0 where d = 0 < radius gives the last truth's id.  The same with the smallest radii whose reciprocal is
    still finite, and with a line of truths (extent in one axis only)."""
    spot = np.array([-699896.66055029, -699955.7594064])
    motor = np.array([spot + (7.8e-5, 7.2e-5), spot, spot - (1.2e-3, 7.9e-4), spot])
    tids = np.arange(1, 13, dtype=np.int32)
    for txy in (np.tile(spot, (12, 1)), np.c_[np.full(12, spot[0]), spot[1] + np.arange(12) * 0.5]):
        for radius in (5e-324, 1e-310, 5.562684646268003e-309, np.nextafter(5.562684646268003e-309, 1.0), 2.3e-308):
            o_ids, o_out = oracle.assign_truths(motor, txy, tids, radius)
            g_ids, g_out = vcp_ctx.assign_truths(motor, txy, tids, radius)
            assert o_ids[1] != 0 and o_ids[3] != 0 and o_out == 2
            assert np.array_equal(o_ids, g_ids) and o_out == g_out, radius


def test_import_conversion_and_duplicate_removal(vcp_ctx, oracle):
    """MainForm.AddFolder: Distance filter, spherical -> Cartesian, first-occurrence dedupe."""
    rng = np.random.default_rng(12)
    n = 400_000
    rows = np.c_[rng.random(n) * 40, rng.random(n) * 40, rng.random(n) * 1100]
    rows[200000:250000] = rows[0:50000]       # 50k exact duplicates of earlier rows
    rows[70000] = rows[123]
    rows[7, 2] = 0.0                          # filtered: Distance == 0
    o = oracle.import_convert(rows, 1.5, -0.5, 2, 1, True)
    g = vcp_ctx.import_convert(rows, 1.5, -0.5, 2, 1, True)
    assert np.array_equal(o["state"], g["state"]) and o["kept"] == g["kept"] and o["duplicates"] == g["duplicates"]
    assert g["duplicates"] >= 40000 and (g["state"] == 0).sum() > 0.05 * n
    assert np.allclose(o["xyz"], g["xyz"], rtol=1e-12, atol=1e-9)  # device sin/cos vs host libm: a few ulp
    # the hash version of the oracle equals the C#'s literal O(n^2) FindAll on a small prefix
    lit = oracle.import_convert(rows[:6000], 1.5, -0.5, 2, 1, True, literal=True)
    assert np.array_equal(lit["state"], oracle.import_convert(rows[:6000], 1.5, -0.5, 2, 1, True)["state"])
    assert np.array_equal(lit["state"], vcp_ctx.import_convert(rows[:6000], 1.5, -0.5, 2, 1, True)["state"])
    # no dedupe, other axis choices
    o = oracle.import_convert(rows, 0.0, 0.0, 4, 3, False)
    g = vcp_ctx.import_convert(rows, 0.0, 0.0, 4, 3, False)
    assert np.array_equal(o["state"], g["state"]) and np.allclose(o["xyz"], g["xyz"], rtol=1e-12, atol=1e-9)
    with pytest.raises(N.VcpError) as e:
        vcp_ctx.import_convert(rows[:10], 0.0, 0.0, 4, 3, True)
    assert e.value.code == -8


def test_fixed_points_centroid_weighted(vcp_ctx, oracle):
    """Tools.getFixedPtsCentroid (BC/Tools.cs:78-111; SureDistanceFilter.cs:74): ptsCount-weighted centroids of the
    deduplicated fixed points, with and without isIgnoreDuplication, vs the statement-by-statement oracle."""
    rng = np.random.default_rng(11)
    n, K = 60_000, 37
    xyz = rng.random((n, 3)) * 50
    group = rng.integers(0, K + 1, n).astype(np.int32)  # 0 = in no list
    group[:K] = np.arange(1, K + 1)  # no list is empty
    pts = rng.integers(1, 9, n).astype(np.int32)
    cid = np.where(rng.random(n) < 0.2, 0, group).astype(np.int32)  # some members carry clusterId 0
    for ignore in (False, True):
        for c in (cid, None):
            g3, gi = vcp_ctx.centroids_weighted(xyz, group, c, pts, K, ignore)
            o3, oi = oracle.fixed_centroids(xyz, group, c, pts, K, ignore)
            assert np.array_equal(gi, oi)
            assert np.allclose(g3, o3, rtol=RTOL, atol=1e-12)
            t3, ti = R.tree_centroids_weighted(xyz, group, c, pts, K, ignore)
            assert np.array_equal(gi, ti) and same(g3, t3)
    # unweighted limit: ptsCount 1 everywhere equals Tools.GetClusList's mean
    ones = np.ones(n, np.int32)
    g3, gi = vcp_ctx.centroids_weighted(xyz, group, None, ones, K, False)
    c3, _, cnt = vcp_ctx.centroids(xyz, None, group, K)
    assert np.array_equal(gi, cnt) and np.allclose(g3, c3, rtol=RTOL)
    # insideNum == 0 (all weights zero): 0/0 = NaN rows, like the C#
    z3, zi = vcp_ctx.centroids_weighted(xyz, group, None, np.zeros(n, np.int32), K, False)
    assert np.isnan(z3).all() and not zi.any()
    # an empty list: clusList[i].li[0] throws (Tools.cs:106)
    group[group == 5] = 0
    with pytest.raises(N.VcpError) as e:
        vcp_ctx.centroids_weighted(xyz, group, None, pts, K, False)
    assert e.value.code == -4
    with pytest.raises(oracle.OracleError):
        oracle.fixed_centroids(xyz, group, None, pts, K, False)
