"""vcp_cluster_shapes / vcp_cluster_filter on the MI355X: the circle stays vcp_mcc's, the hull is the oracle's, the
rectangle equals the numpy restatement of include/vcp.h bit for bit and is the minimum by an independent check, the
device forms return the host forms' bits, the filter equals its expression, and -- the reason for the feature -- the
filter in front of multi-start ICP removes the streaks that are no targets."""
import math

import numpy as np
import pytest

import shapes_ref as S
from icpms_data import angle_diff, angle_of, planted, random_truths
from vtkcloudpoint_amd import _native as N
from vtkcloudpoint_amd import synth

pytestmark = pytest.mark.gpu

RECT = ("rect_valid", "rect_edge", "rect_len", "rect_xy")


def _same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


@pytest.fixture(scope="module")
def clouds(oracle):
    """The clouds of test_minimal_bounding_circles: C1 and config_cloud(300 k, seed 23), motor and xy views, the
    oracle's block-pipeline labels and order."""
    out = []
    for d in (synth.config_c1(), synth.config_cloud(300_000, seed=23)):
        big = len(d["motor"]) > 20000
        o = oracle.block_pipeline(d["motor"], 0.1 if big else 0.3, 10 if big else 5, 200, 3)
        for coords in (d["motor"], d["xyz"][:, :2].copy()):
            out.append(dict(xy=np.ascontiguousarray(coords), labels=o["labels"], order=o["order"],
                            K=o["cluster_amount"]))
    return out


def _lattice_cloud():
    """Clusters built to tie: axis-parallel integer rectangles (opposite edges give equal areas), clusters on one
    line, clusters of one repeated point, a cluster of 3 points, noise; duplicates everywhere; list order shuffled."""
    rng = np.random.default_rng(17)
    pts, lab, kinds = [], [], []
    k = 0
    for w, h, x0, y0 in ((3, 1, 0, 0), (5, 5, 10, -3), (1, 7, -20, 4), (6, 2, 100, 100), (2, 2, 7, 50), (9, 4, -64, -64)):
        k += 1
        g = np.array([(x0 + i, y0 + j) for i in range(w + 1) for j in range(h + 1)], float)
        g = np.r_[g, g[rng.integers(0, len(g), 6)]]  # duplicates
        pts.append(g[rng.permutation(len(g))]), lab.append(np.full(len(g), k)), kinds.append("box")
    for a, b, cnt in ((1, 2, 6), (1, 0, 9), (0, 1, 5), (3, -1, 12), (0.125, 0.375, 7)):
        k += 1
        g = np.array([(30 + i * a, -7 + i * b) for i in range(cnt)], float)
        g = np.r_[g, g[:2]]
        pts.append(g[rng.permutation(len(g))]), lab.append(np.full(len(g), k)), kinds.append("line")
    for p, cnt in (((2.5, -1.0), 5), ((0.0, 0.0), 4), ((-3.0, 1e6), 9)):
        k += 1
        pts.append(np.tile([p], (cnt, 1))), lab.append(np.full(cnt, k)), kinds.append("point")
    k += 1
    pts.append(np.array([[0, 0], [1, 0], [0, 1]], float)), lab.append(np.full(3, k)), kinds.append("small")
    pts.append(rng.integers(-50, 50, (40, 2)).astype(float)), lab.append(np.zeros(40))
    xy, lab = np.concatenate(pts), np.concatenate(lab).astype(np.int32)
    order = rng.permutation(len(lab)).astype(np.int64)
    return dict(xy=np.ascontiguousarray(xy), labels=lab, order=order, K=k, kinds=kinds)


def _random_cloud():
    """Gaussian clusters of random anisotropy, uniformly filled boxes at random angles, clusters on the 2^-10 lattice
    and on a 6 x 6 integer lattice (duplicates, collinear runs); behind them 16 lines that are collinear up to rounding
    (centre + s * d in binary64), on which the reference's wrap can close early."""
    rng = np.random.default_rng(29)
    pts, lab, kinds = [], [], []
    for k in range(1, 161):
        cnt = int(rng.integers(8, 300))
        kind = ("gauss", "box", "fine", "coarse")[(k - 1) % 4]
        c = rng.uniform(-500, 500, 2)
        th = rng.uniform(0, math.pi)
        R = np.array([[math.cos(th), -math.sin(th)], [math.sin(th), math.cos(th)]])
        if kind == "gauss":
            g = rng.normal(0, 1, (cnt, 2)) * rng.uniform(0.2, 5.0, 2) @ R.T + c
        elif kind == "box":
            g = rng.uniform(-1, 1, (cnt, 2)) * rng.uniform(0.5, 8.0, 2) @ R.T + c
        elif kind == "fine":
            g = np.round((rng.normal(0, 0.05, (cnt, 2)) @ R.T + c) * 1024) / 1024
        else:
            g = rng.integers(0, 6, (cnt, 2)).astype(float) + np.round(c)
        pts.append(g), lab.append(np.full(cnt, k)), kinds.append(kind)
    near = np.random.default_rng(31)  # a stream of its own: the 160 clusters above stay what they were
    for k in range(161, 177):
        cnt = int(near.integers(5, 41))
        th = near.uniform(0, 2 * math.pi)
        d = np.array([math.cos(th), math.sin(th)]) * near.uniform(0.5, 3.0)
        g = near.uniform(-500, 500, 2) * (k % 2) + near.uniform(-1, 1, (cnt, 1)) * d
        pts.append(g), lab.append(np.full(cnt, k)), kinds.append("nearline")
    xy, lab = np.concatenate(pts), np.concatenate(lab).astype(np.int32)
    p = rng.permutation(len(lab))
    return dict(xy=np.ascontiguousarray(xy[p]), labels=lab[p], order=None, K=176, kinds=kinds)


def _oracle_hulls(oracle, c):
    """Per cluster: (member indices in list order, the oracle's hull or None for a cluster of <= 3 points).
    c["inserted"][k]: how many members the circle's insertion rule added (the rectangle then spans the members)."""
    if "hulls" not in c:
        fits = [oracle.min_circle_ex(c["xy"][idx]) if len(idx) > 3 else None
                for idx in S.members(c["labels"], c["K"], c["order"])]
        c["hulls"] = [(idx, None if f is None else f["hull"])
                      for idx, f in zip(S.members(c["labels"], c["K"], c["order"]), fits)]
        c["inserted"] = [0 if f is None else f["inserted"] for f in fits]
    return c["hulls"]


def _shapes(vcp_ctx, c):
    if "got" not in c:
        c["got"] = vcp_ctx.cluster_shapes(c["xy"], c["labels"], c["K"], c["order"])
    return c["got"]


def test_circle_unchanged(vcp_ctx, oracle, clouds):
    for c in list(clouds) + [_lattice_cloud(), _random_cloud()]:
        got = _shapes(vcp_ctx, c)
        mcc = vcp_ctx.mcc(c["xy"], c["labels"], c["K"], c["order"])
        ref = oracle.get_circles(c["xy"], c["labels"], c["K"], c["order"])
        for k in ("centers", "radius", "valid", "hull_n"):
            assert _same(got[k], mcc[k]) and _same(got[k], ref[k]), k
        assert ref["valid"].sum() > 0


def _check_hull(c, got, hulls, literal):
    xy, off, hidx = c["xy"], got["hull_off"], got["hull_idx"]
    assert off[0] == 0 and _same(np.diff(off), np.where(got["valid"] == 1, got["hull_n"], 0)) and off[-1] == len(hidx)
    for k, (idx, hull) in enumerate(hulls):
        if got["valid"][k] != 1:
            continue
        mine = hidx[off[k]:off[k + 1]]
        assert _same(xy[mine], hull), k
        used = set()
        for i in mine:  # the first list position with those coordinates that is still in the list
            eq = idx[(xy[idx, 0] == xy[i, 0]) & (xy[idx, 1] == xy[i, 1])]
            if literal:
                assert i == eq[0], k
            assert i == next(j for j in eq if j not in used), k
            used.add(int(i))


def test_hull_is_the_oracles_and_indexes_the_callers_points(vcp_ctx, oracle, clouds):
    for c in clouds:
        _check_hull(c, _shapes(vcp_ctx, c), _oracle_hulls(oracle, c), literal=True)
    for c in (_lattice_cloud(), _random_cloud()):
        _check_hull(c, _shapes(vcp_ctx, c), _oracle_hulls(oracle, c), literal=False)


def _check_rectangles(c, got, hulls):
    n_valid = 0
    for k, (idx, hull) in enumerate(hulls):
        if got["valid"][k] != 1:
            assert got["valid"][k] == 0 and hull is None
            assert got["rect_valid"][k] == 0 and got["rect_edge"][k] == -1
            assert not got["rect_len"][k].any() and not got["rect_xy"][k].any()
            continue
        r = S.rectangle(hull, c["xy"][idx] if c["inserted"][k] else None)
        assert got["rect_valid"][k] == r["valid"] and got["rect_edge"][k] == r["edge"], k
        assert _same(got["rect_len"][k], r["len"]) and _same(got["rect_xy"][k], r["xy"]), k
        assert r["valid"] == (1 if len(hull) >= 2 else 0)
        n_valid += 1
    return n_valid


def test_rectangle_bit_for_bit(vcp_ctx, oracle, clouds):
    for c in clouds:
        assert _check_rectangles(c, _shapes(vcp_ctx, c), _oracle_hulls(oracle, c)) > 0
    lat = _lattice_cloud()
    got, hulls = _shapes(vcp_ctx, lat), _oracle_hulls(oracle, lat)
    assert _check_rectangles(lat, got, hulls) == lat["K"] - 1
    for k, kind in enumerate(lat["kinds"]):
        if kind == "box":  # opposite edges tie exactly; the lower edge index wins
            areas = S.rectangle(hulls[k][1])["areas"]
            e = got["rect_edge"][k]
            assert sum(a == areas[e] for a in areas) >= 2 and all(a is None or a > areas[e] for a in areas[:e])
            assert got["rect_valid"][k] == 1 and got["rect_len"][k].min() > 0
        elif kind == "line":
            assert got["rect_valid"][k] == 1 and got["rect_len"][k, 1] == 0.0 and got["rect_len"][k, 0] > 0
        elif kind == "point":
            assert got["valid"][k] == 1 and got["hull_n"][k] == 1 and got["rect_valid"][k] == 0
            assert _same(got["rect_xy"][k], np.tile(hulls[k][1][0], (4, 1)))
        else:
            assert got["valid"][k] == 0
    rnd = _random_cloud()
    assert _check_rectangles(rnd, _shapes(vcp_ctx, rnd), _oracle_hulls(oracle, rnd)) == rnd["K"]


STEPS = 20000


def _min_box_area(pts):
    """Smallest axis-aligned bounding-box area of the points over STEPS rotations evenly spaced in [0, pi/2)."""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(pts)).cuda()
    best = math.inf
    chunk = max(1, min(STEPS, (1 << 24) // max(len(pts), 1)))
    for lo in range(0, STEPS, chunk):
        th = torch.arange(lo, min(lo + chunk, STEPS), dtype=torch.float64, device="cuda") * (math.pi / 2 / STEPS)
        cs, sn = torch.cos(th), torch.sin(th)
        x = t[:, 0:1] * cs + t[:, 1:2] * sn
        y = t[:, 1:2] * cs - t[:, 0:1] * sn
        area = (x.max(0).values - x.min(0).values) * (y.max(0).values - y.min(0).values)
        best = min(best, float(area.min()))
    return best


def test_rectangle_is_the_minimum(vcp_ctx, oracle, clouds):
    """A = len0 * len1 against the smallest bounding box S over 20 000 rotations (step d): A <= S (1 + 1e-12) and
    S <= A (1 + d (L/W + W/L)) -- the first-order growth of the box area half a step from the optimum, with a factor 2
    for the second-order term; every point inside the rectangle to 1e-12 (1 + max |coordinate|)."""
    d = math.pi / 2 / STEPS
    worst = 0.0
    for c in list(clouds) + [_lattice_cloud(), _random_cloud()]:
        got = _shapes(vcp_ctx, c)
        checked = 0
        for k, idx in enumerate(S.members(c["labels"], c["K"], c["order"])):
            if got["valid"][k] != 1:
                continue
            pts = c["xy"][idx]
            l0, l1 = got["rect_len"][k]
            tol = 1e-12 * (1 + np.abs(pts).max())
            if got["rect_valid"][k] == 1:
                assert S.inside_rectangle(pts, got["rect_xy"][k], tol) <= 0, k
            if not (got["rect_valid"][k] == 1 and l1 > 0):  # V == 0: the only clusters this check may skip
                assert not ("kinds" in c and c["kinds"][k] in ("gauss", "box")), k
                continue
            A, L, W = l0 * l1, max(l0, l1), min(l0, l1)
            Smin = _min_box_area(pts)
            assert A <= Smin * (1 + 1e-12), (k, A, Smin)
            assert Smin <= A * (1 + d * (L / W + W / L)), (k, A, Smin)
            worst = max(worst, Smin / A - 1)
            checked += 1
        assert checked > 0
    print("largest S / A - 1 = %.3g" % worst)


def _dev_shapes(vcp_ctx, c, full=True):
    import torch
    K, n = c["K"], len(c["labels"])
    order = c["order"]
    m = n if order is None else len(order)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    xy, lab = dev(c["xy"]), dev(c["labels"])
    od = None if order is None else dev(order)
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device="cuda")
    o = dict(centers=z((K, 2), torch.float64), radius=z(K, torch.float64), valid=z(K, torch.uint8), hull_n=z(K, torch.int32))
    if full:
        o.update(rect_xy=z((K, 4, 2), torch.float64), rect_len=z((K, 2), torch.float64), rect_edge=z(K, torch.int32),
                 rect_valid=z(K, torch.uint8), hull_off=z(K + 1, torch.int32), hull_idx=z(max(m, 1), torch.int32))
    torch.cuda.synchronize()
    p = {k: v.data_ptr() for k, v in o.items()}
    vcp_ctx.cluster_shapes_dev(xy.data_ptr(), lab.data_ptr(), None if od is None else od.data_ptr(), m, n, K, p["centers"],
                               p["radius"], p["valid"], p["hull_n"], p.get("rect_xy"), p.get("rect_len"), p.get("rect_edge"),
                               p.get("rect_valid"), p.get("hull_off"), p.get("hull_idx"))
    r = {k: v.cpu().numpy() for k, v in o.items()}
    if full:
        r["hull_idx"] = r["hull_idx"][: r["hull_off"][K]]
    return r


def test_device_form(vcp_ctx, clouds):
    for c in list(clouds) + [_lattice_cloud()]:
        host = _shapes(vcp_ctx, c)
        a, b = _dev_shapes(vcp_ctx, c), _dev_shapes(vcp_ctx, c)
        assert set(a) == set(host)
        for k in host:
            assert _same(a[k], host[k]), k
            assert _same(a[k], b[k]), k
        mcc = vcp_ctx.mcc(c["xy"], c["labels"], c["K"], c["order"])
        circle = _dev_shapes(vcp_ctx, c, full=False)
        for k in mcc:
            assert _same(circle[k], mcc[k]), k
        only = vcp_ctx.cluster_shapes(c["xy"], c["labels"], c["K"], c["order"], rect=False, hull=False)
        for k in mcc:
            assert _same(only[k], mcc[k]), k


def test_phases_and_errors(vcp_ctx):
    c = _lattice_cloud()
    vcp_ctx.timing_enable(True)
    try:
        vcp_ctx.cluster_shapes(c["xy"], c["labels"], c["K"], c["order"])
        assert [p for p, _ in vcp_ctx.timing()] == ["shapes_group", "shapes_fit", "shapes_hull"]
        g = vcp_ctx.cluster_shapes(c["xy"], c["labels"], c["K"], c["order"], hull=False)
        assert [p for p, _ in vcp_ctx.timing()] == ["shapes_group", "shapes_fit"]
        vcp_ctx.cluster_filter(c["labels"], c["K"], g["radius"], g["valid"], g["rect_len"], g["rect_valid"], 1.0, 2.0)
        assert [p for p, _ in vcp_ctx.timing()] == ["filter"]
    finally:
        vcp_ctx.timing_enable(False)
    with pytest.raises(N.VcpError) as e:
        vcp_ctx.cluster_shapes(c["xy"], c["labels"] + 5, c["K"], c["order"])
    assert e.value.code == -4
    xy = c["xy"].copy()
    xy[c["labels"] == 2] = np.nan  # a cluster without a finite point
    with pytest.raises(N.VcpError) as e:
        vcp_ctx.cluster_shapes(xy, c["labels"], c["K"], c["order"])
    assert e.value.code == -2
    th = np.arange(2100) * (2 * math.pi / 2100)  # 2100 points on a circle: every one is a hull point
    with pytest.raises(N.VcpError) as e:
        vcp_ctx.cluster_shapes(np.c_[np.cos(th), np.sin(th)], np.ones(2100, np.int32), 1)
    assert e.value.code == -5
    assert vcp_ctx.cluster_shapes(np.zeros((0, 2)), np.zeros(0, np.int32), 0)["hull_idx"].size == 0


def test_filter(vcp_ctx, clouds):
    import torch
    from vtkcloudpoint_amd.datamodel import ClusObj, Point3D
    from vtkcloudpoint_amd.tools import Tools
    c = clouds[2]  # the 300 k cloud, motor view
    g = _shapes(vcp_ctx, c)
    K, lab, n = c["K"], c["labels"], len(c["labels"])
    med = float(np.median(g["radius"][g["valid"] == 1]))
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    d_lab, d_rad, d_val, d_len, d_rv = dev(lab), dev(g["radius"]), dev(g["valid"]), dev(g["rect_len"]), dev(g["rect_valid"])
    for mr, ma in ((med, math.inf), (math.inf, 2.0), (med, 2.0), (math.nan, math.nan), (-1.0, math.inf)):
        ref = S.cluster_filter(lab, K, g["radius"], g["valid"], g["rect_len"], g["rect_valid"], mr, ma)
        got = vcp_ctx.cluster_filter(lab, K, g["radius"], g["valid"], g["rect_len"], g["rect_valid"], mr, ma)
        for k in ref:
            assert _same(ref[k], got[k]), (mr, ma, k)
        d_f = torch.zeros(K, dtype=torch.uint8, device="cuda")
        d_keep = torch.zeros(n, dtype=torch.uint8, device="cuda")
        d_idx = torch.zeros(n, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        nf, nk = vcp_ctx.cluster_filter_dev(d_lab.data_ptr(), n, K, d_rad.data_ptr(), d_val.data_ptr(), d_len.data_ptr(),
                                            d_rv.data_ptr(), mr, ma, d_f.data_ptr(), d_keep.data_ptr(), d_idx.data_ptr())
        assert (nf, nk) == (got["n_filtered"], got["n_kept"])
        assert _same(d_f.cpu().numpy(), got["filtered"]) and _same(d_keep.cpu().numpy(), got["keep"])
        assert _same(d_idx.cpu().numpy()[:nk], got["kept_idx"])
        nf2, nk2 = vcp_ctx.cluster_filter_dev(d_lab.data_ptr(), n, K, d_rad.data_ptr(), d_val.data_ptr(), d_len.data_ptr(),
                                              d_rv.data_ptr(), mr, ma, d_f.data_ptr())  # keep and kept_idx NULL
        assert (nf2, nk2) == (nf, nk)
        if mr != mr:
            assert got["n_filtered"] == 0 and got["n_kept"] == n
        if mr == -1.0:
            assert _same(got["filtered"], (g["valid"] == 1).astype(np.uint8)) and got["n_filtered"] > 0
        if ma == 2.0 and mr == math.inf:
            assert 0 < got["n_filtered"] < (g["valid"] == 1).sum()
    # radius alone (no rectangle arrays) is the reference's FilterClustersByRadius
    a = vcp_ctx.cluster_filter(lab, K, g["radius"], g["valid"], None, None, med, 2.0)
    b = S.cluster_filter(lab, K, g["radius"], g["valid"], None, None, med, math.inf)
    assert _same(a["filtered"], b["filtered"]) and _same(a["kept_idx"], b["kept_idx"])
    bad = lab.copy()
    bad[7] = K + 1
    with pytest.raises(N.VcpError) as e:
        vcp_ctx.cluster_filter(bad, K, g["radius"], g["valid"], g["rect_len"], g["rect_valid"], med, 2.0)
    assert e.value.code == -4
    # Tools.filterClusters + removeFilterPointFromClustering leave the points of kept_idx
    raw = [Point3D(0.0, 0.0, 0.0, int(l), True) for l in lab]
    for i, p in enumerate(raw):
        p.motor_x, p.motor_y, p.pathId = c["xy"][i, 0], c["xy"][i, 1], i
    clus = [ClusObj() for _ in range(K)]
    for i in c["order"]:
        if lab[i]:
            clus[lab[i] - 1].li.append(raw[i])
    ids = Tools.filterClusters(clus, False, med, 2.0, ctx=vcp_ctx)
    ref = S.cluster_filter(lab, K, g["radius"], g["valid"], g["rect_len"], g["rect_valid"], med, 2.0)
    assert ids == (np.flatnonzero(ref["filtered"]) + 1).tolist() and len(ids) > 0
    Tools.removeFilterPointFromClustering(raw, ids)
    assert [p.pathId for p in raw] == ref["kept_idx"].tolist()
    rects = Tools.getRectangles(clus, False, ctx=vcp_ctx)
    assert [r.clusID for r in rects] == (np.flatnonzero(g["rect_valid"]) + 1).tolist()
    assert all(_same(r.corners, g["rect_xy"][r.clusID - 1]) for r in rects)


def test_filter_in_front_of_multistart_icp(vcp_ctx):
    """K planar truths, per truth an isotropic blob of 200 raw points, K / 5 streaks of 200 points along a unit segment
    (transverse sigma 1 / 100 of its length) between them.  The filter at max_aspect = 3 removes every streak and no
    blob (blobs of 200 points reach aspect 1.83 at most, the streaks 12.6 at least); multi-start ICP on the centroids
    of the kept points makes every one of them an inlier, which the unfiltered centroids cannot."""
    K, dist, theta = 100, 2.0, math.radians(140.0)
    rng = np.random.default_rng(71)
    tru = random_truths(K, 70)
    cen, R, t = planted(tru, theta, 72, keep=1.0, noise=0.0)
    assert len(cen) == K
    lo, hi = cen[:, :2].min(0), cen[:, :2].max(0)
    spur = []
    while len(spur) < K // 5:  # a streak whose centroid, under the planted transform, is far from every truth
        p = rng.uniform(lo, hi)
        q = R @ np.array([p[0], p[1], 0.0]) + t
        if np.sqrt(((tru - q) ** 2).sum(1)).min() >= 3 * dist + 1.0:
            spur.append(p)
    pts = [c[:2] + rng.normal(0, 0.3, (200, 2)) for c in cen]
    for p in spur:
        a = rng.uniform(0, math.pi)
        along = rng.uniform(-0.5, 0.5, (200, 1)) * [math.cos(a), math.sin(a)]
        across = rng.normal(0, 0.01, (200, 1)) * [-math.sin(a), math.cos(a)]
        pts.append(p + along + across)
    Kall = K + K // 5
    xy = np.concatenate(pts)
    lab = np.repeat(np.arange(1, Kall + 1, dtype=np.int32), 200)
    perm = rng.permutation(len(lab))
    xy, lab = np.ascontiguousarray(xy[perm]), lab[perm]
    g = vcp_ctx.cluster_shapes(xy, lab, Kall)
    assert g["valid"].all() and g["rect_valid"].all()
    asp = g["rect_len"].max(1) / g["rect_len"].min(1)
    print("aspect: blobs <= %.3f, streaks >= %.3f" % (asp[:K].max(), asp[K:].min()))
    f = vcp_ctx.cluster_filter(lab, Kall, g["radius"], g["valid"], g["rect_len"], g["rect_valid"], math.inf, 3.0)
    assert f["filtered"].tolist() == [0] * K + [1] * (K // 5)
    assert f["n_kept"] == 200 * K

    def centroids(idx):
        xyz = np.c_[xy[idx], np.zeros(len(idx))]
        c3, _, cnt = vcp_ctx.centroids(xyz, None, lab[idx], Kall)
        return np.ascontiguousarray(c3[cnt > 0])

    def pose_error(M):
        return angle_diff(angle_of(M), theta), float(np.abs(M[:3, 3] - t).max())

    kept = centroids(f["kept_idx"])
    assert len(kept) == K
    r = vcp_ctx.icp_multistart(kept, tru, 36, None, 100, 200, dist)
    assert r["inliers"][r["best"]] == len(kept) == K
    full = centroids(np.arange(len(lab)))
    assert len(full) == Kall
    u = vcp_ctx.icp_multistart(full, tru, 36, None, 100, 200, dist)
    assert u["inliers"][u["best"]] <= K
    print("pose error (angle, shift): filtered %.3g %.3g, unfiltered %.3g %.3g" % (pose_error(r["M"]) + pose_error(u["M"])))
