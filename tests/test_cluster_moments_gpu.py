"""vcp_cluster_moments on the MI355X: every output of the host form and of the device-pointer form equal to the numpy
restatement of the definition (tests/cluster_moments_ref.py), doubles by their bits, on the cluster sizes around the chunk
boundaries, with weights, and on the values that are hard in kind; the geometry that motivates the call against closed forms
and exact lattice moments; the filter built on it; and the contracts every entry point keeps (independence from the
context's history, untouched outputs on every error, NULL outputs, empty calls, timing phases, the caller's stream)."""
import ctypes as C
import functools
from fractions import Fraction

import numpy as np
import pytest
import torch

import centroid_ref as CR
import cluster_moments_ref as R
import shapes_ref
from vtkcloudpoint_amd import _native as N
from vtkcloudpoint_amd import moments as M

pytestmark = pytest.mark.gpu

POISON = -7.25
U = float(R.U)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _outs(K, dim, keys=R.KEYS):
    shapes = dict(mean=(K, dim), cov=(K, R.npk(dim)), eval=(K, dim), evec=(K, dim, dim), shape=(K, 4), valid=(K,),
                  counts=(K,))
    o = {}
    for k in keys:
        if k == "valid":
            o[k] = torch.full(shapes[k], 9, dtype=torch.uint8, device="cuda")
        elif k == "counts":
            o[k] = torch.full(shapes[k], -7, dtype=torch.int64, device="cuda")
        else:
            o[k] = torch.full(shapes[k], POISON, dtype=torch.float64, device="cuda")
    return o


def _dev_call(ctx, wide, off, dim, labels, K, weights=None, keys=R.KEYS):
    """The device-pointer form on columns off .. off + dim of the [n, ld] array `wide`, read in place."""
    wide = np.ascontiguousarray(wide, np.float64)
    dw, dl = _dev(wide), _dev(np.ascontiguousarray(labels, np.int32))
    dwt = None if weights is None else _dev(np.ascontiguousarray(weights, np.int32))
    o = _outs(K, dim, keys)
    torch.cuda.synchronize()
    ctx.cluster_moments_dev(dw.data_ptr() + 8 * off, wide.shape[1], dim, dl.data_ptr(),
                            None if dwt is None else dwt.data_ptr(), len(labels), K,
                            **{"d_" + k: v.data_ptr() for k, v in o.items()})
    return {k: v.cpu().numpy() for k, v in o.items()}


def _check(ctx, pts, labels, K, weights=None, want=None, pad=0):
    """Host form and device-pointer form == the restatement, with the points as columns pad .. pad + dim of an array
    2 * pad wider.  Returns the restatement."""
    n, dim = pts.shape
    want = R.moments(pts, labels, K, weights) if want is None else want
    wide = np.full((n, dim + 2 * pad), 1e300)          # what stands beside the columns must not matter
    wide[:, pad:pad + dim] = pts
    got = ctx.cluster_moments(wide[:, pad:pad + dim], labels, K, weights)
    assert R.differs(got, want) is None, "host form, ld %d: %s" % (dim + 2 * pad, R.differs(got, want))
    got = _dev_call(ctx, wide, pad, dim, labels, K, weights)
    assert R.differs(got, want) is None, "device form, ld %d: %s" % (dim + 2 * pad, R.differs(got, want))
    return want


# ---- size classes -----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _labels():
    return CR.case_labels()


K_CASE = max(CR.SLOTS)


@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("family", CR.FAMILIES)
def test_size_classes(vcp_ctx, family, dim):
    lab = _labels()
    pts = CR.case_values(family, lab, dim)
    want = _check(vcp_ctx, pts, lab, K_CASE)                       # ld = dim
    _check(vcp_ctx, pts, lab, K_CASE, want=want, pad=1)            # ld = dim + 2: columns of a wider array
    sizes = dict(zip(CR.SLOTS, CR.SIZES))
    assert [int(c) for c in want["counts"]] == [sizes.get(k, 0) for k in range(1, K_CASE + 1)]
    assert [int(v) for v in want["valid"]] == [1 if sizes.get(k, 0) >= 2 else 0 for k in range(1, K_CASE + 1)]
    empty = want["counts"] == 0
    for k in ("mean", "cov", "eval", "evec", "shape"):
        assert np.isnan(want[k][empty]).all() and np.isfinite(want[k][~empty]).all(), k
    one = CR.SLOTS[CR.SIZES.index(1)] - 1                          # total weight 1: cov +0, the identity, not valid
    assert R.same(want["cov"][one], np.zeros(R.npk(dim))) and R.same(want["evec"][one], np.eye(dim))


def test_mean_is_vcp_centroids_without_weights(vcp_ctx):
    lab = _labels()
    for family in ("uniform", "offset"):
        xyz, motor, _ = CR.case(family)
        c3, c2, cnt = vcp_ctx.centroids(xyz, motor, lab, K_CASE)
        m3 = vcp_ctx.cluster_moments(xyz, lab, K_CASE, outputs=("mean", "counts"))
        m2 = vcp_ctx.cluster_moments(motor, lab, K_CASE, outputs=("mean", "counts"))
        assert R.same(m3["mean"], R.canon(c3)) and R.same(m2["mean"], R.canon(c2))
        assert np.array_equal(m3["counts"], cnt) and np.array_equal(m2["counts"], cnt)


# ---- weights ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [2, 3])
def test_weights(vcp_ctx, dim):
    lab = _labels()
    _, w = CR.case_weights(lab)
    w = w.copy()
    rng = np.random.default_rng(41)
    w[rng.random(len(w)) < 0.1] = 0                                  # some zeros: rows that count for nothing
    two = lab == CR.SLOTS[CR.SIZES.index(2)]
    w[two] = 0                                                       # members, but total weight 0: an empty cluster
    pts = CR.case_values("uniform", lab, dim)
    want = _check(vcp_ctx, pts, lab, K_CASE, w)
    _check(vcp_ctx, pts, lab, K_CASE, w, want=want, pad=1)
    k2 = CR.SLOTS[CR.SIZES.index(2)] - 1
    assert want["counts"][k2] == 0 and want["valid"][k2] == 0 and np.isnan(want["cov"][k2]).all()
    big = CR.SLOTS[CR.SIZES.index(257)] - 1
    assert want["counts"][big] > 200 * 2 ** 20 and want["valid"][big] == 1


def test_weights_against_duplicated_rows(vcp_ctx):
    """Row i repeated w_i times with weight 1 is the same point set: the same counts, and a covariance within the sum of
    the two derived bounds of the weighted one (both lie within their bound of the one exact covariance).  Not the same
    bits: the duplicated rows fill the tree differently."""
    rng = np.random.default_rng(43)
    n, K = 4000, 6
    lab = rng.integers(0, K + 1, n).astype(np.int32)
    w = rng.integers(0, 6, n).astype(np.int32)
    pts = 1e4 + rng.uniform(-3, 3, (n, 3))
    rep = np.repeat(np.arange(n), w)
    got_w = vcp_ctx.cluster_moments(pts, lab, K, w)
    got_d = vcp_ctx.cluster_moments(pts[rep], lab[rep], K)
    assert R.differs(got_w, R.moments(pts, lab, K, w)) is None and R.differs(got_d, R.moments(pts[rep], lab[rep], K)) is None
    assert np.array_equal(got_w["counts"], got_d["counts"]) and (got_w["counts"] > 1000).all()
    ex = R.exact_cov(pts, lab, K, w)
    bw, bd = R.cov_bound(pts, lab, K, w, ex=ex), R.cov_bound(pts[rep], lab[rep], K)
    pairs = [(a, b) for a in range(3) for b in range(a, 3)]
    for k in range(K):
        for j, ab in enumerate(pairs):
            diff = abs(Fraction(float(got_w["cov"][k, j])) - Fraction(float(got_d["cov"][k, j])))
            assert diff <= bw[k][ab] + bd[k][ab], (k, ab, float(diff), float(bw[k][ab] + bd[k][ab]))
    assert not R.same(got_w["cov"], got_d["cov"])


# ---- hard values ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [2, 3])
def test_hard_values(vcp_ctx, dim):
    """Every kind case of centroid_ref as a cluster of its own, with ordinary clusters and the small exact shapes in the
    same call: the restatement's bits everywhere, valid == 0 exactly where a moment is not finite."""
    rng = np.random.default_rng(47)
    cols, lab, names = [], [], []
    for name, col in CR.kind_cases().items():
        names.append(name)
        cols.append(np.repeat(col[:, None], dim, 1))
        lab.append(np.full(len(col), len(names)))
    extra = {
        "ordinary_a": rng.uniform(-5, 5, (300, dim)),
        "one_point": np.full((1, dim), 3.25),
        "two_equal_points": np.full((2, dim), -1.5),
        "collinear": np.stack([np.arange(9) * 0.25 + 7.0] + [np.arange(9) * 0.5 - 2.0] * (dim - 1), axis=1),
        "rectangle": np.stack(np.meshgrid(np.arange(4) * 0.5 + 10.0, np.arange(8) * 0.5 - 3.0, *([np.zeros(1)] * (dim - 2)),
                                          indexing="ij"), axis=-1).reshape(-1, dim),
        "ordinary_b": rng.normal(0, 2, (500, dim)) + 1e3,
    }
    for name, p in extra.items():
        names.append(name)
        cols.append(p)
        lab.append(np.full(len(p), len(names)))
    pts, lab = np.concatenate(cols), np.concatenate(lab).astype(np.int32)
    slots = rng.permutation(len(lab))
    P, L = np.zeros_like(pts), np.zeros(len(lab), np.int32)
    for k in range(1, len(names) + 1):                     # label k's members, in their own order, at scattered rows:
        rows = np.sort(slots[lab == k])                    # the kind cases depend on the order of the members
        P[rows], L[rows] = pts[lab == k], k
    K = len(names)
    with np.errstate(all="ignore"):
        want = _check(vcp_ctx, P, L, K)
    at = {nm: j for j, nm in enumerate(names)}
    finite = np.isfinite(want["mean"]).all(1) & np.isfinite(want["cov"]).all(1)
    assert np.array_equal(want["valid"], (finite & (want["counts"] >= 2)).astype(np.uint8))
    for nm in ("overflow_tree_only", "inf_member", "inf_both_signs", "nan_member"):
        assert want["valid"][at[nm]] == 0 and np.isnan(want["eval"][at[nm]]).all(), nm
    for nm in ("negative_zero", "subnormal", "ordinary_a", "ordinary_b", "two_equal_points", "collinear", "rectangle"):
        assert want["valid"][at[nm]] == 1, nm
    assert want["valid"][at["one_point"]] == 0 and R.same(want["cov"][at["one_point"]], np.zeros(R.npk(dim)))
    assert R.same(want["eval"][at["two_equal_points"]], np.zeros(dim))
    # the ordinary clusters are what they are alone
    for nm in ("ordinary_a", "ordinary_b"):
        alone = vcp_ctx.cluster_moments(extra[nm], np.ones(len(extra[nm]), np.int32), 1)
        for key in R.KEYS:
            assert R.same(np.asarray(alone[key][0]), np.asarray(want[key][at[nm]])), (nm, key)
        assert alone["valid"][0] == 1 and alone["counts"][0] == len(extra[nm])
    # collinear lattice points: the covariance is exact and of rank one; what the solve leaves beside the one eigenvalue is
    # within its residual (8 u |S|, twice the worst test_cluster_moments.py measures), of either sign, reported as computed
    c = at["collinear"]
    assert want["eval"][c, 0] > 0 and np.abs(want["eval"][c, 1:]).max() <= 8 * U * want["eval"][c, 0]
    assert want["shape"][c, 1] <= (8 * U * want["eval"][c, 0]) ** 0.5
    # an axis-aligned lattice rectangle, longer in y: cov exactly diagonal, the axes a permutation of the identity
    r = at["rectangle"]
    cov = R.unpack(want["cov"][r])
    assert np.count_nonzero(cov - np.diag(np.diag(cov))) == 0 and cov[1, 1] > cov[0, 0] > 0
    assert want["eval"][r].tolist() == sorted(np.diag(cov).tolist(), reverse=True)
    ev = want["evec"][r]
    assert set(np.abs(ev).ravel()) == {0.0, 1.0} and ev[0, 1] == 1.0 and ev[1, 0] == 1.0
    assert R.same(want["eval"][r, :2], np.array([5.25, 1.25]) * 0.25)      # (n^2 - 1) / 12 of the pitch squared


# ---- the geometry that motivates it -------------------------------------------------------------------------------------------
def _tol(bound_k, Cx, dim):
    """How far an eigenvalue of the computed covariance can lie from the exact one's: |cov - C|_F by the derived bound,
    plus 8 u |C|_F for the solve (twice the worst residual test_cluster_moments.py measures)."""
    fro = lambda d: float(sum((1 if a == b else 2) * d[(a, b)] ** 2 for a in range(dim) for b in range(a, dim))) ** 0.5
    return fro(bound_k) + 8 * U * fro(Cx)


def _one(vcp_ctx, pts):
    """The moments of one cluster, held to the restatement, with its exact covariance and the eigenvalue tolerance."""
    lab = np.ones(len(pts), np.int32)
    got = vcp_ctx.cluster_moments(pts, lab, 1)
    assert R.differs(got, R.moments(pts, lab, 1)) is None
    ex = R.exact_cov(pts, lab, 1)
    dim = pts.shape[1]
    return M.ClusterMoments(dim, 1, **got), ex[0][2], _tol(R.cov_bound(pts, lab, 1, ex=ex)[0], ex[0][2], dim)


def test_disc_ellipse_and_one_outlier(vcp_ctx):
    step, r = 0.125, 3.15
    centre = np.array([100.25, -37.5])
    disc = R.lattice_disc(r, step) + centre
    assert 1900 < len(disc) < 2100
    mom, Cx, tol = _one(vcp_ctx, disc)
    lam = R.exact_eig(Cx, 2)
    assert Cx[(0, 1)] == 0 and Cx[(0, 0)] == Cx[(1, 1)]              # the lattice disc's own symmetry, exactly
    lattice_r = 2 * lam[0] ** 0.5                                    # the lattice's own 2 sigma
    disc_err = abs(lattice_r - r)                                    # the discretisation error: from exact moments
    assert disc_err < step                                           # the rim is known to one pitch
    slack = tol / lam[0] ** 0.5 + 4 * U * r                          # d(2 sqrt(l)) = dl / sqrt(l); the sqrt and the product
    er = float(M.ellipse_radius(mom)[0])
    assert abs(er - lattice_r) <= slack and abs(er - r) <= disc_err + slack
    print("\ndisc: r %.4f, lattice 2 sigma %.6f, computed %.6f (discretisation %.2e, slack %.2e)" % (r, lattice_r, er, disc_err, slack))
    # a filled a x b ellipse turned by 30 degrees
    a, b = 4.0, 1.5
    ell = R.lattice_ellipse(a, b, step, 30.0) + centre
    mom_e, Ce, tol_e = _one(vcp_ctx, ell)
    le = R.exact_eig(Ce, 2)
    lattice_aspect = (le[0] / le[1]) ** 0.5
    asp_err = abs(lattice_aspect - a / b)
    assert asp_err <= (a / b) * (step / a + step / b)                # each semi-axis known to one pitch
    sides = M.ellipse_sides(mom_e)[0]
    aspect = float(sides[0] / sides[1])
    slack_e = lattice_aspect * 0.5 * (tol_e / le[0] + tol_e / le[1]) + 8 * U * lattice_aspect
    assert abs(aspect - lattice_aspect) <= slack_e and abs(aspect - a / b) <= asp_err + slack_e
    axis = mom_e.evec[0, 0]
    assert abs(abs(axis[0] * np.cos(np.radians(30)) + axis[1] * np.sin(np.radians(30))) - 1.0) < 1e-3   # along the long axis
    # one stray return at 10 r: the circle follows it, the ellipse moves by what the exact moments say
    out = np.concatenate([disc, centre[None] + [10 * r, 0.0]])
    lab = np.ones(len(out), np.int32)
    sh = vcp_ctx.cluster_shapes(out, lab, 1, hull=False)
    assert sh["radius"][0] >= 5 * r
    mom_o, Co, tol_o = _one(vcp_ctx, out)
    lo = R.exact_eig(Co, 2)
    predicted = 2 * lo[0] ** 0.5
    got = float(M.ellipse_radius(mom_o)[0])
    assert abs(got - predicted) <= tol_o / lo[0] ** 0.5 + 4 * U * predicted
    assert predicted < 1.2 * r                                       # 1 / count of the distance, not all of it
    print("outlier at 10 r: circle radius %.3f r, ellipse radius %.4f r (exact moments: %.4f r)"
          % (sh["radius"][0] / r, got / r, predicted / r))


def test_planarity(vcp_ctx):
    """A lattice patch on the plane z = x / 2 + y / 4 (every coordinate a multiple of 1 / 32: exactly planar), and the same
    patch thickened to a lattice box."""
    g = np.arange(24) * 0.125
    x, y = (v.ravel() for v in np.meshgrid(g, g[:16], indexing="ij"))
    patch = np.stack([x + 50.0, y - 20.0, 0.5 * x + 0.25 * y + 8.0], axis=1)
    normal = np.array([-0.5, -0.25, 1.0]) / np.sqrt(0.25 + 0.0625 + 1.0)
    mom, Cx, tol = _one(vcp_ctx, patch)
    lam = R.exact_eig(Cx, 3)
    trace = float(sum(Cx[(a, a)] for a in range(3)))
    assert abs(lam[2]) <= 1e-25 * trace                              # the exact smallest eigenvalue is 0 (60-digit solve)
    assert abs(float(mom.flatness[0])) <= tol / (trace - tol)        # flatness at rounding level
    nrm = mom.normal[0]
    assert np.linalg.norm(np.cross(nrm, normal)) <= 2 * tol / (lam[1] - lam[2]) + 8 * U   # parallel, to the solver's residual
    assert abs(float(mom.tilt[0]) - normal[2]) <= 2 * tol / (lam[1] - lam[2]) + 8 * U
    box = np.concatenate([patch + [0.0, 0.0, j * 0.125] for j in range(4)])
    mom_b, Cb, tol_b = _one(vcp_ctx, box)
    lb = R.exact_eig(Cb, 3)
    exact_flat = lb[2] / sum(lb)
    assert exact_flat > 1e-3 > abs(float(mom.flatness[0]))
    assert abs(float(mom_b.flatness[0]) - exact_flat) <= 2 * tol_b / (sum(lb) - 3 * tol_b) + 4 * U
    print("\npatch: flatness %.3g, tilt %.6f; box: flatness %.6f (exact %.6f)"
          % (mom.flatness[0], mom.tilt[0], mom_b.flatness[0], exact_flat))


# ---- the pipeline ------------------------------------------------------------------------------------------------------------
def _blobs():
    rng = np.random.default_rng(53)
    parts = [np.round(rng.normal(0, 0.4, (400, 3)) * 64) / 64 + c for c in ([0, 0, 5.0], [6, 1, 5.0], [2, 7, 5.0])]
    rail = np.round(np.stack([rng.uniform(-4, 4, 500), rng.normal(0, 0.1, 500), rng.normal(0, 0.1, 500)], 1) * 64) / 64
    parts.append(rail + [12.0, 12.0, 5.0])                                          # the elongated false cluster
    parts.append(np.round(rng.normal(0, 0.4, (400, 3)) * 64) / 64 + [20.0, 0, 5.0])  # a ball: not flat
    parts[4][:, 2] *= 3.0
    parts[:3] = [p * [1, 1, 0.02] + [0, 0, 4.9] for p in parts[:3]]                  # the targets are flat patches facing z
    pts = np.concatenate(parts + [rng.uniform(-5, 25, (200, 3))])
    lab = np.concatenate([np.full(len(p), k + 1) for k, p in enumerate(parts)] + [np.zeros(200)]).astype(np.int32)
    p = rng.permutation(len(lab))
    return np.ascontiguousarray(pts[p]), lab[p], 5


def test_pipeline_filter(vcp_ctx):
    pts, lab, K = _blobs()
    d_pts, d_lab = _dev(pts), _dev(lab)
    # 2-D, device tensors: the (X, Y) columns of the resident xyz, read in place
    mom = M.cluster_moments(d_pts[:, :2], d_lab, K, ctx=vcp_ctx)
    assert mom.mean.is_cuda and R.differs({k: getattr(mom, k).cpu().numpy() for k in R.KEYS}, R.moments(pts[:, :2], lab, K)) is None
    rad, sides, valid = (t.cpu().numpy() for t in (M.ellipse_radius(mom), M.ellipse_sides(mom), mom.valid))
    max_r, max_a = 2.0, 3.0
    restated = (valid == 1) & ((rad > max_r) | (sides[:, 0] > max_a * sides[:, 1]))
    assert restated.tolist() == [False, False, False, True, False]
    full = M.filter_by_moments(d_lab, mom, max_r, max_a, ctx=vcp_ctx, full=True)
    assert M.filter_by_moments(d_lab, mom, max_r, max_a, ctx=vcp_ctx) == [4]
    same_arrays = vcp_ctx.cluster_filter(lab, K, rad, valid, sides, valid, max_r, max_a)
    ref = shapes_ref.cluster_filter(lab, K, rad, valid, sides, valid, max_r, max_a)
    for r in (same_arrays, ref):
        assert np.array_equal(full["filtered"].cpu().numpy(), r["filtered"]) and full["n_kept"] == r["n_kept"]
        assert np.array_equal(full["keep"].cpu().numpy(), r["keep"]) and np.array_equal(full["kept_idx"].cpu().numpy(), r["kept_idx"])
    # 3-D, numpy: flatness and tilt beside radius and aspect; NaN and inf switch a criterion off
    mom3 = M.cluster_moments(pts, lab, K, ctx=vcp_ctx)
    assert R.differs({k: getattr(mom3, k) for k in R.KEYS}, R.moments(pts, lab, K)) is None
    flat = (mom3.valid == 1) & (mom3.flatness > 0.05)
    assert flat.tolist() == [False, False, False, False, True]
    assert M.filter_by_moments(lab, mom3, max_flatness=0.05, ctx=vcp_ctx) == [5]
    assert M.filter_by_moments(lab, mom3, max_r, max_a, max_flatness=0.05, ctx=vcp_ctx) == [4, 5]
    assert M.filter_by_moments(lab, mom3, min_tilt=0.9, ctx=vcp_ctx) == [j + 1 for j in range(K) if mom3.tilt[j] < 0.9]
    assert 5 in M.filter_by_moments(lab, mom3, min_tilt=0.9, ctx=vcp_ctx) and mom3.tilt[:3].min() > 0.99
    assert M.filter_by_moments(lab, mom3, np.nan, np.inf, np.nan, 0.0, ctx=vcp_ctx) == []
    f = M.filter_by_moments(lab, mom3, max_r, max_a, max_flatness=0.05, ctx=vcp_ctx, full=True)
    hit = np.isin(lab, [4, 5])
    assert np.array_equal(f["keep"], (~hit).astype(np.uint8)) and np.array_equal(f["kept_idx"], np.flatnonzero(~hit))
    # tools.getEllipses: the same numbers through the reference's class surface
    from vtkcloudpoint_amd import tools
    from vtkcloudpoint_amd.datamodel import ClusObj, Point3D
    clus = []
    for k in range(1, K + 1):
        ob = ClusObj()
        ob.li = [Point3D(*p) for p in pts[lab == k]]
        clus.append(ob)
    ells = tools.getEllipses(clus, True, ctx=vcp_ctx)
    assert [e.clusID for e in ells] == [1, 2, 3, 4, 5] and max(ells, key=lambda e: e.a / e.b).clusID == 4


def test_a_hull_beyond_2048_points_gets_moments_and_a_verdict(vcp_ctx):
    th = np.arange(2049) * (2 * np.pi / 2049)
    ring = np.round(np.c_[np.cos(th), np.sin(th)] * 2.0 ** 30) / 2.0 ** 30      # a lattice-approximated circle: all hull
    lab = np.ones(len(ring), np.int32)
    with pytest.raises(N.VcpError) as e:
        vcp_ctx.cluster_shapes(ring, lab, 1)
    assert e.value.code == -5
    mom = M.cluster_moments(ring, lab, 1, ctx=vcp_ctx)
    assert R.differs({k: getattr(mom, k) for k in R.KEYS}, R.moments(ring, lab, 1)) is None
    assert mom.valid[0] == 1 and mom.counts[0] == 2049
    assert abs(M.ellipse_radius(mom)[0] - 2 ** 0.5) < 1e-6                        # a ring of radius 1: variance 1 / 2 per axis
    assert M.filter_by_moments(lab, mom, max_radius=1.0, ctx=vcp_ctx) == [1]
    assert M.filter_by_moments(lab, mom, max_radius=2.0, max_aspect=1.5, ctx=vcp_ctx) == []


# ---- contracts -----------------------------------------------------------------------------------------------------------------
def _small(seed, n, K, dim=3):
    rng = np.random.default_rng(seed)
    return rng.uniform(-9, 9, (n, dim)), rng.integers(0, K + 1, n).astype(np.int32), rng.integers(0, 4, n).astype(np.int32)


def test_independent_of_the_contexts_history_and_run_to_run(vcp_ctx):
    pts, lab, w = _small(61, 40000, 9)
    first = _dev_call(vcp_ctx, pts, 0, 3, lab, 9, w)
    assert R.differs(first, R.moments(pts, lab, 9, w)) is None
    again = _dev_call(vcp_ctx, pts, 0, 3, lab, 9, w)
    assert all(R.same(first[k], again[k]) for k in R.KEYS)                         # run to run
    big = _small(62, 200000, 300)
    _dev_call(vcp_ctx, big[0], 0, 3, big[1], 300, big[2])                         # a larger call in between
    assert all(R.same(first[k], _dev_call(vcp_ctx, pts, 0, 3, lab, 9, w)[k]) for k in R.KEYS)
    tiny = _small(63, 50, 2, 2)
    _dev_call(vcp_ctx, tiny[0], 0, 2, tiny[1], 2)                                 # a smaller one, another dim, no weights
    assert all(R.same(first[k], _dev_call(vcp_ctx, pts, 0, 3, lab, 9, w)[k]) for k in R.KEYS)
    vcp_ctx.release_workspace()
    assert all(R.same(first[k], _dev_call(vcp_ctx, pts, 0, 3, lab, 9, w)[k]) for k in R.KEYS)
    host = vcp_ctx.cluster_moments(pts, lab, 9, w)
    assert all(R.same(first[k], host[k]) for k in R.KEYS)


def _raw(ctx, dev, pts, ld, dim, lab, w, n, K, outs):
    f = N.lib().vcp_cluster_moments_dev if dev else N.lib().vcp_cluster_moments
    p = (lambda a: None if a is None else C.c_void_p(a.data_ptr())) if dev else (lambda a: None if a is None else C.c_void_p(a.ctypes.data))
    return f(ctx._h, p(pts), C.c_int64(ld), C.c_int(dim), p(lab), p(w), C.c_int64(n), C.c_int32(K),
             *(p(outs.get(k)) for k in R.KEYS))


def test_errors_leave_the_outputs_untouched(vcp_ctx):
    pts, lab, w = _small(64, 500, 4)
    bad_lab, neg_lab, bad_w = lab.copy(), lab.copy(), w.copy()
    bad_lab[77], neg_lab[3], bad_w[123] = 5, -1, -1
    cases = [("label above K", dict(lab=bad_lab), -4), ("negative label", dict(lab=neg_lab), -4),
             ("negative weight", dict(w=bad_w), -1), ("dim 1", dict(dim=1), -1), ("dim 4", dict(dim=4, ld=4), -1),
             ("ld below dim", dict(ld=2), -1), ("n negative", dict(n=-1), -1), ("K negative", dict(K=-1), -1),
             ("n beyond 32-bit indexing", dict(n=0x7FFFFFF0), -5)]
    for dev in (False, True):
        for name, ch, code in cases:
            a = dict(lab=lab, w=w, dim=3, ld=3, n=len(lab), K=4)
            a.update(ch)
            if dev:
                outs = _outs(4, 3)
                args = (_dev(pts), a["ld"], a["dim"], _dev(a["lab"]), _dev(a["w"]))
                torch.cuda.synchronize()
            else:
                outs = {k: v.cpu().numpy() for k, v in _outs(4, 3).items()}
                args = (pts, a["ld"], a["dim"], a["lab"], a["w"])
            poison = {k: (v.clone() if dev else v.copy()) for k, v in outs.items()}
            rc = _raw(vcp_ctx, dev, *args, a["n"], a["K"], outs)
            assert rc == code, (dev, name, rc)
            for k in R.KEYS:
                got, was = (outs[k].cpu().numpy(), poison[k].cpu().numpy()) if dev else (outs[k], poison[k])
                assert R.same(got, was), (dev, name, k)
    assert N.lib().vcp_cluster_moments(None, None, C.c_int64(3), C.c_int(3), None, None, C.c_int64(0), C.c_int32(0),
                                       None, None, None, None, None, None, None) == -1     # NULL ctx
    assert R.differs(vcp_ctx.cluster_moments(pts, lab, 4, w), R.moments(pts, lab, 4, w)) is None   # and the context works on


def test_null_outputs_and_empty_calls(vcp_ctx):
    pts, lab, w = _small(65, 3000, 6)
    want = R.moments(pts, lab, 6, w)
    for keys in (("cov",), ("valid",), ("counts", "mean"), ("eval", "evec"), ("shape",), ()):
        got = vcp_ctx.cluster_moments(pts, lab, 6, w, outputs=keys)
        assert set(got) == set(keys) and R.differs(got, want, keys) is None
        got = _dev_call(vcp_ctx, pts, 0, 3, lab, 6, w, keys)
        assert R.differs(got, want, keys) is None
    # n == 0: every cluster is empty; K == 0: nothing to write
    for dim in (2, 3):
        e = vcp_ctx.cluster_moments(np.zeros((0, dim)), np.zeros(0, np.int32), 3)
        assert R.differs(e, R.moments(np.zeros((0, dim)), np.zeros(0, np.int32), 3)) is None
        assert (e["counts"] == 0).all() and (e["valid"] == 0).all() and np.isnan(e["shape"]).all()
        z = vcp_ctx.cluster_moments(np.ones((5, dim)), np.zeros(5, np.int32), 0)
        assert all(len(v) == 0 for v in z.values())
        assert _dev_call(vcp_ctx, np.zeros((1, dim)), 0, dim, np.zeros(0, np.int32), 2)["counts"].tolist() == [0, 0]
    with pytest.raises(N.VcpError) as err:                                           # K == 0 still checks the labels
        vcp_ctx.cluster_moments(np.ones((5, 3)), np.ones(5, np.int32), 0)
    assert err.value.code == -4


def test_timing_phases(vcp_ctx):
    pts, lab, w = _small(66, 20000, 8)
    vcp_ctx.timing_enable(True)
    try:
        _dev_call(vcp_ctx, pts, 0, 3, lab, 8, w)
        phases = vcp_ctx.timing()
    finally:
        vcp_ctx.timing_enable(False)
    assert [nm for nm, _ in phases] == ["moments_group", "moments_mean", "moments_cov"]
    assert all(ms >= 0.0 for _, ms in phases)


def test_on_the_callers_stream():
    """vcp_set_stream holds for vcp_cluster_moments_dev, by the method of test_stream_gpu.py (its rig, imported): the
    input is swapped behind a running filler on the caller's stream, so a launch on any other stream reads cloud A."""
    from test_stream_gpu import Rig
    rig = Rig()
    try:
        n, K = 30000, 7
        A, lab, w = _small(67, n, K)
        B = _small(68, n, K)[0]
        wa, wb = R.moments(A, lab, K, w), R.moments(B, lab, K, w)
        assert not R.same(wa["cov"], wb["cov"])
        buf, dB, dl, dw = _dev(A), _dev(B), _dev(lab), _dev(w)
        o = _outs(K, 3)
        rig.run(lambda: rig.ctx.cluster_moments_dev(buf.data_ptr(), 3, 3, dl.data_ptr(), dw.data_ptr(), n, K,
                                                    **{"d_" + k: v.data_ptr() for k, v in o.items()}),
                [(buf, dB)], [(v, 9 if v.dtype == torch.uint8 else -7) for v in o.values()])
        assert R.differs({k: v.cpu().numpy() for k, v in o.items()}, wb) is None
    finally:
        rig.close()
