"""vcp_icp_multistart on the MI355X: the vcp_icp_vtklike loop from many start rotations in one call, scored by inliers.
Both nearest-neighbour paths of the target run: nt <= 512 (scalar-cache scan) and nt > 512 (grid)."""
import ctypes as C
import math

import numpy as np
import pytest

from vtkcloudpoint_amd import _native as N
from vtkcloudpoint_amd.icp import multistart_icp, rotations_about_z

from icpms_data import angle_diff, angle_of, l_lattice, planted, random_truths

pytestmark = pytest.mark.gpu

SIZES = [(300, 11), (3000, 12)]  # (truths, seed): scalar-cache path, grid path


def _same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b))


def _case(n, seed, deg=20.0, noise=0.05):
    tru = random_truths(n, seed)
    cen, _, _ = planted(tru, math.radians(deg), seed + 1, noise=noise)
    return cen, tru


@pytest.mark.parametrize("n,seed", SIZES)
@pytest.mark.parametrize("ml", [200, 100000])
def test_single_pose_equals_vtklike(vcp_ctx, n, seed, ml):
    cen, tru = _case(n, seed)
    r = vcp_ctx.icp_multistart(cen, tru, 1, None, 100, ml, 1.0)
    v = vcp_ctx.icp_vtklike(cen, tru, 100, ml, True)
    assert r["best"] == 0
    assert _same(r["M"], v["M"]) and _same(r["M_all"][0], v["M"])
    assert _same(r["mean_dist"][0], v["mean_dist"])
    # identity start without the centroid translation = start_by_matching_centroids off
    r0 = vcp_ctx.icp_multistart(cen, tru, np.eye(3)[None], np.zeros((1, 3)), 100, ml, 1.0)
    v0 = vcp_ctx.icp_vtklike(cen, tru, 100, ml, False)
    assert _same(r0["M"], v0["M"]) and _same(r0["mean_dist"][0], v0["mean_dist"])
    # the generated pose 0 is exactly the identity: a 36-pose call's pose 0 is the single start too
    r36 = vcp_ctx.icp_multistart(cen, tru, 36, None, 100, ml, 1.0)
    assert _same(r36["M_all"][0], v["M"]) and _same(r36["mean_dist"][0], v["mean_dist"])


@pytest.mark.parametrize("n,seed", SIZES)
def test_batch_independence(vcp_ctx, n, seed):
    cen, tru = _case(n, seed, deg=140.0)
    rng = np.random.default_rng(seed)
    Rs = rotations_about_z(18, mirror=True)
    Ts = rng.normal(0.0, 20.0, (36, 3))
    Ts[:, 2] = 0.0
    for init_T in (None, Ts):
        r = vcp_ctx.icp_multistart(cen, tru, Rs, init_T, 60, 200, 1.0)
        for h in (0, 5, 17, 18, 29, 35):
            one = vcp_ctx.icp_multistart(cen, tru, Rs[h:h + 1], None if init_T is None else init_T[h:h + 1], 60, 200,
                                         1.0)
            assert _same(one["M_all"][0], r["M_all"][h]), h
            assert _same(one["mean_dist"][0], r["mean_dist"][h]) and one["inliers"][0] == r["inliers"][h], h


def _host_loop(oracle, src, tgt, R, T, max_iter, ml):
    """The vcp_icp_vtklike loop restated with the oracle: landmarks, closest target point, sums, Horn, R <- R1 R,
    T <- R1 T + T1."""
    ns = len(src)
    step = ns // ml if ns > ml else 1
    lm = src[::step][: ns // step]
    for _ in range(max_iter):
        P = oracle.trans_point(lm, R, T)
        s = oracle.icp_sums(tgt, P)
        R1, T1 = oracle.horn_from_sums(s, len(lm))
        R, T = R1 @ R, R1 @ T + T1
    return R, T, np.sqrt(s[15] / len(lm)), lm


@pytest.mark.parametrize("nt,seed", [(150, 31), (700, 32)])
def test_restated_on_the_host(vcp_ctx, oracle, nt, seed):
    tru = random_truths(nt, seed)
    cen, _, _ = planted(tru, math.radians(75.0), seed, keep=0.6, noise=0.1)
    Rs = rotations_about_z(8)
    r = vcp_ctx.icp_multistart(cen, tru, Rs, None, 30, 50, 1.0)
    ms, mt = cen.mean(axis=0), tru.mean(axis=0)
    for h in (0, 3, 6):
        R, T, md, lm = _host_loop(oracle, cen, tru, Rs[h], mt - Rs[h] @ ms, 30, 50)
        Mg = r["M_all"][h]
        assert np.abs(Mg[:3, :3] - R).max() < 1e-9 and np.abs(Mg[:3, 3] - T).max() < 1e-9, h
        assert abs(r["mean_dist"][h] - md) < 1e-9
        _, nn = vcp_ctx.icp_sums(tru, lm, Mg[:3, :3], Mg[:3, 3])
        assert _same(nn, oracle.find_closest(tru, oracle.trans_point(lm, R, T))), h


@pytest.mark.parametrize("n,seed,noise,dist", [(300, 11, 0.05, 2.0), (3000, 12, 0.02, 1.0)])
def test_planted_rotation(vcp_ctx, n, seed, noise, dist):
    tru = random_truths(n, seed)
    for deg in (100, 180, 263):
        th = math.radians(deg)
        cen, R, t = planted(tru, th, seed + deg, noise=noise)
        if deg == 180:  # the case is hard: the centroid start alone ends in a local minimum
            v = vcp_ctx.icp_vtklike(cen, tru, 100, 200, True)
            assert angle_diff(angle_of(v["M"]), th) > 0.1
            assert vcp_ctx.match(cen, tru, v["M"], dist)["count"] < 0.5 * len(cen)
        r = vcp_ctx.icp_multistart(cen, tru, 36, None, 100, 200, dist)
        M = r["M"]
        assert _same(M, r["M_all"][r["best"]])
        assert angle_diff(angle_of(M), th) < 1e-3, deg
        assert np.abs(M[:3, 3] - t).max() < 0.05
        assert r["inliers"][r["best"]] >= 0.9 * len(cen)
        if deg == 100:  # every pose's score is vcp_match's count under its matrix
            for h in range(36):
                assert r["inliers"][h] == vcp_ctx.match(cen, tru, r["M_all"][h], dist)["count"], h


@pytest.mark.parametrize("nx,ny,deg", [(16, 12, 143), (30, 30, 200)])
def test_checkerboard(vcp_ctx, nx, ny, deg):
    """The reference README's case: truths on a lattice (inside an L, so that one pose fits), centroids a rotated,
    slightly noisy subset.  The single start stops a lattice step or a turn away; one of 36 starts finds the pose."""
    tru = l_lattice(nx, ny)
    th = math.radians(deg)
    cen, R, t = planted(tru, th, 7 + deg, keep=0.9, noise=0.05)
    v = vcp_ctx.icp_vtklike(cen, tru, 100, 200, True)
    assert vcp_ctx.match(cen, tru, v["M"], 2.0)["count"] < len(cen)
    r = multistart_icp(cen, tru, 36, inlier_dist=2.0, ctx=vcp_ctx)
    assert r["inliers"][r["best"]] == len(cen)
    assert angle_diff(angle_of(r["M"]), th) < 1e-3 and np.abs(r["M"][:3, 3] - t).max() < 0.05
    assert vcp_ctx.match(cen, tru, r["M"], 2.0)["count"] == len(cen)


@pytest.mark.parametrize("n,seed", [(300, 21), (3000, 22)])
def test_mirror(vcp_ctx, n, seed):
    tru = random_truths(n, seed)
    th = math.radians(130.0)
    cen, R, t = planted(tru, th, seed, noise=0.02, mirror=True)
    r = multistart_icp(cen, tru, 36, mirror=True, inlier_dist=1.0, ctx=vcp_ctx)
    assert len(r["inliers"]) == 72 and r["best"] >= 36
    assert np.linalg.det(r["M"][:3, :3]) == pytest.approx(-1.0, abs=1e-9)
    assert r["inliers"][r["best"]] == len(cen)
    assert np.abs(r["M"][:3, :3] - R).max() < 1e-3
    # without the mirrored starts no pose fits (Horn's rotations are proper)
    p = multistart_icp(cen, tru, 36, inlier_dist=1.0, ctx=vcp_ctx)
    assert p["inliers"].max() < 0.5 * len(cen)
    assert np.allclose(np.linalg.det(p["M_all"][:, :3, :3]), 1.0, atol=1e-9)


@pytest.mark.parametrize("n,seed", SIZES)
def test_deterministic(vcp_ctx, n, seed):
    cen, tru = _case(n, seed, deg=250.0)
    a = vcp_ctx.icp_multistart(cen, tru, 360, None, 100, 200, 1.0)
    b = vcp_ctx.icp_multistart(cen, tru, 360, None, 100, 200, 1.0)
    for k in ("M", "M_all", "mean_dist", "inliers"):
        assert _same(a[k], b[k]), k
    assert a["best"] == b["best"]


def test_4096_poses(vcp_ctx):
    tru = random_truths(80, 41)
    cen, _, _ = planted(tru, math.radians(300.0), 42, keep=0.75, noise=0.05)
    a = vcp_ctx.icp_multistart(cen, tru, 4096, None, 20, 200, 5.0)
    b = vcp_ctx.icp_multistart(cen, tru, 4096, None, 20, 200, 5.0)
    for k in ("M", "M_all", "mean_dist", "inliers"):
        assert _same(a[k], b[k]), k
    assert a["best"] == b["best"] and a["M_all"].shape == (4096, 4, 4)
    Rs = rotations_about_z(4096)
    c = vcp_ctx.icp_multistart(cen, tru, Rs, None, 20, 200, 5.0)
    for h in (0, 1, 1000, 2047, 4095):
        one = vcp_ctx.icp_multistart(cen, tru, Rs[h:h + 1], None, 20, 200, 5.0)
        assert _same(one["M_all"][0], c["M_all"][h]) and _same(one["mean_dist"][0], c["mean_dist"][h]), h


def test_best_rule_and_null_outputs(vcp_ctx):
    cen, tru = _case(300, 11, deg=180.0)
    r = vcp_ctx.icp_multistart(cen, tru, 36, None, 100, 200, 2.0)
    inl, md = r["inliers"], r["mean_dist"]
    top = np.flatnonzero(inl == inl.max())
    want = top[np.lexsort((top, md[top]))[0]]
    assert r["best"] == want
    # the required outputs only
    M = np.zeros(16)
    best = C.c_int32(-1)
    src, tgt = np.ascontiguousarray(cen), np.ascontiguousarray(tru)
    rc = N.lib().vcp_icp_multistart(vcp_ctx._h, N._ptr(src), C.c_int64(len(src)), N._ptr(tgt), C.c_int64(len(tgt)),
                                    C.c_int32(36), None, None, 100, 200, C.c_double(2.0), N._ptr(M), C.byref(best),
                                    None, None, None)
    assert rc == 0 and best.value == r["best"] and _same(M.reshape(4, 4), r["M"])
    # inlier_dist = +inf: every finite point counts
    f = vcp_ctx.icp_multistart(cen, tru, 4, None, 10, 200)
    assert (f["inliers"] == len(cen)).all()


def test_errors(vcp_ctx):
    cen, tru = _case(300, 11)
    z = np.zeros((0, 3))

    def code(*a, **k):
        with pytest.raises(N.VcpError) as e:
            vcp_ctx.icp_multistart(*a, **k)
        return e.value.code

    assert code(z, tru) == -2 and code(cen, z) == -2
    assert code(cen, tru, 0) == -1 and code(cen, tru, -3) == -1
    assert code(cen, tru, 4097) == -8
    assert code(cen, tru, 4, max_iter=0) == -1 and code(cen, tru, 4, max_landmarks=0) == -1
    for d in (0.0, -1.0, np.nan, -np.inf):
        assert code(cen, tru, 4, inlier_dist=d) == -1
    Rs = rotations_about_z(4)
    for bad in (np.nan, np.inf):
        R = Rs.copy()
        R[2, 1, 1] = bad
        assert code(cen, tru, R) == -1
        T = np.zeros((4, 3))
        T[3, 0] = bad
        assert code(cen, tru, Rs, T) == -1
    # a failed Horn solve (non-finite sums) in one pose fails the call
    Tn = np.zeros((4, 3))
    Tn[1, 0] = 1e308  # pose 1: the sum of the moved landmarks overflows
    assert code(cen, tru, Rs, Tn) == -1
    # required outputs
    M = np.zeros(16)
    best = C.c_int32(0)
    src, tgt = np.ascontiguousarray(cen), np.ascontiguousarray(tru)
    rc = N.lib().vcp_icp_multistart(vcp_ctx._h, N._ptr(src), C.c_int64(len(src)), N._ptr(tgt), C.c_int64(len(tgt)),
                                    C.c_int32(4), None, None, 10, 200, C.c_double(1.0), None, C.byref(best),
                                    None, None, None)
    assert rc == -1
    rc = N.lib().vcp_icp_multistart(vcp_ctx._h, N._ptr(src), C.c_int64(len(src)), N._ptr(tgt), C.c_int64(len(tgt)),
                                    C.c_int32(4), None, None, 10, 200, C.c_double(1.0), N._ptr(M), None,
                                    None, None, None)
    assert rc == -1
    # the context stays usable
    assert vcp_ctx.icp_multistart(cen, tru, 2, None, 10, 200, 1.0)["M"].shape == (4, 4)
