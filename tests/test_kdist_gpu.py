"""vcp_kdist on the MI355X: bit-identical to a numpy brute force of the same binary64 expression, the identity
vcp_dbscan(eps, min_pts = k).is_core == (kdist <= eps) at scale, the edge rules of vcp.h, determinism, the torch
device path and suggest_eps on planted blobs."""
import time

import numpy as np
import pytest

from vtkcloudpoint_amd import _native as N
from vtkcloudpoint_amd import kdist as KD
from vtkcloudpoint_amd import synth

# the brute force: shared with tests/fuzz_queries.py
from kdist_ref import brute_rows as _brute_rows, dist_rows as _dist_rows  # noqa: F401

pytestmark = pytest.mark.gpu


def _same(a, b, msg):
    assert np.array_equal(a, b, equal_nan=True), msg


def test_ties_brute_force(vcp_ctx):
    rng = np.random.default_rng(11)
    for trial in range(300):
        n = int(rng.integers(1, 301))
        metric = int(rng.integers(0, 3))
        dim = 3 if metric == N.L2_3D else int(rng.integers(2, 4))
        c = rng.integers(0, 12, size=(n, dim)).astype(np.float64) * 0.25
        k = int(rng.integers(1, min(64, n + 3) + 1))
        kd, knn = vcp_ctx.kdist(c, k, metric, want_knn=True)
        bkd, bknn = _brute_rows(c, k, metric, np.arange(n))
        _same(kd, bkd, "trial %d kdist (n %d k %d metric %d)" % (trial, n, k, metric))
        _same(knn, bknn, "trial %d knn" % trial)


@pytest.mark.parametrize("shape", ["uniform", "blobs"])
def test_unquantised_clouds(vcp_ctx, shape):
    from scipy.spatial import cKDTree
    rng = np.random.default_rng(3 if shape == "uniform" else 4)
    for n, metric, k in ((20000, N.L1_2D, 10), (20000, N.L2_3D, 7), (5000, N.L2_2D, 33), (3000, N.L2_3D, 64)):
        dim = 3 if metric == N.L2_3D else 2
        if shape == "uniform":
            c = rng.uniform(-5, 5, (n, dim))
        else:
            cen = rng.uniform(-50, 50, (8, dim))
            c = cen[rng.integers(0, 8, n)] + rng.normal(0, 0.3, (n, dim))
            c[: n // 10] = rng.uniform(-60, 60, (n // 10, dim))
        kd, knn = vcp_ctx.kdist(c, k, metric, want_knn=True)
        bkd, bknn = _brute_rows(c, k, metric, np.arange(n))
        _same(kd, bkd, "%s n %d metric %d kdist" % (shape, n, metric))
        _same(knn, bknn, "%s knn" % shape)
        gd = 3 if metric == N.L2_3D else 2
        t, _ = cKDTree(c[:, :gd]).query(c[:, :gd], k=k, p=1 if metric == N.L1_2D else 2)
        np.testing.assert_allclose(kd, t[:, k - 1], rtol=1e-15, atol=0)


def _identity(ctx, c, metric, kd, eps_list, k):
    for eps in eps_list:
        g = ctx.dbscan(c, float(eps), k, metric)
        want = (kd <= eps).astype(np.uint8)
        bad = np.nonzero(g["is_core"] != want)[0]
        assert bad.size == 0, "eps %r: %d points disagree, first %s" % (eps, bad.size, bad[:5])


@pytest.mark.parametrize("n", [1_000_000, 10_000_000])
def test_dbscan_identity_at_scale(vcp_ctx, n):
    d = synth.config_cloud(n)
    rng = np.random.default_rng(n % 1000 + 1)
    k = 10
    for coords, metric, eps0 in ((d["motor"], N.L1_2D, d["eps_l1"]), (d["xyz"], N.L2_3D, d["eps_l2"])):
        kd, _ = vcp_ctx.kdist(coords, k, metric)
        assert np.isfinite(kd).all()
        picks = kd[rng.integers(0, n, 3)]
        eps_list = [eps0] + list(np.quantile(kd, [0.1, 0.5, 0.9], method="lower")) + list(picks) + \
            [np.nextafter(v, -np.inf) for v in picks]
        _identity(vcp_ctx, coords, metric, kd, eps_list, k)


def test_sampled_brute_force_10m(vcp_ctx):
    d = synth.config_cloud(10_000_000)
    c = d["motor"]
    k = 10
    kd, knn = vcp_ctx.kdist(c, k, N.L1_2D, want_knn=True)
    rows = np.random.default_rng(9).choice(len(c), 256, replace=False)
    bkd, bknn = _brute_rows(c, k, N.L1_2D, rows)
    _same(kd[rows], bkd, "kdist")
    _same(knn[rows], bknn, "knn")


def test_edge_cases(vcp_ctx):
    kd, knn = vcp_ctx.kdist(np.zeros((0, 2)), 5, N.L1_2D, want_knn=True)
    assert kd.shape == (0,) and knn.shape == (0, 5)
    c = np.array([[0.0, 0.0], [1.0, 0.0], [0.0, 3.0]])
    kd, knn = vcp_ctx.kdist(c, 5, N.L1_2D, want_knn=True)  # n < k
    assert np.all(kd == np.inf)
    assert np.array_equal(knn, [[0, 1, 2, -1, -1], [1, 0, 2, -1, -1], [2, 0, 1, -1, -1]])
    rng = np.random.default_rng(1)
    r = rng.uniform(0, 1, (1000, 3))
    kd, knn = vcp_ctx.kdist(r, 1, N.L2_3D, want_knn=True)  # k = 1: the point itself
    assert np.all(kd == 0.0) and np.array_equal(knn[:, 0], np.arange(1000))
    # 100 k identical points
    same = np.full((100_000, 2), 1.25)
    kd, knn = vcp_ctx.kdist(same, 16, N.L2_2D, want_knn=True)
    assert np.all(kd == 0.0)
    assert np.array_equal(knn, np.broadcast_to(np.arange(16, dtype=np.int32), (100_000, 16)))
    # NaN / inf coordinates: NaN rows, nobody's neighbour
    c = rng.integers(0, 20, (2000, 2)).astype(np.float64) * 0.5
    bad = rng.choice(2000, 40, replace=False)
    c[bad[:20], 0] = np.nan
    c[bad[20:30], 1] = np.inf
    c[bad[30:], 0] = -np.inf
    kd, knn = vcp_ctx.kdist(c, 6, N.L1_2D, want_knn=True)
    assert np.all(np.isnan(kd[bad])) and np.all(knn[bad] == -1)
    bkd, bknn = _brute_rows(c, 6, N.L1_2D, np.arange(2000))
    _same(kd, bkd, "non-finite kdist")
    _same(knn, bknn, "non-finite knn")
    assert not np.isin(knn, bad).any()
    # points on a line (zero extent in y), 2-D and 3-D
    x = rng.uniform(0, 100, 5000)
    line = np.stack([x, np.full(5000, 7.0), np.zeros(5000)], 1)
    for metric in (N.L1_2D, N.L2_3D):
        kd, knn = vcp_ctx.kdist(line, 9, metric, want_knn=True)
        bkd, bknn = _brute_rows(line, 9, metric, np.arange(5000))
        _same(kd, bkd, "line kdist")
        _same(knn, bknn, "line knn")


def test_far_outliers_exact_and_fast(vcp_ctx):
    d = synth.config_cloud(10_000_000)
    base = d["motor"]
    far = np.array([[1e12, 1e12], [-1e12, 1e12], [1e12, -1e12], [-1e12, -1e12], [1e12, 0.0], [5.0, -1e12]])
    c = np.concatenate([base, far])
    k = 10
    vcp_ctx.kdist(base, k, N.L1_2D)  # warm
    t0 = time.perf_counter()
    vcp_ctx.kdist(base, k, N.L1_2D)
    t_plain = time.perf_counter() - t0
    t0 = time.perf_counter()
    kd, knn = vcp_ctx.kdist(c, k, N.L1_2D, want_knn=True)
    t_far = time.perf_counter() - t0
    rows = np.concatenate([np.arange(len(base), len(c)), np.random.default_rng(2).choice(len(base), 64, replace=False)])
    bkd, bknn = _brute_rows(c, k, N.L1_2D, rows)
    _same(kd[rows], bkd, "far kdist")
    _same(knn[rows], bknn, "far knn")
    assert t_far < 5.0 * t_plain + 0.5, (t_far, t_plain)


def test_refusals(vcp_ctx):
    c = np.zeros((10, 2))
    with pytest.raises(N.VcpError) as e:
        vcp_ctx.kdist(c, 65, N.L1_2D)
    assert e.value.code == -8
    with pytest.raises(N.VcpError) as e:
        vcp_ctx.kdist(c, 0, N.L1_2D)
    assert e.value.code == -1
    with pytest.raises(N.VcpError) as e:
        vcp_ctx.kdist(c, 5, N.SIGNED_SUM_2D)
    assert e.value.code == -1
    with pytest.raises(N.VcpError) as e:
        vcp_ctx.kdist(np.array([[-1e308, 0.0], [1e308, 0.0]]), 1, N.L1_2D)
    assert e.value.code == -8


def test_determinism_and_device_path(vcp_ctx):
    import torch
    d = synth.config_cloud(1_000_000)
    a, ka = vcp_ctx.kdist(d["xyz"], 32, N.L2_3D, want_knn=True)
    b, kb = vcp_ctx.kdist(d["xyz"], 32, N.L2_3D, want_knn=True)
    assert a.tobytes() == b.tobytes() and np.array_equal(ka, kb)
    t = torch.from_numpy(d["xyz"]).cuda()
    g = KD.k_distance(t, 32, "L2_3D", ctx=vcp_ctx)
    assert isinstance(g, torch.Tensor) and g.is_cuda
    assert g.cpu().numpy().tobytes() == a.tobytes()
    h = KD.k_distance(d["motor"], 7, "L1_2D", ctx=vcp_ctx)
    tm = torch.from_numpy(d["motor"]).cuda()
    assert KD.k_distance(tm, 7, "L1_2D", ctx=vcp_ctx).cpu().numpy().tobytes() == h.tobytes()


def test_point3d_lists(vcp_ctx):
    from vtkcloudpoint_amd.datamodel import points_from_arrays
    d = synth.config_c1()
    pts = points_from_arrays(motor=d["motor"], xyz=d["xyz"])
    a = KD.k_distance(pts, 10, "L1_2D", ctx=vcp_ctx)
    b, _ = vcp_ctx.kdist(d["motor"], 10, N.L1_2D)
    assert a.tobytes() == b.tobytes()
    a = KD.k_distance(pts, 10, "L2_3D", ctx=vcp_ctx)
    b, _ = vcp_ctx.kdist(d["xyz"], 10, N.L2_3D)
    assert a.tobytes() == b.tobytes()


def test_oracle_is_key(vcp_ctx, oracle):
    d = synth.config_c1()
    kd, _ = vcp_ctx.kdist(d["motor"], d["min_pts"], N.L1_2D)
    o = oracle.dbscan(d["motor"], d["eps_l1"], d["min_pts"], N.L1_2D, literal=True)
    assert np.array_equal(o["is_key"].astype(bool), kd <= d["eps_l1"])


def test_suggest_eps_planted_blobs(vcp_ctx):
    rng = np.random.default_rng(21)
    cen = rng.uniform(5, 95, (20, 2))
    blobs = (cen[:, None, :] + rng.uniform(-0.5, 0.5, (20, 2000, 2))).reshape(-1, 2)   # density 2000 per unit area
    bg = rng.uniform(0, 100, (10000, 2))                                                # density 1
    c = np.concatenate([blobs, bg])
    kd = KD.k_distance(c, 10, "L1_2D", ctx=vcp_ctx)
    e = KD.suggest_eps(c, 10, "L1_2D", ctx=vcp_ctx)
    lo = np.quantile(kd[: len(blobs)], 0.95)
    hi = np.quantile(kd[len(blobs):], 0.05)
    assert lo <= e <= hi, (lo, e, hi)
