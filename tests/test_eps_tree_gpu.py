"""vcp_eps_tree on the MI355X: kdist, reach, the forest and its order equal to the numpy restatement of the Kruskal walk
(tests/eps_tree_ref.py) bit for bit, on the smallest shapes at which each mechanism can go wrong; the four guarantees of
include/vcp.h against vcp_dbscan on the device; the device-pointer form, kdist_given, determinism, phases and errors."""
import ctypes as C
import functools

import numpy as np
import pytest

import eps_tree_ref as R
from vtkcloudpoint_amd import _native as N
from vtkcloudpoint_amd import epstree as ET

pytestmark = pytest.mark.gpu

METRICS = (N.L1_2D, N.L2_2D, N.L2_3D)


def _check(ctx, c, k, eps_max, metric, ref=None, **kw):
    """Device == restatement, exactly; returns (device result, restatement)."""
    c = np.ascontiguousarray(c, np.float64)
    g = ctx.eps_tree(c, k, eps_max, metric, **kw)
    g["n_merge"] = len(g["merge_w"])
    ref = ref or R.eps_tree(c, k, eps_max, metric)
    bad = R.same(g, ref)
    assert bad is None, "%s differs (n %d, k %d, eps_max %r, metric %d)" % (bad, len(c), k, eps_max, metric)
    assert 0 <= g["rounds"] <= R.round_bound(ref["n_p"]), (g["rounds"], ref["n_p"])
    assert (g["rounds"] == 0) == (ref["n_merge"] == 0)
    return g, ref


def _dim(metric):
    return 3 if metric == N.L2_3D else 2


@pytest.mark.parametrize("n", [0, 1, 2])
def test_trivial_sizes(vcp_ctx, n):
    for metric in METRICS:
        c = np.arange(n * _dim(metric), dtype=np.float64).reshape(n, _dim(metric)) * 0.5
        g, ref = _check(vcp_ctx, c, 1, 10.0, metric)
        assert len(g["merge_w"]) == max(n - 1, 0)
        g, _ = _check(vcp_ctx, c, 2, 10.0, metric)          # n = 1: kdist +inf, P empty
        if n == 2:
            assert g["merge_a"].tolist() == [0] and g["merge_b"].tolist() == [1]
            g, _ = _check(vcp_ctx, c, 1, 0.25, metric)      # the two are farther apart than eps_max: no edge
            assert len(g["merge_w"]) == 0 and g["rounds"] == 0


def test_identical_points(vcp_ctx):
    for metric in METRICS:
        g, _ = _check(vcp_ctx, np.full((5, _dim(metric)), 1.25), 3, 0.5, metric)   # every key ties but for the indices
        assert g["merge_a"].tolist() == [0] * 4 and g["merge_b"].tolist() == [1, 2, 3, 4]
    # 3000 in one cell: the heavy kernels, 47 chunks of the one cell.  The walk accepts (0, 1), (0, 2), ... first: a star on index 0.
    # 591 = 9 * 64 + 15 and 592 = 9 * 64 + 16: the last chunk on either side of DENSE_CHUNK (the wave per slot, a lane per slot)
    for n in (3000, 591, 592):
        star = dict(kdist=np.zeros(n), reach=np.zeros(n), n_merge=n - 1, merge_w=np.zeros(n - 1),
                    merge_a=np.zeros(n - 1, np.int32), merge_b=np.arange(1, n, dtype=np.int32), n_p=n)
        for metric in (N.L1_2D, N.L2_3D):
            _check(vcp_ctx, np.full((n, _dim(metric)), -7.5), 7, 0.125, metric, ref=star)


def test_a_sparse_cell_beside_a_dense_one(vcp_ctx):
    """700 points in one cell make their neighbours' walks long; the few points of the next cell are too few for a lane
    each and get the whole wave, one at a time."""
    rng = np.random.default_rng(16)
    for metric in METRICS:
        d = _dim(metric)
        dense = np.full((700, d), 0.5) + rng.integers(0, 3, (700, d)) * 0.125
        few = np.full((5, d), 0.5)
        few[:, 0] = 1.5625 + np.arange(5) * 0.0625       # the box starts at 0.5: the next cell
        far = np.full((1, d), 0.5)
        far[0, 0] = 5.0                                   # stretches the box: cells [0.5, 1.5), [1.5, 2.5), ...
        c = np.concatenate([dense, few, far])
        g, ref = _check(vcp_ctx, c, 3, 1.0, metric)
        assert ref["n_p"] == 705 and len(g["merge_w"]) == 704


@pytest.mark.parametrize("metric", [N.L1_2D, N.L2_2D])
@pytest.mark.parametrize("k", [1, 4])
def test_full_ties_on_a_lattice(vcp_ctx, metric, k):
    x, y = np.meshgrid(np.arange(8.0), np.arange(8.0))
    c = np.stack([x.ravel(), y.ravel()], 1)
    for eps_max in (1.0, 2.0, 20.0):
        _check(vcp_ctx, c, k, eps_max, metric)
    _check(vcp_ctx, c[np.random.default_rng(5).permutation(64)], k, 2.0, metric)


def test_chains(vcp_ctx):
    eq = np.stack([np.arange(9.0), np.zeros(9)], 1)                       # mutual picks everywhere
    g, _ = _check(vcp_ctx, eq, 1, 1.5, N.L1_2D)
    assert len(g["merge_w"]) == 8
    _check(vcp_ctx, eq, 2, 1.5, N.L2_2D)
    # strictly growing gaps: every point's lightest edge is the one to its left, so ONE round picks all 8 edges and
    # hooks the 9 components into a chain 8 long (the path the flattening kernel has to follow)
    grow = np.stack([np.cumsum(np.arange(9.0) * 0.5 + 1.0), np.zeros(9)], 1)
    for metric in (N.L1_2D, N.L2_2D):
        g, _ = _check(vcp_ctx, grow, 1, 6.0, metric)
        assert len(g["merge_w"]) == 8 and g["rounds"] == 1
    _check(vcp_ctx, grow[::-1], 1, 6.0, N.L1_2D)
    # several rounds: gaps 1 2 1 3 1 2 1 4 ... (the ruler sequence) join pairs, then fours, then eights, then all 16 --
    # floor(log2 16) rounds, the bound met exactly
    ruler = [1.0 + ((i & -i).bit_length() - 1) for i in range(1, 16)]
    line = np.stack([np.concatenate([[0.0], np.cumsum(ruler)]), np.zeros(16)], 1)
    for metric in (N.L1_2D, N.L2_2D):
        g, _ = _check(vcp_ctx, line, 1, 6.0, metric)
        assert len(g["merge_w"]) == 15 and g["rounds"] == 4


def test_forest_not_a_tree(vcp_ctx):
    rng = np.random.default_rng(12)
    a = rng.uniform(0, 1, (200, 2))
    b = rng.uniform(0, 1, (200, 2)) + [3.0, 0.0]
    c = np.concatenate([a, b, [[2.0, 0.5]]])                             # the bridge point is >= 1 from either blob
    for metric in (N.L1_2D, N.L2_2D):
        g, ref = _check(vcp_ctx, c, 1, 0.9, metric)
        assert ref["n_p"] == 401 and len(g["merge_w"]) < ref["n_p"] - 1
        g, ref = _check(vcp_ctx, c, 1, 1.6, metric)                       # and with it, one tree
        assert len(g["merge_w"]) == 400


def test_sparse_ring_reaches_without_being_core(vcp_ctx):
    rng = np.random.default_rng(13)
    blob = rng.uniform(-0.5, 0.5, (300, 2))
    t = np.linspace(0, 2 * np.pi, 12, endpoint=False)
    ring = 0.9 * np.stack([np.cos(t), np.sin(t)], 1)                      # 12 points, ~0.47 apart, ~0.3 off the blob
    c = np.concatenate([blob, ring])
    for metric in (N.L1_2D, N.L2_2D):
        g, ref = _check(vcp_ctx, c, 6, 0.45, metric)
        out = ~(g["kdist"][300:] <= 0.45)
        assert out.any() and np.isfinite(g["reach"][300:][out]).any()


def test_non_finite_rows(vcp_ctx):
    rng = np.random.default_rng(14)
    for metric in METRICS:
        c = rng.integers(0, 16, (400, _dim(metric))).astype(np.float64) * 0.25
        bad = rng.choice(400, 30, replace=False)
        c[bad[:10], 0] = np.nan
        c[bad[10:20], 1] = np.inf
        c[bad[20:], _dim(metric) - 1] = -np.inf
        g, _ = _check(vcp_ctx, c, 3, 0.75, metric)
        assert np.isnan(g["kdist"][bad]).all() and np.isnan(g["reach"][bad]).all()
        assert not np.isin(g["merge_a"], bad).any() and not np.isin(g["merge_b"], bad).any()
    allbad = np.full((7, 2), np.nan)
    g, _ = _check(vcp_ctx, allbad, 1, 1.0, N.L1_2D)
    assert len(g["merge_w"]) == 0


def test_high_k(vcp_ctx):
    c = np.random.default_rng(15).uniform(0, 1, (300, 3))
    for metric in (N.L1_2D, N.L2_3D):
        _check(vcp_ctx, c if metric == N.L2_3D else c[:, :2], 64, 0.6, metric)


@functools.lru_cache(maxsize=None)
def _cloud(metric):
    """3000 unquantised random points, eps_max at about 3 mean spacings; the restatement, computed once."""
    d = _dim(metric)
    c = np.random.default_rng(20 + metric).uniform(0, 1, (3000, d))
    eps_max = 3.0 * (1.0 / 3000) ** (1.0 / d)
    k = 4
    return c, k, eps_max, R.eps_tree(c, k, eps_max, metric)


@pytest.mark.parametrize("metric", METRICS)
def test_many_cells(vcp_ctx, metric):
    c, k, eps_max, ref = _cloud(metric)
    g, _ = _check(vcp_ctx, c, k, eps_max, metric, ref=ref)
    assert len(g["merge_w"]) > 2000


@pytest.mark.parametrize("metric", METRICS)
def test_one_cell(vcp_ctx, metric):
    c = _cloud(metric)[0][:600]
    g, ref = _check(vcp_ctx, c, 4, 4.0, metric)          # eps_max above the extent: everybody is everybody's candidate
    assert len(g["merge_w"]) == 599


@pytest.mark.parametrize("metric", METRICS)
def test_the_four_guarantees_against_dbscan(vcp_ctx, metric):
    c, k, eps_max, ref = _cloud(metric)
    g = vcp_ctx.eps_tree(c, k, eps_max, metric)
    tree = ET.EpsTree(g["kdist"], g["reach"], g["merge_w"], g["merge_a"], g["merge_b"], eps_max, k, g["rounds"])
    kd = np.sort(g["kdist"][g["kdist"] <= eps_max])
    v_kd, v_w = float(kd[len(kd) // 2]), float(g["merge_w"][len(g["merge_w"]) // 2])
    eps_list = [eps_max, v_kd, v_w, np.nextafter(v_kd, -np.inf), np.nextafter(v_w, -np.inf)]
    eps_list += list(np.linspace(kd[0], eps_max, 5)[1:4])
    for eps in eps_list:
        eps = float(eps)
        r = vcp_ctx.dbscan(c, eps, k, metric)
        cores, clusters, labelled = ET.counts_at(tree, eps)
        assert int(r["is_core"].sum()) == cores == int((g["kdist"] <= eps).sum()), eps
        assert r["cf"] == clusters == cores - int((g["merge_w"] <= eps).sum()), eps
        assert int((r["labels"] != 0).sum()) == labelled == int((g["reach"] <= eps).sum()), eps
        core = r["is_core"].astype(bool)
        assert np.array_equal(ET.core_labels_at(tree, eps)[core], r["labels"][core]), eps
        assert not ET.core_labels_at(tree, eps)[~core].any()


def test_device_form_given_kdist_no_edges_and_determinism(vcp_ctx):
    import torch
    c, k, eps_max, ref = _cloud(N.L2_3D)
    n = len(c)
    a = vcp_ctx.eps_tree(c, k, eps_max, N.L2_3D)
    b = vcp_ctx.eps_tree(c, k, eps_max, N.L2_3D)
    for key in ("kdist", "reach", "merge_w", "merge_a", "merge_b"):
        assert a[key].tobytes() == b[key].tobytes(), key
    # kdist_given on the call's own output: identical bits, and the array is read, not written
    kd = a["kdist"].copy()
    h = vcp_ctx.eps_tree(c, k, eps_max, N.L2_3D, kdist=kd)
    for key in ("kdist", "reach", "merge_w", "merge_a", "merge_b"):
        assert a[key].tobytes() == h[key].tobytes(), key
    kd2, _ = vcp_ctx.kdist(c, k, N.L2_3D)
    assert kd2.tobytes() == a["kdist"].tobytes()
    # want_edges = False
    e = vcp_ctx.eps_tree(c, k, eps_max, N.L2_3D, want_edges=False)
    assert e["merge_a"] is None and e["merge_b"] is None
    assert e["merge_w"].tobytes() == a["merge_w"].tobytes() and e["reach"].tobytes() == a["reach"].tobytes()
    # device pointers
    t = torch.from_numpy(c).cuda()
    d_kd = torch.empty(n, dtype=torch.float64, device="cuda")
    d_re = torch.empty(n, dtype=torch.float64, device="cuda")
    d_w = torch.empty(n - 1, dtype=torch.float64, device="cuda")
    d_a = torch.empty(n - 1, dtype=torch.int32, device="cuda")
    d_b = torch.empty(n - 1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    m, rounds = vcp_ctx.eps_tree_dev(t.data_ptr(), n, 3, k, eps_max, d_w.data_ptr(), d_a.data_ptr(), d_b.data_ptr(),
                                     d_kd.data_ptr(), d_re.data_ptr(), metric=N.L2_3D)
    assert m == len(a["merge_w"]) and rounds == a["rounds"]
    assert d_kd.cpu().numpy().tobytes() == a["kdist"].tobytes() and d_re.cpu().numpy().tobytes() == a["reach"].tobytes()
    assert d_w[:m].cpu().numpy().tobytes() == a["merge_w"].tobytes()
    assert np.array_equal(d_a[:m].cpu().numpy(), a["merge_a"]) and np.array_equal(d_b[:m].cpu().numpy(), a["merge_b"])
    # the same with the k-distances given and nothing but merge_w asked for
    d_w2 = torch.zeros(n - 1, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    m2, _ = vcp_ctx.eps_tree_dev(t.data_ptr(), n, 3, k, eps_max, d_w2.data_ptr(), d_kdist=d_kd.data_ptr(),
                                 kdist_given=True, metric=N.L2_3D)
    assert m2 == m and d_w2[:m].cpu().numpy().tobytes() == a["merge_w"].tobytes()


def test_python_front_end(vcp_ctx):
    c, k, eps_max, ref = _cloud(N.L1_2D)
    tree = ET.eps_tree(c, k, eps_max, "L1_2D", ctx=vcp_ctx)
    assert R.same(dict(kdist=tree.kdist, reach=tree.reach, merge_w=tree.merge_w, merge_a=tree.merge_a,
                       merge_b=tree.merge_b), ref) is None
    auto = ET.eps_tree(c, k, None, "L1_2D", ctx=vcp_ctx, kd=tree.kdist)
    from vtkcloudpoint_amd.kdist import suggest_eps
    assert auto.eps_max == 2.0 * suggest_eps(None, k, kd=tree.kdist)
    assert auto.kdist.tobytes() == tree.kdist.tobytes()
    breaks, clusters = ET.cluster_count_steps(tree)
    target = int(clusters[len(clusters) // 2])
    lo, hi = ET.eps_for_clusters(tree, target)[0]
    assert vcp_ctx.dbscan(c, 0.5 * (lo + hi), k, N.L1_2D)["cf"] == target


def test_phase_names(vcp_ctx):
    c = np.random.default_rng(30).uniform(0, 1, (500, 2))
    vcp_ctx.timing_enable(True)
    try:
        g = vcp_ctx.eps_tree(c, 4, 0.1, N.L1_2D)
        assert [p[0] for p in vcp_ctx.timing()] == ["epst_kdist", "epst_grid", "epst_rounds", "epst_reach", "epst_sort"]
        vcp_ctx.eps_tree(c, 4, 0.1, N.L1_2D, kdist=g["kdist"])
        assert [p[0] for p in vcp_ctx.timing()] == ["epst_grid", "epst_rounds", "epst_reach", "epst_sort"]
    finally:
        vcp_ctx.timing_enable(False)


def test_every_error_leaves_the_outputs_alone(vcp_ctx):
    lib = N.lib()
    c = np.random.default_rng(31).uniform(0, 1, (10, 3))
    far = np.array([[-1e308, 0.0, 0.0], [1e308, 0.0, 0.0]])

    def call(code, coords=c, n=10, dim=2, metric=N.L1_2D, k=2, eps_max=0.5, given=0, drop=()):
        kd, reach, mw = np.full(10, 77.0), np.full(10, 77.0), np.full(9, 77.0)
        ma, mb = np.full(9, 77, np.int32), np.full(9, 77, np.int32)
        m, rounds = C.c_int64(77), C.c_int32(77)
        p = dict(coords=N._ptr(coords), kd=N._ptr(kd), reach=N._ptr(reach), m=C.byref(m), mw=N._ptr(mw), ma=N._ptr(ma),
                 mb=N._ptr(mb), rounds=C.byref(rounds))
        for name in drop:
            p[name] = None
        rc = lib.vcp_eps_tree(vcp_ctx._h, p["coords"], C.c_int64(n), int(dim), int(metric), int(k), C.c_double(eps_max),
                              int(given), p["kd"], p["reach"], p["m"], p["mw"], p["ma"], p["mb"], p["rounds"])
        assert rc == code, (rc, code, n, dim, metric, k, eps_max, given, drop)
        if code != 0:
            assert (kd == 77.0).all() and (reach == 77.0).all() and (mw == 77.0).all()
            assert (ma == 77).all() and (mb == 77).all() and m.value == 77 and rounds.value == 77

    ARG, UNSUP, LARGE = -1, -8, -5
    call(0)
    call(0, drop=("kd", "reach", "ma", "mb", "rounds"))
    call(ARG, drop=("m",))
    call(ARG, drop=("mw",))
    call(ARG, drop=("coords",))
    call(ARG, drop=("ma",))
    call(ARG, drop=("mb",))
    call(ARG, given=1, drop=("kd",))
    call(ARG, dim=1)
    call(ARG, dim=4)
    call(ARG, dim=2, metric=N.L2_3D)
    call(ARG, metric=N.SIGNED_SUM_2D)
    call(ARG, k=0)
    for e in (np.nan, 0.0, -1.0, np.inf):
        call(ARG, eps_max=e)
    call(ARG, n=-1)
    call(UNSUP, k=65)
    call(UNSUP, coords=far, n=2, dim=3)
    call(UNSUP, coords=far, n=2, dim=3, given=1)
    call(LARGE, n=1 << 31)
    call(0, n=0)
