"""vcp_gdbscan on the MI355X: labels, core flags, the cluster count and the neighbourhood weights equal to the numpy
restatement of the definition (tests/gdbscan_ref.py), and where stated to vcp_dbscan on the device, on the smallest shapes
at which each mechanism can go wrong; the device-pointer form, the early exit, independence from the context's history,
phases and errors.  Every comparison is equality."""
import ctypes as C

import numpy as np
import pytest

import gdbscan_ref as R
from vtkcloudpoint_amd import _native as N

pytestmark = pytest.mark.gpu

METRICS = (N.L1_2D, N.L2_2D, N.L2_3D)


def _dim(metric):
    return 3 if metric == N.L2_3D else 2


def _check(ctx, c, eps, mw, metric, weights=None, aux=None, gate=None, cf_in=0, ref=None):
    """Device == restatement, exactly, with W asked for and with the early exit; returns (device result, restatement)."""
    c = np.ascontiguousarray(c, np.float64)
    ref = ref or R.gdbscan(c, eps, mw, metric, weights, aux, gate, cf_in)
    what = "(n %d, eps %r, min_weight %d, metric %d)" % (len(c), eps, mw, metric)
    g = ctx.gdbscan(c, eps, mw, metric, weights, aux, gate, cf_in, want_wsum=True)
    bad = R.same(g, ref)
    assert bad is None, "%s differs %s" % (bad, what)
    e = ctx.gdbscan(c, eps, mw, metric, weights, aux, gate, cf_in)
    bad = R.same(e, ref)
    assert bad is None and e["wsum"] is None, "%s differs without wsum %s" % (bad, what)
    return g, ref


def _dev(ctx, c, eps, mw, metric, weights=None, aux=None, gate=0.0, cf_in=0, wsum=True):
    """The device-pointer form on torch tensors."""
    import torch
    c = np.ascontiguousarray(c, np.float64)
    n, dim = c.shape
    t = torch.from_numpy(c).cuda()
    tw = None if weights is None else torch.from_numpy(np.ascontiguousarray(weights, np.int32)).cuda()
    ta = None if aux is None else torch.from_numpy(np.ascontiguousarray(aux, np.float64)).cuda()
    lab = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    core = torch.full((n,), 9, dtype=torch.uint8, device="cuda")
    ws = torch.full((n,), -5, dtype=torch.int64, device="cuda") if wsum else None
    torch.cuda.synchronize()                      # the library runs on its own stream
    cf = ctx.gdbscan_dev(t.data_ptr(), n, dim, eps, mw, lab.data_ptr(), metric,
                         d_weights=None if tw is None else tw.data_ptr(), d_aux=None if ta is None else ta.data_ptr(),
                         gate=gate, cf_in=cf_in, d_is_core=core.data_ptr(), d_wsum=None if ws is None else ws.data_ptr())
    return dict(labels=lab.cpu().numpy(), is_core=core.cpu().numpy(), cf=cf, wsum=None if ws is None else ws.cpu().numpy())


def _dbscan_dev(ctx, c, eps, min_pts, metric):
    import torch
    c = np.ascontiguousarray(c, np.float64)
    n, dim = c.shape
    t = torch.from_numpy(c).cuda()
    lab = torch.zeros(n, dtype=torch.int32, device="cuda")
    core = torch.zeros(n, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    cf, _ = ctx.dbscan_dev(t.data_ptr(), n, dim, eps, min_pts, metric, d_labels=lab.data_ptr(), d_is_core=core.data_ptr())
    return dict(labels=lab.cpu().numpy(), is_core=core.cpu().numpy(), cf=cf)


@pytest.mark.parametrize("n", [0, 1, 2])
def test_trivial_sizes(vcp_ctx, n):
    for metric in METRICS:
        c = np.arange(n * _dim(metric), dtype=np.float64).reshape(n, _dim(metric)) * 0.5
        g, _ = _check(vcp_ctx, c, 10.0, 1, metric, cf_in=3)
        assert g["cf"] == 3 + (n > 0) and g["labels"].tolist() == [4] * n
        _check(vcp_ctx, c, 10.0, 3, metric)                  # nobody is core
        _check(vcp_ctx, c, 0.25, 1, metric)                  # farther apart than eps: a cluster each
        _check(vcp_ctx, c, 10.0, 5, metric, weights=[2, 3][:n], aux=[1.0, 1.5][:n], gate=0.5)


def test_identical_points(vcp_ctx):
    for metric in METRICS:
        g, _ = _check(vcp_ctx, np.full((5, _dim(metric)), 1.25), 0.5, 5, metric)
        assert g["labels"].tolist() == [1] * 5 and g["wsum"].tolist() == [5] * 5
        _check(vcp_ctx, np.full((5, _dim(metric)), 1.25), 0.0, 6, metric)
    # 3000 in one cell: the heavy kernels, 47 chunks of the one cell; every W is the total weight.  591 = 9 * 64 + 15 and
    # 592 = 9 * 64 + 16: the last chunk on either side of DENSE_CHUNK (the wave per slot, a lane per slot)
    for n in (3000, 591, 592):
        w = (np.arange(n) % 4).astype(np.int32)
        total = int(w.sum())
        ref = dict(labels=np.ones(n, np.int32), is_core=np.ones(n, np.uint8), wsum=np.full(n, total, np.int64), cf=1)
        none = dict(labels=np.zeros(n, np.int32), is_core=np.zeros(n, np.uint8), wsum=np.full(n, total, np.int64), cf=0)
        for metric in (N.L1_2D, N.L2_3D):
            c = np.full((n, _dim(metric)), -7.5)
            _check(vcp_ctx, c, 0.125, total, metric, weights=w, ref=ref)
            _check(vcp_ctx, c, 0.125, total + 1, metric, weights=w, ref=none)


def test_a_sparse_cell_beside_a_dense_one(vcp_ctx):
    """600 points in one cell make their neighbours' walks long; the few points of the next cell are too few for a lane
    each and get the whole wave, one at a time."""
    rng = np.random.default_rng(16)
    for metric in METRICS:
        d = _dim(metric)
        dense = np.full((600, d), 0.5) + rng.integers(0, 3, (600, d)) * 0.125
        few = np.full((5, d), 0.5)
        few[:, 0] = 1.5625 + np.arange(5) * 0.0625       # the box starts at 0.5: the next cell
        far = np.full((1, d), 0.5)
        far[0, 0] = 5.0                                   # stretches the box: cells [0.5, 1.5), [1.5, 2.5), ...
        c = np.concatenate([dense, few, far])
        w = rng.integers(0, 3, len(c)).astype(np.int32)
        aux = rng.integers(0, 2, len(c)).astype(np.float64)
        g, ref = _check(vcp_ctx, c, 1.0, 400, metric)
        assert ref["is_core"][:600].any() and not ref["is_core"][600:].all()
        _check(vcp_ctx, c, 1.0, 300, metric, weights=w, aux=aux, gate=0.5)
        _check(vcp_ctx, c, 1.0, 606, metric)             # the few are border rows of the dense cell's cores, or noise
        _check(vcp_ctx, c[::-1], 1.0, 500, metric, weights=w)


@pytest.mark.parametrize("metric", [N.L1_2D, N.L2_2D])
def test_full_ties_on_a_lattice(vcp_ctx, metric):
    x, y = np.meshgrid(np.arange(8.0), np.arange(8.0))
    c = np.stack([x.ravel(), y.ravel()], 1) * 0.375       # spacing exactly eps
    for mw in (3, 4, 5, 6):                               # corners have 3 neighbours, edges 4, the inside 5
        g, ref = _check(vcp_ctx, c, 0.375, mw, metric)
    assert ref["cf"] == 0
    _check(vcp_ctx, c[np.random.default_rng(5).permutation(64)], 0.375, 5, metric)
    _check(vcp_ctx, c, 0.375, 9, metric, weights=np.arange(64) % 3)


def test_a_chain_whose_aux_steps_equal_the_gate(vcp_ctx):
    n = 30
    c = np.stack([np.arange(n) * 0.25, np.zeros(n)], 1)
    aux = 4.0 + np.arange(n) * 0.125                      # exact steps inside one binade: the same ulp everywhere
    g, ref = _check(vcp_ctx, c, 0.25, 3, N.L1_2D, aux=aux, gate=0.125)
    assert ref["cf"] == 1 and ref["labels"].all()
    up = aux.copy()
    up[20:] = np.nextafter(up[20:], np.inf) + 0.0         # the step 19 -> 20 is one ulp above the gate
    assert up[20] - up[19] > 0.125
    g, ref = _check(vcp_ctx, c, 0.25, 3, N.L1_2D, aux=up, gate=0.125)
    assert ref["cf"] == 2 and ref["labels"][19] == 1 and ref["labels"][20] == 2
    _check(vcp_ctx, c, 0.25, 2, N.L2_2D, aux=up, gate=np.inf)
    _check(vcp_ctx, c, 0.25, 2, N.L2_2D, aux=up, gate=0.0)


def test_special_rows_and_parameters(vcp_ctx):
    rng = np.random.default_rng(8)
    for metric in METRICS:
        d = _dim(metric)
        c = np.round(rng.uniform(0, 2, (400, d)) * 16) / 16
        c[rng.integers(0, 400, 12), rng.integers(0, d, 12)] = np.nan
        c[rng.integers(0, 400, 6), 0] = np.inf
        c[rng.integers(0, 400, 6), 1] = -np.inf
        aux = rng.integers(0, 3, 400).astype(np.float64)
        aux[rng.integers(0, 400, 10)] = np.nan
        aux[rng.integers(0, 400, 5)] = np.inf
        w = rng.integers(0, 4, 400).astype(np.int32)      # zeros included
        eps = 0.2 if d == 2 else 0.3
        for mw in (6, 1, 0, -3):
            _check(vcp_ctx, c, eps, mw, metric, cf_in=10)
            _check(vcp_ctx, c, eps, mw, metric, weights=w, aux=aux, gate=1.0, cf_in=-4)
        for bad_eps in (-1.0, np.nan):
            g, _ = _check(vcp_ctx, c, bad_eps, 1, metric, weights=w)
            assert not g["labels"].any() and not g["wsum"].any()
            g, _ = _check(vcp_ctx, c, bad_eps, 0, metric, aux=aux, gate=1.0, cf_in=7)
            assert g["labels"].tolist() == list(range(8, 408))
        _check(vcp_ctx, c, np.inf, 50, metric, weights=w)  # one cell, every finite pair
        allbad = np.full((7, d), np.nan)
        _check(vcp_ctx, allbad, 1.0, 1, metric)
        _check(vcp_ctx, allbad, 1.0, 0, metric, cf_in=2)
    # three rows of weight 2^30: the sum does not fit an int32
    big = [1 << 30] * 3
    g, _ = _check(vcp_ctx, np.zeros((3, 2)), 0.5, 3 << 30, N.L1_2D, weights=big)
    assert g["is_core"].all() and g["wsum"].tolist() == [3 << 30] * 3
    g, _ = _check(vcp_ctx, np.zeros((3, 2)), 0.5, (3 << 30) + 1, N.L1_2D, weights=big)
    assert not g["is_core"].any()


@pytest.fixture(scope="module")
def random_clouds():
    """3000 random points per metric over many cells with weights 1..3 and two range layers; the restatement's results."""
    rng = np.random.default_rng(77)
    out = {}
    for metric in METRICS:
        d = _dim(metric)
        n = 3000
        c = rng.uniform(0, 4, (n, d))
        c[: n // 4] = 1.0 + rng.normal(0, 0.2, (n // 4, d))           # two dense blobs over a sparse background
        c[n // 4: n // 2] = 3.0 + rng.normal(0, 0.2, (n // 2 - n // 4, d))
        c = np.round(c * 256) / 256
        w = rng.integers(1, 4, n).astype(np.int32)
        aux = np.where(rng.uniform(size=n) < 0.5, 5.0, 9.0) + rng.uniform(0, 0.5, n)
        eps, mw = (0.06, 0.06, 0.16)[metric], 8
        out[metric] = dict(c=c, w=w, aux=aux, eps=eps, mw=mw)
    return out


@pytest.mark.parametrize("metric", METRICS)
def test_random_sweep(vcp_ctx, random_clouds, metric):
    s = random_clouds[metric]
    c, w, aux, eps, mw = s["c"], s["w"], s["aux"], s["eps"], s["mw"]
    # plain: the restatement, and vcp_dbscan on the device
    g, ref = _check(vcp_ctx, c, eps, mw, metric)
    assert ref["cf"] >= 2 and 0 < ref["is_core"].sum() < len(c)
    d = vcp_ctx.dbscan(c, eps, mw, metric)
    assert R.same(g, dict(labels=d["labels"], is_core=d["is_core"], cf=d["cf"]), wsum=False) is None
    # weighted: the restatement, and vcp_dbscan on the expanded cloud restricted to the first copies
    g, refw = _check(vcp_ctx, c, eps, mw, metric, weights=w)
    assert not np.array_equal(refw["is_core"], ref["is_core"])
    d = vcp_ctx.dbscan(R.expand(c, w), eps, mw, metric)
    n = len(c)
    assert R.same(g, dict(labels=d["labels"][:n], is_core=d["is_core"][:n], cf=d["cf"]), wsum=False) is None
    # gated, and both
    g, refg = _check(vcp_ctx, c, eps, mw // 2, metric, aux=aux, gate=0.5)
    assert not np.array_equal(refg["labels"], R.gdbscan(c, eps, mw // 2, metric)["labels"])
    _check(vcp_ctx, c, eps, mw, metric, weights=w, aux=aux, gate=0.5, cf_in=100)


def test_expanded_cloud_where_a_row_is_not_its_own_neighbour(vcp_ctx):
    """Found by tests/fuzz_queries.py (gdbscan, seed 10, case 144): one row of weight 3, eps = -5e-324 (the double below
    a distance of 0), min_weight 0.  N is empty, the row is core by min_weight <= 0 and one cluster; in the expanded
    cloud its three copies are no neighbours of each other and make three.  The device follows the definition (the
    restatement); include/vcp.h now says where the two readings part: the first copies' labels agree, cf_out does not.
    With min_weight >= 1, or eps >= 0 on finite rows, they are one reading."""
    c = np.array([[2.0 ** 40, 2.0 ** 40], [2.0 ** 40 + 1.0, 2.0 ** 40], [np.nan, 0.0]])
    w = np.array([3, 1, 2], np.int32)
    for eps, mw, together in ((-5e-324, 0, False), (np.nan, -1, False), (0.0, 0, False), (-5e-324, 1, True),
                              (0.0, 1, True), (1.0, 0, False), (1.0, 2, True)):
        g, ref = _check(vcp_ctx, c, eps, mw, N.L1_2D, weights=w, cf_in=3)
        d = vcp_ctx.dbscan(R.expand(c, w), eps, mw, N.L1_2D, 3)
        assert np.array_equal(g["labels"], d["labels"][:3]) and np.array_equal(g["is_core"], d["is_core"][:3]), (eps, mw)
        assert (g["cf"] == d["cf"]) == together, (eps, mw, g["cf"], d["cf"])
    fin, wf = c[:2], w[:2]                                   # finite rows, eps >= 0: one reading for every min_weight
    for eps, mw in ((0.0, 0), (0.0, -2), (1.0, 0), (1.0, 4), (1.0, 5)):
        g, _ = _check(vcp_ctx, fin, eps, mw, N.L1_2D, weights=wf, cf_in=3)
        d = vcp_ctx.dbscan(R.expand(fin, wf), eps, mw, N.L1_2D, 3)
        assert R.same(g, dict(labels=d["labels"][:2], is_core=d["is_core"][:2], cf=d["cf"]), wsum=False) is None, (eps, mw)


def test_context_history(vcp_ctx, random_clouds):
    s = random_clouds[N.L2_2D]
    c, w, aux, eps, mw = s["c"], s["w"], s["aux"], s["eps"], s["mw"]
    a = vcp_ctx.gdbscan(c, eps, mw, N.L2_2D, w, aux, 0.5, 3, want_wsum=True)
    b = vcp_ctx.gdbscan(c, eps, mw, N.L2_2D, w, aux, 0.5, 3, want_wsum=True)
    assert R.same(a, b) is None                                           # two calls: identical bits
    dv = _dev(vcp_ctx, c, eps, mw, N.L2_2D, w, aux, 0.5, 3)
    assert R.same(dv, a) is None                                          # the device form equals the host form
    dv = _dev(vcp_ctx, c, eps, mw, N.L2_2D, w, aux, 0.5, 3, wsum=False)
    assert R.same(dv, a) is None
    other = random_clouds[N.L2_3D]
    vcp_ctx.dbscan(other["c"], 0.3, 5, N.L2_3D)
    vcp_ctx.eps_tree(other["c"][:500], 4, 0.5, N.L2_3D)
    vcp_ctx.gdbscan(other["c"][:100], 1.0, 2, N.L2_3D)
    b = vcp_ctx.gdbscan(c, eps, mw, N.L2_2D, w, aux, 0.5, 3, want_wsum=True)
    assert R.same(a, b) is None                                           # after other calls on the same context
    fresh = N.Context(0)
    try:
        assert R.same(fresh.gdbscan(c, eps, mw, N.L2_2D, w, aux, 0.5, 3, want_wsum=True), a) is None
    finally:
        fresh.close()


def test_timing_phases(vcp_ctx, random_clouds):
    s = random_clouds[N.L1_2D]
    vcp_ctx.timing_enable(True)
    try:
        vcp_ctx.gdbscan(s["c"], s["eps"], s["mw"], N.L1_2D, s["w"])
        names = [nm for nm, _ in vcp_ctx.timing()]
    finally:
        vcp_ctx.timing_enable(False)
    assert names == ["gdb_bounds", "gdb_grid", "gdb_count", "gdb_union", "gdb_label"]


def _raw(ctx, c, metric, eps, mw, weights=None, aux=None, gate=0.0, n=None, dim=None, handle=True, coords=True,
         labels=True, cf_out=True):
    """The C entry point on sentinel-filled outputs: (status, outputs untouched?)."""
    c = np.ascontiguousarray(c, np.float64)
    rows = len(c)
    lab = np.full(rows, -7, np.int32)
    core = np.full(rows, 9, np.uint8)
    ws = np.full(rows, -5, np.int64)
    cf = C.c_int32(-3)
    w = None if weights is None else np.ascontiguousarray(weights, np.int32)
    a = None if aux is None else np.ascontiguousarray(aux, np.float64)
    p = N._ptr
    rc = N.lib().vcp_gdbscan(ctx._h if handle else None, p(c) if coords else None, C.c_int64(rows if n is None else n),
                             int(c.shape[1] if dim is None else dim), int(metric), C.c_double(eps), p(a), C.c_double(gate),
                             p(w), C.c_int64(mw), C.c_int32(0), p(lab) if labels else None, p(core), p(ws),
                             C.byref(cf) if cf_out else None)
    untouched = (lab == -7).all() and (core == 9).all() and (ws == -5).all() and cf.value == -3
    return rc, bool(untouched)


def test_error_codes_leave_the_outputs_untouched(vcp_ctx):
    ARG, TOO_LARGE, UNSUPPORTED = -1, -5, -8
    c2, c3 = np.zeros((4, 2)), np.zeros((4, 3))
    assert _raw(vcp_ctx, c2, N.L1_2D, 1.0, 1, handle=False) == (ARG, True)
    assert _raw(vcp_ctx, c2, N.L1_2D, 1.0, 1, coords=False) == (ARG, True)
    assert _raw(vcp_ctx, c2, N.L1_2D, 1.0, 1, labels=False) == (ARG, True)
    assert _raw(vcp_ctx, c2, N.L1_2D, 1.0, 1, cf_out=False) == (ARG, True)
    assert _raw(vcp_ctx, c2, N.L1_2D, 1.0, 1, dim=4) == (ARG, True)
    assert _raw(vcp_ctx, c2, N.L1_2D, 1.0, 1, dim=1) == (ARG, True)
    assert _raw(vcp_ctx, c2, N.L2_3D, 1.0, 1) == (ARG, True)
    assert _raw(vcp_ctx, c3, N.SIGNED_SUM_2D, 1.0, 1) == (ARG, True)
    assert _raw(vcp_ctx, c2, N.L1_2D, 1.0, 1, aux=np.zeros(4), gate=np.nan) == (ARG, True)
    assert _raw(vcp_ctx, c2, N.L1_2D, 1.0, 1, aux=np.zeros(4), gate=-0.5) == (ARG, True)
    assert _raw(vcp_ctx, c2, N.L1_2D, 1.0, 1, aux=np.zeros(4), gate=np.inf) == (0, False)
    assert _raw(vcp_ctx, c2, N.L1_2D, 1.0, 1, gate=np.nan) == (0, False)            # no aux: the gate is not read
    assert _raw(vcp_ctx, c2, N.L1_2D, 1.0, 1, weights=[1, 0, -1, 2]) == (ARG, True)
    assert _raw(vcp_ctx, c2, N.L1_2D, 1.0, 1, n=1 << 31) == (TOO_LARGE, True)
    assert _raw(vcp_ctx, c2, N.L1_2D, 1.0, 1, n=-1) == (ARG, True)
    wide = np.array([[-1.7e308, 0.0], [1.7e308, 0.0], [0.0, 0.0], [0.0, 0.0]])
    assert _raw(vcp_ctx, wide, N.L2_2D, 1.0, 1) == (UNSUPPORTED, True)
    # one negative weight in the last row of 100 000: found on the device before any output is touched
    n = 100_000
    c = np.random.default_rng(4).uniform(0, 30, (n, 2))
    w = np.ones(n, np.int32)
    w[-1] = -1
    assert _raw(vcp_ctx, c, N.L1_2D, 0.1, 3, weights=w) == (ARG, True)
    with pytest.raises(N.VcpError) as e:
        vcp_ctx.gdbscan(c, 0.1, 3, N.L1_2D, weights=w)
    assert e.value.code == ARG and "weight" in str(e.value)
    # and the call after the error is a clean one
    w[-1] = 1
    g = vcp_ctx.gdbscan(c, 0.1, 3, N.L1_2D, weights=w)
    d = vcp_ctx.dbscan(c, 0.1, 3, N.L1_2D)
    assert R.same(g, dict(labels=d["labels"], is_core=d["is_core"], cf=d["cf"]), wsum=False) is None
    # n == 0: cf_out = cf_in, nothing else
    cf = C.c_int32(-3)
    assert N.lib().vcp_gdbscan(vcp_ctx._h, None, C.c_int64(0), 2, 0, C.c_double(1.0), None, C.c_double(0.0), None,
                               C.c_int64(1), C.c_int32(12), None, None, None, C.byref(cf)) == 0 and cf.value == 12


def test_a_million_points_with_unit_weights_equal_vcp_dbscan(vcp_ctx):
    from vtkcloudpoint_amd import synth
    d = synth.config_cloud(1_000_000)
    want = _dbscan_dev(vcp_ctx, d["motor"], d["eps_l1"], d["min_pts"], N.L1_2D)
    assert want["cf"] > 1
    got = _dev(vcp_ctx, d["motor"], d["eps_l1"], d["min_pts"], N.L1_2D, wsum=False)
    assert R.same(got, want, wsum=False) is None


def test_counts_on_distinct_rows_equal_vcp_dbscan_on_the_expanded_cloud(vcp_ctx):
    from vtkcloudpoint_amd import synth
    from vtkcloudpoint_amd.gdbscan import multiplicity
    motor = synth.config_cloud(300_000)["motor"]
    first, _ = multiplicity(motor)
    rows = motor[first]                                   # ~300 k distinct rows
    n = len(rows)
    counts = np.random.default_rng(6).integers(1, 4, n).astype(np.int32)
    big = R.expand(rows, counts)                          # ~600 k rows: every row counts[i] times
    assert n > 290_000 and len(big) == counts.sum()
    want = _dbscan_dev(vcp_ctx, big, 0.1, 10, N.L1_2D)
    got = _dev(vcp_ctx, rows, 0.1, 10, N.L1_2D, weights=counts, wsum=False)
    assert want["cf"] > 1
    assert R.same(got, dict(labels=want["labels"][:n], is_core=want["is_core"][:n], cf=want["cf"]), wsum=False) is None
    # and multiplicity() undoes the expansion, whatever the order of the raw rows
    perm = np.random.default_rng(7).permutation(len(big))
    f2, c2 = multiplicity(big[perm])
    back = _dev(vcp_ctx, big[perm][f2], 0.1, 10, N.L1_2D, weights=c2, wsum=False)
    assert back["cf"] == want["cf"] and int(back["is_core"].sum()) == int(got["is_core"].sum())


def test_host_mirror(vcp_ctx):
    from vtkcloudpoint_amd.datamodel import points_from_arrays
    from vtkcloudpoint_amd.dbscan import DBImproved
    from vtkcloudpoint_amd.gdbscan import gdbscan
    rng = np.random.default_rng(31)
    motor = np.round(rng.uniform(0, 1, (500, 2)) * 64) / 64
    motor[7, 0] = np.nan
    dist = np.where(rng.uniform(size=500) < 0.5, 3.0, 8.0) + rng.uniform(0, 0.25, 500)
    cnt = rng.integers(1, 4, 500).astype(np.int32)
    for gate, use in ((None, False), (0.5, False), (None, True), (0.5, True)):
        lst = points_from_arrays(motor=motor)
        for p, dd, k in zip(lst, dist, cnt):
            p.Distance, p.ptsCount = float(dd), int(k)
        db = DBImproved(vcp_ctx)
        db.cf = 4
        db.dbscanGeneral(lst, 0.05, 6, gate=gate, usePtsCount=use)
        labels, core, k = gdbscan(motor, 0.05, 6, weights=cnt if use else None, aux=None if gate is None else dist,
                                  gate=gate, cf_in=4, ctx=vcp_ctx)
        assert [p.clusterId for p in lst] == labels.tolist() and [p.isKeyPoint for p in lst] == core.tolist()
        assert [p.isClassed for p in lst] == (labels != 0).tolist()
        assert db.clusterAmount == 4 + k == db.cf and db.pointsAmount == 500 and k >= 1
    # min_weight <= 0: the non-finite row is a cluster of its own and, like the C#'s seed with an empty list, not classed
    lst = points_from_arrays(motor=motor[:20])
    db = DBImproved(vcp_ctx)
    db.dbscanGeneral(lst, 0.05, 0)
    assert lst[7].clusterId != 0 and lst[7].isKeyPoint and not lst[7].isClassed
    assert all(p.isClassed for i, p in enumerate(lst) if i != 7)
