"""vcp_cluster_spheres on the MI355X: every output of the host form and of the device-pointer form equal to the numpy
restatement of the definition (tests/cluster_spheres_ref.py), doubles by their bits, on the cluster sizes around the chunk
boundaries, with the radius free and fixed, with weights, on strided rows and on the clusters that are hard in kind; the
contracts every entry point keeps (independence from the context's history, untouched outputs on every error, NULL outputs,
empty calls, timing phases, the caller's stream); and one scene from resident tensors through the fit, the rejection step
and the match."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import centroid_ref as CR
import cluster_spheres_ref as R
from vtkcloudpoint_amd import _native as N
from vtkcloudpoint_amd import spheres as S

pytestmark = pytest.mark.gpu

POISON = -7.25
K_CASE = max(CR.SLOTS)
FIXED = 0.25            # the fixed radius of the parity cases: inside the range of the clusters' own radii
NAN = 0x7FF8000000000000


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _outs(K, dim, keys=R.KEYS):
    shapes = dict(centre=(K, dim), radius=(K,), rms=(K,), cap=(K,), step=(K,), alg=(K, dim + 1), valid=(K,), counts=(K,))
    o = {}
    for k in keys:
        if k == "valid":
            o[k] = torch.full(shapes[k], 9, dtype=torch.uint8, device="cuda")
        elif k == "counts":
            o[k] = torch.full(shapes[k], -7, dtype=torch.int64, device="cuda")
        else:
            o[k] = torch.full(shapes[k], POISON, dtype=torch.float64, device="cuda")
    return o


def _dev_call(ctx, wide, off, dim, labels, K, weights=None, fixed=0.0, rounds=3, keys=R.KEYS):
    """The device-pointer form on columns off .. off + dim of the [n, ld] array `wide`, read in place."""
    wide = np.ascontiguousarray(wide, np.float64)
    dw, dl = _dev(wide), _dev(np.ascontiguousarray(labels, np.int32))
    dwt = None if weights is None else _dev(np.ascontiguousarray(weights, np.int32))
    o = _outs(K, dim, keys)
    torch.cuda.synchronize()
    ctx.cluster_spheres_dev(dw.data_ptr() + 8 * off, wide.shape[1], dim, dl.data_ptr(),
                            None if dwt is None else dwt.data_ptr(), len(labels), K, fixed, rounds,
                            **{"d_" + k: v.data_ptr() for k, v in o.items()})
    return {k: v.cpu().numpy() for k, v in o.items()}


def _check(ctx, pts, labels, K, weights=None, fixed=0.0, rounds=3, want=None, pad=0):
    """Host form and device-pointer form == the restatement, with the points as columns pad .. pad + dim of an array
    2 * pad wider.  Returns the restatement."""
    n, dim = pts.shape
    want = R.spheres(pts, labels, K, weights, fixed, rounds) if want is None else want
    wide = np.full((n, dim + 2 * pad), 1e300)          # what stands beside the columns must not matter
    wide[:, pad:pad + dim] = pts
    got = ctx.cluster_spheres(wide[:, pad:pad + dim], labels, K, weights, fixed_radius=fixed, rounds=rounds)
    assert R.differs(got, want) is None, "host form, ld %d: %s" % (dim + 2 * pad, R.differs(got, want))
    got = _dev_call(ctx, wide, pad, dim, labels, K, weights, fixed, rounds)
    assert R.differs(got, want) is None, "device form, ld %d: %s" % (dim + 2 * pad, R.differs(got, want))
    return want


# ---- size classes -----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _case():
    lab = CR.case_labels()
    return lab, R.case_points(lab), R.case_weights(lab)


@pytest.mark.parametrize("weighted", [False, True], ids=["w1", "weights"])
@pytest.mark.parametrize("fixed", [0.0, FIXED], ids=["free", "fixed"])
@pytest.mark.parametrize("rounds", [0, 1, 3])
@pytest.mark.parametrize("dim", [2, 3])
def test_size_classes(vcp_ctx, dim, rounds, fixed, weighted):
    """Every cluster a cap of a sphere of its own, every fourth a blob (parity only); dim 2 reads X, Y of the same rows."""
    lab, xyz, w = _case()
    w = w if weighted else None
    pts = np.ascontiguousarray(xyz[:, :dim])
    want = _check(vcp_ctx, pts, lab, K_CASE, w, fixed, rounds)                       # ld = dim
    _check(vcp_ctx, pts, lab, K_CASE, w, fixed, rounds, want=want, pad=1)            # ld = dim + 2
    if dim == 2:                                                                     # xyz[:, :2] in place: ld = 3
        got = vcp_ctx.cluster_spheres(xyz[:, :2], lab, K_CASE, w, fixed_radius=fixed, rounds=rounds)
        assert R.differs(got, want) is None, R.differs(got, want)
    sizes = dict(zip(CR.SLOTS, CR.SIZES))
    rows = np.array([sizes.get(k, 0) for k in range(1, K_CASE + 1)])
    if not weighted:
        assert want["counts"].tolist() == rows.tolist()
        need = dim if fixed else dim + 1
        assert (want["valid"][rows < need] == 0).all() and (want["valid"][rows >= 63] == 1).all()
    else:
        big = CR.SLOTS[CR.SIZES.index(257)] - 1
        assert want["counts"][big] > 2 ** 20 and want["valid"][big] == 1
    bad = want["valid"] == 0
    for k in ("centre", "radius", "rms", "cap", "step", "alg"):
        assert (R.bits(want[k][bad]) == NAN).all() and np.isfinite(want[k][~bad]).all(), k
    if dim == 3 and not fixed and rounds == 3 and not weighted:                      # the caps are fitted, not only equal
        shaped = (rows >= 255) & (np.arange(K_CASE) % 4 != 3)                        # case_points: every fourth is a blob
        assert shaped.sum() >= 6 and (want["rms"][shaped] < 0.004).all() and (want["cap"][shaped] > 0.5).all()
        assert ((want["radius"][shaped] > 0.04) & (want["radius"][shaped] < 0.55)).all()


def test_counts_and_mean_are_those_of_cluster_moments(vcp_ctx):
    """counts on the size classes, with and without weights; the mean on the lattice, where u0 is exactly 0 and alg's
    centre therefore is the mean the fit started from."""
    lab, xyz, w = _case()
    for wt in (None, w):
        s = vcp_ctx.cluster_spheres(xyz, lab, K_CASE, wt, rounds=0, outputs=("counts",))
        m = vcp_ctx.cluster_moments(xyz, lab, K_CASE, wt, outputs=("counts",))
        assert np.array_equal(s["counts"], m["counts"])
    for dim in (2, 3):
        x, c, r = R.exact_family(dim)
        one = np.ones(len(x), np.int32)
        s = vcp_ctx.cluster_spheres(x, one, 1, rounds=0)
        m = vcp_ctx.cluster_moments(x, one, 1, outputs=("mean", "counts"))
        assert R.same(s["alg"][:, :dim], m["mean"]) and np.array_equal(s["counts"], m["counts"])
        assert s["centre"][0].tolist() == c.tolist() and s["radius"][0] == r and s["alg"][0, dim] == r


def test_weights_against_duplicated_rows(vcp_ctx):
    """Row i repeated w_i times with weight 1 is the same point set: the same counts and, to the rounding of sums that
    fill the tree differently, the same fit.  |centre| <= 30 and 5 rounds: 1e-9 is far above either form's error
    (tests/test_cluster_spheres.py measures below 1e-14) and far below any difference in the fit."""
    rng = np.random.default_rng(43)
    K, per = 5, 700
    lab = np.repeat(np.arange(1, K + 1), per).astype(np.int32)
    pts = np.vstack([R.cap_points(rng, rng.uniform(5, 12) * np.array([1.0, 0.5 * k, -1.0]) / 2, per, R=0.3, noise=0.002)
                     for k in range(K)])
    perm = rng.permutation(len(lab))
    lab, pts = lab[perm], pts[perm]
    w = rng.integers(0, 5, len(lab)).astype(np.int32)
    rep = np.repeat(np.arange(len(lab)), w)
    for fixed in (0.0, 0.3):
        gw = _check(vcp_ctx, pts, lab, K, w, fixed, 5)
        gd = _check(vcp_ctx, pts[rep], lab[rep], K, None, fixed, 5)
        assert np.array_equal(gw["counts"], gd["counts"]) and (gw["valid"] == 1).all() and (gd["valid"] == 1).all()
        for k in ("centre", "radius", "rms", "cap", "alg"):
            assert np.abs(gw[k] - gd[k]).max() <= 1e-9, k


# ---- hard clusters -----------------------------------------------------------------------------------------------------------
def _hard(dim):
    """name -> (points [m, dim], weights or None, valid expected for (free, fixed); None where only parity is asked)."""
    rng = np.random.default_rng([77, dim])
    x, c, r = R.exact_family(dim)
    cases = {}
    for m in (1, 2, 3, 4, 5):
        cases["lattice_%d" % m] = (x[:m], None, None)
        cases["random_%d" % m] = (rng.uniform(-4, 4, (m, dim)), None, None)
    cases["lattice"] = (x, None, (1, 1))
    cases["coincident"] = (np.tile(c, (7, 1)), None, (0, 0))
    cases["collinear"] = (np.outer(np.arange(8.0), [1.0, 2.0, -1.0][:dim]) + c, None, (0, 0))
    if dim == 3:
        cases["coplanar"] = (np.array([[a, b, 3.0] for a in range(4) for b in range(4)], np.float64), None, (0, 0))
    cases["nan_member"] = (np.vstack([x, [np.nan] + [0.0] * (dim - 1)]), None, (0, 0))
    cases["inf_member"] = (np.vstack([x, [0.0] * (dim - 1) + [np.inf]]), None, (0, 0))
    cases["minus_inf_member"] = (np.vstack([x, [-np.inf] * dim]), None, (0, 0))
    w0 = np.ones(len(x) + 1, np.int32)
    w0[-1] = 0
    cases["member_at_the_centre_w0"] = (np.vstack([x, c]), w0, (1, 1))
    cases["member_at_the_centre"] = (np.vstack([x, c]), None, None)
    cases["all_weights_zero"] = (x, np.zeros(len(x), np.int32), (0, 0))
    cases["far_1e8"] = (R.cap_points(rng, np.array([9.0, -4.0, 3.0][:dim]), 200, noise=0.001, dim=dim) + 1e8, None, (1, None))
    return cases, r


@pytest.mark.parametrize("dim", [2, 3])
def test_hard_clusters(vcp_ctx, dim):
    """K = 1 with 1 to 5 members (the validity limits of both forms) and every degenerate kind, each also as one cluster
    among ordinary ones in a single call."""
    cases, r = _hard(dim)
    for name, (x, w, valid) in cases.items():
        lab = np.ones(len(x), np.int32)
        for fi, fixed in enumerate((0.0, r)):
            for rounds in (0, 1, 3):
                want = _check(vcp_ctx, x, lab, 1, w, fixed, rounds)
                assert want["counts"][0] == (len(x) if w is None else int(w.sum())), name
                m = len(x)
                if name.startswith(("lattice_", "random_")) and m < (dim if fixed else dim + 1):
                    assert want["valid"][0] == 0, (name, fixed)
                if valid is not None and valid[fi] is not None:
                    assert want["valid"][0] == valid[fi], (name, fixed, rounds)
                if want["valid"][0] == 0:
                    assert all((R.bits(want[k]) == NAN).all() for k in ("centre", "radius", "rms", "cap", "step", "alg"))
    names = sorted(cases)                                                            # all of them in one call: odd labels,
    pts = np.vstack([cases[nm][0] for nm in names])                                  # the even ones empty
    lab = np.concatenate([np.full(len(cases[nm][0]), 2 * j + 1, np.int32) for j, nm in enumerate(names)])
    w = np.concatenate([np.ones(len(cases[nm][0]), np.int32) if cases[nm][1] is None else cases[nm][1] for nm in names])
    for fixed in (0.0, r):
        both = _check(vcp_ctx, pts, lab, 2 * len(names), w, fixed, 3)
        for j, nm in enumerate(names):                   # a cluster's result is its own, and a weight of 1 is no weight
            alone = R.spheres(cases[nm][0], np.ones(len(cases[nm][0]), np.int32), 1, cases[nm][1], fixed, 3)
            assert all(R.same(both[k][2 * j], alone[k][0]) for k in R.KEYS), (nm, fixed)
        assert (both["counts"][1::2] == 0).all() and (both["valid"][1::2] == 0).all()


# ---- contracts -----------------------------------------------------------------------------------------------------------------
def _small(seed, n, K, dim=3):
    """K noisy caps and some rows in no cluster, scattered; weights 0..3."""
    rng = np.random.default_rng(seed)
    lab = rng.integers(0, K + 1, n).astype(np.int32)
    pts = rng.uniform(-9, 9, (n, dim))
    for k in range(1, K + 1):
        ix = np.flatnonzero(lab == k)
        v = rng.normal(size=dim)
        pts[ix] = R.cap_points(rng, rng.uniform(5, 20) * v / np.linalg.norm(v), len(ix), R=0.4, noise=0.002, dim=dim)
    return pts, lab, rng.integers(0, 4, n).astype(np.int32)


def test_independent_of_the_contexts_history_and_run_to_run(vcp_ctx):
    pts, lab, w = _small(61, 40000, 9)
    first = _dev_call(vcp_ctx, pts, 0, 3, lab, 9, w)
    assert R.differs(first, R.spheres(pts, lab, 9, w, 0.0, 3)) is None and (first["valid"] == 1).all()
    again = _dev_call(vcp_ctx, pts, 0, 3, lab, 9, w)
    assert all(R.same(first[k], again[k]) for k in R.KEYS)                         # run to run
    big = _small(62, 200000, 300)
    _dev_call(vcp_ctx, big[0], 0, 3, big[1], 300, big[2], 0.4, 5)                  # a larger call in between, other arguments
    assert all(R.same(first[k], _dev_call(vcp_ctx, pts, 0, 3, lab, 9, w)[k]) for k in R.KEYS)
    tiny = _small(63, 50, 2, 2)
    _dev_call(vcp_ctx, tiny[0], 0, 2, tiny[1], 2)                                  # a smaller one, another dim, no weights
    assert all(R.same(first[k], _dev_call(vcp_ctx, pts, 0, 3, lab, 9, w)[k]) for k in R.KEYS)
    vcp_ctx.cluster_moments(pts, lab, 9, w)                                        # the call that shares the grouping
    assert all(R.same(first[k], _dev_call(vcp_ctx, pts, 0, 3, lab, 9, w)[k]) for k in R.KEYS)
    vcp_ctx.release_workspace()
    assert all(R.same(first[k], _dev_call(vcp_ctx, pts, 0, 3, lab, 9, w)[k]) for k in R.KEYS)
    host = vcp_ctx.cluster_spheres(pts, lab, 9, w, rounds=3)
    assert all(R.same(first[k], host[k]) for k in R.KEYS)


def _raw(ctx, dev, pts, ld, dim, lab, w, n, K, fixed, rounds, outs):
    f = N.lib().vcp_cluster_spheres_dev if dev else N.lib().vcp_cluster_spheres
    p = (lambda a: None if a is None else C.c_void_p(a.data_ptr())) if dev else (lambda a: None if a is None else C.c_void_p(a.ctypes.data))
    return f(ctx._h, p(pts), C.c_int64(ld), C.c_int(dim), p(lab), p(w), C.c_int64(n), C.c_int32(K), C.c_double(fixed),
             C.c_int(rounds), *(p(outs.get(k)) for k in R.KEYS))


def test_errors_leave_the_outputs_untouched(vcp_ctx):
    pts, lab, w = _small(64, 500, 4)
    bad_lab, neg_lab, bad_w = lab.copy(), lab.copy(), w.copy()
    bad_lab[77], neg_lab[3], bad_w[123] = 5, -1, -1
    cases = [("label above K", dict(lab=bad_lab), -4), ("negative label", dict(lab=neg_lab), -4),
             ("negative weight", dict(w=bad_w), -1), ("dim 1", dict(dim=1), -1), ("dim 4", dict(dim=4, ld=4), -1),
             ("ld below dim", dict(ld=2), -1), ("n negative", dict(n=-1), -1), ("K negative", dict(K=-1), -1),
             ("n beyond 32-bit indexing", dict(n=0x7FFFFFF0), -5),
             ("negative radius", dict(fixed=-0.1), -1), ("NaN radius", dict(fixed=float("nan")), -1),
             ("infinite radius", dict(fixed=float("inf")), -1), ("rounds -1", dict(rounds=-1), -1),
             ("rounds 65", dict(rounds=65), -1)]
    for dev in (False, True):
        for name, ch, code in cases:
            a = dict(lab=lab, w=w, dim=3, ld=3, n=len(lab), K=4, fixed=0.0, rounds=3)
            a.update(ch)
            if dev:
                outs = _outs(4, 3)
                args = (_dev(pts), a["ld"], a["dim"], _dev(a["lab"]), _dev(a["w"]))
                torch.cuda.synchronize()
            else:
                outs = {k: v.cpu().numpy() for k, v in _outs(4, 3).items()}
                args = (pts, a["ld"], a["dim"], a["lab"], a["w"])
            poison = {k: (v.clone() if dev else v.copy()) for k, v in outs.items()}
            rc = _raw(vcp_ctx, dev, *args, a["n"], a["K"], a["fixed"], a["rounds"], outs)
            assert rc == code, (dev, name, rc)
            for k in R.KEYS:
                got, was = (outs[k].cpu().numpy(), poison[k].cpu().numpy()) if dev else (outs[k], poison[k])
                assert R.same(got, was), (dev, name, k)
    assert N.lib().vcp_cluster_spheres(None, None, C.c_int64(3), C.c_int(3), None, None, C.c_int64(0), C.c_int32(0),
                                       C.c_double(0.0), C.c_int(0), None, None, None, None, None, None, None,
                                       None) == -1                                     # NULL ctx
    for rounds in (0, 64):                                                             # the ends of the range are in it
        assert R.differs(vcp_ctx.cluster_spheres(pts, lab, 4, w, rounds=rounds), R.spheres(pts, lab, 4, w, 0.0, rounds)) is None


def test_null_outputs_and_empty_calls(vcp_ctx):
    pts, lab, w = _small(65, 3000, 6)
    want = R.spheres(pts, lab, 6, w, 0.0, 3)
    for keys in (("centre",), ("valid",), ("counts", "radius"), ("rms", "cap"), ("alg", "step"), ()):
        got = vcp_ctx.cluster_spheres(pts, lab, 6, w, rounds=3, outputs=keys)
        assert set(got) == set(keys) and R.differs(got, want, keys) is None
        got = _dev_call(vcp_ctx, pts, 0, 3, lab, 6, w, keys=keys)
        assert R.differs(got, want, keys) is None
    # n == 0: every cluster is empty; K == 0: nothing to write
    for dim in (2, 3):
        e = vcp_ctx.cluster_spheres(np.zeros((0, dim)), np.zeros(0, np.int32), 3)
        assert R.differs(e, R.spheres(np.zeros((0, dim)), np.zeros(0, np.int32), 3)) is None
        assert (e["counts"] == 0).all() and (e["valid"] == 0).all() and (R.bits(e["alg"]) == NAN).all()
        z = vcp_ctx.cluster_spheres(np.ones((5, dim)), np.zeros(5, np.int32), 0)
        assert all(len(v) == 0 for v in z.values())
        assert _dev_call(vcp_ctx, np.zeros((1, dim)), 0, dim, np.zeros(0, np.int32), 2)["counts"].tolist() == [0, 0]
    with pytest.raises(N.VcpError) as err:                                           # K == 0 still checks the labels
        vcp_ctx.cluster_spheres(np.ones((5, 3)), np.ones(5, np.int32), 0)
    assert err.value.code == -4


def test_timing_phases(vcp_ctx):
    pts, lab, w = _small(66, 20000, 8)
    vcp_ctx.timing_enable(True)
    try:
        for rounds in (0, 4):
            _dev_call(vcp_ctx, pts, 0, 3, lab, 8, w, rounds=rounds)
            phases = vcp_ctx.timing()
            assert [nm for nm, _ in phases] == ["spheres_group", "spheres_start", "spheres_rounds"]
            assert all(ms >= 0.0 for _, ms in phases)
    finally:
        vcp_ctx.timing_enable(False)


def test_on_the_callers_stream():
    """vcp_set_stream holds for vcp_cluster_spheres_dev, by the method of test_stream_gpu.py (its rig, imported): the
    input is swapped behind a running filler on the caller's stream, so a launch on any other stream reads cloud A."""
    from test_stream_gpu import Rig
    rig = Rig()
    try:
        n, K = 30000, 7
        A, lab, w = _small(67, n, K)
        B = A + np.random.default_rng(68).normal(0, 0.01, A.shape)
        wa, wb = R.spheres(A, lab, K, w, 0.0, 3), R.spheres(B, lab, K, w, 0.0, 3)
        assert not R.same(wa["centre"], wb["centre"])
        buf, dB, dl, dw = _dev(A), _dev(B), _dev(lab), _dev(w)
        o = _outs(K, 3)
        rig.run(lambda: rig.ctx.cluster_spheres_dev(buf.data_ptr(), 3, 3, dl.data_ptr(), dw.data_ptr(), n, K, 0.0, 3,
                                                    **{"d_" + k: v.data_ptr() for k, v in o.items()}),
                [(buf, dB)], [(v, 9 if v.dtype == torch.uint8 else -7) for v in o.values()])
        assert R.differs({k: v.cpu().numpy() for k, v in o.items()}, wb) is None
    finally:
        rig.close()


# ---- end to end -------------------------------------------------------------------------------------------------------------
T_SCENE, B_SCENE, PER = 12, 3, 300


@functools.lru_cache(maxsize=None)
def _scene():
    """(pts [n, 3], labels, truths [12, 3]): twelve sphere targets (R = 0.0725, 5 to 20 from the instrument, 300 returns,
    range noise 0.0005), three blobs of the same size, 500 rows in no cluster; scattered."""
    rng = np.random.default_rng(91)
    truths = np.zeros((T_SCENE, 3))
    pts, lab = [], []
    for k in range(T_SCENE + B_SCENE):
        v = rng.normal(size=3)
        c = rng.uniform(5, 20) * v / np.linalg.norm(v)
        if k < T_SCENE:
            truths[k] = c
            pts.append(R.cap_points(rng, c, PER, noise=0.0005))
        else:
            pts.append(c + rng.normal(0, 0.05, (PER, 3)))
        lab.append(np.full(PER, k + 1, np.int32))
    pts.append(rng.uniform(-20, 20, (500, 3)))
    lab.append(np.zeros(500, np.int32))
    perm = rng.permutation((T_SCENE + B_SCENE) * PER + 500)
    return np.vstack(pts)[perm], np.concatenate(lab)[perm], truths


def test_scene_fit_reject_match(vcp_ctx):
    """The scene resident on the GPU.  The radius band with max_rms rejects exactly the blobs; vcp_match at a threshold of
    R / 4 pairs every target's fitted centre with its truth and none of the centroids.  R / 4 = 0.018 lies between the
    fit's error (below 0.002 here: the noise over sqrt(300), times the geometry of a cap) and the 2R/3 = 0.048 by which a
    mean sits in front of its centre."""
    RT, T, B, per = R.R_TARGET, T_SCENE, B_SCENE, PER
    pts, lab, truths = _scene()
    K = T + B
    d_pts, d_lab = _dev(pts), _dev(lab)
    fit = S.cluster_spheres(d_pts, d_lab, K, ctx=vcp_ctx)
    assert torch.is_tensor(fit.centre) and fit.centre.is_cuda
    want = R.spheres(pts, lab, K, None, 0.0, 12)
    assert R.differs({k: getattr(fit, k).cpu().numpy() for k in R.KEYS}, want) is None
    rejected = S.filter_by_spheres(d_lab, fit, r_min=0.8 * RT, r_max=1.25 * RT, max_rms=0.004, ctx=vcp_ctx)
    assert rejected == list(range(T + 1, K + 1))
    full = S.filter_by_spheres(d_lab, fit, r_min=0.8 * RT, r_max=1.25 * RT, max_rms=0.004, ctx=vcp_ctx, full=True)
    assert full["n_filtered"] == B and full["n_kept"] == T * per + 500
    assert np.array_equal(full["keep"].cpu().numpy() != 0, lab <= T)
    c3, _, cnt = vcp_ctx.centroids(pts, None, lab, K)
    centres = S.sphere_centres(fit, fallback=_dev(c3)).cpu().numpy()
    assert centres.shape == c3.shape and np.array_equal(cnt, want["counts"])
    thr = RT / 4
    m_fit = vcp_ctx.match(centres, truths, np.eye(4), thr)
    m_cen = vcp_ctx.match(c3, truths, np.eye(4), thr)
    err_fit = np.linalg.norm(centres[:T] - truths, axis=1)
    err_cen = np.linalg.norm(c3[:T] - truths, axis=1)
    print("\nfit error %.2e..%.2e, centroid error %.3f..%.3f (2R/3 = %.3f), threshold %.4f"
          % (err_fit.min(), err_fit.max(), err_cen.min(), err_cen.max(), 2 * RT / 3, thr))
    assert (m_fit["is_matched"][:T] == 1).all() and m_fit["nearest"][:T].tolist() == list(range(T))
    assert (m_cen["is_matched"][:T] == 0).all()
    assert err_fit.max() < thr / 4 and err_cen.min() > 2 * thr
    fixed = S.cluster_spheres(d_pts, d_lab, K, radius=RT, ctx=vcp_ctx)               # the known radius: fixed, as reported
    assert (fixed.radius[:T].cpu().numpy() == RT).all() and (fixed.valid[:T].cpu().numpy() == 1).all()


def test_host_surface_of_the_scene(vcp_ctx):
    """The same scene from numpy arrays: the package's lazy names, the host path of cluster_spheres and filter_by_spheres
    (the same bits and the same verdict as from tensors), and tools.getSpheres over the reference's class surface."""
    import vtkcloudpoint_amd as pkg
    from vtkcloudpoint_amd import tools
    from vtkcloudpoint_amd.datamodel import ClusObj, Point3D
    assert pkg.cluster_spheres is S.cluster_spheres and pkg.filter_by_spheres is S.filter_by_spheres
    assert pkg.sphere_centres is S.sphere_centres and pkg.ClusterSpheres is S.ClusterSpheres
    RT, T, K = R.R_TARGET, T_SCENE, T_SCENE + B_SCENE
    pts, lab, truths = _scene()
    fit = S.cluster_spheres(pts, lab, K, ctx=vcp_ctx)
    assert isinstance(fit.centre, np.ndarray) and (fit.dim, fit.K, fit.rounds, fit.fixed_radius) == (3, K, 12, 0.0)
    assert R.differs({k: getattr(fit, k) for k in R.KEYS}, R.spheres(pts, lab, K, None, 0.0, 12)) is None
    band = dict(r_min=0.8 * RT, r_max=1.25 * RT, max_rms=0.004, ctx=vcp_ctx)
    assert S.filter_by_spheres(lab, fit, **band) == list(range(T + 1, K + 1))
    full = S.filter_by_spheres(lab, fit, full=True, **band)
    assert np.array_equal(full["keep"] != 0, lab <= T) and np.array_equal(full["kept_idx"], np.flatnonzero(lab <= T))
    assert S.filter_by_spheres(lab, fit, ctx=vcp_ctx) == []                               # no criterion: nothing rejected
    assert S.filter_by_spheres(lab, fit, max_cap=0.4, ctx=vcp_ctx) == list(range(1, T + 1))   # caps are one-sided, blobs not
    assert S.filter_by_spheres(lab, fit, np.nan, np.nan, np.nan, np.nan, ctx=vcp_ctx) == []
    with pytest.raises(ValueError):
        S.cluster_spheres(pts, lab, K, radius=0.0, ctx=vcp_ctx)
    few = S.cluster_spheres(pts[:40], np.r_[np.ones(3, np.int32), np.full(37, 2, np.int32)], 3, ctx=vcp_ctx)
    assert few.valid.tolist() == [0, 1, 0] and few.counts.tolist() == [3, 37, 0]          # too few, fitted, empty
    assert S.filter_by_spheres(np.zeros(0, np.int32), few, ctx=vcp_ctx) == [1]            # members but no fit: rejected
    assert S.filter_by_spheres(np.zeros(0, np.int32), few, ctx=vcp_ctx, reject_invalid=False) == []
    cen = np.full((3, 3), 7.0)
    assert S.sphere_centres(few, fallback=cen)[[0, 2]].tolist() == [[7.0] * 3] * 2 and np.isnan(S.sphere_centres(few)[0]).all()
    clus = []
    for k in range(1, K + 1):
        ob = ClusObj()
        ob.li = [Point3D(*p) for p in pts[lab == k]]
        clus.append(ob)
    sph = tools.getSpheres(clus, True, ctx=vcp_ctx)
    assert [s.clusID for s in sph] == list(range(1, K + 1))
    assert all(np.linalg.norm(s.center - truths[s.clusID - 1]) < RT / 16 and abs(s.radius - RT) < 0.02 * RT for s in sph[:T])
    fixed = tools.getSpheres(clus[:T], True, radius=RT, ctx=vcp_ctx)
    assert all(s.radius == RT and np.linalg.norm(s.center - truths[s.clusID - 1]) < RT / 16 for s in fixed)
