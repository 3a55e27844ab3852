"""The binary32 screens on near-threshold inputs (tests/nearthr.py): pairs, rings and dumbbells whose distances are
eps or one reachable value either side of it, in frames where the screening copies round by far more than that gap,
and ICP data points on the bisector of two model points.  Every result is compared with an exact binary64 brute force
and with the oracle."""
import numpy as np
import pytest
import torch

import nearthr as T
from vtkcloudpoint_amd import _native as N
from vtkcloudpoint_amd import distributed as D

pytestmark = pytest.mark.gpu

FRAMES = [(m, f) for m in T.METRICS for f in T.frames(m)]
IDS = ["m%d-%s" % (m, f[0]) for m, f in FRAMES]


def _same(g, o, what):
    assert np.array_equal(g["labels"], o["labels"]), what + ": labels"
    assert np.array_equal(g["is_classed"], o["classed"]), what + ": classed"
    assert g["cf"] == o["cf"], what + ": cf"
    assert g["evals"] == o["evals"], what + ": evals"


def _check(ctx, oracle, c, eps, mp, metric, want_core, what):
    """vcp_dbscan with in_classed NULL and with an all-zero in_classed (same semantics, no neighbour lists), and for a
    2-D metric the same cloud passed with stride 3: is_core against the exact reference, the rest against the oracle."""
    o = oracle.dbscan(c, eps, mp, metric)
    assert np.array_equal(o["is_key"], want_core), what + ": oracle is_key"
    zero = np.zeros(len(c), np.uint8)
    runs = [(c, {}, "NULL in_classed"), (c, dict(in_classed=zero, labels=np.zeros(len(c), np.int32)), "zero in_classed")]
    if T.gd_of(metric) == 2:
        c3 = np.concatenate([c, np.random.default_rng(len(c)).uniform(-1e9, 1e9, (len(c), 1))], 1)
        runs.append((c3, {}, "stride 3"))
    for cc, kw, how in runs:
        g = ctx.dbscan(cc, eps, mp, metric, **kw)
        bad = np.nonzero(g["is_core"] != want_core)[0]
        assert bad.size == 0, "%s, %s: %d core flags differ from the exact reference, first %s" % (
            what, how, bad.size, bad[:5])
        _same(g, o, "%s, %s" % (what, how))


@pytest.mark.parametrize("metric,frame", FRAMES, ids=IDS)
def test_isolated_pairs_dbscan_and_kdist(vcp_ctx, oracle, metric, frame):
    d = T.frame_pairs(metric, frame, 7)
    c, eps = d["coords"], d["eps"]
    core = T.exact_core(c, metric, eps, 2)
    _check(vcp_ctx, oracle, c, eps, 2, metric, core, frame[0])
    # kdist with k = 2: an isolated pair member's 2nd distance (the 1st is itself) is its partner's, bit for bit
    kd, _ = vcp_ctx.kdist(c, 2, metric)
    want = T.dist(c[d["ia"]], c[d["ib"]], metric)
    assert kd[d["ia"]].tobytes() == want.tobytes() and kd[d["ib"]].tobytes() == want.tobytes()
    wa = T.dist(c[d["axis_a"]], c[d["axis_b"]], metric)
    assert (kd[d["axis_a"]] == wa).all() and (kd[d["axis_b"]] == wa).all()
    # the identity is_core == (kdist <= eps) at eps and one ulp either side
    for e in (eps, np.nextafter(eps, -np.inf), np.nextafter(eps, np.inf)):
        g = vcp_ctx.dbscan(c, float(e), 2, metric)
        assert np.array_equal(g["is_core"], (kd <= e).astype(np.uint8)), "identity at eps %r" % e


@pytest.mark.parametrize("metric", T.METRICS)
@pytest.mark.parametrize("fi", [1, 2, 5])
def test_rings_and_dumbbells(vcp_ctx, oracle, metric, fi):
    """Rings: one wrongly rejected inside point, or one wrongly accepted outside point, flips a probe's core flag;
    min_pts > 16 (the union and border kernels screen on their own) and hundreds of points per cell (beyond the LDS
    tile).  Dumbbells: one link pair decides whether two clumps are one cluster, one lone point whether it is a border
    point; min_pts 6 (neighbour lists) and 20."""
    frame = T.frames(metric)[fi]
    r = T.rings_cloud(metric, frame, 5 + fi)
    core = T.exact_core(r["coords"], metric, r["eps"], r["min_pts"])
    assert np.array_equal(core[r["probes"]].astype(bool), r["probe_core"])
    _check(vcp_ctx, oracle, r["coords"], r["eps"], r["min_pts"], metric, core, "rings " + frame[0])
    for mp in (6, 20):
        db = T.dumbbells_cloud(metric, frame, 9 + fi, min_pts=mp)
        c = db["coords"]
        core = T.exact_core(c, metric, db["eps"], mp)
        _check(vcp_ctx, oracle, c, db["eps"], mp, metric, core, "dumbbells mp %d %s" % (mp, frame[0]))
        lab = vcp_ctx.dbscan(c, db["eps"], mp, metric)["labels"]
        for a0, b0, b1, link, lone in db["bells"]:
            assert (lab[a0] == lab[b0]) == (link != T.OUT), "link pair class %d" % link
            assert (lab[b1] == lab[a0]) == (lone != T.OUT), "lone point class %d" % lone


@pytest.mark.parametrize("pic,small", [(150, True), (3000, False)])
def test_block_pipeline_pairs_across_blocks(vcp_ctx, oracle, pic, small):
    """dbscan_blocks vs the oracle with blocks of at most 1024 points (all-pairs kernel) and larger ones (grid engine);
    near-threshold pairs split between two blocks go through the noise pass and its 2 eps band."""
    keys = ("labels", "block_of", "order", "rows", "cols", "kept", "del_sum", "cluster_amount", "evals")
    for fi in (2, 3):
        frame = T.frames(T.L1_2D)[fi]
        d = T.frame_pairs(T.L1_2D, frame, 7)
        c, eps = d["coords"], d["eps"]
        o = oracle.block_pipeline(c, eps, 2, pic, 3)
        bo = o["block_of"]
        sizes = np.bincount(bo[bo >= 0])
        assert (sizes.max() <= 1024) == small, sizes.max()
        split = int((bo[d["ia"]] != bo[d["ib"]]).sum())
        if fi == 2:
            assert split >= 10, split
        g = vcp_ctx.dbscan_blocks(c, eps, 2, pic, 3)
        for k in keys:
            if isinstance(o[k], np.ndarray):
                assert np.array_equal(g[k], o[k]), "%s pic %d: %s" % (frame[0], pic, k)
            else:
                assert g[k] == o[k], "%s pic %d: %s %r != %r" % (frame[0], pic, k, g[k], o[k])


@pytest.fixture(scope="module")
def ctxs():
    cs = [N.Context(0) for _ in range(4)]
    yield cs
    for c in cs:
        c.close()


@pytest.mark.parametrize("metric", T.METRICS)
def test_slabs_cut_through_near_threshold_pairs(ctxs, oracle, metric):
    """exact_slabs_local with the cuts where the most near-threshold pairs straddle them (the m1 / m2 margins)."""
    for fi in (1, 2):
        d = T.frame_pairs(metric, T.frames(metric)[fi], 7)
        c, eps = d["coords"], d["eps"]
        order = np.argsort(c[:, 0], kind="stable")
        pts = c[order]
        pos = np.empty(len(c), np.int64)
        pos[order] = np.arange(len(c))
        lo = np.minimum(pos[d["ia"]], pos[d["ib"]])
        hi = np.maximum(pos[d["ia"]], pos[d["ib"]])
        n = len(pts)
        # straddle(k) = #(lo < k <= hi), best k in each quarter
        delta = np.zeros(n + 2, np.int64)
        np.add.at(delta, lo + 1, 1)
        np.add.at(delta, hi + 1, -1)
        st = np.cumsum(delta)[: n + 1]
        cuts = [0] + [int(q * n // 4 + np.argmax(st[q * n // 4:(q + 1) * n // 4])) for q in (1, 2, 3)] + [n]
        assert sum(int(st[k]) for k in cuts[1:-1]) >= 30
        parts = [torch.from_numpy(np.ascontiguousarray(pts[a:b])).cuda() for a, b in zip(cuts, cuts[1:])]
        res = D.exact_slabs_local(ctxs[:len(parts)], parts, eps, 2, metric, 0)
        lab = np.concatenate([x["labels"].cpu().numpy() for x in res])
        core = np.concatenate([x["is_core"].cpu().numpy() for x in res])
        ref = oracle.dbscan(pts, eps, 2, metric)
        assert np.array_equal(core, T.exact_core(pts, metric, eps, 2)), "frame %d core" % fi
        assert np.array_equal(lab, ref["labels"]) and np.array_equal(core, ref["is_key"]), "frame %d" % fi
        for x in res:
            assert x["cf"] == ref["cf"] and x["dist_evals"] == ref["evals"]


def test_dead_class_DB_signed_sum_at_eps(vcp_ctx, oracle):
    """VCP_SIGNED_SUM_2D (DB.cs: signed dx + dy) on pairs whose signed sum is eps or one reachable value either side,
    unquantised: the 1-D shortcut must see them within rounding of the threshold and hand them to the pair test."""
    rng = np.random.default_rng(31)
    for origin, eps in ((0.0, T.trunc_bits(0.7318)), (1e5, T.trunc_bits(0.7318)), (-7e5, T.trunc_bits(3.3))):
        n_pairs = 500
        a = origin + rng.uniform(0, 600 * eps, (n_pairs, 2))
        w = rng.uniform(0.2, 0.8, n_pairs)
        b = a + np.stack([w, 1.0 - w], 1) * eps
        # walk b's y by ulps: s(t) = (b.x - a.x) + (b.y - a.y), rising with b.y
        o0 = T.to_ord(a[:, 1])
        span = T.to_ord(a[:, 1] + 2.5 * eps) - o0

        def at(t):
            q = b.copy()
            q[:, 1] = T.from_ord(o0 + t)
            return q

        s = lambda q: (q[:, 0] - a[:, 0]) + (q[:, 1] - a[:, 1])
        zero = np.zeros(n_pairs, np.int64)
        t_le = T._last_true(lambda t: s(at(t)) <= eps, zero, span)
        t_lt = T._last_true(lambda t: s(at(t)) < eps, zero, span)
        cls = np.arange(n_pairs) % 3
        t = np.where(cls == 0, t_le, np.where(cls == 1, t_lt, t_le + 1))
        p = at(t)
        sv = s(p)
        assert (sv[cls == 2] > eps).all() and (sv[cls == 1] < eps).all() and (sv[cls == 0] <= eps).all()
        assert (sv == eps).sum() >= 50
        c = np.concatenate([p, a])[rng.permutation(2 * n_pairs)]
        for mp in (2, 3):
            o = oracle.db_literal(c, eps, mp)
            g = vcp_ctx.dbscan(c, eps, mp, N.SIGNED_SUM_2D)
            what = "origin %g mp %d" % (origin, mp)
            assert np.array_equal(g["labels"], o["labels"]), what
            assert np.array_equal(g["is_classed"], o["classed"]), what
            assert np.array_equal(g["is_core"], o["is_key"]), what
            assert g["cf"] == o["cluster_amount"] and g["evals"] == o["evals"], what


ICP_CASES = [(2, 6000, False, False), (2, 6000, True, False), (100, 6000, False, False), (100, 70000, False, False),
             (100, 6000, True, False), (512, 6000, False, False), (512, 70000, True, False), (513, 6000, False, False),
             (3000, 70000, True, False), (3000, 6000, False, True), (3000, 6000, True, True)]


@pytest.mark.parametrize("nm,nd,far,bad", ICP_CASES)
def test_icp_nearest_on_bisectors(vcp_ctx, oracle, nm, nd, far, bad):
    """icp_sums' nearest model point (R = identity) on data points whose two best binary64 squared distances are equal
    or 1-2 ulps apart: the scalar-cache path with 1..9 packed index bits, the grid (nm > 512), the LDS-tiled full scan
    (a non-finite model point), one-wave workgroups (nd <= 64 x 1024) and full ones."""
    t = T.icp_ties(nm, nd, 1000 + nm + nd + 7 * far + 3 * bad, far=far, bad_model_point=bad)
    m, q = t["model"], t["data"]
    ref = T.first_argmin(m, q)
    _, nn = vcp_ctx.icp_sums(m, q)
    bad_rows = np.nonzero(nn != ref)[0]
    assert bad_rows.size == 0, "%d of %d nearest indices differ, first rows %s kinds %s" % (
        bad_rows.size, nd, bad_rows[:5], t["kind"][bad_rows[:5]])
    assert np.array_equal(oracle.find_closest(m, q), ref)
