"""The near-threshold generator (tests/nearthr.py) on the CPU: its clouds are what they claim to be, a naive binary32
decision is wrong on hundreds of their pairs in each direction, and the oracle agrees with the exact binary64
reference built here independently of it."""
import numpy as np
import pytest

import nearthr as T

FRAMES = [(m, f) for m in T.METRICS for f in T.frames(m)]
IDS = ["m%d-%s" % (m, f[0]) for m, f in FRAMES]


@pytest.mark.parametrize("metric,frame", FRAMES, ids=IDS)
def test_pairs_are_what_they_claim_and_defeat_a_naive_binary32_screen(metric, frame):
    d = T.frame_pairs(metric, frame, 7)
    c, eps = d["coords"], d["eps"]
    a, b = c[d["ia"]], c[d["ib"]]
    dd = T.dist(a, b, metric)
    cls = d["cls"]
    assert (dd[cls == T.AT] == eps).all() and (dd[cls == T.IN] < eps).all() and (dd[cls == T.OUT] > eps).all()
    # IN / OUT are the reachable values next to eps: one more ulp of the walked coordinate crosses it
    assert (cls == T.IN).sum() >= 500 and (cls == T.OUT).sum() >= 400
    if metric == T.L1_2D:
        assert (cls == T.AT).sum() >= 400
    # the distance form against the threshold the library compares with
    assert ((T.form(a, b, metric) <= d["thr"]) == (dd <= eps)).all()
    ax, bx = c[d["axis_a"]], c[d["axis_b"]]
    assert len(ax) >= 100
    assert ((bx[:, 0] - ax[:, 0]) == eps).all() and (bx[:, 1:] == ax[:, 1:]).all()
    assert (T.dist(ax, bx, metric) == eps).all()
    # the grid origin is the bounding-box minimum: the frame's corner
    mn, scale, E = T.screen_view(c, metric)
    assert (mn == d["frame"].origin).all()
    inside_rejected, outside_accepted = T.power(a, b, metric, mn, scale, d["thr"])
    assert inside_rejected >= 200 and outside_accepted >= 200, (inside_rejected, outside_accepted)
    # the selection kept pairs whose binary32 value is off by about the copies' rounding (u E), not less
    assert d["max_err"] >= 1.0, d["max_err"]
    if frame[3] != 1.0:
        raw = float(np.abs(c.max(0) - c.min(0)).max())
        assert not (1e-20 <= raw <= 1e30) and scale != 1.0
    else:
        assert scale == 1.0


@pytest.mark.parametrize("metric", T.METRICS)
def test_frames_straddle_the_accept_switch(metric):
    for name, origin, ratio, scale in T.frames(metric):
        fr = T.Frame(metric, name, origin, ratio, scale)
        s = T.grid_scale(fr.E)
        k = s if metric == T.L1_2D else s * s
        on = T.accept_side_on(metric, fr.thr * k, fr.E * s)
        assert on == (name != "above_switch"), name


def test_l2_threshold_port():
    rng = np.random.default_rng(1)
    for eps in list(rng.uniform(1e-3, 1e3, 200)) + [1.0, 0.1, 3.0, 1e-25 * 0.7, 1e35 * 0.7]:
        t = T.l2_threshold(eps)
        assert np.sqrt(t) <= eps < np.sqrt(np.nextafter(t, np.inf))


def test_ordinal_walk_round_trips():
    x = np.array([-3.5, -1e-300, -0.0, 0.0, 5e-324, 1.0, 7e5])
    o = T.to_ord(x)
    assert (np.diff(o) >= 0).all()
    nz = x != 0.0   # (-0.0 and 0.0 share a key)
    assert (T.from_ord(o + 1)[nz] == np.nextafter(x, np.inf)[nz]).all()
    assert (T.from_ord(o) == x).all()


def test_exact_reference_on_a_brute_force():
    for metric in T.METRICS:
        d = T.pairs_cloud(metric, T.frames(metric)[2], 11, n_pairs=200, n_axis=20)
        c, eps = d["coords"], d["eps"]
        p = np.sort(T.exact_pairs(c, metric, eps), 1)
        i, j = np.triu_indices(len(c), 1)
        want = np.stack([i, j], 1)[T.dist(c[i], c[j], metric) <= eps]
        got = p[np.lexsort((p[:, 1], p[:, 0]))]
        assert np.array_equal(got, want)


@pytest.mark.parametrize("metric", T.METRICS)
def test_oracle_matches_the_exact_reference(oracle, metric):
    for fi, frame in enumerate(T.frames(metric)):
        d = T.frame_pairs(metric, frame, 7)
        c, eps = d["coords"], d["eps"]
        o = oracle.dbscan(c, eps, 2, metric)
        core = T.exact_core(c, metric, eps, 2)
        assert np.array_equal(o["is_key"], core), frame[0]
        # every member of an isolated pair is core exactly when the pair is within eps; one cluster per such pair
        inside = d["cls"] != T.OUT
        assert (core[d["ia"]] == inside).all() and (core[d["ib"]] == inside).all()
        lab = o["labels"]
        assert (lab[d["ia"]][inside] == lab[d["ib"]][inside]).all() and (lab[d["ia"]][inside] > 0).all()
        assert (lab[d["ia"]][~inside] == 0).all()


@pytest.mark.parametrize("metric", T.METRICS)
def test_oracle_follows_rings_and_dumbbells(oracle, metric):
    frame = T.frames(metric)[1]
    r = T.rings_cloud(metric, frame, 5)
    c = r["coords"]
    core = T.exact_core(c, metric, r["eps"], r["min_pts"])
    assert np.array_equal(core[r["probes"]].astype(bool), r["probe_core"])
    assert core.sum() == r["probe_core"].sum()    # nothing else is core
    o = oracle.dbscan(c, r["eps"], r["min_pts"], metric)
    assert np.array_equal(o["is_key"], core)
    for mp in (6, 20):
        db = T.dumbbells_cloud(metric, frame, 9, min_pts=mp)
        c = db["coords"]
        o = oracle.dbscan(c, db["eps"], mp, metric)
        assert np.array_equal(o["is_key"], T.exact_core(c, metric, db["eps"], mp))
        lab = o["labels"]
        for a0, b0, b1, link, lone in db["bells"]:
            assert (o["is_key"][a0:b1] == 1).all() and o["is_key"][b1] == 0
            assert len(set(lab[a0:b0])) == 1 and len(set(lab[b0:b1])) == 1 and lab[a0] > 0
            assert (lab[a0] == lab[b0]) == (link != T.OUT)
            assert (lab[b1] == lab[a0]) == (lone != T.OUT) and (lab[b1] == 0) == (lone == T.OUT)


@pytest.mark.parametrize("nm,far", [(2, False), (100, False), (100, True), (512, False), (3000, True)])
def test_icp_ties_are_ties(oracle, nm, far):
    t = T.icp_ties(nm, 3000, 21 + nm, far=far)
    m, q = t["model"], t["data"]
    dj, dk = T.d2(q, m[t["j"]]), T.d2(q, m[t["k"]])
    gap = np.abs(T.to_ord(dj) - T.to_ord(dk))
    assert (gap <= 2).all()
    for kind in (0, 1, 2):
        assert (t["kind"] == kind).sum() >= 200, kind
    ref = T.first_argmin(m, q)
    assert set(np.unique(ref)) <= set(np.concatenate([t["j"], t["k"]]))
    assert np.array_equal(ref, np.where(t["kind"] == 1, np.maximum(t["j"], t["k"]),
                                        np.where(t["kind"] == 0, np.minimum(t["j"], t["k"]),
                                                 np.where(dj < dk, t["j"], t["k"]))))
    assert np.array_equal(oracle.find_closest(m, q), ref)
    # the binary32 scores of the kernel's screen (fused, relative to the model's bounding-box centre) order many of
    # them the other way round
    sj, sk = T.score32(m, q, t["j"]), T.score32(m, q, t["k"])
    wrong = ((sj < sk) & (ref == t["k"])) | ((sk < sj) & (ref == t["j"]))
    assert wrong.sum() >= (200 if nm > 2 else 20), wrong.sum()
