"""Similarity ICP on the MI355X (include/vcp.h, "similarity ICP").  One pass is held to the replayed reduction tree, all
18 columns, on every path and workgroup size, and to vcp_icp_sums_gated in the sixteen they share; whole runs to a
round-by-round restatement from one-pass calls and the host step; a closed ratio range to vcp_icp_gated and infinite
gates to vcp_icp_multistart, bit for bit; the behaviour scene in another unit to the conditions its numpy reference
meets (tests/icp_sim_ref.py); and global_similarity_icp's polish to that reference on the golden scaled scenes."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import icp_gated_ref as G
import icp_sim_ref as S
import icp_sums_ref as R
import register_ref as RR
import register_sim_ref as RS
from vtkcloudpoint_amd import _native as N
from vtkcloudpoint_amd.icp import gate_schedule, gated_icp, global_similarity_icp, similarity_icp

pytestmark = pytest.mark.gpu

INF = math.inf
ALL = 100000                    # max_landmarks: every source point is a landmark
TINY = 5e-324                   # the gate that drops every pair with a non-zero distance

# the small shapes (pairs at nm 1, 2, 512, grid at 513 and 600, tiled at 600), the switch to 256-wide workgroups and the
# second trip at the workgroup cap on the pairs path, and both on the other two paths
PASS_SHAPES = (R.SMALL_SHAPES + [("pairs", 100, nd) for nd in (1, 129, 65537, 524289)]
               + [("grid", 600, 8193), ("tiled", 600, 65537)])
PASS_FAMILIES = ("generic", "offset", "cancel", "lattice")
BRUTE_MAX = 70000               # beyond: the neighbours are vcp_icp_sums's (held to brute force by its own tests)


def _same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b))


def test_shapes_are_the_ones_meant():
    assert all(s in R.SHAPES for s in PASS_SHAPES[len(R.SMALL_SHAPES):])
    pl = [R.plan(nm, nd, path != "tiled") for path, nm, nd in PASS_SHAPES]
    assert {(p["path"], p["tb"]) for p in pl} == {(a, b) for a in ("pairs", "grid", "tiled") for b in (64, 256)}
    assert any(p["trips"] == 2 and p["nb"] == R.MAX_BLOCKS for p in pl)


@pytest.mark.parametrize("pose", R.POSES)
@pytest.mark.parametrize("family", PASS_FAMILIES)
@pytest.mark.parametrize("path,nm,nd", PASS_SHAPES)
def test_one_pass_is_the_replay(vcp_ctx, path, nm, nd, family, pose):
    model, data, Rm, T = R.case(path, nm, nd, family, pose)
    ungated, nn_u = vcp_ctx.icp_sums(model, data, Rm, T)
    if nd <= BRUTE_MAX:
        nn, _ = G.brute_nn(model, R.transform(data, Rm, T))
        assert _same(nn_u, nn)
    else:
        nn = nn_u.astype(np.int64)
    dist = np.sqrt(R.terms(model, data, Rm, T, nn)[:, 15])
    half = float(np.median(dist))
    for gate, what in ((INF, "none"), (half if half > 0 else 1.0, "half"), (TINY, "all")):
        want, kept, keep = S.sim_sums(model, data, Rm, T, nn, gate)
        if what == "none":
            assert kept == nd
        elif what == "all":
            assert kept == int((dist == 0).sum()) and kept <= nd // 100
        S18, k, g_nn, g_keep = vcp_ctx.icp_sums_sim(model, data, gate, Rm, T)
        assert k == kept, (what, k, kept)
        assert _same(g_keep, keep) and _same(g_nn, nn), what
        assert S18.tobytes() == want.tobytes(), (what, S18, want)        # every bit: no sum is ever -0.0
        # the sixteen shared columns and every other output are the gated pass's
        S16, k16, nn16, keep16 = vcp_ctx.icp_sums_gated(model, data, gate, Rm, T)
        assert S18[:16].tobytes() == S16.tobytes() and k16 == k and _same(nn16, g_nn) and _same(keep16, g_keep), what
        if what == "none":
            assert _same(S18[:16], ungated)
        if what == "all" and kept == 0:
            assert not S18.any() and not np.signbit(S18).any()
        # the outputs that may be NULL change nothing
        S2, k2, _, _ = vcp_ctx.icp_sums_sim(model, data, gate, Rm, T, want_nn=False, want_keep=False)
        assert S2.tobytes() == S18.tobytes() and k2 == k


def test_a_nan_pair_is_kept_and_poisons_the_new_columns(vcp_ctx):
    model, data, Rm, T = R.case("pairs", 100, 129, "generic")
    data = data.copy()
    data[7, 1] = math.nan
    S18, kept, _, keep = vcp_ctx.icp_sums_sim(model, data, 1e-3, Rm, T)
    assert keep[7] == 1 and kept >= 1
    assert np.isnan(S18[16]) and np.isnan(S18[15]) and np.isnan(S18[0])
    assert np.isfinite(S18[17])              # its nearest model point is a model point


# ---- whole runs -------------------------------------------------------------------------------------------------------
def _three_poses(sc):
    """The scene's start and two more: rotated a little either way about the start's own image of the origin."""
    Rs, Ts = [], []
    for da, dt in ((0.0, (0.0, 0.0, 0.0)), (0.02, (0.05, -0.02, 0.0)), (-0.03, (-0.04, 0.06, 0.0))):
        Rs.append(G.rz(da) @ sc["R0"])
        Ts.append(G.rz(da) @ sc["T0"] + np.array(dt))
    return np.ascontiguousarray(Rs), np.ascontiguousarray(Ts)


RUN_ROUNDS = (1, 2, 9, 17)


@pytest.mark.parametrize("err,rng", [(0.02, S.RATIO_RANGE), (0.05, (0.99, 1.01))])
@pytest.mark.parametrize("nt,ntrue,nclutter", G.SIZES[:2])
def test_whole_runs_are_the_replay(vcp_ctx, nt, ntrue, nclutter, err, rng):
    sc = S.scaled_scene(nt, ntrue, nclutter, G.SEEDS[nt], err)
    src, tgt = sc["centers"], sc["truths"]
    Rs, Ts = _three_poses(sc)
    gates = G.schedule()
    tr = [S.replay_run(vcp_ctx, N, tgt, src, Rs[h], Ts[h], gates, max(RUN_ROUNDS), rng) for h in range(3)]
    for r in RUN_ROUNDS:
        g = vcp_ctx.icp_sim(src, tgt, gates, rng, Rs, Ts, r, ALL, G.MIN_PAIRS, 0.1)
        for h in range(3):
            one = vcp_ctx.icp_sim(src, tgt, gates, rng, Rs[h:h + 1], Ts[h:h + 1], r, ALL, G.MIN_PAIRS, 0.1)
            want = tr[h][r - 1]
            for res, i in ((g, h), (one, 0)):
                assert res["M_all"][i].tobytes() == want["M"].tobytes(), ("rounds", r, "pose", h)
                assert res["mean_dist"][i] == want["mean_dist"]
                assert res["kept"][i] == want["kept"] and res["starved"][i] == want["starved"]
                assert res["ratio"][i] == want["ratio"] and res["unscaled"][i] == want["unscaled"]
            assert one["inliers"][0] == g["inliers"][h] and _same(one["M"], one["M_all"][0])
    last = tr[0][-1]
    assert last["starved"] == 0 and last["unscaled"] == 0 and 0 < last["kept"] < len(src)
    if rng == S.RATIO_RANGE:
        assert rng[0] < last["ratio"] < rng[1] and abs(last["ratio"] * (1.0 + err) - 1.0) < 1e-3
    else:
        assert last["ratio"] == rng[0] and tr[0][0]["ratio"] == rng[0]     # clamped from the first round on


@pytest.mark.parametrize("nt,ntrue,nclutter", [G.SIZES[0], G.SIZES[2]])
def test_closed_range_is_the_gated_call(vcp_ctx, nt, ntrue, nclutter):
    sc = S.scaled_scene(nt, ntrue, nclutter, G.SEEDS[nt], 0.02)
    src, tgt = sc["centers"] * S.K_UNIT, sc["truths"]      # the default starts are rotations: the scene's own unit
    for gates, ml, ungated in ((G.schedule(), ALL, False), ([1e-9, 2.0, 1.0, 0.5, 0.2], 200, False), ([INF], ALL, True)):
        a = vcp_ctx.icp_gated(src, tgt, gates, 36, None, 12, ml, G.MIN_PAIRS, 0.1)
        b = vcp_ctx.icp_sim(src, tgt, gates, (1.0, 1.0), 36, None, 12, ml, G.MIN_PAIRS, 0.1)
        for k in ("M", "M_all", "mean_dist", "inliers", "kept", "starved"):
            assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), k
        assert a["best"] == b["best"]
        assert (b["ratio"] == 1.0).all()
        if ungated:
            m = vcp_ctx.icp_multistart(src, tgt, 36, None, 12, ml, 0.1)
            for k in ("M", "M_all", "mean_dist", "inliers"):
                assert np.asarray(m[k]).tobytes() == np.asarray(b[k]).tobytes(), k
            assert m["best"] == b["best"] and (b["kept"] == len(src)).all() and (b["starved"] == 0).all()
    assert len(set(a["inliers"].tolist())) > 1             # the 36 poses do differ


# ---- behaviour --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("err", S.START_ERRORS)
@pytest.mark.parametrize("nt,ntrue,nclutter", G.SIZES)
def test_behaviour_on_the_device(vcp_ctx, nt, ntrue, nclutter, err):
    """The conditions of tests/test_icp_sim.py::test_reference_behaviour, same seeds, through similarity_icp."""
    sc = S.scaled_scene(nt, ntrue, nclutter, G.SEEDS[nt], err)
    R0, T0 = sc["R0"].reshape(1, 3, 3), sc["T0"].reshape(1, 3)
    g = similarity_icp(sc["centers"], sc["truths"], G.schedule(), S.RATIO_RANGE, n_angles=R0, init_T=T0,
                       max_iter=G.ROUNDS, max_landmarks=ALL, min_pairs=G.MIN_PAIRS, inlier_dist=0.1, ctx=vcp_ctx)
    M = g["M"]
    within, perr = G.conditions(sc, M[:3, :3], M[:3, 3])
    k = S.linear_scale(M[:3, :3])
    print("similarity: start error", err, "within", within, "pose error", perr, "k", k, "ratio", g["ratio"][0], "kept",
          g["kept"][0], "starved", g["starved"][0], "unscaled", g["unscaled"][0])
    assert within == 1.0
    assert perr < 0.01
    assert abs(k / S.K_UNIT - 1.0) < 1e-3
    assert g["kept"][0] == ntrue and g["inliers"][0] == ntrue and g["unscaled"][0] == 0
    assert abs(k / (S.K_UNIT * (1.0 + err) * g["ratio"][0]) - 1.0) < 1e-12
    if err == 0.02:
        u = gated_icp(sc["centers"], sc["truths"], G.schedule(), n_angles=R0, init_T=T0, max_iter=G.ROUNDS,
                      max_landmarks=ALL, min_pairs=G.MIN_PAIRS, inlier_dist=0.1, ctx=vcp_ctx)
        within_u, perr_u = G.conditions(sc, u["M"][:3, :3], u["M"][:3, 3])
        print("rigid from the same start: within", within_u, "pose error", perr_u)
        assert within_u < 0.5
    if err == 0.05:
        c = similarity_icp(sc["centers"], sc["truths"], G.schedule(), (0.99, 1.01), n_angles=R0, init_T=T0,
                           max_iter=G.ROUNDS, max_landmarks=ALL, min_pairs=G.MIN_PAIRS, inlier_dist=0.1, ctx=vcp_ctx)
        assert c["ratio"][0] == 0.99


PLANTED = {"half": 98, "third": 49}
GLOBAL_RANGE = (0.95, 1.05)


@pytest.mark.parametrize("name", sorted(RR.SCENES))
def test_global_similarity_icp(vcp_ctx, name):
    """register_similarity, then ONE vcp_icp_sim call from the registered similarities: every planted centroid ends on
    its truth, and the scale is no farther from the planted 2.5 than twice what the numpy reference loop reaches from
    the winning start (the factor 2 is for the different order of the sums).
    Measured on an MI355X: see DESIGN.md section 22."""
    assert sorted(RR.SCENES) == sorted(PLANTED)
    sc, bases = RS.scaled_scene(name)
    assert sc["planted"] == PLANTED[name]
    g0, g1, gr, rounds = RR.POLISH
    gates = gate_schedule(g0, g1, gr)
    q = global_similarity_icp(sc["source"], sc["truths"], bases, RS.RANGE, RR.INLIER, gates, GLOBAL_RANGE,
                              max_iter=rounds, ctx=vcp_ctx)
    ref = RS.golden(name)
    RS.same(q["registration"], ref)
    b = q["bases_used"][q["best"]]
    assert q["scale_registration"] == ref["scale"][b]
    M0 = ref["M_all"][b]
    lm = G.landmarks(sc["source"], 200)
    want = S.ref_icp(lm, sc["truths"], M0[:3, :3], M0[:3, 3], gates, rounds, GLOBAL_RANGE)
    e_ref, e_dev = abs(S.linear_scale(want["R"]) - RS.SCALE), abs(q["scale"] - RS.SCALE)
    print(name, "inliers", q["inliers"][q["best"]], "scale", q["scale"], "|scale - 2.5|", e_dev, "reference loop", e_ref,
          "registered", q["scale_registration"], "ratio", q["ratio"][q["best"]])
    assert q["inliers"][q["best"]] == PLANTED[name]
    assert RR.inliers_of(sc, q["M"][:3, :3], q["M"][:3, 3]) == q["inliers"][q["best"]]
    assert e_dev <= 2.0 * e_ref
    assert "ratio" in q and "unscaled" in q and q["scale"] == S.linear_scale(q["M"][:3, :3])


def test_undetermined_scale_counts_and_passes(vcp_ctx):
    """Two coincident truths as the whole model: every pair lands on one place, vY is exactly zero in every round."""
    tgt = np.array([[1.0, 2.0, 0.0], [1.0, 2.0, 0.0]])
    src = np.random.default_rng(5).uniform(-1.0, 1.0, (50, 3)) * (1, 1, 0)
    g = vcp_ctx.icp_sim(src, tgt, [INF], (0.5, 2.0), 2, None, 7, ALL, 3, 0.1)
    assert (g["unscaled"] == 7).all() and (g["ratio"] == 1.0).all() and (g["starved"] == 0).all()
    r = vcp_ctx.icp_gated(src, tgt, [INF], 2, None, 7, ALL, 3, 0.1)
    assert g["M_all"].tobytes() == r["M_all"].tobytes()      # k_used = 1.0: the rigid rounds


# ---- errors and determinism -------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _cloud():
    rng = np.random.default_rng(11)
    tgt = np.zeros((300, 3))
    tgt[:, :2] = rng.uniform(-10.0, 10.0, (300, 2))
    x = tgt[rng.integers(0, 300, 400)].copy()
    x[:, :2] += 0.05 * rng.normal(size=(400, 2))
    src = ((x - np.array([0.7, -0.4, 0.0])) @ G.rz(0.1)) / 1.03
    src[:, 2] = 0.0
    return np.ascontiguousarray(tgt), np.ascontiguousarray(src)


def test_errors_leave_the_outputs_untouched(vcp_ctx):
    tgt, src = _cloud()
    z = np.zeros((0, 3))

    def code(f, *a, **k):
        with pytest.raises(N.VcpError) as e:
            f(*a, **k)
        return e.value.code

    si, ss = vcp_ctx.icp_sim, vcp_ctx.icp_sums_sim
    ok = (0.9, 1.1)
    for bad in ((math.nan, 1.1), (0.0, 1.1), (-0.5, 1.1), (0.9, math.nan), (0.9, INF), (1.0, 0.99), (1.01, 1.1), (0.5, 0.9),
                (INF, INF)):
        assert code(si, src, tgt, [1.0], bad) == -1, bad
    for bad in (0.0, -1.0, math.nan, -INF):
        assert code(ss, tgt, src, bad) == -1
        assert code(si, src, tgt, [1.0, bad], ok) == -1
    assert code(si, src, tgt, [], ok) == -1 and code(si, src, tgt, [1.0], ok, min_pairs=0) == -1
    assert code(si, z, tgt, [1.0], ok) == -2 and code(si, src, z, [1.0], ok) == -2
    assert code(si, src, tgt, [1.0], ok, 0) == -1 and code(si, src, tgt, [1.0], ok, 4097) == -8
    assert code(si, src, tgt, [1.0], ok, max_iter=0) == -1 and code(si, src, tgt, [1.0], ok, max_landmarks=0) == -1
    assert code(si, src, tgt, [1.0], ok, inlier_dist=0.0) == -1
    assert code(ss, z, src, 1.0) == -2 and code(ss, tgt, z, 1.0) == -1
    # a failed Horn solve in a round that is not starved fails the call; starved, the same pose passes
    bad_src = src.copy()
    bad_src[4, 0] = math.nan
    Rs, Tz = np.stack([np.eye(3), np.eye(3)]), np.zeros((2, 3))
    assert code(si, bad_src, tgt, [INF], ok, Rs, Tz, 3) == -1
    g = si(bad_src, tgt, [1e-9], ok, Rs, Tz, 3)
    assert (g["starved"] == 3).all() and (g["kept"] == 1).all() and (g["ratio"] == 1.0).all()
    # nothing is written on an error (raw calls: every output pre-filled)
    s, t = np.ascontiguousarray(src), np.ascontiguousarray(tgt)

    def raw(gates, n_gates, min_pairs, lo, hi, n_poses=2, outs=True):
        gates = np.array(gates)
        o = dict(M=np.full(16, 7.0), Ma=np.full(32, 7.0), md=np.full(2, 7.0), inl=np.full(2, 7, np.int32),
                 st=np.full(2, 7, np.int32), kept=np.full(2, 7, np.int64), ratio=np.full(2, 7.0),
                 un=np.full(2, 7, np.int32))
        best = C.c_int32(7)
        p = (lambda a: N._ptr(a)) if outs else (lambda a: None)
        rc = N.lib().vcp_icp_sim(vcp_ctx._h, N._ptr(s), C.c_int64(len(s)), N._ptr(t), C.c_int64(len(t)),
                                 C.c_int32(n_poses), None, None, 5, 200, N._ptr(gates), C.c_int32(n_gates),
                                 C.c_int32(min_pairs), C.c_double(lo), C.c_double(hi), C.c_double(1.0), N._ptr(o["M"]),
                                 C.byref(best), p(o["Ma"]), p(o["md"]), p(o["inl"]), p(o["kept"]), p(o["st"]),
                                 p(o["ratio"]), p(o["un"]))
        return rc, best.value, o

    for a in (([math.nan], 1, 3, 0.9, 1.1), ([1.0], 0, 3, 0.9, 1.1), ([1.0], 1, 0, 0.9, 1.1), ([1.0], 1, 3, 1.01, 1.1),
              ([1.0], 1, 3, 0.9, INF), ([1.0], 1, 3, math.nan, 1.1), ([1.0], 1, 3, 0.0, 1.1), ([1.0], 1, 3, 1.0, 0.5)):
        rc, best, o = raw(*a)
        assert rc == -1 and best == 7 and all((v == 7).all() for v in o.values()), a
    S18, nn, keep = np.full(18, 7.0), np.full(len(s), 7, np.int32), np.full(len(s), 7, np.uint8)
    k = C.c_int64(7)
    rc = N.lib().vcp_icp_sums_sim(vcp_ctx._h, N._ptr(t), C.c_int64(len(t)), N._ptr(s), C.c_int64(len(s)), None, None,
                                  C.c_double(0.0), N._ptr(S18), C.byref(k), N._ptr(nn), N._ptr(keep))
    assert rc == -1 and k.value == 7 and (S18 == 7).all() and (nn == 7).all() and (keep == 7).all()
    # every optional output may be NULL, and the context stays usable
    rc, best, o = raw([1.0, 0.5], 2, 3, 0.9, 1.1, outs=False)
    assert rc == 0 and best in (0, 1)
    assert o["M"].reshape(4, 4).tobytes() == si(src, tgt, [1.0, 0.5], ok, 2, None, 5, 200, 3, 1.0)["M"].tobytes()


def test_determinism_and_the_calls_between(vcp_ctx):
    tgt, src = _cloud()
    gates = [2.0, 1.0, 0.5, 0.2]

    def call():
        return vcp_ctx.icp_sim(src, tgt, gates, (0.9, 1.1), 8, None, 12, 200, 3, 0.2)

    a = call()
    b = call()
    r = vcp_ctx.icp_gated(src, tgt, gates, 8, None, 12, 200, 3, 0.2)
    c = call()
    r2 = vcp_ctx.icp_gated(src, tgt, gates, 8, None, 12, 200, 3, 0.2)
    for k in a:
        assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() == np.asarray(c[k]).tobytes(), k
    for k in r:
        assert np.asarray(r[k]).tobytes() == np.asarray(r2[k]).tobytes(), k
    assert a["M_all"].tobytes() != r["M_all"].tobytes()     # the source is 3 % small: the similarity rounds do act
    assert 1.02 < a["ratio"][a["best"]] < 1.04
    # a one-pass call between changes nothing either
    vcp_ctx.icp_sums_sim(tgt, src, 1.0)
    d = call()
    assert d["M_all"].tobytes() == a["M_all"].tobytes() and d["ratio"].tobytes() == a["ratio"].tobytes()


def test_timing_phases(vcp_ctx):
    tgt, src = _cloud()
    vcp_ctx.timing_enable(True)
    try:
        vcp_ctx.icp_sim(src, tgt, [1.0], (0.9, 1.1), 2, None, 3, 200, 3, 0.2)
        assert [p[0] for p in vcp_ctx.timing()] == ["icps_rounds", "icps_score"]
    finally:
        vcp_ctx.timing_enable(False)
