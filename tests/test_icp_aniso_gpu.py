"""Anisotropic ICP on the MI355X (include/vcp.h, "anisotropic ICP").  One pass is held to the replayed reduction tree, all
18 columns, on every path and workgroup size, and to vcp_icp_sums_gated under the identity pose; whole runs to a
round-by-round restatement from one-pass calls and the host step, which sets the pose; closed ratios to scales that never
move; and the behaviour scene in two units to the conditions its numpy reference meets (tests/icp_aniso_ref.py)."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import icp_aniso_ref as A
import icp_gated_ref as G
import icp_sums_ref as R
from vtkcloudpoint_amd import _native as N
from vtkcloudpoint_amd.icp import anisotropic_icp, gated_icp, rotations_about_z, similarity_icp

pytestmark = pytest.mark.gpu

INF = math.inf
ALL = 100000                    # max_landmarks: every source point is a landmark
TINY = 5e-324                   # the gate that drops every pair with a non-zero distance

# the small shapes (pairs at nm 1, 2, 512, grid at 513 and 600, tiled at 600 with a non-finite model point), nd 1 and 129,
# and the switch to 256-wide workgroups on each path
PASS_SHAPES = (R.SMALL_SHAPES + [("pairs", 100, nd) for nd in (1, 129, 66000)]
               + [("grid", 600, 8193), ("tiled", 600, 65537)])
PASS_FAMILIES = ("generic", "offset", "cancel", "lattice")
BRUTE_MAX = 70000
STRETCH = np.array([1.1, 0.9, 1.0])     # the pass's pose is any finite matrix: the case's rotation with its columns scaled


def _same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b))


def test_shapes_are_the_ones_meant():
    pl = [R.plan(nm, nd, path != "tiled") for path, nm, nd in PASS_SHAPES]
    assert {(p["path"], p["tb"]) for p in pl} == {(a, b) for a in ("pairs", "grid", "tiled") for b in (64, 256)}
    assert {nm for path, nm, _ in PASS_SHAPES if path == "pairs"} == {1, 2, 100, 512}


@pytest.mark.parametrize("pose", R.POSES)
@pytest.mark.parametrize("family", PASS_FAMILIES)
@pytest.mark.parametrize("path,nm,nd", PASS_SHAPES)
def test_one_pass_is_the_replay(vcp_ctx, path, nm, nd, family, pose):
    model, data, Rm, T = R.case(path, nm, nd, family, pose)
    Am = None if Rm is None else np.ascontiguousarray(Rm * STRETCH)
    _, nn_u = vcp_ctx.icp_sums(model, data, Am, T)
    if nd <= BRUTE_MAX:
        nn, _ = G.brute_nn(model, R.transform(data, Am, T))
        assert _same(nn_u, nn)
    else:
        nn = nn_u.astype(np.int64)
    dist = np.sqrt(R.terms(model, data, Am, T, nn)[:, 15])
    half = float(np.median(dist))
    for gate, what in ((INF, "none"), (half if half > 0 else 1.0, "half"), (TINY, "all")):
        want, kept, keep = A.aniso_sums(model, data, Am, T, nn, gate)
        if what == "none":
            assert kept == nd
        elif what == "all":
            assert kept == int((dist == 0).sum()) and kept <= nd // 100
        elif nd >= 100 and half > 0:
            assert nd // 4 <= kept <= 3 * nd // 4
        S18, k, g_nn, g_keep = vcp_ctx.icp_sums_aniso(model, data, gate, Am, T)
        assert k == kept, (what, k, kept)
        assert _same(g_keep, keep) and _same(g_nn, nn), what
        assert S18.tobytes() == want.tobytes(), (what, S18, want)        # every bit: no sum is ever -0.0
        # the pair, the gate and every output but the d-side columns are the gated pass's under the same pose
        S16, k16, nn16, keep16 = vcp_ctx.icp_sums_gated(model, data, gate, Am, T)
        assert k16 == k and _same(nn16, g_nn) and _same(keep16, g_keep), what
        assert S18[3:6].tobytes() == S16[3:6].tobytes() and S18[15:16].tobytes() == S16[15:16].tobytes()
        if pose == "none":               # identity pose, finite data: p is d, the sixteen shared columns bit for bit
            assert S18[:16].tobytes() == S16.tobytes(), what
        if what == "all" and kept == 0:
            assert not S18.any() and not np.signbit(S18).any()
        # the outputs that may be NULL change nothing
        S2, k2, _, _ = vcp_ctx.icp_sums_aniso(model, data, gate, Am, T, want_nn=False, want_keep=False)
        assert S2.tobytes() == S18.tobytes() and k2 == k


def test_a_nan_row_is_kept_and_poisons_its_columns(vcp_ctx):
    model, data, Rm, T = R.case("pairs", 100, 129, "generic")
    data = data.copy()
    data[7, 1] = math.nan
    S18, kept, _, keep = vcp_ctx.icp_sums_aniso(model, data, 1e-3, Rm, T)
    assert keep[7] == 1 and kept >= 1
    assert np.isnan(S18[1]) and np.isnan(S18[15]) and np.isnan(S18[17]) and np.isnan(S18[9:12]).all()
    assert np.isfinite(S18[0]) and np.isfinite(S18[16]) and np.isfinite(S18[6:9]).all()   # d0 is a number: raw, not p
    assert np.isfinite(S18[3:6]).all()       # its nearest model point is a model point


# ---- whole runs -------------------------------------------------------------------------------------------------------
def _three_poses(sc):
    """The scene's start and two more: rotated a little either way, shifted, with other start scales."""
    Rs, Ts, ss = [], [], []
    for da, dt, ds in ((0.0, (0.0, 0.0, 0.0), (1.0, 1.0)), (0.02, (0.05, -0.02, 0.0), (0.99, 1.01)),
                       (-0.03, (-0.04, 0.06, 0.0), (1.02, 1.0))):
        Rs.append(G.rz(da) @ sc["R0"])
        Ts.append(G.rz(da) @ sc["T0"] + np.array(dt))
        ss.append(sc["s0"] * np.array(ds))
    return np.ascontiguousarray(Rs), np.ascontiguousarray(Ts), np.ascontiguousarray(ss)


RUN_ROUNDS = (1, 2, 9, 17)
SMALLEST = G.SIZES[0]


@pytest.mark.parametrize("err,ratio", [(A.WRONG_STARTS[0], A.RATIO), (A.WRONG_STARTS[1], (0.99, 1.01))])
def test_whole_runs_are_the_replay(vcp_ctx, err, ratio):
    nt, ntrue, nclutter = SMALLEST
    sc = A.aniso_scene(nt, ntrue, nclutter, G.SEEDS[nt], err)
    src, tgt = sc["centers"], sc["truths"]
    Rs, Ts, ss = _three_poses(sc)
    gates = G.schedule()
    tr = [A.replay_run(vcp_ctx, N, tgt, src, Rs[h], ss[h], Ts[h], gates, max(RUN_ROUNDS), ratio) for h in range(3)]
    for r in RUN_ROUNDS:
        g = vcp_ctx.icp_aniso(src, tgt, gates, ratio, Rs, Ts, ss, r, ALL, G.MIN_PAIRS, 0.1)
        again = vcp_ctx.icp_aniso(src, tgt, gates, ratio, Rs, Ts, ss, r, ALL, G.MIN_PAIRS, 0.1)
        for k in g:
            assert np.asarray(g[k]).tobytes() == np.asarray(again[k]).tobytes(), k       # two calls, identical bits
        for h in range(3):
            one = vcp_ctx.icp_aniso(src, tgt, gates, ratio, Rs[h:h + 1], Ts[h:h + 1], ss[h:h + 1], r, ALL, G.MIN_PAIRS, 0.1)
            want = tr[h][r - 1]
            for res, i in ((g, h), (one, 0)):          # in the batch and alone: a pose's bits are its own
                assert res["M_all"][i].tobytes() == want["M"].tobytes(), ("rounds", r, "pose", h)
                assert res["mean_dist"][i] == want["mean_dist"]
                assert res["kept"][i] == want["kept"] and res["starved"][i] == want["starved"]
                assert res["scale"][i].tolist() == want["scale"] and res["unscaled"][i].tolist() == want["unscaled"]
            assert one["inliers"][0] == g["inliers"][h] and _same(one["M"], one["M_all"][0])
    last = tr[0][-1]
    assert last["starved"] == 0 and last["unscaled"] == [0, 0] and 0 < last["kept"] < len(src)
    if ratio == A.RATIO:
        assert np.allclose(last["scale"], A.K_XY, rtol=2e-3)
    else:                                              # held on the bound from the first round on
        assert tr[0][0]["scale"][0] == ratio[0] * ss[0][0] and last["scale"][0] == ratio[0] * ss[0][0]


def test_a_starved_round_leaves_pose_and_scales_alone(vcp_ctx):
    nt, ntrue, nclutter = SMALLEST
    sc = A.aniso_scene(nt, ntrue, nclutter, G.SEEDS[nt], A.WRONG_STARTS[0])
    Rs, Ts, ss = _three_poses(sc)
    g = vcp_ctx.icp_aniso(sc["centers"], sc["truths"], [1e-9], A.RATIO, Rs, Ts, ss, 5, ALL, G.MIN_PAIRS, 0.1)
    assert (g["starved"] == 5).all() and (g["kept"] == 0).all() and (g["unscaled"] == 0).all()
    assert g["scale"].tobytes() == ss.tobytes()
    for h in range(3):
        want = np.eye(4)
        want[:3, :3] = np.array(A.pose_matrix(Rs[h].reshape(9).tolist(), ss[h].tolist())).reshape(3, 3)
        want[:3, 3] = Ts[h]
        assert g["M_all"][h].tobytes() == want.tobytes()
    # starved rounds before the gate opens: the rounds behind them start from the untouched pose
    mixed = vcp_ctx.icp_aniso(sc["centers"], sc["truths"], [1e-9, 1e-9, 0.6], A.RATIO, Rs, Ts, ss, 3, ALL, G.MIN_PAIRS, 0.1)
    first = vcp_ctx.icp_aniso(sc["centers"], sc["truths"], [0.6], A.RATIO, Rs, Ts, ss, 1, ALL, G.MIN_PAIRS, 0.1)
    assert (mixed["starved"] == 2).all() and mixed["M_all"].tobytes() == first["M_all"].tobytes()
    assert mixed["scale"].tobytes() == first["scale"].tobytes()


@pytest.mark.parametrize("nt,ntrue,nclutter", [G.SIZES[0], G.SIZES[2]])
def test_closed_ratios_leave_the_scales_and_fit_rigidly(vcp_ctx, nt, ntrue, nclutter):
    sc = A.aniso_scene(nt, ntrue, nclutter, G.SEEDS[nt], (0.0, 0.0))
    Rs, Ts, ss = _three_poses(sc)
    Rs, Ts, ss = Rs[:1], Ts[:1], ss[:1]
    g = vcp_ctx.icp_aniso(sc["centers"], sc["truths"], G.schedule(), (1.0, 1.0), Rs, Ts, ss, G.ROUNDS, ALL, G.MIN_PAIRS, 0.1)
    assert g["scale"].tobytes() == ss.tobytes() and (g["unscaled"] == 0).all()
    # the rigid fit from A: vcp_icp_gated's from the start A, to rounding only (this step sets, that one composes)
    r = vcp_ctx.icp_gated(sc["centers"], sc["truths"], G.schedule(), sc["A0"].reshape(1, 3, 3), Ts, G.ROUNDS, ALL,
                          G.MIN_PAIRS, 0.1)
    assert g["kept"][0] == r["kept"][0] == ntrue and g["inliers"][0] == r["inliers"][0]
    assert np.abs(g["M_all"] - r["M_all"]).max() < 1e-9


def test_default_starts_are_the_explicit_ones(vcp_ctx):
    nt, ntrue, nclutter = SMALLEST
    sc = A.aniso_scene(nt, ntrue, nclutter, G.SEEDS[nt], (0.0, 0.0))
    src, tgt = sc["centers"], sc["truths"]
    ss = np.ascontiguousarray(np.tile(sc["s0"], (4, 1)) * np.array([[1.0, 1.0], [1.01, 0.99], [1.0, 1.02], [0.98, 1.0]]))
    Rs = rotations_about_z(4)
    ms, mt = G.seq_mean(src), G.seq_mean(tgt)
    Ts = np.zeros((4, 3))
    for h in range(4):
        Ah = A.pose_matrix(Rs[h].reshape(9).tolist(), ss[h].tolist())
        for r in range(3):
            Ts[h, r] = mt[r] - (Ah[3 * r] * ms[0] + Ah[3 * r + 1] * ms[1] + Ah[3 * r + 2] * ms[2])
    a = vcp_ctx.icp_aniso(src, tgt, [2.0, 1.0], A.RATIO, 4, None, ss, 6, ALL, G.MIN_PAIRS, 0.1)
    b = vcp_ctx.icp_aniso(src, tgt, [2.0, 1.0], A.RATIO, Rs, Ts, ss, 6, ALL, G.MIN_PAIRS, 0.1)
    for k in a:
        assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), k
    # init_scale NULL is all ones
    c = vcp_ctx.icp_aniso(src, tgt, [2.0, 1.0], A.RATIO, 4, None, None, 2, ALL, G.MIN_PAIRS, 0.1)
    d = vcp_ctx.icp_aniso(src, tgt, [2.0, 1.0], A.RATIO, 4, None, np.ones((4, 2)), 2, ALL, G.MIN_PAIRS, 0.1)
    for k in c:
        assert np.asarray(c[k]).tobytes() == np.asarray(d[k]).tobytes(), k


# ---- behaviour --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("err", A.START_ERRORS)
@pytest.mark.parametrize("nt,ntrue,nclutter", G.SIZES)
def test_behaviour_on_the_device(vcp_ctx, nt, ntrue, nclutter, err):
    """The conditions of tests/test_icp_aniso.py's reference tests, same seeds, through anisotropic_icp; gated_icp and
    similarity_icp from the same start matrix."""
    sc = A.aniso_scene(nt, ntrue, nclutter, G.SEEDS[nt], err)
    R0, T0 = sc["R0"].reshape(1, 3, 3), sc["T0"].reshape(1, 3)
    g = anisotropic_icp(sc["centers"], sc["truths"], sc["s0"], A.RATIO, G.schedule(), n_angles=R0, init_T=T0,
                        max_iter=G.ROUNDS, max_landmarks=ALL, min_pairs=G.MIN_PAIRS, inlier_dist=0.1, ctx=vcp_ctx)
    M = g["M"]
    within, perr = G.conditions(sc, M[:3, :3], M[:3, 3])
    print("anisotropic: start errors", err, "within", within, "pose error", perr, "scales", g["scale"][0], "kept",
          g["kept"][0], "starved", g["starved"][0], "unscaled", g["unscaled"][0])
    assert within == 1.0
    assert perr <= 0.02
    assert g["kept"][0] == ntrue and g["inliers"][0] == ntrue and (g["unscaled"][0] == 0).all() and g["starved"][0] == 0
    A0 = sc["A0"].reshape(1, 3, 3)
    u = gated_icp(sc["centers"], sc["truths"], G.schedule(), n_angles=A0, init_T=T0, max_iter=G.ROUNDS,
                  max_landmarks=ALL, min_pairs=G.MIN_PAIRS, inlier_dist=0.1, ctx=vcp_ctx)
    v = similarity_icp(sc["centers"], sc["truths"], G.schedule(), A.RATIO, n_angles=A0, init_T=T0, max_iter=G.ROUNDS,
                       max_landmarks=ALL, min_pairs=G.MIN_PAIRS, inlier_dist=0.1, ctx=vcp_ctx)
    pu = G.conditions(sc, u["M"][:3, :3], u["M"][:3, 3])[1]
    pv = G.conditions(sc, v["M"][:3, :3], v["M"][:3, 3])[1]
    print("from the same start: rigid pose error", pu, "similarity pose error", pv)
    if err in A.WRONG_STARTS:
        assert pu > 0.2 and pv > 0.2
    else:
        assert pu <= 0.02 and pv <= 0.02


# ---- errors, determinism, timing --------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _cloud():
    rng = np.random.default_rng(11)
    tgt = np.zeros((300, 3))
    tgt[:, :2] = rng.uniform(-10.0, 10.0, (300, 2))
    x = tgt[rng.integers(0, 300, 400)].copy()
    x[:, :2] += 0.05 * rng.normal(size=(400, 2))
    src = ((x - np.array([0.7, -0.4, 0.0])) @ G.rz(0.1)) / np.array([1.03, 0.98, 1.0])
    src[:, 2] = 0.0
    return np.ascontiguousarray(tgt), np.ascontiguousarray(src)


def test_errors_leave_the_outputs_untouched(vcp_ctx):
    tgt, src = _cloud()
    z = np.zeros((0, 3))

    def code(f, *a, **k):
        with pytest.raises(N.VcpError) as e:
            f(*a, **k)
        return e.value.code

    ai, asum = vcp_ctx.icp_aniso, vcp_ctx.icp_sums_aniso
    ok = (0.9, 1.1)
    for bad in ((math.nan, 1.1), (0.0, 1.1), (-0.5, 1.1), (0.9, math.nan), (0.9, INF), (1.0, 0.99), (1.01, 1.1), (0.5, 0.9),
                (INF, INF)):
        assert code(ai, src, tgt, [1.0], bad) == -1, bad
    for bad in (math.nan, 0.0, -1.0, INF, 1.7e308):                  # the last: its upper bound is not finite
        for a in range(2):
            s0 = np.ones((1, 2))
            s0[0, a] = bad
            assert code(ai, src, tgt, [1.0], ok, 1, None, s0) == -1, (bad, a)
    for bad in (0.0, -1.0, math.nan, -INF):
        assert code(asum, tgt, src, bad) == -1
        assert code(ai, src, tgt, [1.0, bad], ok) == -1
    assert code(ai, src, tgt, [], ok) == -1 and code(ai, src, tgt, [1.0], ok, min_pairs=0) == -1
    assert code(ai, z, tgt, [1.0], ok) == -2 and code(ai, src, z, [1.0], ok) == -2
    assert code(ai, src, tgt, [1.0], ok, 0) == -1 and code(ai, src, tgt, [1.0], ok, 4097) == -8
    assert code(ai, src, tgt, [1.0], ok, max_iter=0) == -1 and code(ai, src, tgt, [1.0], ok, max_landmarks=0) == -1
    assert code(ai, src, tgt, [1.0], ok, inlier_dist=0.0) == -1
    assert code(ai, src, tgt, [1.0], ok, np.full((1, 3, 3), math.nan)) == -1
    assert code(asum, z, src, 1.0) == -2 and code(asum, tgt, z, 1.0) == -1
    # a failed Horn solve in a round that is not starved fails the call; starved, the same pose passes
    bad_src = src.copy()
    bad_src[4, 0] = math.nan
    Rs, Tz = np.stack([np.eye(3), np.eye(3)]), np.zeros((2, 3))
    assert code(ai, bad_src, tgt, [INF], ok, Rs, Tz, None, 3) == -1
    g = ai(bad_src, tgt, [1e-9], ok, Rs, Tz, None, 3)
    assert (g["starved"] == 3).all() and (g["kept"] == 1).all() and (g["scale"] == 1.0).all()
    # nothing is written on an error (raw calls: every output pre-filled)
    s, t = np.ascontiguousarray(src), np.ascontiguousarray(tgt)

    def raw(gates, n_gates, min_pairs, lo, hi, scale0=(1.0, 1.0, 1.0, 1.0), n_poses=2, outs=True):
        gates = np.array(gates)
        s0 = np.array(scale0)
        o = dict(M=np.full(16, 7.0), Ma=np.full(32, 7.0), md=np.full(2, 7.0), inl=np.full(2, 7, np.int32),
                 st=np.full(2, 7, np.int32), kept=np.full(2, 7, np.int64), scale=np.full(4, 7.0),
                 un=np.full(4, 7, np.int32))
        best = C.c_int32(7)
        p = (lambda a: N._ptr(a)) if outs else (lambda a: None)
        rc = N.lib().vcp_icp_aniso(vcp_ctx._h, N._ptr(s), C.c_int64(len(s)), N._ptr(t), C.c_int64(len(t)),
                                   C.c_int32(n_poses), None, None, N._ptr(s0), 5, 200, N._ptr(gates), C.c_int32(n_gates),
                                   C.c_int32(min_pairs), C.c_double(lo), C.c_double(hi), C.c_double(1.0), N._ptr(o["M"]),
                                   C.byref(best), p(o["Ma"]), p(o["md"]), p(o["inl"]), p(o["kept"]), p(o["st"]),
                                   p(o["scale"]), p(o["un"]))
        return rc, best.value, o

    for a in (([math.nan], 1, 3, 0.9, 1.1), ([1.0], 0, 3, 0.9, 1.1), ([1.0], 1, 0, 0.9, 1.1), ([1.0], 1, 3, 1.01, 1.1),
              ([1.0], 1, 3, 0.9, INF), ([1.0], 1, 3, math.nan, 1.1), ([1.0], 1, 3, 0.0, 1.1), ([1.0], 1, 3, 1.0, 0.5),
              ([1.0], 1, 3, 0.9, 1.1, (1.0, 1.0, 1.0, math.nan)), ([1.0], 1, 3, 0.9, 1.1, (1.0, 0.0, 1.0, 1.0)),
              ([1.0], 1, 3, 0.9, 1.1, (-2.0, 1.0, 1.0, 1.0)), ([1.0], 1, 3, 0.9, 1.1, (1.0, 1.0, INF, 1.0))):
        rc, best, o = raw(*a)
        assert rc == -1 and best == 7 and all((v == 7).all() for v in o.values()), a
    S18, nn, keep = np.full(18, 7.0), np.full(len(s), 7, np.int32), np.full(len(s), 7, np.uint8)
    k = C.c_int64(7)
    rc = N.lib().vcp_icp_sums_aniso(vcp_ctx._h, N._ptr(t), C.c_int64(len(t)), N._ptr(s), C.c_int64(len(s)), None, None,
                                    C.c_double(0.0), N._ptr(S18), C.byref(k), N._ptr(nn), N._ptr(keep))
    assert rc == -1 and k.value == 7 and (S18 == 7).all() and (nn == 7).all() and (keep == 7).all()
    # every optional output may be NULL, and the context stays usable
    rc, best, o = raw([1.0, 0.5], 2, 3, 0.9, 1.1, outs=False)
    assert rc == 0 and best in (0, 1)
    assert o["M"].reshape(4, 4).tobytes() == ai(src, tgt, [1.0, 0.5], ok, 2, None, None, 5, 200, 3, 1.0)["M"].tobytes()


def test_determinism_and_the_calls_between(vcp_ctx):
    tgt, src = _cloud()
    gates = [2.0, 1.0, 0.5, 0.2]

    def call():
        return vcp_ctx.icp_aniso(src, tgt, gates, (0.9, 1.1), 8, None, None, 12, 200, 3, 0.2)

    a = call()
    b = call()
    vcp_ctx.icp_sim(src, tgt, gates, (0.9, 1.1), 8, None, 12, 200, 3, 0.2)
    c = call()
    for k in a:
        assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() == np.asarray(c[k]).tobytes(), k
    assert (a["scale"] != 1.0).all() and (a["unscaled"] == 0).all()       # every pose's rounds did fit both scales
    vcp_ctx.icp_sums_aniso(tgt, src, 1.0)                     # a one-pass call between changes nothing either
    d = call()
    assert d["M_all"].tobytes() == a["M_all"].tobytes() and d["scale"].tobytes() == a["scale"].tobytes()


def test_timing_phases(vcp_ctx):
    tgt, src = _cloud()
    vcp_ctx.timing_enable(True)
    try:
        vcp_ctx.icp_aniso(src, tgt, [1.0], (0.9, 1.1), 2, None, None, 3, 200, 3, 0.2)
        assert [p[0] for p in vcp_ctx.timing()] == ["icpa_rounds", "icpa_score"]
    finally:
        vcp_ctx.timing_enable(False)
