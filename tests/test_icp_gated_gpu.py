"""Gated ICP on the MI355X (include/vcp.h, "gated ICP").  One pass is held to the replayed reduction tree with the
dropped rows zeroed (tests/icp_sums_ref.py) on every path and workgroup size, the threshold to exactly representable
distances, whole runs to a round-by-round restatement from one-pass calls and the host Horn step, all-infinite gates to
vcp_icp_multistart, and the behaviour scene to the conditions its numpy reference meets (tests/icp_gated_ref.py)."""
import ctypes as C
import math

import numpy as np
import pytest

import icp_gated_ref as G
import icp_sums_ref as R
from vtkcloudpoint_amd import _native as N
from vtkcloudpoint_amd.icp import gated_icp

pytestmark = pytest.mark.gpu

INF = math.inf
RUN_ROUNDS = (1, 2, 8, 9, 17)   # around the 8-round batch boundary of the ungated loops
ALL = 100000                    # max_landmarks: every source point is a landmark

# (path, nm, nd): the smallest shapes that reach each pass kernel at both workgroup sizes (64 lanes up to 65536 slots,
# 256 beyond; the grid path has 8 slots per point)
PASS_SHAPES = ([("pairs", nm, nd) for nm in (1, 2, 100, 512) for nd in (1, 129, 1000)]
               + [("pairs", nm, 66000) for nm in (1, 2, 100, 512)]
               + [("grid", 513, 1000), ("grid", 513, 9000), ("tiled", 513, 1000), ("tiled", 513, 66000)])


def _same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b))


@pytest.mark.parametrize("path,nm,nd", PASS_SHAPES)
def test_one_pass_is_the_replay(vcp_ctx, path, nm, nd):
    pl = R.plan(nm, nd, path != "tiled")
    assert pl["path"] == path and pl["tb"] == (64 if nd <= 1000 else 256)
    model, data, Rm, T = R.case(path, nm, nd)
    nn, dd = G.brute_nn(model, R.transform(data, Rm, T))
    dist = np.sqrt(dd)
    half = float(np.median(dist))
    ungated, nn_u = vcp_ctx.icp_sums(model, data, Rm, T)
    assert _same(nn_u, nn)
    for gate, what in ((half, "half"), (1e-9, "all"), (INF, "none")):
        want, kept, keep = G.gated_sums(model, data, Rm, T, nn, gate)
        if what == "half":
            assert kept == int((dist < gate).sum()) and abs(kept - nd / 2) <= 1
        elif what == "all":
            assert kept == 0 and not want.any()
        else:
            assert kept == nd
        S, k, g_nn, g_keep = vcp_ctx.icp_sums_gated(model, data, gate, Rm, T)
        assert k == kept, (what, k, kept)
        assert _same(g_keep, keep) and _same(g_nn, nn), what
        assert _same(S, want), (what, S, want)
        assert not (np.signbit(S) & (S == 0.0)).any()       # a dropped pair adds +0.0: no sum is ever -0.0
        if what == "none":
            assert _same(S, ungated)
        # the outputs that may be NULL change nothing
        S2, k2, _, _ = vcp_ctx.icp_sums_gated(model, data, gate, Rm, T, want_nn=False, want_keep=False)
        assert _same(S2, S) and k2 == k


@pytest.mark.parametrize("path,nm", [("pairs", 100), ("grid", 600)])
def test_the_threshold_is_exact(vcp_ctx, path, nm):
    """Lattice coordinates, identity pose, pairs at distances exactly 5 * 2^-k (3-4-5 offsets of 2^-k): dd and its root
    are exact, so gate = the distance must drop the pair and the next binary64 number above it must keep it."""
    rng = np.random.default_rng(nm)
    side = int(math.ceil(math.sqrt(nm)))
    model = np.array([[8.0 * (j % side), 8.0 * (j // side), 0.0] for j in range(nm)])
    assert R.plan(nm, 1, True)["path"] == path
    ks = np.arange(1, 11)
    data, want_nn, kk = [], [], []
    for k in ks:
        for rep in range(24):
            j = int(rng.integers(0, nm))
            off = np.array([(3.0, 4.0, 0.0), (4.0, 3.0, 0.0), (0.0, 3.0, 4.0), (3.0, 0.0, 4.0)][rep % 4]) * 2.0 ** -k
            off *= rng.choice([-1.0, 1.0], 3)
            data.append(model[j] + off)
            want_nn.append(j)
            kk.append(k)
    data, want_nn, kk = np.array(data), np.array(want_nn), np.array(kk)
    assert (data * 1024 == np.round(data * 1024)).all()
    for k in ks:
        d = 5.0 * 2.0 ** -k
        for gate, keep in ((d, kk > k), (np.nextafter(d, INF), kk >= k)):
            S, kept, nn, g_keep = vcp_ctx.icp_sums_gated(model, data, gate)
            assert _same(nn, want_nn)
            assert _same(g_keep, keep.astype(np.uint8)), (k, gate)
            assert kept == int(keep.sum())
            assert S[15] == (25.0 * 4.0 ** -kk[keep]).sum()    # multiples of 2^-20 below 2^33: exact in any order


def _start(sc):
    return sc["R0"].reshape(1, 3, 3), sc["T0"].reshape(1, 3)


def _check_runs(ctx, sc, gates, rounds=RUN_ROUNDS):
    src, tgt = sc["centers"], sc["truths"]
    R0, T0 = _start(sc)
    lm = G.landmarks(src, ALL)
    assert len(lm) == len(src)
    tr = G.replay_run(ctx, N, tgt, lm, R0, T0, gates, max(rounds))
    for r in rounds:
        g = ctx.icp_gated(src, tgt, gates, R0, T0, r, ALL, G.MIN_PAIRS, 0.1)
        want = tr[r - 1]
        assert _same(g["M_all"][0], want["M"]) and _same(g["M"], want["M"]), ("rounds", r)
        assert g["mean_dist"][0] == want["mean_dist"], ("rounds", r)
        assert g["kept"][0] == want["kept"] and g["starved"][0] == want["starved"], ("rounds", r)
        assert g["best"] == 0
    return tr


@pytest.mark.parametrize("nt,ntrue,nclutter", G.SIZES[1:])   # 300 truths: the scalar-cache scan; 600: the grid
def test_whole_runs_are_the_replay(vcp_ctx, nt, ntrue, nclutter):
    sc = G.scene(nt, ntrue, nclutter, G.SEEDS[nt])
    tr = _check_runs(vcp_ctx, sc, G.schedule())
    assert tr[-1]["starved"] == 0 and 0 < tr[-1]["kept"] < len(sc["centers"])   # the gate does drop pairs


@pytest.mark.parametrize("nt,ntrue,nclutter", G.SIZES[1:])
def test_starved_rounds(vcp_ctx, nt, ntrue, nclutter):
    sc = G.scene(nt, ntrue, nclutter, G.SEEDS[nt])
    src, tgt = sc["centers"], sc["truths"]
    R0, T0 = _start(sc)
    M0 = np.eye(4)
    M0[:3, :3], M0[:3, 3] = sc["R0"], sc["T0"]
    gates = [1e-9, 1e-9, 1e-9, INF]
    tr = _check_runs(vcp_ctx, sc, gates, rounds=(1, 3, 4, 9))
    for r in (1, 2, 3):                                      # R and T untouched through the starved rounds
        assert _same(tr[r - 1]["M"], M0) and tr[r - 1]["starved"] == r and tr[r - 1]["kept"] == 0
        assert tr[r - 1]["mean_dist"] == INF
    assert tr[3]["starved"] == 3 and tr[3]["kept"] == len(src) and not _same(tr[3]["M"], M0)   # then it proceeds
    assert tr[8]["starved"] == 3
    # round 4 starts from a cold basis and the start pose: it is round 1 of the ungated run
    one = vcp_ctx.icp_multistart(src, tgt, R0, T0, 1, ALL, 0.1)
    assert _same(tr[3]["M"], one["M_all"][0]) and tr[3]["mean_dist"] == one["mean_dist"][0]
    for max_iter in (1, 9):                                  # every round starved
        g = vcp_ctx.icp_gated(src, tgt, [1e-9], R0, T0, max_iter, ALL, G.MIN_PAIRS, 0.1)
        assert _same(g["M_all"][0], M0) and _same(g["M"], M0)
        assert g["mean_dist"][0] == INF and g["starved"][0] == max_iter and g["kept"][0] == 0
    # min_pairs decides: with all pairs kept and min_pairs above their number every round starves too
    g = vcp_ctx.icp_gated(src, tgt, [INF], R0, T0, 5, ALL, len(src) + 1, 0.1)
    assert _same(g["M_all"][0], M0) and g["starved"][0] == 5 and g["kept"][0] == len(src)
    g = vcp_ctx.icp_gated(src, tgt, [INF], R0, T0, 5, ALL, len(src), 0.1)
    assert g["starved"][0] == 0 and not _same(g["M_all"][0], M0)


def _eight_poses():
    """8 rotations about z, one of them a reflection."""
    Rs = []
    for h in range(8):
        th = h * (2 * math.pi / 8)
        c, s = math.cos(th), math.sin(th)
        Rs.append([c, -s, 0.0, s, c, 0.0, 0.0, 0.0, 1.0])
    Rs[5] = [Rs[5][0], -Rs[5][1], 0.0, Rs[5][3], -Rs[5][4], 0.0, 0.0, 0.0, 1.0]
    Rs = np.array(Rs).reshape(8, 3, 3)
    assert np.linalg.det(Rs[5]) < -0.99
    return Rs


def _cloud(nt, ns, seed):
    """Planar truths and ns noisy samples of them moved back by a small rigid motion."""
    rng = np.random.default_rng(seed)
    tgt = np.zeros((nt, 3))
    tgt[:, :2] = rng.uniform(-10.0, 10.0, (nt, 2))
    x = tgt[rng.integers(0, nt, ns)].copy()
    x[:, :2] += 0.05 * rng.normal(size=(ns, 2))
    src = (x - np.array([0.7, -0.4, 0.0])) @ G.rz(0.1)
    src[:, 2] = 0.0
    return np.ascontiguousarray(tgt), np.ascontiguousarray(src)


@pytest.mark.parametrize("nt", [300, 3000])
@pytest.mark.parametrize("ml", [200, ALL])
def test_infinite_gates_equal_multistart(vcp_ctx, nt, ml):
    tgt, src = _cloud(nt, 1000, 500 + nt)
    Rs = _eight_poses()
    nlm = len(G.landmarks(src, ml))
    for init_T in (None, np.random.default_rng(nt).normal(0.0, 3.0, (8, 3)) * (1, 1, 0)):
        m = vcp_ctx.icp_multistart(src, tgt, Rs, init_T, 17, ml, 0.2)
        for gates in ([INF], [INF, INF, INF]):
            g = vcp_ctx.icp_gated(src, tgt, gates, Rs, init_T, 17, ml, 1, 0.2)
            for k in ("M", "M_all", "mean_dist", "inliers"):
                assert _same(g[k], m[k]), k
            assert g["best"] == m["best"]
            assert (g["kept"] == nlm).all() and (g["starved"] == 0).all()
    assert np.linalg.det(m["M_all"][5][:3, :3]) < 0


@pytest.mark.parametrize("nt", [300, 3000])
def test_batch_independence(vcp_ctx, nt):
    tgt, src = _cloud(nt, 1000, 700 + nt)
    Rs = _eight_poses()
    gates = [1e-9, 2.0, 1.0, 0.5, 0.2]          # a starved round, then a schedule that drops pairs in some poses
    g = vcp_ctx.icp_gated(src, tgt, gates, Rs, None, 12, 200, 3, 0.2)
    assert (g["starved"] >= 1).all() and len(set(g["kept"].tolist())) > 1
    for h in range(8):
        one = vcp_ctx.icp_gated(src, tgt, gates, Rs[h:h + 1], None, 12, 200, 3, 0.2)
        for k in ("M_all", "mean_dist", "inliers", "kept", "starved"):
            assert _same(one[k][0], g[k][h]), (h, k)
    # the default poses: an integer count gives the library's rotations, pose 0 the identity
    d = vcp_ctx.icp_gated(src, tgt, gates, 8, None, 12, 200, 3, 0.2)
    i0 = vcp_ctx.icp_gated(src, tgt, gates, np.eye(3)[None], None, 12, 200, 3, 0.2)
    assert _same(d["M_all"][0], i0["M_all"][0]) and d["kept"][0] == i0["kept"][0]


@pytest.mark.parametrize("nt,ntrue,nclutter", G.SIZES)
def test_behaviour_on_the_device(vcp_ctx, nt, ntrue, nclutter):
    """The conditions of tests/test_icp_gated.py::test_reference_behaviour, same seeds, through gated_icp."""
    sc = G.scene(nt, ntrue, nclutter, G.SEEDS[nt])
    R0, T0 = _start(sc)
    g = gated_icp(sc["centers"], sc["truths"], G.schedule(), n_angles=R0, init_T=T0, max_iter=G.ROUNDS,
                  max_landmarks=ALL, min_pairs=G.MIN_PAIRS, inlier_dist=0.1, ctx=vcp_ctx)
    M = g["M"]
    within, err = G.conditions(sc, M[:3, :3], M[:3, 3])
    print("gated: within", within, "pose error", err, "kept", g["kept"][0], "starved", g["starved"][0])
    assert within == 1.0
    assert err < 0.01
    assert g["kept"][0] == ntrue
    assert g["inliers"][0] == ntrue                          # the score is not gated: clutter has no truth within 0.1
    u = vcp_ctx.icp_multistart(sc["centers"], sc["truths"], R0, T0, G.ROUNDS, ALL, 0.1)
    Mu = u["M"]
    within_u, err_u = G.conditions(sc, Mu[:3, :3], Mu[:3, 3])
    print("ungated: within", within_u, "pose error", err_u)
    assert within_u < 0.5


def test_errors(vcp_ctx):
    tgt, src = _cloud(300, 400, 9)
    z = np.zeros((0, 3))

    def code(f, *a, **k):
        with pytest.raises(N.VcpError) as e:
            f(*a, **k)
        return e.value.code

    gi, gs = vcp_ctx.icp_gated, vcp_ctx.icp_sums_gated
    for bad in (0.0, -1.0, math.nan, -INF):
        assert code(gs, tgt, src, bad) == -1
        assert code(gi, src, tgt, [bad]) == -1
        assert code(gi, src, tgt, [1.0, bad, 0.5]) == -1
    assert code(gi, src, tgt, []) == -1                       # n_gates < 1
    assert code(gi, src, tgt, [1.0], min_pairs=0) == -1 and code(gi, src, tgt, [1.0], min_pairs=-2) == -1
    # vcp_icp_multistart's
    assert code(gi, z, tgt, [1.0]) == -2 and code(gi, src, z, [1.0]) == -2
    assert code(gi, src, tgt, [1.0], 0) == -1 and code(gi, src, tgt, [1.0], 4097) == -8
    assert code(gi, src, tgt, [1.0], max_iter=0) == -1 and code(gi, src, tgt, [1.0], max_landmarks=0) == -1
    assert code(gi, src, tgt, [1.0], inlier_dist=0.0) == -1 and code(gi, src, tgt, [1.0], inlier_dist=math.nan) == -1
    assert code(gs, z, src, 1.0) == -2 and code(gs, tgt, z, 1.0) == -1
    # a failed Horn solve in a round that is not starved fails the call; starved, the same pose passes
    # (a NaN landmark: its dd is NaN, which no gate drops, and the sums it poisons fail the solve)
    bad_src = src.copy()
    bad_src[4, 0] = math.nan   # source point 4 = landmark 2 (every second point is one)
    Rs, Tz = np.stack([np.eye(3), np.eye(3)]), np.zeros((2, 3))
    assert code(gi, bad_src, tgt, [INF], Rs, Tz, 3) == -1
    ok = gi(bad_src, tgt, [1e-9], Rs, Tz, 3)
    assert (ok["starved"] == 3).all() and (ok["kept"] == 1).all()
    # an overflowing dd is +inf and sqrt(inf) >= inf: dropped even by the infinite gate, so this pose starves
    Tn = np.zeros((2, 3))
    Tn[1, 0] = 1e308
    ok = gi(src, tgt, [INF], Rs, Tn, 3)
    assert ok["starved"].tolist() == [0, 3] and ok["kept"].tolist() == [200, 0]
    # nothing is written to the outputs on an error (raw calls: every output pre-filled)
    s, t = np.ascontiguousarray(src), np.ascontiguousarray(tgt)
    for gates, n_gates, min_pairs in (([math.nan], 1, 3), ([1.0], 0, 3), ([1.0], 1, 0), ([1.0, -1.0], 2, 3)):
        gates = np.array(gates)
        M, Ma, md = np.full(16, 7.0), np.full(32, 7.0), np.full(2, 7.0)
        inl, st = np.full(2, 7, np.int32), np.full(2, 7, np.int32)
        kept = np.full(2, 7, np.int64)
        best = C.c_int32(7)
        rc = N.lib().vcp_icp_gated(vcp_ctx._h, N._ptr(s), C.c_int64(len(s)), N._ptr(t), C.c_int64(len(t)), C.c_int32(2),
                                   None, None, 5, 200, N._ptr(gates), C.c_int32(n_gates), C.c_int32(min_pairs),
                                   C.c_double(1.0), N._ptr(M), C.byref(best), N._ptr(Ma), N._ptr(md), N._ptr(inl),
                                   N._ptr(kept), N._ptr(st))
        assert rc == -1
        assert best.value == 7 and (M == 7).all() and (Ma == 7).all() and (md == 7).all()
        assert (inl == 7).all() and (kept == 7).all() and (st == 7).all()
    S, nn, keep = np.full(16, 7.0), np.full(len(s), 7, np.int32), np.full(len(s), 7, np.uint8)
    k = C.c_int64(7)
    rc = N.lib().vcp_icp_sums_gated(vcp_ctx._h, N._ptr(t), C.c_int64(len(t)), N._ptr(s), C.c_int64(len(s)), None, None,
                                    C.c_double(0.0), N._ptr(S), C.byref(k), N._ptr(nn), N._ptr(keep))
    assert rc == -1 and k.value == 7 and (S == 7).all() and (nn == 7).all() and (keep == 7).all()
    # kept and starved may be NULL, and the context stays usable
    M, best = np.zeros(16), C.c_int32(-1)
    gates = np.array([1.0, 0.5])
    rc = N.lib().vcp_icp_gated(vcp_ctx._h, N._ptr(s), C.c_int64(len(s)), N._ptr(t), C.c_int64(len(t)), C.c_int32(2),
                               None, None, 5, 200, N._ptr(gates), C.c_int32(2), C.c_int32(3), C.c_double(1.0), N._ptr(M),
                               C.byref(best), None, None, None, None, None)
    assert rc == 0 and best.value in (0, 1)
    assert _same(M.reshape(4, 4), gi(src, tgt, gates, 2, None, 5, 200, 3, 1.0)["M"])
