"""Trimmed ICP on the MI355X (include/vcp.h, "trimmed ICP").  One pass is held to the replayed reduction tree with the
dropped rows zeroed (tests/icp_sums_ref.py) on every path and workgroup size, the select to exact ties on both sides of
the threshold between its two forms, whole runs to a round-by-round restatement from one-pass calls and the host Horn
step, share 1.0 to vcp_icp_multistart, and the behaviour scene to the conditions its numpy reference meets
(tests/icp_trimmed_ref.py)."""
import ctypes as C
import math

import numpy as np
import pytest

import icp_gated_ref as G
import icp_sums_ref as R
import icp_trimmed_ref as TR
from vtkcloudpoint_amd import _native as N
from vtkcloudpoint_amd.icp import trimmed_icp

pytestmark = pytest.mark.gpu

INF, NAN = math.inf, math.nan
RUN_ROUNDS = (1, 2, 8, 9, 17)
ALL = 100000                    # max_landmarks: every source point is a landmark
WG = TR.SELECT_WG_MAX           # the select: one workgroup per pose up to this many landmarks, histogram launches beyond

# (path, nm, nd): the shapes of tests/test_icp_gated_gpu.py -- each pass kernel at both workgroup sizes; nd = 1000 and
# below take the one-workgroup select, 9000 and 66 000 the histogram form
PASS_SHAPES = ([("pairs", nm, nd) for nm in (1, 2, 100, 512) for nd in (1, 129, 1000)]
               + [("pairs", nm, 66000) for nm in (1, 2, 100, 512)]
               + [("grid", 513, 1000), ("grid", 513, 9000), ("tiled", 513, 1000), ("tiled", 513, 66000)])


def _same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b))


def _same_nan(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


def _ms(nd):
    return sorted({m for m in (1, nd // 2, nd - 1, nd) if 1 <= m <= nd})


def _check_pass(ctx, model, data, Rm, T, m, nn, nullable=False):
    want, keep, thr = TR.trimmed_sums(model, data, Rm, T, nn, m)
    S, g_thr, g_nn, g_keep = ctx.icp_sums_trimmed(model, data, m, Rm, T)
    assert _same(g_nn, nn), m
    assert _same(g_keep, keep), (m, np.flatnonzero(g_keep != keep)[:8])
    assert int(g_keep.sum()) == m
    assert TR.same_float(g_thr, thr), (m, g_thr, thr)
    assert _same_nan(S, want), (m, S, want)
    assert not (np.signbit(S) & (S == 0.0)).any()           # a dropped pair adds +0.0: no sum is ever -0.0
    if nullable:                                            # the outputs that may be NULL change nothing
        S2, thr2, _, _ = ctx.icp_sums_trimmed(model, data, m, Rm, T, want_nn=False, want_keep=False)
        assert _same_nan(S2, S) and TR.same_float(thr2, g_thr)
    return S, g_keep, g_thr


@pytest.mark.parametrize("path,nm,nd", PASS_SHAPES)
def test_one_pass_is_the_replay(vcp_ctx, path, nm, nd):
    pl = R.plan(nm, nd, path != "tiled")
    assert pl["path"] == path and pl["tb"] == (64 if nd <= 1000 else 256)
    model, data, Rm, T = R.case(path, nm, nd)
    nn, dd = G.brute_nn(model, R.transform(data, Rm, T))
    ungated, nn_u = vcp_ctx.icp_sums(model, data, Rm, T)
    assert _same(nn_u, nn)
    for m in _ms(nd):
        S, keep, thr = _check_pass(vcp_ctx, model, data, Rm, T, m, nn, nullable=m == nd // 2)
        assert thr == np.sort(dd)[m - 1]
        if m == nd:
            assert _same(S, ungated) and keep.all()


# ---- the select ------------------------------------------------------------------------------------------------------
def _lattice(nm):
    side = int(math.ceil(math.sqrt(nm)))
    return np.array([[8.0 * (j % side), 8.0 * (j // side), 0.0] for j in range(nm)])


# both forms of the select on both sides of SELECT_WG_MAX (= VCP_ICPT_SELECT_WG_MAX), and well inside each
SELECT_ND = (1, 2, 255, 1000, WG - 1, WG, WG + 1, 9000)


@pytest.mark.parametrize("path,nm", [("pairs", 100), ("grid", 600)])
@pytest.mark.parametrize("nd", SELECT_ND)
def test_select_on_equal_distances(vcp_ctx, path, nm, nd):
    """data = targets + (3, 4, 0) 2^-k: every dd is exactly 25 * 2^-2k, the keys differ in the index alone, and the kept
    set must be the first m landmarks -- ranks 1 and L included."""
    assert R.plan(nm, nd, True)["path"] == path
    rng = np.random.default_rng([nm, nd])
    model = _lattice(nm)
    k = 3
    nn = rng.integers(0, nm, nd)
    data = model[nn] + np.array([3.0, 4.0, 0.0]) * 2.0 ** -k
    ms = sorted({1, 2, nd // 3 + 1, nd // 2, nd - 1, nd, int(rng.integers(1, nd + 1))} & set(range(1, nd + 1)))
    for m in ms:
        S, thr, g_nn, keep = vcp_ctx.icp_sums_trimmed(model, data, m)
        assert _same(g_nn, nn)
        assert thr == 25.0 * 4.0 ** -k
        assert keep[:m].all() and not keep[m:].any(), (m, np.flatnonzero(keep)[-3:])
        assert S[15] == m * 25.0 * 4.0 ** -k                 # multiples of 2^-6: exact in any order


@pytest.mark.parametrize("path,nm", [("pairs", 100), ("grid", 600)])
@pytest.mark.parametrize("nd", (255, 1000, WG, WG + 1, 9000))
def test_select_on_two_levels(vcp_ctx, path, nm, nd):
    """Offsets of 5 * 2^-k and 10 * 2^-k in shuffled order, m inside the lower level, on the boundary and inside the upper
    level: the lower level goes first whatever its indices, each level in index order."""
    rng = np.random.default_rng([nm, nd, 2])
    model = _lattice(nm)
    k = 4
    nn = rng.integers(0, nm, nd)
    upper = rng.random(nd) < 0.4
    off = np.where(upper[:, None], np.array([6.0, 8.0, 0.0]), np.array([4.0, 3.0, 0.0])) * 2.0 ** -k
    off *= rng.choice([-1.0, 1.0], (nd, 3))
    data = model[nn] + off
    lo, hi = np.flatnonzero(~upper), np.flatnonzero(upper)
    nl = len(lo)
    assert 0 < nl < nd
    d_lo, d_hi = 25.0 * 4.0 ** -k, 100.0 * 4.0 ** -k
    for m in sorted({1, nl // 2, nl - 1, nl, nl + 1, nl + len(hi) // 2, nd - 1, nd} & set(range(1, nd + 1))):
        want = np.zeros(nd, np.uint8)
        want[lo[:m]] = 1
        want[hi[:max(0, m - nl)]] = 1
        ref_keep, ref_thr = TR.trim_mask(np.where(upper, d_hi, d_lo), m)
        assert _same(ref_keep, want.astype(bool)) and ref_thr == (d_lo if m <= nl else d_hi)
        S, thr, g_nn, keep = vcp_ctx.icp_sums_trimmed(model, data, m)
        assert _same(g_nn, nn)
        assert thr == ref_thr, m
        assert _same(keep, want), (m, nl)
        assert S[15] == min(m, nl) * d_lo + max(0, m - nl) * d_hi


@pytest.mark.parametrize("nd", (WG, WG + 1))
def test_select_on_distinct_distances(vcp_ctx, nd):
    """Random distances at the threshold between the forms, every rank of a spread of 40 and the two ends."""
    model, data, Rm, T = R.case("pairs", 100, nd)
    nn, dd = G.brute_nn(model, R.transform(data, Rm, T))
    order = np.lexsort((np.arange(nd), TR.keys(dd)))
    for m in sorted({1, nd} | set(np.linspace(2, nd - 1, 40).astype(int).tolist())):
        S, thr, _, keep = vcp_ctx.icp_sums_trimmed(model, data, m, Rm, T, want_nn=False)
        assert thr == dd[order[m - 1]], m
        want = np.zeros(nd, np.uint8)
        want[order[:m]] = 1
        assert _same(keep, want), m


# ---- NaN and overflow ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nd", (1000, WG + 1))
def test_nan_ranks_last_and_inf_before_it(vcp_ctx, nd):
    model, data, Rm, T = R.case("pairs", 100, nd)
    data = data.copy()
    i_nan, i_inf = nd // 3, nd // 3 + 7                       # the overflowing row has the HIGHER index and still goes first
    data[i_nan, 1] = NAN
    data[i_inf] = (1e200, -1e200, 1e200)
    nn, dd = G.brute_nn(model, R.transform(data, Rm, T))
    assert math.isnan(dd[i_nan]) and dd[i_inf] == INF and np.isfinite(np.delete(dd, [i_nan, i_inf])).all()
    S, keep, thr = _check_pass(vcp_ctx, model, data, Rm, T, nd - 2, nn)
    assert np.isfinite(S).all() and not keep[i_nan] and not keep[i_inf] and np.isfinite(thr)
    S, keep, thr = _check_pass(vcp_ctx, model, data, Rm, T, nd - 1, nn)   # m reaches +inf, not the NaN
    assert keep[i_inf] and not keep[i_nan] and thr == INF and S[15] == INF and not np.isnan(S[:6]).any()
    S, keep, thr = _check_pass(vcp_ctx, model, data, Rm, T, nd, nn)       # m reaches the NaN: it poisons the sums
    assert keep.all() and math.isnan(thr) and np.isnan(S[15]) and np.isnan(S[1])
    # one NaN row alone
    data[i_inf] = data[0]
    nn, dd = G.brute_nn(model, R.transform(data, Rm, T))
    S, keep, thr = _check_pass(vcp_ctx, model, data, Rm, T, nd - 1, nn)
    assert np.isfinite(S).all() and not keep[i_nan] and keep.sum() == nd - 1
    S, keep, thr = _check_pass(vcp_ctx, model, data, Rm, T, nd, nn)
    assert np.isnan(S[15]) and math.isnan(thr)


# ---- whole runs ------------------------------------------------------------------------------------------------------
def _start(sc):
    return sc["R0"].reshape(1, 3, 3), sc["T0"].reshape(1, 3)


def _check_runs(ctx, sc, keep, rounds=RUN_ROUNDS, scale=1.0):
    src, tgt = sc["centers"] * scale, sc["truths"] * scale
    R0, T0 = _start(sc)
    T0 = T0 * scale
    lm = G.landmarks(src, ALL)
    assert len(lm) == len(src)
    tr = TR.replay_run(ctx, N, tgt, lm, R0, T0, keep, max(rounds))
    runs = {}
    for r in rounds:
        g = ctx.icp_trimmed(src, tgt, keep, R0, T0, r, ALL, G.MIN_PAIRS, 0.1 * scale)
        want = tr[r - 1]
        assert _same(g["M_all"][0], want["M"]) and _same(g["M"], want["M"]), ("rounds", r)
        assert g["mean_dist"][0] == want["mean_dist"], ("rounds", r)
        assert g["kept"][0] == want["kept"] and g["starved"][0] == want["starved"], ("rounds", r)
        assert g["trim_dist"][0] == want["trim_dist"], ("rounds", r)
        assert g["best"] == 0
        runs[r] = g
    return tr, runs


def _shares(sc):
    """A schedule that falls to the share of true centroids over five rounds and stays there."""
    from vtkcloudpoint_amd.icp import expected_share, trim_schedule
    n = len(sc["centers"])
    f = expected_share(n, len(sc["truths"]), sc["is_true"].sum() / len(sc["truths"]))
    assert TR.keep_count(f, n) == sc["is_true"].sum()
    return trim_schedule(1.0, f, 5)


@pytest.mark.parametrize("nt,ntrue,nclutter", G.SIZES[1:])   # 300 truths: the scalar-cache scan; 600: the grid
def test_whole_runs_are_the_replay(vcp_ctx, nt, ntrue, nclutter):
    sc = G.scene(nt, ntrue, nclutter, G.SEEDS[nt])
    tr, _ = _check_runs(vcp_ctx, sc, _shares(sc))
    assert tr[-1]["starved"] == 0 and tr[-1]["kept"] == ntrue and tr[0]["kept"] == ntrue + nclutter
    assert tr[-1]["trim_dist"] > 0.0 and len({t["kept"] for t in tr}) == 5       # every step of the schedule was used


@pytest.mark.parametrize("nt,ntrue,nclutter", G.SIZES[1:])
def test_scaling_by_a_power_of_two(vcp_ctx, nt, ntrue, nclutter):
    """Every coordinate times 2^10: the same pairs kept, the same rotation, lengths times 2^10.  The scaled run is held
    to its own replay first (the requirement), then to the unscaled run (the Horn step's invariance, vcp.h)."""
    sc = G.scene(nt, ntrue, nclutter, G.SEEDS[nt])
    k = 1024.0
    # one pass
    model, data = sc["truths"], sc["centers"]
    m = ntrue
    S, thr, nn, keep = vcp_ctx.icp_sums_trimmed(model, data, m, sc["R0"], sc["T0"])
    S2, thr2, nn2, keep2 = vcp_ctx.icp_sums_trimmed(model * k, data * k, m, sc["R0"], sc["T0"] * k)
    assert _same(nn2, nn) and _same(keep2, keep) and thr2 == thr * k * k
    assert _same(S2[:6], S[:6] * k) and _same(S2[6:], S[6:] * k * k)
    # whole runs
    keep = _shares(sc)
    rounds = (2, 17)
    _, a = _check_runs(vcp_ctx, sc, keep, rounds)
    _, b = _check_runs(vcp_ctx, sc, keep, rounds, scale=k)
    for r in rounds:
        assert _same(b[r]["kept"], a[r]["kept"]) and _same(b[r]["starved"], a[r]["starved"]), r
        assert b[r]["best"] == a[r]["best"]
        assert _same(b[r]["M_all"][:, :3, :3], a[r]["M_all"][:, :3, :3]), r
        assert _same(b[r]["M_all"][:, :3, 3], a[r]["M_all"][:, :3, 3] * k), r
        assert _same(b[r]["mean_dist"], a[r]["mean_dist"] * k) and _same(b[r]["trim_dist"], a[r]["trim_dist"] * k), r


@pytest.mark.parametrize("nt,ntrue,nclutter", G.SIZES[1:])
def test_starved_rounds(vcp_ctx, nt, ntrue, nclutter):
    sc = G.scene(nt, ntrue, nclutter, G.SEEDS[nt])
    src, tgt = sc["centers"], sc["truths"]
    n = len(src)
    R0, T0 = _start(sc)
    M0 = np.eye(4)
    M0[:3, :3], M0[:3, 3] = sc["R0"], sc["T0"]
    tiny = 1.5 / n                                           # m = ceil(1.5) = 2 < min_pairs = 3
    assert TR.keep_count(tiny, n) == 2
    keep = [tiny, tiny, tiny, 1.0]
    tr, _ = _check_runs(vcp_ctx, sc, keep, rounds=(1, 3, 4, 9))
    for r in (1, 2, 3):                                      # R and T untouched through the starved rounds
        assert _same(tr[r - 1]["M"], M0) and tr[r - 1]["starved"] == r and tr[r - 1]["kept"] == 2
    assert tr[3]["starved"] == 3 and tr[3]["kept"] == n and not _same(tr[3]["M"], M0)   # then it proceeds
    assert tr[8]["starved"] == 3
    # round 4 starts from a cold basis and the start pose: it is round 1 of the untrimmed run
    one = vcp_ctx.icp_multistart(src, tgt, R0, T0, 1, ALL, 0.1)
    assert _same(tr[3]["M"], one["M_all"][0]) and tr[3]["mean_dist"] == one["mean_dist"][0]
    # every round starved: the start pose comes back; the select still ran
    nn, dd = G.brute_nn(tgt, R.transform(src, sc["R0"], sc["T0"]))
    two = np.sort(dd)[:2]
    for max_iter in (1, 9):
        g = vcp_ctx.icp_trimmed(src, tgt, [tiny], R0, T0, max_iter, ALL, G.MIN_PAIRS, 0.1)
        assert _same(g["M_all"][0], M0) and _same(g["M"], M0)
        assert g["starved"][0] == max_iter and g["kept"][0] == 2
        assert g["trim_dist"][0] == math.sqrt(two[1]) and g["mean_dist"][0] == math.sqrt((two[0] + two[1]) / 2)
    # min_pairs decides: with all pairs kept and min_pairs above their number every round starves too
    g = vcp_ctx.icp_trimmed(src, tgt, [1.0], R0, T0, 5, ALL, n + 1, 0.1)
    assert _same(g["M_all"][0], M0) and g["starved"][0] == 5 and g["kept"][0] == n
    g = vcp_ctx.icp_trimmed(src, tgt, [1.0], R0, T0, 5, ALL, n, 0.1)
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
def test_share_one_equals_multistart(vcp_ctx, nt, ml):
    tgt, src = _cloud(nt, 1000, 500 + nt)
    Rs = _eight_poses()
    nlm = len(G.landmarks(src, ml))
    for init_T in (None, np.random.default_rng(nt).normal(0.0, 3.0, (8, 3)) * (1, 1, 0)):
        m = vcp_ctx.icp_multistart(src, tgt, Rs, init_T, 17, ml, 0.2)
        for keep in ([1.0], [1.0, 1.0, 1.0]):
            g = vcp_ctx.icp_trimmed(src, tgt, keep, Rs, init_T, 17, ml, 1, 0.2)
            for k in ("M", "M_all", "mean_dist", "inliers"):
                assert _same(g[k], m[k]), k
            assert g["best"] == m["best"]
            assert (g["kept"] == nlm).all() and (g["starved"] == 0).all()
            assert (g["trim_dist"] > 0).all() and (g["trim_dist"] >= g["mean_dist"]).all()
    assert np.linalg.det(m["M_all"][5][:3, :3]) < 0


@pytest.mark.parametrize("nt,ns,ml", [(300, 1000, 200), (3000, 1000, 200), (300, 2 * WG + 2, ALL)])
def test_batch_independence(vcp_ctx, nt, ns, ml):
    """Each of 8 poses alone has the bits it has in the batch, and a second call repeats the first -- with the select in
    its one-workgroup form (200 landmarks) and in its histogram form (more than SELECT_WG_MAX)."""
    tgt, src = _cloud(nt, ns, 700 + nt)
    Rs = _eight_poses()
    L = len(G.landmarks(src, ml))
    assert (L > WG) == (ml == ALL)
    keep = [1.5 / L, 1.0, 0.9, 0.8, 0.7]        # a starved round (m = 2), then a schedule that drops pairs
    rounds = 12 if L <= WG else 4
    g = vcp_ctx.icp_trimmed(src, tgt, keep, Rs, None, rounds, ml, 3, 0.2)
    assert (g["starved"] == 1).all() and (g["kept"] == TR.keep_count(keep[min(rounds, 5) - 1], L)).all()
    assert len(set(g["trim_dist"].tolist())) > 1
    again = vcp_ctx.icp_trimmed(src, tgt, keep, Rs, None, rounds, ml, 3, 0.2)
    for k in ("M", "M_all", "mean_dist", "inliers", "kept", "starved", "trim_dist"):
        assert _same(again[k], g[k]), k
    assert again["best"] == g["best"]
    for h in range(8):
        one = vcp_ctx.icp_trimmed(src, tgt, keep, Rs[h:h + 1], None, rounds, ml, 3, 0.2)
        for k in ("M_all", "mean_dist", "inliers", "kept", "starved", "trim_dist"):
            assert _same(one[k][0], g[k][h]), (h, k)
    # the default poses: an integer count gives the library's rotations, pose 0 the identity
    d = vcp_ctx.icp_trimmed(src, tgt, keep, 8, None, rounds, ml, 3, 0.2)
    i0 = vcp_ctx.icp_trimmed(src, tgt, keep, np.eye(3)[None], None, rounds, ml, 3, 0.2)
    assert _same(d["M_all"][0], i0["M_all"][0]) and d["trim_dist"][0] == i0["trim_dist"][0]


@pytest.mark.parametrize("nt,ntrue,nclutter", G.SIZES)
def test_behaviour_on_the_device(vcp_ctx, nt, ntrue, nclutter):
    """The conditions of tests/test_icp_trimmed.py::test_reference_behaviour, same seeds, through trimmed_icp."""
    sc = G.scene(nt, ntrue, nclutter, G.SEEDS[nt])
    R0, T0 = _start(sc)
    n = len(sc["centers"])

    def run(share):
        g = trimmed_icp(sc["centers"], sc["truths"], share, n_angles=R0, init_T=T0, max_iter=G.ROUNDS,
                        max_landmarks=ALL, min_pairs=G.MIN_PAIRS, inlier_dist=0.1, ctx=vcp_ctx)
        M = g["M"]
        within, err = G.conditions(sc, M[:3, :3], M[:3, 3])
        print("share", share, "within", within, "pose error", err, "kept", g["kept"][0], "trim_dist", g["trim_dist"][0])
        return g, within, err

    g, within, err = run(ntrue / n)
    assert within == 1.0
    assert err < 0.01
    assert g["kept"][0] == ntrue
    assert g["inliers"][0] == ntrue                          # the score is not trimmed: clutter has no truth within 0.1
    g, within, err = run(0.6)
    assert within == 1.0
    assert err < 0.01
    g, within_u, err_u = run(1.0)
    assert within_u < 0.5
    assert g["kept"][0] == n


def test_global_icp_with_a_keep_share(vcp_ctx):
    """global_icp(keep=...) is register_pairs followed by trimmed_icp on the winners; keep=None is the gated polish it
    was."""
    import register_ref as RG
    from vtkcloudpoint_amd.icp import choose_bases, expected_share, gate_schedule, global_icp, register_pairs
    window, seed, bseed = RG.SCENES["half"]
    sc = RG.overlap_scene(window, seed)
    src, tgt = sc["source"], sc["truths"]
    bases = choose_bases(src, RG.N_BASES, RG.MIN_LEN, RG.MAX_LEN, bseed)
    reg = register_pairs(src, tgt, bases, RG.LEN_TOL, RG.INLIER, ctx=vcp_ctx)
    used = np.flatnonzero(reg["score"] >= 0)
    assert len(used) > 0
    Ms = reg["M_all"][used]
    g0, g1, gr, rounds = RG.POLISH
    share = expected_share(len(src), sc["planted"], 1.0)
    assert 0.0 < share < 1.0
    p = global_icp(src, tgt, bases, RG.LEN_TOL, RG.INLIER, None, max_iter=rounds, keep=share, ctx=vcp_ctx)
    want = trimmed_icp(src, tgt, share, n_angles=np.ascontiguousarray(Ms[:, :3, :3]),
                       init_T=np.ascontiguousarray(Ms[:, :3, 3]), max_iter=rounds, inlier_dist=RG.INLIER, ctx=vcp_ctx)
    for k in ("M", "M_all", "mean_dist", "inliers", "kept", "starved", "trim_dist"):
        assert _same(p[k], want[k]), k
    assert p["best"] == want["best"] and _same(p["bases_used"], used)
    for k in ("M_all", "score", "inliers", "pick", "n_hyp"):
        assert _same(p["registration"][k], reg[k]), k
    print("planted", sc["planted"], "registration", reg["inliers"][used], "after the trimmed polish", p["inliers"])
    assert p["inliers"][p["best"]] >= 0.95 * sc["planted"]
    # keep=None: the gated polish, unchanged
    gates = gate_schedule(g0, g1, gr)
    q = global_icp(src, tgt, bases, RG.LEN_TOL, RG.INLIER, gates, max_iter=rounds, ctx=vcp_ctx)
    q2 = global_icp(src, tgt, bases, RG.LEN_TOL, RG.INLIER, gates, max_iter=rounds, ctx=vcp_ctx, keep=None)
    old = vcp_ctx.icp_gated(src, tgt, gates, np.ascontiguousarray(Ms[:, :3, :3]), np.ascontiguousarray(Ms[:, :3, 3]),
                            rounds, 200, 3, RG.INLIER)
    assert "trim_dist" not in q
    for k in ("M", "M_all", "mean_dist", "inliers", "kept", "starved"):
        assert _same(q[k], old[k]) and _same(q2[k], old[k]), k


def test_errors(vcp_ctx):
    tgt, src = _cloud(300, 400, 9)
    z = np.zeros((0, 3))

    def code(f, *a, **k):
        with pytest.raises(N.VcpError) as e:
            f(*a, **k)
        return e.value.code

    ti, ts = vcp_ctx.icp_trimmed, vcp_ctx.icp_sums_trimmed
    for bad in (0, -1, len(src) + 1):
        assert code(ts, tgt, src, bad) == -1
    for bad in (0.0, -0.5, NAN, np.nextafter(1.0, 2.0), 2.0, INF, -INF):
        assert code(ti, src, tgt, [bad]) == -1
        assert code(ti, src, tgt, [1.0, bad, 0.5]) == -1
    assert code(ti, src, tgt, []) == -1                       # n_keep < 1
    assert code(ti, src, tgt, [1.0], min_pairs=0) == -1 and code(ti, src, tgt, [1.0], min_pairs=-2) == -1
    # vcp_icp_multistart's
    assert code(ti, z, tgt, [1.0]) == -2 and code(ti, src, z, [1.0]) == -2
    assert code(ti, src, tgt, [1.0], 0) == -1 and code(ti, src, tgt, [1.0], 4097) == -8
    assert code(ti, src, tgt, [1.0], max_iter=0) == -1 and code(ti, src, tgt, [1.0], max_landmarks=0) == -1
    assert code(ti, src, tgt, [1.0], inlier_dist=0.0) == -1 and code(ti, src, tgt, [1.0], inlier_dist=NAN) == -1
    assert code(ts, z, src, 1) == -2 and code(ts, tgt, z, 1) == -1
    # a failed Horn solve in a round that is not starved fails the call; while m does not reach the NaN pair, the same
    # pose passes (source point 4 = landmark 2: every second point is a landmark)
    bad_src = src.copy()
    bad_src[4, 0] = NAN
    Rs, Tz = np.stack([np.eye(3), np.eye(3)]), np.zeros((2, 3))
    assert code(ti, bad_src, tgt, [1.0], Rs, Tz, 3) == -1
    ok = ti(bad_src, tgt, [198.5 / 200.0], Rs, Tz, 3)       # m = ceil(198.5) = 199
    assert (ok["starved"] == 0).all() and (ok["kept"] == 199).all() and np.isfinite(ok["M_all"]).all()
    ok = ti(bad_src, tgt, [1.0], Rs, Tz, 3, min_pairs=201)   # starved: the poisoned sums are never solved
    assert (ok["starved"] == 3).all() and (ok["kept"] == 200).all() and np.isnan(ok["trim_dist"]).all()
    # nothing is written to the outputs on an error (raw calls: every output pre-filled)
    s, t = np.ascontiguousarray(src), np.ascontiguousarray(tgt)
    for keep, n_keep, min_pairs in (([NAN], 1, 3), ([1.0], 0, 3), ([1.0], 1, 0), ([1.0, -1.0], 2, 3), ([1.5], 1, 3),
                                    ([0.0], 1, 3)):
        keep = np.array(keep)
        M, Ma, md, td = np.full(16, 7.0), np.full(32, 7.0), np.full(2, 7.0), np.full(2, 7.0)
        inl, st = np.full(2, 7, np.int32), np.full(2, 7, np.int32)
        kept = np.full(2, 7, np.int64)
        best = C.c_int32(7)
        rc = N.lib().vcp_icp_trimmed(vcp_ctx._h, N._ptr(s), C.c_int64(len(s)), N._ptr(t), C.c_int64(len(t)),
                                     C.c_int32(2), None, None, 5, 200, N._ptr(keep), C.c_int32(n_keep),
                                     C.c_int32(min_pairs), C.c_double(1.0), N._ptr(M), C.byref(best), N._ptr(Ma),
                                     N._ptr(md), N._ptr(inl), N._ptr(kept), N._ptr(st), N._ptr(td))
        assert rc == -1
        assert best.value == 7 and (M == 7).all() and (Ma == 7).all() and (md == 7).all() and (td == 7).all()
        assert (inl == 7).all() and (kept == 7).all() and (st == 7).all()
    for m in (0, len(s) + 1, -5):
        S, nn, keep = np.full(16, 7.0), np.full(len(s), 7, np.int32), np.full(len(s), 7, np.uint8)
        thr = C.c_double(7.0)
        rc = N.lib().vcp_icp_sums_trimmed(vcp_ctx._h, N._ptr(t), C.c_int64(len(t)), N._ptr(s), C.c_int64(len(s)), None,
                                          None, C.c_int64(m), N._ptr(S), C.byref(thr), N._ptr(nn), N._ptr(keep))
        assert rc == -1 and thr.value == 7.0 and (S == 7).all() and (nn == 7).all() and (keep == 7).all()
    S = np.full(16, 7.0)                                      # thr_dd is required
    rc = N.lib().vcp_icp_sums_trimmed(vcp_ctx._h, N._ptr(t), C.c_int64(len(t)), N._ptr(s), C.c_int64(len(s)), None, None,
                                      C.c_int64(5), N._ptr(S), None, None, None)
    assert rc == -1 and (S == 7).all()
    # kept, starved and trim_dist may be NULL, and the context stays usable
    M, best = np.zeros(16), C.c_int32(-1)
    keep = np.array([1.0, 0.8])
    rc = N.lib().vcp_icp_trimmed(vcp_ctx._h, N._ptr(s), C.c_int64(len(s)), N._ptr(t), C.c_int64(len(t)), C.c_int32(2),
                                 None, None, 5, 200, N._ptr(keep), C.c_int32(2), C.c_int32(3), C.c_double(1.0),
                                 N._ptr(M), C.byref(best), None, None, None, None, None, None)
    assert rc == 0 and best.value in (0, 1)
    assert _same(M.reshape(4, 4), ti(src, tgt, keep, 2, None, 5, 200, 3, 1.0)["M"])


# ---- a seeded sweep of small one-pass cases --------------------------------------------------------------------------
def test_sweep_of_small_cases(vcp_ctx):
    """200 random one-pass calls against the replay: nm <= 600 (all three paths), nd <= 300, random m and pose; half of
    them on lattice coordinates, where distances tie by the dozen and so do the nearest targets."""
    rng = np.random.default_rng(20)
    seen = set()
    for it in range(200):
        nm = int(rng.choice([int(rng.integers(1, 20)), int(rng.integers(1, 513)), int(rng.integers(513, 601))]))
        nd = int(rng.integers(1, 301))
        m = int(rng.integers(1, nd + 1))
        lattice = it % 2 == 1
        if lattice:
            model = rng.integers(-6, 7, (nm, 3)).astype(np.float64)
            data = rng.integers(-6, 7, (nd, 3)).astype(np.float64) * 0.5
            Rm = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]]) if it % 4 == 1 else np.eye(3)
            T = rng.integers(-2, 3, 3).astype(np.float64)
        else:
            model = rng.uniform(-10.0, 10.0, (nm, 3))
            data = rng.uniform(-10.0, 10.0, (nd, 3))
            Rm = R.rotation(rng.normal(size=3), float(rng.uniform(-3.0, 3.0)))
            T = rng.normal(0.0, 2.0, 3)
        if nm > 512 and it % 3 == 0:
            model[int(rng.integers(0, nm)), int(rng.integers(0, 3))] = INF     # the tiled path
        pl = R.plan(nm, nd, np.isfinite(model).all())
        seen.add(pl["path"])
        nn, dd = G.brute_nn(model, R.transform(data, Rm, T))
        _check_pass(vcp_ctx, model, data, Rm, T, m, nn)
    assert seen == {"pairs", "grid", "tiled"}
