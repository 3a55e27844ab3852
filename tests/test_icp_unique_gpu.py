"""Unique-correspondence ICP on the MI355X (include/vcp.h, "unique-correspondence ICP").  One round's passes are held to
the replayed reduction tree with the dropped rows zeroed (tests/icp_sums_ref.py) on every path and workgroup size, the
winner rule to exact ties, duplicates, NaN and overflow, whole runs to a round-by-round restatement from one-pass calls
and the host Horn step (a slot left over from one round would decide the next: that is what fails there), an injective
scene to vcp_icp_gated, and the ghost scene to the conditions its numpy reference meets (tests/icp_unique_ref.py)."""
import ctypes as C
import math

import numpy as np
import pytest

import icp_gated_ref as G
import icp_sums_ref as R
import icp_unique_ref as U
from vtkcloudpoint_amd import _native as N
from vtkcloudpoint_amd.icp import unique_icp

pytestmark = pytest.mark.gpu

INF, NAN = math.inf, math.nan
ALL = 100000                    # max_landmarks: every source point is a landmark
RESET_STEP_MAX = 4096           # UNIQ_RESET_STEP_MAX (icp.hip): beyond it a kernel of its own sets the slots back

# (path, nm, nd): the shapes of tests/test_icp_trimmed_gpu.py -- each pass kernel at both workgroup sizes (64 threads up
# to nd = 1000, 256 at 9000 and 66 000) -- and the smallest ones
PASS_SHAPES = ([("pairs", nm, nd) for nm in (1, 2, 100, 512) for nd in (1, 129, 1000)]
               + [("pairs", nm, 66000) for nm in (1, 2, 100, 512)]
               + [("grid", 513, 1000), ("grid", 513, 9000), ("tiled", 513, 1000), ("tiled", 513, 66000)]
               + [("pairs", 1, 7), ("pairs", 3, 200)])


def _same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b))


def _same_nan(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


def _check_pass(ctx, model, data, Rm, T, gate, nn, nullable=False):
    want, kept, lost, code = U.unique_sums(model, data, Rm, T, nn, gate)
    S, g_kept, g_lost, g_nn, g_keep = ctx.icp_sums_unique(model, data, gate, Rm, T)
    assert _same(g_nn, nn), gate
    assert _same(g_keep, code), (gate, np.flatnonzero(g_keep != code)[:8])
    assert g_kept == kept and g_lost == lost, (gate, g_kept, kept, g_lost, lost)
    assert g_lost == len(data) - len(np.unique(nn))          # one winner per claimed target
    assert _same_nan(S, want), (gate, S, want)
    assert not (np.signbit(S) & (S == 0.0)).any()            # a dropped pair adds +0.0: no sum is ever -0.0
    if nullable:                                             # the outputs that may be NULL change nothing
        S2, k2, l2, _, _ = ctx.icp_sums_unique(model, data, gate, Rm, T, want_nn=False, want_keep=False)
        assert _same_nan(S2, S) and k2 == g_kept and l2 == g_lost
    return S, g_kept, g_lost, g_keep


def _mid_gate(dd, win):
    """A gate between the winners' distances: it drops about half of them."""
    d = np.sqrt(dd[win & np.isfinite(dd)])
    return float(np.median(d)) if len(d) else 1.0


@pytest.mark.parametrize("path,nm,nd", PASS_SHAPES)
def test_one_pass_is_the_replay(vcp_ctx, path, nm, nd):
    pl = R.plan(nm, nd, path != "tiled")
    assert pl["path"] == path and pl["tb"] == (64 if nd <= 1000 else 256)
    model, data, Rm, T = R.case(path, nm, nd)
    nn, dd = G.brute_nn(model, R.transform(data, Rm, T))
    win = U.unique_mask(nn, dd)
    mid = _mid_gate(dd, win)
    for gate in (INF, mid, 1e-3):
        S, kept, lost, keep = _check_pass(vcp_ctx, model, data, Rm, T, gate, nn, nullable=gate == mid)
        assert kept <= min(nm, nd) and kept + lost <= nd
    if np.isfinite(dd).all():
        assert 0 < U.keep_codes(nn, dd, mid).tolist().count(0) or win.sum() == 1      # the middle gate drops winners


@pytest.mark.parametrize("path,nm,nd", [("pairs", 100, 99), ("pairs", 512, 300), ("grid", 600, 599), ("grid", 600, 200),
                                        ("tiled", 513, 129)])
def test_injective_pass_is_the_ungated_pass(vcp_ctx, path, nm, nd):
    """gate = +inf and every data point on a target of its own: sums bit-identical to vcp_icp_sums, nothing lost."""
    rng = np.random.default_rng([nm, nd])
    model = np.zeros((nm, 3))
    side = int(math.ceil(math.sqrt(nm)))
    model[:, 0], model[:, 1] = 2.0 * (np.arange(nm) % side), 2.0 * (np.arange(nm) // side)
    if path == "tiled":
        model[nm - 1, 2] = INF
    nn = rng.permutation(nm - 1)[:nd]
    data = model[nn] + rng.uniform(-0.3, 0.3, (nd, 3)) * (1, 1, 0)
    assert R.plan(nm, nd, np.isfinite(model).all())["path"] == path
    plain, nn_p = vcp_ctx.icp_sums(model, data)
    assert _same(nn_p, nn)
    S, kept, lost, g_nn, keep = vcp_ctx.icp_sums_unique(model, data, INF)
    assert _same(S, plain) and kept == nd and lost == 0 and _same(g_nn, nn) and (keep == 1).all()
    _check_pass(vcp_ctx, model, data, None, None, 0.2, nn)


# ---- the winner rule on exact ties -----------------------------------------------------------------------------------
def _lattice(nm):
    side = int(math.ceil(math.sqrt(nm)))
    return np.array([[8.0 * (j % side), 8.0 * (j // side), 0.0] for j in range(nm)])


@pytest.mark.parametrize("path,nm", [("pairs", 100), ("grid", 600)])
@pytest.mark.parametrize("nd", (2, 255, 1000, 9000))
def test_mirrored_rows_tie_bit_for_bit(vcp_ctx, path, nm, nd):
    """data = target +- (3, 4, 0) 2^-k in shuffled order: every dd on a target of one level is the same number, so the
    index alone decides among them, and a closer level beats a lower index."""
    assert R.plan(nm, nd, True)["path"] == path
    rng = np.random.default_rng([nm, nd])
    model = _lattice(nm)
    nn = rng.integers(0, nm, nd)
    far = rng.random(nd) < 0.5
    off = np.where(far[:, None], np.array([6.0, 8.0, 0.0]), np.array([3.0, 4.0, 0.0])) * 2.0 ** -4
    off *= rng.choice([-1.0, 1.0], (nd, 1))                  # mirrored about the target
    data = model[nn] + off
    d_lo, d_hi = 25.0 * 4.0 ** -4, 100.0 * 4.0 ** -4
    want = np.full(nd, 2, np.uint8)
    for j in np.unique(nn):
        on = np.flatnonzero(nn == j)
        near = on[~far[on]]
        want[near[0] if len(near) else on[0]] = 1
    nn_b, dd = G.brute_nn(model, data)
    assert _same(nn_b, nn) and _same(dd, np.where(far, d_hi, d_lo)) and _same(U.keep_codes(nn, dd, INF), want)
    S, kept, lost, g_nn, keep = vcp_ctx.icp_sums_unique(model, data, INF)
    assert _same(g_nn, nn) and _same(keep, want), np.flatnonzero(keep != want)[:8]
    assert kept == (want == 1).sum() == len(np.unique(nn)) and lost == nd - kept
    assert S[15] == dd[want == 1].sum()                      # multiples of 2^-8: exact in any order
    # a gate between the levels drops the winners of the far level and hands their targets to nobody
    gate = 0.5
    assert math.sqrt(d_lo) < gate < math.sqrt(d_hi)
    want_g = np.where((want == 1) & far, 0, want).astype(np.uint8)
    S, kept, lost_g, _, keep = vcp_ctx.icp_sums_unique(model, data, gate)
    assert _same(keep, want_g) and lost_g == lost and kept == (want_g == 1).sum() and S[15] == kept * d_lo
    _check_pass(vcp_ctx, model, data, None, None, gate, nn)
    # the gate exactly at a level: sqrt(dd) >= gate drops it
    S, kept, _, _, keep = vcp_ctx.icp_sums_unique(model, data, math.sqrt(d_lo))
    assert kept == 0 and not (keep == 1).any() and (S == 0.0).all()


@pytest.mark.parametrize("path,nm,nd", [("pairs", 100, 1000), ("grid", 600, 9000), ("tiled", 513, 1000)])
def test_duplicated_rows(vcp_ctx, path, nm, nd):
    """Every data row three times, in shuffled places: the first copy of the closest row wins its target."""
    model, data, Rm, T = R.case(path, nm, nd // 3 + 1)
    rng = np.random.default_rng(nd)
    data = np.ascontiguousarray(np.tile(data, (3, 1))[rng.permutation(3 * len(data))][:nd])
    nn, dd = G.brute_nn(model, R.transform(data, Rm, T))
    for gate in (INF, _mid_gate(dd, U.unique_mask(nn, dd))):
        S, kept, lost, keep = _check_pass(vcp_ctx, model, data, Rm, T, gate, nn)
    assert lost >= nd - nd // 3 - 1 - 1


@pytest.mark.parametrize("nd", (1000, 9000))
def test_nan_and_overflow(vcp_ctx, nd):
    model, data, Rm, T = R.case("pairs", 100, nd)
    data = data.copy()
    nn0, _ = G.brute_nn(model, R.transform(data, Rm, T))
    i_nan, i_inf = nd // 3, nd // 3 + 7
    data[i_nan, 1] = NAN                                     # its nn is target 0 (every comparison fails)
    data[i_inf] = (1e200, -1e200, 1e200)
    nn, dd = G.brute_nn(model, R.transform(data, Rm, T))
    assert math.isnan(dd[i_nan]) and dd[i_inf] == INF
    # a NaN pair loses to any number on its target, +inf included
    S, kept, lost, keep = _check_pass(vcp_ctx, model, data, Rm, T, INF, nn)
    assert keep[i_nan] == 2 and np.isfinite(S[:15]).all()
    # a target whose pairs are all NaN keeps the lowest index, which poisons the sums whatever the gate
    only = np.flatnonzero(nn == nn[i_nan])
    data[only] = NAN
    nn, dd = G.brute_nn(model, R.transform(data, Rm, T))
    first = np.flatnonzero(np.isnan(dd))[0]
    for gate in (INF, 0.5):
        S, kept, lost, keep = _check_pass(vcp_ctx, model, data, Rm, T, gate, nn)
        assert keep[first] == 1 and (keep[np.flatnonzero(np.isnan(dd))[1:]] == 2).all() and np.isnan(S[15])
    # a winner at +inf is dropped even by the infinite gate
    model2 = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0]])
    data2 = np.array([[1e200, 0.0, 0.0], [1.1, 0.0, 0.0], [1e200, 1.0, 0.0]])
    nn2, dd2 = G.brute_nn(model2, data2)
    assert np.isinf(dd2[[0, 2]]).all() and nn2.tolist() == [0, 1, 0]
    S, kept, lost, keep = _check_pass(vcp_ctx, model2, data2, None, None, INF, nn2)
    assert keep.tolist() == [0, 1, 2] and (kept, lost) == (1, 1)


def test_gate_on_winner_and_loser(vcp_ctx):
    """The gate plays no part in the choice of the winner: a loser inside the gate stays out, and a gate that drops a
    winner drops its loser too (the loser is never closer) and leaves the target empty."""
    model = _lattice(9)
    nn = np.array([4, 4, 0, 7, 7, 7])
    off = np.array([[0.5, 0, 0], [0.25, 0, 0], [0, 1.0, 0], [0, -2.0, 0], [1.0, 0, 0], [0, 1.5, 0]])
    data = model[nn] + off
    S, kept, lost, g_nn, keep = vcp_ctx.icp_sums_unique(model, data, INF)
    assert _same(g_nn, nn) and keep.tolist() == [2, 1, 1, 2, 1, 2] and (kept, lost) == (3, 3)
    S, kept, lost, _, keep = vcp_ctx.icp_sums_unique(model, data, 0.75)     # the loser at 0.5 lies inside: still lost
    assert keep.tolist() == [2, 1, 0, 2, 0, 2] and (kept, lost) == (1, 3) and S[15] == 0.0625
    S, kept, lost, _, keep = vcp_ctx.icp_sums_unique(model, data, 0.25)
    assert keep.tolist() == [2, 0, 0, 2, 0, 2] and (kept, lost) == (0, 3) and (S == 0.0).all()
    _check_pass(vcp_ctx, model, data, None, None, 0.75, nn)


# ---- whole runs ------------------------------------------------------------------------------------------------------
def _start(sc):
    return sc["R0"].reshape(1, 3, 3), sc["T0"].reshape(1, 3)


KEYS = ("M_all", "mean_dist", "inliers", "kept", "starved", "lost")


def _five_starts(sc):
    """The scene's start and four near it."""
    rng = np.random.default_rng(3)
    Rs = np.stack([G.rz(G.ANGLE + G.D_ANGLE + a) for a in (0.0, 0.02, -0.02, 0.05, -0.04)])
    Ts = sc["T0"] + np.concatenate([np.zeros((1, 3)), rng.normal(0.0, 0.1, (4, 3)) * (1, 1, 0)])
    return Rs, np.ascontiguousarray(Ts)


@pytest.mark.parametrize("nt,ntrue,nclutter", G.SIZES[:2])   # 40 and 300 truths
def test_whole_runs_are_the_replay(vcp_ctx, nt, ntrue, nclutter):
    sc = U.ghost_scene(nt, ntrue, nclutter, U.SEEDS[nt][0])
    src, tgt = sc["centers"], sc["truths"]
    lm = G.landmarks(src, ALL)
    assert len(lm) == len(src)
    gates = G.schedule()
    Rs, Ts = _five_starts(sc)
    rounds = (1, 2, 8, 9, 17)
    tr = [U.replay_run(vcp_ctx, N, tgt, lm, Rs[h], Ts[h], gates, max(rounds)) for h in range(5)]
    # the scene does what the test needs: winners and claimed targets change from round to round, pairs are lost, the
    # gate drops winners
    assert all(not _same(t[0]["keep"] == 1, t[1]["keep"] == 1) for t in tr)           # every pose changes winners
    assert sum(not _same(t[r]["nn"], t[r + 1]["nn"]) for t in tr for r in range(8)) >= 4
    assert any(len({tuple(np.unique(x["nn"]).tolist()) for x in t}) > 2 for t in tr)   # and some the claimed targets
    assert all(x["lost"] >= sc["n_ghost"] for t in tr for x in t) and all((x["keep"] == 0).any() for t in tr for x in t)
    for r in rounds:
        one = vcp_ctx.icp_unique(src, tgt, gates, Rs[:1], Ts[:1], r, ALL, G.MIN_PAIRS, 0.1)
        five = vcp_ctx.icp_unique(src, tgt, gates, Rs, Ts, r, ALL, G.MIN_PAIRS, 0.1)
        for h, g in [(0, one)] + [(h, five) for h in range(5)]:
            k = 0 if g is one else h
            want = tr[h][r - 1]
            assert _same(g["M_all"][k], want["M"]), ("rounds", r, "pose", h)
            assert g["mean_dist"][k] == want["mean_dist"], ("rounds", r, "pose", h)
            assert g["kept"][k] == want["kept"] and g["starved"][k] == want["starved"], ("rounds", r, "pose", h)
            assert g["lost"][k] == want["lost"], ("rounds", r, "pose", h)
        assert _same(five["M"], five["M_all"][five["best"]])
        again = vcp_ctx.icp_unique(src, tgt, gates, Rs, Ts, r, ALL, G.MIN_PAIRS, 0.1)      # two calls: identical bits
        assert all(again[k].tobytes() == five[k].tobytes() for k in KEYS) and again["best"] == five["best"]


def _cloud(nt, ns, seed):
    """Planar truths and ns noisy samples of them moved back by a small rigid motion: many samples per truth."""
    rng = np.random.default_rng(seed)
    tgt = np.zeros((nt, 3))
    tgt[:, :2] = rng.uniform(-10.0, 10.0, (nt, 2))
    x = tgt[rng.integers(0, nt, ns)].copy()
    x[:, :2] += 0.05 * rng.normal(size=(ns, 2))
    src = (x - np.array([0.7, -0.4, 0.0])) @ G.rz(0.1)
    src[:, 2] = 0.0
    return np.ascontiguousarray(tgt), np.ascontiguousarray(src)


@pytest.mark.parametrize("nt", [300, 3000])
def test_runs_beyond_the_step_reset(vcp_ctx, nt):
    """More landmarks than the step sets back itself (a kernel of its own does it), on the scalar-cache and the grid
    path, three poses: the replay, pose by pose, and the poses alone."""
    tgt, src = _cloud(nt, 2 * RESET_STEP_MAX + 2, 900 + nt)
    lm = G.landmarks(src, ALL)
    assert len(lm) > RESET_STEP_MAX
    gates = [2.0, 0.5, 0.2]
    Rs = np.stack([np.eye(3), G.rz(0.05), G.rz(-0.08)])
    Ts = np.array([[0.0, 0.0, 0.0], [0.3, 0.1, 0.0], [-0.2, 0.4, 0.0]])
    rounds = 5
    g = vcp_ctx.icp_unique(src, tgt, gates, Rs, Ts, rounds, ALL, 3, 0.2)
    assert (g["lost"] >= len(lm) - nt).all() and (g["kept"] <= nt).all() and (g["kept"] >= 3).all()
    assert (g["starved"] == 0).all() and len(set(g["kept"].tolist())) == 3
    for h in range(3):
        want = U.replay_run(vcp_ctx, N, tgt, lm, Rs[h], Ts[h], gates, rounds, 3)[-1]
        assert _same(g["M_all"][h], want["M"]) and g["mean_dist"][h] == want["mean_dist"], h
        assert (g["kept"][h], g["lost"][h], g["starved"][h]) == (want["kept"], want["lost"], want["starved"]), h
        one = vcp_ctx.icp_unique(src, tgt, gates, Rs[h:h + 1], Ts[h:h + 1], rounds, ALL, 3, 0.2)
        assert all(one[k][0].tobytes() == g[k][h].tobytes() for k in KEYS), h


def test_independent_of_the_context_history(vcp_ctx):
    """A call after a call with a larger nt (and more landmarks, and more poses) on the same context equals the call
    on a fresh context: the slots are filled per call, whatever the workspace held."""
    sc = U.ghost_scene(*G.SIZES[0], U.SEEDS[40][0])
    big_tgt, big_src = _cloud(3000, 5000, 77)
    gates = G.schedule()
    R0, T0 = _start(sc)
    fresh_ctx = N.Context(0)
    try:
        fresh = fresh_ctx.icp_unique(sc["centers"], sc["truths"], gates, R0, T0, 12, ALL, G.MIN_PAIRS, 0.1)
    finally:
        fresh_ctx.close()
    vcp_ctx.icp_unique(big_src, big_tgt, [1.0, 0.3], 4, None, 6, ALL, 3, 0.2)
    after = vcp_ctx.icp_unique(sc["centers"], sc["truths"], gates, R0, T0, 12, ALL, G.MIN_PAIRS, 0.1)
    vcp_ctx.icp_sums_unique(big_tgt, big_src, 0.3)
    vcp_ctx.icp_trimmed(big_src, big_tgt, [0.5], 2, None, 3, ALL, 3, 0.2)     # shares the workspace
    later = vcp_ctx.icp_unique(sc["centers"], sc["truths"], gates, R0, T0, 12, ALL, G.MIN_PAIRS, 0.1)
    for k in KEYS + ("M",):
        assert after[k].tobytes() == fresh[k].tobytes() and later[k].tobytes() == fresh[k].tobytes(), k
    assert fresh["lost"][0] > 0


@pytest.mark.parametrize("nt", [300, 600])
def test_injective_runs_equal_gated(vcp_ctx, nt):
    """No ghosts, no clutter, a start close enough that no two centroids share a truth in any round (the replay shows
    lost = 0 throughout): every output is vcp_icp_gated's, bit for bit."""
    sc = G.scene(nt, nt - 60, 0, G.SEEDS[nt])
    src, tgt = sc["centers"], sc["truths"]
    Rs = np.stack([G.rz(G.ANGLE + a) for a in (0.002, -0.003, 0.0)])
    Ts = sc["T_true"] + np.array([[0.02, -0.015, 0.0], [-0.03, 0.01, 0.0], [0.0, 0.04, 0.0]])
    gates = G.schedule()
    lm = G.landmarks(src, ALL)
    rounds = 12
    for h in range(3):
        tr = U.replay_run(vcp_ctx, N, tgt, lm, Rs[h], Ts[h], gates, rounds)
        assert all(t["lost"] == 0 for t in tr) and tr[-1]["kept"] == len(lm)
    u = vcp_ctx.icp_unique(src, tgt, gates, Rs, Ts, rounds, ALL, G.MIN_PAIRS, 0.1)
    g = vcp_ctx.icp_gated(src, tgt, gates, Rs, Ts, rounds, ALL, G.MIN_PAIRS, 0.1)
    for k in ("M", "M_all", "mean_dist", "inliers", "kept", "starved"):
        assert u[k].tobytes() == g[k].tobytes(), k
    assert u["best"] == g["best"] and (u["lost"] == 0).all() and (u["starved"] == 0).all()


@pytest.mark.parametrize("nt,ntrue,nclutter", G.SIZES)
def test_behaviour_on_the_device(vcp_ctx, nt, ntrue, nclutter):
    """The conditions of tests/test_icp_unique.py::test_reference_behaviour, same seeds, through unique_icp and
    gated_icp."""
    from vtkcloudpoint_amd.icp import gated_icp
    for seed in U.SEEDS[nt]:
        sc = U.ghost_scene(nt, ntrue, nclutter, seed)
        R0, T0 = _start(sc)
        gates = G.schedule()
        bias = sc["bias"]
        kw = dict(n_angles=R0, init_T=T0, max_iter=G.ROUNDS, max_landmarks=ALL, min_pairs=G.MIN_PAIRS, inlier_dist=0.1,
                  ctx=vcp_ctx)
        a = gated_icp(sc["centers"], sc["truths"], gates, **kw)
        within_a, err_a = G.conditions(sc, a["M"][:3, :3], a["M"][:3, 3])
        u = unique_icp(sc["centers"], sc["truths"], gates, **kw)
        within_u, err_u = G.conditions(sc, u["M"][:3, :3], u["M"][:3, 3])
        print("seed", seed, "bias", bias, "gated: within", within_a, "pose error", err_a, "| unique: within", within_u,
              "pose error", err_u, "kept", u["kept"][0], "lost", u["lost"][0])
        assert within_a == 1.0 and within_u == 1.0
        assert err_a >= 0.75 * bias
        assert err_u <= 0.5 * bias
        assert u["kept"][0] == ntrue and u["lost"][0] >= sc["n_ghost"] and u["starved"][0] == 0


def test_global_unique_icp(vcp_ctx):
    """global_unique_icp is register_pairs followed by one unique_icp call from the winners."""
    import register_ref as RG
    from vtkcloudpoint_amd.icp import choose_bases, gate_schedule, global_unique_icp, register_pairs
    window, seed, bseed = RG.SCENES["half"]
    sc = RG.overlap_scene(window, seed)
    src, tgt = sc["source"], sc["truths"]
    bases = choose_bases(src, RG.N_BASES, RG.MIN_LEN, RG.MAX_LEN, bseed)
    reg = register_pairs(src, tgt, bases, RG.LEN_TOL, RG.INLIER, ctx=vcp_ctx)
    used = np.flatnonzero(reg["score"] >= 0)
    assert len(used) > 0
    Ms = reg["M_all"][used]
    g0, g1, gr, rounds = RG.POLISH
    gates = gate_schedule(g0, g1, gr)
    p = global_unique_icp(src, tgt, bases, RG.LEN_TOL, RG.INLIER, gates, max_iter=rounds, ctx=vcp_ctx)
    want = unique_icp(src, tgt, gates, n_angles=np.ascontiguousarray(Ms[:, :3, :3]),
                      init_T=np.ascontiguousarray(Ms[:, :3, 3]), max_iter=rounds, inlier_dist=RG.INLIER, ctx=vcp_ctx)
    for k in KEYS + ("M",):
        assert _same(p[k], want[k]), k
    assert p["best"] == want["best"] and _same(p["bases_used"], used)
    for k in ("M_all", "score", "inliers", "pick", "n_hyp"):
        assert _same(p["registration"][k], reg[k]), k
    assert p["inliers"][p["best"]] >= 0.95 * sc["planted"]


def test_errors(vcp_ctx):
    tgt, src = _cloud(300, 400, 9)
    z = np.zeros((0, 3))

    def code(f, *a, **k):
        with pytest.raises(N.VcpError) as e:
            f(*a, **k)
        return e.value.code

    ui, us = vcp_ctx.icp_unique, vcp_ctx.icp_sums_unique
    for bad in (0.0, -1.0, NAN, -INF):
        assert code(us, tgt, src, bad) == -1
        assert code(ui, src, tgt, [bad]) == -1
        assert code(ui, src, tgt, [1.0, bad, 0.5]) == -1
    assert code(ui, src, tgt, []) == -1                       # n_gates < 1
    assert code(ui, src, tgt, [1.0], min_pairs=0) == -1 and code(ui, src, tgt, [1.0], min_pairs=-2) == -1
    # vcp_icp_multistart's
    assert code(ui, z, tgt, [1.0]) == -2 and code(ui, src, z, [1.0]) == -2
    assert code(ui, src, tgt, [1.0], 0) == -1 and code(ui, src, tgt, [1.0], 4097) == -8
    assert code(ui, src, tgt, [1.0], max_iter=0) == -1 and code(ui, src, tgt, [1.0], max_landmarks=0) == -1
    assert code(ui, src, tgt, [1.0], inlier_dist=0.0) == -1 and code(ui, src, tgt, [1.0], inlier_dist=NAN) == -1
    assert code(us, z, src, 1.0) == -2 and code(us, tgt, z, 1.0) == -1
    # a failed Horn solve in a round that is not starved fails the call; starved, the same pose passes.  The NaN
    # landmark's nn is target 0; with the start at the identity no other landmark of this cloud is on target 0, so it
    # is its target's winner, which no gate drops
    bad_src = src.copy()
    bad_src[4, 0] = NAN        # source point 4 = landmark 2 (every second point is one)
    lm = G.landmarks(bad_src, 200)
    nn, dd = G.brute_nn(tgt, lm)
    assert math.isnan(dd[2]) and nn[2] == 0
    lm_ok = np.delete(lm, 2, axis=0)
    lm_ok = lm_ok[G.brute_nn(tgt, lm_ok)[0] != 0]
    bad2 = np.concatenate([lm[2:3], lm_ok])                   # the NaN row and rows that leave target 0 to it
    Rs, Tz = np.stack([np.eye(3), np.eye(3)]), np.zeros((2, 3))
    assert code(ui, bad2, tgt, [INF], Rs, Tz, 3, ALL) == -1
    ok = ui(bad2, tgt, [1e-9], Rs, Tz, 3, ALL)
    assert (ok["starved"] == 3).all() and (ok["kept"] == 1).all()
    # nothing is written to the outputs on an error (raw calls: every output pre-filled)
    s, t = np.ascontiguousarray(src), np.ascontiguousarray(tgt)
    for gates, n_gates, min_pairs in (([NAN], 1, 3), ([1.0], 0, 3), ([1.0], 1, 0), ([1.0, -1.0], 2, 3)):
        gates = np.array(gates)
        M, Ma, md = np.full(16, 7.0), np.full(32, 7.0), np.full(2, 7.0)
        inl, st = np.full(2, 7, np.int32), np.full(2, 7, np.int32)
        kept, lost = np.full(2, 7, np.int64), np.full(2, 7, np.int64)
        best = C.c_int32(7)
        rc = N.lib().vcp_icp_unique(vcp_ctx._h, N._ptr(s), C.c_int64(len(s)), N._ptr(t), C.c_int64(len(t)), C.c_int32(2),
                                    None, None, 5, 200, N._ptr(gates), C.c_int32(n_gates), C.c_int32(min_pairs),
                                    C.c_double(1.0), N._ptr(M), C.byref(best), N._ptr(Ma), N._ptr(md), N._ptr(inl),
                                    N._ptr(kept), N._ptr(st), N._ptr(lost))
        assert rc == -1
        assert best.value == 7 and (M == 7).all() and (Ma == 7).all() and (md == 7).all()
        assert (inl == 7).all() and (kept == 7).all() and (st == 7).all() and (lost == 7).all()
    S, nn, keep = np.full(16, 7.0), np.full(len(s), 7, np.int32), np.full(len(s), 7, np.uint8)
    k, l = C.c_int64(7), C.c_int64(7)
    rc = N.lib().vcp_icp_sums_unique(vcp_ctx._h, N._ptr(t), C.c_int64(len(t)), N._ptr(s), C.c_int64(len(s)), None, None,
                                     C.c_double(0.0), N._ptr(S), C.byref(k), N._ptr(nn), N._ptr(keep), C.byref(l))
    assert rc == -1 and k.value == 7 and l.value == 7 and (S == 7).all() and (nn == 7).all() and (keep == 7).all()
    # lost is required on the handle, as kept is
    rc = N.lib().vcp_icp_sums_unique(vcp_ctx._h, N._ptr(t), C.c_int64(len(t)), N._ptr(s), C.c_int64(len(s)), None, None,
                                     C.c_double(1.0), N._ptr(S), C.byref(k), N._ptr(nn), N._ptr(keep), None)
    assert rc == -1 and k.value == 7 and (S == 7).all() and (nn == 7).all() and (keep == 7).all()
    rc = N.lib().vcp_icp_sums_unique(vcp_ctx._h, N._ptr(t), C.c_int64(len(t)), N._ptr(s), C.c_int64(len(s)), None, None,
                                     C.c_double(1.0), N._ptr(S), None, N._ptr(nn), N._ptr(keep), C.byref(l))
    assert rc == -1 and l.value == 7 and (S == 7).all()
    # the key holds the landmark in 32 bits (refused before anything is read)
    rc = N.lib().vcp_icp_sums_unique(vcp_ctx._h, N._ptr(t), C.c_int64(len(t)), N._ptr(s), C.c_int64(1 << 32), None, None,
                                     C.c_double(1.0), N._ptr(S), C.byref(k), None, None, C.byref(l))
    assert rc == -5 and (S == 7).all()
    # kept, starved and lost may be NULL, and the context stays usable
    M, best = np.zeros(16), C.c_int32(-1)
    gates = np.array([1.0, 0.5])
    rc = N.lib().vcp_icp_unique(vcp_ctx._h, N._ptr(s), C.c_int64(len(s)), N._ptr(t), C.c_int64(len(t)), C.c_int32(2),
                                None, None, 5, 200, N._ptr(gates), C.c_int32(2), C.c_int32(3), C.c_double(1.0), N._ptr(M),
                                C.byref(best), None, None, None, None, None, None)
    assert rc == 0 and best.value in (0, 1)
    assert _same(M.reshape(4, 4), ui(src, tgt, gates, 2, None, 5, 200, 3, 1.0)["M"])


def test_timing_phases(vcp_ctx):
    tgt, src = _cloud(300, 400, 9)
    vcp_ctx.timing_enable(True)
    try:
        vcp_ctx.icp_unique(src, tgt, [1.0], 2, None, 3, 200, 3, 0.2)
        assert [p[0] for p in vcp_ctx.timing()] == ["icpu_rounds", "icpu_score"]
    finally:
        vcp_ctx.timing_enable(False)
