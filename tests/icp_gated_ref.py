"""Gated ICP (include/vcp.h, "gated ICP"): what the tests of vcp_icp_sums_gated / vcp_icp_gated share.  No GPU here.

  * the scene of the behaviour tests: planar truths, noisy true centroids, a band of clutter beside the truth region,
    everything moved back by a known pose, a start near that pose;
  * ref_icp: a plain numpy binary64 gated ICP (brute-force NN, the header's drop rule, Kabsch fit) -- the REFERENCE of
    the behaviour conditions, independent of the library;
  * conditions(): the behaviour conditions themselves, so that the reference and the device are held to the same ones;
  * gated_terms / gated_sums: icp_sums_ref's terms with the dropped rows zeroed, through its replay of the tree;
  * replay_run: a whole gated run restated round by round from one-pass calls, the host Horn step and the composition
    (the few lines of tests/test_icp_replay_gpu.py it needs are restated here).
"""
import ctypes as C
import math

import numpy as np

import icp_sums_ref as R

# ---- the scene -------------------------------------------------------------------------------------------------------
SIZES = [(40, 32, 12), (300, 240, 80), (600, 500, 150)]   # (truths, true centroids, clutter)
SEEDS = {40: 1, 300: 2, 600: 3}                            # fixed after tests/test_icp_gated.py showed they hold
ROUNDS = 30
MIN_PAIRS = 3
GATE_START, GATE_END, GATE_ROUNDS = 0.6, 0.1, 10
SEPARATION = 0.6
NOISE = 0.01
ANGLE, SHIFT = 2.0, (1.5, -0.8, 0.0)            # the true pose: centroids -> truths
D_ANGLE, D_SHIFT = 0.03, (0.2, -0.15, 0.0)      # the start = the true pose perturbed by these


def rz(a):
    c, s = math.cos(a), math.sin(a)
    return np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])


def scene(nt, ntrue, nclutter, seed):
    """dict: truths [nt,3]; centers [ntrue + nclutter, 3] (shuffled, moved back by the true pose); is_true [n] and
    truth_of [n] (index of a true centroid's truth, -1 for clutter); R_true, T_true; the start R0, T0."""
    rng = np.random.default_rng([seed, nt])
    truths = np.zeros((nt, 3))
    k = 0
    while k < nt:                                 # rejection: pairwise separation > SEPARATION
        c = rng.uniform(0.0, 20.0, 2)
        if k == 0 or ((truths[:k, :2] - c) ** 2).sum(axis=1).min() > SEPARATION ** 2:
            truths[k, :2] = c
            k += 1
    pick = rng.permutation(nt)[:ntrue]
    true_c = truths[pick].copy()
    true_c[:, :2] += rng.normal(0.0, NOISE, (ntrue, 2))
    clutter = np.zeros((nclutter, 3))
    clutter[:, 0] = rng.uniform(21.0, 26.0, nclutter)
    clutter[:, 1] = rng.uniform(0.0, 20.0, nclutter)
    x = np.concatenate([true_c, clutter])
    truth_of = np.concatenate([pick, np.full(nclutter, -1)])
    perm = rng.permutation(len(x))
    x, truth_of = x[perm], truth_of[perm]
    Rt, Tt = rz(ANGLE), np.array(SHIFT)
    centers = np.ascontiguousarray((x - Tt) @ Rt)          # Rt centers + Tt = x
    centers[:, 2] = 0.0
    return dict(truths=np.ascontiguousarray(truths), centers=centers, is_true=truth_of >= 0, truth_of=truth_of,
                R_true=Rt, T_true=Tt, R0=rz(ANGLE + D_ANGLE), T0=Tt + np.array(D_SHIFT))


def schedule():
    from vtkcloudpoint_amd.icp import gate_schedule
    return gate_schedule(GATE_START, GATE_END, GATE_ROUNDS)


# ---- the reference: plain numpy ----------------------------------------------------------------------------------------
def brute_nn(model, p, chunk=4096):
    """(nn, dd): nearest model point of every p by the pass's expression (e0*e0 + e1*e1) + e2*e2 in binary64, lowest
    index among the minima (np.argmin returns the first)."""
    model = np.ascontiguousarray(model, np.float64).reshape(-1, 3)
    nn = np.zeros(len(p), np.int64)
    dd = np.zeros(len(p))
    with np.errstate(all="ignore"):
        for a in range(0, len(p), chunk):
            e = p[a:a + chunk, None, :] - model[None, :, :]
            d = (e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]
            j = np.argmin(d, axis=1)
            nn[a:a + chunk] = j
            dd[a:a + chunk] = d[np.arange(len(j)), j]
    return nn, dd


def kept_mask(dd, gate):
    """The header's rule: dropped iff sqrt(dd) >= gate (a NaN compares false: kept)."""
    with np.errstate(all="ignore"):
        return ~(np.sqrt(dd) >= gate)


def _kabsch(P, Y):
    """The proper rotation and translation that best move P onto Y in the least-squares sense."""
    mp, my = P.mean(axis=0), Y.mean(axis=0)
    U, _, Vt = np.linalg.svd((P - mp).T @ (Y - my))
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(Vt.T @ U.T))])
    Rm = Vt.T @ D @ U.T
    return Rm, my - Rm @ mp


def ref_icp(src, tgt, R0, T0, gates, rounds, min_pairs=MIN_PAIRS):
    """Gated ICP as vcp.h defines it, in numpy: dict(R, T, kept, starved, mean_dist) after `rounds` rounds.  gates None:
    the ungated loop."""
    Rm, T = np.array(R0, np.float64), np.array(T0, np.float64)
    kept, starved, md = 0, 0, math.inf
    for r in range(1, rounds + 1):
        g = math.inf if gates is None else float(gates[min(r, len(gates)) - 1])
        p = src @ Rm.T + T
        nn, dd = brute_nn(tgt, p)
        keep = kept_mask(dd, g)
        kept = int(keep.sum())
        md = math.sqrt(dd[keep].sum() / kept) if kept else math.inf
        if kept < min_pairs:
            starved += 1
            continue
        R1, T1 = _kabsch(p[keep], tgt[nn[keep]])
        Rm, T = R1 @ Rm, R1 @ T + T1
    return dict(R=Rm, T=T, kept=kept, starved=starved, mean_dist=md)


def conditions(sc, Rm, T):
    """(fraction of true centroids within 0.1 of their truth, the pose's largest coordinate error over the true
    centroids) of the pose (Rm, T).  The coordinate error is that of the POSE: where it puts a true centroid against
    where the true pose puts it (the centroids' own noise, sigma 0.01, is no error of the pose)."""
    c = sc["centers"][sc["is_true"]]
    got = c @ np.asarray(Rm).T + np.asarray(T)
    want = c @ sc["R_true"].T + sc["T_true"]
    truth = sc["truths"][sc["truth_of"][sc["is_true"]]]
    within = np.sqrt(((got - truth) ** 2).sum(axis=1)) < 0.1
    return within.mean(), np.abs(got - want).max()


# ---- one pass through the replayed tree ------------------------------------------------------------------------------
def gated_terms(model, data, Rm, T, nn, gate):
    """(terms [nd,16] with the dropped rows +0.0, keep [nd] bool): icp_sums_ref.terms and the drop rule on its SSE
    column, which is dd."""
    t = R.terms(model, data, Rm, T, nn)
    keep = kept_mask(t[:, 15], gate)
    t[~keep] = 0.0
    return t, keep


def gated_sums(model, data, Rm, T, nn, gate):
    """What vcp_icp_sums_gated must return: (sums [16], kept, keep [nd] uint8)."""
    model = np.ascontiguousarray(model, np.float64).reshape(-1, 3)
    data = np.ascontiguousarray(data, np.float64).reshape(-1, 3)
    t, keep = gated_terms(model, data, Rm, T, nn, gate)
    pl = R.plan(len(model), len(data), np.isfinite(model).all())
    return R.replay(t, len(data), pl), int(keep.sum()), keep.astype(np.uint8)


# ---- whole runs, restated from one-pass calls ------------------------------------------------------------------------
def _horn(N, S, n, V):
    R1, T1 = np.zeros(9), np.zeros(3)
    Vb = np.ascontiguousarray(V, np.float64).copy()
    rc = N.lib().vcp_selftest_horn(S.ctypes.data_as(C.c_void_p), C.c_int64(n), Vb.ctypes.data_as(C.c_void_p), C.c_int(1),
                                   R1.ctypes.data_as(C.c_void_p), T1.ctypes.data_as(C.c_void_p))
    assert rc == 1
    return [float(x) for x in R1], [float(x) for x in T1], Vb


def _compose(R1, T1, Rm, T):
    """R <- R1 R, T <- R1 T + T1 in the step's order: row by row, k ascending, acc + T1[i] last."""
    tR, tT = [0.0] * 9, [0.0] * 3
    for i in range(3):
        for j in range(3):
            acc = 0.0
            for k in range(3):
                acc += R1[3 * i + k] * Rm[3 * k + j]
            tR[3 * i + j] = acc
    for i in range(3):
        acc = 0.0
        for k in range(3):
            acc += R1[3 * i + k] * T[k]
        tT[i] = acc + T1[i]
    return tR, tT


def seq_mean(a):
    """Sequential binary64 sums over all points, one division (vcp_icp_vtklike's centroid start)."""
    s = [0.0, 0.0, 0.0]
    for row in a.tolist():
        for c in range(3):
            s[c] += row[c]
    return [s[c] / float(len(a)) for c in range(3)]


def landmarks(src, ml):
    ns = len(src)
    step = ns // ml if ns > ml else 1
    return np.ascontiguousarray(src[::step][: ns // step])


def replay_run(ctx, N, tgt, lm, R0, T0, gates, rounds, min_pairs=MIN_PAIRS):
    """[per round: dict(M [4,4], mean_dist, kept, starved)]: each round is icp_sums_gated at that round's gate from
    the state so far, then -- unless starved -- the host Horn step on (sums, kept) with the carried basis and the
    composition."""
    Rm = [float(x) for x in np.asarray(R0).reshape(9)]
    T = [float(x) for x in np.asarray(T0).reshape(3)]
    V = np.zeros(16)
    starved = 0
    out = []
    for r in range(1, rounds + 1):
        g = float(gates[min(r, len(gates)) - 1])
        S, kept, _, _ = ctx.icp_sums_gated(tgt, lm, g, np.array(Rm).reshape(3, 3), np.array(T), want_nn=False,
                                           want_keep=False)
        if kept < min_pairs:
            starved += 1
        else:
            R1, T1, V = _horn(N, S, kept, V)
            Rm, T = _compose(R1, T1, Rm, T)
        M = np.eye(4)
        M[:3, :3] = np.array(Rm).reshape(3, 3)
        M[:3, 3] = T
        out.append(dict(M=M, mean_dist=math.sqrt(float(S[15]) / kept) if kept else math.inf, kept=kept, starved=starved))
    return out
