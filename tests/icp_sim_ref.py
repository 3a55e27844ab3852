"""Similarity ICP (include/vcp.h, "similarity ICP"): what the tests of vcp_icp_sums_sim / vcp_selftest_horn_sim /
vcp_icp_sim share.  No GPU here.

  * sim_terms / sim_sums: the gated terms of tests/icp_gated_ref.py with the two columns of the scale, through
    icp_sums_ref's replay of the tree (which takes 16 columns and treats every column alike: the two new ones ride in a
    second 16-wide array);
  * step: the step of the header restated in Python floats on top of the rotation vcp_selftest_horn returns;
  * exact_k2 / k_bound: the exact rational vY / vP of given sums and the bound of DESIGN.md section 22 on the computed k;
  * scaled_scene: icp_gated_ref's behaviour scene with the centroids in another unit and a start whose scale is off;
  * ref_icp: a plain numpy similarity ICP (brute-force NN, the drop rule, Kabsch plus Horn's symmetric scale, the
    clamp) -- the REFERENCE of the behaviour conditions, independent of the library;
  * replay_run: a whole run restated round by round from one-pass calls, the host step and the composition.
"""
import ctypes as C
import math
from fractions import Fraction

import numpy as np

import icp_gated_ref as G
import icp_sums_ref as R

K_UNIT = 2.5                          # the truths' unit over the centroids'
START_ERRORS = (0.0, 0.01, 0.02, 0.05)
RATIO_RANGE = (0.9, 1.1)
U = Fraction(1, 2 ** 53)


# ---- one pass through the replayed tree ------------------------------------------------------------------------------
def sim_terms(model, data, Rm, T, nn, gate):
    """(terms [nd, 18] with the dropped rows +0.0, keep [nd] bool).  Columns 0:16 are icp_gated_ref.gated_terms';
    16 is (p0*p0 + p1*p1) + p2*p2 and 17 the same of y, each operation one binary64 ufunc call."""
    t16 = R.terms(model, data, Rm, T, nn)
    keep = G.kept_mask(t16[:, 15], gate)
    p, y = t16[:, 0:3], t16[:, 3:6]
    t = np.empty((len(t16), 18))
    t[:, :16] = t16
    with np.errstate(all="ignore"):
        t[:, 16] = (p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1]) + p[:, 2] * p[:, 2]
        t[:, 17] = (y[:, 0] * y[:, 0] + y[:, 1] * y[:, 1]) + y[:, 2] * y[:, 2]
    t[~keep] = 0.0
    return t, keep


def replay18(t, nd, pl):
    """The 18 sums of terms t [nd, 18] in the kernels' order: icp_sums_ref.replay on columns 0:16, and once more on a
    16-wide array that carries columns 16 and 17 in its first two places (every column goes through the same tree)."""
    extra = np.zeros((nd, 16))
    extra[:, 0:2] = t[:, 16:18]
    return np.concatenate([R.replay(np.ascontiguousarray(t[:, :16]), nd, pl), R.replay(extra, nd, pl)[0:2]])


def sim_sums(model, data, Rm, T, nn, gate):
    """What vcp_icp_sums_sim must return: (sums [18], kept, keep [nd] uint8)."""
    model = np.ascontiguousarray(model, np.float64).reshape(-1, 3)
    data = np.ascontiguousarray(data, np.float64).reshape(-1, 3)
    t, keep = sim_terms(model, data, Rm, T, nn, gate)
    pl = R.plan(len(model), len(data), np.isfinite(model).all())
    return replay18(t, len(data), pl), int(keep.sum()), keep.astype(np.uint8)


def case_sums(path, nm, nd, family, pose="generic"):
    """(sums [18], n) of one icp_sums_ref.case, all pairs kept, nearest neighbours by brute force: inputs of the step."""
    model, data, Rm, T = R.case(path, nm, nd, family, pose)
    nn, _ = G.brute_nn(model, R.transform(data, Rm, T))
    S, kept, _ = sim_sums(model, data, Rm, T, nn, math.inf)
    return S, kept


# ---- the step --------------------------------------------------------------------------------------------------------
def horn(N, S, n, V=None):
    """vcp_selftest_horn on S[0:16]: (rc, R1 [9 floats], T1 [3 floats]); V [16] is updated in place when given."""
    S16 = np.ascontiguousarray(np.asarray(S, np.float64)[:16])
    R1, T1 = np.zeros(9), np.zeros(3)
    rc = N.lib().vcp_selftest_horn(S16.ctypes.data_as(C.c_void_p), C.c_int64(n),
                                   None if V is None else V.ctypes.data_as(C.c_void_p), C.c_int(0 if V is None else 1),
                                   R1.ctypes.data_as(C.c_void_p), T1.ctypes.data_as(C.c_void_p))
    return rc, [float(x) for x in R1], [float(x) for x in T1]


def step(S, n, R1, c, ratio_min, ratio_max):
    """The header's step in Python floats, given horn()'s rotation R1 of the same sums: (rc, R1s [9], T1 [3], k_used,
    c_new).  Every line is one binary64 operation per operator; math.sqrt is correctly rounded."""
    S = [float(x) for x in S]
    N_ = float(n)
    muP = [S[a] / N_ for a in range(3)]
    muY = [S[3 + a] / N_ for a in range(3)]
    with np.errstate(all="ignore"):
        S16, S17 = np.float64(S[16]), np.float64(S[17])     # numpy scalars: inf - inf is NaN, not an exception
        vP = float(S16 / np.float64(N_) - np.float64((muP[0] * muP[0] + muP[1] * muP[1]) + muP[2] * muP[2]))
        vY = float(S17 / np.float64(N_) - np.float64((muY[0] * muY[0] + muY[1] * muY[1]) + muY[2] * muY[2]))
    det = 0.0 < vP < math.inf and 0.0 < vY < math.inf
    k_used, c_new = 1.0, c
    if det:
        with np.errstate(all="ignore"):
            k = float(np.sqrt(np.float64(vY) / np.float64(vP)))
            t = float(np.float64(c) * np.float64(k))
        if t < ratio_min:
            c_new, k_used = ratio_min, ratio_min / c
        elif t > ratio_max:
            c_new, k_used = ratio_max, ratio_max / c
        else:
            c_new, k_used = t, k
    R1s = [k_used * R1[j] for j in range(9)]
    T1 = [muY[i] - ((R1s[3 * i] * muP[0] + R1s[3 * i + 1] * muP[1]) + R1s[3 * i + 2] * muP[2]) for i in range(3)]
    return (1 if det else 2), R1s, T1, k_used, c_new


def exact_k2(S, n):
    """(vY / vP, qP, qY) as Fractions from finite sums: v = S/N - |s/N|^2 with no rounding, q = (S/N) / v.  None when
    the exact vP or vY is not positive (the scale is not determined)."""
    S = [Fraction(float(x)) for x in S]
    n = Fraction(int(n))
    eP = sum((S[a] / n) ** 2 for a in range(3))
    eY = sum((S[3 + a] / n) ** 2 for a in range(3))
    vP, vY = S[16] / n - eP, S[17] / n - eY
    if vP <= 0 or vY <= 0:
        return None
    return vY / vP, (S[16] / n) / vP, (S[17] / n) / vY


K_A, K_B = 3, 4          # |k^ / k - 1| <= u (K_A + K_B (qP + qY)) while u (qP + qY) <= 2^-12
K_VALID = Fraction(1, 2 ** 12)


def k_bound(qP, qY):
    """The bound, or None outside its domain (the spread has all but cancelled: nothing is promised there)."""
    if U * (qP + qY) > K_VALID:
        return None
    return U * (K_A + K_B * (qP + qY))


# ---- the behaviour scene in another unit -----------------------------------------------------------------------------
def scaled_scene(nt, ntrue, nclutter, seed, err, K=K_UNIT):
    """icp_gated_ref.scene with the centroids divided by K (so the true pose is the similarity K R_true, T_true) and
    the scene's start pose with its scale wrong by the fraction err: R0 = K (1 + err) R0', and T0 such that the mean of
    the true centroids lands where the scene's own start puts it."""
    sc = dict(G.scene(nt, ntrue, nclutter, seed))
    m = sc["centers"][sc["is_true"]].mean(axis=0)
    where = sc["R0"] @ m + sc["T0"]
    sc["centers"] = np.ascontiguousarray(sc["centers"] / K)
    sc["R_true"] = K * sc["R_true"]
    sc["R0"] = (K * (1.0 + err)) * sc["R0"]
    sc["T0"] = where - sc["R0"] @ (m / K)
    return sc


def linear_scale(Rm):
    Rm = np.asarray(Rm)
    return math.sqrt(abs(float(Rm[0, 0] * Rm[1, 1] - Rm[0, 1] * Rm[1, 0])))


# ---- the reference: plain numpy --------------------------------------------------------------------------------------
def ref_icp(src, tgt, R0, T0, gates, rounds, ratio_range, min_pairs=G.MIN_PAIRS):
    """Similarity ICP as vcp.h defines it, in numpy: dict(R, T, kept, starved, mean_dist, ratio, unscaled) after
    `rounds` rounds.  The fit of a round is Kabsch's rotation and Horn's symmetric scale of the kept pairs, the product
    of the scales held in ratio_range."""
    lo, hi = ratio_range
    Rm, T = np.array(R0, np.float64), np.array(T0, np.float64)
    kept, starved, unscaled, md, c = 0, 0, 0, math.inf, 1.0
    for r in range(1, rounds + 1):
        g = float(gates[min(r, len(gates)) - 1])
        p = src @ Rm.T + T
        nn, dd = G.brute_nn(tgt, p)
        keep = G.kept_mask(dd, g)
        kept = int(keep.sum())
        md = math.sqrt(dd[keep].sum() / kept) if kept else math.inf
        if kept < min_pairs:
            starved += 1
            continue
        P, Y = p[keep], tgt[nn[keep]]
        R1, _ = G._kabsch(P, Y)
        mp, my = P.mean(axis=0), Y.mean(axis=0)
        vP, vY = ((P - mp) ** 2).sum(), ((Y - my) ** 2).sum()
        k = 1.0
        if 0.0 < vP < math.inf and 0.0 < vY < math.inf:
            k = math.sqrt(vY / vP)
            cn = min(max(c * k, lo), hi)
            k, c = (k, cn) if cn == c * k else (cn / c, cn)
        else:
            unscaled += 1
        R1 = k * R1
        Rm, T = R1 @ Rm, R1 @ T + (my - R1 @ mp)
    return dict(R=Rm, T=T, kept=kept, starved=starved, mean_dist=md, ratio=c, unscaled=unscaled)


# ---- whole runs, restated from one-pass calls ------------------------------------------------------------------------
def replay_run(ctx, N, tgt, lm, R0, T0, gates, rounds, ratio_range, min_pairs=G.MIN_PAIRS):
    """[per round: dict(M [4,4], mean_dist, kept, starved, ratio, unscaled)]: each round is icp_sums_sim at that round's
    gate from the state so far, then -- unless starved -- vcp_selftest_horn_sim on (sums, kept, c) with the carried
    basis and icp_gated_ref's composition."""
    Rm = [float(x) for x in np.asarray(R0).reshape(9)]
    T = [float(x) for x in np.asarray(T0).reshape(3)]
    V = np.zeros(16)
    starved, unscaled, c = 0, 0, 1.0
    out = []
    for r in range(1, rounds + 1):
        g = float(gates[min(r, len(gates)) - 1])
        S, kept, _, _ = ctx.icp_sums_sim(tgt, lm, g, np.array(Rm).reshape(3, 3), np.array(T), want_nn=False,
                                         want_keep=False)
        if kept < min_pairs:
            starved += 1
        else:
            h = N.selftest_horn_sim(S, kept, c, ratio_range, V)
            assert h["rc"] in (1, 2)
            unscaled += h["rc"] == 2
            c = h["c_new"]
            Rm, T = G._compose([float(x) for x in h["R1s"]], [float(x) for x in h["T1"]], Rm, T)
        M = np.eye(4)
        M[:3, :3] = np.array(Rm).reshape(3, 3)
        M[:3, 3] = T
        out.append(dict(M=M, mean_dist=math.sqrt(float(S[15]) / kept) if kept else math.inf, kept=kept, starved=starved,
                        ratio=c, unscaled=unscaled))
    return out
