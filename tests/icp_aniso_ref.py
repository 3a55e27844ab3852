"""Anisotropic ICP (include/vcp.h, "anisotropic ICP"): what the tests of vcp_icp_sums_aniso / vcp_selftest_horn_aniso /
vcp_icp_aniso share.  No GPU here.

  * aniso_terms / aniso_sums: the gated terms of tests/icp_gated_ref.py with the d-side columns taken from the RAW landmark
    and the two columns of the scales, through icp_sim_ref.replay18 (the tree of all 18 columns);
  * step: the step of the header restated in Python floats, one operation per operator, on top of the rotation
    vcp_selftest_horn returns for the scaled sums S';
  * exact_s / s_bound: the exact rational g_a / D_a of given sums and the bound of DESIGN.md section 25 on the computed one;
  * aniso_scene: icp_gated_ref's behaviour scene with the centroids' x and y in two other units and a start whose two
    scales are off;
  * ref_icp: a plain numpy anisotropic ICP (brute-force NN, the drop rule, the per-axis least-squares scale, Kabsch, the
    clamp) -- the REFERENCE of the behaviour conditions, independent of the library;
  * replay_run: a whole run restated round by round from one-pass calls and the host step, which SETS the pose.
"""
import math
from fractions import Fraction

import numpy as np

import icp_gated_ref as G
import icp_sim_ref as S
import icp_sums_ref as R

K_XY = (2.5, 2.2)                       # the truths' unit over the centroids', per axis
START_ERRORS = ((0.02, -0.02), (0.03, 0.0), (0.0, 0.0))
WRONG_STARTS = START_ERRORS[:2]
RATIO = (0.9, 1.1)
U = Fraction(1, 2 ** 53)
INF = math.inf


# ---- one pass through the replayed tree ------------------------------------------------------------------------------
def aniso_terms(model, data, A, T, nn, gate):
    """(terms [nd, 18] with the dropped rows +0.0, keep [nd] bool).  Pair, dd (column 15) and the drop rule are
    icp_gated_ref's under the pose (A, T); columns 0:3 are d, 3:6 y, 6 + 3r + c is d_r * y_c, 16 is d0*d0, 17 d1*d1, each
    operation one binary64 ufunc call."""
    model = np.ascontiguousarray(model, np.float64).reshape(-1, 3)
    d = np.ascontiguousarray(data, np.float64).reshape(-1, 3)
    t16 = R.terms(model, d, A, T, nn)
    keep = G.kept_mask(t16[:, 15], gate)
    y = t16[:, 3:6]
    t = np.empty((len(d), 18))
    with np.errstate(all="ignore"):
        t[:, 0:3] = d
        t[:, 3:6] = y
        for r in range(3):
            for c in range(3):
                t[:, 6 + 3 * r + c] = d[:, r] * y[:, c]
        t[:, 15] = t16[:, 15]
        t[:, 16] = d[:, 0] * d[:, 0]
        t[:, 17] = d[:, 1] * d[:, 1]
    t[~keep] = 0.0
    return t, keep


def aniso_sums(model, data, A, T, nn, gate):
    """What vcp_icp_sums_aniso must return: (sums [18], kept, keep [nd] uint8)."""
    model = np.ascontiguousarray(model, np.float64).reshape(-1, 3)
    data = np.ascontiguousarray(data, np.float64).reshape(-1, 3)
    t, keep = aniso_terms(model, data, A, T, nn, gate)
    pl = R.plan(len(model), len(data), np.isfinite(model).all())
    return S.replay18(t, len(data), pl), int(keep.sum()), keep.astype(np.uint8)


def case_sums(path, nm, nd, family, pose="generic"):
    """(sums [18], n, rotation [9 floats]) of one icp_sums_ref.case, all pairs kept, nearest neighbours by brute force:
    inputs of the step.  The rotation is the case's pose (the identity for pose "none")."""
    model, data, Rm, T = R.case(path, nm, nd, family, pose)
    nn, _ = G.brute_nn(model, R.transform(data, Rm, T))
    Ssum, kept, _ = aniso_sums(model, data, Rm, T, nn, INF)
    rot = np.eye(3) if Rm is None else np.asarray(Rm, np.float64)
    return Ssum, kept, [float(x) for x in rot.reshape(9)]


# ---- the step --------------------------------------------------------------------------------------------------------
def _f(x):
    return np.float64(x)


def scales(Ssum, n, Rm, s, lo, hi):
    """Steps 1 and 2 of the header in binary64, one operation per operator: (s' [2 floats], determined bit mask)."""
    Sv = [_f(x) for x in Ssum]
    N_ = _f(float(n))
    out, det = [], 0
    with np.errstate(all="ignore"):
        muY = [Sv[3 + b] / N_ for b in range(3)]
        for a in range(2):
            muD = Sv[a] / N_
            C = [Sv[6 + 3 * a + b] / N_ - muD * muY[b] for b in range(3)]
            D = Sv[16 + a] / N_ - muD * muD
            g = (_f(Rm[a]) * C[0] + _f(Rm[3 + a]) * C[1]) + _f(Rm[6 + a]) * C[2]
            v = float(s[a])
            if 0.0 < D < INF and 0.0 < g < INF:
                v = float(g / D)
                v = float(lo[a]) if v < lo[a] else float(hi[a]) if v > hi[a] else v
                det |= 1 << a
            out.append(v)
    return out, det


def scaled_sums(Ssum, sp):
    """Step 3: S' [16], rows 0 and 1 of the d-side times s'."""
    Sp = np.array(Ssum[:16], np.float64)
    with np.errstate(all="ignore"):
        for a in range(2):
            Sp[a] = _f(sp[a]) * _f(Ssum[a])
            for b in range(3):
                Sp[6 + 3 * a + b] = _f(sp[a]) * _f(Ssum[6 + 3 * a + b])
    return Sp


def step(N, Ssum, n, Rm, s, lo, hi, V=None):
    """The header's step: (rc, R_new [9], T_new [3], s_new [2], determined, A_new [9]); rc 0: the others are None.  The
    rotation of S' is vcp_selftest_horn's (icp_sim_ref.horn: V is updated in place when given); T_new is restated from it."""
    sp, det = scales(Ssum, n, Rm, s, lo, hi)
    Sp = scaled_sums(Ssum, sp)
    rc, R1, T1h = S.horn(N, Sp, n, V)
    if rc != 1:
        return 0, None, None, None, None, None
    with np.errstate(all="ignore"):
        N_ = _f(float(n))
        muP = [_f(Sp[a]) / N_ for a in range(3)]
        muY = [_f(Sp[3 + a]) / N_ for a in range(3)]
        T1 = [float(muY[i] - ((_f(R1[3 * i]) * muP[0] + _f(R1[3 * i + 1]) * muP[1]) + _f(R1[3 * i + 2]) * muP[2]))
              for i in range(3)]
    assert np.array(T1).tobytes() == np.array(T1h).tobytes()        # horn's own expression
    return 1, R1, T1, sp, det, pose_matrix(R1, sp)


def pose_matrix(Rm, s):
    """Step 5: A[3i+a] = R[3i+a] * s_a for a = 0, 1, A[3i+2] = R[3i+2], in Python floats."""
    A = [float(x) for x in Rm]
    for i in range(3):
        for a in range(2):
            A[3 * i + a] = float(_f(Rm[3 * i + a]) * _f(s[a]))
    return A


# ---- the scales against exact arithmetic -------------------------------------------------------------------------------
def exact_s(Ssum, n, Rm):
    """Per axis (g / D, q, p) as Fractions from the same doubles with no rounding, or None where the exact D or g is not
    positive: q = (sums[16+a]/N) / D, p = sum_b |R[3b+a]| (|sums[6+3a+b]/N| + |muD_a muY_b|) / g."""
    Sv = [Fraction(float(x)) for x in Ssum]
    N_ = Fraction(int(n))
    out = []
    for a in range(2):
        muD = Sv[a] / N_
        muY = [Sv[3 + b] / N_ for b in range(3)]
        D = Sv[16 + a] / N_ - muD * muD
        Rc = [Fraction(float(Rm[3 * b + a])) for b in range(3)]
        g = sum(Rc[b] * (Sv[6 + 3 * a + b] / N_ - muD * muY[b]) for b in range(3))
        if D <= 0 or g <= 0:
            out.append(None)
            continue
        P = sum(abs(Rc[b]) * (abs(Sv[6 + 3 * a + b] / N_) + abs(muD * muY[b])) for b in range(3))
        out.append((g / D, (Sv[16 + a] / N_) / D, P / g))
    return out


# DESIGN.md section 25.  With Q = sums[16+a]/N, E = muD^2 <= Q (D > 0): the computed D carries u Q (the division), 3 u E
# (muD twice, the product) and its own rounding: |D^/D - 1| <= u (1 + 4 q) to first order.  A computed C_ab carries
# u |X/N| + 3 u |muD muY| + u |C| <= 4 u (|X/N| + |muD muY|); its product with R and the two additions of g add
# 3 u |R C|: |g^/g - 1| <= 7 u p.  The quotient adds u.  First order: u (2 + 4 q + 7 p).  The constants below leave
# u (1 + q + p) for the higher-order terms, which are below 2^-9 of the first-order sum inside the domain.
S_A, S_B, S_C = 3, 5, 8
S_VALID = Fraction(1, 2 ** 12)         # the domain: u (q + p) <= 2^-12, no overflow, no underflow


def s_bound(q, p):
    """|s^ / s - 1| <= u (S_A + S_B q + S_C p), or None outside the domain (D or g has all but cancelled)."""
    if U * (q + p) > S_VALID:
        return None
    return U * (S_A + S_B * q + S_C * p)


# ---- the behaviour scene in two other units ----------------------------------------------------------------------------
def aniso_scene(nt, ntrue, nclutter, seed, err, K=K_XY):
    """icp_gated_ref.scene with the centroids' x divided by K[0] and y by K[1] (so the true pose is R_true diag(K, 1),
    T_true) and a start whose scales are wrong by the fractions err: rotation R0 = the scene's, s0 = K (1 + err), and T0
    such that the mean of the true centroids lands where the scene's own start puts it.  A0 = R0 diag(s0, 1) is the start
    matrix a loop without scales is given."""
    sc = dict(G.scene(nt, ntrue, nclutter, seed))
    m = sc["centers"][sc["is_true"]].mean(axis=0)
    where = sc["R0"] @ m + sc["T0"]
    k3 = np.array([K[0], K[1], 1.0])
    sc["centers"] = np.ascontiguousarray(sc["centers"] / k3)
    sc["R_true"] = sc["R_true"] * k3            # columns scaled: R diag(K, 1)
    sc["s0"] = np.array([K[0] * (1.0 + err[0]), K[1] * (1.0 + err[1])])
    sc["A0"] = sc["R0"] * np.array([sc["s0"][0], sc["s0"][1], 1.0])
    sc["T0"] = where - sc["A0"] @ (m / k3)
    return sc


# ---- the reference: plain numpy --------------------------------------------------------------------------------------
def ref_icp(src, tgt, R0, s0, T0, gates, rounds, ratio=RATIO, min_pairs=G.MIN_PAIRS):
    """Anisotropic ICP as vcp.h defines it, in numpy: dict(A, R, s, T, kept, starved, mean_dist, unscaled [2]) after
    `rounds` rounds.  A round's fit is, per axis, the least-squares scale for the current rotation (held in ratio times the
    start), then Kabsch's rotation of the scaled kept landmarks."""
    Rm, T = np.array(R0, np.float64), np.array(T0, np.float64)
    s = np.array(s0, np.float64)
    lo, hi = ratio[0] * s, ratio[1] * s
    kept, starved, md, unscaled = 0, 0, INF, [0, 0]
    for r in range(1, rounds + 1):
        g = float(gates[min(r, len(gates)) - 1])
        A = Rm * np.array([s[0], s[1], 1.0])
        p = src @ A.T + T
        nn, dd = G.brute_nn(tgt, p)
        keep = G.kept_mask(dd, g)
        kept = int(keep.sum())
        md = math.sqrt(dd[keep].sum() / kept) if kept else INF
        if kept < min_pairs:
            starved += 1
            continue
        Dk, Y = src[keep], tgt[nn[keep]]
        dc, yc = Dk - Dk.mean(axis=0), Y - Y.mean(axis=0)
        for a in range(2):
            num = float((dc[:, a] * (yc @ Rm[:, a])).sum())
            den = float((dc[:, a] ** 2).sum())
            if 0.0 < den < INF and 0.0 < num < INF:
                s[a] = min(max(num / den, lo[a]), hi[a])
            else:
                unscaled[a] += 1
        k3 = np.array([s[0], s[1], 1.0])
        Rm, T = G._kabsch(Dk * k3, Y)
    return dict(A=Rm * np.array([s[0], s[1], 1.0]), R=Rm, s=s, T=T, kept=kept, starved=starved, mean_dist=md,
                unscaled=unscaled)


# ---- whole runs, restated from one-pass calls ------------------------------------------------------------------------
def replay_run(ctx, N, tgt, lm, R0, s0, T0, gates, rounds, ratio=RATIO, min_pairs=G.MIN_PAIRS):
    """[per round: dict(M [4,4], mean_dist, kept, starved, scale [2], unscaled [2])]: each round is icp_sums_aniso at that
    round's gate under the pose so far, then -- unless starved -- vcp_selftest_horn_aniso on (sums, kept) with the carried
    basis, rotation and scales; its results ARE the new pose."""
    Rm = [float(x) for x in np.asarray(R0).reshape(9)]
    s = [float(x) for x in np.asarray(s0).reshape(2)]
    lo, hi = [ratio[0] * s[0], ratio[0] * s[1]], [ratio[1] * s[0], ratio[1] * s[1]]
    A = pose_matrix(Rm, s)
    T = [float(x) for x in np.asarray(T0).reshape(3)]
    V = np.zeros(16)
    starved, unscaled = 0, [0, 0]
    out = []
    for r in range(1, rounds + 1):
        g = float(gates[min(r, len(gates)) - 1])
        Ssum, kept, _, _ = ctx.icp_sums_aniso(tgt, lm, g, np.array(A).reshape(3, 3), np.array(T), want_nn=False,
                                              want_keep=False)
        if kept < min_pairs:
            starved += 1
        else:
            h = N.selftest_horn_aniso(Ssum, kept, Rm, s, lo, hi, V)
            assert h["rc"] == 1
            for a in range(2):
                unscaled[a] += 0 if h["determined"] >> a & 1 else 1
            Rm, s, T = h["R_new"].tolist(), h["s_new"].tolist(), h["T_new"].tolist()
            A = pose_matrix(Rm, s)
        M = np.eye(4)
        M[:3, :3] = np.array(A).reshape(3, 3)
        M[:3, 3] = T
        out.append(dict(M=M, mean_dist=math.sqrt(float(Ssum[15]) / kept) if kept else INF, kept=kept, starved=starved,
                        scale=list(s), unscaled=list(unscaled)))
    return out
