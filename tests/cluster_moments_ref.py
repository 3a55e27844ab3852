"""vcp_cluster_moments' definition (include/vcp.h) restated in numpy binary64: the sums through the centroid tree of
centroid_ref (stated once, there), the eigen-solve as the operation sequence of csrc/symeig.hpp on numpy float64 scalars,
the derived numbers; the exact covariance in rational arithmetic, the a-priori bound of DESIGN.md section 33, and the
inputs of the tests.  No GPU, no oracle.  Every numpy operation is one binary64 ufunc call; numpy contracts nothing."""
from fractions import Fraction

import numpy as np

import centroid_ref as CR

U = CR.U
SWEEPS = 32          # SYMEIG_SWEEPS
F = np.float64


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def canon(a):
    """Every NaN as 0x7FF8000000000000, which is what the library writes."""
    a = np.array(a, np.float64)
    a[np.isnan(a)] = np.nan
    return a


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype.kind == "f":
        return a.shape == b.shape and np.array_equal(bits(a), bits(b))
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b)


def npk(dim):
    return dim * (dim + 1) // 2


def pack(S):
    S = np.asarray(S, np.float64)
    return np.ascontiguousarray(S[np.triu_indices(S.shape[0])])


def unpack(s):
    s = np.asarray(s, np.float64)
    D = {3: 2, 6: 3}[len(s)]
    S = np.zeros((D, D))
    S[np.triu_indices(D)] = s
    return S + np.triu(S, 1).T


# ---- the solver: csrc/symeig.hpp, step by step ---------------------------------------------------------------------------
def _rot(A, V, p, q, D):
    apq = A[p][q]
    if apq == 0.0:
        return
    theta = (A[q][q] - A[p][p]) / (F(2.0) * apq)
    t = (F(1.0) if theta >= 0 else F(-1.0)) / (np.abs(theta) + np.sqrt(theta * theta + F(1.0)))
    c = F(1.0) / np.sqrt(t * t + F(1.0))
    s = t * c
    h = t * apq
    A[p][p] = A[p][p] - h
    A[q][q] = A[q][q] + h
    A[p][q] = A[q][p] = F(0.0)
    if D == 3:
        r = 3 - p - q
        x, y = A[r][p], A[r][q]
        A[r][p] = A[p][r] = c * x - s * y
        A[r][q] = A[q][r] = s * x + c * y
    for k in range(D):
        x, y = V[k][p], V[k][q]
        V[k][p] = c * x - s * y
        V[k][q] = s * x + c * y


def sym_eig(S):
    """S: symmetric [D, D] (the upper triangle is read) or packed.  Returns (eval [D], evec [D, D] rows, sweeps)."""
    S = np.asarray(S, np.float64)
    if S.ndim == 1:
        S = unpack(S)
    D = S.shape[0]
    up = [S[r, c] for r in range(D) for c in range(r, D)]
    if not np.all(np.isfinite(up)):
        return np.full(D, np.nan), np.full((D, D), np.nan), 0
    with np.errstate(all="ignore"):
        g = F(0.0)
        for x in up:
            g = np.abs(x) if np.abs(x) > g else g
        e = int(np.frexp(g)[1])
        A = [[np.ldexp(F(S[min(r, c), max(r, c)]), -e) for c in range(D)] for r in range(D)]
        V = [[F(1.0) if r == c else F(0.0) for c in range(D)] for r in range(D)]
        sweeps = 0
        while sweeps < SWEEPS:
            if all(A[r][c] == 0.0 for r in range(D) for c in range(r + 1, D)):
                break
            _rot(A, V, 0, 1, D)
            if D == 3:
                _rot(A, V, 0, 2, D)
                _rot(A, V, 1, 2, D)
            sweeps += 1
        lam = [np.ldexp(A[i][i], e) + F(0.0) for i in range(D)]
    ev, vec = np.zeros(D), np.zeros((D, D))
    for i in range(D):
        rank = sum(1 for k in range(D) if lam[k] > lam[i] or (lam[k] == lam[i] and k < i))
        v = [V[k][i] for k in range(D)]
        big, neg = np.abs(v[0]), v[0] < 0.0
        for k in range(1, D):
            if np.abs(v[k]) > big:
                big, neg = np.abs(v[k]), v[k] < 0.0
        ev[rank] = lam[i]
        vec[rank] = [-x if neg else x for x in v]
    return ev, vec, sweeps


def shape_of(ev, vec):
    D = len(ev)
    if np.isnan(ev[0]):
        return np.full(4, np.nan)
    with np.errstate(all="ignore"):
        s0 = np.sqrt(ev[0] if ev[0] > 0.0 else F(0.0))
        s1 = np.sqrt(ev[1] if ev[1] > 0.0 else F(0.0))
        if D == 3:
            tot = (F(ev[0]) + F(ev[1])) + F(ev[2])
            flat = F(0.0) if tot == 0.0 else F(ev[2]) / tot
            return np.array([s0, s1, flat, np.abs(vec[2, 2])])
    return np.array([s0, s1, 0.0, 1.0])


# ---- the restatement -------------------------------------------------------------------------------------------------------
def moments(pts, labels, K, weights=None):
    """pts [n, D] (D = 2 or 3: the columns the call reads), labels [n] in 0..K, weights int or None.  Returns the dict
    Context.cluster_moments returns, plus S [K, D (D + 1) / 2]: the sums of step 4 before the division."""
    pts = np.ascontiguousarray(pts, np.float64)
    n, D = pts.shape
    labels = np.ascontiguousarray(labels, np.int32)
    idx = CR._members(labels, K)
    wi = np.ones(n, np.int64) if weights is None else np.asarray(weights, np.int64)
    w = wi.astype(np.float64)
    pairs = [(a, b) for a in range(D) for b in range(a, D)]
    with np.errstate(all="ignore"):
        s1, _ = CR._tree_sums(pts * w[:, None], idx, CR.KERNEL)
        W = np.array([int(wi[ix].sum()) for ix in idx], np.int64).reshape(K)
        Wd = W.astype(np.float64)
        mean = s1 / Wd[:, None]
        d = pts - mean[np.maximum(labels, 1) - 1] if K > 0 else pts * 0.0    # rows of label 0: never summed
        wd = w[:, None] * d
        prod = np.stack([wd[:, a] * d[:, b] for a, b in pairs], axis=1) if n else np.zeros((0, len(pairs)))
        S, _ = CR._tree_sums(prod, idx, CR.KERNEL)
        cov = S / Wd[:, None]
    ev, vec, shp = np.zeros((K, D)), np.zeros((K, D, D)), np.zeros((K, 4))
    for k in range(K):
        ev[k], vec[k], _ = sym_eig(cov[k])
        shp[k] = shape_of(ev[k], vec[k])
    valid = ((W >= 2) & np.isfinite(mean).all(1) & np.isfinite(cov).all(1)).astype(np.uint8)
    return dict(mean=canon(mean), cov=canon(cov), eval=canon(ev), evec=canon(vec), shape=canon(shp), valid=valid,
                counts=W, S=S)


KEYS = ("mean", "cov", "eval", "evec", "shape", "valid", "counts")


def differs(got, want, keys=KEYS):
    """None, or the first output whose bits differ with the clusters (0-based) at which they do."""
    for k in keys:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        if g.shape != w.shape:
            return "%s: shape %s, want %s" % (k, g.shape, w.shape)
        ne = bits(g) != bits(w) if w.dtype.kind == "f" else g.astype(np.int64) != w.astype(np.int64)
        if ne.any():
            return "%s at clusters %s" % (k, sorted(set(np.nonzero(ne)[0].tolist()))[:8])
    return None


# ---- exact arithmetic --------------------------------------------------------------------------------------------------------
def _split(x):
    """x = hi + lo exactly, both of at most 26 significant bits (Veltkamp): products of two such are exact in binary64."""
    c = 134217729.0 * x
    hi = c - (c - x)
    return hi, x - hi


def _exact_dot(x, y, w=None):
    """sum(w x y) of finite binary64 x, y (w integers or None) as a Fraction: four exact partial products, each summed by
    centroid_ref._exact_int_sum.  The magnitudes must stay clear of overflow and of the subnormals."""
    xh, xl = _split(np.asarray(x, np.float64))
    yh, yl = _split(np.asarray(y, np.float64))
    return sum((CR._exact_int_sum(p, w) for p in (xh * yh, xh * yl, xl * yh, xl * yl)), Fraction(0))


def exact_cov(pts, labels, K, w=None):
    """[K] of (W, mu [D] Fractions, C {(a, b): Fraction}) or None where the total weight is 0: the population covariance
    sum w (x - mu)(x - mu)^T / W of the finite inputs, no rounding anywhere."""
    pts = np.asarray(pts, np.float64)
    D = pts.shape[1]
    out = []
    for ix in CR._members(labels, K):
        wk = None if w is None else np.asarray(w, np.int64)[ix]
        W = len(ix) if w is None else int(wk.sum())
        if W == 0:
            out.append(None)
            continue
        mu = [CR._exact_int_sum(pts[ix, a], wk) / W for a in range(D)]
        C = {(a, b): _exact_dot(pts[ix, a], pts[ix, b], wk) / W - mu[a] * mu[b] for a in range(D) for b in range(a, D)}
        out.append((W, mu, C))
    return out


def cov_bound(pts, labels, K, w=None, ex=None):
    """[K] of {(a, b): Fraction} with |cov_ab - C_ab| <= it for the restatement, None where the
    total weight is 0:
        (1 + u) (gamma_(d + k) E_ab / W + beta_a beta_b) + u |C_ab|
    d = centroid_ref.tree_depth(members); k = 3 roundings per product (two differences, one product; 4 with weights);
    E_ab = sum |p_ab| / (1 - gamma_k) over the products the definition forms (the computed doubles, added exactly);
    beta = centroid_ref.bound, the bound of the mean.  It presumes no overflow and no underflow."""
    pts = np.ascontiguousarray(pts, np.float64)
    D = pts.shape[1]
    ex = exact_cov(pts, labels, K, w) if ex is None else ex
    beta = CR.bound(pts, labels, K, w)
    r = moments(pts, labels, K, w)
    kk = 3 if w is None else 4
    wf = np.ones(len(pts)) if w is None else np.asarray(w, np.float64)
    out = []
    for k, ix in enumerate(CR._members(labels, K)):
        if ex[k] is None:
            out.append(None)
            continue
        W, _, C = ex[k]
        dd = pts[ix] - r["mean"][k]
        wd = wf[ix, None] * dd
        gd = CR.gamma(CR.tree_depth(len(ix)) + kk)
        row = {}
        for a in range(D):
            for b in range(a, D):
                E = CR._exact_int_sum(np.abs(wd[:, a] * dd[:, b])) / (1 - CR.gamma(kk))
                row[(a, b)] = (1 + U) * (gd * E / W + beta[k][a] * beta[k][b]) + U * abs(C[(a, b)])
        out.append(row)
    return out


def raw_moment_cov(pts, labels, K):
    """The covariance the library does NOT compute: sum(x x^T) / W - m m^T in binary64 (numpy's pairwise sums)."""
    pts = np.asarray(pts, np.float64)
    D = pts.shape[1]
    out = np.full((K, npk(D)), np.nan)
    for k, ix in enumerate(CR._members(labels, K)):
        if len(ix) == 0:
            continue
        x = pts[ix]
        m = x.sum(0) / len(ix)
        out[k] = [(x[:, a] * x[:, b]).sum() / len(ix) - m[a] * m[b] for a in range(D) for b in range(a, D)]
    return out


# ---- matrices for the solver -------------------------------------------------------------------------------------------------
def _sym(rng, D, lo=-1.0, hi=1.0):
    A = rng.uniform(lo, hi, (D, D))
    return np.triu(A) + np.triu(A, 1).T


def _rotation(rng, D):
    Q, R = np.linalg.qr(rng.normal(size=(D, D)))
    return Q * np.sign(np.diag(R))


def _spectral(rng, D, lam):
    Q = _rotation(rng, D)
    S = (Q * np.asarray(lam)) @ Q.T
    return np.triu(S) + np.triu(S, 1).T


EIG_FAMILIES = ("uniform", "graded", "isotropic", "planar", "diagonal", "zero", "one_offdiag", "equal_diag", "nonfinite",
                "overflow_end", "underflow_end")
# the families on which an error relative to |S|_F is defined and LAPACK can be asked: not all-zero, not non-finite
EIG_ACCURACY = tuple(f for f in EIG_FAMILIES if f not in ("zero", "nonfinite"))


def eig_family(name, D, count, seed=7):
    """`count` symmetric [D, D] matrices of one family (fewer where the family is a finite list)."""
    rng = np.random.default_rng([seed, EIG_FAMILIES.index(name), D])
    pairs = [(p, q) for p in range(D) for q in range(p + 1, D)]
    out = []
    for j in range(count):
        if name == "uniform":
            S = _sym(rng, D)
        elif name == "graded":          # eight decades, rotated
            S = _spectral(rng, D, 10.0 ** rng.uniform(-2, 2) * 10.0 ** (-8.0 * np.arange(D) / (D - 1)))
        elif name == "isotropic":
            S = np.eye(D) + 1e-13 * _sym(rng, D)
        elif name == "planar":          # the last axis 1e-9 of the others: its variance is below the rounding of the rest
            sd = rng.uniform(0.5, 2.0, D)
            sd[-1] *= 1e-9
            S = _spectral(rng, D, sd * sd)
        elif name == "diagonal":
            S = np.diag(rng.uniform(-1, 1, D))
        elif name == "zero":
            S = np.zeros((D, D)) if j % 2 == 0 else -np.zeros((D, D))
            if j >= 2:
                break
        elif name == "one_offdiag":
            S = np.zeros((D, D))
            p, q = pairs[j % len(pairs)]
            S[p, q] = S[q, p] = rng.uniform(-1, 1) * 10.0 ** rng.integers(-3, 4)
        elif name == "equal_diag":
            S = _sym(rng, D)
            S[np.diag_indices(D)] = rng.uniform(-1, 1)
        elif name == "nonfinite":
            S = _sym(rng, D)
            tri = list(zip(*np.triu_indices(D)))
            p, q = tri[j % len(tri)]
            S[p, q] = S[q, p] = [np.nan, np.inf, -np.inf][(j // len(tri)) % 3]
            if j >= 3 * len(tri):
                break
        elif name == "overflow_end":    # j even: entries up to 2^1000, where LAPACK still answers; odd: up to DBL_MAX
            S = _sym(rng, D) * (2.0 ** 1000 if j % 2 == 0 else 2.0 ** 1023)
        elif name == "underflow_end":   # j even: normal numbers near 2^-1000; odd: subnormal entries
            S = _sym(rng, D) * (2.0 ** -1000 if j % 2 == 0 else 2.0 ** -1065)
        else:
            raise ValueError(name)
        out.append(np.ascontiguousarray(S))
    return out


def eig_family_in_range(name, D, count, seed=7):
    """The matrices of eig_family on which the accuracy measures are taken: of the two end families only the even ones
    (squares and sums of the entries stay finite and normal, so LAPACK and the measures themselves are defined)."""
    m = eig_family(name, D, 2 * count if name.endswith("_end") else count, seed)
    return m[::2] if name.endswith("_end") else m


# ---- lattice shapes with closed forms ----------------------------------------------------------------------------------------
def lattice_disc(r, step):
    """The lattice points of pitch `step` inside the circle of radius r around the origin, [m, 2]."""
    k = int(np.floor(r / step))
    g = np.arange(-k, k + 1) * step
    x, y = np.meshgrid(g, g, indexing="ij")
    keep = x * x + y * y <= r * r
    return np.stack([x[keep], y[keep]], axis=1)


def lattice_ellipse(a, b, step, deg):
    """The lattice points inside the ellipse of semi-axes a, b turned by deg degrees, [m, 2].  The lattice itself is
    axis-aligned: the shape turns, the points stay representable."""
    k = int(np.floor(max(a, b) / step)) + 1
    g = np.arange(-k, k + 1) * step
    x, y = np.meshgrid(g, g, indexing="ij")
    c, s = np.cos(np.radians(deg)), np.sin(np.radians(deg))
    u, v = c * x + s * y, -s * x + c * y
    keep = (u / a) ** 2 + (v / b) ** 2 <= 1.0
    return np.stack([x[keep], y[keep]], axis=1)


def exact_eig(C, D):
    """Eigenvalues, descending, of the exact symmetric {(a, b): Fraction}, as floats from 60-digit arithmetic."""
    import mpmath
    with mpmath.workdps(60):
        M = mpmath.matrix(D, D)
        for (a, b), v in C.items():
            M[a, b] = M[b, a] = mpmath.mpf(v.numerator) / mpmath.mpf(v.denominator)
        return sorted((float(x) for x in mpmath.eigsy(M, eigvals_only=True)), reverse=True)
