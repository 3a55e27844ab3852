"""vcp_cluster_spheres' definition (include/vcp.h) restated in numpy binary64: the sums through the centroid tree of
centroid_ref (stated once, there), the solve as the operation sequence of csrc/spdsolve.hpp on numpy float64 scalars; the
same iteration at 60 digits (mpmath) as the measure of accuracy, a plain numpy Gauss-Newton as the yardstick, and the
inputs of the tests.  No GPU, no oracle.  Every numpy operation is one binary64 ufunc call; numpy contracts nothing."""
import numpy as np

import centroid_ref as CR
from cluster_moments_ref import bits, canon, same   # noqa: F401  (the tests use them through this module)

F = np.float64
R_TARGET = 0.0725      # the sphere targets' radius
KEYS = ("centre", "radius", "rms", "cap", "step", "alg", "valid", "counts")


def npk(dim):
    return dim * (dim + 1) // 2


# ---- the solve: csrc/spdsolve.hpp, step by step ----------------------------------------------------------------------------
def _pivot_ok(p):
    return bool(p > 0.0) and bool(p <= 1.7976931348623157e308)


def spd_solve(s, b):
    """s packed upper triangle (3 or 6), b [D] -> (x [D], ok)."""
    s = [F(v) for v in np.asarray(s, np.float64)]
    b = [F(v) for v in np.asarray(b, np.float64)]
    D = {3: 2, 6: 3}[len(s)]
    with np.errstate(all="ignore"):
        if D == 2:
            a00, a01, a11 = s
            p0 = a00
            l10 = a01 / p0
            p1 = a11 - l10 * a01
            if not (_pivot_ok(p0) and _pivot_ok(p1)):
                return np.full(2, np.nan), 0
            y0 = b[0]
            y1 = b[1] - l10 * y0
            z0, z1 = y0 / p0, y1 / p1
            return np.array([z0 - l10 * z1, z1]), 1
        a00, a01, a02, a11, a12, a22 = s
        p0 = a00
        l10, l20 = a01 / p0, a02 / p0
        p1 = a11 - l10 * a01
        t = a12 - l20 * a01
        l21 = t / p1
        p2 = (a22 - l20 * a02) - l21 * t
        if not (_pivot_ok(p0) and _pivot_ok(p1) and _pivot_ok(p2)):
            return np.full(3, np.nan), 0
        y0 = b[0]
        y1 = b[1] - l10 * y0
        y2 = (b[2] - l20 * y0) - l21 * y1
        z0, z1, z2 = y0 / p0, y1 / p1, y2 / p2
        x2 = z2
        x1 = z1 - l21 * x2
        return np.array([(z0 - l10 * x1) - l20 * x2, x1, x2]), 1


def _dot(a, b):
    """Row-wise a . b in the definition's association: (a0 b0 + a1 b1) + a2 b2."""
    r = a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]
    if a.shape[-1] == 3:
        r = r + a[..., 2] * b[..., 2]
    return r


# ---- the restatement -------------------------------------------------------------------------------------------------------
def spheres(pts, labels, K, weights=None, fixed_radius=0.0, rounds=12, raw=False, trace=None):
    """pts [n, D] (D = 2 or 3: the columns the call reads), labels [n] in 0..K, weights int or None.  Returns the dict
    Context.cluster_spheres returns.  raw=True is the variant the library does NOT compute: e is formed from raw
    coordinates, fl(x - c) with c = fl(m + u), instead of fl(d - u).  trace: a list that receives step [K] of every
    round."""
    pts = np.ascontiguousarray(pts, np.float64)
    n, D = pts.shape
    NP = npk(D)
    labels = np.ascontiguousarray(labels, np.int32)
    idx = CR._members(labels, K)
    wi = np.ones(n, np.int64) if weights is None else np.asarray(weights, np.int64)
    w = wi.astype(np.float64)
    pairs = [(a, b) for a in range(D) for b in range(a, D)]
    diag = [pairs.index((a, a)) for a in range(D)]
    fixed = fixed_radius > 0.0
    own = np.maximum(labels, 1) - 1          # rows of label 0 are never summed

    def tree(cols):
        v = np.stack(cols, axis=1) if n else np.zeros((0, len(cols)))
        return CR._tree_sums(v, idx, CR.KERNEL)[0]

    def member(u):
        if raw:
            e = pts - (mean + u)[own]
        else:
            e = d - u[own]
        rho = np.sqrt(_dot(e, e))
        nu = np.where((rho == 0.0)[:, None], 0.0, e / rho[:, None])
        return rho, nu

    with np.errstate(all="ignore"):
        s1 = tree([pts[:, a] * w for a in range(D)])
        W = np.array([int(wi[ix].sum()) for ix in idx], np.int64).reshape(K)
        Wd = W.astype(np.float64)
        mean = s1 / Wd[:, None]
        d = pts - mean[own] if K > 0 else pts * 0.0
        wd = w[:, None] * d
        wq = w * _dot(d, d)
        st = tree([wd[:, a] * d[:, b] for a, b in pairs] + [wq * d[:, a] for a in range(D)])
        u, ok = np.zeros((K, D)), np.ones(K, bool)
        for k in range(K):
            u[k], g = spd_solve(st[k, :NP], st[k, NP:] * F(0.5))
            ok[k] &= bool(g)
        tr = st[:, diag[0]] + st[:, diag[1]]
        if D == 3:
            tr = tr + st[:, diag[2]]
        r0 = np.sqrt(_dot(u, u) + tr / Wd)
        alg = np.concatenate([mean + u, r0[:, None]], axis=1)
        rref = np.full(K, F(fixed_radius)) if fixed else r0.copy()
        step = np.zeros(K)
        for _ in range(rounds):
            rho, nu = member(u)
            wn = w[:, None] * nu
            wr = w * rho
            sr = tree([wn[:, a] * nu[:, b] for a, b in pairs] + [wn[:, a] for a in range(D)] + [wr] +
                      [wr * nu[:, a] for a in range(D)])
            N, b, R, g = sr[:, :NP], sr[:, NP:NP + D], sr[:, NP + D], sr[:, NP + D + 1:]
            if fixed:
                M = N
                y = g - F(fixed_radius) * b
            else:
                M = np.stack([N[:, j] - (b[:, p] * b[:, q]) / Wd for j, (p, q) in enumerate(pairs)], axis=1)
                y = g - (R[:, None] * b) / Wd[:, None]
                rref = R / Wd
            dl = np.zeros((K, D))
            for k in range(K):
                dl[k], gk = spd_solve(M[k], y[k])
                ok[k] &= bool(gk)
            u = u + dl
            step = np.sqrt(_dot(dl, dl))
            if trace is not None:
                trace.append(step.copy())
        rho, nu = member(u)
        c = rho - rref[own]
        wc = w * c
        sc = tree([w * nu[:, a] for a in range(D)] + [wc, wc * c])
        b, C1, C2 = sc[:, :D], sc[:, D], sc[:, D + 1]
        if fixed:
            radius = np.full(K, F(fixed_radius))
            rms = np.sqrt(C2 / Wd)
        else:
            cb = C1 / Wd
            radius = rref + cb
            v = C2 / Wd - cb * cb
            rms = np.sqrt(np.where(v < 0.0, 0.0, v))
        centre = mean + u
        cap = np.sqrt(_dot(b, b)) / Wd
    outs = np.concatenate([centre, radius[:, None], rms[:, None], cap[:, None], step[:, None], alg], axis=1)
    valid = (W >= (D if fixed else D + 1)) & ok & np.isfinite(outs).all(1)
    bad = ~valid

    def fin(a):
        a = np.array(a, np.float64)
        a[bad] = np.nan
        return canon(a)

    return dict(centre=fin(centre), radius=fin(radius), rms=fin(rms), cap=fin(cap), step=fin(step), alg=fin(alg),
                valid=valid.astype(np.uint8), counts=W)


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


# ---- the yardstick and the 60-digit minimiser --------------------------------------------------------------------------------
def plain_gn(x, fixed_radius=0.0, rounds=12):
    """The same iteration on ONE cluster x [m, D] the way one would write it in numpy: np.sum, np.linalg.solve, raw
    coordinates shifted by the mean.  Returns (centre [D], radius)."""
    x = np.asarray(x, np.float64)
    m = x.mean(0)
    d = x - m
    q = np.sum(d * d, axis=1)
    u = np.linalg.solve(d.T @ d, 0.5 * (d * q[:, None]).sum(0))
    W = float(len(x))
    for _ in range(rounds):
        e = d - u
        rho = np.sqrt(np.sum(e * e, axis=1))
        nu = e / rho[:, None]
        b = nu.sum(0)
        if fixed_radius > 0.0:
            dl = np.linalg.solve(nu.T @ nu, (rho[:, None] * nu).sum(0) - fixed_radius * b)
        else:
            dl = np.linalg.solve(nu.T @ nu - np.outer(b, b) / W, (rho[:, None] * nu).sum(0) - rho.sum() * b / W)
        u = u + dl
    rho = np.sqrt(np.sum((d - u) ** 2, axis=1))
    return m + u, (fixed_radius if fixed_radius > 0.0 else rho.sum() / W)


def minimiser(x, centre, fixed_radius=0.0, tol="1e-40", cap=200):
    """The least-squares centre and radius of ONE cluster x [m, D] (exact binary64 inputs) at 60 digits: the iteration of
    the definition in mpmath, continued from `centre` until |delta| < tol.  Returns (centre [D] mpf, radius mpf)."""
    import mpmath
    with mpmath.workdps(60):
        X = [[mpmath.mpf(float(v)) for v in row] for row in np.asarray(x, np.float64)]
        D, W = len(X[0]), mpmath.mpf(len(X))
        c = [mpmath.mpf(float(v)) for v in centre]
        fr = mpmath.mpf(float(fixed_radius))
        for _ in range(cap):
            E = [[xi[a] - c[a] for a in range(D)] for xi in X]
            rho = [mpmath.sqrt(sum(v * v for v in e)) for e in E]
            nu = [[v / r for v in e] for e, r in zip(E, rho)]
            b = [sum(v[a] for v in nu) for a in range(D)]
            R = sum(rho)
            M = mpmath.matrix(D, D)
            y = mpmath.matrix(D, 1)
            for a in range(D):
                ga = sum(r * v[a] for r, v in zip(rho, nu))
                y[a] = ga - fr * b[a] if fixed_radius > 0.0 else ga - R * b[a] / W
                for bb in range(D):
                    nab = sum(v[a] * v[bb] for v in nu)
                    M[a, bb] = nab if fixed_radius > 0.0 else nab - b[a] * b[bb] / W
            dl = mpmath.lu_solve(M, y)
            c = [c[a] + dl[a] for a in range(D)]
            if mpmath.sqrt(sum(v * v for v in dl)) < mpmath.mpf(tol):
                break
        else:
            raise RuntimeError("the 60-digit iteration did not settle")
        rho = [mpmath.sqrt(sum((xi[a] - c[a]) ** 2 for a in range(D))) for xi in X]
        return c, (fr if fixed_radius > 0.0 else sum(rho) / W)


def error_to(cm, rm, centre, radius):
    """(|centre - cm|, |radius - rm|) as floats; cm, rm from minimiser."""
    import mpmath
    with mpmath.workdps(60):
        ec = mpmath.sqrt(sum((mpmath.mpf(float(v)) - t) ** 2 for v, t in zip(centre, cm)))
        return float(ec), float(abs(mpmath.mpf(float(radius)) - rm))


# ---- inputs -----------------------------------------------------------------------------------------------------------------
def cap_points(rng, centre, m, R=R_TARGET, inner=1.0, noise=0.0, dim=3):
    """m returns of a sphere (dim 3) or of its rim circle in the plane through the origin (dim 2), seen from the origin:
    uniform on the projected disc (3-D) or on the projected chord (2-D), of which the inner share `inner` returns;
    `noise` is the standard deviation of a range error along the ray.  [m, dim]."""
    centre = np.asarray(centre, np.float64)
    D = np.linalg.norm(centre)
    ax = -centre / D                                   # from the centre to the instrument
    if dim == 3:
        t = np.cross(ax, [0.0, 0.0, 1.0] if abs(ax[2]) < 0.9 else [1.0, 0.0, 0.0])
        t /= np.linalg.norm(t)
        t2 = np.cross(ax, t)
        s = inner * np.sqrt(rng.uniform(0, 1, m))      # uniform on the disc of radius `inner`
        phi = rng.uniform(0, 2 * np.pi, m)
        lat = s[:, None] * (np.cos(phi)[:, None] * t + np.sin(phi)[:, None] * t2)
    else:
        t = np.array([-ax[1], ax[0]])
        s = inner * rng.uniform(-1, 1, m)
        lat = s[:, None] * t
        s = np.abs(s)
    p = centre + R * (lat + np.sqrt(1.0 - s * s)[:, None] * ax)
    if noise > 0.0:
        p = p * (1.0 + rng.normal(0, noise, m) / np.linalg.norm(p, axis=1))[:, None]
    return np.ascontiguousarray(p)


ACC_FAMILIES = ("clean", "noisy", "inner60", "few", "near")


def accuracy_cases(family, dim, count=6, seed=11):
    """`count` of (x [m, dim], true centre) of one family of caps seen from the origin, R = R_TARGET:
      clean    distance 5..20, 60..400 points, no noise, the whole cap
      noisy    the same with range noise up to 0.005
      inner60  the inner 60 % .. 100 % of the cap, noise up to 0.002
      few      60 points, noise 0.001
      near     distance 5, 400 points, noise 0.005"""
    rng = np.random.default_rng([seed, ACC_FAMILIES.index(family), dim])
    out = []
    for _ in range(count):
        dist, m, noise, inner = rng.uniform(5, 20), int(rng.integers(60, 401)), 0.0, 1.0
        if family == "noisy":
            noise = rng.uniform(0.0005, 0.005)
        elif family == "inner60":
            inner, noise = rng.uniform(0.6, 1.0), rng.uniform(0, 0.002)
        elif family == "few":
            m, noise = 60, 0.001
        elif family == "near":
            dist, m, noise = 5.0, 400, 0.005
        v = rng.normal(size=dim)
        c = dist * v / np.linalg.norm(v)
        out.append((cap_points(rng, c, m, inner=inner, noise=noise, dim=dim), c))
    return out


def lattice(dim):
    """Integer points at one distance from the origin: the 12 of radius 5 in the plane, the 24 of radius 3 in space."""
    if dim == 2:
        p = [(sx * a, sy * b) for a, b in ((3, 4), (4, 3)) for sx in (1, -1) for sy in (1, -1)]
        p += [(5, 0), (-5, 0), (0, 5), (0, -5)]
        return np.array(p, np.float64), 5.0
    p = set()
    for perm in ((1, 2, 2), (2, 1, 2), (2, 2, 1)):
        for sx in (1, -1):
            for sy in (1, -1):
                for sz in (1, -1):
                    p.add((sx * perm[0], sy * perm[1], sz * perm[2]))
    return np.array(sorted(p), np.float64), 3.0


def exact_family(dim):
    """(x, centre, radius): the lattice scaled by a power of two and shifted by a dyadic offset."""
    p, r = lattice(dim)
    if dim == 2:
        c, s = np.array([1000.25, -77.5]), 0.125
    else:
        c, s = np.array([3.5, 100.125, -9.0]), 0.0625
    return p * s + c, c, r * s


SPD_FAMILIES = ("random", "graded", "scaled_up", "scaled_down", "subnormal", "identity", "indefinite", "semidefinite",
                "zero", "nonfinite", "nonfinite_rhs")


def spd_family(name, D, count, seed=3):
    """`count` of (S symmetric [D, D], b [D]) of one family (fewer where the family is a finite list)."""
    rng = np.random.default_rng([seed, SPD_FAMILIES.index(name), D])
    tri = list(zip(*np.triu_indices(D)))
    out = []
    for j in range(count):
        A = rng.normal(size=(D + 2, D))
        S, b = A.T @ A, rng.normal(size=D)
        if name == "graded":
            sc = 10.0 ** (-4.0 * np.arange(D))
            S = S * sc[:, None] * sc[None, :]
        elif name == "scaled_up":
            S, b = S * 2.0 ** 1000, b * 2.0 ** 990
        elif name == "scaled_down":
            S, b = S * 2.0 ** -1000, b * 2.0 ** -1000
        elif name == "subnormal":           # entries of a few bits: a pivot may round to 0 and fail
            S, b = S * 2.0 ** -1070, b * 2.0 ** -1000
        elif name == "identity":
            S = np.eye(D)
        elif name == "indefinite":
            S = S - np.eye(D) * (np.linalg.eigvalsh(S)[j % D] + 0.25)
        elif name == "semidefinite":        # L diag(p) L^T of dyadic numbers with one pivot 0: every step is exact
            L = np.tril(rng.integers(-8, 9, (D, D)) / 4.0, -1) + np.eye(D)
            p = 2.0 ** rng.integers(-3, 4, D)
            p[j % D] = 0.0
            S = (L * p) @ L.T
        elif name == "zero":
            S = np.zeros((D, D)) if j % 2 == 0 else -np.zeros((D, D))
            if j >= 2:
                break
        elif name == "nonfinite":
            p, q = tri[j % len(tri)]
            S[p, q] = S[q, p] = [np.nan, np.inf, -np.inf][(j // len(tri)) % 3]
            if j >= 3 * len(tri):
                break
        elif name == "nonfinite_rhs":
            b[j % D] = [np.nan, np.inf, -np.inf][(j // D) % 3]
            if j >= 3 * D:
                break
        elif name != "random":
            raise ValueError(name)
        out.append((np.ascontiguousarray(S), np.ascontiguousarray(b)))
    return out


# ---- the device tests' clusters ---------------------------------------------------------------------------------------------
def case_points(labels, seed=21):
    """xyz [n, 3] on the shared labels (centroid_ref.case_labels): every cluster a noisy cap of a sphere of its own, seen
    from the origin; every fourth cluster (by label) an unshaped blob, for which only parity is asserted; the rows of
    label 0 scattered.  Columns 0, 1 of it are the 2-D input: arcs and blobs of the projection."""
    rng = np.random.default_rng(seed)
    labels = np.asarray(labels)
    xyz = rng.uniform(-30, 30, (len(labels), 3))
    for j, ix in enumerate(CR._members(labels, int(labels.max()))):
        if len(ix) == 0:
            continue
        v = rng.normal(size=3)
        c = rng.uniform(5, 20) * v / np.linalg.norm(v)
        if j % 4 == 3:
            xyz[ix] = c + rng.normal(0, 0.05, (len(ix), 3))
        else:
            xyz[ix] = cap_points(rng, c, len(ix), R=rng.uniform(0.05, 0.5), noise=0.002)
    return np.ascontiguousarray(xyz)


def case_weights(labels, seed=22):
    """int32 weights 0..5 (about a sixth are 0), one of 2^20 in the 257-member cluster."""
    rng = np.random.default_rng(seed)
    w = rng.integers(0, 6, len(labels)).astype(np.int32)
    cnt = np.bincount(labels)
    big = np.flatnonzero(labels == [k for k in range(1, len(cnt)) if cnt[k] == 257][0])
    w[big[5]] = 2 ** 20
    return w
