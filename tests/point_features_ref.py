"""vcp_point_features' definition (include/vcp_features.h) restated in numpy binary64, sor_keep and centre_votes of
vtkcloudpoint_amd/features.py beside it, and the inputs the tests share.  No GPU, no library.

The sums run slot by slot in the order of the neighbour row (one numpy ufunc call per operation, over all rows at once:
each row's arithmetic is its own, sequential, acc = fl(acc + term)); the eigen-solve is cluster_moments_ref.sym_eig, row
by row.  numpy contracts nothing, its / and sqrt are correctly rounded."""
import numpy as np

import cluster_moments_ref as MR

F = np.float64
canon, same, bits = MR.canon, MR.same, MR.bits
KEYS = ("normal", "eval", "variation", "mean_dist", "count", "valid")
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1


# ---- the restatement --------------------------------------------------------------------------------------------------------
def features(pts, nbr, viewpoint=None, rows=None):
    """pts [n, D] (D = 2 or 3: the columns the call reads), nbr [n, k] int32, viewpoint D numbers or None.  Returns the dict
    of KEYS plus mean [n, D] and cov [n, D (D + 1) / 2]; with `rows` (indices) for those rows only, in that order."""
    allpts = np.ascontiguousarray(pts, np.float64)
    n, D = allpts.shape
    nbr = np.ascontiguousarray(nbr, np.int32)
    assert nbr.ndim == 2 and len(nbr) == n
    k = nbr.shape[1]
    pairs = [(a, b) for a in range(D) for b in range(a, D)]
    rows = np.arange(n) if rows is None else np.asarray(rows, np.int64)
    nbr, pts = nbr[rows], allpts[rows]                          # the rows the features are of; members come from allpts
    mem = (nbr >= 0) & (nbr < n)
    src = np.where(mem, nbr, rows[:, None])                     # a skipped slot reads no row through its value
    m = mem.sum(1).astype(np.int32)
    nr = len(rows)
    with np.errstate(all="ignore"):
        acc, sd, q = np.zeros((nr, D)), np.zeros(nr), np.zeros(nr, np.int64)
        for s in range(k):
            x = allpts[src[:, s]]
            e = x - pts
            e2 = e[:, 0] * e[:, 0]
            for a in range(1, D):
                e2 = e2 + e[:, a] * e[:, a]
            dist = np.sqrt(e2)
            acc = np.where(mem[:, s, None], acc + x, acc)
            other = mem[:, s] & (nbr[:, s] != rows)
            sd = np.where(other, sd + dist, sd)
            q += other
        md = m.astype(np.float64)
        mean = acc / md[:, None]
        S = np.zeros((nr, len(pairs)))
        for s in range(k):
            d = allpts[src[:, s]] - mean
            for j, (a, b) in enumerate(pairs):
                S[:, j] = np.where(mem[:, s], S[:, j] + d[:, a] * d[:, b], S[:, j])
        cov = S / md[:, None]
        mean_dist = sd / q.astype(np.float64)
        ev, normal, var = np.zeros((nr, D)), np.zeros((nr, D)), np.zeros(nr)
        vp = None if viewpoint is None else np.asarray(viewpoint, np.float64).reshape(-1)[:D]
        for i in range(nr):
            ev[i], vec, _ = MR.sym_eig(cov[i])
            nv = vec[D - 1]
            if vp is not None:
                t = [F(nv[a]) * (F(vp[a]) - F(pts[i, a])) for a in range(D)]
                sgn = t[0]
                for a in range(1, D):
                    sgn = sgn + t[a]
                if sgn < 0.0:
                    nv = -nv
            normal[i] = nv
            tot = F(ev[i, 0])
            for a in range(1, D):
                tot = tot + F(ev[i, a])
            var[i] = F(0.0) if tot == 0.0 else F(ev[i, D - 1]) / tot
    valid = ((m >= D) & np.isfinite(mean).all(1) & np.isfinite(cov).all(1)).astype(np.uint8)
    return dict(normal=canon(normal), eval=canon(ev), variation=canon(var), mean_dist=canon(mean_dist), count=m, valid=valid,
                mean=canon(mean), cov=canon(cov))


def differs(got, want, keys=KEYS):
    """None, or the first output whose bits differ with the rows at which they do."""
    for key in keys:
        g, w = np.asarray(got[key]), np.asarray(want[key])
        if g.shape != w.shape:
            return "%s: shape %s, want %s" % (key, g.shape, w.shape)
        ne = bits(g) != bits(w) if w.dtype.kind == "f" else g.astype(np.int64) != w.astype(np.int64)
        if ne.any():
            return "%s at rows %s" % (key, sorted(set(np.nonzero(ne)[0].tolist()))[:8])
    return None


def as_dict(f):
    """A features.PointFeatures (numpy or torch members) as the dict differs() takes."""
    h = lambda a: a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)
    return {key: h(getattr(f, key)) for key in KEYS}


def lower_median(v):
    v = np.sort(np.asarray(v, np.float64))
    return F(np.nan) if len(v) == 0 else v[(len(v) - 1) // 2]


def sor_keep(mean_dist, c=6.0, floor=0.0):
    """(keep, median, mad): the lower median of the finite entries, the lower median of fl(|v - median|) over them,
    keep = v <= fl(median + max(fl(c mad), floor)) (False for NaN)."""
    v = np.asarray(mean_dist, np.float64).reshape(-1)
    fin = v[np.isfinite(v)]
    with np.errstate(all="ignore"):
        med = lower_median(fin)
        mad = lower_median(np.abs(fin - med))
        keep = v <= med + max(F(c) * mad, F(floor))
    return keep, float(med), float(mad)


def centre_votes(pts, normal, radius, valid):
    D = normal.shape[1]
    with np.errstate(all="ignore"):
        votes = np.asarray(pts, np.float64)[:, :D] - F(radius) * np.asarray(normal, np.float64)
    return canon(np.where(np.asarray(valid).reshape(-1, 1) != 0, votes, np.nan))


# ---- inputs --------------------------------------------------------------------------------------------------------------------
def lattice_rows(n, D, seed, span=4096):
    """[n, D] on the 2^-10 lattice in +-span / 1024: differences, squares of them and short sums are exact."""
    return np.random.default_rng([seed, D, 1]).integers(-span, span + 1, (n, D)).astype(np.float64) * 2.0 ** -10


def generic_rows(n, D, seed, offset=0.0, scale=1.0):
    """[n, D]: blobs of every width around `offset`, so that near and far neighbours, rounded sums and (at an offset of
    1e8) the cancellation the centred form is there for all occur."""
    rng = np.random.default_rng([seed, D, 2])
    c = rng.normal(size=(max(n // 40, 1), D)) * scale
    return offset + c[rng.integers(0, len(c), n)] + rng.normal(size=(n, D)) * scale * 10.0 ** rng.uniform(-4, -1, (n, 1))


def mixed_nbr(n, k, seed):
    """[n, k] int32 rows with every kind of slot: members, -1, values out of range on both ends (just outside and at the
    ends of int32), repeats, the row itself present (at a random slot) or absent; rows 0 .. 5 (where they exist) are
    all -1, a single member, the row alone, one index k times, out of range only, and -1 in front, middle and end."""
    rng = np.random.default_rng([seed, n, k])
    nbr = rng.integers(0, max(n, 1), (n, k)).astype(np.int64)
    bad = np.array([-1, -1, -1, -2, n, n + 1, I32_MIN, I32_MAX], np.int64)
    kind = rng.random((n, k))
    nbr = np.where(kind < 0.12, bad[rng.integers(0, len(bad), (n, k))], nbr)
    rep = (kind > 0.9) & (np.arange(k) > 0)
    nbr = np.where(rep, np.roll(nbr, 1, axis=1), nbr)                       # a repeat of the slot before
    rows = np.arange(n)
    has_self = rng.random(n) < 0.6
    slot = rng.integers(0, k, n)
    nbr[rows[has_self], slot[has_self]] = rows[has_self]
    drop = ~has_self
    nbr[drop] = np.where(nbr[drop] == rows[drop, None], (nbr[drop] + 1) % max(n, 1), nbr[drop])
    special = [np.full(k, -1), np.r_[np.full(k - 1, -1), min(1, n - 1)], np.r_[2, np.full(k - 1, -1)] if k > 1 else np.array([3]),
               np.full(k, 0), np.resize([n, -7, I32_MAX, I32_MIN], k), np.resize([-1, 1, 0, -1, 2, -1], k)]
    special[5][-1] = -1
    for r, row in enumerate(special):
        if r < n:
            nbr[r] = row
    return nbr.astype(np.int32)


def tiled_case(n, k, D, seed, period=509):
    """A cloud of n rows too long for a row-by-row restatement: row i has the coordinates of row i % period, and slot s of
    its neighbour row holds an index congruent to local[i % period, s] modulo period -- the row i itself where that is
    i % period, a pseudo-random row of that residue otherwise -- or the skipped value local holds there.  The features of
    row i are then those of row i % period of the first `period` rows under `local`, which is what want_tiled returns.
    Returns (pts [n, D], nbr [n, k], base [period, D], local [period, k])."""
    base = generic_rows(period, D, seed)
    local = mixed_nbr(period, k, seed + 1)
    i = np.arange(n, dtype=np.int64)
    r = i % period
    loc = local[r].astype(np.int64)                                          # [n, k]
    mem = (loc >= 0) & (loc < period)
    copies = (n - 1 - np.where(mem, loc, 0)) // period + 1                   # rows of that residue below n: >= 1
    pick = (i[:, None] * 2654435761 + np.arange(k) * 40503 + seed) % copies
    j = np.where(mem, loc + pick * period, loc)
    j = np.where(mem & (loc == r[:, None]), i[:, None], j)
    clash = mem & (loc != r[:, None]) & (j == i[:, None])                    # cannot happen: another residue
    assert not clash.any()
    j = np.where(~mem & (loc >= period), np.maximum(loc, n), j)              # still out of range for n rows
    return base[r], j.astype(np.int32), base, local


def want_tiled(base, local, n, viewpoint=None):
    w = features(base, local, viewpoint)
    r = np.arange(n) % len(base)
    return {key: w[key][r] for key in KEYS}


# ---- the scene -------------------------------------------------------------------------------------------------------------------
R_SPHERE = 0.0725
N_SPHERES, PER_SPHERE, N_FLOOR, N_STRAY = 5, 600, 20000, 300
SCENE_SEEDS = (11, 12)
_scenes = {}


def scene(seed):
    """The scene of the trial: the instrument at the origin; a floor patch of 20 000 returns (z = -1.2, 1.2 m x 1.0 m);
    five spheres of radius 0.0725 0.25 m above it with 600 returns each on the half the instrument sees; 300 strays uniform
    in the box around them; gaussian range noise along the ray, sigma drawn per surface from 0.5 .. 1 mm.  Returns
    (pts [23300, 3], kind [n]: 0 stray, -1 floor, 1 .. 5 the sphere, centres [5, 3])."""
    rng = np.random.default_rng([seed, 77])
    x0, x1, y0, y1, zf = 2.4, 3.6, -0.5, 0.5, -1.2
    centres = []
    while len(centres) < N_SPHERES:
        c = np.array([rng.uniform(x0 + 0.15, x1 - 0.15), rng.uniform(y0 + 0.15, y1 - 0.15), zf + 0.25])
        if all(np.linalg.norm(c - o) >= 0.3 for o in centres):
            centres.append(c)
    centres = np.array(centres)

    def noisy(p):
        rr = np.linalg.norm(p, axis=1, keepdims=True)
        return p + p / rr * rng.normal(size=(len(p), 1)) * rng.uniform(0.0005, 0.001)

    parts, kind = [], []
    for j, c in enumerate(centres):
        got = np.zeros((0, 3))
        while len(got) < PER_SPHERE:
            v = rng.normal(size=(4 * PER_SPHERE, 3))
            p = c + R_SPHERE * v / np.linalg.norm(v, axis=1, keepdims=True)
            got = np.concatenate([got, p[((p - c) * (0.0 - p)).sum(1) > 0.0]])      # the side that faces the origin
        parts.append(noisy(got[:PER_SPHERE]))
        kind.append(np.full(PER_SPHERE, j + 1))
    floor = np.column_stack([rng.uniform(x0, x1, N_FLOOR), rng.uniform(y0, y1, N_FLOOR), np.full(N_FLOOR, zf)])
    parts.append(noisy(floor))
    kind.append(np.full(N_FLOOR, -1))
    parts.append(np.column_stack([rng.uniform(x0, x1, N_STRAY), rng.uniform(y0, y1, N_STRAY), rng.uniform(zf + 0.02, zf + 0.6, N_STRAY)]))
    kind.append(np.zeros(N_STRAY, np.int64))
    pts, kind = np.concatenate(parts), np.concatenate(kind)
    order = rng.permutation(len(pts))
    return np.ascontiguousarray(pts[order]), kind[order], centres


def knn_rows(pts, k):
    """[n, k] int32: per row the k smallest (d, j) pairs by the expression of vcp_kdist (kdist_ref.dist_rows, L2), the row
    itself included.  scipy's tree proposes k + 8 candidates per row, which are re-ranked exactly; a row whose k-th exact
    distance does not lie strictly inside the candidates' reach is ranked by brute force."""
    import kdist_ref
    pts = np.ascontiguousarray(pts, np.float64)
    n, D = pts.shape
    metric = kdist_ref.L2_3D if D == 3 else kdist_ref.L2_2D
    try:
        from scipy.spatial import cKDTree
        cand = cKDTree(pts).query(pts, k=min(k + 8, n))[1].reshape(n, -1)
    except ImportError:
        return kdist_ref.brute_rows(pts, k, metric, np.arange(n))[1]
    out = np.zeros((n, k), np.int32)
    for i in range(n):
        c = np.sort(cand[i])
        d = kdist_ref.dist_rows(pts[c], pts[i], metric)
        o = np.argsort(d, kind="stable")
        if len(c) > k and not d[o[k - 1]] < d[o[-1]]:
            out[i] = kdist_ref.brute_rows(pts, k, metric, [i])[1][0]
        else:
            out[i] = c[o[:k]]
    return out


def scene_features(seed, k=16):
    """(pts, kind, centres, knn, the restatement's features with the viewpoint at the origin), computed once per seed."""
    if seed not in _scenes:
        pts, kind, centres = scene(seed)
        knn = knn_rows(pts, k)
        _scenes[seed] = (pts, kind, centres, knn, features(pts, knn, (0.0, 0.0, 0.0)))
    return _scenes[seed]


def scene_subset(seed, rows=5000):
    """`rows` rows of the scene (the first of its shuffled order, so every kind is among them)."""
    pts, kind, centres = scene(seed)
    return np.ascontiguousarray(pts[:rows]), kind[:rows], centres
