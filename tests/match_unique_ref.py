"""vcp_match_unique's definition (include/vcp.h) restated in numpy: the transform and the distance in the stated operand
order, the candidate set, and the SEQUENTIAL greedy walk over the key (d, j, i).  The device works by rounds of locally
dominant pairs; `rounds_matching` writes those out too, for the tests that show the two agree.  `nearest_match` is
vcp_match's rule (nearest truth, strict <, lowest index on ties), for the two properties that tie the calls together."""
import numpy as np


def transform(centers, M):
    """m_j = M * (c_j, 1): row by row, left to right, every operation rounded on its own."""
    c = np.asarray(centers, np.float64).reshape(-1, 3)
    M = np.asarray(M, np.float64).reshape(4, 4)
    m = np.empty_like(c)
    with np.errstate(all="ignore"):
        for r in range(3):
            m[:, r] = c[:, 0] * M[r, 0] + c[:, 1] * M[r, 1] + c[:, 2] * M[r, 2] + M[r, 3]
    return m


def distances(m_rows, truth_rows):
    """d = sqrt(dx*dx + dy*dy + dz*dz), dx = truth - m, on matching rows (or broadcast)."""
    with np.errstate(all="ignore"):
        dx = truth_rows[..., 0] - m_rows[..., 0]
        dy = truth_rows[..., 1] - m_rows[..., 1]
        dz = truth_rows[..., 2] - m_rows[..., 2]
        return np.sqrt(dx * dx + dy * dy + dz * dz)


def candidates(m, truths, max_dist, dense_limit=4_000_000):
    """(j, i, d) arrays of E = { d(j,i) < max_dist, d not +inf }, in no particular order."""
    K, T = len(m), len(truths)
    empty = (np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0))
    if K == 0 or T == 0 or not (max_dist > 0):
        return empty
    if K * T <= dense_limit or not np.isfinite(max_dist):
        D = distances(m[:, None, :], truths[None, :, :])
        with np.errstate(invalid="ignore"):
            ok = (D < max_dist) & (D < np.inf)
        j, i = np.nonzero(ok)
        return j.astype(np.int64), i.astype(np.int64), D[j, i]
    from scipy.spatial import cKDTree
    tf = np.flatnonzero(np.isfinite(truths).all(1))
    cf = np.flatnonzero(np.isfinite(m).all(1))
    if len(tf) == 0 or len(cf) == 0:
        return empty
    tree = cKDTree(truths[tf])
    near = tree.query_ball_point(m[cf], max_dist * (1.0 + 1e-9) + 1e-300)
    jj = np.repeat(cf, [len(x) for x in near]).astype(np.int64)
    ii = tf[np.concatenate([np.asarray(x, np.int64) for x in near]).astype(np.int64)] if len(jj) else np.zeros(0, np.int64)
    d = distances(m[jj], truths[ii])
    ok = (d < max_dist) & (d < np.inf)
    return jj[ok], ii[ok].astype(np.int64), d[ok]


def _result(K, T, m, truth_of, pair_dist, rounds=None):
    center_of = np.full(T, -1, np.int32)
    js = np.flatnonzero(truth_of >= 0)
    center_of[truth_of[js]] = js
    out = dict(matched_xyz=m, truth_of=truth_of, center_of=center_of, pair_dist=pair_dist, count=int(len(js)))
    if rounds is not None:
        out["rounds"] = rounds
    return out


def greedy_matching(centers, truths, M, max_dist):
    """The specification: walk E in ascending (d, j, i), accept a pair when neither end is taken."""
    truths = np.asarray(truths, np.float64).reshape(-1, 3)
    m = transform(centers, M)
    K, T = len(m), len(truths)
    j, i, d = candidates(m, truths, float(max_dist))
    order = np.lexsort((i, j, d))
    truth_of = np.full(K, -1, np.int32)
    pair_dist = np.full(K, np.inf)
    taken = np.zeros(T, bool)
    for e in order:
        a, b = int(j[e]), int(i[e])
        if truth_of[a] < 0 and not taken[b]:
            truth_of[a] = b
            taken[b] = True
            pair_dist[a] = d[e]
    return _result(K, T, m, truth_of, pair_dist)


def rounds_matching(centers, truths, M, max_dist):
    """The device's method on a dense distance matrix: per round every pair that is the minimum-key candidate of both its
    ends among the free points is accepted at once; stops when a round accepts nothing."""
    truths = np.asarray(truths, np.float64).reshape(-1, 3)
    m = transform(centers, M)
    K, T = len(m), len(truths)
    D = distances(m[:, None, :], truths[None, :, :]) if K and T else np.zeros((K, T))
    with np.errstate(invalid="ignore"):
        E = (D < max_dist) & (D < np.inf)
    Dk = np.where(E, D, np.inf)
    truth_of = np.full(K, -1, np.int32)
    pair_dist = np.full(K, np.inf)
    free_c, free_t = np.ones(K, bool), np.ones(T, bool)
    rounds = 0
    while K and T:
        A = np.where(free_c[:, None] & free_t[None, :], Dk, np.inf)
        best_i = A.argmin(1)            # lowest i among equal d
        best_j = A.argmin(0)            # lowest j among equal d
        js = np.flatnonzero(np.isfinite(A[np.arange(K), best_i]))
        acc = [a for a in js if best_j[best_i[a]] == a]
        if not acc:
            break
        rounds += 1
        for a in acc:
            b = int(best_i[a])
            truth_of[a], pair_dist[a] = b, D[a, b]
            free_c[a] = free_t[b] = False
    return _result(K, T, m, truth_of, pair_dist, rounds)


def nearest_match(centers, truths, M, max_dist):
    """vcp_match's rule on a dense matrix (finite inputs): nearest truth, strict <, lowest index; matched iff d < max_dist."""
    truths = np.asarray(truths, np.float64).reshape(-1, 3)
    m = transform(centers, M)
    D = distances(m[:, None, :], truths[None, :, :])
    nearest = D.argmin(1).astype(np.int32)
    nd = D[np.arange(len(m)), nearest]
    return dict(matched_xyz=m, nearest=nearest, nearest_dist=nd, is_matched=(nd < max_dist).astype(np.uint8),
                count=int((nd < max_dist).sum()))


# ---- shared inputs ---------------------------------------------------------------------------------------------------
def chain(n, step=0.001):
    """n centroids and n truths alternating on a line, gaps strictly decreasing (1 - step k): nearest is injective, yet
    only the last pair is locally dominant, then the one before it, ...: n rounds."""
    gaps = 1.0 - step * np.arange(2 * n - 1)
    x = np.concatenate([[0.0], np.cumsum(gaps)])
    z = np.zeros(n)
    centers = np.c_[x[0::2], z, z]
    truths = np.c_[x[1::2], z, z]
    return centers, truths


def lattice(seed=7, T=2000, K=2200):
    """Exact ties and duplicates: truths on a 0.5 lattice, centroids on a 0.25 lattice, rows repeated in both lists."""
    rng = np.random.default_rng(seed)
    t = np.c_[rng.integers(0, 30, (T - 100, 2)), rng.integers(0, 3, T - 100)] * 0.5
    c = np.c_[rng.integers(0, 60, (K - 100, 2)), rng.integers(0, 6, K - 100)] * 0.25
    t = np.r_[t, t[rng.integers(0, len(t), 100)]]
    c = np.r_[c, c[rng.integers(0, len(c), 100)]]
    return c[rng.permutation(K)], t[rng.permutation(T)]


def field(seed, T=30000, n_det=26000, n_clutter=4000, sigma=0.02, pitch=1.0):
    """Truths on a jittered 2-D field (z = 0, as the reference feeds them), detections = truths + noise, plus clutter, a
    quarter of it right beside a detection (the false cluster next to a target)."""
    rng = np.random.default_rng(seed)
    side = int(np.ceil(np.sqrt(T)))
    g = np.stack(np.meshgrid(np.arange(side), np.arange(side), indexing="ij"), -1).reshape(-1, 2)[:T] * pitch
    truths = np.c_[g + rng.uniform(-0.2, 0.2, (T, 2)) * pitch, np.zeros(T)]
    det = truths[rng.choice(T, n_det, replace=False)] + np.c_[rng.normal(0, sigma, (n_det, 2)), np.zeros(n_det)]
    near = det[rng.integers(0, n_det, n_clutter // 4)] + np.c_[rng.normal(0, 2 * sigma, (n_clutter // 4, 2)),
                                                                np.zeros(n_clutter // 4)]
    far = np.c_[rng.uniform(-1, side, (n_clutter - n_clutter // 4, 2)) * pitch, np.zeros(n_clutter - n_clutter // 4)]
    centers = np.r_[det, near, far]
    return centers[rng.permutation(len(centers))], truths
