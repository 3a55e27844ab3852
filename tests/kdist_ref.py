"""vcp_kdist restated in numpy, brute force: the binary64 expression of include/vcp.h row by row and the k smallest
(d, j) pairs over the finite points.  The device is compared with this for equality (tests/test_kdist_gpu.py,
tests/fuzz_queries.py).  No GPU here."""
import numpy as np

L1_2D, L2_2D, L2_3D = 0, 1, 2


def dist_rows(c, q, metric):
    """d(q, j) for every row of c, the expression vcp_dbscan tests (numpy: IEEE binary64, left to right, no FMA)."""
    dx = q[0] - c[:, 0]
    dy = q[1] - c[:, 1]
    if metric == L1_2D:
        return np.abs(dx) + np.abs(dy)
    if metric == L2_2D:
        return np.sqrt(dx * dx + dy * dy)
    dz = q[2] - c[:, 2]
    return np.sqrt(dx * dx + dy * dy + dz * dz)


def brute_rows(c, k, metric, rows):
    """kdist and knn of the given rows: k smallest (d, j) pairs over the finite points."""
    gd = 3 if metric == L2_3D else 2
    fin = np.isfinite(c[:, :gd]).all(1)
    fidx = np.nonzero(fin)[0]
    cf = c[fidx]
    kd = np.full(len(rows), np.nan)
    knn = np.full((len(rows), k), -1, np.int32)
    for r, i in enumerate(rows):
        if not fin[i]:
            continue
        d = dist_rows(cf, c[i], metric)
        if len(d) > k:
            v = np.partition(d, k - 1)[k - 1]
            sel = np.nonzero(d <= v)[0]
        else:
            sel = np.arange(len(d))
        o = sel[np.argsort(d[sel], kind="stable")][:k]  # stable on ascending j: lexicographic (d, j)
        knn[r, :len(o)] = fidx[o]
        kd[r] = d[o[k - 1]] if len(o) >= k else np.inf
    return kd, knn
