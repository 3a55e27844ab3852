"""The definition of vcp_gdbscan (include/vcp.h) restated in numpy, O(n^2): the boolean neighbourhood matrix, int64
weighted row sums, union by smaller root, ids by smallest core index, border = max.  The device is compared with this for
equality (tests/test_gdbscan_gpu.py); this is compared with the project's oracle and with scikit-learn
(tests/test_gdbscan.py)."""
import numpy as np

L1_2D, L2_2D, L2_3D = 0, 1, 2


def dist_matrix(c, metric):
    """d(i, j) of vcp_kdist: binary64, sums left to right, correctly rounded sqrt."""
    c = np.asarray(c, np.float64)
    with np.errstate(all="ignore"):
        dx = c[:, None, 0] - c[None, :, 0]
        dy = c[:, None, 1] - c[None, :, 1]
        if metric == L1_2D:
            return np.abs(dx) + np.abs(dy)
        if metric == L2_2D:
            return np.sqrt(dx * dx + dy * dy)
        dz = c[:, None, 2] - c[None, :, 2]
        return np.sqrt(dx * dx + dy * dy + dz * dz)


def neighbourhoods(c, eps, metric, aux=None, gate=None):
    """N [n, n] bool: N[i, j] <=> j in N(i)."""
    c = np.asarray(c, np.float64)
    gd = 3 if metric == L2_3D else 2
    fin = np.isfinite(c[:, :gd]).all(1)
    with np.errstate(all="ignore"):
        N = dist_matrix(c, metric) <= eps
        if aux is not None:
            aux = np.asarray(aux, np.float64)
            fin &= np.isfinite(aux)
            N &= np.abs(aux[:, None] - aux[None, :]) <= gate
    return N & fin[:, None] & fin[None, :]


def _find(par, x):
    while par[x] != x:
        par[x] = par[par[x]]
        x = par[x]
    return x


def gdbscan(coords, eps, min_weight, metric=L1_2D, weights=None, aux=None, gate=None, cf_in=0):
    """dict(labels int32 [n], is_core uint8 [n], wsum int64 [n], cf)."""
    c = np.asarray(coords, np.float64)
    n = len(c)
    if n == 0:
        return dict(labels=np.zeros(0, np.int32), is_core=np.zeros(0, np.uint8), wsum=np.zeros(0, np.int64), cf=cf_in)
    N = neighbourhoods(c, eps, metric, aux, gate)
    w = np.ones(n, np.int64) if weights is None else np.asarray(weights).astype(np.int64)
    wsum = N.astype(np.int64) @ w
    core = wsum >= min_weight
    par = list(range(n))
    ii, jj = np.nonzero(np.tril(N, -1) & core[:, None] & core[None, :])
    for i, j in zip(ii.tolist(), jj.tolist()):
        a, b = _find(par, i), _find(par, j)
        if a != b:
            par[max(a, b)] = min(a, b)           # the root of a component is its smallest index
    root = np.array([_find(par, i) for i in range(n)])
    first = np.zeros(n, np.int64)
    first[np.unique(root[core])] = 1
    rank = np.cumsum(first) - first
    labels = np.zeros(n, np.int64)
    labels[core] = rank[root[core]] + cf_in + 1
    for i in np.nonzero(~core)[0].tolist():
        ids = labels[N[i] & core]
        if len(ids):
            labels[i] = ids.max()
    return dict(labels=labels.astype(np.int32), is_core=core.astype(np.uint8), wsum=wsum, cf=cf_in + int(first.sum()))


def expand(c, weights):
    """The cloud in which row j stands weights[j] times (>= 1): the copies appended after index n - 1."""
    c = np.asarray(c, np.float64)
    extra = np.repeat(np.arange(len(c)), np.asarray(weights) - 1)
    return np.concatenate([c, c[extra]])


def renumber(labels, core, cf_in=0):
    """Ids renumbered by smallest core member (the clusters of several runs laid over one index space)."""
    labels = np.asarray(labels)
    out = np.zeros(len(labels), np.int32)
    ids = labels[np.asarray(core, bool)]
    idx = np.nonzero(np.asarray(core, bool))[0]
    seen = {}
    for i, l in zip(idx.tolist(), ids.tolist()):
        seen.setdefault(l, i)
    order = sorted(seen, key=seen.get)
    new = {l: cf_in + 1 + k for k, l in enumerate(order)}
    for i, l in enumerate(labels.tolist()):
        if l != 0:
            out[i] = new[l]
    return out, len(order)


def same(g, r, wsum=True):
    """None when the device result g equals the restatement r, else the name of the first field that differs."""
    if not np.array_equal(g["labels"], r["labels"]):
        return "labels"
    if not np.array_equal(np.asarray(g["is_core"]) != 0, np.asarray(r["is_core"]) != 0):
        return "is_core"
    if g["cf"] != r["cf"]:
        return "cf"
    if wsum and g.get("wsum") is not None and not np.array_equal(g["wsum"], r["wsum"]):
        return "wsum"
    return None
