"""vcp_eps_tree restated in numpy, brute force: the n x n matrix of d with the exact expression and operand order, kdist
from a row sort, the Kruskal walk over the edges in ascending (w, i, j) order, and reach.  The library's result is held
to this for equality, bit for bit (include/vcp.h: the walk is the specification)."""
import numpy as np

L1_2D, L2_2D, L2_3D = 0, 1, 2


def dist_matrix(c, metric):
    """d(i, j) for all pairs: the binary64 expression vcp_dbscan tests (left to right, no FMA)."""
    with np.errstate(all="ignore"):
        dx = c[:, None, 0] - c[None, :, 0]
        dy = c[:, None, 1] - c[None, :, 1]
        if metric == L1_2D:
            return np.abs(dx) + np.abs(dy)
        if metric == L2_2D:
            return np.sqrt(dx * dx + dy * dy)
        dz = c[:, None, 2] - c[None, :, 2]
        return np.sqrt(dx * dx + dy * dy + dz * dz)


def finite_rows(c, metric):
    return np.isfinite(c[:, :3 if metric == L2_3D else 2]).all(1)


def kdist_of(D, fin, k):
    """k-th smallest d(i, j) over the finite j (j = i included); +inf with fewer than k of them, NaN for a non-finite i."""
    n = len(D)
    kd = np.full(n, np.nan)
    idx = np.nonzero(fin)[0]
    if idx.size:
        rows = np.sort(D[np.ix_(idx, idx)], axis=1)
        kd[idx] = rows[:, k - 1] if idx.size >= k else np.inf
    return kd


def eps_tree(coords, k, eps_max, metric, kdist=None):
    """dict(kdist, reach, n_merge, merge_w, merge_a, merge_b, n_p): the specification of vcp_eps_tree."""
    c = np.ascontiguousarray(coords, np.float64)
    if c.ndim != 2:
        c = c.reshape(0, 2)
    n = len(c)
    fin = finite_rows(c, metric)
    D = dist_matrix(c, metric)
    kd = kdist_of(D, fin, k) if kdist is None else np.array(kdist, np.float64)
    with np.errstate(invalid="ignore"):
        inp = fin & (kd <= eps_max)
        near = (D <= eps_max) & fin[:, None] & fin[None, :]
    # reach[i] = min over j in P with d(i, j) <= eps_max of max(kdist[j], d(i, j))
    reach = np.full(n, np.nan)
    with np.errstate(invalid="ignore"):
        cand = np.where(near & inp[None, :], np.maximum(kd[None, :], D), np.inf)
    if n:
        reach[fin] = cand[fin].min(axis=1)
    # the Kruskal walk
    i, j = np.nonzero(np.triu(near & inp[:, None] & inp[None, :], 1))
    w = np.maximum(np.maximum(kd[i], kd[j]), D[i, j])
    order = np.lexsort((j, i, w))
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    mw, ma, mb = [], [], []
    for t in order.tolist():
        a, b = int(i[t]), int(j[t])
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[ra] = rb
            mw.append(w[t])
            ma.append(a)
            mb.append(b)
    return dict(kdist=kd, reach=reach, n_merge=len(mw), merge_w=np.array(mw, np.float64), merge_a=np.array(ma, np.int32),
                merge_b=np.array(mb, np.int32), n_p=int(inp.sum()))


def w_matrix(coords, k, metric):
    """(w, kdist): the full matrix of mutual-reachability weights max(kdist[i], kdist[j], d(i, j))."""
    c = np.ascontiguousarray(coords, np.float64)
    D = dist_matrix(c, metric)
    kd = kdist_of(D, finite_rows(c, metric), k)
    return np.maximum(np.maximum(kd[:, None], kd[None, :]), D), kd


def round_bound(n_p):
    """floor(log2 |P|), 0 when |P| < 2."""
    return int(n_p).bit_length() - 1 if n_p >= 2 else 0


def same(got, ref):
    """Bits of the doubles, values of the integers; returns the name of the first field that differs, or None."""
    for key in ("kdist", "reach", "merge_w"):
        a, b = np.ascontiguousarray(got[key], np.float64), np.ascontiguousarray(ref[key], np.float64)
        if a.shape != b.shape or not np.array_equal(a.view(np.uint64), b.view(np.uint64)):
            # every NaN the library writes is the quiet NaN of its own NAN; compare NaN-ness, not payloads
            if a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)) or \
                    not np.array_equal(a[~np.isnan(a)].view(np.uint64), b[~np.isnan(b)].view(np.uint64)):
                return key
    for key in ("merge_a", "merge_b"):
        if got.get(key) is not None and not np.array_equal(got[key], ref[key]):
            return key
    if "n_merge" in got and got["n_merge"] != ref["n_merge"]:
        return "n_merge"
    return None


def boruvka(coords, k, eps_max, metric, seed=0):
    """Host emulation of the device's rounds (csrc/eps_tree.hip), step for step: the vertices of P in an arbitrary slot
    order (`seed` shuffles it, as the atomics do inside a cell), per round every non-interior slot's best key (w, lo, hi)
    to another component (kept from the round before while it still leaves the component), the component words lowered first to w and then to lo << 32 | hi, the hook of the one slot that
    holds both -- the larger root alone on a mutual pick -- and the flattening.  Returns (merge_w, merge_a, merge_b,
    rounds) with the edges sorted by key; it must equal eps_tree()'s walk."""
    c = np.ascontiguousarray(coords, np.float64)
    D = dist_matrix(c, metric)
    fin = finite_rows(c, metric)
    kd = kdist_of(D, fin, k)
    with np.errstate(invalid="ignore"):
        slots = np.nonzero(fin & (kd <= eps_max))[0]
    slots = slots[np.random.default_rng(seed).permutation(len(slots))]
    np_ = len(slots)
    comp = list(range(np_))
    interior = [False] * np_
    edges, rounds = [], 0
    Dp = D[np.ix_(slots, slots)]
    Wp = np.maximum(np.maximum(kd[slots][:, None], kd[slots][None, :]), Dp)
    near = Dp <= eps_max
    best = [None] * np_
    while len(edges) + 1 < np_:
        best_prev, best = best, [None] * np_
        cw, ce = {}, {}
        for s in range(np_):                                   # k_et_best
            if interior[s]:
                continue
            b = best_prev[s]
            if b is not None and comp[b[3]] != comp[s]:        # last round's best still leaves the component: kept
                best[s] = b
                cw[comp[s]] = min(cw.get(comp[s], np.inf), b[0])
                continue
            b = None
            for t in np.nonzero(near[s])[0].tolist():
                if comp[t] == comp[s]:
                    continue
                i, j = int(slots[s]), int(slots[t])
                key = (Wp[s, t], min(i, j), max(i, j), t)
                if b is None or key[:3] < b[:3]:
                    b = key
            best[s] = b
            if b is None:
                interior[s] = True
            else:
                cw[comp[s]] = min(cw.get(comp[s], np.inf), b[0])
        for s in range(np_):                                   # k_et_name
            if best[s] is not None and best[s][0] == cw[comp[s]]:
                e = best[s][1:3]
                ce[comp[s]] = min(ce.get(comp[s], e), e)
        par = list(range(np_))
        emitted = 0
        for s in range(np_):                                   # k_et_hook
            b = best[s]
            if b is None or b[0] != cw[comp[s]] or b[1:3] != ce[comp[s]]:
                continue
            cs, co = comp[s], comp[b[3]]
            if cw.get(co) == b[0] and ce.get(co) == b[1:3] and cs < co:
                continue
            par[cs] = co
            edges.append(b[:3])
            emitted += 1
        if not emitted:
            break
        rounds += 1
        for s in range(np_):                                   # k_et_flat
            r, steps = comp[s], 0
            while par[r] != r:
                r = par[r]
                steps += 1
                assert steps <= np_, "a cycle of hooks"
            comp[s] = r
    edges.sort()
    return (np.array([e[0] for e in edges], np.float64), np.array([e[1] for e in edges], np.int32),
            np.array([e[2] for e in edges], np.int32), rounds)
