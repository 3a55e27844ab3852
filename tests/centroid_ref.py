"""The centroid kernels' summation tree (csrc/centroids.hip on csrc/reduce.hpp) replayed in numpy binary64, the exact
means in rational arithmetic, the a-priori error bound of the tree, and the shared input set of the centroid tests.
No GPU, no oracle.

The order the kernels state, and the replay follows:
  * the members of a label in ascending point index (the stable sort of (label, index));
  * chunks of CH = 16384 consecutive members, one workgroup of 256 threads each;
  * thread t adds members t, t + 256, t + 512, ... of its chunk in that order, starting from +0.0;
  * inside a wave, __shfl_down at offsets 32, 16, 8, 4, 2, 1: lane 0 ends with 6 pairwise levels over the 64 lanes;
  * the 4 wave results are added in wave order, the chunk results in chunk order starting from 0.0, then ONE division.
A thread's sum starts at +0.0 and (+0.0) + (-0.0) = +0.0, so it is never -0.0 and adding +0.0 to it changes nothing
(NaN stays NaN, payloads aside): padding a chunk with +0.0 rows is exact, and the replay pads only to whole rows of
256.  Every numpy operation below is one binary64 ufunc call; numpy contracts nothing.
"""
from fractions import Fraction

import numpy as np

CH = 16384   # members per chunk (centroids.hip)
CT = 256     # threads per workgroup
U = Fraction(1, 2 ** 53)   # unit roundoff of binary64

# the kernel's order; every other setting of a knob breaks exactly one property of it
KERNEL = dict(chunk_reversed=False, wave_reversed=False, lane_tree=True, threads=CT, descending=False, chunk_len=CH)
KNOBS = {
    "chunk_reversed": dict(chunk_reversed=True),
    "wave_reversed": dict(wave_reversed=True),
    "lane_sequential": dict(lane_tree=False),
    "threads_128": dict(threads=128),
    "members_descending": dict(descending=True),
    "chunk_len_minus_1": dict(chunk_len=CH - 1),
    "chunk_len_plus_1": dict(chunk_len=CH + 1),
}


def _members(labels, K):
    """idx[k - 1] = the point indices carrying label k, ascending (k = 1..K)."""
    labels = np.ascontiguousarray(labels, np.int32)
    order = np.argsort(labels, kind="stable")
    cut = np.searchsorted(labels[order], np.arange(1, K + 2))
    return [order[cut[k]:cut[k + 1]] for k in range(K)]


def _chunk_partial(v, cfg):
    """One workgroup: v [m, A] (m <= chunk length) -> [A]."""
    tb = cfg["threads"]
    m, A = v.shape
    rows = -(-m // tb)
    pad = np.zeros((rows * tb, A))
    pad[:m] = v
    pad = pad.reshape(rows, tb, A)
    acc = np.zeros((tb, A))
    for r in range(rows):            # thread t: members t, t + tb, ... in order
        acc = acc + pad[r]
    w = acc.reshape(tb // 64, 64, A)
    if cfg["lane_tree"]:
        d = 32
        while d:                     # lane i takes lane i + d; only lanes < d feed lane 0
            w = w[:, :d] + w[:, d:2 * d]
            d >>= 1
        w = w[:, 0]
    else:
        r = w[:, 0]
        for lane in range(1, 64):
            r = r + w[:, lane]
        w = r
    order = list(range(tb // 64))
    if cfg["wave_reversed"]:
        order.reverse()
    r = w[order[0]]
    for j in order[1:]:
        r = r + w[j]
    return r


def _tree_sums(vals, idx, cfg):
    """vals [n, A], idx = _members(...) -> sums [K, A] (0.0 rows for empty labels), counts [K]."""
    K, A = len(idx), vals.shape[1]
    sums = np.zeros((K, A))
    counts = np.zeros(K, np.int64)
    ch = cfg["chunk_len"]
    with np.errstate(all="ignore"):
        for k, ix in enumerate(idx):
            counts[k] = len(ix)
            if cfg["descending"]:
                ix = ix[::-1]
            v = vals[ix]
            parts = [_chunk_partial(v[b:b + ch], cfg) for b in range(0, len(ix), ch)]
            if cfg["chunk_reversed"]:
                parts.reverse()
            s = np.zeros(A)
            for p in parts:
                s = s + p
            sums[k] = s
    return sums, counts


def _cfg(knobs):
    cfg = dict(KERNEL)
    for k in knobs:
        if k not in KERNEL:
            raise TypeError("unknown replay knob %r" % k)
    cfg.update(knobs)
    return cfg


def tree_centroids(xyz, motor, labels, K, **knobs):
    """Context.centroids: (c3 [K,3], c2 [K,2], counts [K]); NaN rows for empty labels and for an absent input."""
    cfg = _cfg(knobs)
    idx = _members(labels, K)
    out = []
    for a, c in ((xyz, 3), (motor, 2)):      # one pass per array: no joined copy of a 50 M-point cloud
        if a is None:
            out.append(np.full((K, c), np.nan))
            continue
        sums, counts = _tree_sums(np.ascontiguousarray(a, np.float64).reshape(-1, c), idx, cfg)
        with np.errstate(all="ignore"):
            out.append(np.where(counts[:, None] > 0, sums / counts[:, None].astype(np.float64), np.nan))
    return out[0], out[1], np.array([len(ix) for ix in idx], np.int64)


def weights_of(group, cluster_id, pts_count, ignore_dup):
    """w of getFixedPtsCentroid: 1 where the member's clusterId != 0 and duplicates are ignored, else its ptsCount."""
    cid = np.asarray(group if cluster_id is None else cluster_id, np.int32)
    pc = np.asarray(pts_count, np.int32)
    return np.where((cid != 0) & bool(ignore_dup), 1, pc).astype(np.int64)


def tree_centroids_weighted(xyz, group, cluster_id, pts_count, K, ignore_dup, **knobs):
    """Context.centroids_weighted: (c3 [K,3], inside_num [K]).  x * w is rounded before it is added (the library is
    built without FMA contraction); the fourth sum is sum(w); the result is s / sum(w) (0/0 = NaN)."""
    cfg = _cfg(knobs)
    xyz = np.ascontiguousarray(xyz, np.float64).reshape(-1, 3)
    w = weights_of(group, cluster_id, pts_count, ignore_dup).astype(np.float64)
    with np.errstate(all="ignore"):
        vals = np.concatenate([xyz * w[:, None], w[:, None]], axis=1)
        sums, _ = _tree_sums(vals, _members(group, K), cfg)
        c3 = sums[:, :3] / sums[:, 3:4]
    return np.ascontiguousarray(c3), sums[:, 3].astype(np.int64)


def relabel(labels, K, map_by_id):
    """refreshCensAndClusByDictionary's relabelling: merged ids go to their target, survivors are renumbered 1..K' in
    ascending id.  Returns (labels', K')."""
    labels = np.asarray(labels, np.int32)
    m = np.asarray(map_by_id, np.int32)
    alive = m == 0
    rank = np.cumsum(alive) - alive          # exclusive scan
    target = np.where(alive, np.arange(1, K + 1), m)
    new_of = np.concatenate([[0], rank[target - 1] + 1]).astype(np.int32)
    return new_of[labels], int(alive.sum())


def tree_refresh(xyz, motor, labels, K, map_by_id, **knobs):
    """Context.refresh_by_dictionary: (labels', K', c3, c2, counts).  The kernel relabels first and then sorts by
    (label, index), so a merged cluster's members are summed in ascending point index, not appended."""
    lab, nk = relabel(labels, K, map_by_id)
    c3, c2, counts = tree_centroids(xyz, motor, lab, nk, **knobs)
    return lab, nk, c3, c2, counts


# ---- exact arithmetic ----------------------------------------------------------------------------------------------
def _exact_int_sum(x, w=None):
    """sum(w * x) of finite binary64 x (w integers, default 1) as a Fraction, no rounding anywhere: the 53-bit
    mantissas are split in halves and added per exponent in int64, the exponents are combined in Python integers."""
    x = np.asarray(x, np.float64)
    if len(x) == 0:
        return Fraction(0)
    m, e = np.frexp(x)
    mi = (m * 2.0 ** 53).astype(np.int64)   # |m| < 1: m * 2^53 is an integer below 2^53
    hi = mi >> 26
    lo = mi - (hi << 26)                    # 0 <= lo < 2^26
    if w is not None:
        w = np.asarray(w, np.int64)
        assert len(x) * int(np.abs(w).max()) < 2 ** 35   # the int64 sums below cannot overflow
        hi, lo = hi * w, lo * w
    else:
        assert len(x) < 2 ** 35
    order = np.argsort(e, kind="stable")
    es = e[order]
    first = np.flatnonzero(np.r_[True, es[1:] != es[:-1]])
    H, L = np.add.reduceat(hi[order], first), np.add.reduceat(lo[order], first)
    e0 = int(es[0])
    tot = sum(((int(h) << 26) + int(l)) << (int(ee) - e0) for h, l, ee in zip(H, L, es[first]))
    return Fraction(tot) * Fraction(2) ** (e0 - 53)


def exact_means(vals, labels, K, w=None):
    """[K][A] Fractions: sum(w x) / sum(w) per label and column of vals [n, A] (w = None: the plain mean); None for a
    label with sum(w) == 0.  The inputs must be finite."""
    vals = np.asarray(vals, np.float64)
    out = []
    for ix in _members(labels, K):
        wk = None if w is None else np.asarray(w)[ix]
        den = len(ix) if w is None else int(np.asarray(wk, np.int64).sum())
        out.append(None if den == 0 else [_exact_int_sum(vals[ix, a], wk) / den for a in range(vals.shape[1])])
    return out


def gamma(d):
    return d * U / (1 - d * U)


def tree_depth(n):
    """Additions an input passes through at most: its thread's (CH/256), 6 lane levels, 3 wave adds, one per chunk."""
    return CH // CT + 6 + 3 + -(-n // CH)


def bound(vals, labels, K, w=None, sequential=False):
    """[K][A] Fractions b with |c - mean| <= b for the tree (default) or for a sequential sum in list order:
        tree:        gamma_d * sum|x| / n * (1 + u) + u * |mean|,  d = tree_depth(n)
        sequential:  gamma_(n-1) * sum|x| / n
    weighted (w given): d + 1 (the rounded product), sum|w x| and sum(w) in place of d, sum|x| and n; sequential: n.
    It presumes no overflow and no underflow (DESIGN.md lists what happens then)."""
    vals = np.asarray(vals, np.float64)
    means = exact_means(vals, labels, K, w)
    out = []
    for k, ix in enumerate(_members(labels, K)):
        if means[k] is None:
            out.append(None)
            continue
        n = len(ix)
        wk = None if w is None else np.asarray(w)[ix]
        den = n if w is None else int(np.asarray(wk, np.int64).sum())
        extra = 0 if w is None else 1
        row = []
        for a in range(vals.shape[1]):
            sabs = _exact_int_sum(np.abs(vals[ix, a]), wk)
            if sequential:
                row.append(gamma(n - 1 + extra) * sabs / den)
            else:
                row.append(gamma(tree_depth(n) + extra) * sabs / den * (1 + U) + U * abs(means[k][a]))
        out.append(row)
    return out


# ---- the shared input set ------------------------------------------------------------------------------------------
SIZES = [1, 2, 63, 64, 65, 255, 256, 257, CH - 1, CH, CH + 1, 2 * CH - 1, 2 * CH, 2 * CH + 1, 3 * CH + 17]
SLOTS = [2 + 17 * j for j in range(len(SIZES))]    # their labels: 2, 19, ..., 240; every other label is empty,
N_POINTS = 250_000                                  # label 1 and label K (255 / 256 / 257) among them
FAMILIES = ("uniform", "offset", "cancel", "range", "grid")
INEXACT = ("uniform", "offset", "cancel", "range")  # families whose sums round


def case_labels(seed=1):
    """[N_POINTS] int32: SIZES[j] points of label SLOTS[j], the rest noise (0), scattered by a fixed permutation."""
    lab = np.zeros(N_POINTS, np.int32)
    lab[:sum(SIZES)] = np.repeat(np.array(SLOTS, np.int32), SIZES)
    return np.ascontiguousarray(lab[np.random.default_rng(seed).permutation(N_POINTS)])


def case_values(family, labels, cols, seed=2):
    """[n, cols] float64 of one value family.
      uniform  in +-100
      offset   1e8 plus a unit spread          (atol = 1e-12 means nothing here)
      cancel   +-M in pairs plus a unit spread (the mean is ~1, the members ~1e6: rtol means nothing here)
      range    17 decades, random sign
      grid     multiples of 2^-10 below 100    (every partial sum is exact)"""
    rng = np.random.default_rng([seed, FAMILIES.index(family), cols])
    n = len(labels)
    if family == "uniform":
        return rng.uniform(-100, 100, (n, cols))
    if family == "offset":
        return 1e8 + rng.uniform(-0.5, 0.5, (n, cols))
    if family == "range":
        return 10.0 ** rng.uniform(-8, 9, (n, cols)) * rng.choice([-1.0, 1.0], (n, cols))
    if family == "grid":
        return np.round(rng.uniform(0, 100, (n, cols)) * 1024) / 1024
    if family == "cancel":
        v = rng.uniform(-1, 1, (n, cols))
        for ix in _members(labels, int(labels.max())):
            m = len(ix)
            mag = np.repeat(rng.uniform(1e5, 1e6, (-(-m // 2), cols)), 2, axis=0)[:m]
            ix = ix[rng.permutation(m)]  # the partners sit anywhere in the cluster: no level of the tree is exact
            sign = np.where(np.arange(m) % 2 == 0, 1.0, -1.0)[:, None]
            v[ix] += sign * mag
        return v
    raise ValueError(family)


def case(family, seed=1):
    """(xyz [n,3], motor [n,2], labels [n]) of one family on the shared labels."""
    lab = case_labels(seed)
    return case_values(family, lab, 3, seed + 1), case_values(family, lab, 2, seed + 1), lab


def case_weights(labels, seed=5):
    """(cluster_id, pts_count): weights 1..8, near 2^20 in the 257-member cluster (sum(w) stays below 2^31: the C#'s
    insideNum is a 32-bit int); about a fifth of the members carry clusterId 0."""
    rng = np.random.default_rng(seed)
    n = len(labels)
    pts = rng.integers(1, 9, n).astype(np.int32)
    cnt = np.bincount(labels)
    big = labels == [k for k in range(1, len(cnt)) if cnt[k] == 257][0]   # whatever label that cluster carries
    pts[big] = (2 ** 20 - rng.integers(0, 16, int(big.sum()))).astype(np.int32)
    cid = np.where(rng.random(n) < 0.2, 0, labels).astype(np.int32)
    return cid, pts


def compact(labels):
    """The labels with the empty ones squeezed out (1..15): an empty list is an error in the weighted form."""
    new_of = np.zeros(max(SLOTS) + 1, np.int32)
    new_of[SLOTS] = np.arange(1, len(SLOTS) + 1)
    return new_of[labels], len(SLOTS)


def case_dictionary(K):
    """map_by_id [K] for refresh_by_dictionary on the shared labels: every empty label is merged into a live one (a
    surviving empty cluster is an error), and three live clusters are merged so that sizes land on chunk boundaries:
    1 into CH - 1 (= CH), 2 into 2 CH - 1 (= 2 CH + 1), 63 into CH + 1."""
    m = np.zeros(K, np.int32)
    slot = dict(zip(SIZES, SLOTS))
    live = [s for s in SLOTS if s not in (slot[1], slot[2], slot[63])]
    for k in range(1, K + 1):
        if k not in SLOTS:
            m[k - 1] = live[k % len(live)]
    m[slot[1] - 1] = slot[CH - 1]
    m[slot[2] - 1] = slot[2 * CH - 1]
    m[slot[63] - 1] = slot[CH + 1]
    return m


BIG = 1e308
SUB = 5e-324


def kind_cases():
    """Inputs on which the tree and a sequential sum differ in kind, not in last bits: name -> one column of members
    (every coordinate of xyz and motor carries it; one cluster, K = 1)."""
    return {
        "overflow_sequential_only": np.array([BIG, BIG, -BIG, -BIG]),   # tree: lanes 0+2 and 1+3 cancel first
        "overflow_tree_only": np.array([BIG, -BIG, BIG, -BIG]),         # tree: lanes 0+2 = inf, 1+3 = -inf -> NaN
        "negative_zero": np.full(5, -0.0),
        "subnormal": np.array([3 * SUB, SUB, SUB]),
        "inf_member": np.array([1.0, np.inf, 2.0]),
        "inf_both_signs": np.array([np.inf, 1.0, -np.inf]),
        "nan_member": np.array([1.0, np.nan, 2.0]),
    }


def kind_arrays(col):
    n = len(col)
    return np.repeat(col[:, None], 3, 1).copy(), np.repeat(col[:, None], 2, 1).copy(), np.ones(n, np.int32)
