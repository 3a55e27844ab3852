"""vcp_cluster_quantiles' and vcp_cluster_mad's definition (include/vcp.h) restated in numpy: the key map on the bit
patterns, an np.sort of the keys per group, the rank formula, and the MAD chain with its single subtraction.  The tests
compare the library with it for equality, doubles by their bits.  Also the inputs the tests share."""
import numpy as np

NAN_KEY = np.uint64(0xFFFFFFFFFFFFFFFF)
SIGN = np.uint64(0x8000000000000000)
NAN_BITS = np.uint64(0x7FF8000000000000)
CANON_NAN = np.array([NAN_BITS]).view(np.float64)[0]
WAVE_MAX, WG_MAX, NQ_MAX = 64, 4096, 16      # VCP_CQ_WAVE_MAX, VCP_CQ_WG_MAX, VCP_CQ_NQ_MAX (tests hold them to the header)


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def key(v):
    """The key of every value: unsigned order = numeric order, -0 before +0, every NaN last."""
    v = np.ascontiguousarray(v, np.float64)
    u = v.view(np.uint64)
    k = np.where((u & SIGN) != 0, ~u, u ^ SIGN)
    return np.where(np.isnan(v), NAN_KEY, k).astype(np.uint64)


def unkey(k):
    k = np.ascontiguousarray(k, np.uint64)
    u = np.where((k & SIGN) != 0, k ^ SIGN, ~k)
    return np.where(k == NAN_KEY, NAN_BITS, u).astype(np.uint64).view(np.float64)


def rank(q, c):
    return int(np.floor(np.float64(q) * np.float64(c - 1)))


def rows(values, n, stride=1):
    return np.ascontiguousarray(values, np.float64).reshape(-1)[: max((n - 1) * stride + 1, 0) : stride][:n]


def quantiles(values, group, K, q, stride=1):
    """(out [K, nq], counts [K])."""
    group = np.asarray(group, np.int32).reshape(-1)
    v = rows(values, len(group), stride)
    q = np.asarray(q, np.float64).reshape(-1)
    out = np.full((K, len(q)), CANON_NAN)
    counts = np.zeros(K, np.int64)
    k_all = key(v)
    for k in range(1, K + 1):
        ks = np.sort(k_all[group == k])
        counts[k - 1] = c = len(ks)
        if c:
            out[k - 1] = unkey(np.array([ks[rank(x, c)] for x in q], np.uint64))
    return out, counts


def mad(values, group, K, c_mad=3.0, floor=0.0, stride=1):
    """dict(med, mad, thr [K], reject [n] uint8, kept [K] int64, n_rejected)."""
    group = np.asarray(group, np.int32).reshape(-1)
    v = rows(values, len(group), stride)
    med = quantiles(v, group, K, [0.5])[0][:, 0]
    mk = np.where(group >= 1, group - 1, 0)
    with np.errstate(invalid="ignore"):
        dev = np.abs(v - (med[mk] if K else np.zeros(len(v))))       # one subtraction in binary64
        md = quantiles(dev, group, K, [0.5])[0][:, 0]
        band = np.float64(c_mad) * md
        thr = np.where(band > np.float64(floor), band, np.float64(floor))
        reject = (group >= 1) & ~(dev <= (thr[mk] if K else np.zeros(len(v))))
    kept = np.array([int(((group == k) & ~reject).sum()) for k in range(1, K + 1)], np.int64).reshape(K)
    return dict(med=med, mad=md, thr=thr, reject=reject.astype(np.uint8), kept=kept, n_rejected=int(reject.sum()))


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape:
        return False
    if a.dtype == np.float64:
        return b.dtype == np.float64 and np.array_equal(bits(a), bits(b))
    return np.array_equal(a, b)


MAD_KEYS = ("med", "mad", "thr", "reject", "kept")


def same_mad(got, want):
    """None, or the name of the first entry that differs."""
    for nm in MAD_KEYS:
        if not same_bits(got[nm], want[nm]):
            return nm
    return None if int(got["n_rejected"]) == int(want["n_rejected"]) else "n_rejected"


# ---- shared inputs -----------------------------------------------------------------------------------------------------------
def hard_values():
    """Values the key has to order right: +-0, subnormals, +-inf, NaNs with payloads and either sign, one-ulp neighbours."""
    tiny = np.array([1, 2, 0x000FFFFFFFFFFFFF, 0x0010000000000000], np.uint64).view(np.float64)
    nans = np.array([0x7FF8000000000000, 0x7FF0000000000001, 0x7FFFFFFFFFFFFFFF, 0xFFF8000000000000, 0xFFF0000000000001,
                     0xFFFFFFFFFFFFFFFF, 0x7FF8000000000123], np.uint64).view(np.float64)
    base = np.array([0.0, -0.0, 1.0, -1.0, 1.5, -2.5, 1e300, -1e300, 1e-300, 123.456, np.inf, -np.inf,
                     np.finfo(np.float64).max, np.finfo(np.float64).tiny])
    nb = np.concatenate([np.nextafter(base[2:10], np.inf), np.nextafter(base[2:10], -np.inf)])
    return np.concatenate([base, tiny, -tiny, nb, nans])


def size_class_case(seed, stride=1):
    """One call with a group of every size in {0, 1, 2, 3, 63, 64, 65}, each class limit L at L - 1, L, L + 1 and a group of
    about 5 L, the rows interleaved in random order with rows of group 0.  Returns (values (flat, strided), group, K, sizes)."""
    rng = np.random.default_rng(seed)
    sizes = [0, 1, 2, 3, 63, 64, 65, WAVE_MAX - 1, WAVE_MAX, WAVE_MAX + 1, 5 * WAVE_MAX, WG_MAX - 1, WG_MAX, WG_MAX + 1,
             5 * WG_MAX + 7]
    K = len(sizes)
    group = np.concatenate([np.full(s, k + 1, np.int32) for k, s in enumerate(sizes)] + [np.zeros(3000, np.int32)])
    rng.shuffle(group)
    n = len(group)
    v = rng.normal(50.0, 20.0, n)
    v[rng.integers(0, n, n // 50)] = np.round(v[rng.integers(0, n, n // 50)])   # some ties
    flat = rng.normal(0.0, 1.0, (n - 1) * stride + 1) if stride > 1 else np.zeros(n)
    flat[::stride] = v
    return flat, group, K, sizes


def mad_scene(seed=7):
    """3 000 rows in 6 groups at ranges 5 .. 600 (noise sigma 0.02), 5 % of every group planted 3 .. 8 away from its range:
    nearer than the gap between two groups' ranges, so that no single band of Distance separates them.  Returns (dist,
    group, planted [n] bool, K)."""
    rng = np.random.default_rng(seed)
    centres = np.array([5.0, 12.0, 40.0, 41.5, 250.0, 600.0])
    K, per = len(centres), 500
    group = np.repeat(np.arange(1, K + 1, dtype=np.int32), per)
    dist = centres[group - 1] + rng.normal(0.0, 0.02, K * per)
    planted = np.zeros(K * per, bool)
    for k in range(K):
        idx = k * per + rng.choice(per, per // 20, replace=False)
        planted[idx] = True
        dist[idx] = centres[k] + rng.choice([-1.0, 1.0], len(idx)) * rng.uniform(3.0, 8.0, len(idx))
    order = rng.permutation(K * per)
    return dist[order], group[order], planted[order], K
