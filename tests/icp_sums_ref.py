"""The ICP round's 16 binary64 moment sums (csrc/icp.hip: k_icp_pass / k_icp_pass_small, folded by k_icp_step on
csrc/reduce.hpp) replayed in numpy binary64, the exact sums in rational arithmetic, the a-priori error bound of the
tree, the ways of getting the tree wrong, and the shared input set of the ICP sums tests.  No GPU, no oracle.

The order the kernels state, and the replay follows.

Point terms.  For data point i, with the pass's R (row major) and T:
    p[r] = (((0.0 + R[3r] * d0) + R[3r+1] * d1) + R[3r+2] * d2) + T[r]          (TransPoint; R, T absent: identity, 0)
    y    = model[nn[i]], the chosen model point
the 16 terms are p[0..3), y[0..3), the nine products p[r] * y[c] at 6 + 3r + c, each rounded on its own, and the SSE
term (e0*e0 + e1*e1) + e2*e2 with e = p - y.  Nothing is contracted: the library is built with -ffp-contract=off.

Path and partition (icp_run).  vcp_blocks(x, tb, cap) = clamp(ceil(x / tb), 1, cap); the cap is ICP_MAX_BLOCKS = 1024.
    path    when                                         small (tb = 64) when     work (slots that carry a point)
    pairs   nm <= 512                                    nd <= 65536              half = (nd + 1) >> 1
    tiled   nm > 512, a non-finite model coordinate      nd <= 65536              nd
    grid    nm > 512, finite model                       8 nd <= 65536            8 nd   (nng::NNG = 8 lanes per point)
tb = 256 when the path is not small; nb = vcp_blocks(work, tb, 1024) workgroups; trips = ceil(work / (nb tb)).  The
partition is a function of (nm, nd, model finite) alone, never of the device.

Thread sums start from +0.0.  Slot v = blk * tb + t + trip * nb * tb, trips ascending:
    pairs   per trip the slot adds the terms of point v, then of point v + half, each only if it exists;
    tiled   the slot adds point v;
    grid    the slot belongs to point v / 8 and only the lane with v % 8 == 0 adds it; the other seven stay +0.0.

Fold.  In the workgroup __shfl_down at offsets 32, 16, 8, 4, 2, 1 (lane 0 ends with 6 pairwise levels over its 64
lanes), then the tb / 64 wave results in wave order: partial[blk].  In k_icp_step thread t of 256 adds rows t, t + 256,
... from +0.0, then the same 256-thread fold.

A thread's sum starts at +0.0 and (+0.0) + (-0.0) = +0.0, so no sum is ever -0.0 and adding the +0.0 of an idle slot
changes nothing (NaN stays NaN, payloads aside): the replay adds +0.0 rows for idle slots.  Every numpy operation below
is one binary64 ufunc call; numpy contracts nothing.

The bound (bound()).  Write u = 2^-53 and gamma_k = k u / (1 - k u).  A term reaches the result through at most
    d = A + (6 + tb/64 - 1) + (ceil(nb / 256) + 6 + 3)
rounded additions: A = trips thread adds (2 trips on the pairs path: two points per trip), 6 lane levels and tb/64 - 1
wave adds in its workgroup, then in the step ceil(nb / 256) row adds, 6 lane levels and 3 wave adds.  (The first add of
every chain is 0.0 + x, which is exact; it is counted all the same: d is an upper bound, not a count to tune.)  By the
standard argument (Higham, Accuracy and Stability of Numerical Algorithms, 4.2: any order of additions in which each
term passes through at most d of them) the computed sum of computed terms t^_i is sum t^_i (1 + theta_i), |theta_i| <=
gamma_d.  p and y are the binary64 numbers the exact sums are taken over, so for the six plain sums t^ = t.  A product
is rounded once more, t^ = p y (1 + delta): d + 1.  In the SSE term each exact square passes through its own rounding
and the two adds of the expression: d + 3.  Hence, with k = 0, 1, 3 extra roundings,
    |sum^ - sum t_i| <= gamma_(d+k) * sum|t_i| <= gamma_(d+k) * (1 + gamma_k) * sum|t^_i|
(|t| <= |t^| / (1 - u)^k <= |t^| (1 + gamma_k)), which bound() evaluates in rational arithmetic on the rounded terms.  A sequential
sum in point order has d = nd - 1.  The bound presumes no overflow and no underflow.
"""
import math
from fractions import Fraction

import numpy as np

from centroid_ref import U   # unit roundoff of binary64 as a Fraction

MAX_BLOCKS = 1024   # ICP_MAX_BLOCKS (icp.hip)
NNG = 8             # nng::NNG (nngrid.hpp)
NM_SCALAR = 512     # models up to this size take the pairs path
STEP_TB = 256       # ITPB: k_icp_step's workgroup
FMA_MAX_POINTS = 20_000   # the contraction mutants run exact rational arithmetic per point

# the kernels' order; every other setting of a knob breaks exactly one property of it
KERNEL = dict(tb=None, cap=MAX_BLOCKS, interleaved=False, tail=None, ungrouped=False, step_tree=True,
              wave_reversed=False, fma=False)
KNOBS = {
    "tb_other": dict(tb="other"),              # 256 threads where the kernel takes 64 and the reverse
    "cap_2048": dict(cap=2048),
    "pairs_interleaved": dict(interleaved=True),   # a slot works points 2v, 2v + 1 instead of v, v + half
    "tail_dropped": dict(tail="dropped"),      # the last slot never adds its v + half point (even nd: point nd-1 is lost)
    "tail_counted": dict(tail="counted"),      # odd nd: the last slot's idle half adds the point it recomputed (nd-1, twice)
    "grid_ungrouped": dict(ungrouped=True),    # grid launch, but slot v adds point v (path treated as tiled)
    "step_sequential": dict(step_tree=False),  # the step adds the partial rows one after the other
    "wave_reversed": dict(wave_reversed=True),
    "fma_products": dict(fma=True),            # s = fma(p[r], y[c], s): one rounding per accumulate
    "sse_contracted": dict(),                  # a knob of terms(): fma(e2, e2, fma(e1, e1, e0 * e0))
}


def vcp_blocks(x, tb, cap):
    return max(1, min(cap, -(-x // tb)))


def plan(nm, nd, model_finite=True):
    """The launch icp_run makes for (nm, nd, model finite): path, tb, nb, trips, and work = slots that carry a point."""
    grid = nm > NM_SCALAR and bool(model_finite)
    tiled = nm > NM_SCALAR and not grid
    path = "grid" if grid else "tiled" if tiled else "pairs"
    work = nd * NNG if grid else nd if tiled else (nd + 1) >> 1
    small = (nd * NNG if grid else nd) <= 64 * MAX_BLOCKS
    tb = 64 if small else 256
    nb = vcp_blocks(work, tb, MAX_BLOCKS)
    return dict(path=path, tb=tb, nb=nb, trips=-(-work // (nb * tb)), work=work)


def _fma(a, b, c):
    """fma(a, b, c) of finite binary64 numbers, correctly rounded (Fraction -> float rounds to nearest even)."""
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def transform(data, R=None, T=None):
    """TransPoint as the pass does it; R, T absent: the identity state (1 * x + 0 * y + 0 * z + 0, still evaluated)."""
    data = np.ascontiguousarray(data, np.float64).reshape(-1, 3)
    R = np.eye(3) if R is None else np.asarray(R, np.float64).reshape(3, 3)
    T = np.zeros(3) if T is None else np.asarray(T, np.float64).reshape(3)
    p = np.empty_like(data)
    with np.errstate(all="ignore"):
        for r in range(3):
            acc = 0.0 + R[r, 0] * data[:, 0]
            acc = acc + R[r, 1] * data[:, 1]
            acc = acc + R[r, 2] * data[:, 2]
            p[:, r] = acc + T[r]
    return p


def terms(model, data, R, T, nn, sse_contracted=False):
    """[nd, 16]: the terms every data point adds (columns 0:3 are p, 3:6 are y).  sse_contracted (a mutant, at most
    FMA_MAX_POINTS points): the SSE expression as a contracting compiler would emit it."""
    model = np.ascontiguousarray(model, np.float64).reshape(-1, 3)
    p = transform(data, R, T)
    y = model[np.asarray(nn, np.int64)]
    t = np.empty((len(p), 16))
    with np.errstate(all="ignore"):
        t[:, 0:3] = p
        t[:, 3:6] = y
        for r in range(3):
            for c in range(3):
                t[:, 6 + 3 * r + c] = p[:, r] * y[:, c]
        e = p - y
        t[:, 15] = (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]
        if sse_contracted:
            assert len(p) <= FMA_MAX_POINTS and np.isfinite(e).all()
            for i in range(len(p)):
                e0, e1, e2 = (float(v) for v in e[i])
                t[i, 15] = _fma(e2, e2, _fma(e1, e1, e0 * e0))
    return t


def _wg_fold(acc, cfg):
    """acc [nb, tb, 16] thread sums -> [nb, 16]: block_fold<TB> of reduce.hpp with FoldSum."""
    nb, tb, _ = acc.shape
    w = acc.reshape(nb, tb // 64, 64, 16)
    d = 32
    while d:                       # lane i takes lane i + d; only lanes < d feed lane 0
        w = w[:, :, :d] + w[:, :, d:2 * d]
        d >>= 1
    w = w[:, :, 0]
    order = list(range(tb // 64))
    if cfg["wave_reversed"]:
        order.reverse()
    r = w[:, order[0]]
    for j in order[1:]:
        r = r + w[:, j]
    return r


def _adds(nd, pl, tb, nb, cfg):
    """The point index every slot adds, per thread add in order: a list of [nb * tb] int64 arrays, nd = nothing."""
    stride = nb * tb
    path = "tiled" if cfg["ungrouped"] and pl["path"] == "grid" else pl["path"]
    if path == "pairs":
        half = (nd + 1) >> 1
        out = []
        for trip in range(-(-half // stride)):
            v = np.arange(trip * stride, (trip + 1) * stride, dtype=np.int64)
            a, b = (2 * v, 2 * v + 1) if cfg["interleaved"] else (v, v + half)
            a = np.where((v < half) & (a < nd), a, nd)
            b = np.where((v < half) & (b < nd), b, nd)
            if cfg["tail"] == "dropped":
                b[v == half - 1] = nd
            if cfg["tail"] == "counted":
                b[(v == half - 1) & (b == nd)] = nd - 1   # idle slots recompute the last point
            out += [a, b]
        return out
    lpq = NNG if path == "grid" else 1
    out = []
    for trip in range(-(-(nd * lpq) // stride)):
        v = np.arange(trip * stride, (trip + 1) * stride, dtype=np.int64)
        out.append(np.where((v % lpq == 0) & (v // lpq < nd), v // lpq, nd))
    return out


def replay(t, nd, pl, **knobs):
    """The 16 sums of terms t [nd, 16] under plan pl, in the kernels' order (KERNEL) or with knobs of KNOBS set."""
    cfg = dict(KERNEL)
    for k in knobs:
        if k not in KERNEL:
            raise TypeError("unknown replay knob %r" % k)
    cfg.update(knobs)
    assert t.shape == (nd, 16)
    tb = pl["tb"] if cfg["tb"] is None else 320 - pl["tb"] if cfg["tb"] == "other" else cfg["tb"]
    nb = vcp_blocks(pl["work"], tb, cfg["cap"])
    tz = np.concatenate([t, np.zeros((1, 16))])     # row nd: what an idle slot adds
    s = np.zeros((nb * tb, 16))
    assert not cfg["fma"] or (nd <= FMA_MAX_POINTS and np.isfinite(t).all())
    with np.errstate(all="ignore"):
        for ix in _adds(nd, pl, tb, nb, cfg):
            nxt = s + tz[ix]
            if cfg["fma"]:
                # fma(p, y, +0.0) is the rounded product: only accumulates onto a non-zero sum can differ
                for v in np.flatnonzero((ix < nd) & (s[:, 6:15] != 0.0).any(axis=1)):
                    for r in range(3):
                        for c in range(3):
                            k = 6 + 3 * r + c
                            nxt[v, k] = _fma(float(t[ix[v], r]), float(t[ix[v], 3 + c]), float(s[v, k]))
            s = nxt
        part = _wg_fold(s.reshape(nb, tb, 16), cfg)                  # partial[blk]
        if not cfg["step_tree"]:
            r = np.zeros(16)
            for b in range(nb):
                r = r + part[b]
            return r
        rows = -(-nb // STEP_TB)
        pad = np.zeros((rows * STEP_TB, 16))
        pad[:nb] = part
        pad = pad.reshape(rows, STEP_TB, 16)
        s = np.zeros((STEP_TB, 16))
        for k in range(rows):                                        # thread t: rows t, t + 256, ...
            s = s + pad[k]
        return _wg_fold(s.reshape(1, STEP_TB, 16), cfg)[0]


def sums(model, data, R, T, nn, knob=None):
    """What vcp_icp_sums must return for these inputs (knob: the sums of that mutant of KNOBS instead)."""
    model = np.ascontiguousarray(model, np.float64).reshape(-1, 3)
    data = np.ascontiguousarray(data, np.float64).reshape(-1, 3)
    pl = plan(len(model), len(data), np.isfinite(model).all())
    t = terms(model, data, R, T, nn, sse_contracted=knob == "sse_contracted")
    return replay(t, len(data), pl, **(KNOBS[knob] if knob else {}))


def sequential(t):
    """The plain sum in point order from +0.0 (what the C# and the oracle do with the same terms)."""
    s = np.zeros(16)
    with np.errstate(all="ignore"):
        for row in t:
            s = s + row
    return s


def in_play(knob, pl, nd):
    """Whether the property a knob breaks can change the tree at this shape at all (derived from the order above, not
    from results): where it is False the mutant IS the true replay, where it is True their trees differ."""
    path, tb, nb, work = pl["path"], pl["tb"], pl["nb"], pl["work"]
    if knob == "tb_other":          # up to two waves of slots both sizes compute w0 + w1; a third meets (w0 + w1) + w2
        return work > 128           # in one workgroup of 256 but (w0 + w2) + w1 in the step's lanes over 64-thread rows
    if knob == "cap_2048":
        return work > MAX_BLOCKS * tb
    if knob == "pairs_interleaved":
        return path == "pairs" and nd >= 3
    if knob == "tail_dropped":
        return path == "pairs" and nd % 2 == 0
    if knob == "tail_counted":
        return path == "pairs" and nd % 2 == 1
    if knob == "grid_ungrouped":
        return path == "grid" and nd >= 3
    if knob == "step_sequential":   # lanes fold rows as (r0 + r2) + r1
        return nb >= 3
    if knob == "wave_reversed":     # three live waves: in a 256-thread workgroup, or in the step beyond 128 rows
        return (tb == 256 and work > 128) or nb > 128
    if knob == "fma_products":      # an accumulate onto a non-zero sum: the pairs path's second point (the other paths
        return nd <= FMA_MAX_POINTS and path == "pairs" and nd >= 2   # add one point per trip: one trip up to this size)
    if knob == "sse_contracted":
        return nd <= FMA_MAX_POINTS
    raise KeyError(knob)


def shows(knob, pl, nd):
    """Where tests/test_icp_sums_tree.py DEMANDS that a mutant changes bits on every family whose sums round: where it
    is in play, less the shapes at which it moves too little for a demand (there it may or may not show):
      * the contraction mutants re-round single operations by half an ulp of a TERM; in a sum of thousands of squares
        that drowns (about a fifth of the SSE terms change, the sum of 20 000 of them did not in any family).  They are
        demanded of probes() instead: calls of one and two points, where the sum is the term;
      * fewer than 8 points: reordering so few terms often rounds to the same 16 sums;
      * the block cap with less than one wave in the second trip: 524 289, 262 145 and 32 769 points put ONE slot
        there, and with 2048 workgroups that one term merely folds in elsewhere."""
    if knob in ("fma_products", "sse_contracted"):
        return False
    if knob == "cap_2048":
        return pl["work"] - MAX_BLOCKS * pl["tb"] >= 64
    if knob in ("tail_dropped", "tail_counted"):   # a point lost or doubled is no matter of rounding
        return in_play(knob, pl, nd)
    return in_play(knob, pl, nd) and nd >= 8


# ---- exact arithmetic ----------------------------------------------------------------------------------------------
_SPLIT = 134217729.0   # 2^27 + 1 (Veltkamp)


def _two_prod(a, b):
    """a * b = x + e exactly (Dekker), elementwise, for finite a, b whose product neither overflows nor underflows."""
    x = a * b
    ca, cb = _SPLIT * a, _SPLIT * b
    ah, bh = ca - (ca - a), cb - (cb - b)
    al, bl = a - ah, b - bh
    e = ((ah * bh - x) + ah * bl + al * bh) + al * bl
    return x, e


def _exact_sum(x):
    """sum(x) of finite binary64 x as a Fraction, no rounding anywhere: the 53-bit mantissas are split in halves and
    added per exponent (np.bincount adds in binary64: below 2^53, here below 2^27 * len(x), that is exact), the
    exponents are combined in Python integers.  (centroid_ref._exact_int_sum does the same by sorting; this one is
    linear, for columns of 600 000.)"""
    x = np.asarray(x, np.float64)
    if len(x) == 0:
        return Fraction(0)
    assert len(x) < 2 ** 26
    m, e = np.frexp(x)
    mi = (m * 2.0 ** 53).astype(np.int64)   # |m| < 1: m * 2^53 is an integer below 2^53
    hi = mi >> 26
    lo = mi - (hi << 26)                    # 0 <= lo < 2^26
    e0 = int(e.min())
    b = (e - e0).astype(np.int64)
    H, L = np.bincount(b, hi.astype(np.float64)), np.bincount(b, lo.astype(np.float64))
    tot = sum(((int(h) << 26) + int(l)) << k for k, (h, l) in enumerate(zip(H, L)) if h or l)
    return Fraction(tot) * Fraction(2) ** (e0 - 53)


def _exact_dot(a, b):
    x, e = _two_prod(a, b)
    return _exact_sum(x) + _exact_sum(e)


def _exact_columns(t):
    """The 16 exact sums over the binary64 p = t[:, 0:3], y = t[:, 3:6] and e = fl(p - y)."""
    p, y = t[:, 0:3], t[:, 3:6]
    assert np.isfinite(t).all()
    out = [_exact_sum(t[:, k]) for k in range(6)]
    for r in range(3):
        for c in range(3):
            out.append(_exact_dot(p[:, r], y[:, c]))
    e = p - y
    out.append(sum(_exact_dot(e[:, a], e[:, a]) for a in range(3)))
    return out


def exact(model, data, R, T, nn):
    """16 Fractions: the sums of p, y, the exact products p[r] y[c] and the exact e0^2 + e1^2 + e2^2, no rounding."""
    return _exact_columns(terms(model, data, R, T, nn))


def gamma(d):
    return d * U / (1 - d * U)


EXTRA = [0] * 6 + [1] * 9 + [3]   # roundings of a term before it is added: none, the product's, a square's and two adds


def depth(pl):
    """Additions a term passes through at most (see the module docstring)."""
    thread = pl["trips"] * (2 if pl["path"] == "pairs" else 1)
    return thread + 6 + (pl["tb"] // 64 - 1) + -(-pl["nb"] // STEP_TB) + 6 + 3


def abs_sums(t):
    """16 Fractions >= sum|t^| per column of the rounded terms: the binary64 sum of non-negative numbers, in whatever
    order, is at least (1 - n u) times the exact one, so for n <= 2^22 rows the exact sum is at most (1 + 2^-30)
    times the computed one.  (A 1e-9 of slack on a bound, for a tenth of the time of the exact sums.)"""
    assert len(t) <= 2 ** 22
    return [Fraction(float(v)) * (1 + Fraction(1, 2 ** 30)) for v in np.abs(t).sum(axis=0)]


def bound(pl, t, sequential=False, sabs=None):
    """16 Fractions b with |sum - exact sum| <= b for the tree of plan pl (default) or a sequential sum of the rows of
    t: gamma_(d + k) (1 + gamma_k) sum|t^|, d = depth(pl) or len(t) - 1, k = EXTRA.  sabs: abs_sums(t), if at hand."""
    d = max(len(t) - 1, 0) if sequential else depth(pl)
    sabs = abs_sums(t) if sabs is None else sabs
    return [gamma(d + EXTRA[k]) * (1 + gamma(EXTRA[k])) * sabs[k] for k in range(16)]


# ---- the shared input set ------------------------------------------------------------------------------------------
# (path, nm, nd): the smallest shapes at which each partition property can go wrong
SHAPES = (
    [("pairs", 100, nd) for nd in (1, 2, 3, 127, 128, 129, 65535, 65536)]          # tb 64
    + [("pairs", 100, nd) for nd in (65537, 524288, 524289, 600001)]               # tb 256: nb 129, 1024; second trip
    + [("tiled", 600, nd) for nd in (1, 65, 65536, 65537, 262145, 300001)]
    + [("grid", 600, nd) for nd in (1, 9, 8192, 8193, 32769, 40001)]
)
# the further conditions are taken at these: model sizes at and next to the path switch, and a few hundred to a few
# thousand points per path (the contraction mutants need at most FMA_MAX_POINTS)
SMALL_SHAPES = [("pairs", nm, 1000) for nm in (1, 2, 512)] + [("grid", 513, 1000), ("pairs", 100, 129),
                                                               ("pairs", 100, 20000), ("tiled", 600, 1000),
                                                               ("grid", 600, 1000)]
FAMILIES = ("generic", "offset", "scaled", "planar", "cancel", "lattice")
INEXACT = ("generic", "offset", "scaled", "planar", "cancel")   # families whose sums round
POSES = ("none", "generic")


def rotation(axis, angle):
    a = np.asarray(axis, np.float64)
    a = a / np.sqrt((a * a).sum())
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + math.sin(angle) * K + (1 - math.cos(angle)) * (K @ K)


def case(path, nm, nd, family="generic", pose="generic", seed=7):
    """(model [nm,3], data [nd,3], R, T) of one shape, value family and pose; seeded and deterministic.
      generic  uniform in +-10
      offset   1e5 plus the same (the sums round hard; the binary32 screening is ambiguous for most points)
      scaled   generic times 2^40
      planar   z = 0 in model and data, rotation about z (products with a signed zero)
      cancel   the data come in pairs x, -x (plus a spread of 1e-3) in shuffled order: sum p is ~1, sum|p| ~ 5 nd
      lattice  multiples of 2^-10 in +-10; the pose is a quarter turn about z and a lattice shift: every partial sum is
               exact
    pose "none": R = T = None (the identity state).  path "tiled": model[nm // 2, 1] = inf."""
    assert plan(nm, nd, path != "tiled")["path"] == path
    rng = np.random.default_rng([seed, nm, nd, FAMILIES.index(family)])
    model = rng.uniform(-10, 10, (nm, 3))
    data = rng.uniform(-10, 10, (nd, 3))
    R, T = rotation((1.0, 2.0, 3.0), 0.3), np.array([0.1, 0.2, -0.3])
    if family == "offset":
        model, data = model + 1e5, data + 1e5
    elif family == "scaled":
        model, data, T = model * 2.0 ** 40, data * 2.0 ** 40, T * 2.0 ** 40
    elif family == "planar":
        model[:, 2] = 0.0
        data[:, 2] = 0.0
        R, T = rotation((0.0, 0.0, 1.0), 0.3), np.array([0.1, 0.2, 0.0])
    elif family == "cancel":
        h = (nd + 1) // 2
        data = np.concatenate([data[:h], -data[:h]])[:nd] + rng.uniform(-1e-3, 1e-3, (nd, 3))
        data = data[rng.permutation(nd)]
        model[1::2] = -model[:-1:2][:len(model[1::2])]
    elif family == "lattice":
        model, data = np.round(model * 1024) / 1024, np.round(data * 1024) / 1024
        R, T = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]]), np.array([0.125, -2.5, 3.0 / 1024])
    if path == "tiled":
        model[nm // 2, 1] = np.inf
    if pose == "none":
        R, T = None, None
    return np.ascontiguousarray(model), np.ascontiguousarray(data), R, T


N_PROBES = 32


def probes(family):
    """Calls in which the sum is the term: N_PROBES of two points on the pairs path (one thread: the rounded product of
    the first, then ONE accumulate of the second onto it; two SSE terms) and of one point on the tiled and the grid
    path.  A fifth of all SSE terms and about as many accumulates change under contraction, so 32 probes miss a
    contracting build with probability 0.8^32 < 0.1 %; the set is fixed, and test_icp_sums_tree.py asserts that it
    does not."""
    out = []
    for path, nm, nd in (("pairs", 100, 2), ("tiled", 600, 1), ("grid", 600, 1)):
        out += [case(path, nm, nd, family, "generic", seed=100 + k) for k in range(N_PROBES)]
    return out
