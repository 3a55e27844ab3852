"""Seeded cluster families for the exact shape tests (test_circle_exact.py, test_circle_exact_gpu.py): the smallest
inputs at which the per-cluster shape pass (csrc/hull.hpp) can go wrong.  Every generator returns
dict(xy, labels, order, K, kinds): kinds[k] names what cluster k + 1 is.  About 390 clusters and 15 500 points in all."""
import math

import numpy as np

import circle_ref as CR
import shapes_ref as S

# kinds on which the wrap's hull need not be the exact hull: the circle and the rectangle are
# held to containment there instead
HULL_EXEMPT = ("near", "near_doubled", "near_verbatim", "sliver13")

# the 7-point cluster on which the reference's gift wrap closes after 5 points (hexadecimal doubles)
VERBATIM7 = [
    ("0x1.48fe7fe334453p-1", "-0x1.d245fe9a7f0bep+0"),
    ("0x1.2d4b15b83ff7ap-1", "-0x1.ab038c29f6829p+0"),
    ("0x1.189f308375519p-2", "-0x1.8db7813635570p-1"),
    ("0x1.817d871362d36p-1", "-0x1.112c00b8f042bp+1"),
    ("0x1.783e218afc6dep-3", "-0x1.0a9e621367b64p-1"),
    ("0x1.7e255990bfd67p-2", "-0x1.0ecd49118b05ep+0"),
    ("0x1.9bc86e2df1eebp-4", "-0x1.23cdc147702bfp-2"),
]


def verbatim7():
    return np.array([[float.fromhex(x), float.fromhex(y)] for x, y in VERBATIM7])


class _Cloud:
    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.pts, self.lab, self.kinds = [], [], []

    def add(self, g, kind, shuffle=True):
        g = np.asarray(g, np.float64).reshape(-1, 2)
        if shuffle:
            g = g[self.rng.permutation(len(g))]
        self.kinds.append(kind)
        self.pts.append(g), self.lab.append(np.full(len(g), len(self.kinds)))

    def done(self, by_order):
        """by_order: the points stay where they are and `order` is a shuffled list; otherwise the array itself is
        shuffled and order is None.  20 noise points (label 0) go along."""
        K = len(self.kinds)
        noise = self.rng.uniform(-50, 50, (20, 2))
        xy = np.concatenate(self.pts + [noise])
        lab = np.concatenate(self.lab + [np.zeros(20)]).astype(np.int32)
        p = self.rng.permutation(len(lab))
        if by_order:
            return dict(xy=np.ascontiguousarray(xy), labels=lab, order=p.astype(np.int64), K=K, kinds=self.kinds)
        return dict(xy=np.ascontiguousarray(xy[p]), labels=lab[p], order=None, K=K, kinds=self.kinds)


def sizes():
    """Member counts at the decision and stride edges of the 256-thread workgroup; hulls of one and two points."""
    c = _Cloud(101)
    c.add([[0, 0], [1, 0], [0, 1]], "three")
    c.add([[0, 0], [2, 0], [2, 1], [0.5, 3]], "four")
    c.add([[0, 0], [4, 0], [1, 0], [3, 0]], "four_on_a_line")
    for cnt in (255, 256, 257, 513):
        c.add(c.rng.integers(0, 8, (cnt, 2)).astype(float) + [cnt, -3.0], "n%d" % cnt)
    for cnt in (4, 5, 300):
        c.add(np.tile([[2.5, -1.0]], (cnt, 1)), "one_point")
    for cnt in (6, 257, 514):
        c.add(np.tile([[1.0, 2.0], [-3.5, 0.25]], (cnt // 2, 1)), "two_points")
    return c.done(True)


def long_hull():
    """Every member a hull vertex, more of them than one and than two passes of the lanes."""
    c = _Cloud(103)
    for cnt, r, cx, cy in ((300, 2.5, 100.25, -7.0), (515, 1.0, 0.0, 0.0)):
        th = np.arange(cnt) * (2 * math.pi / cnt)
        c.add(np.c_[cx + r * np.cos(th), cy + r * np.sin(th)], "on_circle")
    return c.done(False)


def lattice_circle(N):
    r = int(math.isqrt(N))
    return np.array([(x, y) for x in range(-r, r + 1) for y in range(-r, r + 1) if x * x + y * y == N], float)


def ties():
    """Exact ties in radius: integer rectangles and squares (both diagonals give the same circle), and the integer
    points of x^2 + y^2 = N with interior points and duplicates."""
    c = _Cloud(107)
    for w, h, x0, y0 in ((3, 1, 0, 0), (5, 5, 10, -3), (1, 7, -20, 4), (2, 2, 7, 50), (9, 4, -64, -64), (8, 8, 1000, 1)):
        g = np.array([(x0 + i, y0 + j) for i in range(w + 1) for j in range(h + 1)], float)
        c.add(np.r_[g, g[c.rng.integers(0, len(g), 6)]], "box")
    for w, h in ((4, 3), (6, 6)):  # the four corners alone, each twice
        g = np.array([(0, 0), (w, 0), (w, h), (0, h)], float) + [31.0, 17.0]
        c.add(np.r_[g, g], "corners")
    for N in (25, 50, 65, 325, 1105):
        g = lattice_circle(N)
        r = math.isqrt(N)
        inner = c.rng.integers(-r // 2, r // 2 + 1, (10, 2)).astype(float)
        full = np.r_[g, inner, g[c.rng.integers(0, len(g), 5)]]
        c.add(full, "cocircular")
        c.add(full + [1000.5, 7.0], "cocircular_moved")
        c.add(full * 0.1, "cocircular_scaled")
    return c.done(True)


def polygons():
    """Regular n-gons, n = 5 .. 64, around the origin and far from it (offsets 10^0 .. 10^6); the centre is a member."""
    c = _Cloud(109)

    def gon(n, cx, cy, r, ph):
        th = ph + np.arange(n) * (2 * math.pi / n)
        return np.r_[np.c_[cx + r * np.cos(th), cy + r * np.sin(th)], [[cx, cy]]]

    for n in range(5, 65):
        c.add(gon(n, 0.0, 0.0, 1.0, 0.1 * n), "gon")
    for e in range(7):
        for n in (5, 6, 7, 8, 12, 17, 31, 64):
            c.add(gon(n, 10.0 ** e, -0.375 * 10.0 ** e, 1.0 + 0.25 * (n % 3), 0.3), "gon_far")
    return c.done(False)


def near_collinear():
    """Clusters collinear up to rounding: off + s * d in binary64, offsets 0 and 10^0 .. 10^5; the same with every point
    twice; exactly collinear dyadic ones as a control; the 7-point cluster of DESIGN.md section 12, in its order."""
    c = _Cloud(113)

    def line(off):
        cnt = int(c.rng.integers(5, 41))
        a = c.rng.uniform(0, 2 * math.pi)
        d = np.array([math.cos(a), math.sin(a)]) * c.rng.uniform(0.5, 3.0)
        o = off * c.rng.uniform(0.5, 1.0, 2) * c.rng.choice([-1.0, 1.0], 2)
        return o + c.rng.uniform(-1, 1, (cnt, 1)) * d

    for off in [0.0] + [10.0 ** e for e in range(6)]:
        for _ in range(12):
            c.add(line(off), "near", shuffle=False)
        for _ in range(4):
            g = line(off)
            c.add(np.repeat(g, 2, axis=0), "near_doubled")
    for a, b, cnt in ((0.125, 0.375, 7), (1.0, 2.0, 6), (-0.5, 0.0, 9), (0.0, 0.25, 5), (3.0, -1.0, 12), (2.0 ** -10, 2.0 ** -9, 33)):
        c.add([(30 + i * a, -7 + i * b) for i in range(cnt)], "dyadic_line")
    c.add(verbatim7(), "near_verbatim", shuffle=False)
    return c.done(True)


def slivers():
    """Unit segments at random angles with a transverse sigma of 1e-9 and of 1e-13."""
    c = _Cloud(127)
    for sigma, kind in ((1e-9, "sliver9"), (1e-13, "sliver13")):
        for _ in range(16):
            cnt = int(c.rng.integers(8, 60))
            a = c.rng.uniform(0, math.pi)
            along = c.rng.uniform(-0.5, 0.5, (cnt, 1)) * [math.cos(a), math.sin(a)]
            across = c.rng.normal(0, sigma, (cnt, 1)) * [-math.sin(a), math.cos(a)]
            c.add(c.rng.uniform(-5, 5, 2) + along + across, kind)
    return c.done(False)


def blobs():
    """Gaussian clusters and clusters on the 2^-10 lattice, at offsets up to 10^6."""
    c = _Cloud(131)
    for off in (0.0, 1.0, 1e2, 1e4, 1e6):
        for i in range(12):
            cnt = int(c.rng.integers(8, 120))
            o = off * c.rng.uniform(0.5, 1.0, 2) * c.rng.choice([-1.0, 1.0], 2)
            th = c.rng.uniform(0, math.pi)
            R = np.array([[math.cos(th), -math.sin(th)], [math.sin(th), math.cos(th)]])
            if i % 2 == 0:
                c.add(c.rng.normal(0, 1, (cnt, 2)) * c.rng.uniform(0.2, 5.0, 2) @ R.T + o, "gauss")
            else:
                c.add(np.round((c.rng.normal(0, 0.05, (cnt, 2)) @ R.T + o) * 1024) / 1024, "fine")
    return c.done(False)


def nonfinite():
    """Members that are not finite: for parity with the oracle only."""
    c = _Cloud(137)
    nan, inf = math.nan, math.inf
    base = lambda: c.rng.normal(0, 1, (12, 2))
    c.add(np.r_[base(), [[nan, 0.5]]], "nan_x")          # HullCull keeps a point with one NaN coordinate
    c.add(np.r_[base(), [[0.25, nan]]], "nan_y")
    c.add(np.r_[base(), [[nan, nan], [nan, nan]]], "nan_both")
    c.add(np.r_[[[nan, nan]], base()], "nan_both_first", shuffle=False)
    c.add(np.r_[base(), [[inf, 0.0]]], "inf_x")
    c.add(np.r_[base(), [[1.0, -inf]]], "minus_inf_y")
    c.add(np.r_[base(), [[inf, inf]]], "inf_both")
    c.add(base(), "finite")
    return c.done(True)


FINITE = dict(sizes=sizes, long_hull=long_hull, ties=ties, polygons=polygons, near_collinear=near_collinear,
              slivers=slivers, blobs=blobs)
ALL = dict(FINITE, nonfinite=nonfinite)
# families on which the insertion rule of DESIGN.md section 12 must never fire, and the one on which it must
NEVER_FIRES = ("long_hull", "ties", "polygons", "blobs")
MUST_FIRE = ("near_collinear",)

# The worst figures of the oracle against exact geometry per family, in units (unit() below), as test_circle_exact.py
# measures and prints them; DESIGN.md section 12 has the table.  The tests assert twice these.
BOUNDS = dict(
    sizes=dict(beyond=0.0, r=0.144, c=0.0, rect=0.0),
    long_hull=dict(beyond=0.431, r=0.302, c=0.141, rect=1.74),
    ties=dict(beyond=0.4, r=0.4, c=0.0, rect=0.51),
    polygons=dict(beyond=0.958, r=1.23, c=1.25, rect=2.42),
    near_collinear=dict(beyond=2.39, r=1.2, c=1.3, rect=1.35),
    slivers=dict(beyond=1.49, r=0.743, c=0.886, rect=0.615),
    blobs=dict(beyond=1.37, r=0.851, c=0.919, rect=0.834),
)

_cache = {}


def family(name):
    """The cloud of a family, built once; callers may add their own keys but leave xy, labels and order alone."""
    if name not in _cache:
        _cache[name] = ALL[name]()
    return _cache[name]


def unit(pts, r):
    """2^-53 (max |coordinate of the cluster| + r): the unit of the circle bounds (r = the exact radius) and of the
    rectangle bound (r = the longer side)."""
    return 2.0 ** -53 * (float(np.abs(pts).max()) + r)


def exact(c):
    """Per cluster of a finite family: None for a cluster of <= 3 members, else dict(idx, P, H, cx, cy, r2, r): the
    members in list order, their Fractions, the exact hull and the exact minimum enclosing circle.  Built once."""
    if "exact" not in c:
        out = []
        for idx in S.members(c["labels"], c["K"], c["order"]):
            if len(idx) <= 3:
                out.append(None)
                continue
            P = CR.fractions_of(c["xy"][idx])
            H = CR.convex_hull(P)
            cx, cy, r2 = CR.min_circle(H)
            out.append(dict(idx=idx, P=P, H=H, cx=cx, cy=cy, r2=r2, r=CR._sqrt(r2)))
        c["exact"] = out
    return c["exact"]


def figures(c, res):
    """The worst figures of a result (centers, radius, valid and, when present, rect_xy, rect_len, rect_valid) on a
    finite family against exact geometry, in units: dict(beyond, r, c, rect, checked).  A convex function takes its
    maximum over a cluster at a vertex of the exact hull, so the members are represented by that hull."""
    w = dict(beyond=0.0, r=0.0, c=0.0, rect=0.0, checked=0, rect_checked=0)
    for k, e in enumerate(exact(c)):
        if res["valid"][k] != 1:
            assert e is None, (k, c["kinds"][k])
            continue
        pts = c["xy"][e["idx"]]
        u = unit(pts, e["r"])
        cx, cy, r = float(res["centers"][k][0]), float(res["centers"][k][1]), float(res["radius"][k])
        w["beyond"] = max(w["beyond"], CR.beyond(CR.max_dist2(e["H"], cx, cy), r) / u)
        w["r"] = max(w["r"], abs(CR.beyond(e["r2"], r)) / u)
        w["c"] = max(w["c"], CR.dist(cx, cy, e["cx"], e["cy"]) / u)
        w["checked"] += 1
        if "rect_xy" in res and res["rect_valid"][k] == 1:
            ur = unit(pts, float(np.max(res["rect_len"][k])))
            w["rect"] = max(w["rect"], CR.outside_rectangle(e["H"], res["rect_xy"][k]) / ur)
            w["rect_checked"] += 1
    return w


def hull_is_exact(c, k, hull_xy):
    """The hull's coordinates are the exact hull's vertex set plus, at most, members lying exactly on an exact hull
    edge."""
    e = exact(c)[k]
    mine = set(CR.fractions_of(hull_xy))
    return set(e["H"]) <= mine and all(CR.on_hull_edge(p, e["H"]) for p in mine - set(e["H"]))


def check_bounds(name, w):
    """Twice the recorded worst figure of the family (BOUNDS), for each of the four figures."""
    assert w["checked"] > 0, name
    for key in ("beyond", "r", "c", "rect"):
        assert w[key] <= 2 * BOUNDS[name][key], (name, key, w[key], BOUNDS[name][key])


def oracle_shapes(oracle, c):
    """What vcp_cluster_shapes has to return on the cloud c, from the oracle's circle and hull cluster by cluster (the
    two rules of DESIGN.md section 12 included) and the numpy restatement of the rectangle: the arrays of the entry
    point, plus inserted [K] and hull_xy (the wrap's hull per cluster, None where valid is 0).  Built once per cloud."""
    if "oracle" in c:
        return c["oracle"]
    K = c["K"]
    r = dict(centers=np.zeros((K, 2)), radius=np.zeros(K), valid=np.zeros(K, np.uint8), hull_n=np.zeros(K, np.int32),
             inserted=np.zeros(K, np.int32), rect_valid=np.zeros(K, np.uint8), rect_edge=np.full(K, -1, np.int32),
             rect_len=np.zeros((K, 2)), rect_xy=np.zeros((K, 4, 2)), hull_xy=[None] * K)
    for k, idx in enumerate(S.members(c["labels"], K, c["order"])):
        if len(idx) <= 3:  # Tools.cs:400
            continue
        pts = c["xy"][idx]
        one = oracle.min_circle_ex(pts)
        rect = S.rectangle(one["hull"], pts if one["inserted"] else None)
        r["centers"][k], r["radius"][k], r["valid"][k] = one["center"], one["radius"], 1
        r["hull_n"][k], r["inserted"][k], r["hull_xy"][k] = len(one["hull"]), one["inserted"], one["hull"]
        r["rect_valid"][k], r["rect_edge"][k], r["rect_len"][k], r["rect_xy"][k] = rect["valid"], rect["edge"], rect["len"], rect["xy"]
    c["oracle"] = r
    return r
