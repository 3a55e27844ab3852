"""Near-threshold clouds for the binary32 screens of vcp_dbscan / vcp_kdist and of the ICP nearest-neighbour pass.

Everything is built from a seed and checked against the binary64 expression the library must reproduce:

  d(a, b)   VCP_L1_2D |dx| + |dy|, VCP_L2_2D sqrt(dx*dx + dy*dy), VCP_L2_3D sqrt(dx*dx + dy*dy + dz*dz): numpy binary64,
            left to right, no FMA contraction (include/vcp.h, vcp_kdist)

Isolated pairs put a partner at distance eps from an unquantised anchor and then walk the partner's last coordinate by
ulps until d is exactly eps (AT, when reachable), the largest reachable value below eps (IN) or the smallest above it
(OUT).  Rings put hundreds of such points round one probe; dumbbells join two clumps by one such pair.  On these pairs
the binary32 copies the screen works on round by far more than the gap between d and eps, so a screen that decides
them on binary32 evidence alone is wrong on about half of them: power() counts how often, in each direction.

ICP ties put data points on the bisector plane of two model points, walked until the two binary64 squared distances
(the oracle's FindClosestPointSet expression) are equal or one or two ulps apart."""
import math

import numpy as np

L1_2D, L2_2D, L2_3D, SIGNED_SUM_2D = 0, 1, 2, 3
U = 2.0 ** -24            # binary32 unit roundoff
AT, IN, OUT = 0, 1, 2     # pair classes
METRICS = (L1_2D, L2_2D, L2_3D)


def gd_of(metric):
    return 3 if metric == L2_3D else 2


def dist(a, b, metric):
    """d(a, b) row by row (a, b: [..., >= gd])."""
    dx = a[..., 0] - b[..., 0]
    dy = a[..., 1] - b[..., 1]
    if metric == L1_2D:
        return np.abs(dx) + np.abs(dy)
    if metric == L2_2D:
        return np.sqrt(dx * dx + dy * dy)
    dz = a[..., 2] - b[..., 2]
    return np.sqrt(dx * dx + dy * dy + dz * dz)


def form(a, b, metric):
    """The quantity the library compares with thr(eps): d itself for L1, the sum of squares for L2."""
    dx = a[..., 0] - b[..., 0]
    dy = a[..., 1] - b[..., 1]
    if metric == L1_2D:
        return np.abs(dx) + np.abs(dy)
    if metric == L2_2D:
        return dx * dx + dy * dy
    dz = a[..., 2] - b[..., 2]
    return dx * dx + dy * dy + dz * dz


def l2_threshold(eps):
    """Largest binary64 s with sqrt(s) <= eps, so that sqrt(s) <= eps <=> s <= thr (dbscan.hip: l2_threshold)."""
    if math.isinf(eps):
        return eps
    t = eps * eps
    if math.isinf(t):
        t = np.finfo(np.float64).max
    while math.sqrt(t) > eps:
        t = math.nextafter(t, 0.0)
    while True:
        u = math.nextafter(t, math.inf)
        if math.isinf(u) or math.sqrt(u) > eps:
            return t
        t = u


def thr_of(eps, metric):
    return eps if metric == L1_2D else l2_threshold(eps)


def accept_side_on(metric, thr, E):
    """Whether the binary32 screen may accept a pair outright (Screen.lo >= 0) for threshold thr and extent E, both in
    the units of the screening copies -- the rule of screen_bounds, used here only to place frames on both sides of
    the point where it switches off."""
    u = 5.9604644775390625e-08
    alpha = 2.0 * u * E * (1.0 + 2.0 * u)
    gd = 3 if metric == L2_3D else 2
    if metric == L1_2D:
        err = 2.0 * alpha * (1.0 + u) + 2.0 * u * (1.0 + u) * thr
        ok = True
    else:
        err = 2.0 * alpha * math.sqrt(gd * thr) * (1.0 + u) + gd * alpha * alpha + 6.0 * u * (1.0 + u) * thr
        ok = math.sqrt(thr) > 4.0 * alpha * math.sqrt(gd)
    err = err * 1.0625 + 1e-14 * thr + 1e-300
    return ok and thr - err >= 0.0


def switch_ratio(metric, eps):
    """E / eps where accept_side_on turns false (bisection on E)."""
    thr = thr_of(eps, metric)
    lo, hi = 1.0, 1e9
    for _ in range(200):
        mid = math.sqrt(lo * hi)
        if accept_side_on(metric, thr, mid * eps):
            lo = mid
        else:
            hi = mid
    return hi


def grid_scale(E):
    """g.scale of run_dbscan: a power of two bringing an extent outside [1e-20, 1e30] to [1, 2)."""
    if E > 1e30 or (0.0 < E < 1e-20):
        return math.ldexp(1.0, -(math.frexp(E)[1] - 1))
    return 1.0


# ---- ordinal walks ----------------------------------------------------------------------------------------------
_MAG = np.int64(0x7FFFFFFFFFFFFFFF)
_SIGN = np.int64(-0x8000000000000000)


def to_ord(x):
    """Monotone int64 key of binary64 values: consecutive keys are consecutive doubles."""
    i = np.asarray(x, np.float64).view(np.int64)
    return np.where(i < 0, -(i & _MAG), i)


def from_ord(o):
    o = np.asarray(o, np.int64)
    return np.where(o < 0, (-o) | _SIGN, o).view(np.float64)


def _last_true(pred, lo, hi):
    """Per row the largest t in [lo, hi) with pred(t) true, for pred true at lo and false at hi (monotone)."""
    lo = lo.copy()
    hi = hi.copy()
    while True:
        act = hi - lo > 1
        if not act.any():
            return lo
        mid = lo + (hi - lo) // 2
        ok = pred(mid)
        lo = np.where(act & ok, mid, lo)
        hi = np.where(act & ~ok, mid, hi)


def walk_to_eps(a, b, metric, eps):
    """Walk b's last metric coordinate by ulps (away from a's) to the three reachable values round eps.  Returns
    (b_at, b_in, b_out, at_ok): b_at has d == eps where at_ok, b_in the largest d < eps, b_out the smallest d > eps."""
    gd = gd_of(metric)
    c = gd - 1
    a = np.asarray(a, np.float64)
    b = np.array(b, np.float64)
    s = np.where(b[:, c] >= a[:, c], 1, -1).astype(np.int64)
    o0 = to_ord(a[:, c])
    far = a[:, c] + s * 2.5 * eps
    T = np.abs(to_ord(far) - o0)

    def at(t):
        q = b.copy()
        q[:, c] = from_ord(o0 + s * t)
        return q

    zero = np.zeros(len(a), np.int64)
    t_le = _last_true(lambda t: dist(a, at(t), metric) <= eps, zero, T)
    t_lt = _last_true(lambda t: dist(a, at(t), metric) < eps, zero, T)
    b_at, b_in, b_out = at(t_le), at(t_lt), at(t_le + 1)
    return b_at, b_in, b_out, dist(a, b_at, metric) == eps


def trunc_bits(x, bits=20):
    """x with its significand cut to `bits` bits (eps values whose multiples the coordinates can hold exactly)."""
    m, e = math.frexp(x)
    return math.ldexp(math.floor(m * 2 ** bits) / 2 ** bits, e)


def unit_dirs(rng, n, metric, min_last=0.3):
    """Random unit vectors in the metric's norm with |last component| >= min_last."""
    gd = gd_of(metric)
    out = np.zeros((0, gd))
    while len(out) < n:
        if metric == L1_2D:
            w = rng.uniform(0, 1, 2 * n)
            v = np.stack([w, 1.0 - w], 1) * rng.choice([-1.0, 1.0], (2 * n, 2))
        else:
            v = rng.normal(size=(2 * n, gd))
            v /= np.sqrt((v * v).sum(1))[:, None]
        out = np.concatenate([out, v[np.abs(v[:, -1]) >= min_last]])
    return out[:n]


# ---- frames -----------------------------------------------------------------------------------------------------
def frames(metric):
    """(name, origin, E / eps, coordinate scale): cells of about eps (E / eps 1e3 in 2-D, 1e2 in 3-D, at two origins),
    a coarse grid (1e4), both sides of the screen's accept switch, and clouds x 1e-25 / x 1e35 (g.scale != 1)."""
    fine = 1e3 if gd_of(metric) == 2 else 1e2
    sw = switch_ratio(metric, 1.0)
    return [("fine_o0", 0.0, fine, 1.0), ("fine_o1e5", 1e5, fine, 1.0), ("coarse_om7e5", -7e5, 1e4, 1.0),
            ("below_switch", -7e5, sw * 0.97, 1.0), ("above_switch", 1e5, sw * 1.03, 1.0),
            ("tiny", 1e5, fine, 1e-25), ("huge", -7e5, 1e3, 1e35)]


class Frame:
    def __init__(self, metric, name, origin, ratio, scale, eps0=0.7318):
        self.metric, self.name, self.ratio = metric, name, ratio
        self.gd = gd_of(metric)
        self.eps = trunc_bits(eps0 * scale)
        self.origin = float(origin * scale)
        self.E = trunc_bits(ratio * self.eps, 30)
        self.thr = thr_of(self.eps, metric)

    def corners(self):
        lo = np.full((1, self.gd), self.origin)
        return np.concatenate([lo, lo + self.E])

    def sites(self, rng, count, spacing=6.0):
        """Jittered lattice points, at least `spacing` - 0.8 eps apart per axis and 3 eps inside the box."""
        inner = self.E - 6.0 * self.eps
        per = max(1, int(math.ceil(count ** (1.0 / self.gd))))
        step = inner / per
        while step < spacing * self.eps and per > 1:
            per -= 1
            step = inner / per
        grid = np.stack(np.meshgrid(*[np.arange(per)] * self.gd, indexing="ij"), -1).reshape(-1, self.gd)
        if len(grid) < count:
            raise ValueError("frame %s holds %d sites, %d wanted" % (self.name, len(grid), count))
        grid = grid[rng.permutation(len(grid))[:count]]
        jit = rng.uniform(-0.4, 0.4, (count, self.gd)) * self.eps
        return self.origin + 3.0 * self.eps + (grid + 0.5) * step + jit


def _pairs(fr, rng, anchors):
    u = unit_dirs(rng, len(anchors), fr.metric)
    b = anchors + fr.eps * u
    return walk_to_eps(anchors, b, fr.metric, fr.eps)


def screen_view(pts, metric):
    """(mn, scale, E) the screen works with: the bounding box minimum, g.scale and the scaled extent."""
    gd = gd_of(metric)
    fin = np.isfinite(pts[:, :gd]).all(1)
    mn = pts[fin, :gd].min(0)
    mx = pts[fin, :gd].max(0)
    E = float(max(np.abs(mx - mn).max(), 0.0))
    s = grid_scale(E)
    return mn, s, E * s


def value32(a, b, metric, mn, scale):
    """The screen's binary32 value of a pair: copies float32((x - mn) * scale), then value32 (dbscan.hip) in numpy
    float32 without FMA."""
    gd = gd_of(metric)
    fa = ((a[:, :gd] - mn) * scale).astype(np.float32)
    fb = ((b[:, :gd] - mn) * scale).astype(np.float32)
    d = fa - fb
    if metric == L1_2D:
        return np.abs(d[:, 0]) + np.abs(d[:, 1])
    s = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]
    if gd == 3:
        s = s + d[:, 2] * d[:, 2]
    return np.abs(s)


def pair_error(a, b, metric, mn, scale, E, eps):
    """|v32 - m| in units of u E (L1) or u E eps (L2), m the binary64 form, all in screen units."""
    k = scale if metric == L1_2D else scale * scale
    v = value32(a, b, metric, mn, scale).astype(np.float64)
    m = form(a, b, metric) * k
    unit = U * E if metric == L1_2D else U * E * eps * scale
    return np.abs(v - m) / unit


def power(a, b, metric, mn, scale, thr):
    """Pairs where the naive binary32 decision v32 <= float32(thr) disagrees with the binary64 one:
    (inside but rejected, outside but accepted)."""
    k = scale if metric == L1_2D else scale * scale
    v = value32(a, b, metric, mn, scale)
    naive = v <= np.float32(thr * k)
    exact = form(a, b, metric) <= thr
    return int((exact & ~naive).sum()), int((~exact & naive).sum())


def pairs_cloud(metric, frame, seed, n_pairs=2400, n_axis=300, min_points=0):
    """Isolated AT / IN / OUT pairs (the best-stressed of twice as many candidates), axis-aligned AT pairs whose left
    end sits near a multiple of the narrowest cell edge eps (1 + 2^-20) the grid may use, tight filler clumps up to
    min_points points (so that the grid keeps cells of about eps), and the box corners."""
    fr = Frame(metric, *frame)
    rng = np.random.default_rng(seed)
    n_cand = 2 * n_pairs
    cand_sites = fr.sites(rng, n_cand + n_axis + 64)
    used = 0
    corners = fr.corners()
    mn = corners[0]
    sc = grid_scale(fr.E)
    E = fr.E * sc
    anchors = cand_sites[:n_cand]
    used += n_cand
    b_at, b_in, b_out, at_ok = _pairs(fr, rng, anchors)
    # class per candidate: AT (where reachable), IN, OUT in turn
    cls = np.arange(n_cand) % 3
    cls = np.where((cls == AT) & ~at_ok, IN, cls)
    part = np.where((cls == AT)[:, None], b_at, np.where((cls == IN)[:, None], b_in, b_out))
    err = pair_error(anchors, part, metric, mn, sc, E, fr.eps)
    keep = np.sort(np.argsort(-err, kind="stable")[:n_pairs])
    A, B, C = anchors[keep], part[keep], cls[keep]
    max_err = float(err.max())
    # axis-aligned pairs: dx == eps exactly, the other coordinates equal
    ax_sites = cand_sites[used:used + n_axis]
    used += n_axis
    cw = fr.eps * (1.0 + 2.0 ** -20)
    k = np.floor((ax_sites[:, 0] - mn[0]) / cw)
    ulp32 = np.spacing(np.float32(k * cw * sc)).astype(np.float64) / sc
    a0 = mn[0] + k * cw + rng.integers(-3, 4, n_axis) * 0.5 * ulp32
    aa = ax_sites.copy()
    aa[:, 0] = a0
    ab = aa.copy()
    ab[:, 0] = aa[:, 0] + fr.eps
    ok = ((ab[:, 0] - aa[:, 0]) == fr.eps) & (dist(aa, ab, metric) == fr.eps)
    aa, ab = aa[ok], ab[ok]
    pts = [corners, A, B, aa, ab]
    n_now = sum(len(p) for p in pts)
    fill_sites = cand_sites[used:]
    if min_points > n_now:
        per = int(math.ceil((min_points - n_now) / max(len(fill_sites), 1)))
        if per > 0:
            clump = fill_sites[:, None, :] + rng.uniform(-0.05, 0.05, (len(fill_sites), per, fr.gd)) * fr.eps
            pts.append(clump.reshape(-1, fr.gd))
    c = np.concatenate(pts)
    n0 = len(corners)
    ia = np.arange(n0, n0 + len(A))
    ib = ia + len(A)
    ja = np.arange(n0 + 2 * len(A), n0 + 2 * len(A) + len(aa))
    jb = ja + len(aa)
    return dict(coords=c, eps=fr.eps, thr=fr.thr, metric=metric, frame=fr, cls=C, ia=ia, ib=ib, axis_a=ja,
                axis_b=jb, max_err=max_err, E=fr.E)


def frame_pairs(metric, frame, seed):
    """The pairs cloud of a frame: fine frames get filler clumps up to 32 points per eps-cell of the box."""
    fr = Frame(metric, *frame)
    need = 0
    if frame[0].startswith("fine"):
        need = int((fr.E / fr.eps + 2) ** fr.gd / 32) + 1000
    n_pairs = 2400 if fr.gd == 2 else 1500
    return pairs_cloud(metric, frame, seed, n_pairs=n_pairs, n_axis=300 if fr.gd == 2 else 150, min_points=need)


def _shell(fr, rng, centre, count):
    u = unit_dirs(rng, count, fr.metric)
    return walk_to_eps(np.broadcast_to(centre, (count, fr.gd)).copy(), centre + fr.eps * u, fr.metric, fr.eps)


def rings_cloud(metric, frame, seed, n_rings=6, ring=600, inside=400):
    """Probes with `ring` points on their eps-sphere.  Kind 0 (even rings): `inside` of them AT or IN, so with
    min_pts = 1 + inside the probe is core only if none is wrongly rejected; kind 1 (odd rings): inside - 1, so it is
    core only if some OUT point is wrongly accepted."""
    fr = Frame(metric, *frame)
    rng = np.random.default_rng(seed)
    cen = fr.sites(rng, n_rings, spacing=8.0)
    pts = [fr.corners()]
    probes, core = [], []
    n = 2
    for r in range(n_rings):
        b_at, b_in, b_out, at_ok = _shell(fr, rng, cen[r], ring)
        k_in = inside - (r % 2)
        cls = np.full(ring, OUT)
        cls[:k_in] = np.where(np.arange(k_in) % 2 == 0, AT, IN)
        cls = cls[rng.permutation(ring)]
        cls = np.where((cls == AT) & ~at_ok, IN, cls)
        p = np.where((cls == AT)[:, None], b_at, np.where((cls == IN)[:, None], b_in, b_out))
        pts += [cen[r][None], p]
        probes.append(n)
        core.append(r % 2 == 0)
        n += 1 + ring
    return dict(coords=np.concatenate(pts), eps=fr.eps, thr=fr.thr, metric=metric, frame=fr, min_pts=1 + inside,
                probes=np.array(probes), probe_core=np.array(core))


def dumbbells_cloud(metric, frame, seed, n_bells=24, min_pts=20):
    """Pairs of clumps of min_pts points, joined only by one AT / IN / OUT pair of their front points; a lone point at
    AT / IN / OUT behind each first clump's back point (border or noise)."""
    fr = Frame(metric, *frame)
    rng = np.random.default_rng(seed)
    cen = fr.sites(rng, n_bells, spacing=8.0)
    e = fr.eps
    u = unit_dirs(rng, n_bells, metric)
    # link pair: a = centre, b at eps along u
    b_at, b_in, b_out, at_ok = walk_to_eps(cen, cen + e * u, metric, e)
    link = np.arange(n_bells) % 3
    link = np.where((link == AT) & ~at_ok, IN, link)
    b = np.where((link == AT)[:, None], b_at, np.where((link == IN)[:, None], b_in, b_out))
    pts = [fr.corners()]
    info = []
    n = 2
    for k in range(n_bells):
        # clump points behind a (-u) and behind b (+u), 0.02 .. 0.1 eps deep, lateral offsets <= 0.004 eps
        def clump(base, sign, m):
            t = rng.uniform(0.02, 0.1, m) * e
            lat = rng.uniform(-0.002, 0.002, (m, fr.gd)) * e
            return base + sign * t[:, None] * u[k] + lat
        A = np.concatenate([cen[k][None], clump(cen[k], -1.0, min_pts - 2)])
        back = cen[k] - 0.15 * e * u[k]                    # the back point of clump A
        A = np.concatenate([A, back[None]])
        Bc = np.concatenate([b[k][None], clump(b[k], 1.0, min_pts - 1)])
        lb_at, lb_in, lb_out, lok = walk_to_eps(back[None], (back - e * u[k])[None], metric, e)
        lone_cls = k % 3 if (k % 3 != AT or lok[0]) else IN
        lone = (lb_at, lb_in, lb_out)[lone_cls]
        pts += [A, Bc, lone]
        info.append((n, n + len(A), n + len(A) + len(Bc), link[k], lone_cls))
        n += len(A) + len(Bc) + 1
    return dict(coords=np.concatenate(pts), eps=e, thr=fr.thr, metric=metric, frame=fr, min_pts=min_pts, bells=info)


# ---- exact reference --------------------------------------------------------------------------------------------
def exact_pairs(c, metric, eps):
    """Every unordered pair (i < j) with d(i, j) <= eps in binary64: candidates from cKDTree with a slightly larger
    radius, then the exact expression."""
    from scipy.spatial import cKDTree
    gd = gd_of(metric)
    x = c[:, :gd]
    fin = np.isfinite(x).all(1)
    idx = np.nonzero(fin)[0]
    t = cKDTree(x[idx])
    p = t.query_pairs(eps * (1.0 + 1e-9) + 1e-300, p=1 if metric == L1_2D else 2, output_type="ndarray")
    if len(p) == 0:
        return np.zeros((0, 2), np.int64)
    p = idx[p]
    keep = dist(c[p[:, 0]], c[p[:, 1]], metric) <= eps
    return p[keep]


def exact_core(c, metric, eps, min_pts):
    """is_core of DBImproved (the point counts itself) from exact_pairs."""
    n = len(c)
    p = exact_pairs(c, metric, eps)
    cnt = np.ones(n, np.int64) + np.bincount(p[:, 0], minlength=n) + np.bincount(p[:, 1], minlength=n)
    fin = np.isfinite(c[:, :gd_of(metric)]).all(1)
    return ((cnt >= min_pts) & fin).astype(np.uint8)


# ---- ICP ties ---------------------------------------------------------------------------------------------------
def d2(p, m):
    """The oracle's squared distance (FindClosestPointSet): (p0 - m0)*(p0 - m0) + ... left to right."""
    return (p[..., 0] - m[..., 0]) * (p[..., 0] - m[..., 0]) + (p[..., 1] - m[..., 1]) * (p[..., 1] - m[..., 1]) + \
        (p[..., 2] - m[..., 2]) * (p[..., 2] - m[..., 2])


def first_argmin(model, data, chunk=2048):
    """numpy brute force: index of the first exact minimum of d2 (NaN distances never win)."""
    out = np.zeros(len(data), np.int64)
    for s in range(0, len(data), chunk):
        q = data[s:s + chunk]
        d = d2(q[:, None, :], model[None, :, :])
        d = np.where(np.isnan(d), np.inf, d)
        out[s:s + chunk] = np.argmin(d, 1)
    return out


def score32(model, data, j):
    """The ICP screen's binary32 score h_j - q.m_j of model point j for each data point (k_icp_pass: coordinates
    relative to the centre of the model's bounding box, three fused multiply-adds; a fused operation is emulated as
    the exact binary64 product-sum rounded once)."""
    fin = np.isfinite(model).all(1)
    cen = (model[fin].min(0) + model[fin].max(0)) * 0.5
    mc = model[j] - cen
    mf = mc.astype(np.float32).astype(np.float64)
    w = (0.5 * (mc[:, 0] * mc[:, 0] + mc[:, 1] * mc[:, 1] + mc[:, 2] * mc[:, 2])).astype(np.float32).astype(np.float64)
    q = (data - cen).astype(np.float32).astype(np.float64)
    f32 = lambda x: x.astype(np.float32).astype(np.float64)
    s = f32(-q[:, 2] * mf[:, 2] + w)
    s = f32(-q[:, 1] * mf[:, 1] + s)
    return f32(-q[:, 0] * mf[:, 0] + s)


def icp_ties(nm, nd, seed, far=False, bad_model_point=False):
    """Model of nm points (random in a unit ball, plus tie pairs on a shell of radius 1.5 when nm > 2) and nd data
    points on the bisector planes of the tie pairs -- near the pair, or 1e3 away along the pair's outward direction,
    where the data point's own distance to the model's centre sets the screen's scale.  Each data point's two best
    squared distances are equal or 1-2 ulps apart, no third model point is nearer; for about half of the unequal ones
    the lower index is the farther point.  Returns dict(model, data, kind) with kind 0 = equal, 1 = lower index farther,
    2 = lower index nearer."""
    rng = np.random.default_rng(seed)
    n_tie = 1 if nm == 2 else min(48, (nm - 1) // 4)
    # A tie pair is split along (mostly) axis c with its midpoint ON the plane x_c = 0: the walked coordinate of a
    # data point near that plane has ulps far below the other distances' and can bring the two squared distances
    # within an ulp of each other.  The outward direction w of the pair has w_c = 0.
    ax = rng.integers(0, 3, n_tie)
    e_ax = np.eye(3)[ax]
    w = rng.normal(size=(n_tie, 3)) * (1.0 - e_ax)
    w /= np.sqrt((w * w).sum(1))[:, None]
    tilt = np.cross(w, e_ax) * rng.uniform(-0.3, 0.3, (n_tie, 1))
    nrm = e_ax + tilt
    nrm /= np.sqrt((nrm * nrm).sum(1))[:, None]
    delta = 0.05
    mid = 1.5 * w
    pj = mid + delta * nrm
    pk = mid - delta * nrm
    if nm == 2:
        model = np.concatenate([pj, pk])
        tie_j, tie_k = np.array([0]), np.array([1])
    else:
        rest = nm - 2 * n_tie
        r = rng.normal(size=(rest, 3))
        r = r / np.sqrt((r * r).sum(1))[:, None] * rng.uniform(0, 1, (rest, 1)) ** (1 / 3)
        model = np.concatenate([r, pj, pk])
        perm = rng.permutation(nm)
        model = model[perm]
        inv = np.argsort(perm)
        tie_j, tie_k = inv[rest:rest + n_tie], inv[rest + n_tie:]
    if bad_model_point:
        model[1 + rng.integers(0, nm - 1)] = [np.nan, 0.0, 0.0]   # never index 0: the reference seeds with model[0]
    # candidates: several per wanted point, walked on the coordinate along which the pair is split most
    m = 5 * nd + 64
    t = rng.integers(0, n_tie, m)
    j, k = tie_j[t], tie_k[t]
    mj, mk = model[j], model[k]
    mmid = (mj + mk) * 0.5
    diff = mk - mj
    nn = diff / np.sqrt((diff * diff).sum(1))[:, None]
    lat = rng.normal(size=(m, 3))
    lat -= (lat * nn).sum(1)[:, None] * nn
    lat *= (rng.uniform(0, 0.5 * delta, m) / np.sqrt((lat * lat).sum(1)))[:, None]
    p = mmid + lat
    if far:
        p = p + 1e3 * w[t]
    c = ax[t]
    rows = np.arange(m)
    o0 = to_ord(p[rows, c])
    span = np.abs(to_ord(p[rows, c] + 0.5 * delta) - o0)
    sgn = np.where(diff[rows, c] > 0, 1, -1)   # moving p towards mk along c makes d2(p, mk) smaller

    def at(tt):
        q = p.copy()
        q[rows, c] = from_ord(o0 + sgn * tt)
        return q

    lo = -span
    hi = span
    # largest step with d2(p, mj) <= d2(p, mk) (true far on the mj side, false far on the mk side)
    tc = _last_true(lambda tt: d2(at(tt), mj) <= d2(at(tt), mk), lo, hi)
    off = rng.integers(-1, 3, m)                   # the crossing and its neighbours: equal or 1-2 ulps apart
    q = at(tc + off)
    dj, dk = d2(q, mj), d2(q, mk)
    gap = np.abs(to_ord(dj) - to_ord(dk))
    ok = gap <= 2
    # no third model point as near as the nearer of the two (candidates from cKDTree, decided on the exact d2)
    from scipy.spatial import cKDTree
    fin = np.nonzero(np.isfinite(model).all(1))[0]
    _, nb = cKDTree(model[fin]).query(q, k=min(3, len(fin)))
    nb = fin[nb.reshape(m, -1)]
    best = np.minimum(dj, dk)
    ok &= (np.minimum(nb[:, 0], nb[:, 1]) == np.minimum(j, k)) & (np.maximum(nb[:, 0], nb[:, 1]) == np.maximum(j, k))
    if nb.shape[1] > 2:
        ok &= d2(q, model[nb[:, 2]]) > best * (1.0 + 1e-9)
    lowj = j < k
    d_low = np.where(lowj, dj, dk)
    d_high = np.where(lowj, dk, dj)
    kind = np.where(gap == 0, 0, np.where(d_low > d_high, 1, 2))
    sel = np.nonzero(ok)[0]
    if len(sel) < nd:
        raise ValueError("icp_ties: %d of %d candidates kept" % (len(sel), nd))
    sel = rng.permutation(sel)[:nd]
    return dict(model=model, data=q[sel], kind=kind[sel], j=j[sel], k=k[sel])
