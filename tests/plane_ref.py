"""The definition of include/vcp_planes.h restated in numpy binary64 and Python integers: the residual, the inlier rule,
the plane of a triple, the score, the splitmix64 sampler, the extraction loop with its refit through
cluster_moments_ref.moments, and the inputs of the tests.  No GPU, no library.  Every numpy operation is one binary64 ufunc
call (numpy contracts nothing); the counts are integers, so the library's results are compared with these for equality."""
import numpy as np

import cluster_moments_ref as MR

M64 = (1 << 64) - 1
MAX_H = 65536
MAX_PLANES = 64


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def same(a, b):
    """Equal shapes and equal bits (floats) or values (integers)."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape:
        return False
    if b.dtype.kind == "f":
        return a.dtype == b.dtype and np.array_equal(bits(a), bits(b))
    return np.array_equal(a.astype(np.int64), b.astype(np.int64))


# ---- the sampler --------------------------------------------------------------------------------------------------------
def mix(seed, c):
    z = (seed + 0x9E3779B97F4A7C15 * (c + 1)) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def sample_slot(seed, c, m):
    """The high half of the 128-bit product mix(seed, c) * m: a slot of the active list."""
    return (mix(seed, c) * m) >> 64


def sample(seed, r, H, act):
    """The triples [H, 3] int32 of round r from the active list act (rows in ascending index)."""
    m = len(act)
    return np.array([[act[sample_slot(seed, (r * H + h) * 3 + j, m)] for j in range(3)] for h in range(H)],
                    np.int32).reshape(H, 3)


# ---- residual, inlier, score ------------------------------------------------------------------------------------------------
def residual(pts, plane):
    """r = fl(fl(fl(fl(a x) + fl(b y)) + fl(c z)) + d) per row of pts [n, >= 3]."""
    pts = np.asarray(pts, np.float64)
    a, b, c, d = (np.float64(v) for v in plane)
    with np.errstate(all="ignore"):
        return ((a * pts[:, 0] + b * pts[:, 1]) + c * pts[:, 2]) + d


def inliers(pts, plane, thr, active=None):
    """bool [n]: active and fabs(r) <= thr (false for NaN)."""
    with np.errstate(all="ignore"):
        inl = np.abs(residual(pts, plane)) <= np.float64(thr)
    return inl if active is None else inl & (np.asarray(active) != 0)


def score(pts, planes, thr, active=None):
    """counts [H] int64."""
    pts = np.asarray(pts, np.float64)
    planes = np.asarray(planes, np.float64).reshape(-1, 4)
    H, n = len(planes), len(pts)
    out = np.zeros(H, np.int64)
    if n == 0:
        return out
    act = None if active is None else np.asarray(active) != 0
    x, y, z = pts[:, 0], pts[:, 1], pts[:, 2]
    step = max(1, (1 << 22) // n)
    with np.errstate(all="ignore"):
        for h0 in range(0, H, step):
            p = planes[h0:h0 + step]
            r = ((p[:, 0:1] * x + p[:, 1:2] * y) + p[:, 2:3] * z) + p[:, 3:4]
            inl = np.abs(r) <= np.float64(thr)
            if act is not None:
                inl &= act
            out[h0:h0 + step] = inl.sum(1)
    return out


# ---- the plane of a triple ----------------------------------------------------------------------------------------------------
def from_triples(pts, tri):
    """(planes [H, 4], valid [H] uint8) of the triples tri [H, 3]."""
    pts = np.asarray(pts, np.float64)
    tri = np.asarray(tri, np.int64).reshape(-1, 3)
    n, H = len(pts), len(tri)
    inr = ((tri >= 0) & (tri < n)).all(1)
    t = np.where(inr[:, None], tri, 0)
    planes = np.full((H, 4), np.nan)
    if n == 0:
        return planes, np.zeros(H, np.uint8)
    p0, p1, p2 = pts[t[:, 0], :3], pts[t[:, 1], :3], pts[t[:, 2], :3]
    with np.errstate(all="ignore"):
        u, v = p1 - p0, p2 - p0
        cx = u[:, 1] * v[:, 2] - u[:, 2] * v[:, 1]
        cy = u[:, 2] * v[:, 0] - u[:, 0] * v[:, 2]
        cz = u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0]
        nrm = np.sqrt((cx * cx + cy * cy) + cz * cz)
        a, b, c = cx / nrm, cy / nrm, cz / nrm
        d = -((a * p0[:, 0] + b * p0[:, 1]) + c * p0[:, 2])
        ok = inr & np.isfinite(nrm) & (nrm > 0.0) & np.isfinite(a) & np.isfinite(b) & np.isfinite(c) & np.isfinite(d)
    planes[ok] = np.stack([a, b, c, d], axis=1)[ok]
    return planes, ok.astype(np.uint8)


# ---- label --------------------------------------------------------------------------------------------------------------------
def label(pts, plane, thr, ident, labels, active=None):
    """(labels, active, n_labelled) after vcp_plane_label_dev; the inputs are not modified."""
    inl = inliers(pts, plane, thr, active)
    labels = np.array(labels, np.int32)
    labels[inl] = ident
    if active is not None:
        active = np.array(active, np.uint8)
        active[inl] = 0
    return labels, active, int(inl.sum())


# ---- the extraction -------------------------------------------------------------------------------------------------------------
def refit_plane(pts, inl):
    """(plane [4], valid) from vcp_cluster_moments of the rows inl: the axis of the smallest eigenvalue through the mean."""
    mom = MR.moments(np.ascontiguousarray(pts[:, :3]), inl.astype(np.int32), 1)
    a, b, c = (np.float64(v) for v in mom["evec"][0, 2])
    m = mom["mean"][0]
    with np.errstate(all="ignore"):
        d = -((a * m[0] + b * m[1]) + c * m[2])
    return np.array([a, b, c, d]), int(mom["valid"][0])


def ransac(pts, thr, H, max_planes, min_inliers=0, seed=0, refit=True, active=None):
    """dict(labels [n] int32, planes [max_planes, 4], counts, hyp_counts [max_planes] int64, n_planes, winners [h per
    round]) by the extraction of vcp_plane_ransac."""
    pts = np.asarray(pts, np.float64)
    n = len(pts)
    act = np.ones(n, bool) if active is None else np.asarray(active) != 0
    labels = np.zeros(n, np.int32)
    planes = np.full((max_planes, 4), np.nan)
    counts, hyp = np.zeros(max_planes, np.int64), np.zeros(max_planes, np.int64)
    need, np_, winners = max(int(min_inliers), 3), 0, []
    for r in range(max_planes):
        lst = np.nonzero(act)[0]
        if len(lst) < 3:
            break
        hp, _ = from_triples(pts, sample(seed, r, H, lst))
        cnt = score(pts, hp, thr, act)
        h = int(np.argmax(cnt))                     # the first of the largest: the lowest h
        if cnt[h] < need:
            break
        acc = hp[h]
        if refit:
            rp, ok = refit_plane(pts, inliers(pts, acc, thr, act))
            if ok == 1 and inliers(pts, rp, thr, act).sum() >= cnt[h]:
                acc = rp
        inl = inliers(pts, acc, thr, act)
        labels[inl] = r + 1
        act = act & ~inl
        planes[r], counts[r], hyp[r] = acc, inl.sum(), cnt[h]
        winners.append(h)
        np_ += 1
    return dict(labels=labels, planes=planes, counts=counts, hyp_counts=hyp, n_planes=np_, winners=winners)


KEYS = ("labels", "planes", "counts", "hyp_counts", "n_planes")


def differs(got, want, keys=KEYS):
    """None, or the first output of a ransac result that differs."""
    for k in keys:
        if k == "n_planes":
            if int(got[k]) != int(want[k]):
                return "n_planes %d, want %d" % (got[k], want[k])
        elif not same(got[k], want[k]):
            return k
    return None


# ---- inputs ---------------------------------------------------------------------------------------------------------------------
TRUE_PLANES = (((0.0, 0.0, 1.0), -1.5), ((1.0, 0.0, 0.0), 5.0), ((0.6, 0.75, 0.28), 6.0))
SCENE = dict(thr=0.012, H=256, max_planes=5, min_inliers=1000)


def scene(seed, per_plane=4000, spheres=20, per_sphere=150, background=3000):
    """(pts [n, 3] on the 2^-20 lattice, shuffled; truth [n] int32: 1..3 the plane a row was drawn on, 0 otherwise; normals
    [3, 3]; offsets [3]): three planes n . p = offset, uniform in +-4 along two in-plane axes with normal noise sigma
    0.004, sphere targets of radius 0.0725, uniform background in [-5, 7]^3."""
    rng = np.random.default_rng(seed)
    rows, truth, normals, offs = [], [], [], []
    for k, (nv, off) in enumerate(TRUE_PLANES):
        nv = np.asarray(nv, np.float64)
        nv = nv / np.linalg.norm(nv)
        e1 = np.cross(nv, [0.3, 0.5, 0.8])
        e1 /= np.linalg.norm(e1)
        e2 = np.cross(nv, e1)
        s = rng.uniform(-4, 4, (per_plane, 2))
        rows.append(off * nv + s[:, :1] * e1 + s[:, 1:] * e2 + rng.normal(0, 0.004, (per_plane, 1)) * nv)
        truth.append(np.full(per_plane, k + 1))
        normals.append(nv)
        offs.append(off)
    for _ in range(spheres):
        c = rng.uniform(-3, 3, 3) + np.array([0.0, 0.0, 1.0])
        v = rng.normal(size=(per_sphere, 3))
        v /= np.linalg.norm(v, axis=1)[:, None]
        rows.append(c + 0.0725 * v)
        truth.append(np.zeros(per_sphere))
    rows.append(rng.uniform(-5, 7, (background, 3)))
    truth.append(np.zeros(background))
    pts, truth = np.concatenate(rows), np.concatenate(truth).astype(np.int32)
    pts = np.round(pts * 2.0 ** 20) / 2.0 ** 20
    order = rng.permutation(len(pts))
    return np.ascontiguousarray(pts[order]), truth[order], np.array(normals), np.array(offs)


def scene_call(k):
    """The arguments of the recovery call on scene k."""
    return dict(SCENE, seed=12345 + k)


def scene_mask(k, n=18000):
    """The `active` of the masked runs on scene k: about four rows in five."""
    return (np.random.default_rng([81, k]).random(n) < 0.8).astype(np.uint8)


_fits = {}


def scene_fit(k, refit=True, masked=False):
    """(pts, truth, normals, the restatement's result) of the recovery call on scene k, computed once per process and
    shared by the tests that need it; nobody modifies it."""
    key = (k, bool(refit), bool(masked))
    if key not in _fits:
        pts, truth, normals, _ = scene(k)
        fit = ransac(pts, refit=refit, active=scene_mask(k, len(pts)) if masked else None, **scene_call(k))
        for a in (pts, truth, normals, fit["labels"], fit["planes"], fit["counts"], fit["hyp_counts"]):
            a.setflags(write=False)
        _fits[key] = (pts, truth, normals, fit)
    return _fits[key]


def recovery(fit, truth, normals):
    """Per accepted plane (matched true plane, angle in degrees, recall, foreign rows)."""
    out = []
    for r in range(fit["n_planes"]):
        nv = fit["planes"][r, :3]
        cosv = np.abs(normals @ nv) / np.linalg.norm(nv)
        k = int(np.argmax(cosv))
        ang = float(np.degrees(np.arccos(min(1.0, cosv[k]))))
        on = fit["labels"] == r + 1
        out.append((k, ang, float((on & (truth == k + 1)).sum()) / float((truth == k + 1).sum()),
                    int((on & (truth != k + 1)).sum())))
    return out


def lattice_rows(n, seed, span=4.0, step=2.0 ** -10):
    """n rows [n, 3] on the lattice of pitch 2^-10 in [-span, span)^3."""
    rng = np.random.default_rng([78, seed])
    k = int(span / step)
    return rng.integers(-k, k, (n, 3)).astype(np.float64) * step


def lattice_planes(H, seed):
    """H planes [H, 4] whose coefficients are small multiples of 1/8: every product and sum with lattice_rows is exact, and
    the residuals fall on thr = 0.25 exactly for many rows."""
    rng = np.random.default_rng([79, seed])
    return rng.integers(-8, 9, (H, 4)).astype(np.float64) / 8.0


def generic_planes(H, seed):
    """H unit-normal planes through the box of lattice_rows."""
    rng = np.random.default_rng([80, seed])
    nv = rng.normal(size=(H, 3))
    nv /= np.linalg.norm(nv, axis=1)[:, None]
    return np.concatenate([nv, rng.uniform(-3, 3, (H, 1))], axis=1)
