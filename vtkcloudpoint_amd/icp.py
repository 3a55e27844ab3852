"""Drop-in mirrors of BaseClass/ICP.cs and the slice of BaseClass/Matrix.cs it uses, and multi-start, gated, trimmed,
similarity and global (congruent-pair) ICP for MainForm.ICP's centroid-to-truth matching."""
import math

import numpy as np

from . import _native
from .datamodel import xyz_array
from .runtime import default_context


class MException(Exception):
    """BaseClass/Matrix.cs:710-715."""


class Matrix:
    """Row-major double matrix, BaseClass/Matrix.cs:18-34 (storage + indexer), :286-293 (Transpose),
    :500-561 (multiply/add/trace), :692-705 (operators).  Only what ICP's R / T carriers need."""

    def __init__(self, iRows, iCols):
        self.rows, self.cols = int(iRows), int(iCols)
        self.mat = [0.0] * (self.rows * self.cols)

    def __getitem__(self, rc):
        r, c = rc
        return self.mat[r * self.cols + c]  # flat-array bounds only, like the C# (Matrix.cs:30-34)

    def __setitem__(self, rc, v):
        r, c = rc
        self.mat[r * self.cols + c] = float(v)

    @staticmethod
    def ZeroMatrix(r, c):
        return Matrix(r, c)

    @staticmethod
    def IdentityMatrix(r, c):
        m = Matrix(r, c)
        for i in range(min(r, c)):
            m[i, i] = 1.0
        return m

    def Duplicate(self):
        m = Matrix(self.rows, self.cols)
        m.mat = list(self.mat)
        return m

    @staticmethod
    def Transpose(m):
        t = Matrix(m.cols, m.rows)
        for i in range(m.rows):
            for j in range(m.cols):
                t[j, i] = m[i, j]
        return t

    @staticmethod
    def Multiply(a, b):
        if isinstance(a, (int, float)):
            r = Matrix(b.rows, b.cols)
            r.mat = [v * a for v in b.mat]
            return r
        if a.cols != b.rows:
            raise MException("Wrong dimension of matrix!")
        r = Matrix(a.rows, b.cols)
        for i in range(a.rows):
            for j in range(b.cols):
                s = 0.0
                for k in range(a.cols):
                    s += a[i, k] * b[k, j]  # StupidMultiply, Matrix.cs:500-510
                r[i, j] = s
        return r

    @staticmethod
    def Add(a, b):
        if a.rows != b.rows or a.cols != b.cols:
            raise MException("Matrices must have the same dimensions!")
        r = Matrix(a.rows, a.cols)
        r.mat = [x + y for x, y in zip(a.mat, b.mat)]
        return r

    @staticmethod
    def TR(m):
        return sum(m[i, i] for i in range(m.rows))

    def __add__(self, o):
        return Matrix.Add(self, o)

    def __sub__(self, o):
        return Matrix.Add(self, Matrix.Multiply(-1, o))

    def __mul__(self, o):
        return Matrix.Multiply(self, o)

    def __rmul__(self, n):
        return Matrix.Multiply(n, self)

    def to_numpy(self):
        return np.array(self.mat).reshape(self.rows, self.cols)


class ICP:
    """BaseClass/ICP.cs:8-314.  go_hell_ICP keeps the C#'s signature and in-place outputs (R 3x3, T 3x1).
    The arithmetic is the INTENDED Besl-McKay / Horn loop: the as-written C# is non-functional (integer
    division :53, '+' at :66, delta index :76, Jacobi indexing Matrix.cs:636-666, i<9 loop :170-174)."""

    max_iter = 1000  # the C# loops until |d - pre_d| < e with no bound; this is the safety net

    def __init__(self, ctx=None):
        self._ctx = ctx
        self.last = None

    def go_hell_ICP(self, model, data, R, T, e):
        if R.rows != 3 or R.cols != 3 or T.rows != 3 or T.cols != 1:
            raise MException("R must be 3x3 and T 3x1")
        ctx = self._ctx or default_context()
        if len(data) == 0:
            return
        r = ctx.icp(xyz_array(model), xyz_array(data), float(e), self.max_iter, _native.STOP_SSE_DELTA)
        self.last = r
        if r["iters"] == 1 and r["sse"] < e:
            return  # the C# never writes R, T when the very first round already satisfies the stop rule
        for i in range(3):
            for j in range(3):
                R[i, j] = r["R"][i, j]
            T[i, 0] = r["T"][i]

    # the individually-correct sub-functions, kept for source compatibility (host side, tiny inputs)
    @staticmethod
    def CalculateRotation(q, R):
        """ICP.cs:274-285 (Matrix form) / :183-194 (array form)."""
        g = (lambda i: q[i, 0]) if isinstance(q, Matrix) else (lambda i: q[i])
        q0, q1, q2, q3 = g(0), g(1), g(2), g(3)
        vals = [q0 * q0 + q1 * q1 - q2 * q2 - q3 * q3, 2.0 * (q1 * q2 - q0 * q3), 2.0 * (q1 * q3 + q0 * q2),
                2.0 * (q1 * q2 + q0 * q3), q0 * q0 - q1 * q1 + q2 * q2 - q3 * q3, 2.0 * (q2 * q3 - q0 * q1),
                2.0 * (q1 * q3 - q0 * q2), 2.0 * (q2 * q3 + q0 * q1), q0 * q0 - q1 * q1 - q2 * q2 + q3 * q3]
        for k, v in enumerate(vals):
            if isinstance(R, Matrix):
                R[k // 3, k % 3] = v
            else:
                R[k] = v

    def FindClosestPointSet(self, model, data):
        """ICP.cs:224-250 on the GPU: returns the list Y of matched model points."""
        ctx = self._ctx or default_context()
        if len(model) == 0:
            raise IndexError("model[0] (ICP.cs:233)")
        if len(data) == 0:
            return []
        _, nn = ctx.icp_sums(xyz_array(model), xyz_array(data))
        return [model[int(j)] for j in nn]


def rotations_about_z(n, mirror=False):
    """[n, 3, 3] rotations Rz(h * 2 pi / n), h = 0..n-1 (element 0 exactly the identity); mirror=True appends the n
    reflections Rz(theta) @ diag(1, -1, 1) (det -1: the source's y axis reversed), giving [2n, 3, 3]."""
    n = int(n)
    out = []
    for h in range(n):
        t = h * (2.0 * math.pi / n)
        c, s = math.cos(t), math.sin(t)
        out.append([[c, 0.0 - s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])
    if mirror:
        for h in range(n):
            c, s = out[h][0][0], out[h][1][0]
            out.append([[c, s, 0.0], [s, 0.0 - c, 0.0], [0.0, 0.0, 1.0]])
    return np.array(out, dtype=np.float64).reshape(-1, 3, 3)


def multistart_icp(centers, truths, n_angles=36, mirror=False, init_T=None, max_iter=100, max_landmarks=200,
                   inlier_dist=np.inf, ctx=None):
    """MainForm.ICP()'s match of cluster centroids to truth points, started from n_angles rotations about z (and their
    mirror images with mirror=True) instead of the centroid start alone; the pose with the most centroids within
    inlier_dist of a truth wins.  centers / truths: [n, 3] arrays or lists of points with X, Y, Z.  Returns
    Context.icp_multistart's dict (best, M, M_all, mean_dist, inliers)."""
    ctx = ctx or default_context()
    src = _points(centers)
    tgt = _points(truths)
    poses = rotations_about_z(n_angles, mirror) if mirror else int(n_angles)
    return ctx.icp_multistart(src, tgt, poses, init_T, max_iter, max_landmarks, inlier_dist)


def gate_schedule(start, end, rounds):
    """`rounds` gates from `start` to `end` in geometric steps: the first entry is exactly `start`, the last exactly
    `end`, and the list never rises (start >= end > 0).  rounds = 1 gives [end].  vcp_icp_gated holds the last gate for
    every round beyond the schedule."""
    start, end, rounds = float(start), float(end), int(rounds)
    if rounds < 1:
        raise ValueError("rounds < 1")
    if not (end > 0.0 and start >= end):
        raise ValueError("need start >= end > 0")
    if rounds == 1:
        return np.array([end])
    if math.isinf(start):
        g = np.full(rounds, start)
    else:
        la, lb = math.log(start), math.log(end)
        g = np.array([math.exp(la + (lb - la) * (k / (rounds - 1.0))) for k in range(rounds)])
    g[0], g[-1] = start, end
    g = np.minimum.accumulate(np.clip(g, end, start))  # rounding may not undo the order
    return g


def gated_icp(centers, truths, gates, n_angles=1, mirror=False, init_T=None, max_iter=100, max_landmarks=200,
              min_pairs=3, inlier_dist=np.inf, ctx=None):
    """multistart_icp with a gate on the correspondence distance: round r leaves every centroid whose nearest truth is
    gates[min(r, len(gates)) - 1] or farther away out of that round's fit, so false clusters beside or between the
    targets stop pulling the pose once the gate has closed below their distance (gate_schedule makes a shrinking
    schedule).  n_angles may also be an [H, 3, 3] array of start rotations.  Returns Context.icp_gated's dict (best, M,
    M_all, mean_dist, inliers, kept, starved)."""
    ctx = ctx or default_context()
    src = _points(centers)
    tgt = _points(truths)
    if isinstance(n_angles, (int, np.integer)):
        poses = rotations_about_z(n_angles, mirror) if mirror else int(n_angles)
    else:
        poses = np.asarray(n_angles, np.float64)
    return ctx.icp_gated(src, tgt, gates, poses, init_T, max_iter, max_landmarks, min_pairs, inlier_dist)


def unique_icp(centers, truths, gates, n_angles=1, mirror=False, init_T=None, max_iter=100, max_landmarks=200,
               min_pairs=3, inlier_dist=np.inf, ctx=None):
    """gated_icp where a truth takes one centroid per round (vcp_icp_unique, "picky ICP"): of the centroids whose
    nearest truth is the same one, only the closest enters that round's fit (ties: the lower index), and the round's
    gate then decides on it as in gated_icp.  A target makes one centroid; a second cluster beside it (a split target, a
    reflection, an edge return) lies inside any gate that admits the real centroids and pulls gated_icp's pose by its
    offset times the ghosts' share of the pairs.  n_angles may also be an [H, 3, 3] array of start rotations.  Returns
    Context.icp_unique's dict (gated_icp's plus lost, the last round's count of centroids that lost their truth)."""
    ctx = ctx or default_context()
    src = _points(centers)
    tgt = _points(truths)
    if isinstance(n_angles, (int, np.integer)):
        poses = rotations_about_z(n_angles, mirror) if mirror else int(n_angles)
    else:
        poses = np.asarray(n_angles, np.float64)
    return ctx.icp_unique(src, tgt, gates, poses, init_T, max_iter, max_landmarks, min_pairs, inlier_dist)


def similarity_icp(centers, truths, gates, ratio_range, n_angles=1, mirror=False, init_T=None, max_iter=100,
                   max_landmarks=200, min_pairs=3, inlier_dist=np.inf, ctx=None):
    """gated_icp whose every round also fits one isotropic scale (vcp_icp_sim: Horn's symmetric scale of the kept pairs,
    sqrt(spread of the truths / spread of the centroids)), for centroids whose unit is only roughly the truths': a start
    scale that is off by 2 % moves the edge of a 20 x 20 field by more than a closed gate of 0.1, and the rigid loop then
    keeps only the middle of the field.  ratio_range = (lo, hi), lo <= 1 <= hi, bounds the product of the factors a pose
    applies to its start; (1, 1) is gated_icp bit for bit.  n_angles may also be an [H, 3, 3] array of start matrices
    (rotations times the start scale).  Returns Context.icp_sim's dict (gated_icp's plus ratio, unscaled)."""
    ctx = ctx or default_context()
    src = _points(centers)
    tgt = _points(truths)
    if isinstance(n_angles, (int, np.integer)):
        poses = rotations_about_z(n_angles, mirror) if mirror else int(n_angles)
    else:
        poses = np.asarray(n_angles, np.float64)
    return ctx.icp_sim(src, tgt, gates, ratio_range, poses, init_T, max_iter, max_landmarks, min_pairs, inlier_dist)


def bbox_scale_xy(centers, truths):
    """(sx, sy): the reference's two factors, sx = the truths' x extent over the centroids' and sy likewise for y
    (MainForm.showTruesAndCenters, FrmMain.cs:3046-3049), as a START value for anisotropic_icp.  Its weakness is the
    bounding box's: the factors are only right when the scan covers the whole truth field, one false cluster outside
    the field stretches an extent by its whole distance, and the boxes are taken along the centroids' own axes, so a
    rotation between the two frames mixes the extents.  anisotropic_icp refines the start; it cannot repair one that
    lies outside its ratio range."""
    src, tgt = _points(centers), _points(truths)
    return tuple((float(tgt[:, c].max()) - float(tgt[:, c].min())) / (float(src[:, c].max()) - float(src[:, c].min()))
                 for c in (0, 1))


def anisotropic_icp(centers, truths, scale0=None, ratio=(0.9, 1.1), gates=None, n_angles=1, mirror=False, init_T=None,
                    max_iter=100, max_landmarks=200, min_pairs=3, inlier_dist=np.inf, ctx=None):
    """gated_icp whose every round also fits one scale for x and one for y (vcp_icp_aniso): the pose is
    truth ~ R diag(sx, sy, 1) centroid + t, the reference's tmp_X = X * scale[0], tmp_Y = Y * scale[1] followed by its
    rigid ICP, with the two factors fitted by least squares on the kept pairs in every round instead of taken once from
    two bounding boxes.  The motor's two axes do not have the same gain, so sx != sy is the normal case, and
    similarity_icp's one factor leaves half the difference at the edge of the field.
    scale0: None (1, 1), one (sx, sy) for every start, or [H, 2] (bbox_scale_xy gives the reference's value);
    ratio = (lo, hi), lo <= 1 <= hi, bounds each scale to that multiple of its start; gates: None is the ungated loop.
    n_angles may also be an [H, 3, 3] array of start ROTATIONS (the scales are applied to them by the library).  Returns
    Context.icp_aniso's dict (gated_icp's plus scale [H, 2], unscaled [H, 2]); M holds [R diag(sx, sy, 1) | t]."""
    ctx = ctx or default_context()
    src = _points(centers)
    tgt = _points(truths)
    if isinstance(n_angles, (int, np.integer)):
        poses = rotations_about_z(n_angles, mirror) if mirror else int(n_angles)
        H = len(poses) if mirror else poses
    else:
        poses = np.asarray(n_angles, np.float64)
        H = len(poses.reshape(-1, 9))
    if scale0 is not None:
        scale0 = np.asarray(scale0, np.float64)
        scale0 = np.ascontiguousarray(np.broadcast_to(scale0.reshape(-1, 2), (H, 2)))
    gates = [np.inf] if gates is None else gates
    return ctx.icp_aniso(src, tgt, gates, ratio, poses, init_T, scale0, max_iter, max_landmarks, min_pairs, inlier_dist)


def trim_schedule(start, end, rounds):
    """`rounds` keep shares that fall linearly from `start` to `end` (1 >= start >= end > 0): the first entry is exactly
    `start`, the last exactly `end`, and the list never rises.  rounds = 1 gives [end].  vcp_icp_trimmed holds the last
    share for every round beyond the schedule."""
    start, end, rounds = float(start), float(end), int(rounds)
    if rounds < 1:
        raise ValueError("rounds < 1")
    if not (end > 0.0 and start >= end and start <= 1.0):
        raise ValueError("need 1 >= start >= end > 0")
    if rounds == 1:
        return np.array([end])
    f = np.array([start + (end - start) * (k / (rounds - 1.0)) for k in range(rounds)])
    f[0], f[-1] = start, end
    return np.minimum.accumulate(np.clip(f, end, start))  # rounding may not undo the order


def expected_share(n_centers, n_truths, visible=1.0):
    """min(1, visible * n_truths / n_centers): the share of the centroids that are real targets when the scan sees the
    fraction `visible` of the truths -- the keep share trimmed_icp is meant to be given."""
    n_centers, n_truths, visible = int(n_centers), int(n_truths), float(visible)
    if n_centers < 1 or n_truths < 1 or not (0.0 < visible <= 1.0):
        raise ValueError("need n_centers >= 1, n_truths >= 1 and 0 < visible <= 1")
    return min(1.0, visible * n_truths / n_centers)


def trimmed_icp(centers, truths, keep, n_angles=1, mirror=False, init_T=None, max_iter=100, max_landmarks=200,
                min_pairs=3, inlier_dist=np.inf, ctx=None):
    """multistart_icp where every round fits on a share of the pairs: round r keeps the
    ceil(keep[min(r, len(keep)) - 1] * L) of the L landmarks closest to their nearest truth and leaves the others out
    of that round's fit (Chetverikov's trimmed ICP).  The share is what the caller knows before any pose exists
    (expected_share), where gated_icp's distances need the start error, the noise and the unit; keep may be one number.
    n_angles may also be an [H, 3, 3] array of start rotations.  Returns Context.icp_trimmed's dict (best, M, M_all,
    mean_dist, inliers, kept, starved, trim_dist)."""
    ctx = ctx or default_context()
    src = _points(centers)
    tgt = _points(truths)
    if isinstance(n_angles, (int, np.integer)):
        poses = rotations_about_z(n_angles, mirror) if mirror else int(n_angles)
    else:
        poses = np.asarray(n_angles, np.float64)
    keep = np.atleast_1d(np.asarray(keep, np.float64))
    return ctx.icp_trimmed(src, tgt, keep, poses, init_T, max_iter, max_landmarks, min_pairs, inlier_dist)


def choose_bases(source, n_bases, min_len, max_len, seed=0):
    """[n_bases, 2] int32 pairs of source indices for register_pairs: np.random.default_rng(seed).integers(0, ns, 2) is
    drawn until n_bases pairs are accepted, a pair (a, b) being accepted when a != b and its planar length lies in
    [min_len, max_len].  A short base fits many target pairs (slow, ambiguous), a long one may leave the overlap.
    Raises ValueError after 1000 * n_bases draws."""
    src = _points(source)
    ns, n_bases = len(src), int(n_bases)
    if ns < 2 or n_bases < 1:
        raise ValueError("need two source points and n_bases >= 1")
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(1000 * n_bases):
        a, b = (int(v) for v in rng.integers(0, ns, 2))
        ux, uy = float(src[b, 0] - src[a, 0]), float(src[b, 1] - src[a, 1])
        if a != b and min_len <= math.sqrt(ux * ux + uy * uy) <= max_len:
            out.append((a, b))
            if len(out) == n_bases:
                return np.array(out, np.int32)
    raise ValueError("%d of %d bases with a length in [%g, %g] after %d draws" % (len(out), n_bases, min_len, max_len,
                                                                               1000 * n_bases))


def register_pairs(centers, truths, bases, len_tol, inlier_dist, mirror=False, max_landmarks=200, ctx=None):
    """A pose of the centroids on the truths without any start (vcp_register_pairs): each base (choose_bases) is laid on
    every ordered pair of truths of its own length within len_tol, and the pose that puts the most landmarks within
    inlier_dist of a truth is kept per base.  Works where the scan sees only part of the truth field, which the centroid
    start of multistart_icp / gated_icp cannot.  Returns Context.register_pairs's dict (best, M, M_all, score, inliers,
    pick, n_hyp)."""
    ctx = ctx or default_context()
    return ctx.register_pairs(_points(centers), _points(truths), bases, len_tol, inlier_dist, mirror, max_landmarks)


def global_icp(centers, truths, bases, len_tol, inlier_dist, gates, mirror=False, max_iter=20, max_landmarks=200,
               min_pairs=3, ctx=None, keep=None):
    """register_pairs, then ONE gated_icp call started from the pose of every base that found one (score >= 0).  Returns
    gated_icp's dict (best indexes the started poses) plus registration = register_pairs's dict and bases_used = the base
    of every started pose.  ValueError when no base has a hypothesis.  keep (a share or a schedule of shares): the
    polish is one trimmed_icp call instead (its dict, with trim_dist), and gates may be None."""
    ctx = ctx or default_context()
    src, tgt = _points(centers), _points(truths)
    reg = ctx.register_pairs(src, tgt, bases, len_tol, inlier_dist, mirror, max_landmarks)
    used = np.flatnonzero(reg["score"] >= 0)
    if len(used) == 0:
        raise ValueError("no base has a target pair of its length within len_tol")
    M = reg["M_all"][used]
    Rs, Ts = np.ascontiguousarray(M[:, :3, :3]), np.ascontiguousarray(M[:, :3, 3])
    if keep is not None:
        out = ctx.icp_trimmed(src, tgt, np.atleast_1d(np.asarray(keep, np.float64)), Rs, Ts, max_iter, max_landmarks,
                              min_pairs, inlier_dist)
    else:
        out = ctx.icp_gated(src, tgt, gates, Rs, Ts, max_iter, max_landmarks, min_pairs, inlier_dist)
    out.update(registration=reg, bases_used=used)
    return out


def global_unique_icp(centers, truths, bases, len_tol, inlier_dist, gates, mirror=False, max_iter=20, max_landmarks=200,
                      min_pairs=3, ctx=None):
    """global_icp whose polish lets a truth take one centroid per round: register_pairs, then ONE unique_icp call
    started from the pose of every base that found one (score >= 0).  Returns unique_icp's dict (best indexes the
    started poses; lost) plus registration = register_pairs's dict and bases_used.  ValueError when no base has a
    hypothesis."""
    ctx = ctx or default_context()
    src, tgt = _points(centers), _points(truths)
    reg = ctx.register_pairs(src, tgt, bases, len_tol, inlier_dist, mirror, max_landmarks)
    used = np.flatnonzero(reg["score"] >= 0)
    if len(used) == 0:
        raise ValueError("no base has a target pair of its length within len_tol")
    M = reg["M_all"][used]
    out = ctx.icp_unique(src, tgt, gates, np.ascontiguousarray(M[:, :3, :3]), np.ascontiguousarray(M[:, :3, 3]), max_iter,
                         max_landmarks, min_pairs, inlier_dist)
    out.update(registration=reg, bases_used=used)
    return out


def register_similarity(centers, truths, bases, scale_range, inlier_dist, mirror=False, max_landmarks=200, ctx=None):
    """register_pairs for centroids whose unit is not the truths' (vcp_register_sim): a base fits an ordered pair of truths
    whose length is k times its own, scale_range[0] <= k <= scale_range[1], and the pose is the planar similarity with
    that k.  Returns Context.register_sim's dict: register_pairs's plus scale [B], the winner's k per base."""
    ctx = ctx or default_context()
    lo, hi = scale_range
    return ctx.register_sim(_points(centers), _points(truths), bases, float(lo), float(hi), inlier_dist, mirror,
                            max_landmarks)


def bbox_scale_range(centers, truths, slack):
    """(min(sx, sy) / slack, max(sx, sy) * slack) from the reference's two factors, sx = the truths' x extent over the
    centroids' and sy likewise for y (MainForm.showTruesAndCenters, FrmMain.cs:3046-3055): a default prior for
    register_similarity's scale_range, slack >= 1.  It is only right when the scan covers the whole truth field and holds
    no false cluster at its edge: on a partial view the factors are the ratio of a window to the field, and a wide
    explicit range must be given instead."""
    src, tgt = _points(centers), _points(truths)
    slack = float(slack)
    if not slack >= 1.0:
        raise ValueError("slack < 1")
    s = [(float(tgt[:, c].max()) - float(tgt[:, c].min())) / (float(src[:, c].max()) - float(src[:, c].min()))
         for c in (0, 1)]
    return min(s) / slack, max(s) * slack


def fit_scale(p, y):
    """Horn's symmetric scale of paired rows, sqrt(sum |y - mean y|^2 / sum |p - mean p|^2): the k of the similarity
    y ~ k R p + T that does not depend on the rotation."""
    p, y = np.asarray(p, np.float64), np.asarray(y, np.float64)
    if p.shape != y.shape or len(p) < 2:
        raise ValueError("need two or more paired rows")
    dp, dy = p - p.mean(axis=0), y - y.mean(axis=0)
    return math.sqrt(float((dy * dy).sum()) / float((dp * dp).sum()))


def _linear_scale(R):
    """The scale of k times a rotation or reflection: sqrt(|det| of the planar block)."""
    return math.sqrt(abs(float(R[0, 0] * R[1, 1] - R[0, 1] * R[1, 0])))


def global_sim_icp(centers, truths, bases, scale_range, inlier_dist, gates, mirror=False, max_iter=20, max_landmarks=200,
                   min_pairs=3, refine=True, ctx=None):
    """global_icp where the centroids' unit is unknown: register_similarity, then ONE gated_icp call started from the
    similarity of every base that found one (vcp_icp_gated takes init_R as given and composes proper rotations onto it,
    so the scale rides through the rounds unchanged).  With refine, the best pose's one-to-one pairs at inlier_dist
    (match_unique) give fit_scale's k', and a second gated_icp call starts from R (k' / k), T0 = mean(y) - R0 mean(p).
    Returns gated_icp's dict (of the last call; best indexes its poses) plus registration = register_similarity's dict,
    bases_used, scale = the returned pose's scale (sqrt |det| of its planar block) and scale_registration = the registered k
    of the base whose start won the first call.  ValueError when
    no base has a hypothesis.  global_similarity_icp is the form whose polish fits the scale on the device."""
    ctx = ctx or default_context()
    src, tgt = _points(centers), _points(truths)
    lo, hi = scale_range
    reg = ctx.register_sim(src, tgt, bases, float(lo), float(hi), inlier_dist, mirror, max_landmarks)
    used = np.flatnonzero(reg["score"] >= 0)
    if len(used) == 0:
        raise ValueError("no base has a target pair with a length ratio in scale_range")
    M = reg["M_all"][used]
    out = ctx.icp_gated(src, tgt, gates, np.ascontiguousarray(M[:, :3, :3]), np.ascontiguousarray(M[:, :3, 3]), max_iter,
                        max_landmarks, min_pairs, inlier_dist)
    scale_reg = float(reg["scale"][used[out["best"]]])
    if refine:
        Mb = out["M"]
        mu = ctx.match_unique(src, tgt, Mb, inlier_dist)
        got = np.flatnonzero(mu["truth_of"] >= 0)
        if len(got) >= 2:
            p, y = src[got], tgt[mu["truth_of"][got]]
            k1 = fit_scale(p, y)
            R0 = np.ascontiguousarray(Mb[:3, :3] * (k1 / _linear_scale(Mb[:3, :3])))
            T0 = y.mean(axis=0) - R0 @ p.mean(axis=0)
            out = ctx.icp_gated(src, tgt, gates, R0[None], np.ascontiguousarray(T0)[None], max_iter, max_landmarks,
                                min_pairs, inlier_dist)
    out.update(registration=reg, bases_used=used, scale=_linear_scale(out["M"][:3, :3]), scale_registration=scale_reg)
    return out


def global_similarity_icp(centers, truths, bases, scale_range, inlier_dist, gates, ratio_range, mirror=False,
                          max_iter=20, max_landmarks=200, min_pairs=3, ctx=None):
    """global_sim_icp whose polish fits the scale itself: register_similarity, then ONE similarity_icp call
    (vcp_icp_sim) started from the similarity of every base that found one, the product of each pose's scale factors
    held in ratio_range = (lo, hi), lo <= 1 <= hi.  There is no host refit: the rounds do on the device what
    global_sim_icp's match_unique / fit_scale / second-call alternation approximates.  Returns similarity_icp's dict
    (best indexes the started poses; ratio, unscaled) plus registration, bases_used, scale = the returned pose's scale
    (sqrt |det| of its planar block) and scale_registration, as global_sim_icp reports them.  ValueError when no base
    has a hypothesis."""
    ctx = ctx or default_context()
    src, tgt = _points(centers), _points(truths)
    lo, hi = scale_range
    reg = ctx.register_sim(src, tgt, bases, float(lo), float(hi), inlier_dist, mirror, max_landmarks)
    used = np.flatnonzero(reg["score"] >= 0)
    if len(used) == 0:
        raise ValueError("no base has a target pair with a length ratio in scale_range")
    M = reg["M_all"][used]
    out = ctx.icp_sim(src, tgt, gates, ratio_range, np.ascontiguousarray(M[:, :3, :3]), np.ascontiguousarray(M[:, :3, 3]),
                      max_iter, max_landmarks, min_pairs, inlier_dist)
    out.update(registration=reg, bases_used=used, scale=_linear_scale(out["M"][:3, :3]),
               scale_registration=float(reg["scale"][used[out["best"]]]))
    return out


def _points(p):
    if isinstance(p, np.ndarray):
        return p
    return xyz_array(p)
