"""DBSCAN's cluster count at every eps in one call (vcp_eps_tree / vcp_eps_tree_dev): eps from the number of targets.

suggest_eps reads eps off the knee of the k-distance curve and knows nothing about the clusters the caller wants.  A
caller who knows how many targets the scan holds wants an eps at which DBSCAN finds about that many clusters, and
preferably a wide range of such eps.  For a fixed minPts = k everything DBSCAN decides at every eps <= eps_max follows
from three arrays, all selections among the binary64 values vcp_kdist defines:

    point i is core at eps            <=>  kdist[i] <= eps
    core points i, j are linked       <=>  max(kdist[i], kdist[j], d(i, j)) <= eps      (the weight w)
    point i carries a label at eps    <=>  reach[i] <= eps,  reach[i] = min over core j of max(kdist[j], d(i, j))

so with the minimum spanning forest of w (merge_w, sorted)

    clusters(eps) = #{kdist <= eps} - #{merge_w <= eps}

exactly what vcp_dbscan(eps, min_pts = k).cf_out is, for every eps in [0, eps_max].
"""
import numpy as np

from . import _native
from .datamodel import motor_array, xyz_array
from .kdist import _metric, suggest_eps
from .runtime import default_context


class EpsTree:
    """Result of eps_tree: kdist [n], reach [n], the forest merge_w / merge_a / merge_b [m] in ascending (w, a, b) order,
    eps_max, min_pts and rounds (device rounds that accepted an edge)."""

    def __init__(self, kdist, reach, merge_w, merge_a, merge_b, eps_max, min_pts=None, rounds=0):
        self.kdist = np.asarray(kdist, np.float64)
        self.reach = np.asarray(reach, np.float64)
        self.merge_w = np.asarray(merge_w, np.float64)
        self.merge_a = None if merge_a is None else np.asarray(merge_a, np.int32)
        self.merge_b = None if merge_b is None else np.asarray(merge_b, np.int32)
        self.eps_max = float(eps_max)
        self.min_pts = min_pts
        self.rounds = int(rounds)
        kd = self.kdist[self.kdist <= self.eps_max]
        self._kd_sorted = np.sort(kd)
        self._reach_sorted = np.sort(self.reach[self.reach <= self.eps_max])


def eps_tree(points, min_pts, eps_max=None, metric="L1_2D", ctx=None, kd=None):
    """The eps tree of a cloud for minPts = min_pts (1 <= min_pts <= 64), as an EpsTree.

    points: what k_distance accepts -- a list of Point3D (motor_x / motor_y for the 2-D metrics, X / Y / Z for L2_3D), a
    numpy array [n, 2 or 3], or a torch tensor (copied to the host; the device-pointer form is Context.eps_tree_dev).
    kd: an already computed k_distance(points, min_pts, metric); it is passed on as given.
    eps_max: the largest eps the tree answers for; the cost grows with the number of points within eps_max of a point.
    None means 2 * suggest_eps(...), with that k-distance passed on.  HEURISTIC: twice the knee is usually beyond every
    eps worth trying, but nothing guarantees that the wanted cluster count occurs below it -- pass eps_max to be sure."""
    m = _metric(metric)
    ctx = ctx or default_context()
    if hasattr(points, "detach"):
        points = points.detach().cpu().numpy()
    if isinstance(points, (list, tuple)) and (len(points) == 0 or hasattr(points[0], "motor_x")):
        coords = xyz_array(points) if m == _native.L2_3D else motor_array(points)
    else:
        coords = np.asarray(points, np.float64)
    if kd is not None and hasattr(kd, "detach"):
        kd = kd.detach().cpu().numpy()
    if eps_max is None:
        if kd is None:
            kd, _ = ctx.kdist(coords, min_pts, m)
        eps_max = 2.0 * suggest_eps(None, min_pts, kd=kd)
        if not (np.isfinite(eps_max) and eps_max > 0.0):
            raise ValueError("no eps_max from the k-distance curve (knee %r): pass eps_max" % (eps_max / 2.0,))
    r = ctx.eps_tree(coords, min_pts, float(eps_max), m, kdist=kd)
    return EpsTree(r["kdist"], r["reach"], r["merge_w"], r["merge_a"], r["merge_b"], eps_max, int(min_pts), r["rounds"])


def _eps_array(tree, eps):
    e = np.asarray(eps, np.float64)
    if np.any(np.isnan(e)) or np.any(e > tree.eps_max):
        raise ValueError("eps beyond the tree's eps_max %r" % tree.eps_max)
    return e


def counts_at(tree, eps):
    """(cores, clusters, labelled) at eps -- scalars for a scalar eps, int64 arrays for an array -- as
    vcp_dbscan(eps, min_pts) gives them: sum(is_core), cf_out, #{labels != 0}.  Raises ValueError for eps > eps_max."""
    e = _eps_array(tree, eps)
    cores = np.searchsorted(tree._kd_sorted, e, side="right")
    merges = np.searchsorted(tree.merge_w, e, side="right")
    labelled = np.searchsorted(tree._reach_sorted, e, side="right")
    out = (cores, cores - merges, labelled)
    if e.ndim == 0:
        return tuple(int(v) for v in out)
    return tuple(np.asarray(v, np.int64) for v in out)


def cluster_count_steps(tree):
    """(breaks, clusters): the cluster count is clusters[i] for breaks[i] <= eps < breaks[i + 1], the last step runs to
    eps_max inclusive.  breaks starts at 0.0 and holds, ascending, every value at which a point turns core or two
    clusters merge."""
    breaks = np.unique(np.concatenate([[0.0], tree._kd_sorted, tree.merge_w]))
    return breaks, counts_at(tree, breaks)[1]


def eps_for_clusters(tree, target, tol=0):
    """The maximal intervals [lo, hi) of eps inside [0, eps_max] on which |clusters(eps) - target| <= tol, as a list of
    (lo, hi) floats, widest first, ties to the lower lo; empty when the count never comes that close.  An interval that
    reaches the end of the tree has hi = eps_max, and eps_max itself belongs to it.  Any eps of an interval gives
    vcp_dbscan that many clusters; the middle of the widest one is the choice least sensitive to eps."""
    breaks, clusters = cluster_count_steps(tree)
    ok = np.abs(clusters - int(target)) <= tol
    ends = np.append(breaks[1:], tree.eps_max)
    out, i, n = [], 0, len(breaks)
    while i < n:
        if not ok[i]:
            i += 1
            continue
        j = i
        while j + 1 < n and ok[j + 1]:
            j += 1
        out.append((float(breaks[i]), float(ends[j])))
        i = j + 1
    out.sort(key=lambda iv: (-(iv[1] - iv[0]), iv[0]))
    return out


def core_labels_at(tree, eps):
    """int32 [n]: the labels vcp_dbscan(eps, min_pts) gives the core points (clusters numbered 1, 2, ... by increasing
    smallest member index), 0 for every other point -- border points included: their label needs vcp_dbscan itself."""
    e = float(_eps_array(tree, eps))
    if tree.merge_a is None:
        raise ValueError("the tree was computed without its edges")
    n = len(tree.kdist)
    parent = np.arange(n)

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    m = int(np.searchsorted(tree.merge_w, e, side="right"))
    for a, b in zip(tree.merge_a[:m].tolist(), tree.merge_b[:m].tolist()):
        ra, rb = find(a), find(b)
        if ra != rb:  # the smaller index stays the root: a root is its component's smallest member
            parent[max(ra, rb)] = min(ra, rb)
    labels = np.zeros(n, np.int32)
    core = np.nonzero(tree.kdist <= e)[0]
    if core.size:
        roots = np.array([find(int(i)) for i in core])
        _, inv = np.unique(roots, return_inverse=True)
        labels[core] = inv + 1
    return labels
