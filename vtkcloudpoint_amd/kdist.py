"""k-distance graph for choosing DBSCAN's eps (Ester et al. 1996) over the C-ABI (vcp_kdist / vcp_kdist_dev).

The reference types eps by hand (0.07 / 7 in the Clustering dialog, 0.06 / 9 in the MATLAB one).  The standard aid is
the k-distance graph: for every point the distance to its k-th nearest neighbour with k = minPts, sorted; eps is read
off the knee.  kdist[i] is exact and counts the point itself, so for every finite eps

    DBImproved / vcp_dbscan(eps, minPts = k).is_core[i]  ==  (kdist[i] <= eps)

bit for bit: the fraction of core points at eps is the fraction of the curve at or below eps.
"""
import math

import numpy as np

from . import _native
from .datamodel import motor_array, xyz_array
from .runtime import default_context

_METRICS = {"L1_2D": _native.L1_2D, "L2_2D": _native.L2_2D, "L2_3D": _native.L2_3D}


def _metric(metric):
    if isinstance(metric, str):
        if metric not in _METRICS:
            raise ValueError("metric must be one of %s" % sorted(_METRICS))
        return _METRICS[metric]
    return int(metric)


def k_distance(points, k, metric="L1_2D", ctx=None):
    """Exact k-distance of every point; k = minPts, 1 <= k <= 64.

    points: a list of Point3D (motor_x / motor_y for the 2-D metrics, X / Y / Z for L2_3D, as DBImproved reads them),
    a numpy array [n, 2 or 3], or a float64 torch tensor on the GPU (run through vcp_kdist_dev without a host copy;
    the result is then a tensor on the same device).  Returns kdist [n]: NaN for a point with a non-finite coordinate,
    +inf for a finite point with fewer than k finite points in the cloud."""
    m = _metric(metric)
    ctx = ctx or default_context()
    try:
        import torch
    except ImportError:  # pragma: no cover
        torch = None
    if torch is not None and isinstance(points, torch.Tensor):
        if not points.is_cuda:
            points = points.numpy()
        else:
            t = points.to(torch.float64).contiguous()
            if t.dim() != 2 or t.shape[1] not in (2, 3):
                raise ValueError("points must be [n, 2] or [n, 3]")
            kd = torch.empty(t.shape[0], dtype=torch.float64, device=t.device)
            torch.cuda.synchronize(t.device)  # the library runs on its own stream
            ctx.kdist_dev(t.data_ptr(), t.shape[0], t.shape[1], k, kd.data_ptr(), metric=m)
            return kd
    if isinstance(points, (list, tuple)) and (len(points) == 0 or hasattr(points[0], "motor_x")):
        coords = xyz_array(points) if m == _native.L2_3D else motor_array(points)
    else:
        coords = np.asarray(points, np.float64)
    kd, _ = ctx.kdist(coords, k, m)
    return kd


def k_nearest(points, k, metric="L1_2D", ctx=None):
    """(kdist [n], knn [n, k]) for a numpy array: row i = the k nearest indices by (distance, index), ascending."""
    ctx = ctx or default_context()
    return ctx.kdist(np.asarray(points, np.float64), k, _metric(metric), want_knn=True)


def k_distance_curve(kd):
    """The k-distance graph: the finite values of kd, sorted ascending (numpy array)."""
    if hasattr(kd, "detach"):
        kd = kd.detach().cpu().numpy()
    kd = np.asarray(kd, np.float64).ravel()
    return np.sort(kd[np.isfinite(kd)])


def eps_from_curve(curve, top_quantile=0.99):
    """Knee of a sorted k-distance curve (the rule suggest_eps applies; a heuristic, not a guarantee).

    1. The curve's values above its top_quantile entry (index ceil(top_quantile * (m - 1))) are dropped, so that a few
       far outliers do not flatten the rest of the curve.
    2. The kept part, m' values, is mapped onto [0, 1]^2: x_i = i / (m' - 1), y_i = (v_i - v_0) / (v_last - v_0).
    3. The answer is v_i at the first i that maximises x_i - y_i: the point farthest below the chord, where the curve
       turns from the dense points' flat part into the steep part of the sparse ones.
    A constant curve (or a single value) gives that value; an empty curve gives NaN.  Deterministic."""
    v = k_distance_curve(curve)
    if v.size == 0:
        return float("nan")
    q = min(max(float(top_quantile), 0.0), 1.0)
    v = v[: int(math.ceil(q * (v.size - 1))) + 1]
    lo, hi = v[0], v[-1]
    if v.size == 1 or not hi > lo:
        return float(lo)
    x = np.arange(v.size, dtype=np.float64) / (v.size - 1)
    y = (v - lo) / (hi - lo)
    return float(v[int(np.argmax(x - y))])


def suggest_eps(points, min_pts, metric="L1_2D", ctx=None, top_quantile=0.99, kd=None):
    """A suggested DBSCAN eps for minPts = min_pts: the knee of the k-distance curve (eps_from_curve).

    HEURISTIC: it finds where the sorted k-distances turn steeply upward, which separates dense clusters from a
    sparse background when the cloud has both; it knows nothing about the clusters the caller wants.  Points within
    the returned eps of at least min_pts points (themselves included) are core points.  kd: an already computed
    k_distance(points, min_pts, metric) (points is then not read)."""
    if kd is None:
        kd = k_distance(points, min_pts, metric, ctx)
    return eps_from_curve(kd, top_quantile)
