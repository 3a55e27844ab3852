"""The local surface at every return (include/vcp_features.h; csrc/point_features.hip): the normal, the eigenvalues and
the surface variation of the covariance of the k nearest neighbours, and the mean distance to them.

Three steps in front of the clustering use them.  sor_keep is statistical outlier removal: a return whose neighbours are
far away is noise, and the band comes from the cloud's own median and MAD of the mean neighbour distance.  The surface
variation lambda_min / sum(lambda) tells a curved target from a flat facet, per row and so before vcp_dbscan.  With
normals oriented towards the instrument and a known target radius R, centre_votes gives p - R n: one vote for the
sphere's centre per return, which fall into a blob a few millimetres wide per target.

The neighbour rows are vcp_kdist's knn (ascending (distance, index): a pinned order, so every sum is pinned) unless the
caller brings its own.  numpy arrays go through the host forms; float64 torch tensors on the GPU go through the
device-pointer forms without a copy (a view with a row stride, such as the resident import's xyz, is read in place), and
the results are torch tensors on the same device.

The ctypes prototypes of vcp_features.h live here, on the library _native loads (SYMBOLS lists them)."""
import ctypes as C
from collections import namedtuple

import numpy as np

from . import _native
from .moments import _is_dev

# every symbol include/vcp_features.h declares (tests/test_point_features.py checks that the library exports all of them)
SYMBOLS = ["vcp_point_features_shape", "vcp_point_features", "vcp_point_features_dev"]

MAX_K = 64

_P, _I32, _I64 = C.c_void_p, C.c_int, C.c_int64
_PROTOTYPES = {
    "vcp_point_features_shape": [_P, _P],
    "vcp_point_features": [_P, _P, _I64, _I32, _I64, _P, _I32, _P, _P, _P, _P, _P, _P, _P],
    "vcp_point_features_dev": [_P, _P, _I64, _I32, _I64, _P, _I32, _P, _P, _P, _P, _P, _P, _P],
}
_bound = None


def _L():
    """libvcp.so with the prototypes of vcp_features.h set.  A library without them is an error (no fallback)."""
    global _bound
    if _bound is None:
        lib = _native.lib()
        for name, args in _PROTOTYPES.items():
            fn = getattr(lib, name)
            fn.argtypes, fn.restype = args, C.c_int
        _bound = lib
    return _bound


def _p(a):
    """The address of a numpy array, a torch tensor or an int, or None."""
    if a is None:
        return None
    if isinstance(a, int):
        return a
    if isinstance(a, np.ndarray):
        return a.ctypes.data
    return a.data_ptr()


def _ctx(ctx):
    from . import runtime
    return ctx or runtime.default_context()


def _sync(dev):
    import torch
    torch.cuda.current_stream(dev).synchronize()  # the library runs on the context's stream, not torch's


PointFeatures = namedtuple("PointFeatures", "normal eval variation mean_dist count valid knn")
PointFeatures.__doc__ = """What point_features returns: normal [n, d] (unit, the axis of the smallest eigenvalue, towards the
viewpoint where one was given), eval [n, d] (descending), variation [n] (eval[d - 1] / sum(eval)), mean_dist [n] (to the
neighbours other than the row itself), count [n] int32 (the members of the row's list), valid [n] uint8 (count >= d and a
finite mean and covariance), knn [n, k] int32 (the neighbour rows used); numpy arrays or torch tensors, as the input was."""


def _viewpoint(viewpoint, dim):
    if viewpoint is None:
        return None
    vp = np.ascontiguousarray(np.asarray(viewpoint, np.float64).reshape(-1)[:dim])
    if len(vp) != dim:
        raise ValueError("viewpoint must hold %d numbers" % dim)
    return vp


def point_features(points, k=16, neighbours=None, viewpoint=(0.0, 0.0, 0.0), ctx=None):
    """vcp_point_features over the k nearest neighbours of every row of points [n, 2 or 3].

    neighbours: None (vcp_kdist finds them: L2_3D for three columns, L2_2D for two; the row itself is among them unless k
    or more lower-indexed duplicates of it exist) or [n, k] int32 rows of the caller's, where any value outside [0, n)
    is a skipped slot; then nothing but the feature pass runs.  viewpoint: where the instrument stood (the normals are
    turned towards it), or None to leave the sign to the eigen-solve's rule.  Returns a PointFeatures."""
    ctx = _ctx(ctx)
    if _is_dev(points):
        import torch
        if not torch.is_tensor(points) or points.dtype != torch.float64 or not points.is_cuda or points.dim() != 2 \
                or points.shape[1] not in (2, 3):
            raise ValueError("points must be a float64 [n, 2 or 3] tensor on the GPU (or a numpy array)")
        n, dim = points.shape
        if n > 1 and not (points.stride(1) == 1 and points.stride(0) >= dim):
            points = points.contiguous()
        ld = int(points.stride(0)) if n > 1 else dim
        dev = points.device
        if neighbours is None:
            k = int(k)
            dense = points.contiguous()                      # vcp_kdist reads point-major rows: for this call only
            kd = torch.empty(n, dtype=torch.float64, device=dev)
            knn = torch.empty((n, max(k, 0)), dtype=torch.int32, device=dev)
            _sync(dev)
            ctx.kdist_dev(dense.data_ptr(), n, dim, k, kd.data_ptr(), knn.data_ptr(),
                          metric=_native.L2_3D if dim == 3 else _native.L2_2D)
        else:
            knn = neighbours if torch.is_tensor(neighbours) else torch.from_numpy(np.ascontiguousarray(neighbours, np.int32))
            knn = knn.to(device=dev, dtype=torch.int32).contiguous()
            if knn.dim() != 2 or knn.shape[0] != n:
                raise ValueError("neighbours must be [n, k]")
            k = knn.shape[1]
        vp = _viewpoint(viewpoint, dim)
        f64 = dict(dtype=torch.float64, device=dev)
        out = PointFeatures(torch.empty((n, dim), **f64), torch.empty((n, dim), **f64), torch.empty(n, **f64),
                            torch.empty(n, **f64), torch.empty(n, dtype=torch.int32, device=dev),
                            torch.empty(n, dtype=torch.uint8, device=dev), knn)
        _sync(dev)
        ctx._chk(_L().vcp_point_features_dev(ctx._h, _p(points), _I64(ld), dim, _I64(n), _p(knn), int(k), _p(vp),
                                             _p(out.normal), _p(out.eval), _p(out.variation), _p(out.mean_dist),
                                             _p(out.count), _p(out.valid)))
        return out
    points = np.asarray(points, np.float64)
    if points.ndim != 2 or points.shape[1] not in (2, 3):
        raise ValueError("points must be [n, 2] or [n, 3]")
    n, dim = points.shape
    if n <= 1 or not (points.strides[1] == 8 and points.strides[0] % 8 == 0 and points.strides[0] >= 8 * dim):
        points = np.ascontiguousarray(points)
    ld = points.strides[0] // 8 if n > 1 else dim
    if neighbours is None:
        k = int(k)
        _, knn = ctx.kdist(np.ascontiguousarray(points), k, _native.L2_3D if dim == 3 else _native.L2_2D, want_knn=True)
    else:
        knn = np.ascontiguousarray(neighbours, np.int32)
        if knn.ndim != 2 or knn.shape[0] != n:
            raise ValueError("neighbours must be [n, k]")
        k = knn.shape[1]
    vp = _viewpoint(viewpoint, dim)
    out = PointFeatures(np.zeros((n, dim)), np.zeros((n, dim)), np.zeros(n), np.zeros(n), np.zeros(n, np.int32),
                        np.zeros(n, np.uint8), knn)
    ctx._chk(_L().vcp_point_features(ctx._h, _p(points), _I64(ld), dim, _I64(n), _p(knn), int(k), _p(vp), _p(out.normal),
                                     _p(out.eval), _p(out.variation), _p(out.mean_dist), _p(out.count), _p(out.valid)))
    return out


def point_features_shape(ctx=None):
    """vcp_point_features_shape: (rows per workgroup, largest grid, the k classes of the kernel) on the context's device."""
    ctx = _ctx(ctx)
    shape = np.zeros(6, np.int32)
    ctx._chk(_L().vcp_point_features_shape(ctx._h, _p(shape)))
    return int(shape[0]), int(shape[1]), tuple(int(v) for v in shape[2:])


def sor_keep(mean_dist, c=6.0, floor=0.0, ctx=None):
    """Statistical outlier removal on the mean neighbour distance: (keep, median, mad).  median is the lower median of the
    finite entries of mean_dist, mad the lower median of |v - median| over them (robust.cluster_quantiles with one group),
    keep = mean_dist <= median + max(c * mad, floor), False for NaN.  One-sided on purpose: a dense row is not an outlier.
    Every step is a selection or one rounding, so the device and the host agree bit for bit."""
    from .robust import cluster_quantiles
    if _is_dev(mean_dist):
        import torch
        v = mean_dist.reshape(-1)
        group = torch.isfinite(v).to(torch.int32)
        absf = torch.abs
    else:
        v = np.asarray(mean_dist, np.float64).reshape(-1)
        group = np.isfinite(v).astype(np.int32)
        absf = np.abs
    median = float(cluster_quantiles(v, group, 1, [0.5], ctx)[0][0, 0])
    mad = float(cluster_quantiles(absf(v - median), group, 1, [0.5], ctx)[0][0, 0])
    keep = v <= median + max(float(c) * mad, float(floor))
    return keep, median, mad


def centre_votes(points, normal, radius, valid=None):
    """p - radius * n per row (each operation rounded on its own), in numpy or torch: with normals oriented towards the
    instrument, the vote of every return for the centre of a sphere of that radius.  normal: [n, d], or a PointFeatures
    (its valid is then used); rows with valid == 0 give NaN."""
    if isinstance(normal, PointFeatures):
        normal, valid = normal.normal, normal.valid if valid is None else valid
    votes = points[:, :normal.shape[1]] - float(radius) * normal
    if valid is not None:
        if _is_dev(votes):
            import torch
            votes = torch.where((valid != 0).reshape(-1, 1), votes, torch.full_like(votes, float("nan")))
        else:
            votes = np.where((np.asarray(valid) != 0).reshape(-1, 1), votes, np.nan)
    return votes
