"""Second central moments per cluster and the ellipse filter built on them (vcp_cluster_moments;
csrc/cluster_moments.hip, csrc/symeig.hpp).

The reference rejects clusters "based on cluster radius and length/width ratio" (its README) from the circumscribed circle
and rectangle, which vcp_cluster_shapes computes: extreme values, moved by one stray return by its full distance, undefined
below four points and beyond 2048 hull points, and 2-D only.  Here every cluster of two or more points gets its mean, its
covariance, the principal axes and eigenvalues, and from them the ellipse 2 sqrt(lambda) (a uniformly filled disc of
radius r has variance r^2 / 4 on every axis, so 2 sigma = r), and in 3-D the surface normal and a flatness measure.
ellipse_radius / ellipse_sides are the arrays vcp_cluster_filter takes as radius / rect_len, so the existing filter judges
them unchanged.

numpy arrays go through the host form; float64 / int32 torch tensors on the GPU go through the device-pointer form without
a copy (a view with a row stride is read in place), and the results are torch tensors on the same device."""
import numpy as np


def _is_dev(*arrays):
    try:
        import torch
    except Exception:
        return False
    return any(torch.is_tensor(a) for a in arrays)


def _dev_rows(points, labels, weights, dim):
    """The (points, labels, weights, n, dim, ld) of the device-pointer forms from torch tensors on the GPU: checked, the
    labels and weights flat, the rows read in place at their stride where the columns are contiguous (else copied)."""
    import torch
    if not (torch.is_tensor(points) and torch.is_tensor(labels) and (weights is None or torch.is_tensor(weights))):
        raise ValueError("points, labels and weights must all be torch tensors on the GPU, or all numpy arrays")
    if points.dtype != torch.float64 or not points.is_cuda or points.dim() != 2:
        raise ValueError("points must be a float64 [n, c] tensor on the GPU (or a numpy array)")
    if labels.dtype != torch.int32 or not labels.is_cuda:
        raise ValueError("labels must be an int32 tensor on the GPU (or a numpy array)")
    if weights is not None and (weights.dtype != torch.int32 or not weights.is_cuda):
        raise ValueError("weights must be an int32 tensor on the GPU (or a numpy array)")
    labels = labels.contiguous().reshape(-1)
    weights = None if weights is None else weights.contiguous().reshape(-1)
    n = labels.numel()
    if points.shape[0] != n or (weights is not None and weights.numel() != n):
        raise ValueError("points, labels and weights disagree on n")
    dim = points.shape[1] if dim is None else int(dim)
    if n > 1 and not (points.stride(1) == 1 and points.stride(0) >= max(dim, 1)):
        points = points.contiguous()
    ld = int(points.stride(0)) if n > 1 else max(points.shape[1], dim)
    return points, labels, weights, n, dim, ld


class ClusterMoments:
    """What cluster_moments returns: mean [K, dim], cov [K, dim (dim + 1) / 2] (xx, xy, (xz,) yy, (yz, zz)), eval [K, dim]
    descending, evec [K, dim, dim] (eigenvector j of cluster k is evec[k, j]), shape [K, 4] = (sigma_max,
    sigma_min_inplane, flatness, tilt), valid [K] uint8, counts [K] int64 (the total weight); numpy arrays or torch
    tensors, as the input was."""

    FIELDS = ("mean", "cov", "eval", "evec", "shape", "valid", "counts")

    def __init__(self, dim, K, **arrays):
        self.dim, self.K = int(dim), int(K)
        for f in self.FIELDS:
            setattr(self, f, arrays[f])

    @property
    def sigma(self):
        return self.shape[:, :2]

    @property
    def flatness(self):
        return self.shape[:, 2]

    @property
    def tilt(self):
        return self.shape[:, 3]

    @property
    def normal(self):
        """The axis of the smallest eigenvalue [K, dim]: in 3-D the surface normal of a flat cluster."""
        return self.evec[:, self.dim - 1]


def cluster_moments(points, labels, K, weights=None, dim=None, ctx=None):
    """Per cluster k = 1..K (labels[i] == k; 0 = in no cluster) the moments of points[i, :dim] (dim = 2 or 3, by default the
    width of points), weighted by the int32 weights where given (the `count` of a deduplicated import: the moments are then
    those of the raw scan).  points is a numpy array or a float64 torch tensor on the GPU; xyz[:, :2] or columns of a wider
    array are read in place.  Returns a ClusterMoments."""
    from . import runtime
    ctx = ctx or runtime.default_context()
    K = int(K)
    if _is_dev(points, labels, weights):
        import torch
        points, labels, weights, n, dim, ld = _dev_rows(points, labels, weights, dim)
        d, kk, dev = (dim if dim in (2, 3) else 3), max(K, 0), points.device
        z = lambda shape, dt=torch.float64: torch.empty(shape, dtype=dt, device=dev)
        out = dict(mean=z((kk, d)), cov=z((kk, d * (d + 1) // 2)), eval=z((kk, d)), evec=z((kk, d, d)), shape=z((kk, 4)),
                   valid=z(kk, torch.uint8), counts=z(kk, torch.int64))
        torch.cuda.current_stream(dev).synchronize()  # the library runs on the context's stream, not torch's
        ctx.cluster_moments_dev(points.data_ptr(), ld, dim, labels.data_ptr(), None if weights is None else weights.data_ptr(),
                                n, K, *(out[f].data_ptr() for f in ClusterMoments.FIELDS))
        return ClusterMoments(d, kk, **out)
    points = np.asarray(points, np.float64)
    r = ctx.cluster_moments(points, labels, K, weights, dim)
    return ClusterMoments(r["mean"].shape[1], max(K, 0), **r)


def ellipse_radius(mom):
    """2 sigma_max [K]: the radius of the uniformly filled disc with the cluster's largest variance (a disc of radius r has
    variance r^2 / 4 on every axis).  What vcp_cluster_filter takes as `radius`."""
    return 2.0 * mom.shape[:, 0]


def ellipse_sides(mom):
    """(2 sigma_max, 2 sigma_min_inplane) [K, 2]: the semi-axes of the uniformly filled ellipse with the cluster's two
    largest variances; their ratio is the aspect.  What vcp_cluster_filter takes as `rect_len`."""
    s = 2.0 * mom.shape[:, :2]
    return s.contiguous() if _is_dev(s) else np.ascontiguousarray(s)


def filter_by_moments(labels, mom, max_radius=np.inf, max_aspect=np.inf, max_flatness=np.inf, min_tilt=0.0, ctx=None,
                      full=False):
    """The radius / aspect filter on the moment ellipse, with two 3-D criteria beside it.  Cluster k (valid ones only) is
    filtered when
        ellipse_radius > max_radius  or  2 sigma_max > max_aspect * 2 sigma_min_inplane      (vcp_cluster_filter, unchanged)
        or  flatness > max_flatness  or  tilt < min_tilt                                      (plain comparisons, [K])
    so a NaN or infinite threshold (and min_tilt = 0) switches its criterion off.  Returns what tools.filterClusters
    returns: the filterID list (cluster ids, position + 1).  With full=True: dict(filtered [K], keep [n], kept_idx
    [n_kept], n_filtered, n_kept) as Context.cluster_filter gives it; where a 3-D criterion flags a cluster the radius /
    aspect filter missed, keep and kept_idx come from a second pass of the same filter over the combined flags."""
    from . import runtime
    ctx = ctx or runtime.default_context()
    K = mom.K
    radius, sides, valid = ellipse_radius(mom), ellipse_sides(mom), mom.valid
    f3 = (mom.valid != 0) & ((mom.flatness > max_flatness) | (mom.tilt < min_tilt))
    if _is_dev(labels, radius):
        import torch
        labels = labels.contiguous().reshape(-1)
        n, dev = labels.numel(), labels.device
        flt, keep = (torch.empty(m, dtype=torch.uint8, device=dev) for m in (K, n))
        idx = torch.empty(max(n, 1), dtype=torch.int32, device=dev)

        def run(rad, val, rl, rv, mr, ma):
            torch.cuda.current_stream(dev).synchronize()
            nf, nk = ctx.cluster_filter_dev(labels.data_ptr(), n, K, rad.data_ptr(), val.data_ptr(),
                                            None if rl is None else rl.data_ptr(), None if rv is None else rv.data_ptr(),
                                            float(mr), float(ma), flt.data_ptr(), keep.data_ptr(), idx.data_ptr())
            return dict(filtered=flt.clone(), keep=keep, kept_idx=idx[:nk], n_filtered=nf, n_kept=nk)

        r = run(radius.contiguous(), valid, sides, valid, max_radius, max_aspect)
        both = (r["filtered"] != 0) | f3
        if bool((both != (r["filtered"] != 0)).any()):
            one = torch.ones(K, dtype=torch.uint8, device=dev)
            r = run(both.to(torch.float64), one, None, None, 0.5, np.inf)
        filtered = r["filtered"].cpu().numpy()
    else:
        r = ctx.cluster_filter(labels, K, radius, valid, sides, valid, max_radius, max_aspect)
        both = (r["filtered"] != 0) | f3
        if (both != (r["filtered"] != 0)).any():
            r = ctx.cluster_filter(labels, K, both.astype(np.float64), np.ones(K, np.uint8), None, None, 0.5, np.inf)
        filtered = r["filtered"]
    if full:
        return r
    return [j + 1 for j in range(K) if filtered[j]]
