"""Least-squares sphere (3-D) or circle (2-D) per cluster and the rejection step built on it (vcp_cluster_spheres;
csrc/cluster_spheres.hip, csrc/spdsolve.hpp).

The instrument is the origin of X, Y, Z, so a target is seen from one side: the mean of a sphere target's returns lies about
2R/3 in front of its centre, and over a field these shifts are a radial shrink that no rigid fit absorbs.  The fit gives
the centre the returns lie around, with the radius free or fixed to the known target radius; its radius, residual and
coverage judge the cluster better than the circumscribed circle, which one stray return moves.  sphere_centres has the
shape `centroids` gives, so the matchers and the ICP forms take the fitted centres unchanged.

numpy arrays go through the host form; float64 / int32 torch tensors on the GPU go through the device-pointer form without
a copy (a view with a row stride is read in place), and the results are torch tensors on the same device."""
import numpy as np

from .moments import _dev_rows, _is_dev


class ClusterSpheres:
    """What cluster_spheres returns: centre [K, dim], radius, rms (of rho - radius), cap (|sum w nu| / W: about 0 for a
    whole sphere, 2/3 for a cap seen from afar, towards 1 for a sliver), step (|delta| of the last round) [K], alg
    [K, dim + 1] (the algebraic start: centre, radius), valid [K] uint8, counts [K] int64 (the total weight); numpy arrays
    or torch tensors, as the input was.  An invalid cluster has NaN in every float field."""

    FIELDS = ("centre", "radius", "rms", "cap", "step", "alg", "valid", "counts")

    def __init__(self, dim, K, fixed_radius, rounds, **arrays):
        self.dim, self.K, self.fixed_radius, self.rounds = int(dim), int(K), float(fixed_radius), int(rounds)
        for f in self.FIELDS:
            setattr(self, f, arrays[f])


def cluster_spheres(points, labels, K, weights=None, dim=None, radius=None, rounds=12, ctx=None):
    """Per cluster k = 1..K (labels[i] == k; 0 = in no cluster) the least-squares sphere (dim 3) or circle (dim 2) of
    points[i, :dim] (dim by default the width of points), weighted by the int32 weights where given.  radius=None fits
    the radius, a value > 0 fixes it to the known target radius; rounds Gauss-Newton rounds (0..64) follow the algebraic
    start.  points is a numpy array or a float64 torch tensor on the GPU; xyz[:, :2] or columns of a wider array are read
    in place.  Returns a ClusterSpheres."""
    from . import runtime
    ctx = ctx or runtime.default_context()
    K, fixed, rounds = int(K), 0.0 if radius is None else float(radius), int(rounds)
    if radius is not None and not fixed > 0.0:
        raise ValueError("radius must be None (fitted) or > 0")
    if _is_dev(points, labels, weights):
        import torch
        points, labels, weights, n, dim, ld = _dev_rows(points, labels, weights, dim)
        d, kk, dev = (dim if dim in (2, 3) else 3), max(K, 0), points.device
        z = lambda shape, dt=torch.float64: torch.empty(shape, dtype=dt, device=dev)
        out = dict(centre=z((kk, d)), radius=z(kk), rms=z(kk), cap=z(kk), step=z(kk), alg=z((kk, d + 1)),
                   valid=z(kk, torch.uint8), counts=z(kk, torch.int64))
        torch.cuda.current_stream(dev).synchronize()  # the library runs on the context's stream, not torch's
        ctx.cluster_spheres_dev(points.data_ptr(), ld, dim, labels.data_ptr(), None if weights is None else weights.data_ptr(),
                                n, K, fixed, rounds, out["centre"].data_ptr(), out["radius"].data_ptr(),
                                out["rms"].data_ptr(), out["cap"].data_ptr(), out["step"].data_ptr(), out["alg"].data_ptr(),
                                out["valid"].data_ptr(), out["counts"].data_ptr())
        return ClusterSpheres(d, kk, fixed, rounds, **out)
    points = np.asarray(points, np.float64)
    r = ctx.cluster_spheres(points, labels, K, weights, dim, fixed_radius=fixed, rounds=rounds)
    return ClusterSpheres(r["centre"].shape[1], max(K, 0), fixed, rounds, **r)


def sphere_centres(fit, fallback=None):
    """The fitted centres [K, dim] in the shape `centroids` gives (c3 for dim 3, c2 for dim 2): NaN rows for the clusters
    without a fit, as centroids has them for empty clusters, or the rows of `fallback` (the centroids, say) there."""
    c = fit.centre
    if fallback is None:
        return c.contiguous() if _is_dev(c) else np.ascontiguousarray(c)
    if _is_dev(c):
        import torch
        return torch.where((fit.valid != 0)[:, None], c, fallback).contiguous()
    return np.ascontiguousarray(np.where((fit.valid != 0)[:, None], c, np.asarray(fallback, np.float64)))


def filter_by_spheres(labels, fit, r_min=0.0, r_max=np.inf, max_rms=np.inf, max_cap=1.0, ctx=None, reject_invalid=True,
                      full=False):
    """The rejection step on the fit.  Cluster k is rejected when
        radius < r_min  or  radius > r_max  or  rms > max_rms  or  cap > max_cap          (valid fits; plain comparisons)
        or the cluster has members and no valid fit (too few, degenerate or non-finite), unless reject_invalid is False
    so a NaN threshold switches its criterion off.  The decision is K comparisons and is made on the host.  Returns the
    filterID list removeFilterPointFromClustering takes (cluster ids, position + 1).  With full=True: dict(filtered [K],
    keep [n], kept_idx [n_kept], n_filtered, n_kept) as Context.cluster_filter gives it, from one pass of that filter over
    the flags."""
    from . import runtime
    ctx = ctx or runtime.default_context()
    K = fit.K
    host = lambda a: a.cpu().numpy() if _is_dev(a) else np.asarray(a)
    radius, rms, cap, valid, counts = (host(getattr(fit, f)) for f in ("radius", "rms", "cap", "valid", "counts"))
    with np.errstate(invalid="ignore"):
        flag = (valid != 0) & ((radius < r_min) | (radius > r_max) | (rms > max_rms) | (cap > max_cap))
    if reject_invalid:
        flag |= (valid == 0) & (counts > 0)
    if not full:
        return [j + 1 for j in range(K) if flag[j]]
    score, one = flag.astype(np.float64), np.ones(K, np.uint8)
    if _is_dev(labels):
        import torch
        labels = labels.contiguous().reshape(-1)
        n, dev = labels.numel(), labels.device
        flt, keep = (torch.empty(m, dtype=torch.uint8, device=dev) for m in (K, n))
        idx = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
        d_score, d_one = torch.from_numpy(score).to(dev), torch.from_numpy(one).to(dev)
        torch.cuda.current_stream(dev).synchronize()
        nf, nk = ctx.cluster_filter_dev(labels.data_ptr(), n, K, d_score.data_ptr(), d_one.data_ptr(), None, None, 0.5,
                                        float("inf"), flt.data_ptr(), keep.data_ptr(), idx.data_ptr())
        return dict(filtered=flt, keep=keep, kept_idx=idx[:nk], n_filtered=nf, n_kept=nk)
    return ctx.cluster_filter(labels, K, score, one, None, None, 0.5, np.inf)
