"""Order statistics per cluster or group, and outlier rejection by the median absolute deviation (vcp_cluster_quantiles,
vcp_cluster_mad; csrc/cluster_quant.hip).

The reference rejects the outliers of its fixed-point files with one band of Distance for all files, typed by hand
(SureDistanceFilter.cs:26-61, Tools.FilterByDistance_FixedPoint, BaseClass/Tools.cs:438-461), seeded by the min / max of
Tools.GetGroupingManOrMin (:468-497).  Here every group gets its own minimum, maximum and median, and a band of its own:
|v - median| <= max(c * MAD, floor).

numpy arrays go through the host forms; float64 / int32 torch tensors on the GPU go through the device-pointer forms
without a copy, and the results are torch tensors on the same device."""
import numpy as np


def _is_dev(*arrays):
    try:
        import torch
    except Exception:
        return False
    return any(torch.is_tensor(a) for a in arrays)


def _dev_args(values, labels):
    """(values float64 tensor, stride, labels int32 tensor, n): a column view of a contiguous [n, d] tensor is read in
    place (stride d), anything else is made contiguous."""
    import torch
    if not torch.is_tensor(values) or not torch.is_tensor(labels):
        raise ValueError("values and labels must both be torch tensors on the GPU, or both numpy arrays")
    if values.dtype != torch.float64 or not values.is_cuda:
        raise ValueError("values must be a float64 tensor on the GPU (or a numpy array)")
    if labels.dtype != torch.int32 or not labels.is_cuda:
        raise ValueError("labels must be an int32 tensor on the GPU (or a numpy array)")
    labels = labels.contiguous().reshape(-1)
    n = labels.numel()
    if values.dim() != 1:
        values = values.reshape(-1)
    if values.numel() != n:
        raise ValueError("values has %d entries for %d labels" % (values.numel(), n))
    stride = int(values.stride(0)) if n > 1 else 1
    if stride < 1:
        values, stride = values.contiguous(), 1
    return values, stride, labels, n


def cluster_quantiles(values, labels, K, q, ctx=None):
    """Per group k = 1..K (labels[i] == k; 0 = in no group) the value of rank floor(q * (c - 1)) among its c values in
    numeric order (-0 before +0, NaN last): q = 0 the minimum, 0.5 the lower median, 1 the maximum.  Returns (out [K, nq],
    counts [K] int64); an empty group is a NaN row with count 0.  values may be a strided 1-D view (a column of xyz)."""
    from . import runtime
    q = np.ascontiguousarray(q, np.float64).reshape(-1)
    if _is_dev(values, labels):
        import torch
        values, stride, labels, n = _dev_args(values, labels)
        ctx = ctx or runtime.default_context()
        out = torch.empty((max(int(K), 0), len(q)), dtype=torch.float64, device=values.device)
        counts = torch.empty(max(int(K), 0), dtype=torch.int64, device=values.device)
        torch.cuda.current_stream(values.device).synchronize()  # the library runs on the context's stream, not torch's
        ctx.cluster_quantiles_dev(values.data_ptr(), stride, labels.data_ptr(), n, int(K), q, out.data_ptr(),
                                  counts.data_ptr())
        return out, counts
    ctx = ctx or runtime.default_context()
    values = np.asarray(values, np.float64)
    if values.ndim != 1:
        values = values.reshape(-1)
    return ctx.cluster_quantiles(np.ascontiguousarray(values), labels, int(K), q)


def cluster_medians(xyz, labels, K, ctx=None):
    """The coordinate-wise lower median [K, 3] of every cluster: three calls, each reading its column of xyz in place."""
    if _is_dev(xyz, labels):
        import torch
        xyz = xyz.contiguous().reshape(-1, 3)
        return torch.cat([cluster_quantiles(xyz[:, a], labels, K, [0.5], ctx)[0] for a in range(3)], dim=1)
    from . import runtime
    ctx = ctx or runtime.default_context()
    xyz = np.ascontiguousarray(xyz, np.float64).reshape(-1, 3)
    flat = xyz.reshape(-1)
    return np.concatenate([ctx.cluster_quantiles(flat[a:], labels, int(K), [0.5], stride=3)[0] for a in range(3)], axis=1)


def cluster_mad(values, labels, K, c=3.0, floor=0.0, ctx=None):
    """Per group the lower median med, the median absolute deviation mad from it, and thr = max(c * mad, floor); a row of a
    group is rejected unless |v - med| <= thr (so a NaN is rejected).  Returns dict(med, mad, thr [K], reject [n] uint8,
    kept [K] int64, n_rejected)."""
    from . import runtime
    if _is_dev(values, labels):
        import torch
        values, stride, labels, n = _dev_args(values, labels)
        ctx = ctx or runtime.default_context()
        kk, dev = max(int(K), 0), values.device
        med, mad, thr = (torch.empty(kk, dtype=torch.float64, device=dev) for _ in range(3))
        reject = torch.empty(n, dtype=torch.uint8, device=dev)
        kept = torch.empty(kk, dtype=torch.int64, device=dev)
        torch.cuda.current_stream(dev).synchronize()
        nr = ctx.cluster_mad_dev(values.data_ptr(), stride, labels.data_ptr(), n, int(K), float(c), float(floor),
                                 med.data_ptr(), mad.data_ptr(), thr.data_ptr(), reject.data_ptr(), kept.data_ptr())
        return dict(med=med, mad=mad, thr=thr, reject=reject, kept=kept, n_rejected=nr)
    ctx = ctx or runtime.default_context()
    return ctx.cluster_mad(np.ascontiguousarray(values, np.float64).reshape(-1), labels, int(K), float(c), float(floor))


def robust_fixed_centroids(fixed, c=3.0, floor=0.0, ignore_duplication=False, ctx=None):
    """The fixed-point workflow with a band per file: `fixed` is what io.add_fixed_folder returns (or its clusList).  MAD
    rejection on Distance per file, the rejected points marked isFilterByDistance and put in group 0, then
    Tools.getFixedPtsCentroid (vcp_centroids_weighted) on the rest.  Returns (c3 [K, 3], inside_num [K], mad: the dict of
    cluster_mad over the points in list order)."""
    from . import runtime
    ctx = ctx or runtime.default_context()
    clusList = fixed[0] if isinstance(fixed, tuple) else fixed
    K = len(clusList)
    pts = [(k, p) for k, ob in enumerate(clusList) for p in ob.li]
    n = len(pts)
    xyz = np.array([(p.X, p.Y, p.Z) for _, p in pts], np.float64).reshape(n, 3)
    dist = np.array([p.Distance for _, p in pts], np.float64)
    group = np.array([k + 1 for k, _ in pts], np.int32)
    cid = np.array([p.clusterId for _, p in pts], np.int32)
    cnt = np.array([p.ptsCount for _, p in pts], np.int32)
    mad = cluster_mad(dist, group, K, c, floor, ctx)
    for (_, p), r in zip(pts, mad["reject"]):
        p.isFilterByDistance = bool(r)
    c3, inside = ctx.centroids_weighted(xyz, np.where(mad["reject"] != 0, 0, group).astype(np.int32), cid, cnt, K,
                                        ignore_duplication)
    return c3, inside, mad
