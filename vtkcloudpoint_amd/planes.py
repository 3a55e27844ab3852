"""Plane extraction by consensus on the device (include/vcp_planes.h; csrc/planes.hip).

Most returns of a scan that are not targets lie on a few large planes: the floor, the walls behind the targets.  Left in
the cloud they become giant DBSCAN clusters.  extract_planes finds the dominant planes by RANSAC (H triples per round,
each triple's plane scored against every remaining row, the best refitted by least squares through vcp_cluster_moments,
its rows labelled and removed) and remove_planes gives what is left for dbscan.

numpy arrays go through the host forms; float64 torch tensors on the GPU go through the device-pointer forms without a
copy (a view with a row stride, such as the resident import's xyz or columns of a wider tensor, is read in place), and the
results are torch tensors on the same device.

The ctypes prototypes of vcp_planes.h live here, on the library _native loads (SYMBOLS lists them)."""
import ctypes as C

import numpy as np

from . import _native
from .moments import _is_dev

# every symbol include/vcp_planes.h declares (tests/test_planes.py checks that the library exports all of them)
SYMBOLS = [
    "vcp_plane_score_shape", "vcp_plane_score", "vcp_plane_score_dev", "vcp_planes_from_triples_dev", "vcp_plane_label_dev",
    "vcp_plane_ransac", "vcp_plane_ransac_dev",
]

MAX_HYPOTHESES = 65536
MAX_PLANES = 64

_P, _I32, _I64, _U64, _F64 = C.c_void_p, C.c_int32, C.c_int64, C.c_uint64, C.c_double
_PROTOTYPES = {
    "vcp_plane_score_shape": [_P, _P],
    "vcp_plane_score": [_P, _P, _I64, _I64, _P, _P, _I32, _F64, _P],
    "vcp_plane_score_dev": [_P, _P, _I64, _I64, _P, _P, _I32, _F64, _P],
    "vcp_planes_from_triples_dev": [_P, _P, _I64, _I64, _P, _I32, _P, _P],
    "vcp_plane_label_dev": [_P, _P, _I64, _I64, _P, _P, _F64, _I32, _P, _P],
    "vcp_plane_ransac": [_P, _P, _I64, _I64, _P, _F64, _I32, _I32, _I64, _U64, _I32, _P, _P, _P, _P, _P],
    "vcp_plane_ransac_dev": [_P, _P, _I64, _I64, _P, _F64, _I32, _I32, _I64, _U64, _I32, _P, _P, _P, _P, _P],
}
_bound = None


def _L():
    """libvcp.so with the prototypes of vcp_planes.h set.  A library without them is an error (no fallback)."""
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


def _host_rows(points):
    """(points, n, ld) of the host forms: [n, c >= 3] float64, read in place at its row stride where that is a whole number
    of doubles (else copied)."""
    points = np.asarray(points, np.float64)
    if points.ndim != 2 or points.shape[1] < 3:
        raise ValueError("points must be [n, c] with c >= 3")
    n = points.shape[0]
    if n <= 1 or not (points.strides[1] == 8 and points.strides[0] % 8 == 0 and points.strides[0] >= 24):
        points = np.ascontiguousarray(points)
    return points, n, (points.strides[0] // 8 if n > 1 else max(points.shape[1], 3))


def _dev_rows(points):
    """(points, n, ld) of the device-pointer forms: a float64 [n, c >= 3] tensor on the GPU, read in place at its row stride
    where the columns are contiguous (else copied)."""
    import torch
    if not torch.is_tensor(points) or points.dtype != torch.float64 or not points.is_cuda or points.dim() != 2 \
            or points.shape[1] < 3:
        raise ValueError("points must be a float64 [n, c >= 3] tensor on the GPU (or a numpy array)")
    n = points.shape[0]
    if n > 1 and not (points.stride(1) == 1 and points.stride(0) >= 3):
        points = points.contiguous()
    return points, n, (int(points.stride(0)) if n > 1 else max(points.shape[1], 3))


def _dev_flags(active, n, dev):
    import torch
    if active is None:
        return None
    if not torch.is_tensor(active):
        active = torch.from_numpy(np.ascontiguousarray(active)).to(dev)
    active = (active != 0).to(torch.uint8).contiguous().reshape(-1) if active.dtype != torch.uint8 else active.contiguous().reshape(-1)
    if active.numel() != n or not active.is_cuda:
        raise ValueError("active must hold one flag per row, on the device of points")
    return active


def _host_flags(active, n):
    if active is None:
        return None
    active = np.ascontiguousarray(np.asarray(active) != 0, np.uint8).reshape(-1)
    if len(active) != n:
        raise ValueError("active must hold one flag per row")
    return active


def _sync(dev):
    import torch
    torch.cuda.current_stream(dev).synchronize()  # the library runs on the context's stream, not torch's


class Planes:
    """What extract_planes returns: planes [P, 4] (a, b, c, d with a unit normal; no sign convention), counts [P] (the rows
    each plane labelled), hyp_counts [P] (the count of the hypothesis that won its round), labels [n] int32 (r + 1 for the
    rows of plane r, 0 for rows on no plane), n_planes = P; numpy arrays or torch tensors, as the input was."""

    def __init__(self, planes, counts, hyp_counts, labels, n_planes):
        self.planes, self.counts, self.hyp_counts, self.labels, self.n_planes = planes, counts, hyp_counts, labels, int(n_planes)

    @property
    def normals(self):
        return self.planes[:, :3]


def extract_planes(points, thr, hypotheses=1024, max_planes=4, min_inliers=0, seed=0, refit=True, active=None, ctx=None):
    """vcp_plane_ransac: up to max_planes planes, each the best of `hypotheses` sampled triples over the rows still active
    (inlier: |a x + b y + c z + d| <= thr), accepted while it holds at least max(min_inliers, 3) rows; with refit the
    least-squares plane of the winner's inliers replaces it where it holds at least as many rows.  active: one flag per
    row (rows with 0 are never sampled, counted or labelled), read only.  The result is a function of the arguments
    alone (seed included).  Returns a Planes."""
    ctx = _ctx(ctx)
    mp = int(max_planes)
    k = max(0, min(mp, MAX_PLANES))
    planes, counts, hyp = np.zeros((k, 4)), np.zeros(k, np.int64), np.zeros(k, np.int64)
    npl = C.c_int32(0)
    thr, H, min_inliers, seed, refit = float(thr), int(hypotheses), int(min_inliers), int(seed) & (2 ** 64 - 1), int(bool(refit))
    if _is_dev(points):
        import torch
        points, n, ld = _dev_rows(points)
        act = _dev_flags(active, n, points.device)
        labels = torch.empty(n, dtype=torch.int32, device=points.device)
        _sync(points.device)
        ctx._chk(_L().vcp_plane_ransac_dev(ctx._h, _p(points), _I64(ld), _I64(n), _p(act), _F64(thr), _I32(H), _I32(mp),
                                           _I64(min_inliers), _U64(seed), _I32(refit), _p(labels), _p(planes), _p(counts),
                                           _p(hyp), C.byref(npl)))
        to = lambda a: torch.from_numpy(a[:npl.value].copy()).to(points.device)
        return Planes(to(planes), to(counts), to(hyp), labels, npl.value)
    points, n, ld = _host_rows(points)
    act = _host_flags(active, n)
    labels = np.zeros(n, np.int32)
    ctx._chk(_L().vcp_plane_ransac(ctx._h, _p(points), _I64(ld), _I64(n), _p(act), _F64(thr), _I32(H), _I32(mp),
                                   _I64(min_inliers), _U64(seed), _I32(refit), _p(labels), _p(planes), _p(counts), _p(hyp),
                                   C.byref(npl)))
    return Planes(planes[:npl.value].copy(), counts[:npl.value].copy(), hyp[:npl.value].copy(), labels, npl.value)


def plane_score(points, planes, thr, active=None, ctx=None):
    """vcp_plane_score: counts [H] int64, the active rows within thr of each of planes [H, 4]."""
    ctx = _ctx(ctx)
    if _is_dev(points):
        import torch
        points, n, ld = _dev_rows(points)
        if not torch.is_tensor(planes):
            planes = torch.from_numpy(np.ascontiguousarray(planes, np.float64)).to(points.device)
        planes = planes.to(torch.float64).contiguous().reshape(-1, 4)
        act = _dev_flags(active, n, points.device)
        H = planes.shape[0]
        counts = torch.empty(H, dtype=torch.int64, device=points.device)
        _sync(points.device)
        ctx._chk(_L().vcp_plane_score_dev(ctx._h, _p(points), _I64(ld), _I64(n), _p(act), _p(planes), _I32(H),
                                          _F64(float(thr)), _p(counts)))
        return counts
    points, n, ld = _host_rows(points)
    planes = np.ascontiguousarray(planes, np.float64).reshape(-1, 4)
    act = _host_flags(active, n)
    H = planes.shape[0]
    counts = np.zeros(H, np.int64)
    ctx._chk(_L().vcp_plane_score(ctx._h, _p(points), _I64(ld), _I64(n), _p(act), _p(planes), _I32(H), _F64(float(thr)),
                                  _p(counts)))
    return counts


def planes_from_triples(points, tri, ctx=None):
    """vcp_planes_from_triples_dev: (planes [H, 4], valid [H] uint8) of the triples tri [H, 3] of row indices.  An invalid
    triple (an index out of range, a repeated or collinear member, a non-finite result) gives four NaN and valid 0.  numpy
    inputs are copied to the device and the results back."""
    import torch
    ctx = _ctx(ctx)
    on_dev = _is_dev(points)
    if not on_dev:
        points = torch.from_numpy(np.ascontiguousarray(np.asarray(points, np.float64))).cuda()
    points, n, ld = _dev_rows(points)
    if not torch.is_tensor(tri):
        tri = torch.from_numpy(np.ascontiguousarray(tri, np.int32)).to(points.device)
    tri = tri.to(torch.int32).contiguous().reshape(-1, 3)
    H = tri.shape[0]
    planes = torch.empty((H, 4), dtype=torch.float64, device=points.device)
    valid = torch.empty(H, dtype=torch.uint8, device=points.device)
    _sync(points.device)
    ctx._chk(_L().vcp_planes_from_triples_dev(ctx._h, _p(points), _I64(ld), _I64(n), _p(tri), _I32(H), _p(planes), _p(valid)))
    return (planes, valid) if on_dev else (planes.cpu().numpy(), valid.cpu().numpy())


def plane_label(points, plane, thr, ident, labels, active=None, ctx=None):
    """vcp_plane_label_dev, in place on torch tensors on the GPU: the active rows within thr of `plane` (four numbers) get
    labels[i] = ident and, where active (uint8) is given, active[i] = 0; nothing else is touched.  Returns the rows
    labelled."""
    import torch
    ctx = _ctx(ctx)
    points, n, ld = _dev_rows(points)
    if not (torch.is_tensor(labels) and labels.dtype == torch.int32 and labels.is_cuda and labels.is_contiguous()
            and labels.numel() == n):
        raise ValueError("labels must be a contiguous int32 [n] tensor on the GPU")
    if active is not None and not (torch.is_tensor(active) and active.dtype == torch.uint8 and active.is_cuda
                                   and active.is_contiguous() and active.numel() == n):
        raise ValueError("active must be a contiguous uint8 [n] tensor on the GPU")
    pl = np.ascontiguousarray(plane, np.float64).reshape(4)
    got = C.c_int64(0)
    _sync(points.device)
    ctx._chk(_L().vcp_plane_label_dev(ctx._h, _p(points), _I64(ld), _I64(n), _p(active), _p(pl), _F64(float(thr)),
                                      _I32(int(ident)), _p(labels), C.byref(got)))
    return got.value


def plane_score_shape(ctx=None):
    """vcp_plane_score_shape: (tile, chunk, grid) of the score kernel on the context's device."""
    ctx = _ctx(ctx)
    shape = np.zeros(3, np.int32)
    ctx._chk(_L().vcp_plane_score_shape(ctx._h, _p(shape)))
    return tuple(int(v) for v in shape)


def plane_residuals(points, plane):
    """The signed residual a x + b y + c z + d of every row, in plain numpy / torch operations (each rounded on its own, in
    the order of the definition)."""
    a, b, c, d = (float(v) for v in plane)
    return ((a * points[:, 0] + b * points[:, 1]) + c * points[:, 2]) + d


def remove_planes(fit):
    """(keep, kept_idx) of an extract_planes result: keep [n] is labels == 0, kept_idx the indices of the kept rows in
    ascending order -- the bulk form of Tools.removeFilterPointFromClustering, as vcp_cluster_filter's keep / kept_idx."""
    keep = fit.labels == 0
    if _is_dev(fit.labels):
        import torch
        return keep.to(torch.uint8), torch.nonzero(keep).reshape(-1).to(torch.int32)
    return keep.astype(np.uint8), np.nonzero(keep)[0].astype(np.int32)
