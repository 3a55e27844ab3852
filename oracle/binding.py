"""ctypes binding of the CPU oracle (oracle/libvcp_oracle.so).

TEST INFRASTRUCTURE ONLY: imported by tests/, __graft_entry__.smoke() and bench.py's
cpu_baseline leg.  Nothing under vtkcloudpoint_amd/ may import this module.
"""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_SO = os.path.join(_HERE, "libvcp_oracle.so")

L1_2D, L2_2D, L2_3D, SIGNED_SUM_2D = 0, 1, 2, 3
STOP_SSE_DELTA, STOP_RMSE = 0, 1
OK, ERR_ARG, ERR_EMPTY, ERR_DEGENERATE, ERR_INDEX, ERR_TOO_LARGE = 0, -1, -2, -3, -4, -5


def build():
    src = [os.path.join(_HERE, f) for f in ("vcp_oracle.cpp", "vcp_oracle.h", "Makefile")]
    if (not os.path.exists(_SO)) or any(os.path.getmtime(s) > os.path.getmtime(_SO) for s in src):
        subprocess.check_call(["make", "-C", _HERE, "-s"])
    return _SO


_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(build())
    return _lib


def _p(a, t):
    return None if a is None else a.ctypes.data_as(C.POINTER(t))


def _f64(a, cols=None):
    a = np.ascontiguousarray(a, dtype=np.float64)
    if cols is not None:
        a = a.reshape(-1, cols)
    return a


class OracleError(RuntimeError):
    def __init__(self, code):
        super().__init__("oracle error %d" % code)
        self.code = code


def _chk(rc):
    if rc != 0:
        raise OracleError(rc)


def _state(n, classed, labels, is_key):
    classed = np.zeros(n, np.uint8) if classed is None else np.array(classed, np.uint8)
    labels = np.zeros(n, np.int32) if labels is None else np.array(labels, np.int32)
    is_key = np.zeros(n, np.uint8) if is_key is None else np.array(is_key, np.uint8)
    return classed, labels, is_key


def dbscan(coords, eps, min_pts, metric=L1_2D, cf_in=0, classed=None, labels=None, is_key=None,
           literal=False, dedupe=False):
    """Returns dict(labels, classed, is_key, cf, evals).  coords [n, dim]."""
    coords = _f64(coords)
    n, dim = coords.shape if coords.ndim == 2 else (0, 2)
    classed, labels, is_key = _state(n, classed, labels, is_key)
    cf = C.c_int32(0)
    ev = C.c_int64(0)
    if literal:
        rc = lib().orc_dbscan_literal(_p(coords, C.c_double), C.c_int64(n), dim, metric, C.c_double(eps),
                                      int(min_pts), C.c_int32(cf_in), _p(classed, C.c_uint8),
                                      _p(labels, C.c_int32), _p(is_key, C.c_uint8), C.byref(cf),
                                      C.byref(ev), int(dedupe))
    else:
        rc = lib().orc_dbscan_canonical(_p(coords, C.c_double), C.c_int64(n), dim, metric, C.c_double(eps),
                                        int(min_pts), C.c_int32(cf_in), _p(classed, C.c_uint8),
                                        _p(labels, C.c_int32), _p(is_key, C.c_uint8), C.byref(cf),
                                        C.byref(ev))
    _chk(rc)
    return dict(labels=labels, classed=classed, is_key=is_key, cf=cf.value, evals=ev.value)


def db_literal(coords, eps, min_pts, shown=None, classed=None, labels=None, is_key=None):
    coords = _f64(coords)
    n, dim = coords.shape
    shown = np.ones(n, np.uint8) if shown is None else np.array(shown, np.uint8)
    classed, labels, is_key = _state(n, classed, labels, is_key)
    ca, pa, ev = C.c_int32(0), C.c_int32(0), C.c_int64(0)
    _chk(lib().orc_db_literal(_p(coords, C.c_double), C.c_int64(n), dim, C.c_double(eps), int(min_pts),
                              _p(shown, C.c_uint8), _p(classed, C.c_uint8), _p(labels, C.c_int32),
                              _p(is_key, C.c_uint8), C.byref(ca), C.byref(pa), C.byref(ev)))
    return dict(labels=labels, classed=classed, is_key=is_key, cluster_amount=ca.value,
                points_amount=pa.value, evals=ev.value)


def block_pipeline(motor, eps, min_pts, pts_in_cell, small_max=3, canonical=True, brute=False, key_xy=None):
    """key_xy: the partition's coordinates (getClusterFromList reads X,Y); None = motor (getClusterFromMotor)."""
    motor = _f64(motor, 2)
    key_xy = motor if key_xy is None else _f64(key_xy, 2)
    n = motor.shape[0]
    labels = np.zeros(n, np.int32)
    block_of = np.zeros(n, np.int32)
    order = np.zeros(max(n, 1), np.int64)
    m = C.c_int64(0)
    rows, cols, kept, dels, ca = (C.c_int32(0) for _ in range(5))
    ev = C.c_int64(0)
    _chk(lib().orc_block_pipeline_keyed(_p(key_xy, C.c_double), _p(motor, C.c_double), C.c_int64(n), C.c_double(eps), int(min_pts),
                                  int(pts_in_cell), int(small_max), int(canonical), int(brute),
                                  _p(labels, C.c_int32), _p(block_of, C.c_int32), _p(order, C.c_int64),
                                  C.byref(m), C.byref(rows), C.byref(cols), C.byref(kept),
                                  C.byref(dels), C.byref(ca), C.byref(ev)))
    return dict(labels=labels, block_of=block_of, order=order[: m.value].copy(), rows=rows.value,
                cols=cols.value, kept=kept.value, del_sum=dels.value, cluster_amount=ca.value,
                evals=ev.value)


def centroids(xyz, motor, labels, K, order=None):
    xyz = None if xyz is None else _f64(xyz, 3)
    motor = None if motor is None else _f64(motor, 2)
    labels = np.ascontiguousarray(labels, np.int32)
    order = None if order is None else np.ascontiguousarray(order, np.int64)
    m = len(labels) if order is None else len(order)
    c3 = np.zeros((K, 3))
    c2 = np.zeros((K, 2))
    counts = np.zeros(K, np.int64)
    _chk(lib().orc_centroids(_p(xyz, C.c_double), _p(motor, C.c_double), _p(labels, C.c_int32),
                             _p(order, C.c_int64), C.c_int64(m), C.c_int32(K), _p(c3, C.c_double),
                             _p(c2, C.c_double), _p(counts, C.c_int64)))
    return c3, c2, counts


def fixed_centroids(xyz, group, cluster_id, pts_count, K, ignore_dup):
    """Tools.getFixedPtsCentroid: returns (c3 [K,3], inside_num [K])."""
    xyz = _f64(xyz, 3)
    group = np.ascontiguousarray(group, np.int32)
    cluster_id = None if cluster_id is None else np.ascontiguousarray(cluster_id, np.int32)
    pts_count = np.ascontiguousarray(pts_count, np.int32)
    c3 = np.zeros((K, 3))
    inside = np.zeros(K, np.int64)
    _chk(lib().orc_fixed_centroids(_p(xyz, C.c_double), _p(group, C.c_int32), _p(cluster_id, C.c_int32),
                                   _p(pts_count, C.c_int32), C.c_int64(len(group)), C.c_int32(K), int(bool(ignore_dup)),
                                   _p(c3, C.c_double), _p(inside, C.c_int64)))
    return c3, inside


def merge_ids(cxy, ids, thr):
    cxy = _f64(cxy, 2)
    ids = np.ascontiguousarray(ids, np.int32)
    K = len(ids)
    map_to = np.zeros(K, np.int32)
    mc = C.c_int32(0)
    _chk(lib().orc_merge_ids(_p(cxy, C.c_double), _p(ids, C.c_int32), C.c_int32(K), C.c_double(thr),
                             _p(map_to, C.c_int32), C.byref(mc)))
    return map_to, mc.value


def refresh_by_dictionary(xyz, motor, labels, K, map_by_id, order=None):
    xyz = _f64(xyz, 3)
    motor = _f64(motor, 2)
    labels = np.array(labels, np.int32)
    map_by_id = np.ascontiguousarray(map_by_id, np.int32)
    order = None if order is None else np.ascontiguousarray(order, np.int64)
    m = len(labels) if order is None else len(order)
    c3 = np.zeros((K, 3))
    c2 = np.zeros((K, 2))
    counts = np.zeros(K, np.int64)
    nk = C.c_int32(0)
    _chk(lib().orc_refresh_by_dictionary(_p(xyz, C.c_double), _p(motor, C.c_double), _p(labels, C.c_int32),
                                         _p(order, C.c_int64), C.c_int64(m), C.c_int32(K),
                                         _p(map_by_id, C.c_int32), C.byref(nk), _p(c3, C.c_double),
                                         _p(c2, C.c_double), _p(counts, C.c_int64)))
    k = nk.value
    return labels, k, c3[:k], c2[:k], counts[:k]


def find_closest(model, p):
    model = _f64(model, 3)
    p = _f64(p, 3)
    idx = np.zeros(len(p), np.int32)
    lib().orc_find_closest(_p(model, C.c_double), C.c_int64(len(model)), _p(p, C.c_double),
                           C.c_int64(len(p)), _p(idx, C.c_int32))
    return idx


def trans_point(src, R, T):
    src = _f64(src, 3)
    R = _f64(R).reshape(9)
    T = _f64(T).reshape(3)
    dst = np.zeros_like(src)
    lib().orc_trans_point(_p(src, C.c_double), C.c_int64(len(src)), _p(R, C.c_double), _p(T, C.c_double),
                          _p(dst, C.c_double))
    return dst


def calc_rotation(q):
    q = _f64(q).reshape(4)
    R = np.zeros(9)
    lib().orc_calc_rotation(_p(q, C.c_double), _p(R, C.c_double))
    return R.reshape(3, 3)


def icp_sums(model, p):
    model = _f64(model, 3)
    p = _f64(p, 3)
    s = np.zeros(16)
    lib().orc_icp_sums(_p(model, C.c_double), C.c_int64(len(model)), _p(p, C.c_double), C.c_int64(len(p)),
                       _p(s, C.c_double))
    return s


def horn_from_sums(s, nd):
    s = _f64(s).reshape(16)
    R1 = np.zeros(9)
    T1 = np.zeros(3)
    _chk(lib().orc_horn_from_sums(_p(s, C.c_double), C.c_int64(nd), _p(R1, C.c_double), _p(T1, C.c_double)))
    return R1.reshape(3, 3), T1


def jacobi_sym(A):
    A = np.array(A, np.float64)
    n = A.shape[0]
    ev = np.zeros(n)
    V = np.zeros((n, n))
    lib().orc_jacobi_sym(_p(A, C.c_double), n, _p(ev, C.c_double), _p(V, C.c_double), 64)
    return ev, V


def icp(model, data, tol=1e-4, max_iter=100, stop_rule=STOP_SSE_DELTA):
    model = _f64(model, 3)
    data = _f64(data, 3)
    R = np.zeros(9)
    T = np.zeros(3)
    sse, rmse = C.c_double(0), C.c_double(0)
    it = C.c_int32(0)
    _chk(lib().orc_icp(_p(model, C.c_double), C.c_int64(len(model)), _p(data, C.c_double),
                       C.c_int64(len(data)), C.c_double(tol), int(max_iter), int(stop_rule),
                       _p(R, C.c_double), _p(T, C.c_double), C.byref(sse), C.byref(rmse), C.byref(it)))
    return dict(R=R.reshape(3, 3), T=T, sse=sse.value, rmse=rmse.value, iters=it.value)


def min_circle_ex(pts, literal=False):
    """dict(center, radius, hull, inserted): literal = the C# as it stands; otherwise with the insertion rule of
    DESIGN.md section 12 (inserted = members it added; hull is the wrap's either way)."""
    pts = _f64(pts, 2)
    c = np.zeros(2)
    r = C.c_double(0)
    hn, ins = C.c_int32(0), C.c_int32(0)
    hull = np.zeros((len(pts), 2))
    _chk(lib().orc_min_circle_ex(_p(pts, C.c_double), C.c_int64(len(pts)), int(literal), _p(c, C.c_double), C.byref(r),
                                 _p(hull, C.c_double), C.c_int64(len(pts)), C.byref(hn), C.byref(ins)))
    return dict(center=c, radius=r.value, hull=hull[: hn.value], inserted=ins.value)


def min_circle(pts, literal=False):
    g = min_circle_ex(pts, literal)
    return g["center"], g["radius"], g["hull"]


def get_circles(xy, labels, K, order=None, literal=False):
    xy = _f64(xy, 2)
    labels = np.ascontiguousarray(labels, np.int32)
    order = None if order is None else np.ascontiguousarray(order, np.int64)
    m = len(labels) if order is None else len(order)
    centers = np.zeros((K, 2))
    radius = np.zeros(K)
    valid = np.zeros(K, np.uint8)
    hn = np.zeros(K, np.int32)
    ins = np.zeros(K, np.int32)
    _chk(lib().orc_get_circles_ex(_p(xy, C.c_double), _p(labels, C.c_int32), _p(order, C.c_int64), C.c_int64(m),
                                  C.c_int32(K), int(literal), _p(centers, C.c_double), _p(radius, C.c_double),
                                  _p(valid, C.c_uint8), _p(hn, C.c_int32), _p(ins, C.c_int32)))
    return dict(centers=centers, radius=radius, valid=valid, hull_n=hn, inserted=ins)


def import_convert(rows, x_angle=0.0, y_angle=0.0, xdir=2, ydir=1, dedupe=True, literal=False):
    rows = _f64(rows, 3)
    n = len(rows)
    xyz = np.zeros((n, 3))
    state = np.zeros(n, np.uint8)
    kept, dup = C.c_int64(0), C.c_int64(0)
    _chk(lib().orc_import_convert(_p(rows, C.c_double), C.c_int64(n), C.c_double(x_angle), C.c_double(y_angle),
                                  int(xdir), int(ydir), int(dedupe), int(literal), _p(xyz, C.c_double),
                                  _p(state, C.c_uint8), C.byref(kept), C.byref(dup)))
    return dict(xyz=xyz, state=state, kept=kept.value, duplicates=dup.value)


def icp_vtklike(source, target, max_iter=100, max_landmarks=200, start_by_centroids=True):
    source = _f64(source, 3)
    target = _f64(target, 3)
    M = np.zeros(16)
    md = C.c_double(0)
    it = C.c_int32(0)
    _chk(lib().orc_icp_vtklike(_p(source, C.c_double), C.c_int64(len(source)), _p(target, C.c_double),
                               C.c_int64(len(target)), int(max_iter), int(max_landmarks), int(start_by_centroids),
                               _p(M, C.c_double), C.byref(md), C.byref(it)))
    return dict(M=M.reshape(4, 4), mean_dist=md.value, iters=it.value)


def assign_truths(motor, truths_xy, truth_ids, radius):
    motor = _f64(motor, 2)
    truths_xy = _f64(truths_xy, 2)
    truth_ids = np.ascontiguousarray(truth_ids, np.int32)
    ids = np.zeros(len(motor), np.int32)
    out = C.c_int64(0)
    _chk(lib().orc_assign_truths(_p(motor, C.c_double), C.c_int64(len(motor)), _p(truths_xy, C.c_double),
                                 _p(truth_ids, C.c_int32), C.c_int32(len(truth_ids)), C.c_double(radius),
                                 _p(ids, C.c_int32), C.byref(out)))
    return ids, out.value


def match(centers, truths, M, max_dist):
    centers = _f64(centers, 3)
    truths = _f64(truths, 3)
    M = _f64(M).reshape(16)
    K, T = len(centers), len(truths)
    mxyz = np.zeros((K, 3))
    is_m = np.zeros(K, np.uint8)
    nearest = np.zeros(K, np.int32)
    nd = np.zeros(K)
    cnt = C.c_int32(0)
    _chk(lib().orc_match(_p(centers, C.c_double), C.c_int32(K), _p(truths, C.c_double), C.c_int32(T),
                         _p(M, C.c_double), C.c_double(max_dist), _p(mxyz, C.c_double), _p(is_m, C.c_uint8),
                         _p(nearest, C.c_int32), _p(nd, C.c_double), C.byref(cnt)))
    return dict(matched_xyz=mxyz, is_matched=is_m, nearest=nearest, nearest_dist=nd, count=cnt.value)


class StagedBlocks:
    """The oracle's block pipeline in stages, with the same method names as the product's Context
    (blocks_begin / blocks_share / blocks_cluster_dev / blocks_finish_dev) so that the distributed driver
    can be exercised on CPU tensors (gloo) in the tests.  Pointers are host addresses here."""

    def __init__(self):
        self.s = None

    def blocks_begin(self, motor, eps, min_pts, pts_in_cell, small_max=3, device_ptr=None, n=None):
        motor = _f64(motor, 2)
        n = len(motor)
        block_of = np.zeros(n, np.int32)
        raw = np.zeros(max(n, 1), np.int64)
        bl = np.zeros(max(n, 1), np.int64)
        rows, cols, m = C.c_int32(0), C.c_int32(0), C.c_int64(0)
        _chk(lib().orc_block_partition(_p(motor, C.c_double), C.c_int64(n), int(pts_in_cell), 0,
                                       _p(block_of, C.c_int32), _p(raw, C.c_int64), _p(bl, C.c_int64), None,
                                       C.c_int64(0), C.byref(rows), C.byref(cols), C.byref(m)))
        nblocks = rows.value * cols.value
        blockstart = np.zeros(nblocks + 1, np.int64)
        np.add.at(blockstart, block_of[block_of >= 0].astype(np.int64) + 1, 1)
        blockstart = np.cumsum(blockstart)
        self.s = dict(motor=motor, n=n, eps=float(eps), min_pts=int(min_pts), small_max=int(small_max),
                      block_of=block_of, bl=bl, blockstart=blockstart, nblocks=nblocks, m=m.value)
        return dict(rows=rows.value, cols=cols.value, nblocks=nblocks, m=m.value)

    def blocks_share(self, rank, world):
        s = self.s

        def cut(r):
            if r <= 0:
                return 0
            if r >= world:
                return s["nblocks"]
            target = (s["m"] * r) // world
            return int(np.searchsorted(s["blockstart"][: s["nblocks"]], target, side="left"))

        lo, hi = cut(rank), cut(rank + 1)
        return lo, hi, int(s["blockstart"][lo]), int(s["blockstart"][hi])

    def blocks_cluster_dev(self, block_lo, block_hi, ptr):
        s = self.s
        local = np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_int32)), shape=(max(s["m"], 1),))
        ev = C.c_int64(0)
        _chk(lib().orc_block_cluster(_p(s["motor"], C.c_double), _p(s["bl"], C.c_int64),
                                     _p(s["blockstart"], C.c_int64), C.c_int64(block_lo), C.c_int64(block_hi),
                                     C.c_double(s["eps"]), s["min_pts"], 1, _p(local, C.c_int32), C.byref(ev)))
        return ev.value

    def blocks_finish_dev(self, local_ptr, evals_blocks, labels_ptr, d_block_of=None, d_merge_order=None):
        s = self.s
        local = np.ctypeslib.as_array(C.cast(local_ptr, C.POINTER(C.c_int32)), shape=(max(s["m"], 1),))
        labels = np.ctypeslib.as_array(C.cast(labels_ptr, C.POINTER(C.c_int32)), shape=(max(s["n"], 1),))
        order = np.zeros(max(s["n"], 1), np.int64)
        m = C.c_int64(0)
        kept, dels, ca = (C.c_int32(0) for _ in range(3))
        ev = C.c_int64(0)
        _chk(lib().orc_block_finish(_p(s["motor"], C.c_double), C.c_int64(s["n"]), _p(s["bl"], C.c_int64),
                                    _p(s["blockstart"], C.c_int64), C.c_int64(s["nblocks"]), _p(local, C.c_int32),
                                    C.c_double(s["eps"]), s["min_pts"], s["small_max"], 1, C.c_int64(evals_blocks),
                                    _p(labels, C.c_int32), _p(order, C.c_int64), C.byref(m), C.byref(kept),
                                    C.byref(dels), C.byref(ca), C.byref(ev)))
        return dict(m=m.value, kept=kept.value, del_sum=dels.value, cluster_amount=ca.value, evals=ev.value,
                    order=order[: m.value].copy())


class StagedSlab:
    """The oracle's staged exact-global DBSCAN with the method names of the product's Context (slab_begin /
    slab_comps / slab_finish), so that distributed.exact_slabs can be exercised on CPU tensors (gloo) in the
    tests.  Pointers are host addresses here."""

    def __init__(self):
        self.s = None

    @staticmethod
    def _view(ptr, ctype, dtype, shape):
        return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(ctype)), shape=shape).view(dtype)

    def slab_begin(self, d_coords, n, dim, metric, eps, min_pts, d_noexpand, d_ord, d_rep, d_is_core=None):
        coords = self._view(d_coords, C.c_double, np.float64, (n * dim,)).copy()
        noexp = None if not d_noexpand else self._view(d_noexpand, C.c_uint8, np.uint8, (n,)).copy()
        ord_ = self._view(d_ord, C.c_uint32, np.uint32, (n,)).copy()
        rep = self._view(d_rep, C.c_uint32, np.uint32, (n,))
        core = None if not d_is_core else self._view(d_is_core, C.c_uint8, np.uint8, (n,))
        nc = C.c_int64(0)
        _chk(lib().orc_slab_begin(_p(coords, C.c_double), C.c_int64(n), int(dim), int(metric), C.c_double(eps),
                                  int(min_pts), None if noexp is None else _p(noexp, C.c_uint8), _p(ord_, C.c_uint32),
                                  _p(rep, C.c_uint32), None if core is None else _p(core, C.c_uint8), C.byref(nc)))
        self.s = dict(coords=coords, n=n, dim=dim, metric=int(metric), eps=float(eps), noexp=noexp, ord=ord_,
                      rep=rep.copy(), n_comp=nc.value)
        return nc.value

    def slab_comps(self):
        rep = self.s["rep"]
        return np.unique(rep[rep != 0xFFFFFFFF]).astype(np.uint32)

    def slab_finish(self, map_rep, map_k, tab_gid, tab_seed, own_lo, own_count, d_labels, d_is_classed=None):
        s = self.s
        n = s["n"]
        map_rep = np.ascontiguousarray(map_rep, np.uint32)
        map_k = np.ascontiguousarray(map_k, np.uint32)
        tab_gid = np.ascontiguousarray(tab_gid, np.int32)
        tab_seed = np.ascontiguousarray(tab_seed, np.uint32)
        labels = self._view(d_labels, C.c_int32, np.int32, (n,))
        classed = None if not d_is_classed else self._view(d_is_classed, C.c_uint8, np.uint8, (n,))
        tw = C.c_int64(0)
        _chk(lib().orc_slab_finish(_p(s["coords"], C.c_double), C.c_int64(n), s["dim"], s["metric"],
                                   C.c_double(s["eps"]), None if s["noexp"] is None else _p(s["noexp"], C.c_uint8),
                                   _p(s["ord"], C.c_uint32), _p(s["rep"], C.c_uint32), _p(map_rep, C.c_uint32),
                                   _p(map_k, C.c_uint32), C.c_int64(len(map_rep)), _p(tab_gid, C.c_int32),
                                   _p(tab_seed, C.c_uint32), C.c_int64(len(tab_gid)), C.c_uint32(own_lo),
                                   C.c_uint32(own_count), _p(labels, C.c_int32),
                                   None if classed is None else _p(classed, C.c_uint8), C.byref(tw)))
        return tw.value


class StagedPipeline(StagedSlab):
    """CPU stand-in for the product's sharded block pipeline (Context.blocks_plan / blocks_plan_cuts / blocks_build /
    blocks_cluster_dev / blocks_finish_local / blocks_finish_zero / blocks_finish_zcoords / blocks_finish_pairs /
    scatter_pairs, plus the slab_* methods of StagedSlab for the global noise pass), so that
    distributed.sharded_pipeline can be exercised on CPU tensors (gloo).  The partition and the per-block DBImproved come
    from the oracle's C++ (orc_block_partition, orc_block_cluster); the per-share CompleteWork3 (FrmMain.cs:1442-1504)
    is restated here in plain numpy / Python loops.  What the tests compare against is orc_block_pipeline, the whole
    single-process pipeline.  Pointers are host addresses; a super-bucket is one block here."""

    def __init__(self):
        super().__init__()
        self.p = None

    def blocks_plan(self, d_motor, n, eps, min_pts, pts_in_cell, small_max=3, d_key=None):
        motor = np.ctypeslib.as_array(C.cast(d_motor, C.POINTER(C.c_double)), shape=(n, 2)).copy()
        block_of = np.zeros(n, np.int32)
        raw = np.zeros(max(n, 1), np.int64)
        bl = np.zeros(max(n, 1), np.int64)
        rows, cols, m = C.c_int32(0), C.c_int32(0), C.c_int64(0)
        _chk(lib().orc_block_partition(_p(motor, C.c_double), C.c_int64(n), int(pts_in_cell), 0,
                                       _p(block_of, C.c_int32), _p(raw, C.c_int64), _p(bl, C.c_int64), None,
                                       C.c_int64(0), C.byref(rows), C.byref(cols), C.byref(m)))
        nblocks = rows.value * cols.value
        blockstart = np.zeros(nblocks + 1, np.int64)
        np.add.at(blockstart, block_of[block_of >= 0].astype(np.int64) + 1, 1)
        blockstart = np.cumsum(blockstart)
        dropped = np.nonzero(block_of < 0)[0].astype(np.int64)
        # the rectangles as FrmMain.cs:1262-1285 evaluates them (for the active set of the noise pass)
        x_min, x_max = motor[:, 0].min(), motor[:, 0].max()
        y_min, y_max = motor[:, 1].min(), motor[:, 1].max()
        first = motor[bl[: int(blockstart[1])]]
        geo = dict(x_min=x_min, x_max=x_max, y_min=y_min, y_max=y_max, cell_x=first[:, 0].max() - x_min,
                   cell_y=first[:, 1].max() - y_min, rows=rows.value, cols=cols.value)
        # "super-bucket" S = block S; the last one (S = nblocks) holds the points in no block
        sbstart = np.concatenate([blockstart, [n]]).astype(np.int64)
        self.p = dict(motor=motor, n=n, eps=float(eps), min_pts=int(min_pts), small_max=int(small_max), bl=bl,
                      blockstart=blockstart, nblocks=nblocks, m=m.value, dropped=dropped, sbstart=sbstart, geo=geo)
        return dict(rows=rows.value, cols=cols.value, nblocks=nblocks, nsuper=nblocks + 1)

    def blocks_plan_cuts(self, world):
        p = self.p
        ns = p["nblocks"] + 1
        cuts = [0]
        for r in range(1, world):
            target = (p["n"] * r) // world
            cuts.append(max(cuts[-1], int(np.searchsorted(p["sbstart"][:ns], target, side="left"))))
        cuts.append(ns)
        return cuts

    def blocks_build(self, super_lo, super_hi):
        p = self.p
        nb = p["nblocks"]
        lo, hi = min(super_lo, nb), min(super_hi, nb)
        p.update(b_lo=lo, b_hi=hi, has_dropped=super_hi == nb + 1 and super_lo <= nb)
        m = int(p["blockstart"][hi] - p["blockstart"][lo])
        n_loc = m + (len(p["dropped"]) if p["has_dropped"] else 0)
        p.update(m_loc=m, n_loc=n_loc)
        return dict(block_lo=lo, block_hi=hi, m=m, n_loc=n_loc)

    def blocks_cluster_dev(self, block_lo, block_hi, ptr):
        p = self.p
        full = np.zeros(max(p["m"], 1), np.int32)
        ev = C.c_int64(0)
        _chk(lib().orc_block_cluster(_p(p["motor"], C.c_double), _p(p["bl"], C.c_int64),
                                     _p(p["blockstart"], C.c_int64), C.c_int64(block_lo), C.c_int64(block_hi),
                                     C.c_double(p["eps"]), p["min_pts"], 1, _p(full, C.c_int32), C.byref(ev)))
        local = np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_int32)), shape=(max(p["m_loc"], 1),))
        s0 = int(p["blockstart"][p["b_lo"]])
        local[: p["m_loc"]] = full[s0: s0 + p["m_loc"]]
        return ev.value

    def blocks_finish_local(self, local_ptr):
        """CompleteWork3 inside the share: FrmMain.cs:1449-1459 (order by local id, stable), :1460-1504 (renumber, demote
        a cluster of <= small_max points when the next id shows up -- clusLen counts one too many for the first cluster of a
        block without noise, the last cluster of a block is never checked, and demoting that over-counted first cluster
        also zeroes the entry in front of the block)."""
        p = self.p
        m = p["m_loc"]
        local = np.ctypeslib.as_array(C.cast(local_ptr, C.POINTER(C.c_int32)), shape=(max(m, 1),))[:m].copy()
        s0 = int(p["blockstart"][p["b_lo"]])
        newlab = np.zeros(m, np.int32)
        order = np.zeros(m, np.int64)  # final order: share-relative positions
        kept = clusters = err = req = 0
        last_block_end = None  # final-order position (exclusive) of the end of the last non-empty block so far
        for b in range(p["b_lo"], p["b_hi"]):
            a, e = int(p["blockstart"][b]) - s0, int(p["blockstart"][b + 1]) - s0
            if e == a:
                continue
            ids = local[a:e]
            o = np.argsort(ids, kind="stable")
            order[a:e] = a + o
            K = int(ids.max())
            zb = int((ids == 0).sum())
            sizes = np.bincount(ids, minlength=K + 1)
            for k in range(1, K + 1):
                eff = int(sizes[k]) + (1 if (zb == 0 and k == 1) else 0)
                demoted = k < K and eff <= p["small_max"]
                clusters += 1
                if demoted:
                    if zb == 0 and k == 1:
                        if last_block_end is None:
                            if p["b_lo"] == 0:
                                err += 1
                            else:
                                req = 1
                        else:
                            newlab[order[last_block_end - 1]] = 0
                else:
                    kept += 1
                    newlab[a + np.nonzero(ids == k)[0]] = kept
            last_block_end = e
        nonempty = last_block_end is not None
        last_nonzero = bool(nonempty and newlab[order[last_block_end - 1]] != 0)
        p.update(newlab=newlab, order=order, last_pos=(int(order[last_block_end - 1]) if nonempty else -1), local=local)
        return dict(clusters=clusters, kept=kept, err=err, req=req, nonempty=int(nonempty),
                    last_nonzero=int(last_nonzero), m=m, n_loc=p["n_loc"])

    def blocks_finish_zero(self, zero_last):
        p = self.p
        if zero_last and p["last_pos"] >= 0:
            p["newlab"][p["last_pos"]] = 0
        inorder = p["newlab"][p["order"]] if p["m_loc"] else np.zeros(0, np.int32)
        zall = p["order"][inorder == 0]  # the zero list, in final order (FrmMain.cs:1510-1515)
        # active = what the noise pass can reach (product: csrc/blocks.hip k_zero_flag): lost a label, or not more than
        # 2 eps inside its rectangle
        g, s0 = p["geo"], int(p["blockstart"][p["b_lo"]])
        idx = p["bl"][s0 + zall]
        xy = p["motor"][idx]
        blk = np.searchsorted(p["blockstart"], s0 + zall, side="right") - 1
        pr, q = blk // g["cols"], blk % g["cols"]
        lox = g["x_min"] + q.astype(np.float64) * g["cell_x"]
        hix = np.where(q == g["cols"] - 1, g["x_max"], g["x_min"] + (q + 1).astype(np.float64) * g["cell_x"])
        loy = g["y_min"] + pr.astype(np.float64) * g["cell_y"]
        hiy = np.where(pr == g["rows"] - 1, g["y_max"], g["y_min"] + (pr + 1).astype(np.float64) * g["cell_y"])
        r2 = 2.0 * p["eps"] * (1.0 + 2.0 ** -40)
        with np.errstate(invalid="ignore"):
            interior = (xy[:, 0] - lox > r2) & (hix - xy[:, 0] > r2) & (xy[:, 1] - loy > r2) & (hiy - xy[:, 1] > r2)
        act = (p["local"][zall] > 0) | ~interior
        if not (p["eps"] >= 0.0):
            act[:] = True
        p["zpos"] = zall[act]
        return int(len(zall)), int(len(p["zpos"]))

    def blocks_finish_zcoords(self, ptr, swap_xy=True):
        p = self.p
        z = len(p["zpos"])
        if z == 0:
            return
        s0 = int(p["blockstart"][p["b_lo"]])
        xy = p["motor"][p["bl"][s0 + p["zpos"]]]
        out = np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_double)), shape=(z, 2))
        out[:] = xy[:, ::-1] if swap_xy else xy

    def blocks_finish_pairs(self, kept_offset, zlab_ptr, pairs_ptr):
        p = self.p
        m, n_loc = p["m_loc"], p["n_loc"]
        s0 = int(p["blockstart"][p["b_lo"]])
        lab = p["newlab"].astype(np.int64)
        lab[lab > 0] += kept_offset
        z = len(p["zpos"])
        if z:
            zlab = np.ctypeslib.as_array(C.cast(zlab_ptr, C.POINTER(C.c_int32)), shape=(z,))
            lab[p["zpos"]] = zlab
        idx = p["bl"][s0: s0 + m].astype(np.int64)
        if p["has_dropped"]:
            idx = np.concatenate([idx, p["dropped"]])
            lab = np.concatenate([lab, np.zeros(len(p["dropped"]), np.int64)])
        out = np.ctypeslib.as_array(C.cast(pairs_ptr, C.POINTER(C.c_int64)), shape=(max(n_loc, 1),))
        out[:n_loc] = (idx << 32) | (lab & 0xFFFFFFFF)

    def dbscan_dev(self, cptr, n, dim, eps, min_pts, metric=L1_2D, cf_in=0, d_in_classed=None, lptr=None, *a):
        coords = np.ctypeslib.as_array(C.cast(cptr, C.POINTER(C.c_double)), shape=(n, dim))
        r = dbscan(coords, eps, min_pts, metric, cf_in)
        np.ctypeslib.as_array(C.cast(lptr, C.POINTER(C.c_int32)), shape=(n,))[:] = r["labels"]
        return r["cf"], r["evals"]

    def scatter_pairs(self, pairs_ptr, count, n, labels_ptr):
        pr = np.ctypeslib.as_array(C.cast(pairs_ptr, C.POINTER(C.c_int64)), shape=(count,))
        labels = np.ctypeslib.as_array(C.cast(labels_ptr, C.POINTER(C.c_int32)), shape=(n,))
        labels[(pr >> 32).astype(np.int64)] = (pr & 0xFFFFFFFF).astype(np.int64).astype(np.int32)
