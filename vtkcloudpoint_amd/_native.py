"""ctypes binding of libvcp.so (include/vcp.h).  No CPU fallback: if the HIP library is missing or
no GPU is present every compute call raises."""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libvcp.so")

L1_2D, L2_2D, L2_3D, SIGNED_SUM_2D = 0, 1, 2, 3
STOP_SSE_DELTA, STOP_RMSE = 0, 1

STATUS = {
    0: "VCP_OK", -1: "VCP_ERR_ARG", -2: "VCP_ERR_EMPTY", -3: "VCP_ERR_DEGENERATE", -4: "VCP_ERR_INDEX",
    -5: "VCP_ERR_TOO_LARGE", -6: "VCP_ERR_NO_DEVICE", -7: "VCP_ERR_HIP", -8: "VCP_ERR_UNSUPPORTED",
    -9: "VCP_ERR_NOMEM",
}

# every symbol include/vcp.h declares (tests check that the library exports all of them)
SYMBOLS = [
    "vcp_create", "vcp_destroy", "vcp_last_error", "vcp_version", "vcp_set_stream", "vcp_dev_alloc",
    "vcp_dev_free", "vcp_h2d", "vcp_d2h", "vcp_timing_enable", "vcp_timing_count", "vcp_timing_get",
    "vcp_dbscan", "vcp_dbscan_dev", "vcp_dbscan_blocks", "vcp_blocks_begin", "vcp_blocks_begin_dev",
    "vcp_blocks_share", "vcp_blocks_cluster_dev", "vcp_blocks_finish_dev", "vcp_centroids", "vcp_centroids_dev",
    "vcp_merge_centroids", "vcp_refresh_by_dictionary", "vcp_icp", "vcp_icp_dev", "vcp_icp_sums",
    "vcp_match", "vcp_mcc", "vcp_assign_truths", "vcp_icp_vtklike", "vcp_import_convert",
    "vcp_slab_begin", "vcp_slab_comps", "vcp_slab_finish", "vcp_release_workspace", "vcp_selftest_scan_dev",
    "vcp_centroids_weighted", "vcp_dbscan_blocks_keyed", "vcp_blocks_begin_keyed", "vcp_blocks_begin_keyed_dev",
    "vcp_selftest_horn", "vcp_create_multi", "vcp_destroy_multi", "vcp_multi_last_error", "vcp_multi_count",
    "vcp_multi_ctx", "vcp_dbscan_blocks_multi", "vcp_blocks_share_plan", "vcp_blocks_plan_dev", "vcp_blocks_plan_cuts",
    "vcp_blocks_build_dev", "vcp_blocks_finish_local_dev", "vcp_blocks_finish_zero_dev", "vcp_blocks_finish_zcoords_dev",
    "vcp_blocks_finish_pairs_dev", "vcp_scatter_pairs_dev", "vcp_kdist", "vcp_kdist_dev", "vcp_icp_multistart",
    "vcp_cluster_shapes", "vcp_cluster_shapes_dev", "vcp_cluster_filter", "vcp_cluster_filter_dev",
    "vcp_icp_sums_gated", "vcp_icp_gated", "vcp_icp_sums_trimmed", "vcp_icp_trimmed", "vcp_match_unique", "vcp_match_unique_dev",
    "vcp_register_pairs", "vcp_register_pairs_dev", "vcp_selftest_register_pose", "vcp_register_sim",
    "vcp_register_sim_dev", "vcp_selftest_register_sim_pose", "vcp_eps_tree", "vcp_eps_tree_dev",
    "vcp_gdbscan", "vcp_gdbscan_dev", "vcp_icp_sums_sim", "vcp_selftest_horn_sim", "vcp_icp_sim",
    "vcp_icp_sums_unique", "vcp_icp_unique", "vcp_icp_sums_aniso", "vcp_selftest_horn_aniso", "vcp_icp_aniso",
    "vcp_import_compact", "vcp_import_compact_dev", "vcp_cluster_quantiles", "vcp_cluster_quantiles_dev",
    "vcp_cluster_mad", "vcp_cluster_mad_dev", "vcp_selftest_rank_key", "vcp_parse_scan_text",
    "vcp_parse_scan_text_dev", "vcp_selftest_parse_field", "vcp_format_rows", "vcp_format_rows_dev",
    "vcp_selftest_format_field", "vcp_selftest_format_total_dev", "vcp_selftest_wave_dev",
    "vcp_cluster_moments", "vcp_cluster_moments_dev", "vcp_selftest_sym_eig",
    "vcp_cluster_spheres", "vcp_cluster_spheres_dev", "vcp_selftest_spd_solve",
    "vcp_selftest_poison", "vcp_selftest_scan_generation",
]


class VcpError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("%s (%d): %s" % (STATUS.get(code, "?"), code, msg))
        self.code = code


_lib = None


def lib():
    """Load libvcp.so; raises if the HIP extension has not been built (no fallback)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError("libvcp.so not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
                              "or `make -C vtkcloudpoint_amd/csrc`")
        # One HIP runtime per process: PyTorch-ROCm ships its own libamdhip64 with the same soname as
        # /opt/rocm's.  Whichever loads first serves both; letting torch load first keeps torch.cuda and
        # torch.distributed (RCCL) working next to libvcp in the same process.
        try:
            import torch  # noqa: F401
        except Exception:
            pass
        _lib = C.CDLL(LIB_PATH)
        _lib.vcp_last_error.restype = C.c_char_p
        _lib.vcp_last_error.argtypes = [C.c_void_p]
        _lib.vcp_create.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
        _lib.vcp_destroy.argtypes = [C.c_void_p]
        _lib.vcp_destroy.restype = None
        _lib.vcp_multi_last_error.restype = C.c_char_p
        _lib.vcp_multi_last_error.argtypes = [C.c_void_p]
        _lib.vcp_destroy_multi.argtypes = [C.c_void_p]
        _lib.vcp_destroy_multi.restype = None
        _lib.vcp_multi_ctx.restype = C.c_void_p
        _lib.vcp_multi_ctx.argtypes = [C.c_void_p, C.c_int]
    return _lib


def _ptr(a):
    if a is None:
        return None
    if isinstance(a, int):
        return C.c_void_p(a)
    return C.c_void_p(a.ctypes.data)


def _cluster_rows(pts, labels, weights, dim, ld):
    """The (pts, labels, weights, n, dim, ld) that vcp_cluster_moments and vcp_cluster_spheres take: pts [n, c] float64
    whose rows are read in place at their stride where that is a whole number of doubles (else copied), or with ld given a
    flat buffer; labels and weights int32 [n]."""
    labels = np.ascontiguousarray(labels, np.int32).reshape(-1)
    n = len(labels)
    pts = np.asarray(pts, np.float64)
    if ld is None:
        if pts.ndim != 2 or pts.shape[0] != n:
            raise ValueError("pts must be [n, c] with one row per label")
        dim = pts.shape[1] if dim is None else int(dim)
        if n > 1 and not (pts.strides[1] == 8 and pts.strides[0] % 8 == 0 and pts.strides[0] >= 8 * max(dim, 1)):
            pts = np.ascontiguousarray(pts)
        ld = pts.strides[0] // 8 if n > 1 else max(pts.shape[1], dim)
        if n == 1:
            pts = np.ascontiguousarray(pts)
    else:
        ld, dim = int(ld), int(dim)
        pts = np.ascontiguousarray(pts).reshape(-1)
        if dim in (2, 3) and ld >= dim and n > 0 and len(pts) < (n - 1) * ld + dim:
            raise ValueError("pts has %d doubles for %d rows of %d at ld %d" % (len(pts), n, dim, ld))
    weights = None if weights is None else np.ascontiguousarray(weights, np.int32).reshape(-1)
    if weights is not None and len(weights) != n:
        raise ValueError("weights has %d entries for %d labels" % (len(weights), n))
    return pts, labels, weights, n, dim, ld


def _f64(a, cols=None):
    a = np.ascontiguousarray(a, dtype=np.float64)
    if cols is not None:
        a = a.reshape(-1, cols)
    return a


class Context:
    """One vcp_ctx: one GPU, one stream.  Not thread-safe; create one per thread."""

    def __init__(self, device=0):
        self._h = C.c_void_p()
        rc = lib().vcp_create(int(device), C.byref(self._h))
        if rc != 0:
            raise VcpError(rc, (lib().vcp_last_error(None) or b"").decode())

    _borrowed = False  # True: the handle belongs to a MultiContext (MultiContext.ctx), which destroys it

    def close(self):
        if self._h and not self._borrowed:
            lib().vcp_destroy(self._h)
        self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        if rc != 0:
            raise VcpError(rc, (lib().vcp_last_error(self._h) or b"").decode())

    # -- plumbing ------------------------------------------------------------------------------
    def set_stream(self, stream_handle):
        self._chk(lib().vcp_set_stream(self._h, C.c_void_p(stream_handle)))

    def selftest_scan_dev(self, in_ptr, out_ptr, n, op=0):
        tot = C.c_uint32(0)
        self._chk(lib().vcp_selftest_scan_dev(self._h, C.c_void_p(in_ptr), C.c_void_p(out_ptr), C.c_int64(n), C.c_int(op),
                                              C.byref(tot)))
        return tot.value

    def selftest_poison(self, word, armed=True):
        """Test hook (vcp_selftest_poison): fill the workspace, the pinned scratch and the staging area with the 32-bit
        word and arm the context, so that every later allocation is filled too; armed=False disarms.  Between independent
        calls only.  Returns (bytes of device memory filled, device buffers filled)."""
        nbytes, nbufs = C.c_uint64(0), C.c_int32(0)
        self._chk(lib().vcp_selftest_poison(self._h, C.c_int(1 if armed else 0), C.c_uint32(word & 0xFFFFFFFF),
                                            C.byref(nbytes), C.byref(nbufs)))
        return nbytes.value, nbufs.value

    def selftest_scan_generation(self, gen):
        """Test hook: set the generation number of the scan's descriptors (to reach its 30-bit wrap)."""
        self._chk(lib().vcp_selftest_scan_generation(self._h, C.c_uint32(gen)))

    def release_workspace(self):
        """Free the device workspace kept between calls (it is re-allocated on demand)."""
        self._chk(lib().vcp_release_workspace(self._h))

    def timing_enable(self, on=True):
        self._chk(lib().vcp_timing_enable(self._h, int(on)))

    def timing(self):
        out = []
        name = C.c_char_p()
        ms = C.c_float()
        for i in range(lib().vcp_timing_count(self._h)):
            self._chk(lib().vcp_timing_get(self._h, i, C.byref(name), C.byref(ms)))
            out.append((name.value.decode(), ms.value))
        return out

    # -- DBSCAN --------------------------------------------------------------------------------
    def dbscan(self, coords, eps, min_pts, metric=L1_2D, cf_in=0, in_classed=None, labels=None,
               in_mask=None):
        """Host-buffer entry point.  Returns dict(labels, is_core, is_classed, cf, evals)."""
        coords = _f64(coords)
        if coords.ndim != 2:
            coords = coords.reshape(0, 2)
        n, dim = coords.shape
        if in_classed is not None:
            in_classed = np.ascontiguousarray(in_classed, np.uint8)
            labels = np.array(labels if labels is not None else np.zeros(n), np.int32)
        else:
            labels = np.zeros(n, np.int32)
        if in_mask is not None:
            in_mask = np.ascontiguousarray(in_mask, np.uint8)
        is_core = np.zeros(n, np.uint8)
        is_classed = np.zeros(n, np.uint8)
        cf = C.c_int32(0)
        ev = C.c_int64(0)
        self._chk(lib().vcp_dbscan(self._h, _ptr(coords), C.c_int64(n), int(dim), int(metric),
                                   C.c_double(eps), int(min_pts), C.c_int32(cf_in), _ptr(in_mask),
                                   _ptr(in_classed), _ptr(labels), _ptr(is_core), _ptr(is_classed),
                                   C.byref(cf), C.byref(ev)))
        return dict(labels=labels, is_core=is_core, is_classed=is_classed, cf=cf.value, evals=ev.value)

    def dbscan_dev(self, d_coords, n, dim, eps, min_pts, metric=L1_2D, cf_in=0, d_in_classed=None,
                   d_labels=None, d_is_core=None, d_is_classed=None):
        """Device-pointer entry point (ints from tensor.data_ptr()).  Returns (cf, evals)."""
        cf = C.c_int32(0)
        ev = C.c_int64(0)
        self._chk(lib().vcp_dbscan_dev(self._h, _ptr(d_coords), C.c_int64(n), int(dim), int(metric),
                                       C.c_double(eps), int(min_pts), C.c_int32(cf_in), _ptr(d_in_classed),
                                       _ptr(d_labels), _ptr(d_is_core), _ptr(d_is_classed), C.byref(cf),
                                       C.byref(ev)))
        return cf.value, ev.value

    # -- k-distance ------------------------------------------------------------------------------
    def kdist(self, coords, k, metric=L1_2D, want_knn=False):
        """Exact k-distance of every point (vcp_kdist): returns (kdist [n] float64, knn [n, k] int32 or None).
        kdist[i] <= eps  <=>  dbscan(coords, eps, min_pts=k).is_core[i]."""
        coords = _f64(coords)
        if coords.ndim != 2:
            coords = coords.reshape(0, 2)
        n, dim = coords.shape
        kd = np.zeros(n, np.float64)
        knn = np.zeros((n, max(int(k), 0)), np.int32) if want_knn else None
        self._chk(lib().vcp_kdist(self._h, _ptr(coords), C.c_int64(n), int(dim), int(metric), int(k), _ptr(kd),
                                  _ptr(knn)))
        return kd, knn

    def kdist_dev(self, d_coords, n, dim, k, d_kdist, d_knn=None, metric=L1_2D):
        """Device-pointer form (ints from tensor.data_ptr()); d_knn may be None."""
        self._chk(lib().vcp_kdist_dev(self._h, _ptr(d_coords), C.c_int64(n), int(dim), int(metric), int(k),
                                      _ptr(d_kdist), _ptr(d_knn)))

    # -- eps tree --------------------------------------------------------------------------------
    def eps_tree(self, coords, k, eps_max, metric=L1_2D, kdist=None, want_edges=True):
        """vcp_eps_tree: what dbscan(min_pts=k) decides at every eps <= eps_max.  kdist: an earlier kdist() / eps_tree()
        result for the same coords, metric and k (read as given), or None (computed).  Returns dict(kdist [n], reach [n],
        merge_w [m], merge_a [m], merge_b [m] (None without want_edges), rounds): the minimum spanning forest of the
        mutual-reachability weights in ascending (w, a, b) order."""
        coords = _f64(coords)
        if coords.ndim != 2:
            coords = coords.reshape(0, 2)
        n, dim = coords.shape
        given = kdist is not None
        kd = np.array(kdist, np.float64).reshape(-1) if given else np.zeros(n, np.float64)
        if given and len(kd) != n:
            raise ValueError("kdist has %d entries for %d points" % (len(kd), n))
        reach = np.zeros(n, np.float64)
        cap = max(n - 1, 0)
        mw = np.zeros(max(cap, 1), np.float64)
        ma = np.zeros(max(cap, 1), np.int32) if want_edges else None
        mb = np.zeros(max(cap, 1), np.int32) if want_edges else None
        m, rounds = C.c_int64(0), C.c_int32(0)
        self._chk(lib().vcp_eps_tree(self._h, _ptr(coords), C.c_int64(n), int(dim), int(metric), int(k),
                                     C.c_double(eps_max), int(given), _ptr(kd), _ptr(reach), C.byref(m), _ptr(mw),
                                     _ptr(ma), _ptr(mb), C.byref(rounds)))
        m = m.value
        return dict(kdist=kd, reach=reach, merge_w=mw[:m].copy(), merge_a=None if ma is None else ma[:m].copy(),
                    merge_b=None if mb is None else mb[:m].copy(), rounds=rounds.value)

    def eps_tree_dev(self, d_coords, n, dim, k, eps_max, d_merge_w, d_merge_a=None, d_merge_b=None, d_kdist=None,
                     d_reach=None, kdist_given=False, metric=L1_2D):
        """Device-pointer form (ints from tensor.data_ptr()); d_merge_* have room for max(n - 1, 0) entries, d_kdist
        (read when kdist_given) and d_reach may be None.  Returns (n_merge, rounds)."""
        m, rounds = C.c_int64(0), C.c_int32(0)
        self._chk(lib().vcp_eps_tree_dev(self._h, _ptr(d_coords), C.c_int64(n), int(dim), int(metric), int(k),
                                         C.c_double(eps_max), int(bool(kdist_given)), _ptr(d_kdist), _ptr(d_reach),
                                         C.byref(m), _ptr(d_merge_w), _ptr(d_merge_a), _ptr(d_merge_b),
                                         C.byref(rounds)))
        return m.value, rounds.value

    # -- generalised DBSCAN ----------------------------------------------------------------------
    def gdbscan(self, coords, eps, min_weight, metric=L1_2D, weights=None, aux=None, gate=None, cf_in=0,
                want_wsum=False):
        """vcp_gdbscan: DBSCAN in which row j counts weights[j] times (None: once) and two rows are neighbours only when
        their aux values are within gate as well (aux None: no second test).  Returns dict(labels, is_core, cf, wsum):
        wsum [n] int64 = the weight of every row's neighbourhood with want_wsum, else None."""
        coords = _f64(coords)
        if coords.ndim != 2:
            coords = coords.reshape(0, 2)
        n, dim = coords.shape
        if weights is not None:
            weights = np.ascontiguousarray(weights, np.int32).reshape(-1)
            if len(weights) != n:
                raise ValueError("weights has %d entries for %d points" % (len(weights), n))
        if aux is not None:
            if gate is None:
                raise ValueError("aux needs a gate")
            aux = _f64(aux).reshape(-1)
            if len(aux) != n:
                raise ValueError("aux has %d entries for %d points" % (len(aux), n))
        labels = np.zeros(n, np.int32)
        is_core = np.zeros(n, np.uint8)
        wsum = np.zeros(n, np.int64) if want_wsum else None
        cf = C.c_int32(0)
        self._chk(lib().vcp_gdbscan(self._h, _ptr(coords), C.c_int64(n), int(dim), int(metric), C.c_double(eps),
                                    _ptr(aux), C.c_double(0.0 if gate is None else gate), _ptr(weights),
                                    C.c_int64(int(min_weight)), C.c_int32(cf_in), _ptr(labels), _ptr(is_core),
                                    _ptr(wsum), C.byref(cf)))
        return dict(labels=labels, is_core=is_core, cf=cf.value, wsum=wsum)

    def gdbscan_dev(self, d_coords, n, dim, eps, min_weight, d_labels, metric=L1_2D, d_weights=None, d_aux=None,
                    gate=0.0, cf_in=0, d_is_core=None, d_wsum=None):
        """Device-pointer form (ints from tensor.data_ptr()): d_weights int32 [n], d_aux float64 [n], d_is_core uint8 [n]
        and d_wsum int64 [n] may be None.  Returns cf."""
        cf = C.c_int32(0)
        self._chk(lib().vcp_gdbscan_dev(self._h, _ptr(d_coords), C.c_int64(n), int(dim), int(metric), C.c_double(eps),
                                        _ptr(d_aux), C.c_double(gate), _ptr(d_weights), C.c_int64(int(min_weight)),
                                        C.c_int32(cf_in), _ptr(d_labels), _ptr(d_is_core), _ptr(d_wsum), C.byref(cf)))
        return cf.value

    # -- ICP -----------------------------------------------------------------------------------
    def icp(self, model, data, tol=1e-4, max_iter=100, stop_rule=STOP_SSE_DELTA):
        model = _f64(model, 3)
        data = _f64(data, 3)
        R = np.zeros(9)
        T = np.zeros(3)
        sse, rmse, it = C.c_double(0), C.c_double(0), C.c_int32(0)
        self._chk(lib().vcp_icp(self._h, _ptr(model), C.c_int64(len(model)), _ptr(data), C.c_int64(len(data)),
                                C.c_double(tol), int(max_iter), int(stop_rule), _ptr(R), _ptr(T),
                                C.byref(sse), C.byref(rmse), C.byref(it)))
        return dict(R=R.reshape(3, 3), T=T, sse=sse.value, rmse=rmse.value, iters=it.value)

    def icp_dev(self, d_model, nm, d_data, nd, tol=1e-4, max_iter=100, stop_rule=STOP_SSE_DELTA):
        R = np.zeros(9)
        T = np.zeros(3)
        sse, rmse, it = C.c_double(0), C.c_double(0), C.c_int32(0)
        self._chk(lib().vcp_icp_dev(self._h, _ptr(d_model), C.c_int64(nm), _ptr(d_data), C.c_int64(nd),
                                    C.c_double(tol), int(max_iter), int(stop_rule), _ptr(R), _ptr(T),
                                    C.byref(sse), C.byref(rmse), C.byref(it)))
        return dict(R=R.reshape(3, 3), T=T, sse=sse.value, rmse=rmse.value, iters=it.value)

    def _icp_sums(self, fn, model, data, R, T, ncol, want_nn, want_keep, call):
        """One call of a vcp_icp_sums* entry point fn.  call(head, sums, nn, keep) lays out fn's arguments: head is the
        common leading ones, sums [ncol] / nn / keep the output arrays as C pointers (NULL where not wanted).  Returns
        (sums, nn [nd] int32 or None, keep [nd] uint8 or None)."""
        model = _f64(model, 3)
        data = _f64(data, 3)
        R = None if R is None else _f64(R).reshape(9)
        T = None if T is None else _f64(T).reshape(3)
        sums = np.zeros(ncol)
        nn = np.zeros(len(data), np.int32) if want_nn else None
        keep = np.zeros(len(data), np.uint8) if want_keep else None
        head = (self._h, _ptr(model), C.c_int64(len(model)), _ptr(data), C.c_int64(len(data)), _ptr(R), _ptr(T))
        self._chk(fn(*call(head, _ptr(sums), _ptr(nn), _ptr(keep))))
        return sums, nn, keep

    def icp_sums(self, model, data, R=None, T=None, want_nn=True):
        sums, nn, _ = self._icp_sums(lib().vcp_icp_sums, model, data, R, T, 16, want_nn, False,
                                     lambda head, sums, nn, keep: head + (sums, nn))
        return sums, nn

    def icp_sums_gated(self, model, data, gate, R=None, T=None, want_nn=True, want_keep=True):
        """One gated pass (vcp_icp_sums_gated): pairs with sqrt(dd) >= gate add +0.0 at their place in icp_sums's
        tree.  Returns (sums [16], kept, nn [nd] int32 or None, keep [nd] uint8 or None)."""
        kept = C.c_int64(0)
        sums, nn, keep = self._icp_sums(
            lib().vcp_icp_sums_gated, model, data, R, T, 16, want_nn, want_keep,
            lambda head, sums, nn, keep: head + (C.c_double(gate), sums, C.byref(kept), nn, keep))
        return sums, kept.value, nn, keep

    def icp_sums_sim(self, model, data, gate, R=None, T=None, want_nn=True, want_keep=True):
        """One pass of the similarity form (vcp_icp_sums_sim): icp_sums_gated with sum |p|^2 at 16 and sum |y|^2 at 17
        over the kept pairs, through the same tree.  Returns (sums [18], kept, nn [nd] int32 or None, keep [nd] uint8 or
        None)."""
        kept = C.c_int64(0)
        sums, nn, keep = self._icp_sums(
            lib().vcp_icp_sums_sim, model, data, R, T, 18, want_nn, want_keep,
            lambda head, sums, nn, keep: head + (C.c_double(gate), sums, C.byref(kept), nn, keep))
        return sums, kept.value, nn, keep

    def icp_sums_aniso(self, model, data, gate, A=None, T=None, want_nn=True, want_keep=True):
        """One pass of the anisotropic form (vcp_icp_sums_aniso): the pair, the distance and the gate are icp_sums_gated's
        under the pose p = A d + T, but columns 0:3 and 6:15 sum the raw landmark d in p's place, 16 is sum d0*d0 and 17
        sum d1*d1 over the kept pairs.  Returns (sums [18], kept, nn [nd] int32 or None, keep [nd] uint8 or None)."""
        kept = C.c_int64(0)
        sums, nn, keep = self._icp_sums(
            lib().vcp_icp_sums_aniso, model, data, A, T, 18, want_nn, want_keep,
            lambda head, sums, nn, keep: head + (C.c_double(gate), sums, C.byref(kept), nn, keep))
        return sums, kept.value, nn, keep

    def icp_sums_trimmed(self, model, data, m, R=None, T=None, want_nn=True, want_keep=True):
        """One trimmed round's passes (vcp_icp_sums_trimmed): the m pairs with the smallest keys [K(dd) | index] are
        kept, the others add +0.0 at their place in icp_sums's tree.  Returns (sums [16], thr_dd = the dd of the kept
        pair with the largest key, nn [nd] int32 or None, keep [nd] uint8 or None)."""
        thr = C.c_double(0)
        sums, nn, keep = self._icp_sums(
            lib().vcp_icp_sums_trimmed, model, data, R, T, 16, want_nn, want_keep,
            lambda head, sums, nn, keep: head + (C.c_int64(int(m)), sums, C.byref(thr), nn, keep))
        return sums, thr.value, nn, keep

    def icp_sums_unique(self, model, data, gate, R=None, T=None, want_nn=True, want_keep=True):
        """One unique-correspondence round's passes (vcp_icp_sums_unique): of the pairs that share a nearest model point
        only the one with the smallest key [K(dd) | index] may be kept, and it is kept unless sqrt(dd) >= gate; the
        others add +0.0 at their place in icp_sums's tree.  Returns (sums [16], kept, lost = the pairs that are not
        their model point's winner, nn [nd] int32 or None, keep [nd] uint8 or None: 1 kept, 0 winner dropped by the
        gate, 2 not the winner)."""
        kept = C.c_int64(0)
        lost = C.c_int64(0)
        sums, nn, keep = self._icp_sums(
            lib().vcp_icp_sums_unique, model, data, R, T, 16, want_nn, want_keep,
            lambda head, sums, nn, keep: head + (C.c_double(gate), sums, C.byref(kept), nn, keep, C.byref(lost)))
        return sums, kept.value, lost.value, nn, keep

    # -- centroids / merge / match -----------------------------------------------------------------
    def centroids(self, xyz, motor, labels, K):
        """Tools.GetClusList: returns (c3 [K,3], c2 [K,2], counts [K]); empty clusters are NaN rows."""
        xyz = None if xyz is None else _f64(xyz, 3)
        motor = None if motor is None else _f64(motor, 2)
        labels = np.ascontiguousarray(labels, np.int32)
        c3 = np.full((K, 3), np.nan)
        c2 = np.full((K, 2), np.nan)
        counts = np.zeros(K, np.int64)
        self._chk(lib().vcp_centroids(self._h, _ptr(xyz), _ptr(motor), _ptr(labels), C.c_int64(len(labels)),
                                      C.c_int32(K), _ptr(c3), _ptr(c2), _ptr(counts)))
        return c3, c2, counts

    def centroids_weighted(self, xyz, group, cluster_id, pts_count, K, ignore_duplication):
        """Tools.getFixedPtsCentroid: returns (c3 [K,3], inside_num [K])."""
        xyz = _f64(xyz, 3)
        group = np.ascontiguousarray(group, np.int32)
        cluster_id = None if cluster_id is None else np.ascontiguousarray(cluster_id, np.int32)
        pts_count = np.ascontiguousarray(pts_count, np.int32)
        c3 = np.zeros((K, 3))
        inside = np.zeros(K, np.int64)
        self._chk(lib().vcp_centroids_weighted(self._h, _ptr(xyz), _ptr(group), _ptr(cluster_id), _ptr(pts_count),
                                               C.c_int64(len(group)), C.c_int32(K), int(bool(ignore_duplication)),
                                               _ptr(c3), _ptr(inside)))
        return c3, inside

    def centroids_dev(self, d_xyz, d_motor, d_labels, n, K, d_c3, d_c2, d_counts):
        """Device-pointer form of centroids (any of d_xyz / d_motor and its output may be None)."""
        self._chk(lib().vcp_centroids_dev(self._h, _ptr(d_xyz), _ptr(d_motor), _ptr(d_labels), C.c_int64(n),
                                          C.c_int32(K), _ptr(d_c3), _ptr(d_c2), _ptr(d_counts)))

    def merge_centroids(self, cxy, ids, thr):
        cxy = _f64(cxy, 2)
        ids = np.ascontiguousarray(ids, np.int32)
        K = len(ids)
        map_to = np.zeros(K, np.int32)
        mc = C.c_int32(0)
        self._chk(lib().vcp_merge_centroids(self._h, _ptr(cxy), _ptr(ids), C.c_int32(K), C.c_double(thr),
                                            _ptr(map_to), C.byref(mc)))
        return map_to, mc.value

    def refresh_by_dictionary(self, xyz, motor, labels, K, map_by_id):
        xyz = _f64(xyz, 3)
        motor = _f64(motor, 2)
        labels = np.array(labels, np.int32)
        map_by_id = np.ascontiguousarray(map_by_id, np.int32)
        c3 = np.zeros((K, 3))
        c2 = np.zeros((K, 2))
        counts = np.zeros(K, np.int64)
        nk = C.c_int32(0)
        self._chk(lib().vcp_refresh_by_dictionary(self._h, _ptr(xyz), _ptr(motor), _ptr(labels),
                                                  C.c_int64(len(labels)), C.c_int32(K), _ptr(map_by_id),
                                                  C.byref(nk), _ptr(c3), _ptr(c2), _ptr(counts)))
        k = nk.value
        return labels, k, c3[:k], c2[:k], counts[:k]

    def match(self, centers, truths, M, max_dist):
        centers = _f64(centers, 3)
        truths = _f64(truths, 3)
        M = _f64(M).reshape(16)
        K, T = len(centers), len(truths)
        mxyz = np.zeros((K, 3))
        is_m = np.zeros(K, np.uint8)
        nearest = np.zeros(K, np.int32)
        nd = np.zeros(K)
        cnt = C.c_int32(0)
        self._chk(lib().vcp_match(self._h, _ptr(centers), C.c_int32(K), _ptr(truths), C.c_int32(T), _ptr(M),
                                  C.c_double(max_dist), _ptr(mxyz), _ptr(is_m), _ptr(nearest), _ptr(nd),
                                  C.byref(cnt)))
        return dict(matched_xyz=mxyz, is_matched=is_m, nearest=nearest, nearest_dist=nd, count=cnt.value)

    def match_unique(self, centers, truths, M, max_dist):
        """vcp_match_unique: the one-to-one pairing of the greedy walk over (d, j, i).  Returns dict(matched_xyz [K,3],
        truth_of [K] (-1 = none), center_of [T] (-1 = none), pair_dist [K] (+inf = none), count, rounds)."""
        centers = _f64(centers, 3)
        truths = _f64(truths, 3)
        M = _f64(M).reshape(16)
        K, T = len(centers), len(truths)
        mxyz = np.zeros((K, 3))
        truth_of = np.full(K, -1, np.int32)
        center_of = np.full(T, -1, np.int32)
        pd = np.full(K, np.inf)
        cnt, rounds = C.c_int32(0), C.c_int32(0)
        self._chk(lib().vcp_match_unique(self._h, _ptr(centers), C.c_int32(K), _ptr(truths), C.c_int32(T), _ptr(M),
                                         C.c_double(max_dist), _ptr(mxyz), _ptr(truth_of), _ptr(center_of), _ptr(pd),
                                         C.byref(cnt), C.byref(rounds)))
        return dict(matched_xyz=mxyz, truth_of=truth_of, center_of=center_of, pair_dist=pd, count=cnt.value,
                    rounds=rounds.value)

    def match_unique_dev(self, d_centers, K, d_truths, T, M, max_dist, d_truth_of, d_center_of, d_pair_dist=None,
                         d_matched_xyz=None):
        """Device-pointer form (ints from tensor.data_ptr()); M is a host array.  The arrays are written in place; returns
        the same dict with the pointers passed in and count, rounds."""
        M = _f64(M).reshape(16)
        cnt, rounds = C.c_int32(0), C.c_int32(0)
        self._chk(lib().vcp_match_unique_dev(self._h, _ptr(d_centers), C.c_int32(K), _ptr(d_truths), C.c_int32(T), _ptr(M),
                                             C.c_double(max_dist), _ptr(d_matched_xyz), _ptr(d_truth_of),
                                             _ptr(d_center_of), _ptr(d_pair_dist), C.byref(cnt), C.byref(rounds)))
        return dict(matched_xyz=d_matched_xyz, truth_of=d_truth_of, center_of=d_center_of, pair_dist=d_pair_dist,
                    count=cnt.value, rounds=rounds.value)

    # -- block-partitioned pipeline ------------------------------------------------------------------
    def dbscan_blocks(self, motor, eps, min_pts, pts_in_cell, small_max=3, key_xy=None):
        """MainForm.getClusterFromMotor + StartCode + CompleteWork3 in one call (host buffers).  key_xy: the (X, Y)
        the partition of the twin getClusterFromList reads (FrmMain.cs:1136-1213); None = the motor coordinates."""
        motor = _f64(motor, 2)
        n = len(motor)
        key_xy = None if key_xy is None else _f64(key_xy, 2)
        labels = np.zeros(n, np.int32)
        block_of = np.zeros(n, np.int32)
        order = np.zeros(max(n, 1), np.int64)
        m = C.c_int64(0)
        rows, cols, kept, dels, ca = (C.c_int32(0) for _ in range(5))
        ev = C.c_int64(0)
        self._chk(lib().vcp_dbscan_blocks_keyed(self._h, _ptr(key_xy), _ptr(motor), C.c_int64(n), C.c_double(eps),
                                                int(min_pts), int(pts_in_cell), int(small_max), _ptr(labels),
                                                _ptr(block_of), _ptr(order), C.byref(m), C.byref(rows), C.byref(cols),
                                                C.byref(kept), C.byref(dels), C.byref(ca), C.byref(ev)))
        return dict(labels=labels, block_of=block_of, order=order[: m.value].copy(), rows=rows.value,
                    cols=cols.value, kept=kept.value, del_sum=dels.value, cluster_amount=ca.value,
                    evals=ev.value)

    def blocks_begin(self, motor, eps, min_pts, pts_in_cell, small_max=3, device_ptr=None, n=None, key_xy=None,
                     key_device_ptr=None):
        rows, cols = C.c_int32(0), C.c_int32(0)
        nb, m = C.c_int64(0), C.c_int64(0)
        if key_xy is not None or key_device_ptr is not None:  # getClusterFromList: partition on (X, Y)
            if device_ptr is None:
                motor, key_xy = _f64(motor, 2), _f64(key_xy, 2)
                self._chk(lib().vcp_blocks_begin_keyed(self._h, _ptr(key_xy), _ptr(motor), C.c_int64(len(motor)),
                                                       C.c_double(eps), int(min_pts), int(pts_in_cell), int(small_max),
                                                       C.byref(rows), C.byref(cols), C.byref(nb), C.byref(m)))
            else:
                self._chk(lib().vcp_blocks_begin_keyed_dev(self._h, _ptr(key_device_ptr), _ptr(device_ptr), C.c_int64(n),
                                                           C.c_double(eps), int(min_pts), int(pts_in_cell),
                                                           int(small_max), C.byref(rows), C.byref(cols), C.byref(nb),
                                                           C.byref(m)))
        elif device_ptr is None:
            motor = _f64(motor, 2)
            self._chk(lib().vcp_blocks_begin(self._h, _ptr(motor), C.c_int64(len(motor)), C.c_double(eps),
                                             int(min_pts), int(pts_in_cell), int(small_max), C.byref(rows),
                                             C.byref(cols), C.byref(nb), C.byref(m)))
        else:
            self._chk(lib().vcp_blocks_begin_dev(self._h, _ptr(device_ptr), C.c_int64(n), C.c_double(eps),
                                                 int(min_pts), int(pts_in_cell), int(small_max), C.byref(rows),
                                                 C.byref(cols), C.byref(nb), C.byref(m)))
        return dict(rows=rows.value, cols=cols.value, nblocks=nb.value, m=m.value)

    def blocks_share(self, rank, world):
        lo, hi = C.c_int32(0), C.c_int32(0)
        plo, phi = C.c_int64(0), C.c_int64(0)
        self._chk(lib().vcp_blocks_share(self._h, int(rank), int(world), C.byref(lo), C.byref(hi), C.byref(plo),
                                         C.byref(phi)))
        return lo.value, hi.value, plo.value, phi.value

    def blocks_cluster_dev(self, block_lo, block_hi, d_local):
        ev = C.c_int64(0)
        self._chk(lib().vcp_blocks_cluster_dev(self._h, C.c_int32(block_lo), C.c_int32(block_hi), _ptr(d_local),
                                               C.byref(ev)))
        return ev.value

    def blocks_finish_dev(self, d_local, evals_blocks, d_labels, d_block_of=None, d_merge_order=None):
        m = C.c_int64(0)
        kept, dels, ca = (C.c_int32(0) for _ in range(3))
        ev = C.c_int64(0)
        self._chk(lib().vcp_blocks_finish_dev(self._h, _ptr(d_local), C.c_int64(evals_blocks), _ptr(d_labels),
                                              _ptr(d_block_of), _ptr(d_merge_order), C.byref(m), C.byref(kept),
                                              C.byref(dels), C.byref(ca), C.byref(ev)))
        return dict(m=m.value, kept=kept.value, del_sum=dels.value, cluster_amount=ca.value, evals=ev.value)

    # -- the block pipeline with every stage sharded (include/vcp.h; driver: distributed.sharded_pipeline) -----------
    def blocks_plan(self, d_motor, n, eps, min_pts, pts_in_cell, small_max=3, d_key=None):
        """The streaming passes that decide the partition (identical on every rank).  d_* are device pointers."""
        rows, cols = C.c_int32(0), C.c_int32(0)
        nb, ns = C.c_int64(0), C.c_int64(0)
        self._chk(lib().vcp_blocks_plan_dev(self._h, _ptr(d_key), _ptr(d_motor), C.c_int64(n), C.c_double(eps),
                                            int(min_pts), int(pts_in_cell), int(small_max), C.byref(rows), C.byref(cols),
                                            C.byref(nb), C.byref(ns)))
        return dict(rows=rows.value, cols=cols.value, nblocks=nb.value, nsuper=ns.value)

    def blocks_plan_cuts(self, world):
        cuts = (C.c_int64 * (world + 1))()
        self._chk(lib().vcp_blocks_plan_cuts(self._h, int(world), cuts))
        return [int(c) for c in cuts]

    def blocks_build(self, super_lo, super_hi):
        lo, hi = C.c_int32(0), C.c_int32(0)
        m, nl = C.c_int64(0), C.c_int64(0)
        self._chk(lib().vcp_blocks_build_dev(self._h, C.c_int64(super_lo), C.c_int64(super_hi), C.byref(lo), C.byref(hi),
                                             C.byref(m), C.byref(nl)))
        return dict(block_lo=lo.value, block_hi=hi.value, m=m.value, n_loc=nl.value)

    def blocks_finish_local(self, d_local):
        info = (C.c_int64 * 8)()
        self._chk(lib().vcp_blocks_finish_local_dev(self._h, _ptr(d_local), info))
        keys = ("clusters", "kept", "err", "req", "nonempty", "last_nonzero", "m", "n_loc")
        return dict(zip(keys, (int(v) for v in info)))

    def blocks_finish_zero(self, zero_last):
        """-> (points of the share's zero list, those of them the noise pass can reach: the ones it runs over)"""
        z, a = C.c_int64(0), C.c_int64(0)
        self._chk(lib().vcp_blocks_finish_zero_dev(self._h, int(bool(zero_last)), C.byref(z), C.byref(a)))
        return z.value, a.value

    def blocks_finish_zcoords(self, d_zcoords, swap_xy=True):
        self._chk(lib().vcp_blocks_finish_zcoords_dev(self._h, int(bool(swap_xy)), _ptr(d_zcoords)))

    def blocks_finish_pairs(self, kept_offset, d_zlab, d_pairs):
        self._chk(lib().vcp_blocks_finish_pairs_dev(self._h, C.c_int32(kept_offset), _ptr(d_zlab), _ptr(d_pairs)))

    def scatter_pairs(self, d_pairs, count, n, d_labels):
        self._chk(lib().vcp_scatter_pairs_dev(self._h, _ptr(d_pairs), C.c_int64(count), C.c_int64(n), _ptr(d_labels)))

    # -- exact DBSCAN over several GPUs: staged engine (all d_* are device pointers) --------------------
    def slab_begin(self, d_coords, n, dim, metric, eps, min_pts, d_noexpand, d_ord, d_rep, d_is_core=None):
        """Grid, core flags and local components of own + halo points; returns the number of local components."""
        nc = C.c_int64(0)
        self._chk(lib().vcp_slab_begin(self._h, _ptr(d_coords), C.c_int64(n), C.c_int(dim), C.c_int(int(metric)),
                                       C.c_double(eps), C.c_int(min_pts), _ptr(d_noexpand), _ptr(d_ord), _ptr(d_rep),
                                       _ptr(d_is_core), C.byref(nc)))
        self._slab_ncomp = nc.value
        return nc.value

    def slab_comps(self):
        """Seeds (smallest global list position) of the local components, ascending."""
        out = np.zeros(self._slab_ncomp, np.uint32)
        self._chk(lib().vcp_slab_comps(self._h, _ptr(out)))
        out.sort()
        return out

    def slab_finish(self, map_rep, map_k, tab_gid, tab_seed, own_lo, own_count, d_labels, d_is_classed=None):
        """Border rule and labels from the resolved global clusters; returns the `twice` count of own points."""
        map_rep = np.ascontiguousarray(map_rep, np.uint32)
        map_k = np.ascontiguousarray(map_k, np.uint32)
        tab_gid = np.ascontiguousarray(tab_gid, np.int32)
        tab_seed = np.ascontiguousarray(tab_seed, np.uint32)
        tw = C.c_int64(0)
        self._chk(lib().vcp_slab_finish(self._h, _ptr(map_rep), _ptr(map_k), C.c_int64(len(tab_gid)), _ptr(tab_gid),
                                        _ptr(tab_seed), C.c_uint32(own_lo), C.c_uint32(own_count), _ptr(d_labels),
                                        _ptr(d_is_classed), C.byref(tw)))
        return tw.value

    def mcc(self, xy, labels, K, order=None):
        """Tools.getCircles: minimal bounding circle of every cluster with more than 3 points."""
        xy = _f64(xy, 2)
        labels = np.ascontiguousarray(labels, np.int32)
        order = None if order is None else np.ascontiguousarray(order, np.int64)
        n = len(labels)
        m = n if order is None else len(order)
        centers = np.zeros((K, 2))
        radius = np.zeros(K)
        valid = np.zeros(K, np.uint8)
        hn = np.zeros(K, np.int32)
        self._chk(lib().vcp_mcc(self._h, _ptr(xy), _ptr(labels), _ptr(order), C.c_int64(m), C.c_int64(n), C.c_int32(K),
                                _ptr(centers), _ptr(radius), _ptr(valid), _ptr(hn)))
        return dict(centers=centers, radius=radius, valid=valid, hull_n=hn)

    # -- cluster shapes and the radius / aspect filter -------------------------------------------------
    def cluster_shapes(self, xy, labels, K, order=None, rect=True, hull=True):
        """vcp_cluster_shapes: hull, minimal bounding circle and minimum-area bounding rectangle of every cluster.
        Returns mcc()'s dict plus rect_xy [K,4,2], rect_len [K,2], rect_edge [K], rect_valid [K] (rect) and hull_off
        [K+1], hull_idx [hull_off[K]] = indices into xy (hull)."""
        xy = _f64(xy, 2)
        labels = np.ascontiguousarray(labels, np.int32)
        order = None if order is None else np.ascontiguousarray(order, np.int64)
        n = len(labels)
        m = n if order is None else len(order)
        centers = np.zeros((K, 2))
        radius = np.zeros(K)
        valid = np.zeros(K, np.uint8)
        hn = np.zeros(K, np.int32)
        rxy = np.zeros((K, 4, 2)) if rect else None
        rlen = np.zeros((K, 2)) if rect else None
        redge = np.full(K, -1, np.int32) if rect else None
        rval = np.zeros(K, np.uint8) if rect else None
        hoff = np.zeros(K + 1, np.int32) if hull else None
        hidx = np.zeros(max(m, 1), np.int32) if hull else None
        self._chk(lib().vcp_cluster_shapes(self._h, _ptr(xy), _ptr(labels), _ptr(order), C.c_int64(m), C.c_int64(n),
                                           C.c_int32(K), _ptr(centers), _ptr(radius), _ptr(valid), _ptr(hn), _ptr(rxy),
                                           _ptr(rlen), _ptr(redge), _ptr(rval), _ptr(hoff), _ptr(hidx)))
        out = dict(centers=centers, radius=radius, valid=valid, hull_n=hn)
        if rect:
            out.update(rect_xy=rxy, rect_len=rlen, rect_edge=redge, rect_valid=rval)
        if hull:
            out.update(hull_off=hoff, hull_idx=hidx[: hoff[K]].copy())
        return out

    def cluster_shapes_dev(self, d_xy, d_labels, d_order, m, n, K, d_centers, d_radius, d_valid, d_hull_n=None,
                           d_rect_xy=None, d_rect_len=None, d_rect_edge=None, d_rect_valid=None, d_hull_off=None,
                           d_hull_idx=None):
        """Device-pointer form (ints from tensor.data_ptr()); the outputs after d_valid may be None."""
        self._chk(lib().vcp_cluster_shapes_dev(self._h, _ptr(d_xy), _ptr(d_labels), _ptr(d_order), C.c_int64(m),
                                               C.c_int64(n), C.c_int32(K), _ptr(d_centers), _ptr(d_radius), _ptr(d_valid),
                                               _ptr(d_hull_n), _ptr(d_rect_xy), _ptr(d_rect_len), _ptr(d_rect_edge),
                                               _ptr(d_rect_valid), _ptr(d_hull_off), _ptr(d_hull_idx)))

    def cluster_filter(self, labels, K, radius, valid, rect_len=None, rect_valid=None, max_radius=np.inf,
                       max_aspect=np.inf):
        """vcp_cluster_filter: dict(filtered [K], keep [n], kept_idx [n_kept], n_filtered, n_kept)."""
        labels = np.ascontiguousarray(labels, np.int32)
        n = len(labels)
        radius = _f64(radius)
        valid = np.ascontiguousarray(valid, np.uint8)
        rect_len = None if rect_len is None else _f64(rect_len, 2)
        rect_valid = None if rect_valid is None else np.ascontiguousarray(rect_valid, np.uint8)
        filtered = np.zeros(K, np.uint8)
        keep = np.zeros(n, np.uint8)
        kept = np.zeros(max(n, 1), np.int32)
        nf, nk = C.c_int32(0), C.c_int64(0)
        self._chk(lib().vcp_cluster_filter(self._h, _ptr(labels), C.c_int64(n), C.c_int32(K), _ptr(radius), _ptr(valid),
                                           _ptr(rect_len), _ptr(rect_valid), C.c_double(max_radius),
                                           C.c_double(max_aspect), _ptr(filtered), _ptr(keep), _ptr(kept), C.byref(nf),
                                           C.byref(nk)))
        return dict(filtered=filtered, keep=keep, kept_idx=kept[: nk.value].copy(), n_filtered=nf.value, n_kept=nk.value)

    def cluster_filter_dev(self, d_labels, n, K, d_radius, d_valid, d_rect_len, d_rect_valid, max_radius, max_aspect,
                           d_filtered, d_keep=None, d_kept_idx=None):
        """Device-pointer form; returns (n_filtered, n_kept)."""
        nf, nk = C.c_int32(0), C.c_int64(0)
        self._chk(lib().vcp_cluster_filter_dev(self._h, _ptr(d_labels), C.c_int64(n), C.c_int32(K), _ptr(d_radius),
                                               _ptr(d_valid), _ptr(d_rect_len), _ptr(d_rect_valid),
                                               C.c_double(max_radius), C.c_double(max_aspect), _ptr(d_filtered),
                                               _ptr(d_keep), _ptr(d_kept_idx), C.byref(nf), C.byref(nk)))
        return nf.value, nk.value

    def assign_truths(self, motor, truths_xy, truth_ids, radius):
        """MainForm.refreshClusList: (ids [n], number of points with no truth within radius)."""
        motor = _f64(motor, 2)
        truths_xy = _f64(truths_xy, 2)
        truth_ids = np.ascontiguousarray(truth_ids, np.int32)
        ids = np.zeros(len(motor), np.int32)
        out = C.c_int64(0)
        self._chk(lib().vcp_assign_truths(self._h, _ptr(motor), C.c_int64(len(motor)), _ptr(truths_xy), _ptr(truth_ids),
                                          C.c_int32(len(truth_ids)), C.c_double(radius), _ptr(ids), C.byref(out)))
        return ids, out.value

    def icp_vtklike(self, source, target, max_iter=100, max_landmarks=200, start_by_centroids=True):
        """MainForm.ICP() (FrmMain.cs:841-907) without VTK: returns dict(M 4x4, mean_dist, iters)."""
        source = _f64(source, 3)
        target = _f64(target, 3)
        M = np.zeros(16)
        md = C.c_double(0)
        it = C.c_int32(0)
        self._chk(lib().vcp_icp_vtklike(self._h, _ptr(source), C.c_int64(len(source)), _ptr(target),
                                        C.c_int64(len(target)), int(max_iter), int(max_landmarks),
                                        int(start_by_centroids), _ptr(M), C.byref(md), C.byref(it)))
        return dict(M=M.reshape(4, 4), mean_dist=md.value, iters=it.value)

    @staticmethod
    def _icp_poses(poses, init_T):
        """The pose arguments of the multi-start entry points -> (H, init_R [H, 9] or None, init_T [H, 3] or None)."""
        if isinstance(poses, (int, np.integer)):
            H, init_R = int(poses), None
        else:
            init_R = _f64(poses).reshape(-1, 9)
            H = len(init_R)
        if init_T is not None:
            init_T = _f64(init_T, 3)
            if len(init_T) != H:
                raise ValueError("init_T has %d rows for %d poses" % (len(init_T), H))
        return H, init_R, init_T

    def _icp_starts(self, fn, source, target, poses, init_T, max_iter, max_landmarks, form_args, inlier_dist, extra=(),
                    start_args=()):
        """One call of a multi-start entry point fn: the common arguments, form_args (arrays or C values) between
        max_landmarks and inlier_dist, the common outputs, then one [H] array per (key, dtype) of extra -- [H, cols] per
        (key, dtype, cols).  start_args (arrays or None) go between init_T and max_iter.  Returns the result dict."""
        source = _f64(source, 3)
        target = _f64(target, 3)
        H, init_R, init_T = self._icp_poses(poses, init_T)
        n = max(H, 0)
        M = np.zeros(16)
        M_all = np.zeros((n, 16))
        md = np.zeros(n)
        inl = np.zeros(n, np.int32)
        best = C.c_int32(0)
        more = [(e[0], np.zeros((n,) + tuple(e[2:]), e[1])) for e in extra]
        c_args = [_ptr(a) if isinstance(a, np.ndarray) else a for a in form_args]  # form_args keeps the arrays alive
        self._chk(fn(self._h, _ptr(source), C.c_int64(len(source)), _ptr(target), C.c_int64(len(target)), C.c_int32(H),
                     _ptr(init_R), _ptr(init_T), *[_ptr(a) for a in start_args], int(max_iter), int(max_landmarks),
                     *c_args, C.c_double(inlier_dist),
                     _ptr(M), C.byref(best), _ptr(M_all), _ptr(md), _ptr(inl), *[_ptr(a) for _, a in more]))
        return dict(best=best.value, M=M.reshape(4, 4), M_all=M_all.reshape(n, 4, 4), mean_dist=md, inliers=inl,
                    **dict(more))

    _ICP_COUNTED = (("kept", np.int64), ("starved", np.int32))  # what every counted form returns per pose

    @staticmethod
    def _icp_schedule(sched, min_pairs):
        """A counted form's schedule (gates or keep shares) and min_pairs as form_args of _icp_starts."""
        sched = _f64(sched).reshape(-1)
        return sched, C.c_int32(len(sched)), C.c_int32(min_pairs)

    def icp_multistart(self, source, target, poses=36, init_T=None, max_iter=100, max_landmarks=200,
                       inlier_dist=np.inf):
        """icp_vtklike (centroid start) from H start rotations in one call, scored by inliers (vcp_icp_multistart).
        poses: an int H (the library's Rz(h * 2 pi / H), h = 0 the identity) or an [H, 3, 3] array of start rotations;
        init_T: None (T0 = target mean - R0 source mean) or [H, 3].  inliers[h] = vcp_match(source, target, M_all[h],
        inlier_dist).count_matched.  Returns dict(best, M [4,4], M_all [H,4,4], mean_dist [H], inliers [H])."""
        return self._icp_starts(lib().vcp_icp_multistart, source, target, poses, init_T, max_iter, max_landmarks, (),
                                inlier_dist)

    def icp_gated(self, source, target, gates, poses=1, init_T=None, max_iter=100, max_landmarks=200, min_pairs=3,
                  inlier_dist=np.inf):
        """icp_multistart with a per-round gate on the correspondence distance (vcp_icp_gated): round r (1-based) leaves
        pairs at gates[min(r, len(gates)) - 1] or farther out of its sums; a round that keeps fewer than min_pairs
        pairs changes nothing and counts as starved.  poses, init_T, inlier_dist: as icp_multistart.  Returns its dict
        plus kept [H] int64 (the last round's count) and starved [H] int32."""
        return self._icp_starts(lib().vcp_icp_gated, source, target, poses, init_T, max_iter, max_landmarks,
                                self._icp_schedule(gates, min_pairs), inlier_dist, self._ICP_COUNTED)

    def icp_sim(self, source, target, gates, ratio_range, poses=1, init_T=None, max_iter=100, max_landmarks=200,
                min_pairs=3, inlier_dist=np.inf):
        """icp_gated whose rounds fit one isotropic scale beside the rotation and the translation (vcp_icp_sim).
        ratio_range = (ratio_min, ratio_max), ratio_min <= 1 <= ratio_max: the bounds on the product of the scale
        factors a pose applies to its start.  Returns icp_gated's dict plus ratio [H] (that product) and unscaled [H]
        int32 (rounds whose scale the kept pairs did not determine)."""
        rmin, rmax = (float(v) for v in ratio_range)
        return self._icp_starts(lib().vcp_icp_sim, source, target, poses, init_T, max_iter, max_landmarks,
                                self._icp_schedule(gates, min_pairs) + (C.c_double(rmin), C.c_double(rmax)), inlier_dist,
                                self._ICP_COUNTED + (("ratio", np.float64), ("unscaled", np.int32)))

    def icp_aniso(self, source, target, gates, ratio_range, poses=1, init_T=None, init_scale=None, max_iter=100,
                  max_landmarks=200, min_pairs=3, inlier_dist=np.inf):
        """icp_gated whose rounds fit one scale for x and one for y beside the rotation and the translation
        (vcp_icp_aniso): the pose is y = R diag(sx, sy, 1) d + t.  init_scale: None (all 1.0) or [H, 2], the start scales
        of every pose; ratio_range = (ratio_min, ratio_max), ratio_min <= 1 <= ratio_max, bounds every scale to that
        multiple of its start.  M and M_all hold [R diag(sx, sy, 1) | t].  Returns icp_gated's dict plus scale [H, 2] and
        unscaled [H, 2] int32 (per axis the rounds whose kept pairs did not determine it)."""
        rmin, rmax = (float(v) for v in ratio_range)
        H = poses if isinstance(poses, (int, np.integer)) else len(_f64(poses).reshape(-1, 9))
        if init_scale is not None:
            init_scale = _f64(init_scale, 2)
            if len(init_scale) != H:
                raise ValueError("init_scale has %d rows for %d poses" % (len(init_scale), H))
        return self._icp_starts(lib().vcp_icp_aniso, source, target, poses, init_T, max_iter, max_landmarks,
                                self._icp_schedule(gates, min_pairs) + (C.c_double(rmin), C.c_double(rmax)), inlier_dist,
                                self._ICP_COUNTED + (("scale", np.float64, 2), ("unscaled", np.int32, 2)),
                                start_args=(init_scale,))

    def icp_trimmed(self, source, target, keep, poses=1, init_T=None, max_iter=100, max_landmarks=200, min_pairs=3,
                    inlier_dist=np.inf):
        """icp_multistart with a per-round keep share (vcp_icp_trimmed): round r (1-based) fits on the
        m = min(L, ceil(keep[min(r, len(keep)) - 1] * L)) of its L landmarks that lie closest to their nearest target;
        a round with m < min_pairs changes nothing and counts as starved.  poses, init_T, inlier_dist: as
        icp_multistart.  Returns icp_gated's dict plus trim_dist [H], the largest kept distance of the last round."""
        return self._icp_starts(lib().vcp_icp_trimmed, source, target, poses, init_T, max_iter, max_landmarks,
                                self._icp_schedule(keep, min_pairs), inlier_dist,
                                self._ICP_COUNTED + (("trim_dist", np.float64),))

    def icp_unique(self, source, target, gates, poses=1, init_T=None, max_iter=100, max_landmarks=200, min_pairs=3,
                   inlier_dist=np.inf):
        """icp_gated where a target takes one landmark per round (vcp_icp_unique): of the landmarks that share a
        nearest target only the closest (ties: the lower index) may enter the round's sums, and the round's gate then
        decides on it as in icp_gated.  Arguments as icp_gated.  Returns its dict plus lost [H] int64, the last round's
        count of landmarks that were not their target's winner."""
        return self._icp_starts(lib().vcp_icp_unique, source, target, poses, init_T, max_iter, max_landmarks,
                                self._icp_schedule(gates, min_pairs), inlier_dist,
                                self._ICP_COUNTED + (("lost", np.int64),))

    def register_pairs(self, source, target, bases, len_tol, inlier_dist, mirror=False, max_landmarks=200):
        """vcp_register_pairs: a pose of source on target without a start.  Every base (two source indices) is laid on
        every ordered pair of targets whose length matches its own within len_tol; each such pose is scored by the
        landmarks it puts within inlier_dist of some target.  Returns dict(best (-1 = no hypothesis), M [4,4], M_all
        [B,4,4], score [B] (-1 = none), inliers [B] (over all source points), pick [B,3] = (f, i, j), n_hyp [B])."""
        source = _f64(source, 3)
        target = _f64(target, 3)
        bases = np.ascontiguousarray(bases, np.int32).reshape(-1, 2)
        B = len(bases)
        M = np.zeros(16)
        M_all = np.zeros((B, 16))
        score = np.zeros(B, np.int32)
        inl = np.zeros(B, np.int32)
        pick = np.zeros((B, 3), np.int32)
        n_hyp = np.zeros(B, np.int64)
        best = C.c_int32(0)
        self._chk(lib().vcp_register_pairs(self._h, _ptr(source), C.c_int64(len(source)), _ptr(target),
                                           C.c_int64(len(target)), _ptr(bases), C.c_int32(B), C.c_double(len_tol),
                                           int(bool(mirror)), int(max_landmarks), C.c_double(inlier_dist), _ptr(M),
                                           C.byref(best), _ptr(M_all), _ptr(score), _ptr(inl), _ptr(pick), _ptr(n_hyp)))
        return dict(best=best.value, M=M.reshape(4, 4), M_all=M_all.reshape(B, 4, 4), score=score, inliers=inl, pick=pick,
                    n_hyp=n_hyp)

    def register_pairs_dev(self, d_source, ns, d_target, nt, d_bases, n_bases, len_tol, inlier_dist, mirror=False,
                           max_landmarks=200, d_M_all=None, d_score=None, d_inliers=None, d_pick=None, d_n_hyp=None):
        """Device-pointer form (ints from tensor.data_ptr()); the per-base arrays are written in place and may be None.
        Returns dict(best, M [4,4])."""
        M = np.zeros(16)
        best = C.c_int32(0)
        self._chk(lib().vcp_register_pairs_dev(self._h, _ptr(d_source), C.c_int64(ns), _ptr(d_target), C.c_int64(nt),
                                               _ptr(d_bases), C.c_int32(n_bases), C.c_double(len_tol), int(bool(mirror)),
                                               int(max_landmarks), C.c_double(inlier_dist), _ptr(M), C.byref(best),
                                               _ptr(d_M_all), _ptr(d_score), _ptr(d_inliers), _ptr(d_pick),
                                               _ptr(d_n_hyp)))
        return dict(best=best.value, M=M.reshape(4, 4))

    def register_sim(self, source, target, bases, scale_min, scale_max, inlier_dist, mirror=False, max_landmarks=200):
        """vcp_register_sim: register_pairs where source and target differ by an unknown scale.  A base fits an ordered
        pair of targets when k = Lv / Lu lies in [scale_min, scale_max]; the pose is the planar similarity with that k.
        Returns register_pairs's dict plus scale [B] (the winner's k; 0.0 = none)."""
        source = _f64(source, 3)
        target = _f64(target, 3)
        bases = np.ascontiguousarray(bases, np.int32).reshape(-1, 2)
        B = len(bases)
        M = np.zeros(16)
        M_all = np.zeros((B, 16))
        score = np.zeros(B, np.int32)
        inl = np.zeros(B, np.int32)
        pick = np.zeros((B, 3), np.int32)
        n_hyp = np.zeros(B, np.int64)
        scale = np.zeros(B)
        best = C.c_int32(0)
        self._chk(lib().vcp_register_sim(self._h, _ptr(source), C.c_int64(len(source)), _ptr(target),
                                         C.c_int64(len(target)), _ptr(bases), C.c_int32(B), C.c_double(scale_min),
                                         C.c_double(scale_max), int(bool(mirror)), int(max_landmarks),
                                         C.c_double(inlier_dist), _ptr(M), C.byref(best), _ptr(M_all), _ptr(score),
                                         _ptr(inl), _ptr(pick), _ptr(n_hyp), _ptr(scale)))
        return dict(best=best.value, M=M.reshape(4, 4), M_all=M_all.reshape(B, 4, 4), score=score, inliers=inl, pick=pick,
                    n_hyp=n_hyp, scale=scale)

    def register_sim_dev(self, d_source, ns, d_target, nt, d_bases, n_bases, scale_min, scale_max, inlier_dist,
                         mirror=False, max_landmarks=200, d_M_all=None, d_score=None, d_inliers=None, d_pick=None,
                         d_n_hyp=None, d_scale=None):
        """Device-pointer form (ints from tensor.data_ptr()); the per-base arrays are written in place and may be None.
        Returns dict(best, M [4,4])."""
        M = np.zeros(16)
        best = C.c_int32(0)
        self._chk(lib().vcp_register_sim_dev(self._h, _ptr(d_source), C.c_int64(ns), _ptr(d_target), C.c_int64(nt),
                                             _ptr(d_bases), C.c_int32(n_bases), C.c_double(scale_min),
                                             C.c_double(scale_max), int(bool(mirror)), int(max_landmarks),
                                             C.c_double(inlier_dist), _ptr(M), C.byref(best), _ptr(d_M_all), _ptr(d_score),
                                             _ptr(d_inliers), _ptr(d_pick), _ptr(d_n_hyp), _ptr(d_scale)))
        return dict(best=best.value, M=M.reshape(4, 4))

    def import_convert(self, rows, x_angle=0.0, y_angle=0.0, xdir=2, ydir=1, dedupe=True):
        """MainForm.AddFolder per-row work: dict(xyz [n,3], state [n] (0 filtered / 1 kept / 2 duplicate), kept, duplicates)."""
        rows = _f64(rows, 3)
        n = len(rows)
        xyz = np.zeros((n, 3))
        state = np.zeros(n, np.uint8)
        kept, dup = C.c_int64(0), C.c_int64(0)
        self._chk(lib().vcp_import_convert(self._h, _ptr(rows), C.c_int64(n), C.c_double(x_angle), C.c_double(y_angle),
                                           int(xdir), int(ydir), int(dedupe), _ptr(xyz), _ptr(state), C.byref(kept),
                                           C.byref(dup)))
        return dict(xyz=xyz, state=state, kept=kept.value, duplicates=dup.value)

    def import_compact(self, rows, group=None, x_angle=0.0, y_angle=0.0, xdir=2, ydir=1, dedupe=True):
        """vcp_import_compact: filter, duplicate classes with their sizes (per group when group [n] int32 is given) and
        the kept rows written densely in input order.  Returns dict(motor [m,2], xyz [m,3], dist [m], src [m], count [m],
        group [m], row_to [n] (-1 = filtered), m, duplicates)."""
        rows = _f64(rows, 3)
        n = len(rows)
        if group is not None:
            group = np.ascontiguousarray(group, np.int32).reshape(-1)
            if len(group) != n:
                raise ValueError("group has %d entries for %d rows" % (len(group), n))
        motor, xyz, dist = np.zeros((n, 2)), np.zeros((n, 3)), np.zeros(n)
        src, count, gout, row_to = (np.zeros(n, np.int32) for _ in range(4))
        m, dup = C.c_int64(0), C.c_int64(0)
        self._chk(lib().vcp_import_compact(self._h, _ptr(rows), C.c_int64(n), _ptr(group), C.c_double(x_angle),
                                           C.c_double(y_angle), int(xdir), int(ydir), int(bool(dedupe)), _ptr(motor),
                                           _ptr(xyz), _ptr(dist), _ptr(src), _ptr(count), _ptr(gout), _ptr(row_to),
                                           C.byref(m), C.byref(dup)))
        k = m.value
        return dict(motor=motor[:k].copy(), xyz=xyz[:k].copy(), dist=dist[:k].copy(), src=src[:k].copy(),
                    count=count[:k].copy(), group=gout[:k].copy(), row_to=row_to, m=k, duplicates=dup.value)

    def import_compact_dev(self, d_rows, n, d_group=None, x_angle=0.0, y_angle=0.0, xdir=2, ydir=1, dedupe=True,
                           d_motor=None, d_xyz=None, d_dist=None, d_src=None, d_count=None, d_group_out=None,
                           d_row_to=None):
        """Device-pointer form (ints from tensor.data_ptr()): d_rows float64 [n*3], d_group int32 [n] or None; every
        output has room for n entries and may be None.  Returns (m, duplicates)."""
        m, dup = C.c_int64(0), C.c_int64(0)
        self._chk(lib().vcp_import_compact_dev(self._h, _ptr(d_rows), C.c_int64(n), _ptr(d_group), C.c_double(x_angle),
                                               C.c_double(y_angle), int(xdir), int(ydir), int(bool(dedupe)),
                                               _ptr(d_motor), _ptr(d_xyz), _ptr(d_dist), _ptr(d_src), _ptr(d_count),
                                               _ptr(d_group_out), _ptr(d_row_to), C.byref(m), C.byref(dup)))
        return m.value, dup.value

    # -- scan text ---------------------------------------------------------------------------------
    def _txt_fail(self, rc, err):
        e = VcpError(rc, (lib().vcp_last_error(self._h) or b"").decode())
        e.err = tuple(int(x) for x in err)      # UNSUPPORTED: (offset, 0, 0); a bad line: (line, segment, kind)
        return e

    @staticmethod
    def _txt_args(data, seg_off):
        """(text argument, nbytes, seg_off, nseg): data is bytes, or a contiguous uint8 numpy array read in place."""
        if isinstance(data, np.ndarray):
            if data.dtype != np.uint8 or data.ndim != 1 or not data.flags.c_contiguous:
                raise ValueError("text must be bytes or a contiguous 1-D uint8 array")
            text, nbytes = _ptr(data), data.size
        else:
            text = bytes(data)
            nbytes = len(text)
        if seg_off is None:
            return text, nbytes, None, 1
        seg_off = np.ascontiguousarray(seg_off, np.uint64).reshape(-1)
        return text, nbytes, seg_off, len(seg_off) - 1

    def parse_scan_text(self, data, seg_off=None, count_only=False):
        """vcp_parse_scan_text: data = the bytes of the scan files one after the other, seg_off [nseg + 1] their offsets
        (None: one file).  Returns dict(rows [n, 3] float64, group [n] int32, seg_first [nseg + 1] int64, n, n_host);
        count_only leaves rows and group None.  A VcpError of this call carries .err = the call's err[3] and, for
        VCP_ERR_INDEX, .n."""
        text, nbytes, seg_off, nseg = self._txt_args(data, seg_off)
        first = np.zeros(nseg + 1, np.int64)
        n, nh = C.c_int64(0), C.c_int64(0)
        err = (C.c_int64 * 3)()
        if count_only:
            rc = lib().vcp_parse_scan_text(self._h, text, C.c_uint64(nbytes), _ptr(seg_off), C.c_int32(nseg),
                                           C.c_int64(0), None, None, _ptr(first), C.byref(n), C.byref(nh), err)
            if rc != 0:
                raise self._txt_fail(rc, err)
            return dict(rows=None, group=None, seg_first=first, n=n.value, n_host=0)
        # Room for one line per 16 bytes (an F6 line has 27 or more), so that the text is uploaded once; a text of shorter
        # lines comes back with VCP_ERR_INDEX and its n, and is parsed again with exactly that room.
        cap = nbytes // 16 + 1024
        while True:
            rows = np.zeros((cap, 3))
            group = np.zeros(cap, np.int32)
            rc = lib().vcp_parse_scan_text(self._h, text, C.c_uint64(nbytes), _ptr(seg_off), C.c_int32(nseg),
                                           C.c_int64(cap), _ptr(rows), _ptr(group), _ptr(first), C.byref(n),
                                           C.byref(nh), err)
            if rc != -4 or n.value <= cap:
                break
            cap = n.value
        if rc != 0:
            raise self._txt_fail(rc, err)
        k = n.value
        if cap > k + k // 4:                              # do not keep the unused room alive
            rows, group = rows[:k].copy(), group[:k].copy()
        return dict(rows=rows[:k], group=group[:k], seg_first=first, n=k, n_host=nh.value)

    def parse_scan_text_dev(self, data, cap, d_rows, d_group=None, seg_off=None):
        """Device-pointer form (ints from tensor.data_ptr()): data stays host bytes; d_rows float64 [cap * 3] (None:
        count-only), d_group int32 [cap] or None.  Returns dict(seg_first, n, n_host).  A VcpError carries .err and, for
        VCP_ERR_INDEX (n > cap), .n."""
        text, nbytes, seg_off, nseg = self._txt_args(data, seg_off)
        first = np.zeros(nseg + 1, np.int64)
        n, nh = C.c_int64(0), C.c_int64(0)
        err = (C.c_int64 * 3)()
        rc = lib().vcp_parse_scan_text_dev(self._h, text, C.c_uint64(nbytes), _ptr(seg_off), C.c_int32(nseg),
                                           C.c_int64(cap), _ptr(d_rows), _ptr(d_group), _ptr(first), C.byref(n),
                                           C.byref(nh), err)
        if rc != 0:
            e = self._txt_fail(rc, err)
            e.n = n.value
            raise e
        return dict(seg_first=first, n=n.value, n_host=nh.value)

    # -- export text ---------------------------------------------------------------------------------
    def _fmt_fail(self, rc, err, nbytes):
        e = VcpError(rc, (lib().vcp_last_error(self._h) or b"").decode())
        e.err = (int(err[0]), int(err[1]))
        e.nbytes = nbytes.value
        return e

    @staticmethod
    def _fmt_col(x):
        """(array kept alive, address, stride in doubles) of a float64 column: a 1-D view with a positive stride is read
        in place, anything else through a contiguous copy."""
        x = np.asarray(x)
        if not (x.dtype == np.float64 and x.ndim == 1 and x.dtype.isnative and len(x) > 0 and x.strides[0] > 0 and
                x.strides[0] % 8 == 0):
            x = np.ascontiguousarray(x, np.float64).reshape(-1)
        return x, x.ctypes.data, (x.strides[0] // 8 if len(x) else 1)

    def format_rows(self, a, b, c, ids=None, order=None, bit=6, eol=1, out=None, count_only=False):
        """vcp_format_rows: line j = `[ids[r] TAB] a[r] TAB b[r] TAB c[r] EOL`, r = order[j] (None: r = j), every number as
        '%.*f' % (bit, v); eol 0 = "\n", 1 = "\r\n".  a, b, c are float64 numpy columns of one length; strided 1-D views
        (rows[:, k]) are read in place.  out: a writable uint8 numpy array that receives the text; None: one is made, by
        a count-only call first.  Returns the text as a uint8 array (a view of out), or with count_only its length.  A
        VcpError of this call carries .err = the call's err[2] and .nbytes."""
        (a, pa, sa), (b, pb, sb), (c, pc, sc) = (self._fmt_col(x) for x in (a, b, c))
        n = len(a)
        if len(b) != n or len(c) != n:
            raise ValueError("columns of %d, %d and %d rows" % (n, len(b), len(c)))
        if ids is not None:
            ids = np.ascontiguousarray(ids, np.int32).reshape(-1)
            if len(ids) != n:
                raise ValueError("ids has %d entries for %d rows" % (len(ids), n))
        if order is not None:
            order = np.ascontiguousarray(order, np.int64).reshape(-1)
        m = n if order is None else len(order)
        nbytes = C.c_uint64(0)
        err = (C.c_int64 * 2)()
        while True:
            rc = lib().vcp_format_rows(self._h, _ptr(ids), C.c_void_p(pa), C.c_int64(sa), C.c_void_p(pb), C.c_int64(sb),
                                       C.c_void_p(pc), C.c_int64(sc), _ptr(order), C.c_int64(n), C.c_int64(m),
                                       C.c_int(bit), C.c_int(eol), _ptr(out),
                                       C.c_uint64(0 if out is None else out.nbytes), C.byref(nbytes), err)
            if rc != 0:
                raise self._fmt_fail(rc, err, nbytes)
            if count_only:
                return nbytes.value
            if out is not None:
                return out[:nbytes.value]
            out = np.empty(max(nbytes.value, 1), np.uint8)

    def format_rows_dev(self, d_a, stride_a, d_b, stride_b, d_c, stride_c, n, d_ids=None, d_order=None, m=None, bit=6,
                        eol=1, out=None):
        """Device-pointer form (ints from tensor.data_ptr()): d_a, d_b, d_c float64 read at their strides, d_ids int32 [n]
        or None, d_order int64 [m] or None (then m = n).  out: a writable uint8 numpy array that receives the text (None:
        count-only).  Returns the number of bytes.  A VcpError carries .err and, for VCP_ERR_INDEX with too small an out,
        .nbytes."""
        m = int(n if m is None else m)
        nbytes = C.c_uint64(0)
        err = (C.c_int64 * 2)()
        rc = lib().vcp_format_rows_dev(self._h, _ptr(d_ids), _ptr(d_a), C.c_int64(stride_a), _ptr(d_b),
                                       C.c_int64(stride_b), _ptr(d_c), C.c_int64(stride_c), _ptr(d_order), C.c_int64(n),
                                       C.c_int64(m), C.c_int(bit), C.c_int(eol), _ptr(out),
                                       C.c_uint64(0 if out is None else out.nbytes), C.byref(nbytes), err)
        if rc != 0:
            raise self._fmt_fail(rc, err, nbytes)
        return nbytes.value

    def selftest_format_total_dev(self, d_totals, n):
        """vcp_selftest_format_total_dev: the 64-bit sum of n uint32 words on the device."""
        total = C.c_uint64(0)
        self._chk(lib().vcp_selftest_format_total_dev(self._h, _ptr(d_totals), C.c_int64(n), C.byref(total)))
        return total.value

    def selftest_wave_dev(self, d_words, d_flags, n, tb, d_counter, d_out):
        """vcp_selftest_wave_dev: the helpers of csrc/wave.hpp run by one workgroup of tb threads on n uint32 words and n
        uint8 flags; d_counter (one uint32, set by the caller) takes the append, d_out [24, tb] uint32 the rows
        include/vcp.h lists.  Device pointers."""
        self._chk(lib().vcp_selftest_wave_dev(self._h, _ptr(d_words), _ptr(d_flags), C.c_int64(n), C.c_int(tb),
                                              _ptr(d_counter), _ptr(d_out)))

    # -- per-cluster quantiles and MAD ---------------------------------------------------------------
    @staticmethod
    def _cq_host(values, group, stride):
        values = np.ascontiguousarray(values, np.float64).reshape(-1)
        group = np.ascontiguousarray(group, np.int32).reshape(-1)
        n, stride = len(group), int(stride)
        if stride >= 1 and n > 0 and len(values) < (n - 1) * stride + 1:
            raise ValueError("values has %d doubles for %d rows at stride %d" % (len(values), n, stride))
        return values, group, n, stride

    def cluster_quantiles(self, values, group, K, q, stride=1):
        """vcp_cluster_quantiles: row i has the value values.flat[i * stride] and the group group[i] in 0..K (0 = none).
        Returns (out [K, nq] float64: the value of rank floor(q * (c - 1)) in every group, NaN for an empty one;
        counts [K] int64)."""
        values, group, n, stride = self._cq_host(values, group, stride)
        q = np.ascontiguousarray(q, np.float64).reshape(-1)
        out = np.zeros((max(int(K), 0), len(q)))
        counts = np.zeros(max(int(K), 0), np.int64)
        self._chk(lib().vcp_cluster_quantiles(self._h, _ptr(values), C.c_int64(stride), _ptr(group), C.c_int64(n),
                                              C.c_int32(K), _ptr(q), C.c_int32(len(q)), _ptr(out), _ptr(counts)))
        return out, counts

    def cluster_quantiles_dev(self, d_values, stride, d_group, n, K, q, d_out, d_counts=None):
        """Device-pointer form (ints from tensor.data_ptr()): d_values float64, d_group int32 [n], d_out float64
        [K * nq], d_counts int64 [K] or None; q is a host sequence."""
        q = np.ascontiguousarray(q, np.float64).reshape(-1)
        self._chk(lib().vcp_cluster_quantiles_dev(self._h, _ptr(d_values), C.c_int64(stride), _ptr(d_group),
                                                  C.c_int64(n), C.c_int32(K), _ptr(q), C.c_int32(len(q)), _ptr(d_out),
                                                  _ptr(d_counts)))

    def cluster_mad(self, values, group, K, c_mad=3.0, floor=0.0, stride=1):
        """vcp_cluster_mad: per group the lower median, the median absolute deviation from it and the threshold
        max(c_mad * mad, floor); a row of a group is rejected unless |v - med| <= thr.  Returns dict(med, mad, thr [K],
        reject [n] uint8, kept [K] int64, n_rejected)."""
        values, group, n, stride = self._cq_host(values, group, stride)
        kk = max(int(K), 0)
        med, mad, thr = np.zeros(kk), np.zeros(kk), np.zeros(kk)
        reject, kept = np.zeros(n, np.uint8), np.zeros(kk, np.int64)
        nr = C.c_int64(0)
        self._chk(lib().vcp_cluster_mad(self._h, _ptr(values), C.c_int64(stride), _ptr(group), C.c_int64(n),
                                        C.c_int32(K), C.c_double(c_mad), C.c_double(floor), _ptr(med), _ptr(mad),
                                        _ptr(thr), _ptr(reject), _ptr(kept), C.byref(nr)))
        return dict(med=med, mad=mad, thr=thr, reject=reject, kept=kept, n_rejected=nr.value)

    def cluster_mad_dev(self, d_values, stride, d_group, n, K, c_mad, floor, d_med, d_mad, d_thr, d_reject, d_kept):
        """Device-pointer form (ints from tensor.data_ptr()): d_med, d_mad, d_thr float64 [K], d_reject uint8 [n],
        d_kept int64 [K].  Returns n_rejected."""
        nr = C.c_int64(0)
        self._chk(lib().vcp_cluster_mad_dev(self._h, _ptr(d_values), C.c_int64(stride), _ptr(d_group), C.c_int64(n),
                                            C.c_int32(K), C.c_double(c_mad), C.c_double(floor), _ptr(d_med), _ptr(d_mad),
                                            _ptr(d_thr), _ptr(d_reject), _ptr(d_kept), C.byref(nr)))
        return nr.value

    # -- per-cluster covariance, principal axes and the ellipse numbers --------------------------------
    def cluster_moments(self, pts, labels, K, weights=None, dim=None, ld=None, outputs=None):
        """vcp_cluster_moments.  pts [n, c] float64: row i is pts[i, :dim] (dim defaults to c); a view with a row stride,
        such as xyz[:, :2] or wide[:, 3:6], is read in place.  With ld given, pts is a flat buffer and row i is
        pts[i * ld + 0 .. dim).  labels [n] in 0..K (0 = none), weights int32 >= 0 or None.  Returns dict(mean [K, dim],
        cov [K, dim (dim + 1) / 2], eval [K, dim], evec [K, dim, dim] (eigenvector j = evec[k, j]), shape [K, 4],
        valid [K] uint8, counts [K] int64); `outputs` names the ones wanted (the others are passed as NULL)."""
        pts, labels, weights, n, dim, ld = _cluster_rows(pts, labels, weights, dim, ld)
        kk, d = max(int(K), 0), dim if dim in (2, 3) else 3
        out = dict(mean=np.zeros((kk, d)), cov=np.zeros((kk, d * (d + 1) // 2)), eval=np.zeros((kk, d)),
                   evec=np.zeros((kk, d, d)), shape=np.zeros((kk, 4)), valid=np.zeros(kk, np.uint8),
                   counts=np.zeros(kk, np.int64))
        if outputs is not None:
            out = {k: v for k, v in out.items() if k in outputs}
        g = out.get
        self._chk(lib().vcp_cluster_moments(self._h, _ptr(pts), C.c_int64(ld), C.c_int(dim), _ptr(labels), _ptr(weights),
                                            C.c_int64(n), C.c_int32(K), _ptr(g("mean")), _ptr(g("cov")), _ptr(g("eval")),
                                            _ptr(g("evec")), _ptr(g("shape")), _ptr(g("valid")), _ptr(g("counts"))))
        return out

    def cluster_moments_dev(self, d_pts, ld, dim, d_labels, d_weights, n, K, d_mean=None, d_cov=None, d_eval=None,
                            d_evec=None, d_shape=None, d_valid=None, d_counts=None):
        """Device-pointer form (ints from tensor.data_ptr()): d_pts float64, d_labels and d_weights (or None) int32 [n];
        the outputs float64 but d_valid uint8 [K] and d_counts int64 [K], any of them None."""
        self._chk(lib().vcp_cluster_moments_dev(self._h, _ptr(d_pts), C.c_int64(ld), C.c_int(dim), _ptr(d_labels),
                                                _ptr(d_weights), C.c_int64(n), C.c_int32(K), _ptr(d_mean), _ptr(d_cov),
                                                _ptr(d_eval), _ptr(d_evec), _ptr(d_shape), _ptr(d_valid), _ptr(d_counts)))

    # -- per-cluster least-squares sphere / circle fit ---------------------------------------------------
    def cluster_spheres(self, pts, labels, K, weights=None, dim=None, ld=None, fixed_radius=0.0, rounds=12, outputs=None):
        """vcp_cluster_spheres.  pts, labels, weights, dim and ld as in cluster_moments (a strided view is read in place).
        fixed_radius 0 fits the radius, > 0 fixes it; rounds 0..64 Gauss-Newton rounds.  Returns dict(centre [K, dim],
        radius, rms, cap, step [K], alg [K, dim + 1] (the algebraic start: centre, radius), valid [K] uint8, counts [K]
        int64); `outputs` names the ones wanted (the others are passed as NULL)."""
        pts, labels, weights, n, dim, ld = _cluster_rows(pts, labels, weights, dim, ld)
        kk, d = max(int(K), 0), dim if dim in (2, 3) else 3
        out = dict(centre=np.zeros((kk, d)), radius=np.zeros(kk), rms=np.zeros(kk), cap=np.zeros(kk), step=np.zeros(kk),
                   alg=np.zeros((kk, d + 1)), valid=np.zeros(kk, np.uint8), counts=np.zeros(kk, np.int64))
        if outputs is not None:
            out = {k: v for k, v in out.items() if k in outputs}
        g = out.get
        self._chk(lib().vcp_cluster_spheres(self._h, _ptr(pts), C.c_int64(ld), C.c_int(dim), _ptr(labels), _ptr(weights),
                                            C.c_int64(n), C.c_int32(K), C.c_double(fixed_radius), C.c_int(rounds),
                                            _ptr(g("centre")), _ptr(g("radius")), _ptr(g("rms")), _ptr(g("cap")),
                                            _ptr(g("step")), _ptr(g("alg")), _ptr(g("valid")), _ptr(g("counts"))))
        return out

    def cluster_spheres_dev(self, d_pts, ld, dim, d_labels, d_weights, n, K, fixed_radius, rounds, d_centre=None,
                            d_radius=None, d_rms=None, d_cap=None, d_step=None, d_alg=None, d_valid=None, d_counts=None):
        """Device-pointer form (ints from tensor.data_ptr()): d_pts float64, d_labels and d_weights (or None) int32 [n];
        the outputs float64 but d_valid uint8 [K] and d_counts int64 [K], any of them None."""
        self._chk(lib().vcp_cluster_spheres_dev(self._h, _ptr(d_pts), C.c_int64(ld), C.c_int(dim), _ptr(d_labels),
                                                _ptr(d_weights), C.c_int64(n), C.c_int32(K), C.c_double(fixed_radius),
                                                C.c_int(rounds), _ptr(d_centre), _ptr(d_radius), _ptr(d_rms), _ptr(d_cap),
                                                _ptr(d_step), _ptr(d_alg), _ptr(d_valid), _ptr(d_counts)))


def selftest_spd_solve(S, b):
    """vcp_selftest_spd_solve: S is a symmetric [2, 2] or [3, 3] matrix (its upper triangle is read) or the packed upper
    triangle (3 or 6 doubles), b [dim].  Returns (x [dim], ok), from the source the kernels are compiled from (no
    device)."""
    S = np.asarray(S, np.float64)
    if S.ndim == 2:
        dim = S.shape[0]
        S = S[np.triu_indices(dim)]
    else:
        dim = {3: 2, 6: 3}.get(len(S), 0)
    S, b = np.ascontiguousarray(S), np.ascontiguousarray(b, np.float64)
    x, ok = np.zeros(max(dim, 1)), C.c_int(0)
    rc = lib().vcp_selftest_spd_solve(C.c_int(dim), _ptr(S), _ptr(b), _ptr(x), C.byref(ok))
    if rc < 0:
        raise VcpError(rc, "vcp_selftest_spd_solve")
    return x, ok.value


def selftest_sym_eig(S):
    """vcp_selftest_sym_eig: S is a symmetric [2, 2] or [3, 3] matrix (its upper triangle is read) or the packed upper
    triangle (3 or 6 doubles).  Returns (eval [dim], evec [dim, dim] with eigenvector j in row j, sweeps), from the source
    the kernel is compiled from (no device)."""
    S = np.asarray(S, np.float64)
    if S.ndim == 2:
        dim = S.shape[0]
        S = S[np.triu_indices(dim)]
    else:
        dim = {3: 2, 6: 3}.get(len(S), 0)
    S = np.ascontiguousarray(S)
    ev, V, sw = np.zeros(max(dim, 1)), np.zeros((max(dim, 1), max(dim, 1))), C.c_int(0)
    rc = lib().vcp_selftest_sym_eig(C.c_int(dim), _ptr(S), _ptr(ev), _ptr(V), C.byref(sw))
    if rc < 0:
        raise VcpError(rc, "vcp_selftest_sym_eig")
    return ev, V, sw.value


def selftest_rank_key(v, q, c):
    """vcp_selftest_rank_key: (key(v) as a Python int, the rank of q in a group of c rows), from the source the kernels
    are compiled from (no device)."""
    key, rank = C.c_uint64(0), C.c_int64(0)
    rc = lib().vcp_selftest_rank_key(C.c_double(v), C.c_double(q), C.c_int64(int(c)), C.byref(key), C.byref(rank))
    if rc < 0:
        raise VcpError(rc, "vcp_selftest_rank_key")
    return key.value, rank.value


def selftest_parse_field(s):
    """vcp_selftest_parse_field: (class 0..3, value or None for class 0) of one field (bytes or str), from the source the
    kernels are compiled from (no device)."""
    if isinstance(s, str):
        s = s.encode("latin-1")
    v = C.c_double(0.0)
    rc = lib().vcp_selftest_parse_field(s, C.c_int64(len(s)), C.byref(v))
    if rc < 0:
        raise VcpError(rc, "vcp_selftest_parse_field")
    return rc, (v.value if rc else None)


def selftest_format_field(v, bit, cap=64):
    """vcp_selftest_format_field: the bytes of '%.*f' % (bit, v) from the source the kernels are compiled from (no
    device), or None for a value the device formatter does not take."""
    out = C.create_string_buffer(max(int(cap), 1))
    n = C.c_int64(-1)
    rc = lib().vcp_selftest_format_field(C.c_double(v), C.c_int(bit), out, C.c_int64(cap), C.byref(n))
    if rc < 0:
        e = VcpError(rc, "vcp_selftest_format_field")
        e.len = n.value
        raise e
    return out.raw[:n.value] if rc else None


def selftest_horn_sim(sums, n, c=1.0, ratio_range=(1.0, 1.0), V=None):
    """vcp_selftest_horn_sim: one step of the similarity ICP on the host (no device), from the source the device runs.
    V [16] (updated in place) is the carried eigenvector basis, None for a cold start.  Returns dict(rc = 1 (scale
    determined), 2 (not determined) or 0 (the Horn solve failed: the other entries are None), R1s [9], T1 [3], k_used,
    c_new)."""
    sums = _f64(sums).reshape(18)
    R1s, T1 = np.zeros(9), np.zeros(3)
    ku, cn = C.c_double(0), C.c_double(0)
    rmin, rmax = ratio_range
    rc = lib().vcp_selftest_horn_sim(_ptr(sums), C.c_int64(int(n)), _ptr(V), C.c_int(0 if V is None else 1),
                                     C.c_double(c), C.c_double(rmin), C.c_double(rmax), _ptr(R1s), _ptr(T1), C.byref(ku),
                                     C.byref(cn))
    if rc < 0:
        raise VcpError(rc, "vcp_selftest_horn_sim")
    if rc == 0:
        return dict(rc=0, R1s=None, T1=None, k_used=None, c_new=None)
    return dict(rc=rc, R1s=R1s, T1=T1, k_used=ku.value, c_new=cn.value)


def selftest_horn_aniso(sums, n, R, s, lo, hi, V=None):
    """vcp_selftest_horn_aniso: one step of the anisotropic ICP on the host (no device), from the source the device runs.
    R [9] is the pose's current rotation, s [2] its scales, lo, hi [2] their bounds; V [16] (updated in place) the
    carried eigenvector basis, None for a cold start.  Returns dict(rc = 1 or 0 (the Horn solve failed: the other entries
    are None), R_new [9], T_new [3], s_new [2], determined = the bit mask of the axes the sums determined)."""
    sums = _f64(sums).reshape(18)
    R, s, lo, hi = _f64(R).reshape(9), _f64(s).reshape(2), _f64(lo).reshape(2), _f64(hi).reshape(2)
    Rn, Tn, sn = np.zeros(9), np.zeros(3), np.zeros(2)
    det = C.c_int32(0)
    rc = lib().vcp_selftest_horn_aniso(_ptr(sums), C.c_int64(int(n)), _ptr(V), C.c_int(0 if V is None else 1), _ptr(R),
                                       _ptr(s), _ptr(lo), _ptr(hi), _ptr(Rn), _ptr(Tn), _ptr(sn), C.byref(det))
    if rc < 0:
        raise VcpError(rc, "vcp_selftest_horn_aniso")
    if rc == 0:
        return dict(rc=0, R_new=None, T_new=None, s_new=None, determined=None)
    return dict(rc=rc, R_new=Rn, T_new=Tn, s_new=sn, determined=det.value)


def selftest_register_pose(a, b, ti, tj, f=0):
    """vcp_selftest_register_pose: the pose arithmetic of vcp_register_pairs run on the host (no device).  Returns (Lu, Lv,
    M [4,4] or None when the hypothesis is skipped)."""
    a, b, ti, tj = (_f64(v).reshape(3) for v in (a, b, ti, tj))
    L, M = np.zeros(2), np.zeros(16)
    rc = lib().vcp_selftest_register_pose(_ptr(a), _ptr(b), _ptr(ti), _ptr(tj), int(f), _ptr(L), _ptr(M))
    if rc < 0:
        raise VcpError(rc, "vcp_selftest_register_pose")
    return float(L[0]), float(L[1]), (M.reshape(4, 4) if rc == 1 else None)


def selftest_register_sim_pose(a, b, ti, tj, f=0):
    """vcp_selftest_register_sim_pose: the pose arithmetic of vcp_register_sim run on the host (no device).  Returns (Lu,
    Lv, k, M [4,4] or None when the hypothesis is skipped)."""
    a, b, ti, tj = (_f64(v).reshape(3) for v in (a, b, ti, tj))
    L, M = np.zeros(3), np.zeros(16)
    rc = lib().vcp_selftest_register_sim_pose(_ptr(a), _ptr(b), _ptr(ti), _ptr(tj), int(f), _ptr(L), _ptr(M))
    if rc < 0:
        raise VcpError(rc, "vcp_selftest_register_sim_pose")
    return float(L[0]), float(L[1]), float(L[2]), (M.reshape(4, 4) if rc == 1 else None)


def blocks_share_plan(blockstart, world):
    """vcp_blocks_share_plan: first block of every rank, [world + 1] (pure host arithmetic, no device)."""
    bs = np.ascontiguousarray(blockstart, np.uint32)
    cuts = np.zeros(int(world) + 1, np.int64)
    rc = lib().vcp_blocks_share_plan(_ptr(bs), C.c_int64(len(bs) - 1), C.c_int(int(world)), _ptr(cuts))
    if rc != 0:
        raise VcpError(rc, "vcp_blocks_share_plan")
    return cuts


class MultiContext:
    """vcp_multi: several GPUs driven from this one process (one vcp_ctx and one host thread per listed device; an id
    may repeat).  dbscan_blocks = Context.dbscan_blocks with every stage sharded over the devices: each one plans the
    partition, then builds, clusters and merges its own share of the blocks; device 0 runs the global noise pass and
    assembles the outputs."""

    def __init__(self, device_ids):
        ids = (C.c_int * len(device_ids))(*[int(d) for d in device_ids])
        self._h = C.c_void_p()
        rc = lib().vcp_create_multi(ids, len(device_ids), C.byref(self._h))
        if rc != 0:
            raise VcpError(rc, (lib().vcp_multi_last_error(None) or b"").decode())

    def close(self):
        if self._h:
            lib().vcp_destroy_multi(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def count(self):
        return int(lib().vcp_multi_count(self._h))

    def ctx(self, i):
        """The context of device i as a Context that does not own it (vcp_multi_ctx: borrowed; closing it does nothing)."""
        h = lib().vcp_multi_ctx(self._h, int(i))
        if not h:
            raise IndexError("no context %d" % i)
        c = Context.__new__(Context)
        c._h, c._borrowed = C.c_void_p(h), True
        return c

    def dbscan_blocks(self, motor, eps, min_pts, pts_in_cell, small_max=3, key_xy=None):
        motor = _f64(motor, 2)
        n = len(motor)
        key_xy = None if key_xy is None else _f64(key_xy, 2)
        labels = np.zeros(n, np.int32)
        block_of = np.zeros(n, np.int32)
        order = np.zeros(max(n, 1), np.int64)
        m = C.c_int64(0)
        rows, cols, kept, dels, ca = (C.c_int32(0) for _ in range(5))
        ev = C.c_int64(0)
        rc = lib().vcp_dbscan_blocks_multi(self._h, _ptr(key_xy), _ptr(motor), C.c_int64(n), C.c_double(eps), int(min_pts),
                                           int(pts_in_cell), int(small_max), _ptr(labels), _ptr(block_of), _ptr(order),
                                           C.byref(m), C.byref(rows), C.byref(cols), C.byref(kept), C.byref(dels),
                                           C.byref(ca), C.byref(ev))
        if rc != 0:
            raise VcpError(rc, (lib().vcp_multi_last_error(self._h) or b"").decode())
        return dict(labels=labels, block_of=block_of, order=order[: m.value].copy(), rows=rows.value, cols=cols.value,
                    kept=kept.value, del_sum=dels.value, cluster_amount=ca.value, evals=ev.value)
