"""The case table of tests/test_poison_cases.py (CPU) and tests/test_workspace_poison_gpu.py: every entry point of
include/vcp.h that takes a context, on a small deterministic input, compared with the reference its own tests use.
Importable without a GPU; everything that needs one is imported inside a check.

    case.name      unique
    case.funcs     the vcp.h functions the check exercises (the coverage test of test_poison_cases.py reads these).  A host
                   form that stages its arrays and then runs the _dev driver -- which is how every host form of the library
                   is written -- names both where the check calls it; a _dev form with its own case is named there too
    case.inputs()  the deterministic inputs (numpy arrays, bytes, numbers; built once and left unchanged)
    case.check(ctx, poison)  runs the functions on ctx and asserts every output against the reference: the CPU oracle, a
                   numpy restatement or a replay of the summation tree, computed once per case and kept.  Never an earlier
                   run of the library.  `poison(c)` overwrites the workspace of the context c with the word under test (a
                   no-op in the unpoisoned run).
    case.staged    the check drives one of the staged sequences (vcp_blocks_*, vcp_slab_*, on one or two contexts): the
                   workspace is overwritten before the first stage only -- ctx by the caller, a second context by the check.

Many checks call more than one entry point (host form and _dev form, the probes of a query family, the one-pass calls a
whole-run replay is restated from).  In every case that is not staged the check gets the context wrapped in EveryCall:
poison(ctx) runs again before EVERY call into the library, so that no entry point meets what the check's previous call
left behind -- which is often exactly what it would need -- but the word.

The inputs are those of the existing tables and corpora, at the smallest shapes that reach each buffer set."""
import math

import numpy as np

L1_2D, L2_2D, L2_3D, SIGNED_SUM_2D = 0, 1, 2, 3
INF = math.inf
ALL = 100000          # max_landmarks: every source point is a landmark

_EXTRA, _MULTI = [], []   # further contexts of the cases that drive more than one (created on first use)


def extra_context(i=0):
    from vtkcloudpoint_amd import _native as N
    while len(_EXTRA) <= i:
        _EXTRA.append(N.Context(0))
    return _EXTRA[i]


def multi_context():
    """The vcp_multi of the multi-device case: devices [0, 0]."""
    from vtkcloudpoint_amd import _native as N
    if not _MULTI:
        _MULTI.append(N.MultiContext([0, 0]))
    return _MULTI[0]


def close_extras():
    while _EXTRA:
        _EXTRA.pop().close()
    while _MULTI:
        _MULTI.pop().close()


def _oracle():
    from oracle import binding as O
    O.build()
    return O


class EveryCall:
    """A context on which every method call -- every call into the library -- is preceded by poison(ctx): each entry
    point of a check that makes several calls meets the overwritten workspace, not what the check's previous call left
    there.  Not for the staged sequences, whose later stages read what the earlier ones wrote."""
    _PLAIN = ("selftest_poison", "close", "timing", "timing_enable")

    def __init__(self, ctx, poison):
        object.__setattr__(self, "_ctx", ctx)
        object.__setattr__(self, "_poison", poison)

    def __getattr__(self, name):
        attr = getattr(self._ctx, name)
        if not callable(attr) or name.startswith("_") or name in self._PLAIN:
            return attr

        def call(*a, **kw):
            self._poison(self._ctx)
            return attr(*a, **kw)
        return call

    def __setattr__(self, name, value):
        setattr(self._ctx, name, value)


class Case:
    def __init__(self, name, funcs, inputs, check, staged=False):
        self.name, self.funcs, self._inputs, self._check = name, tuple(funcs), inputs, check
        self._inp, self.memo, self.staged = None, {}, staged

    def inputs(self):
        if self._inp is None:
            self._inp = self._inputs()
        return self._inp

    def ref(self, key, make):
        """A reference of this case, computed once."""
        if key not in self.memo:
            self.memo[key] = make()
        return self.memo[key]

    def check(self, ctx, poison=None):
        poison = poison or (lambda c: None)
        self._check(self, ctx if self.staged else EveryCall(ctx, poison), self.inputs(), poison)


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _sync():
    import torch
    torch.cuda.synchronize()      # the library runs on a stream of its own: torch's uploads have to be done


def _bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float64).view(np.uint64), np.ascontiguousarray(b, np.float64).view(np.uint64))


# ---- the DBSCAN engine (tests/engine_path_cases.py, compared as tests/_engine_paths_worker.py compares) -----------------
def _engine_oracle(case, inp):
    O = _oracle()
    return case.ref("oracle", lambda: O.dbscan(inp["coords"], inp["eps"], inp["min_pts"], inp["metric"], inp.get("cf_in", 0),
                                               inp.get("in_classed"), inp.get("labels")))


def _check_engine(case, ctx, inp, poison):
    import _engine_paths_worker as EW
    g = ctx.dbscan(inp["coords"], inp["eps"], inp["min_pts"], inp["metric"], cf_in=inp.get("cf_in", 0),
                   in_classed=inp.get("in_classed"), labels=inp.get("labels"))
    EW.same(g, _engine_oracle(case, inp))


def _check_engine_dev(case, ctx, inp, poison):
    import torch
    import _engine_paths_worker as EW
    c = np.ascontiguousarray(inp["coords"], np.float64)
    if c.ndim != 2:
        c = c.reshape(0, 2)
    n, dim = c.shape
    t = _dev(c) if n else torch.zeros((1, dim), dtype=torch.float64, device="cuda")
    cls = inp.get("in_classed")
    d_cls = None if cls is None else _dev(np.ascontiguousarray(cls, np.uint8))
    lab0 = np.zeros(max(n, 1), np.int32)
    if cls is not None and inp.get("labels") is not None:
        lab0[:n] = np.asarray(inp["labels"], np.int32)
    d_lab = _dev(lab0)
    d_core = torch.full((max(n, 1),), 9, dtype=torch.uint8, device="cuda")
    d_out = torch.full((max(n, 1),), 9, dtype=torch.uint8, device="cuda")
    _sync()
    cf, ev = ctx.dbscan_dev(t.data_ptr(), n, dim, inp["eps"], inp["min_pts"], inp["metric"], inp.get("cf_in", 0),
                            None if d_cls is None else d_cls.data_ptr(), d_lab.data_ptr(), d_core.data_ptr(), d_out.data_ptr())
    g = dict(labels=d_lab.cpu().numpy()[:n], is_core=d_core.cpu().numpy()[:n], is_classed=d_out.cpu().numpy()[:n], cf=cf,
             evals=ev)
    EW.same(g, _engine_oracle(case, inp))


def _check_grouped(case, ctx, inp, poison):
    O = _oracle()
    g = ctx.dbscan_blocks(inp["motor"], inp["eps"], inp["min_pts"], inp["pts_in_cell"], 3)
    o = case.ref("oracle", lambda: O.block_pipeline(inp["motor"], inp["eps"], inp["min_pts"], inp["pts_in_cell"], 3))
    for k in ("labels", "block_of", "order"):
        assert np.array_equal(g[k], o[k]), "%s differs" % k
    for k in ("rows", "cols", "kept", "del_sum", "cluster_amount", "evals"):
        assert g[k] == o[k], "%s %r != %r" % (k, g[k], o[k])


def _check_slabs(case, ctx, inp, poison):
    import torch
    import _engine_paths_worker as EW
    from vtkcloudpoint_amd import distributed as D
    O = _oracle()
    other = extra_context(0)
    poison(other)
    pts, cuts = inp["coords"], inp["cuts"]
    parts = [torch.from_numpy(np.ascontiguousarray(pts[a:b])).cuda() for a, b in zip(cuts, cuts[1:])]
    _sync()
    res = D.exact_slabs_local([ctx, other], parts, inp["eps"], inp["min_pts"], inp["metric"], 0)
    o = case.ref("oracle", lambda: O.dbscan(pts, inp["eps"], inp["min_pts"], inp["metric"]))
    whole = {k: np.concatenate([r[k].cpu().numpy() for r in res]) for k in ("labels", "is_core", "is_classed")}
    for r in res:
        EW.same(dict(whole, cf=r["cf"], evals=r["dist_evals"]), o)


def _engine_cases():
    import engine_path_cases as T
    out = []
    for c in T.CASES:
        if c.kind == "engine":
            out.append(Case("engine/" + c.name, ("vcp_dbscan", "vcp_dbscan_dev"), c.build, _check_engine))
            dev = Case("engine_dev/" + c.name, ("vcp_dbscan_dev",), c.build, _check_engine_dev)
            dev.memo = out[-1].memo      # one oracle run serves both forms
            out.append(dev)
        elif c.kind == "blocks":
            out.append(Case("engine/" + c.name, ("vcp_dbscan_blocks",), c.build, _check_grouped))
        else:
            out.append(Case("engine/" + c.name, ("vcp_slab_begin", "vcp_slab_comps", "vcp_slab_finish"), c.build,
                            _check_slabs, staged=True))
    return out


# ---- the block pipeline (tests/block_path_cases.py, compared as tests/_block_paths_worker.py compares) ------------------
def _blocks_oracle(case, inp):
    O = _oracle()

    def make():
        try:
            return O.block_pipeline(inp["motor"], inp["eps"], inp["min_pts"], inp["pts_in_cell"], inp["small_max"],
                                    key_xy=inp.get("key_xy"))
        except O.OracleError as e:
            return e
    return case.ref("oracle", make)


def _check_blocks(call):
    def check(case, ctx, inp, poison):
        import _block_paths_worker as BW
        from vtkcloudpoint_amd import _native as N
        BW.run(ctx, inp, _blocks_oracle(case, inp), getattr(BW, call), N, _oracle())
    return check


SHARED_KEYS = ("rows", "cols", "kept", "del_sum", "cluster_amount", "evals")


def _check_sharded(case, ctx, inp, poison):
    """The sharded stages (vcp_blocks_plan_dev ... vcp_scatter_pairs_dev) on two contexts, both noise modes."""
    from vtkcloudpoint_amd import distributed as D
    o = _blocks_oracle(case, inp)
    other = extra_context(0)
    motor = np.ascontiguousarray(inp["motor"], np.float64)
    d = _dev(motor)
    dk = None if inp.get("key_xy") is None else _dev(inp["key_xy"])
    for k, noise in enumerate(("gather", "slabs")):
        poison(ctx)            # (each noise mode is a whole sequence of its own)
        poison(other)
        _sync()
        res = D.sharded_pipeline_local([ctx, other], d.data_ptr(), len(motor), inp["eps"], inp["min_pts"], inp["pts_in_cell"],
                                       inp["small_max"], device="cuda", noise=noise, d_key=None if dk is None else dk.data_ptr())
        _sync()
        for q, r in enumerate(res):
            assert np.array_equal(r["labels"].cpu().numpy(), o["labels"]), "%s rank %d: labels" % (noise, q)
            for key in SHARED_KEYS:
                assert r[key] == o[key], "%s rank %d: %s %r != %r" % (noise, q, key, r[key], o[key])
            assert r["m"] == len(o["order"]), "%s rank %d: m" % (noise, q)


def _check_multi(case, ctx, inp, poison):
    """vcp_dbscan_blocks_multi on devices [0, 0]: a vcp_multi owns its contexts, so the check overwrites those."""
    o = _blocks_oracle(case, inp)
    mc = multi_context()
    for i in range(mc.count()):
        poison(mc.ctx(i))
    g = mc.dbscan_blocks(inp["motor"], inp["eps"], inp["min_pts"], inp["pts_in_cell"], inp["small_max"], key_xy=inp.get("key_xy"))
    for k in ("labels", "block_of", "order") + SHARED_KEYS:
        assert np.array_equal(g[k], o[k]), k


ONE_SHOT = ("vcp_dbscan_blocks", "vcp_dbscan_blocks_keyed")
STAGED = ("vcp_blocks_begin", "vcp_blocks_begin_keyed", "vcp_blocks_share", "vcp_blocks_cluster_dev",
          "vcp_blocks_finish_local_dev", "vcp_blocks_finish_dev")
SHARDED = ("vcp_blocks_plan_dev", "vcp_blocks_plan_cuts", "vcp_blocks_build_dev", "vcp_blocks_cluster_dev",
           "vcp_blocks_finish_local_dev", "vcp_blocks_finish_zero_dev", "vcp_blocks_finish_zcoords_dev",
           "vcp_blocks_finish_pairs_dev", "vcp_scatter_pairs_dev", "vcp_dbscan_dev", "vcp_slab_begin", "vcp_slab_comps",
           "vcp_slab_finish")
SHARDED_ON = ("tracked_split", "keyed_one_d_big")     # clusters, noise and a split block; the keyed partition
MULTI_ON = "tracked_split"


def _check_begin_dev(case, ctx, inp, poison):
    """vcp_blocks_begin_dev / vcp_blocks_begin_keyed_dev: the staged form of the worker on a resident cloud."""
    import torch
    n = len(inp["motor"])
    d = _dev(np.ascontiguousarray(inp["motor"], np.float64))
    dk = None if inp.get("key_xy") is None else _dev(np.ascontiguousarray(inp["key_xy"], np.float64))
    o = _blocks_oracle(case, inp)
    _sync()
    info = ctx.blocks_begin(None, inp["eps"], inp["min_pts"], inp["pts_in_cell"], inp["small_max"], device_ptr=d.data_ptr(),
                            n=n, key_device_ptr=None if dk is None else dk.data_ptr())
    m = info["m"]
    local = torch.zeros(max(m, 1), dtype=torch.int32, device="cuda")
    lo, hi, plo, phi = ctx.blocks_share(0, 1)
    assert (plo, phi) == (0, m)
    evals = ctx.blocks_cluster_dev(lo, hi, local.data_ptr())
    labels = torch.zeros(n, dtype=torch.int32, device="cuda")
    block_of = torch.zeros(n, dtype=torch.int32, device="cuda")
    order = torch.zeros(max(m, 1), dtype=torch.int64, device="cuda")
    out = ctx.blocks_finish_dev(local.data_ptr(), evals, labels.data_ptr(), block_of.data_ptr(), order.data_ptr())
    out.update(labels=labels.cpu().numpy(), block_of=block_of.cpu().numpy(), order=order.cpu().numpy()[:m], rows=info["rows"],
               cols=info["cols"])
    import _block_paths_worker as BW
    BW.same(out, o)


def _block_cases():
    import block_path_cases as T
    out = []
    for c in T.CASES:
        one = Case("blocks/" + c.name, ONE_SHOT, c.build, _check_blocks("one_shot"))
        staged = Case("blocks/" + c.name + "/staged", STAGED, c.build, _check_blocks("staged"), staged=True)
        staged.memo = one.memo
        out += [one, staged]
        if c.name in SHARDED_ON:
            sh = Case("blocks/" + c.name + "/sharded", SHARDED, c.build, _check_sharded, staged=True)
            bd = Case("blocks/" + c.name + "/begin_dev", ("vcp_blocks_begin_dev", "vcp_blocks_begin_keyed_dev",
                                                           "vcp_blocks_share", "vcp_blocks_cluster_dev", "vcp_blocks_finish_dev"),
                      c.build, _check_begin_dev, staged=True)
            sh.memo = bd.memo = one.memo
            out += [sh, bd]
        if c.name == MULTI_ON:
            mu = Case("blocks/" + c.name + "/multi", ("vcp_dbscan_blocks_multi", "vcp_multi_ctx", "vcp_multi_count"), c.build,
                      _check_multi, staged=True)
            mu.memo = one.memo
            out.append(mu)
    return out


# ---- the dead class (csrc/dbdead.hip, csrc/dbpairs.hip) against the literal transcription ---------------------------------
def _dead_inputs(lattice):
    def build():
        rng = np.random.default_rng(41 if lattice else 43)
        n = 150
        if lattice:   # a binary grid: the relation is provably 1-D (dbdead.hip)
            c = rng.integers(-20, 20, size=(n, 2)).astype(np.float64) * 0.25
        else:         # thirds: no binary grid, pairs within rounding of the threshold (dbpairs.hip, pair by pair)
            c = rng.integers(-12, 12, size=(n, 2)).astype(np.float64) / 3.0
        shown = (rng.random(n) < 0.8).astype(np.uint8)
        cls = (rng.random(n) < 0.3).astype(np.uint8)
        lab0 = (cls * rng.integers(1, 5, n)).astype(np.int32)
        return dict(c=c, eps=1.0 if lattice else 1.0 / 3.0 + 1.0 / 3.0, mp=3, shown=shown, cls=cls, lab0=lab0)
    return build


def _check_dead(case, ctx, inp, poison):
    O = _oracle()
    for masked in (True, False):
        shown, cls, lab0 = (inp["shown"], inp["cls"], inp["lab0"]) if masked else (None, None, None)
        g = ctx.dbscan(inp["c"], inp["eps"], inp["mp"], SIGNED_SUM_2D, 0, cls, lab0, in_mask=shown)
        o = case.ref(("literal", masked), lambda: O.db_literal(inp["c"], inp["eps"], inp["mp"], shown, cls, lab0))
        assert np.array_equal(g["labels"], o["labels"]), ("labels", masked)
        assert np.array_equal(g["is_classed"], o["classed"]), ("is_classed", masked)
        assert np.array_equal(g["is_core"], o["is_key"]), ("is_core", masked)
        assert g["cf"] == o["cluster_amount"] and g["evals"] == o["evals"], ("counters", masked)


# ---- the query families (tests/fuzz_queries.py) ---------------------------------------------------------------------------
FUZZ_COUNT = 6       # the first cases of every family's list in the bounded suite (fuzz_queries.SUITE gives the seed)
FUZZ_FUNCS = {
    "kdist": ("vcp_kdist", "vcp_kdist_dev", "vcp_dbscan"),
    "eps_tree": ("vcp_eps_tree", "vcp_eps_tree_dev", "vcp_kdist", "vcp_dbscan"),
    "gdbscan": ("vcp_gdbscan", "vcp_gdbscan_dev", "vcp_dbscan"),
    "match_unique": ("vcp_match_unique", "vcp_match_unique_dev", "vcp_match"),
    "register_pairs": ("vcp_register_pairs", "vcp_register_pairs_dev"),
    "register_sim": ("vcp_register_sim", "vcp_register_sim_dev"),
    "assign_truths": ("vcp_assign_truths",),
}


def _fuzz_case(family, index, lists):
    def build():
        import fuzz_queries as F
        if family not in lists:      # one list per family and table: a case's reference comes with it
            lists[family] = list(F.case_list(family, FUZZ_COUNT, F.SUITE[family][1]))
        return lists[family][index]

    def check(case, ctx, inp, poison):
        import fuzz_queries as F
        quiet, F.QUIET[0] = F.QUIET[0], True
        try:
            F.CHECK[family](ctx, inp)
        finally:
            F.QUIET[0] = quiet
    return Case("query/%s/%d" % (family, index), FUZZ_FUNCS[family], build, check)


def _heavy_cell(n):
    return lambda: dict(n=n)


def _check_heavy_eps_tree(case, ctx, inp, poison):
    """n identical points in one cell (tests/test_eps_tree_gpu.py): the heavy kernels; the walk's answer is a star on 0."""
    import torch
    import eps_tree_ref as R
    n = inp["n"]
    star = dict(kdist=np.zeros(n), reach=np.zeros(n), n_merge=n - 1, merge_w=np.zeros(n - 1),
                merge_a=np.zeros(n - 1, np.int32), merge_b=np.arange(1, n, dtype=np.int32), n_p=n)
    for metric, dim in ((L1_2D, 2), (L2_3D, 3)):
        c = np.full((n, dim), -7.5)
        g = ctx.eps_tree(c, 7, 0.125, metric)
        g["n_merge"] = len(g["merge_w"])
        bad = R.same(g, star)
        assert bad is None, "%s differs (n %d, metric %d)" % (bad, n, metric)
        assert 0 < g["rounds"] <= R.round_bound(n)
    # the device-pointer form without a kdist array of the caller's: the library's own (b_et_kd)
    c = np.full((n, 2), -7.5)
    t = _dev(c)
    mw = torch.full((n - 1,), -1.0, dtype=torch.float64, device="cuda")
    ma, mb = (torch.full((n - 1,), -1, dtype=torch.int32, device="cuda") for _ in range(2))
    reach = torch.full((n,), -1.0, dtype=torch.float64, device="cuda")
    _sync()
    m, rounds = ctx.eps_tree_dev(t.data_ptr(), n, 2, 7, 0.125, mw.data_ptr(), ma.data_ptr(), mb.data_ptr(), None,
                                 reach.data_ptr(), False, L1_2D)
    g = dict(kdist=np.zeros(n), reach=reach.cpu().numpy(), n_merge=m, merge_w=mw.cpu().numpy()[:m],
             merge_a=ma.cpu().numpy()[:m], merge_b=mb.cpu().numpy()[:m], rounds=rounds)
    bad = R.same(g, star)
    assert bad is None, "device form: %s differs (n %d)" % (bad, n)


def _check_heavy_gdbscan(case, ctx, inp, poison):
    """The same cell with weights 0..3 (tests/test_gdbscan_gpu.py): every W is the total weight."""
    import gdbscan_ref as R
    n = inp["n"]
    w = (np.arange(n) % 4).astype(np.int32)
    total = int(w.sum())
    ref = dict(labels=np.ones(n, np.int32), is_core=np.ones(n, np.uint8), wsum=np.full(n, total, np.int64), cf=1)
    none = dict(labels=np.zeros(n, np.int32), is_core=np.zeros(n, np.uint8), wsum=np.full(n, total, np.int64), cf=0)
    for metric, dim in ((L1_2D, 2), (L2_3D, 3)):
        c = np.full((n, dim), -7.5)
        for mw, want in ((total, ref), (total + 1, none)):
            g = ctx.gdbscan(c, 0.125, mw, metric, w, want_wsum=True)
            bad = R.same(g, want)
            assert bad is None, "%s differs (n %d, metric %d, min_weight %d)" % (bad, n, metric, mw)


def _kdist_heavy_inputs():
    """8300 points on 25 places of one cell and 300 spread wide: the dense cell's block exceeds HEAVY = 8192 points
    (csrc/kdist.hip), so its queries go to the wave-per-query pass."""
    rng = np.random.default_rng(77)
    dense = 0.5 + rng.integers(0, 5, (8300, 2)) * 2.0 ** -12
    wide = rng.uniform(-40.0, 40.0, (300, 2))
    c = np.concatenate([dense, wide])[rng.permutation(8600)]
    return dict(c=np.ascontiguousarray(c), k=9, rows=np.arange(0, 8600, 13))


def _check_kdist_heavy(case, ctx, inp, poison):
    import torch
    import kdist_ref as KR
    c, k, rows = inp["c"], inp["k"], inp["rows"]
    kd, knn = ctx.kdist(c, k, L1_2D, want_knn=True)
    bkd, bknn = case.ref("brute", lambda: KR.brute_rows(c, k, L1_2D, rows))
    assert np.array_equal(kd[rows], bkd, equal_nan=True), "kdist differs at rows %s" % rows[kd[rows] != bkd][:5]
    assert np.array_equal(knn[rows], bknn), "knn differs"
    t = _dev(c)
    d_kd = torch.full((len(c),), -1.0, dtype=torch.float64, device="cuda")
    _sync()
    ctx.kdist_dev(t.data_ptr(), len(c), 2, k, d_kd.data_ptr(), None, L1_2D)
    assert np.array_equal(d_kd.cpu().numpy()[rows], bkd, equal_nan=True), "device form"


def _eps_inf_inputs():
    rng = np.random.default_rng(3)
    c = rng.integers(0, 40, (400, 2)).astype(np.float64) * 0.25
    c[7] = np.nan
    c[11, 0] = np.inf
    w = rng.integers(0, 4, 400).astype(np.int32)
    return dict(c=c, w=w)


def _check_eps_inf(case, ctx, inp, poison):
    """eps = +inf: one cell, every finite pair (tests/test_gdbscan_gpu.py); vcp_dbscan's early out on the same cloud."""
    import gdbscan_ref as R
    O = _oracle()
    c, w = inp["c"], inp["w"]
    g = ctx.gdbscan(c, INF, 50, L1_2D, w, want_wsum=True)
    bad = R.same(g, case.ref("gd", lambda: R.gdbscan(c, INF, 50, L1_2D, w, None, None, 0)))
    assert bad is None, bad
    import _engine_paths_worker as EW
    EW.same(ctx.dbscan(c, INF, 5, L1_2D), case.ref("db", lambda: O.dbscan(c, INF, 5, L1_2D)))


# ---- ICP: the one-pass forms against the replay of the reduction tree ----------------------------------------------------
PASS_SHAPES = (("pairs", 100, 129), ("grid", 513, 1000), ("tiled", 513, 1000))   # tiled: one non-finite model point
PASS_FORMS = ("plain", "gated", "sim", "aniso", "trimmed", "unique")
PASS_FUNCS = {"plain": "vcp_icp_sums", "gated": "vcp_icp_sums_gated", "sim": "vcp_icp_sums_sim", "aniso": "vcp_icp_sums_aniso",
              "trimmed": "vcp_icp_sums_trimmed", "unique": "vcp_icp_sums_unique"}
STRETCH = np.array([1.03, 0.98, 1.0])     # the aniso pass's pose: the columns of R stretched


def _pass_inputs(path, nm, nd):
    def build():
        import icp_sums_ref as S
        model, data, Rm, T = S.case(path, nm, nd)
        return dict(model=model, data=data, R=Rm, T=T)
    return build


def _same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b))


def _same_nan(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


def _check_pass(form):
    def check(case, ctx, inp, poison):
        import icp_gated_ref as G
        import icp_sums_ref as S
        model, data, Rm, T = inp["model"], inp["data"], inp["R"], inp["T"]
        nd = len(data)
        pose = np.ascontiguousarray(Rm * STRETCH) if form == "aniso" else Rm
        nn, dd = case.ref("nn", lambda: G.brute_nn(model, S.transform(data, pose, T)))
        half = float(np.median(np.sqrt(dd)))
        if form == "plain":
            want = case.ref("want", lambda: S.sums(model, data, Rm, T, nn))
            got, gnn = ctx.icp_sums(model, data, Rm, T)
            assert _same(gnn, nn), "nn"
            assert _same_nan(got, want) and _same(np.signbit(got), np.signbit(want)), ("sums", got, want)
        elif form == "gated":
            want, kept, keep = case.ref("want", lambda: G.gated_sums(model, data, Rm, T, nn, half))
            S16, k, g_nn, g_keep = ctx.icp_sums_gated(model, data, half, Rm, T)
            assert k == kept and 0 < kept < nd and _same(g_keep, keep) and _same(g_nn, nn)
            assert _same(S16, want), (S16, want)
        elif form == "sim":
            import icp_sim_ref as SR
            want, kept, keep = case.ref("want", lambda: SR.sim_sums(model, data, Rm, T, nn, half))
            S18, k, g_nn, g_keep = ctx.icp_sums_sim(model, data, half, Rm, T)
            assert k == kept and 0 < kept < nd and _same(g_keep, keep) and _same(g_nn, nn)
            assert S18.tobytes() == want.tobytes(), (S18, want)
        elif form == "aniso":
            import icp_aniso_ref as A
            want, kept, keep = case.ref("want", lambda: A.aniso_sums(model, data, pose, T, nn, half))
            S18, k, g_nn, g_keep = ctx.icp_sums_aniso(model, data, half, pose, T)
            assert k == kept and 0 < kept < nd and _same(g_keep, keep) and _same(g_nn, nn)
            assert S18.tobytes() == want.tobytes(), (S18, want)
        elif form == "trimmed":
            import icp_trimmed_ref as TR
            m = nd // 2
            want, keep, thr = case.ref("want", lambda: TR.trimmed_sums(model, data, Rm, T, nn, m))
            S16, g_thr, g_nn, g_keep = ctx.icp_sums_trimmed(model, data, m, Rm, T)
            assert _same(g_nn, nn) and _same(g_keep, keep) and int(g_keep.sum()) == m
            assert TR.same_float(g_thr, thr) and thr == np.sort(dd)[m - 1]
            assert _same_nan(S16, want), (S16, want)
        else:
            import icp_unique_ref as U
            win = U.unique_mask(nn, dd)
            d = np.sqrt(dd[win & np.isfinite(dd)])
            gate = float(np.median(d)) if len(d) else 1.0
            want, kept, lost, code = case.ref("want", lambda: U.unique_sums(model, data, Rm, T, nn, gate))
            S16, g_kept, g_lost, g_nn, g_keep = ctx.icp_sums_unique(model, data, gate, Rm, T)
            assert _same(g_nn, nn) and _same(g_keep, code) and (g_kept, g_lost) == (kept, lost)
            assert g_lost == nd - len(np.unique(nn))
            assert _same_nan(S16, want), (S16, want)
    return check


def _pass_cases():
    out = []
    shapes = {f: list(PASS_SHAPES) for f in PASS_FORMS}
    shapes["trimmed"].append(("pairs", 100, 4097))    # beyond VCP_ICPT_SELECT_WG_MAX: the multi-workgroup select
    shapes["unique"].append(("pairs", 100, 4097))     # (the one-pass form never resets: icp_run/unique/reset_kernel does)
    for form in PASS_FORMS:
        for path, nm, nd in shapes[form]:
            out.append(Case("icp_pass/%s/%s_%d_%d" % (form, path, nm, nd), (PASS_FUNCS[form],), _pass_inputs(path, nm, nd),
                            _check_pass(form)))
    return out


# ---- ICP: whole runs against their round-by-round restatement ---------------------------------------------------------------
# The restatement of a run is built from one-pass calls on the same context (held to the tree by the cases above) and the
# HOST Horn step; the run itself is called first and so meets the overwritten workspace.
RUN_SIZES = ((300, 240, 80), (600, 500, 150))     # truths: the scalar-cache scan and the grid
RUN_ROUNDS = 9                                    # past the 8-round batch boundary of the loops
SEEDS = {300: 2, 600: 3}


def _run_inputs(form, nt, ntrue, nclutter):
    def build():
        import icp_gated_ref as G
        if form == "sim":
            import icp_sim_ref as SR
            return SR.scaled_scene(nt, ntrue, nclutter, SEEDS[nt], 0.02)
        if form == "aniso":
            import icp_aniso_ref as A
            return A.aniso_scene(nt, ntrue, nclutter, SEEDS[nt], A.WRONG_STARTS[0])
        if form == "unique":
            import icp_unique_ref as U
            return U.ghost_scene(nt, ntrue, nclutter, U.SEEDS[nt][0])
        return G.scene(nt, ntrue, nclutter, SEEDS[nt])
    return build


def _matrix(Rm, T):
    M = np.eye(4)
    M[:3, :3] = np.array(Rm).reshape(3, 3)
    M[:3, 3] = T
    return M


def _check_run(form):
    def check(case, ctx, sc, poison):
        import icp_gated_ref as G
        from vtkcloudpoint_amd import _native as N
        src, tgt = sc["centers"], sc["truths"]
        R0, T0 = sc["R0"].reshape(1, 3, 3), sc["T0"].reshape(1, 3)
        lm = G.landmarks(src, ALL)
        assert len(lm) == len(src)
        r = RUN_ROUNDS
        if form == "gated":
            g = ctx.icp_gated(src, tgt, G.schedule(), R0, T0, r, ALL, G.MIN_PAIRS, 0.1)
            want = G.replay_run(ctx, N, tgt, lm, R0, T0, G.schedule(), r)[-1]
            keys = ()
        elif form == "trimmed":
            import icp_trimmed_ref as TR
            keep = [0.9, 0.8, 0.7]
            g = ctx.icp_trimmed(src, tgt, keep, R0, T0, r, ALL, G.MIN_PAIRS, 0.1)
            want = TR.replay_run(ctx, N, tgt, lm, R0, T0, keep, r)[-1]
            keys = ("trim_dist",)
        elif form == "sim":
            import icp_sim_ref as SR
            g = ctx.icp_sim(src, tgt, G.schedule(), SR.RATIO_RANGE, R0, T0, r, ALL, G.MIN_PAIRS, 0.1)
            want = SR.replay_run(ctx, N, tgt, src, R0[0], T0[0], G.schedule(), r, SR.RATIO_RANGE)[-1]
            keys = ("ratio", "unscaled")
        elif form == "aniso":
            import icp_aniso_ref as A
            s0 = sc["s0"].reshape(1, 2)
            g = ctx.icp_aniso(src, tgt, G.schedule(), A.RATIO, R0, T0, s0, r, ALL, G.MIN_PAIRS, 0.1)
            want = A.replay_run(ctx, N, tgt, src, R0[0], s0[0], T0[0], G.schedule(), r, A.RATIO)[-1]
            assert g["scale"][0].tolist() == want["scale"] and g["unscaled"][0].tolist() == want["unscaled"]
            keys = ()
        else:
            import icp_unique_ref as U
            g = ctx.icp_unique(src, tgt, G.schedule(), R0, T0, r, ALL, G.MIN_PAIRS, 0.1)
            want = U.replay_run(ctx, N, tgt, lm, R0[0], T0[0], G.schedule(), r)[-1]
            keys = ("lost",)
        assert g["M_all"][0].tobytes() == want["M"].tobytes() and g["M"].tobytes() == want["M"].tobytes(), "M"
        assert g["mean_dist"][0] == want["mean_dist"], "mean_dist"
        assert g["kept"][0] == want["kept"] and g["starved"][0] == want["starved"], "kept / starved"
        assert want["starved"] == 0 and 0 < want["kept"] <= len(src)
        for k in keys:
            assert g[k][0] == want[k], k
        assert g["best"] == 0
        # the score: vcp_match's count of all source points under the pose found, by the oracle's match
        o = case.ref("inliers", lambda: _oracle().match(src, tgt, want["M"].reshape(16), 0.1))
        assert g["inliers"][0] == o["count"] > 0, ("inliers", g["inliers"][0], o["count"])
    return check


def _icp_scene(nm):
    def build():
        import test_icp_replay_gpu as IR
        model, data = IR.scene(1000 + nm, nm, 5000, 0.12 if nm < 512 else 0.05, (0.8, -0.5, 0.3), 0.05)
        return dict(model=model, data=data)
    return build


def _check_icp(case, ctx, inp, poison):
    """vcp_icp and vcp_icp_dev against tests/test_icp_replay_gpu.py's trace and stop rule."""
    import torch
    import test_icp_replay_gpu as IR
    from vtkcloudpoint_amd import _native as N
    model, data = inp["model"], inp["data"]
    nd = len(data)
    g = ctx.icp(model, data, 0.0, RUN_ROUNDS, N.STOP_SSE_DELTA)
    dm, dd = _dev(model), _dev(data)
    _sync()
    gd = ctx.icp_dev(dm.data_ptr(), len(model), dd.data_ptr(), nd, 0.0, RUN_ROUNDS, N.STOP_SSE_DELTA)
    tr = IR.trace(ctx, model, data, np.eye(3), np.zeros(3), RUN_ROUNDS, IR.REFERENCE)
    Rw, Tw, d, iters = IR.predict(tr, nd, RUN_ROUNDS, N.STOP_SSE_DELTA, 0.0, [0.0] * 9, [0.0] * 3)
    for what, r in (("host", g), ("dev", gd)):
        assert r["iters"] == iters and r["sse"] == d and r["rmse"] == math.sqrt(d / nd), what
        assert np.array_equal(np.asarray(r["R"]).reshape(9), np.array(Rw)) and np.array_equal(r["T"], np.array(Tw)), what


def _vtk_scene(nt):
    def build():
        import test_icp_replay_gpu as IR
        tgt, src = IR.scene(500 + nt, nt, 1000, 0.1, (0.7, -0.4, 0.0), 0.05, planar=True)
        return dict(tgt=tgt, src=src)
    return build


def _eight_starts():
    Rs = []
    for h in range(8):
        th = h * (2 * math.pi / 8)
        c, s = math.cos(th), math.sin(th)
        Rs.append([c, -s, 0.0, s, c, 0.0, 0.0, 0.0, 1.0])
    Rs[5] = [Rs[5][0], -Rs[5][1], 0.0, Rs[5][3], -Rs[5][4], 0.0, 0.0, 0.0, 1.0]     # one reflection
    return Rs


def _check_vtklike(case, ctx, inp, poison):
    import test_icp_replay_gpu as IR
    tgt, src = inp["tgt"], inp["src"]
    ml = 200
    g = ctx.icp_vtklike(src, tgt, RUN_ROUNDS, ml, True)
    lm = IR._landmarks(src, ml)
    ms, mt = IR._seq_mean(src), IR._seq_mean(tgt)
    d, Rm, T = IR.trace(ctx, tgt, lm, np.eye(3), [mt[c] - ms[c] for c in range(3)], RUN_ROUNDS, IR.VTK)[-1]
    assert g["iters"] == RUN_ROUNDS and np.array_equal(g["M"], _matrix(Rm, T)) and g["mean_dist"] == math.sqrt(d / len(lm))


def _check_multistart(case, ctx, inp, poison):
    import test_icp_replay_gpu as IR
    tgt, src = inp["tgt"], inp["src"]
    ml = 200
    Rs = _eight_starts()
    g = ctx.icp_multistart(src, tgt, np.array(Rs).reshape(8, 3, 3), None, RUN_ROUNDS, ml, 1.0)
    lm = IR._landmarks(src, ml)
    ms, mt = IR._seq_mean(src), IR._seq_mean(tgt)
    for h in range(8):
        R0 = Rs[h]
        T0 = [mt[r] - (R0[3 * r] * ms[0] + R0[3 * r + 1] * ms[1] + R0[3 * r + 2] * ms[2]) for r in range(3)]
        d, Rm, T = IR.trace(ctx, tgt, lm, R0, T0, RUN_ROUNDS, IR.VTK)[-1]
        assert np.array_equal(g["M_all"][h], _matrix(Rm, T)), ("pose", h)
        assert g["mean_dist"][h] == math.sqrt(d / len(lm)), ("pose", h)
    o = _oracle().match(src, tgt, g["M_all"][g["best"]].reshape(16), 1.0)
    assert g["inliers"][g["best"]] == o["count"]


def _unique_reset_inputs():
    """tests/test_icp_unique_gpu.py's cloud beyond UNIQ_RESET_STEP_MAX = 4096 landmarks: k_icpu_reset sets the slots back
    between the rounds (below it the step does)."""
    import test_icp_unique_gpu as TU
    tgt, src = TU._cloud(300, TU.RESET_STEP_MAX + 104, 1200)
    return dict(tgt=tgt, src=src)


def _check_unique_reset(case, ctx, inp, poison):
    import icp_gated_ref as G
    import icp_unique_ref as U
    from vtkcloudpoint_amd import _native as N
    tgt, src = inp["tgt"], inp["src"]
    lm = G.landmarks(src, ALL)
    assert len(lm) == len(src) > 4096
    gates, rounds = [2.0, 0.5, 0.2], 5
    R0, T0 = G.rz(0.05).reshape(1, 3, 3), np.array([[0.3, 0.1, 0.0]])
    g = ctx.icp_unique(src, tgt, gates, R0, T0, rounds, ALL, 3, 0.2)
    want = U.replay_run(ctx, N, tgt, lm, R0[0], T0[0], gates, rounds, 3)[-1]
    assert g["M_all"][0].tobytes() == want["M"].tobytes() and g["mean_dist"][0] == want["mean_dist"]
    assert (g["kept"][0], g["lost"][0], g["starved"][0]) == (want["kept"], want["lost"], want["starved"])
    assert want["starved"] == 0 and 3 <= want["kept"] <= len(tgt) and want["lost"] >= len(lm) - len(tgt)
    o = case.ref("inliers", lambda: _oracle().match(src, tgt, want["M"].reshape(16), 0.2))
    assert g["inliers"][0] == o["count"] > 0


def _run_cases():
    out = [Case("icp_run/unique/reset_kernel", ("vcp_icp_unique", "vcp_icp_sums_unique"), _unique_reset_inputs,
                _check_unique_reset)]
    funcs = {"gated": ("vcp_icp_gated", "vcp_icp_sums_gated"), "trimmed": ("vcp_icp_trimmed", "vcp_icp_sums_trimmed"),
             "sim": ("vcp_icp_sim", "vcp_icp_sums_sim"), "aniso": ("vcp_icp_aniso", "vcp_icp_sums_aniso"),
             "unique": ("vcp_icp_unique", "vcp_icp_sums_unique")}
    for nt, ntrue, nclutter in RUN_SIZES:
        for form in ("gated", "trimmed", "sim", "unique", "aniso"):
            out.append(Case("icp_run/%s/%d" % (form, nt), funcs[form], _run_inputs(form, nt, ntrue, nclutter), _check_run(form)))
        out.append(Case("icp_run/icp/%d" % nt, ("vcp_icp", "vcp_icp_dev", "vcp_icp_sums"), _icp_scene(nt), _check_icp))
        out.append(Case("icp_run/vtklike/%d" % nt, ("vcp_icp_vtklike", "vcp_icp_sums"), _vtk_scene(nt), _check_vtklike))
        out.append(Case("icp_run/multistart/%d" % nt, ("vcp_icp_multistart", "vcp_icp_sums"), _vtk_scene(nt),
                        _check_multistart))
    return out


# ---- matching --------------------------------------------------------------------------------------------------------------
def _match_inputs(T):
    def build():
        rng = np.random.default_rng(11 + T)
        K = 700
        truths = rng.integers(0, 80, size=(T, 3)).astype(np.float64) * 0.5     # a lattice: exact ties
        centers = rng.integers(0, 160, size=(K, 3)).astype(np.float64) * 0.25
        truths[T // 2] = truths[7]                     # a duplicated truth: the lowest index wins
        centers[:50] = truths[:50]
        centers[60] = np.nan
        M = np.eye(4)
        M[:3, 3] = (0.5, -0.25, 0.125)
        txy = np.ascontiguousarray(truths[:, :2])
        tids = rng.integers(0, 50, size=T).astype(np.int32)
        motor = rng.integers(-40, 240, size=(3000, 2)).astype(np.float64) * 0.25
        return dict(centers=centers, truths=truths, M=M, motor=motor, txy=txy, tids=tids)
    return build


def _check_match(case, ctx, inp, poison):
    O = _oracle()
    g = ctx.match(inp["centers"], inp["truths"], inp["M"], 0.6)
    o = case.ref("match", lambda: O.match(inp["centers"], inp["truths"], inp["M"].reshape(16), 0.6))
    for k in ("matched_xyz", "nearest", "is_matched"):          # (the NaN centroid's transformed point is NaN on both sides)
        assert np.array_equal(o[k], g[k], equal_nan=(k == "matched_xyz")), k
    assert np.array_equal(o["nearest_dist"], g["nearest_dist"], equal_nan=True) and o["count"] == g["count"] > 0
    for radius in (1.0, INF):
        ids, out = ctx.assign_truths(inp["motor"], inp["txy"], inp["tids"], radius)
        o_ids, o_out = case.ref(("assign", radius), lambda: O.assign_truths(inp["motor"], inp["txy"], inp["tids"], radius))
        assert np.array_equal(ids, o_ids) and out == o_out, radius


# ---- the centroid family against the replay of its summation tree (tests/centroid_ref.py) ------------------------------------
def _centroid_inputs():
    import centroid_ref as R
    xyz, motor, lab = R.case("uniform")
    assert np.array_equal(lab, R.case_labels())
    grp, Kc = R.compact(lab)
    cid, pts = R.case_weights(grp)
    return dict(xyz=xyz, motor=motor, lab=lab, grp=grp, Kc=Kc, cid=cid, pts=pts, K=257, map=R.case_dictionary(257))


def _check_centroids(which):
    def check(case, ctx, inp, poison):
        import torch
        import centroid_ref as R
        from test_centroid_replay_gpu import same
        xyz, motor, lab, K = inp["xyz"], inp["motor"], inp["lab"], inp["K"]
        if which == "plain":
            g3, g2, gc = ctx.centroids(xyz, motor, lab, K)
            t3, t2, tc = case.ref("tree", lambda: R.tree_centroids(xyz, motor, lab, K))
            assert np.array_equal(gc, tc) and same(g3, t3) and same(g2, t2)
        elif which == "dev":
            dx, dm, dl = _dev(xyz), _dev(motor), _dev(lab)
            d3 = torch.full((K, 3), 7.0, dtype=torch.float64, device="cuda")
            d2 = torch.full((K, 2), 7.0, dtype=torch.float64, device="cuda")
            dc = torch.full((K,), -1, dtype=torch.int64, device="cuda")
            _sync()
            ctx.centroids_dev(dx.data_ptr(), dm.data_ptr(), dl.data_ptr(), len(lab), K, d3.data_ptr(), d2.data_ptr(),
                              dc.data_ptr())
            t3, t2, tc = case.ref("tree", lambda: R.tree_centroids(xyz, motor, lab, K))
            assert np.array_equal(dc.cpu().numpy(), tc) and same(d3.cpu().numpy(), t3) and same(d2.cpu().numpy(), t2)
        elif which == "weighted":
            g3, gi = ctx.centroids_weighted(xyz, inp["grp"], inp["cid"], inp["pts"], inp["Kc"], False)
            t3, ti = case.ref("tree_weighted", lambda: R.tree_centroids_weighted(xyz, inp["grp"], inp["cid"], inp["pts"], inp["Kc"], False))
            assert np.array_equal(gi, ti) and same(g3, t3)
        else:
            O = _oracle()
            gl, gk, g3, g2, gc = ctx.refresh_by_dictionary(xyz, motor, lab, K, inp["map"])
            tl, tk, t3, t2, tc = case.ref("tree_refresh", lambda: R.tree_refresh(xyz, motor, lab, K, inp["map"]))
            assert gk == tk and np.array_equal(gl, tl) and np.array_equal(gc, tc) and same(g3, t3) and same(g2, t2)
            # vcp_merge_centroids on the tree's own centroids, against the oracle's MergeIDByDistance
            c3 = case.ref("c3", lambda: R.tree_centroids(xyz, motor, lab, K)[0])
            live = ~np.isnan(c3[:, 0])
            cxy = np.ascontiguousarray(c3[live, :2])
            ids = (np.flatnonzero(live) + 1).astype(np.int32)
            thr = case.ref("thr", lambda: _merge_threshold(cxy))
            mg, cg = ctx.merge_centroids(cxy, ids, thr)
            mo, co = case.ref("merge", lambda: O.merge_ids(cxy, ids, thr))
            assert np.array_equal(mo, mg) and co == cg > 0
    return check


def _merge_threshold(cxy):
    """A distance that merges some of the centroids, not all: the 10 % quantile of the nearest-neighbour distances times 2."""
    d = np.sqrt(((cxy[:, None, :] - cxy[None, :, :]) ** 2).sum(axis=2))
    np.fill_diagonal(d, np.inf)
    return float(2.0 * np.quantile(d.min(axis=1), 0.1))


# ---- shapes and the per-cluster statistics on two families of tests/shape_families.py ---------------------------------------
SHAPE_FAMILIES = ("sizes", "ties")
CIRCLE = ("centers", "radius", "valid", "hull_n")
RECT = ("rect_valid", "rect_edge", "rect_len", "rect_xy")


def _shape_inputs(name):
    def build():
        import shape_families as SF
        c = SF.family(name)
        rng = np.random.default_rng(len(name))
        z = np.round(rng.normal(0.0, 1.0, len(c["labels"])), 6)
        w = rng.integers(1, 4, len(c["labels"])).astype(np.int32)
        return dict(c, z=z, w=w)
    return build


def _check_shapes(case, ctx, c, poison):
    import shape_families as SF
    import test_circle_exact_gpu as CE
    ref = case.ref("oracle", lambda: SF.oracle_shapes(_oracle(), c))

    def held(got, what):
        for key in CIRCLE + RECT:
            assert _same_nan(got[key], ref[key]), (what, key)
        assert got["hull_off"][0] == 0 and _same(np.diff(got["hull_off"]), np.where(ref["valid"] == 1, ref["hull_n"], 0))
        for k in range(c["K"]):
            if ref["valid"][k] == 1:
                assert _same_nan(CE._hull_xy(c, got, k), ref["hull_xy"][k]), (what, "hull", k)
    if case.name.endswith("/dev"):
        held(CE._dev(ctx, c), "dev")
        return
    held(ctx.cluster_shapes(c["xy"], c["labels"], c["K"], c["order"]), "host")
    mcc = ctx.mcc(c["xy"], c["labels"], c["K"], c["order"])
    for key in CIRCLE:
        assert _same_nan(mcc[key], ref[key]), ("mcc", key)


def _check_filter(case, ctx, c, poison):
    import torch
    import shape_families as SF
    import shapes_ref as S
    g = case.ref("oracle", lambda: SF.oracle_shapes(_oracle(), c))
    lab, K, n = np.ascontiguousarray(c["labels"], np.int32), c["K"], len(c["labels"])
    med = float(np.median(g["radius"][g["valid"] == 1]))
    ref = case.ref("filter", lambda: S.cluster_filter(lab, K, g["radius"], g["valid"], g["rect_len"], g["rect_valid"], med, 2.0))
    if case.name.endswith("/dev"):
        d_lab, d_rad, d_val, d_len, d_rv = _dev(lab), _dev(g["radius"]), _dev(g["valid"]), _dev(g["rect_len"]), _dev(g["rect_valid"])
        d_f = torch.full((K,), 9, dtype=torch.uint8, device="cuda")
        d_keep = torch.full((n,), 9, dtype=torch.uint8, device="cuda")
        d_idx = torch.full((n,), -1, dtype=torch.int32, device="cuda")
        _sync()
        nf, nk = ctx.cluster_filter_dev(d_lab.data_ptr(), n, K, d_rad.data_ptr(), d_val.data_ptr(), d_len.data_ptr(),
                                        d_rv.data_ptr(), med, 2.0, d_f.data_ptr(), d_keep.data_ptr(), d_idx.data_ptr())
        got = dict(filtered=d_f.cpu().numpy(), keep=d_keep.cpu().numpy(), kept_idx=d_idx.cpu().numpy()[:nk], n_filtered=nf,
                   n_kept=nk)
    else:
        got = ctx.cluster_filter(lab, K, g["radius"], g["valid"], g["rect_len"], g["rect_valid"], med, 2.0)
    for k in ref:
        assert _same_nan(ref[k], got[k]), k
    assert 0 < ref["n_filtered"] < K


def _check_quant(case, ctx, c, poison):
    import test_cluster_quant_gpu as Q
    flat = np.ascontiguousarray(c["xy"]).reshape(-1)
    lab = np.ascontiguousarray(c["labels"], np.int32)
    if case.name.endswith("/mad"):
        Q._check_mad(ctx, flat, lab, c["K"], 3.0, 0.0, 2)
    else:
        Q._check_q(ctx, flat, lab, c["K"], Q.Q4, 2)


def _size_class_inputs():
    import cluster_quant_ref as R
    flat, group, K, sizes = R.size_class_case(12, 1)
    return dict(flat=flat, group=group, K=K)


def _check_quant_classes(case, ctx, inp, poison):
    """Every size class of csrc/cluster_quant.hip (the wave, the workgroup and the large segments' select states)."""
    import test_cluster_quant_gpu as Q
    if case.name.endswith("/mad"):
        Q._check_mad(ctx, inp["flat"], inp["group"], inp["K"], 3.0, 0.0, 1)
    else:
        Q._check_q(ctx, inp["flat"], inp["group"], inp["K"], Q.Q4, 1)


def _points(c, dim):
    return np.ascontiguousarray(c["xy"] if dim == 2 else np.c_[c["xy"], c["z"]])


def _check_moments(dim, weighted):
    def check(case, ctx, c, poison):
        import test_cluster_moments_gpu as M
        M._check(ctx, _points(c, dim), np.ascontiguousarray(c["labels"], np.int32), c["K"], c["w"] if weighted else None)
    return check


def _check_spheres(dim, weighted):
    def check(case, ctx, c, poison):
        import test_cluster_spheres_gpu as S
        S._check(ctx, _points(c, dim), np.ascontiguousarray(c["labels"], np.int32), c["K"], c["w"] if weighted else None, 0.0, 3)
    return check


def _shape_cases():
    out = []
    for name in SHAPE_FAMILIES:
        inp = _shape_inputs(name)
        first = Case("shapes/%s/host" % name, ("vcp_cluster_shapes", "vcp_mcc"), inp, _check_shapes)
        rest = [Case("shapes/%s/dev" % name, ("vcp_cluster_shapes_dev",), inp, _check_shapes),
                Case("filter/%s/host" % name, ("vcp_cluster_filter",), inp, _check_filter),
                Case("filter/%s/dev" % name, ("vcp_cluster_filter_dev",), inp, _check_filter),
                Case("quant/%s/quantiles" % name, ("vcp_cluster_quantiles", "vcp_cluster_quantiles_dev"), inp, _check_quant),
                Case("quant/%s/mad" % name, ("vcp_cluster_mad", "vcp_cluster_mad_dev"), inp, _check_quant)]
        for dim in (2, 3):
            for weighted in (False, True):
                tag = "%s/%dd%s" % (name, dim, "_w" if weighted else "")
                rest.append(Case("moments/" + tag, ("vcp_cluster_moments", "vcp_cluster_moments_dev"), inp,
                                 _check_moments(dim, weighted)))
                rest.append(Case("spheres/" + tag, ("vcp_cluster_spheres", "vcp_cluster_spheres_dev"), inp,
                                 _check_spheres(dim, weighted)))
        for r in rest:
            r.memo = first.memo
            r.inputs = first.inputs          # one family, built once
        out += [first] + rest
    out.append(Case("quant/size_classes/quantiles", ("vcp_cluster_quantiles", "vcp_cluster_quantiles_dev"), _size_class_inputs,
                    _check_quant_classes))
    out.append(Case("quant/size_classes/mad", ("vcp_cluster_mad", "vcp_cluster_mad_dev"), _size_class_inputs,
                    _check_quant_classes))
    return out


# ---- import and text -----------------------------------------------------------------------------------------------------------
def _import_inputs():
    import import_ref as I
    return I.load()


def _check_import_convert(case, ctx, f, poison):
    """tests/test_import_accuracy_gpu.py: the decisions are the oracle's, the values within its bound of the 60-digit ones."""
    import import_ref as I
    O = _oracle()
    L = 4.0 * I.HOST_SINCOS_UNITS
    bound = (2 * L + 1, 2 * L + 1, L + 0.5)
    g = ctx.import_convert(f["rows"], f["x_angle"], f["y_angle"], 2, 1, True)
    o = case.ref("oracle", lambda: O.import_convert(f["rows"], f["x_angle"], f["y_angle"], 2, 1, True))
    assert np.array_equal(g["state"], o["state"]) and g["kept"] == o["kept"] and g["duplicates"] == o["duplicates"] >= 100
    e = I.error_units(I.tmp_of(g["xyz"], 2, 1), f)
    for j in range(3):
        assert e[:, j].max() <= bound[j], (j, float(e[:, j].max()))


def _compact_inputs():
    import import_compact_ref as R
    rows, xa, ya = R.mixed_rows()
    return dict(rows=np.ascontiguousarray(rows, np.float64).reshape(-1, 3), xa=xa, ya=ya,
                group=(np.arange(len(rows)) % 3).astype(np.int32))


def _check_import_compact(case, ctx, inp, poison):
    """tests/test_import_compact_gpu.py: the restatement runs on vcp_import_convert(dedupe = 0)'s values, asked for AFTER the
    call under test (those values have a case of their own)."""
    import fuzz_import_compact as F
    import import_compact_ref as R
    rows, xa, ya = inp["rows"], inp["xa"], inp["ya"]
    grouped, dev = "/grouped" in case.name, case.name.endswith("/dev")
    group = inp["group"] if grouped else None
    got = F.run_dev(ctx, rows, group, xa, ya, True, 2, 1) if dev else ctx.import_compact(rows, group, xa, ya, 2, 1, True)
    c = ctx.import_convert(rows, xa, ya, 2, 1, dedupe=False)
    bad = R.same(got, R.compact(rows, c["xyz"], c["state"], group, True))
    assert bad is None, "%s differs" % bad


def _text_inputs():
    import scantext_corpus as K
    import scantext_ref as R
    fields = K.value_fields()
    host = [s for s in fields if R.field_class(s)[0] == 3][:4]      # fields the device leaves to the host: the patch path
    assert host
    return dict(text=K.lines(fields[:600] + host))


def _check_parse(case, ctx, inp, poison):
    import test_scantext_gpu as TS
    got = TS.held(ctx, inp["text"])
    assert got["n_host"] >= 1 and got["n"] == len(inp["text"].splitlines())


def _format_inputs():
    import scanfmt_corpus as K
    v = np.array(K.SUPPORTED[:1800], np.float64).reshape(-1, 3)
    rng = np.random.default_rng(6)
    return dict(v=v, ids=rng.integers(-2 ** 31, 2 ** 31, len(v)).astype(np.int32), order=rng.permutation(len(v))[:500].astype(np.int64))


def _check_format(case, ctx, inp, poison):
    import test_scanfmt_gpu as TF
    v = inp["v"]
    if case.name.endswith("/order"):
        TF.both_forms(ctx, v[:, 0], v[:, 1], v[:, 2], ids=inp["ids"], order=inp["order"], bit=9, eol=0)
    else:
        TF.both_forms(ctx, v[:, 0], v[:, 1], v[:, 2], bit=6, eol=1)


# ---- the device self-tests ---------------------------------------------------------------------------------------------------
SCAN_N = 3 * 8192 + 5     # four tiles of the scan: the look-back crosses every tile boundary


def _scan_inputs():
    rng = np.random.default_rng(8)
    return dict(v=rng.integers(0, 1 << 32, SCAN_N, dtype=np.uint64).astype(np.uint32))


def scan_reference(v):
    """(exclusive sums modulo 2^32, their total, exclusive running maxima, the maximum) of uint32 v."""
    v64 = v.astype(np.uint64)
    cs = np.cumsum(v64)
    mx = np.maximum.accumulate(v)
    return (((cs - v64) & 0xFFFFFFFF).astype(np.uint32), int(cs[-1]) & 0xFFFFFFFF,
            np.concatenate([[0], mx[:-1]]).astype(np.uint32), int(mx[-1]))


def check_scan(ctx, v, d_in, d_out, want):
    """One sum scan and one maximum scan of the resident d_in into d_out against scan_reference's `want`."""
    for op, (out, tot) in ((0, want[:2]), (1, want[2:])):
        d_out.fill_(-1)
        _sync()
        total = ctx.selftest_scan_dev(d_in.data_ptr(), d_out.data_ptr(), len(v), op)
        got = d_out.cpu().numpy().view(np.uint32)
        assert total == tot, ("total", op)
        assert np.array_equal(got, out), ("op %d: first difference at %s" % (op, np.flatnonzero(got != out)[:3]))


def _check_scan(case, ctx, inp, poison):
    import torch
    v = inp["v"]
    d_in = _dev(v.view(np.int32))
    d_out = torch.zeros(len(v), dtype=torch.int32, device="cuda")
    check_scan(ctx, v, d_in, d_out, case.ref("want", lambda: scan_reference(v)))


def _check_wave(case, ctx, inp, poison):
    """tests/test_wave_gpu.py at one size: a workgroup of 256, 255 entries read."""
    import torch
    import test_wave_gpu as W
    tb, n = 256, 255
    rng = np.random.default_rng(tb)
    w = rng.integers(0, 1 << 32, tb, dtype=np.uint64).astype(np.uint32)
    f = rng.integers(0, 2, tb).astype(bool)
    v, p = w.copy(), f.copy()
    v[n:], p[n:] = 0, False
    d_words, d_flags = _dev(w.view(np.int32)), _dev(f.astype(np.uint8) * 3)
    d_counter = torch.full((1,), W.START - (1 << 32), dtype=torch.int32, device="cuda")
    d_out = torch.full((W.ROWS * tb,), -1, dtype=torch.int32, device="cuda")
    _sync()
    ctx.selftest_wave_dev(d_words.data_ptr(), d_flags.data_ptr(), n, tb, d_counter.data_ptr(), d_out.data_ptr())
    out = d_out.cpu().numpy().view(np.uint32).reshape(W.ROWS, tb).astype(np.uint64)
    ref, P = W.reference(v, p, tb)
    for r, want in ref.items():
        assert np.array_equal(out[r], want), "row %d" % r
    assert int(d_counter.cpu().numpy().view(np.uint32)[0]) == (W.START + P) & W.M32


def _check_format_total(case, ctx, inp, poison):
    words = np.random.default_rng(3).integers(0, 1 << 32, 1001, dtype=np.uint64).astype(np.uint32)
    t = _dev(words.view(np.int32))
    _sync()
    assert ctx.selftest_format_total_dev(t.data_ptr(), len(words)) == int(words.astype(np.uint64).sum())


# ---- the table ---------------------------------------------------------------------------------------------------------------
def build_cases():
    import fuzz_queries as F
    t = _engine_cases() + _block_cases()
    t.append(Case("dead/one_d", ("vcp_dbscan",), _dead_inputs(True), _check_dead))
    t.append(Case("dead/pairs", ("vcp_dbscan",), _dead_inputs(False), _check_dead))
    lists = {}
    for family in F.FAMILIES:
        t += [_fuzz_case(family, i, lists) for i in range(FUZZ_COUNT)]
    for n in (3000, 591, 592):
        t.append(Case("query/eps_tree/heavy_%d" % n, ("vcp_eps_tree", "vcp_eps_tree_dev"), _heavy_cell(n), _check_heavy_eps_tree))
        t.append(Case("query/gdbscan/heavy_%d" % n, ("vcp_gdbscan", "vcp_gdbscan_dev"), _heavy_cell(n), _check_heavy_gdbscan))
    t.append(Case("query/kdist/heavy", ("vcp_kdist", "vcp_kdist_dev"), _kdist_heavy_inputs, _check_kdist_heavy))
    t.append(Case("query/eps_inf", ("vcp_gdbscan", "vcp_gdbscan_dev", "vcp_dbscan"), _eps_inf_inputs, _check_eps_inf))
    t += _pass_cases() + _run_cases()
    for T in (300, 700):          # at most 512 truths: the scan; beyond: the truths are binned (csrc/nngrid.hpp)
        t.append(Case("match/%d" % T, ("vcp_match", "vcp_assign_truths"), _match_inputs(T), _check_match))
    cen = Case("centroids/plain", ("vcp_centroids", "vcp_centroids_dev"), _centroid_inputs, _check_centroids("plain"))
    more = [Case("centroids/dev", ("vcp_centroids_dev",), _centroid_inputs, _check_centroids("dev")),
            Case("centroids/weighted", ("vcp_centroids_weighted",), _centroid_inputs, _check_centroids("weighted")),
            Case("centroids/refresh_merge", ("vcp_refresh_by_dictionary", "vcp_merge_centroids"), _centroid_inputs,
                 _check_centroids("refresh"))]
    for c in more:
        c.memo, c.inputs = cen.memo, cen.inputs
    t += [cen] + more + _shape_cases()
    t.append(Case("import/convert", ("vcp_import_convert",), _import_inputs, _check_import_convert))
    for tag, funcs in (("host", ("vcp_import_compact", "vcp_import_compact_dev")), ("dev", ("vcp_import_compact_dev",)),
                       ("grouped/host", ("vcp_import_compact", "vcp_import_compact_dev")), ("grouped/dev", ("vcp_import_compact_dev",))):
        t.append(Case("import/compact/" + tag, funcs + ("vcp_import_convert",), _compact_inputs, _check_import_compact))
    t.append(Case("text/parse", ("vcp_parse_scan_text", "vcp_parse_scan_text_dev"), _text_inputs, _check_parse))
    t.append(Case("text/format", ("vcp_format_rows", "vcp_format_rows_dev"), _format_inputs, _check_format))
    t.append(Case("text/format/order", ("vcp_format_rows", "vcp_format_rows_dev"), _format_inputs, _check_format))
    t.append(Case("selftest/scan", ("vcp_selftest_scan_dev",), _scan_inputs, _check_scan))
    t.append(Case("selftest/wave", ("vcp_selftest_wave_dev",), lambda: dict(), _check_wave))
    t.append(Case("selftest/format_total", ("vcp_selftest_format_total_dev",), lambda: dict(), _check_format_total))
    names = [c.name for c in t]
    assert len(set(names)) == len(names)
    return t


CASES = build_cases()
BY_NAME = {c.name: c for c in CASES}
