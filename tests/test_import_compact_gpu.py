"""vcp_import_compact on the MI355X: the seven arrays, row_to, m and duplicates equal to the restatement of the definition
(tests/import_compact_ref.py) run on the device's own vcp_import_convert(dedupe = 0) values, and src / xyz / duplicates
equal to vcp_import_convert itself, on the smallest shapes at which each mechanism can go wrong; the device-pointer form,
NULL outputs, errors, independence from the context's history, the caller's stream, the chain into vcp_gdbscan_dev /
vcp_dbscan / vcp_centroids_weighted, add_fixed_folder and the bounded fuzz.  Every comparison is equality, doubles by
their bits."""
import ctypes as C

import numpy as np
import pytest
import torch

import fuzz_import_compact as F
import import_compact_ref as R
from vtkcloudpoint_amd import _native as N

pytestmark = pytest.mark.gpu


def _ref(ctx, rows, xa=0.0, ya=0.0, group=None, dedupe=True, xdir=2, ydir=1):
    c = ctx.import_convert(rows, xa, ya, xdir, ydir, dedupe=False)
    return R.compact(rows, c["xyz"], c["state"], group, dedupe)


def _check(ctx, rows, xa=0.0, ya=0.0, group=None, dedupe=True, xdir=2, ydir=1, want=None):
    """Host form and device-pointer form == restatement; returns the restatement."""
    rows = np.ascontiguousarray(rows, np.float64).reshape(-1, 3)
    want = want or _ref(ctx, rows, xa, ya, group, dedupe, xdir, ydir)
    what = "(n %d, dedupe %s, grouped %s)" % (len(rows), dedupe, group is not None)
    bad = R.same(ctx.import_compact(rows, group, xa, ya, xdir, ydir, dedupe), want)
    assert bad is None, "host form: %s differs %s" % (bad, what)
    bad = R.same(F.run_dev(ctx, rows, group, xa, ya, dedupe, xdir, ydir), want)
    assert bad is None, "device form: %s differs %s" % (bad, what)
    return want


def _identities(ctx, rows, xa, ya, got, dedupe=True):
    d = ctx.import_convert(rows, xa, ya, 2, 1, dedupe=dedupe)
    assert np.array_equal(got["src"], np.nonzero(d["state"] == 1)[0]) and got["duplicates"] == d["duplicates"]
    assert np.array_equal(got["xyz"].view(np.uint64), d["xyz"][got["src"]].view(np.uint64))
    assert int(got["count"].sum()) == int((d["state"] != 0).sum())


@pytest.mark.parametrize("n", [0, 1, 255, 256, 257])
def test_workgroup_and_wave_edges(vcp_ctx, n):
    rng = np.random.default_rng(n)
    base = np.c_[rng.uniform(0, 40, (max(n, 1), 2)), rng.uniform(1, 900, max(n, 1))]
    rows = base[np.arange(n) % max(1, (2 * n) // 3)]            # the last third repeats the first
    if n:
        rows[n // 2, 2] = 0.0                                   # one filtered row; the very last row is a duplicate
    for dedupe in (True, False):
        w = _check(vcp_ctx, rows, 1.5, -0.5, dedupe=dedupe)
        _check(vcp_ctx, rows, 1.5, -0.5, group=np.arange(n, dtype=np.int32) % 2, dedupe=dedupe)
        assert w["m"] + w["duplicates"] == max(n - 1, 0)
        assert w["duplicates"] == (0 if not dedupe or n < 2 else n - 1 - len(np.unique(rows[rows[:, 2] != 0], axis=0)))
    assert n < 255 or _ref(vcp_ctx, rows, 1.5, -0.5)["duplicates"] > 80


def test_one_hot_class(vcp_ctx):
    rows = np.tile([[3.25, 4.5, 100.0]], (4096, 1))
    w = _check(vcp_ctx, rows, 1.5, -0.5)
    assert w["m"] == 1 and w["count"].tolist() == [4096] and not w["row_to"].any() and w["duplicates"] == 4095
    g = vcp_ctx.import_compact(rows, None, 1.5, -0.5)
    assert g["m"] == 1 and g["count"].tolist() == [4096] and not g["row_to"].any() and g["src"].tolist() == [0]


@pytest.fixture(scope="module")
def mixed(vcp_ctx):
    rows, xa, ya = R.mixed_rows()
    return rows, xa, ya, _ref(vcp_ctx, rows, xa, ya)


def test_mixed_case(vcp_ctx, mixed):
    rows, xa, ya, want = mixed
    _check(vcp_ctx, rows, xa, ya, want=want)
    _identities(vcp_ctx, rows, xa, ya, vcp_ctx.import_compact(rows, None, xa, ya))
    plain = _check(vcp_ctx, rows, xa, ya, dedupe=False)
    _identities(vcp_ctx, rows, xa, ya, vcp_ctx.import_compact(rows, None, xa, ya, dedupe=False), dedupe=False)
    # what the case is there for
    D, kept = rows[:, 2], np.zeros(len(rows), bool)
    kept[want["src"]] = True
    assert 1000 <= want["m"] <= 1400 and 1 <= want["count"].min() and want["count"].max() == 9
    assert (want["row_to"] == -1).sum() == len(rows) // 10 == ((D == 0) | (D > 1000)).sum()
    assert (want["row_to"][D == 0] == -1).all() and (want["row_to"][D == 1000.5] == -1).all() and (D == 1000.5).any()
    assert kept[D == 1000.0].all() and (D == 1000.0).sum() == 1 and kept[D == -3.5].all() and (D == -3.5).sum() == 1
    nan_mx = np.nonzero(np.isnan(rows[:, 0]))[0]
    assert len(nan_mx) == 2 and kept[nan_mx].all() and want["count"][want["row_to"][nan_mx]].tolist() == [1, 1]
    nan_d = np.nonzero(np.isnan(D))[0]
    assert len(nan_d) == 1 and kept[nan_d].all()
    assert plain["m"] == len(rows) - len(rows) // 10 and (plain["count"] == 1).all()
    # other directions without the duplicate search: xyz is the direction-mapped one
    for xdir, ydir in ((1, 2), (3, 4), (4, 3)):
        _check(vcp_ctx, rows, xa, ya, dedupe=False, xdir=xdir, ydir=ydir)


def test_minus_zero_equals_plus_zero(vcp_ctx):
    rows = R.zero_pair()
    c = vcp_ctx.import_convert(rows, 0.0, 0.0, 2, 1, dedupe=False)
    ty = c["xyz"][:, 1]
    assert ty[0] == ty[1] == 0 and np.signbit(ty[0]) and not np.signbit(ty[1])       # the two tmpy differ in bits
    assert np.array_equal(c["xyz"][0, [0, 2]].view(np.uint64), c["xyz"][1, [0, 2]].view(np.uint64))
    for r in (rows, rows[::-1].copy()):
        w = _check(vcp_ctx, r, 0.0, 0.0)
        assert w["m"] == 1 and w["count"].tolist() == [2] and w["row_to"].tolist() == [0, 0]
        g = vcp_ctx.import_compact(r, None, 0.0, 0.0)
        assert g["count"].tolist() == [2] and g["src"].tolist() == [0]
        assert bool(np.signbit(g["xyz"][0, 1])) == bool(np.signbit(r[0, 0] * -2))      # the first row's sign bit
    # among 300 other rows, in two groups: one class per group
    rng = np.random.default_rng(3)
    more = np.r_[np.c_[rng.uniform(1, 40, (300, 2)), rng.uniform(1, 900, 300)], rows, rows]
    more = more[rng.permutation(len(more))]
    w = _check(vcp_ctx, more, 0.0, 0.0)
    assert w["m"] == 301 and sorted(w["count"].tolist())[-1] == 4
    group = (np.arange(len(more)) % 2).astype(np.int32)
    _check(vcp_ctx, more, 0.0, 0.0, group=group)


def test_probing_on_distinct_rows(vcp_ctx):
    n = 20_000
    rows = np.c_[np.arange(n) * 0.001, (np.arange(n) % 97) * 0.25, 5.0 + np.arange(n) * 0.01]
    g = vcp_ctx.import_compact(rows, None, 1.5, -0.5)
    assert g["m"] == n and g["duplicates"] == 0 and (g["count"] == 1).all()
    assert np.array_equal(g["src"], np.arange(n)) and np.array_equal(g["row_to"], np.arange(n))
    _check(vcp_ctx, rows, 1.5, -0.5)


def test_groups(vcp_ctx):
    rng = np.random.default_rng(12)
    one = R.expanded(rng, 600, 2000)[rng.permutation(2000)]
    one[::50, 2] = 0.0
    gids = np.array([7, -2, 0], np.int32)
    rows = np.repeat(one, 3, axis=0)                              # row i of group k sits at 3 i + k: interleaved
    group = np.tile(gids, 2000)
    alone = _ref(vcp_ctx, one, 1.5, -0.5)
    w = _check(vcp_ctx, rows, 1.5, -0.5, group=group)
    assert alone["duplicates"] > 500 and w["m"] == 3 * alone["m"] and w["duplicates"] == 3 * alone["duplicates"]
    for k, g in enumerate(gids):
        sel = w["group"] == g
        assert sel.sum() == alone["m"]
        assert np.array_equal(w["src"][sel], 3 * alone["src"] + k) and np.array_equal(w["count"][sel], alone["count"])
    assert np.array_equal(w["group"], group[w["src"]])
    # without groups the three copies fall into one class
    flat = _check(vcp_ctx, rows, 1.5, -0.5)
    assert flat["m"] == alone["m"] and np.array_equal(flat["count"], 3 * alone["count"])
    # a group given without the duplicate search is passed through
    p = _check(vcp_ctx, rows, 1.5, -0.5, group=group, dedupe=False)
    assert np.array_equal(p["group"], group[p["src"]]) and (p["count"] == 1).all() and set(p["group"]) == {7, -2, 0}
    # the extreme group numbers
    _check(vcp_ctx, rows, 1.5, -0.5, group=np.where(group == 7, 2 ** 31 - 1, -2 ** 31).astype(np.int32))


OUTS = ("motor", "xyz", "dist", "src", "count", "group", "row_to")


def _raw(ctx, rows, fn="vcp_import_compact", group=None, n=None, xdir=2, ydir=1, dedupe=1, handle=True, with_rows=True,
         with_m=True, skip=()):
    """The C entry point on poisoned outputs (host arrays, or device tensors for the _dev form).  Returns (status, m,
    duplicates, the outputs as host arrays, untouched?)."""
    rows = np.ascontiguousarray(rows, np.float64).reshape(-1, 3)
    cnt = len(rows)
    room = max(cnt, 1)
    grp = None if group is None else np.ascontiguousarray(group, np.int32)
    shape = dict(motor=(room, 2), xyz=(room, 3), dist=(room,))
    host = {k: np.full(shape[k], -7.25) if k in shape else np.full(room, -9, np.int32) for k in OUTS}
    dev = fn.endswith("_dev")
    if dev:
        keep = [torch.from_numpy(rows).cuda(), None if grp is None else torch.from_numpy(grp).cuda()]
        bufs = {k: torch.from_numpy(v).cuda() for k, v in host.items()}
        torch.cuda.synchronize()
        p_rows, p_grp = keep[0].data_ptr(), None if grp is None else keep[1].data_ptr()
        ptr = {k: C.c_void_p(v.data_ptr()) for k, v in bufs.items()}
    else:
        p_rows, p_grp = rows.ctypes.data, None if grp is None else grp.ctypes.data
        ptr = {k: N._ptr(v) for k, v in host.items()}
    m, dup = C.c_int64(-3), C.c_int64(-4)
    rc = getattr(N.lib(), fn)(ctx._h if handle else None, C.c_void_p(p_rows) if with_rows else None,
                              C.c_int64(cnt if n is None else n), None if p_grp is None else C.c_void_p(p_grp),
                              C.c_double(1.5), C.c_double(-0.5), int(xdir), int(ydir), int(dedupe),
                              *[None if k in skip else ptr[k] for k in OUTS], C.byref(m) if with_m else None, C.byref(dup))
    if dev:
        torch.cuda.synchronize()
        host = {k: v.cpu().numpy() for k, v in bufs.items()}
    untouched = all((host[k] == (-7.25 if k in shape else -9)).all() for k in OUTS) and m.value == -3 and dup.value == -4
    return rc, m.value, dup.value, host, bool(untouched)


@pytest.mark.parametrize("fn", ["vcp_import_compact", "vcp_import_compact_dev"])
def test_null_outputs(vcp_ctx, mixed, fn):
    rows, xa, ya, _ = mixed
    group = (np.arange(len(rows)) % 3).astype(np.int32)
    want = _ref(vcp_ctx, rows, 1.5, -0.5, group)
    m = want["m"]
    for skip in [(k,) for k in OUTS] + [OUTS]:
        rc, gm, gdup, out, _ = _raw(vcp_ctx, rows, fn, group=group, skip=skip)
        assert (rc, gm, gdup) == (0, m, want["duplicates"]), skip
        for k in OUTS:
            a = out[k]
            if k in skip:
                assert (a == (-7.25 if a.dtype == np.float64 else -9)).all(), (skip, k)
            else:
                got = a[: len(rows)] if k == "row_to" else a[:m]
                assert np.array_equal(np.ascontiguousarray(got).view(np.uint64 if a.dtype == np.float64 else np.int32),
                                      want[k].view(np.uint64 if a.dtype == np.float64 else np.int32)), (skip, k)
    # duplicates may be NULL too
    mm = C.c_int64(-3)
    d = torch.from_numpy(rows).cuda()
    torch.cuda.synchronize()
    p = C.c_void_p(d.data_ptr()) if fn.endswith("_dev") else N._ptr(rows)
    assert getattr(N.lib(), fn)(vcp_ctx._h, p, C.c_int64(len(rows)), None, C.c_double(1.5), C.c_double(-0.5), 2, 1, 1,
                                *[None] * 7, C.byref(mm), None) == 0
    assert mm.value == _ref(vcp_ctx, rows, 1.5, -0.5)["m"]


@pytest.mark.parametrize("fn", ["vcp_import_compact", "vcp_import_compact_dev"])
def test_error_codes_leave_the_outputs_untouched(vcp_ctx, fn):
    ARG, TOO_LARGE, UNSUPPORTED = -1, -5, -8
    rows = np.c_[np.arange(8.0), np.arange(8.0), np.full(8, 5.0)]

    def status(**kw):
        rc, _, _, _, untouched = _raw(vcp_ctx, rows, fn, **kw)
        return rc, untouched

    assert status(handle=False) == (ARG, True)
    assert status(with_m=False) == (ARG, True)
    assert status(with_rows=False) == (ARG, True)
    assert status(n=-1) == (ARG, True)
    for xdir, ydir in ((0, 1), (5, 1), (2, 0), (2, 5), (-1, -1)):
        assert status(xdir=xdir, ydir=ydir) == (ARG, True)
        assert status(xdir=xdir, ydir=ydir, dedupe=0) == (ARG, True)
    for xdir, ydir in ((1, 1), (2, 2), (1, 2), (4, 3)):
        assert status(xdir=xdir, ydir=ydir) == (UNSUPPORTED, True)
        assert status(xdir=xdir, ydir=ydir, dedupe=0) == (0, False)
    assert status(n=0x7FFFFFF0) == (TOO_LARGE, True)
    assert status(n=1 << 40, dedupe=0) == (TOO_LARGE, True)
    assert status() == (0, False)
    with pytest.raises(N.VcpError) as e:
        vcp_ctx.import_compact(rows, None, 0.0, 0.0, 1, 1)
    assert e.value.code == UNSUPPORTED and "xdir=2" in str(e.value)
    # n == 0: *m = 0, nothing else (rows may be NULL)
    rc, m, dup, _, _ = _raw(vcp_ctx, np.zeros((0, 3)), fn, with_rows=False)
    assert (rc, m, dup) == (0, 0, 0)
    # and the call after the errors is a clean one
    w = _check(vcp_ctx, rows, 1.5, -0.5)
    assert w["m"] == 8


def test_two_calls_and_the_context_history(vcp_ctx, mixed):
    rows, xa, ya, want = mixed
    group = (np.arange(len(rows)) % 4 - 1).astype(np.int32)
    a = vcp_ctx.import_compact(rows, group, xa, ya)
    b = vcp_ctx.import_compact(rows, group, xa, ya)
    assert R.same(a, b) is None                                           # two calls: identical bits
    c = np.random.default_rng(2).uniform(0, 4, (3000, 2))
    lab = torch.zeros(3000, dtype=torch.int32, device="cuda")
    t = torch.from_numpy(c).cuda()
    torch.cuda.synchronize()
    vcp_ctx.dbscan_dev(t.data_ptr(), 3000, 2, 0.1, 4, d_labels=lab.data_ptr())
    vcp_ctx.import_compact(rows[:100], None, xa, ya)                      # a smaller call leaves a table behind
    vcp_ctx.import_convert(rows, xa, ya)
    assert R.same(vcp_ctx.import_compact(rows, group, xa, ya), a) is None  # after other calls on the same context
    assert R.same(F.run_dev(vcp_ctx, rows, group, xa, ya, True), a) is None
    fresh = N.Context(0)
    try:
        assert R.same(fresh.import_compact(rows, group, xa, ya), a) is None
    finally:
        fresh.close()


def test_timing_phases(vcp_ctx, mixed):
    rows, xa, ya, _ = mixed
    vcp_ctx.timing_enable(True)
    try:
        vcp_ctx.import_compact(rows, None, xa, ya)
        names = [nm for nm, _ in vcp_ctx.timing()]
    finally:
        vcp_ctx.timing_enable(False)
    assert names == ["impc_convert", "impc_dedupe", "impc_compact"]


@pytest.fixture(scope="module")
def scan():
    return R.scan_rows()


def test_chain_into_gdbscan_dbscan_and_centroids(vcp_ctx, scan):
    from vtkcloudpoint_amd import io
    from vtkcloudpoint_amd.gdbscan import multiplicity
    raw, xa, ya = scan
    eps, mw, gate = 0.12, 12, 5.0
    res = io.import_scan_resident(raw, x_angle=xa, y_angle=ya, ctx=vcp_ctx)
    m = res["m"]
    assert 2500 < m <= 3000 and res["duplicates"] == 9000 - m
    want = _ref(vcp_ctx, raw, xa, ya)
    got = {k: res[k].cpu().numpy() for k in OUTS}
    got.update(m=m, duplicates=res["duplicates"])
    assert R.same(got, want) is None
    # (a) gdbscan_dev on the resident arrays == gdbscan on the host route
    lab = torch.full((m,), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    cf = vcp_ctx.gdbscan_dev(res["motor"].data_ptr(), m, 2, eps, mw, lab.data_ptr(), N.L1_2D,
                             d_weights=res["count"].data_ptr(), d_aux=res["dist"].data_ptr(), gate=gate)
    c = vcp_ctx.import_convert(raw, xa, ya, 2, 1, dedupe=False)
    unf = np.nonzero(c["state"] != 0)[0]
    q = c["xyz"][unf]
    assert not np.isnan(q).any() and not (np.signbit(q) & (q == 0)).any()
    first, cnt = multiplicity(q)
    h = vcp_ctx.gdbscan(raw[unf[first], :2], eps, mw, N.L1_2D, weights=cnt, aux=raw[unf[first], 2], gate=gate)
    assert cf == h["cf"] and cf >= 12 and np.array_equal(lab.cpu().numpy(), h["labels"])
    # (b) without the gate, labels[row_to] is vcp_dbscan on the raw unfiltered rows at min_pts = min_weight
    cf2 = vcp_ctx.gdbscan_dev(res["motor"].data_ptr(), m, 2, eps, mw, lab.data_ptr(), N.L1_2D,
                              d_weights=res["count"].data_ptr())
    d = vcp_ctx.dbscan(raw[unf, :2], eps, mw, N.L1_2D)
    row_to = got["row_to"]
    assert np.array_equal(row_to >= 0, c["state"] != 0)
    assert cf2 == d["cf"] and cf2 >= 6 and np.array_equal(lab.cpu().numpy()[row_to[unf]], d["labels"])
    assert (d["labels"] == 0).any() and (d["labels"] != 0).any()
    # (c) a grouped import feeds centroids_weighted what the restatement feeds it
    group = (1 + np.arange(len(raw)) % 3).astype(np.int32)
    g = vcp_ctx.import_compact(raw, group, xa, ya)
    w = _ref(vcp_ctx, raw, xa, ya, group)
    assert R.same(g, w) is None and g["count"].max() >= 2
    for ignore in (False, True):
        for cid in (None, np.zeros(g["m"], np.int32)):
            a3, ains = vcp_ctx.centroids_weighted(g["xyz"], g["group"], cid, g["count"], 3, ignore)
            b3, bins = vcp_ctx.centroids_weighted(w["xyz"], w["group"], cid, w["count"], 3, ignore)
            assert np.array_equal(a3.view(np.uint64), b3.view(np.uint64)) and np.array_equal(ains, bins)
            assert np.isfinite(a3).all() and ains.min() > 0


def test_on_the_callers_stream(scan):
    """The copy that fills d_rows is queued on the caller's stream behind a 20 ms filler; the call follows at once.  A
    kernel or copy on another stream would read the rows that were there before."""
    raw, xa, ya = scan
    ctx = N.Context(0)
    try:
        s = torch.cuda.Stream()
        ctx.set_stream(s.cuda_stream)
        n = len(raw)
        before = raw[::-1].copy()
        before[:, 2] = 7.0                                              # cloud A: nothing filtered, other classes
        want_a, want = _ref(ctx, before, xa, ya), _ref(ctx, raw, xa, ya)
        assert want_a["m"] != want["m"]
        d_rows = torch.from_numpy(before).cuda()
        b = torch.from_numpy(raw).cuda()
        out = dict(motor=torch.zeros(n * 2, dtype=torch.float64, device="cuda"),
                   xyz=torch.zeros(n * 3, dtype=torch.float64, device="cuda"),
                   dist=torch.zeros(n, dtype=torch.float64, device="cuda"))
        out.update({k: torch.zeros(n, dtype=torch.int32, device="cuda") for k in ("src", "count", "group", "row_to")})
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            torch.cuda._sleep(50_000_000)                               # some 20 ms
            d_rows.copy_(b, non_blocking=True)
            for k in ("src", "row_to"):
                out[k].fill_(-9)
        assert not s.query()                                            # the filler still runs
        m, dup = ctx.import_compact_dev(d_rows.data_ptr(), n, None, xa, ya, 2, 1, True, out["motor"].data_ptr(),
                                        out["xyz"].data_ptr(), out["dist"].data_ptr(), out["src"].data_ptr(),
                                        out["count"].data_ptr(), out["group"].data_ptr(), out["row_to"].data_ptr())
        assert s.query()                                                # the call blocked until its work on s was done
        got = dict(m=m, duplicates=dup, motor=out["motor"].cpu().numpy()[: 2 * m].reshape(m, 2),
                   xyz=out["xyz"].cpu().numpy()[: 3 * m].reshape(m, 3), dist=out["dist"].cpu().numpy()[:m],
                   src=out["src"].cpu().numpy()[:m], count=out["count"].cpu().numpy()[:m],
                   group=out["group"].cpu().numpy()[:m], row_to=out["row_to"].cpu().numpy())
        assert R.same(got, want) is None
    finally:
        ctx.set_stream(0)
        ctx.close()


def test_add_fixed_folder(vcp_ctx, tmp_path):
    from vtkcloudpoint_amd import io
    rng = np.random.default_rng(5)
    pool = np.c_[np.round(rng.uniform(0, 40, (40, 2)) * 64) / 64, np.round(rng.uniform(1, 900, 40) * 8) / 8]
    files, per_file = [], []
    for k, cnt in enumerate((60, 1, 45)):
        r = pool[rng.integers(0, 40, cnt)]                        # the files share rows: duplicates are per file
        if cnt > 10:
            r[5, 2], r[9, 2] = 0.0, 1000.5
        path = tmp_path / ("fixed%d.pts.txt" % k)
        path.write_text("".join("%r\t%r\t%r\n" % tuple(float(v) for v in row) for row in r))
        files.append(str(path))
        per_file.append(r)
    xa, ya = 1.51, -0.53
    for typpe in (3, 4):
        clus, dup, pts, paths = io.add_fixed_folder(files, xa, ya, typpe=typpe, ctx=vcp_ctx)
        # the literal walk of FrmMain.cs:1069-1085 on the device's X, Y, Z
        want, w_dup, w_pts = [], 0, 0
        for k, r in enumerate(per_file):
            c = vcp_ctx.import_convert(r, xa, ya, 2, 1, dedupe=False)
            li = []
            for i in range(len(r)):
                if r[i, 2] == 0 or r[i, 2] > 1000:
                    continue
                x, y, z = c["xyz"][i].tolist()
                found = [p for p in li if p["X"] == x and p["Y"] == y and p["Z"] == z]
                if not found:
                    li.append(dict(X=x, Y=y, Z=z, ptsCount=1, row=r[i].tolist()))
                    w_pts += 1
                else:
                    found[0]["ptsCount"] += 1
                    if typpe == 3:
                        w_dup += 1
                    else:
                        w_pts += 1
            want.append(li)
        assert (dup, pts, paths) == (w_dup, w_pts, files) and len(clus) == 3
        assert w_dup > 20 or typpe == 4
        for k, (cl, li) in enumerate(zip(clus, want)):
            assert [(p.X, p.Y, p.Z, p.ptsCount) for p in cl.li] == [(p["X"], p["Y"], p["Z"], p["ptsCount"]) for p in li]
            assert [[p.motor_x, p.motor_y, p.Distance] for p in cl.li] == [p["row"] for p in li]
            assert all(p.clusterId == k + 1 and p.pathId == k and p.pointName == "fixed%d" % k for p in cl.li)
    with pytest.raises(ValueError):
        io.add_fixed_folder(files, typpe=1, ctx=vcp_ctx)
    assert io.add_fixed_folder([], typpe=3, ctx=vcp_ctx) == ([], 0, 0, [])


def test_bounded_fuzz(vcp_ctx):
    count, seed = F.SUITE
    lst = F.cases(count, seed)
    s = F.summary(lst, [F.check(vcp_ctx, c) for c in lst])
    print(s)
    assert s["cases"] == count and s["duplicates"] > 10_000 and s["grouped"] >= 8 and s["dev"] >= 6 and s["plain"] >= 2
    assert s["largest"] > 10_000 and s["big_class"] >= 100
