"""Plane extraction on the MI355X (include/vcp_planes.h) against the numpy restatement tests/plane_ref.py, for equality:
counts, every plane as bits, labels, valid, n_planes.  The sizes come from vcp_plane_score_shape: the tile, the chunk of
hypotheses and the grid's cap are where the score kernel takes another path."""
import ctypes as C

import numpy as np
import pytest
import torch

import plane_ref as R
from vtkcloudpoint_amd import planes as PL

pytestmark = pytest.mark.gpu

NAN_BITS = 0x7FF8000000000000


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()                       # a copy: the shared inputs are read-only


def host(t):
    return t.cpu().numpy()


def ptr(t):
    return None if t is None else (t.ctypes.data if isinstance(t, np.ndarray) else t.data_ptr())


@pytest.fixture(scope="module")
def shape(vcp_ctx):
    tile, chunk, grid = PL.plane_score_shape(vcp_ctx)
    assert 64 <= tile <= 1024 and tile % 64 == 0 and chunk >= 64 and 1 <= grid <= 8 * 256
    return dict(tile=tile, chunk=chunk, grid=grid)


def check_score(ctx, pts, planes, thr, active=None):
    """Both forms of the score against the restatement; returns the counts."""
    want = R.score(pts, planes, thr, active)
    got = PL.plane_score(pts, planes, thr, active, ctx=ctx)
    assert got.dtype == np.int64 and np.array_equal(got, want), (np.nonzero(got != want)[0][:8], got[:4], want[:4])
    d = host(PL.plane_score(dev(pts), dev(planes), thr, None if active is None else dev(active), ctx=ctx))
    assert np.array_equal(d, want)
    return want


# ---- the score: sizes ---------------------------------------------------------------------------------------------------------
N_CASES = ("0", "1", "63", "64", "65", "tile-1", "tile", "tile+1", "3*tile+5")
H_CASES = ("1", "63", "64", "65", "chunk", "chunk+1")


@pytest.mark.parametrize("n_case", N_CASES)
def test_score_sizes(vcp_ctx, shape, n_case):
    n = eval(n_case, dict(shape))
    pts = R.lattice_rows(n, 1).reshape(n, 3)
    seen = 0
    for h_case in H_CASES:
        H = eval(h_case, dict(shape))
        seen += int(check_score(vcp_ctx, pts, R.generic_planes(H, H), 0.25).sum())
    assert seen > 0 or n < 63                                                    # the planes cross the cloud


def test_score_a_workgroup_takes_a_second_tile(vcp_ctx, shape):
    n = (shape["grid"] + 1) * shape["tile"] + 1
    pts = R.lattice_rows(n, 2)
    pl = R.generic_planes(8, 3)
    pl[5] = [0.0, 0.0, 1.0, -pts[n - 1, 2]]                                       # the last row, alone in its tile, counts
    want = check_score(vcp_ctx, pts, pl, 0.125)
    assert want.min() > 1000
    last = np.zeros(n, np.uint8)
    last[n - 1] = 1
    last[shape["grid"] * shape["tile"]] = 1                                       # the first row of workgroup 0's second tile
    assert check_score(vcp_ctx, pts, pl, 0.0, last)[5] >= 1


# ---- the score: masks and strides -----------------------------------------------------------------------------------------------
def test_score_masks(vcp_ctx, shape):
    n = 2 * shape["tile"] + 77
    pts, pl = R.lattice_rows(n, 4), R.generic_planes(70, 5)
    full = check_score(vcp_ctx, pts, pl, 0.25)
    rnd = (np.random.default_rng(6).random(n) < 0.4).astype(np.uint8)
    part = check_score(vcp_ctx, pts, pl, 0.25, rnd)
    assert (part <= full).all() and 0 < part.sum() < full.sum()
    assert check_score(vcp_ctx, pts, pl, 0.25, np.zeros(n, np.uint8)).sum() == 0
    rnd[rnd != 0] = 200                                                           # any non-zero byte is active
    assert np.array_equal(check_score(vcp_ctx, pts, pl, 0.25, rnd), part)


@pytest.mark.parametrize("ld,col", [(3, 0), (4, 1), (7, 2)])
def test_score_strided_views_are_read_in_place(vcp_ctx, shape, ld, col):
    n = shape["tile"] + 9
    wide = np.full((n, ld), np.nan)
    pts = R.lattice_rows(n, 7)
    wide[:, col:col + 3] = pts
    pl = R.generic_planes(33, 8)
    want = R.score(pts, pl, 0.25)
    view = wide[:, col:col + 3]
    assert PL._host_rows(view)[0] is view or ld == 3                             # no copy: the rows are read at their stride
    assert np.array_equal(PL.plane_score(view, pl, 0.25, ctx=vcp_ctx), want)
    t = dev(wide)[:, col:col + 3]
    rows, _, got_ld = PL._dev_rows(t)
    assert rows.data_ptr() == t.data_ptr() and got_ld == ld
    assert np.array_equal(host(PL.plane_score(t, dev(pl), 0.25, ctx=vcp_ctx)), want)


# ---- the score: numerics ----------------------------------------------------------------------------------------------------------
def test_score_threshold_is_inclusive_to_the_ulp(vcp_ctx):
    """Rows of the 2^-10 lattice at residual exactly +-thr against (0, 0, 1, -0.5), and the same rows moved one ulp of z to
    either side: fl(z - 0.5) is exact for all of them."""
    thr = 3 * 2.0 ** -10
    z0 = np.array([0.5 + thr, 0.5 - thr])
    z = np.concatenate([np.repeat(z0, 20), np.repeat(np.nextafter(z0, [np.inf, -np.inf]), 30),
                        np.repeat(np.nextafter(z0, 0.5), 40)])
    rng = np.random.default_rng(9)
    pts = np.column_stack([rng.integers(-999, 999, (len(z), 2)) * 2.0 ** -10, z])
    pl = np.array([[0.0, 0.0, 1.0, -0.5], [0.0, 0.0, -1.0, 0.5]])
    r = R.residual(pts, pl[0])
    assert (np.abs(r[:40]) == thr).all() and (np.abs(r[40:100]) > thr).all() and (np.abs(r[100:]) < thr).all()
    assert check_score(vcp_ctx, pts, pl, thr).tolist() == [120, 120]
    assert check_score(vcp_ctx, pts, pl, np.nextafter(thr, 0)).tolist() == [80, 80]
    # a coarse lattice: rows in quarters, normals in halves, offsets in quarters, thr = 0.75: every product and sum is exact
    # and thousands of residuals fall on +-thr exactly
    rng = np.random.default_rng(10)
    pts = rng.integers(-16, 16, (3000, 3)) / 4.0
    lp = np.column_stack([rng.integers(-2, 3, (40, 3)) / 2.0, rng.integers(-8, 9, 40) / 4.0])
    on = sum(int((np.abs(R.residual(pts, p)) == 0.75).sum()) for p in lp)
    assert on > 1000
    at = check_score(vcp_ctx, pts, lp, 0.75)
    below = check_score(vcp_ctx, pts, lp, np.nextafter(0.75, 0))
    assert int((at - below).sum()) == on
    check_score(vcp_ctx, R.lattice_rows(3000, 10), R.lattice_planes(40, 11), 0.25)


def test_score_zero_and_infinite_threshold_and_special_rows(vcp_ctx, shape):
    n = shape["tile"] + 130
    pts = R.lattice_rows(n, 12)
    pl = np.concatenate([R.lattice_planes(20, 13), R.generic_planes(20, 14)])
    pl[7] = [np.nan, 0.0, 1.0, 0.0]                                               # NaN planes among the hypotheses
    pl[8] = [0.0, 0.0, 1.0, np.nan]
    pl[9] = np.nan
    pl[10] = [0.0, 0.0, np.inf, 0.0]
    pts[5] = np.nan
    pts[6, 0] = np.nan
    pts[7, 1] = np.inf
    pts[8, 2] = -np.inf
    pts[9] = [np.inf, -np.inf, 0.0]
    pts[10] = 1e308                                                               # the sums overflow
    pts[11] = 5e-324
    pl[0] = [0.0, 0.0, 1.0, -pts[20, 2]]                                          # row 20 at residual exactly 0
    zero = check_score(vcp_ctx, pts, pl, 0.0)
    assert zero[0] >= 1 and zero[7:10].sum() == 0
    inf = check_score(vcp_ctx, pts, pl, np.inf)
    assert inf[9] == 0 and inf[0] < n and inf.max() >= n - 7                      # every finite residual, and +-inf, but no NaN
    act = (np.arange(n) % 3 != 0).astype(np.uint8)
    check_score(vcp_ctx, pts, pl, np.inf, act)


def test_score_of_a_cloud_far_from_the_origin(vcp_ctx):
    pts = R.lattice_rows(4000, 15) + 1e8
    pl = R.generic_planes(64, 16)
    pl[:, 3] = -(pl[:, :3] @ np.array([1e8, 1e8, 1e8])) + np.linspace(-2, 2, 64)  # through the cloud
    assert check_score(vcp_ctx, pts, pl, 0.05).sum() > 0


# ---- the plane of a triple --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H", [1, 64, 65, 257])
def test_from_triples(vcp_ctx, H):
    n = 500
    rng = np.random.default_rng([17, H])
    pts = rng.normal(size=(n, 3)) * 3.0
    s = 2.0 ** -10
    pts[:3] = np.array([[k * 3 * s, k * 5 * s, k * 7 * s] for k in (1, 2, 5)]) + 0.25   # collinear on the lattice
    pts[3] = [np.nan, 1.0, 2.0]
    pts[4:7] = [[0, 0, 0], [1e200, 0, 0], [0, 1e200, 0]]
    pts[7:10] = [[0, 0, 0], [1e-200, 0, 0], [0, 1e-200, 0]]
    tri = np.array([rng.choice(np.arange(10, n), 3, replace=False) for _ in range(H)], np.int32)   # three distinct rows
    special = [[0, 1, 2], [20, 20, 31], [20, 31, 20], [20, 31, n], [-1, 20, 31], [20, 3, 31], [4, 5, 6], [7, 8, 9],
               [2 ** 31 - 1, 20, 31], [-2 ** 31, 20, 31]]
    k = min(H, len(special))
    tri[H - k:] = special[:k]
    want_pl, want_ok = R.from_triples(pts, tri)
    if H >= len(special):
        assert want_ok[H - k:].sum() == 0 and want_ok[:H - k].all()
    got_pl, got_ok = PL.planes_from_triples(pts, tri, ctx=vcp_ctx)
    assert np.array_equal(got_ok, want_ok) and R.same(got_pl, want_pl)
    assert (R.bits(got_pl[got_ok == 0]) == NAN_BITS).all()
    wide = torch.full((n, 5), float("nan"), dtype=torch.float64, device="cuda")
    wide[:, 1:4] = dev(pts)
    d_pl, d_ok = PL.planes_from_triples(wide[:, 1:4], dev(tri), ctx=vcp_ctx)       # ld 5, in place
    assert np.array_equal(host(d_ok), want_ok) and R.same(host(d_pl), want_pl)
    # valid may be NULL
    out = torch.zeros((H, 4), dtype=torch.float64, device="cuda")
    d_pts, d_tri = dev(pts), dev(tri)
    assert PL._L().vcp_planes_from_triples_dev(vcp_ctx._h, ptr(d_pts), 3, n, ptr(d_tri), H, ptr(out), None) == 0
    assert R.same(host(out), want_pl)


# ---- label -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("masked", [False, True])
def test_label_in_out(vcp_ctx, shape, masked):
    n = 3 * shape["tile"] + 5
    pts = R.lattice_rows(n, 18)
    plane = R.generic_planes(1, 19)[0]
    labels0 = np.random.default_rng(20).integers(-9, -1, n).astype(np.int32)       # sentinels: no row holds the id
    active0 = (np.random.default_rng(21).random(n) < 0.6).astype(np.uint8) * 3 if masked else None
    want_lab, want_act, want_k = R.label(pts, plane, 0.5, 42, labels0, active0)
    assert 0 < want_k < n
    d_lab, d_act = dev(labels0), (dev(active0) if masked else None)
    k = PL.plane_label(dev(pts), plane, 0.5, 42, d_lab, d_act, ctx=vcp_ctx)
    assert k == want_k and np.array_equal(host(d_lab), want_lab)
    assert (host(d_lab) == 42).sum() == k and np.array_equal(host(d_lab)[want_lab != 42], labels0[want_lab != 42])
    if masked:
        assert np.array_equal(host(d_act), want_act)                              # cleared where labelled, untouched elsewhere
        assert PL.plane_label(dev(pts), plane, 0.5, 43, d_lab, d_act, ctx=vcp_ctx) == 0   # they have left the active set
        assert np.array_equal(host(d_lab), want_lab)
    assert PL.plane_label(dev(pts), [np.nan, 0, 0, 0], np.inf, 44, d_lab, d_act, ctx=vcp_ctx) == 0


# ---- the extraction -----------------------------------------------------------------------------------------------------------------
def as_host(fit, max_planes):
    """A Planes (trimmed to n_planes) as the dict of the restatement (padded to max_planes)."""
    planes, counts, hyp = np.full((max_planes, 4), np.nan), np.zeros(max_planes, np.int64), np.zeros(max_planes, np.int64)
    h = lambda a: host(a) if torch.is_tensor(a) else a
    planes[:fit.n_planes], counts[:fit.n_planes], hyp[:fit.n_planes] = h(fit.planes), h(fit.counts), h(fit.hyp_counts)
    return dict(labels=h(fit.labels), planes=planes, counts=counts, hyp_counts=hyp, n_planes=fit.n_planes)


def extract(ctx, pts, on_device, active=None, **call):
    call = dict(call)
    mp = call["max_planes"]
    fit = PL.extract_planes(dev(pts) if on_device else pts, call.pop("thr"), hypotheses=call.pop("H"),
                            active=None if active is None else (dev(active) if on_device else active), ctx=ctx, **call)
    return as_host(fit, mp)


@pytest.mark.parametrize("k", range(5))
@pytest.mark.parametrize("variant", ["refit", "no_refit", "masked"])
def test_ransac_scenes(vcp_ctx, k, variant):
    refit, masked = variant != "no_refit", variant == "masked"
    pts, truth, normals, want = R.scene_fit(k, refit=refit, masked=masked)
    active = R.scene_mask(k) if masked else None
    got = extract(vcp_ctx, pts, True, active, refit=refit, **R.scene_call(k))
    assert R.differs(got, want) is None, (R.differs(got, want), got["counts"], want["counts"])
    assert got["n_planes"] == 3 and got["labels"].dtype == np.int32
    if masked:
        assert (got["labels"][active == 0] == 0).all()
    if k == 0:                                                                    # the host form agrees with the _dev form
        got_h = extract(vcp_ctx, pts, False, active, refit=refit, **R.scene_call(k))
        assert R.differs(got_h, want) is None, R.differs(got_h, want)
    if variant == "refit" and k == 1:                                             # a strided view of a wider resident tensor
        wide = torch.zeros((len(pts), 6), dtype=torch.float64, device="cuda")
        wide[:, 2:5] = dev(pts)
        c = R.scene_call(k)
        fit = PL.extract_planes(wide[:, 2:5], c["thr"], c["H"], c["max_planes"], c["min_inliers"], c["seed"], ctx=vcp_ctx)
        assert R.differs(as_host(fit, c["max_planes"]), want) is None
        keep, idx = PL.remove_planes(fit)
        assert keep.is_cuda and int(keep.sum()) == len(idx) == int((want["labels"] == 0).sum())


def test_ransac_stops(vcp_ctx):
    pts, _, _, want = R.scene_fit(0)
    call = R.scene_call(0)
    none = extract(vcp_ctx, pts, True, **dict(call, min_inliers=18001))            # above every count
    assert none["n_planes"] == 0 and (none["labels"] == 0).all() and (R.bits(none["planes"]) == NAN_BITS).all()
    assert R.differs(none, R.ransac(pts, **dict(call, min_inliers=18001))) is None
    zero = extract(vcp_ctx, pts, True, **dict(call, max_planes=0))
    assert zero["n_planes"] == 0 and (zero["labels"] == 0).all() and zero["planes"].shape == (0, 4)
    one = extract(vcp_ctx, pts, True, **dict(call, max_planes=1))
    assert one["n_planes"] == 1 and R.same(one["planes"][0], want["planes"][0]) and one["counts"][0] == want["counts"][0]
    assert np.array_equal(one["labels"], np.where(want["labels"] == 1, 1, 0))
    for on_device in (True, False):
        few = np.zeros(len(pts), np.uint8)
        few[[3, 4000]] = 1                                                        # m < 3
        assert extract(vcp_ctx, pts, on_device, few, **call)["n_planes"] == 0
        assert extract(vcp_ctx, pts[:2], on_device, **dict(call, min_inliers=0))["n_planes"] == 0
        assert extract(vcp_ctx, pts[:0], on_device, **call)["n_planes"] == 0      # n == 0


@pytest.mark.parametrize("refit", [False, True])
def test_ransac_tie_goes_to_the_lowest_hypothesis(vcp_ctx, refit):
    """A cloud in one exact lattice plane: every valid hypothesis counts every row."""
    s = 2.0 ** -10
    rng = np.random.default_rng(22)
    flat = np.column_stack([rng.integers(-500, 500, (3000, 2)) * s, np.full(3000, 0.25)])
    flat[:2400, 1] = flat[0, 1]                                                   # four rows in five on one line of the plane:
    flat[:2400, 0] = np.arange(2400) * s                                          # about half the hypotheses are invalid
    flat = flat[rng.permutation(3000)]
    want = R.ransac(flat, 0.0, 64, 3, seed=6, refit=refit)
    pl, ok = R.from_triples(flat, R.sample(6, 0, 64, np.arange(3000)))
    first = int(np.nonzero(ok)[0][0])
    assert want["n_planes"] == 1 and want["counts"][0] == 3000 and want["winners"] == [first] and 0 < first and 8 < ok.sum() < 56
    got = extract(vcp_ctx, flat, True, thr=0.0, H=64, max_planes=3, seed=6, refit=refit)
    assert R.differs(got, want) is None, R.differs(got, want)
    if not refit:
        assert R.same(got["planes"][0], pl[want["winners"][0]])


def test_timing_phases(vcp_ctx):
    pts, _, _, _ = R.scene_fit(0)
    vcp_ctx.timing_enable(True)
    try:
        extract(vcp_ctx, pts, True, **R.scene_call(0))
        phases = vcp_ctx.timing()
    finally:
        vcp_ctx.timing_enable(False)
    names = [p for p, _ in phases]
    assert set(names) == {"planes_sample", "planes_score", "planes_refit", "planes_label"}, names
    assert names.count("planes_label") == 3 and names.count("planes_sample") == 4 and all(ms >= 0 for _, ms in phases)


# ---- determinism --------------------------------------------------------------------------------------------------------------------
def test_two_calls_and_a_call_after_dbscan_give_identical_bits(vcp_ctx):
    pts, _, _, want = R.scene_fit(2)
    call = R.scene_call(2)
    a = extract(vcp_ctx, pts, True, **call)
    b = extract(vcp_ctx, pts, True, **call)
    vcp_ctx.dbscan(np.ascontiguousarray(pts[:6000, :2]), 0.05, 5)
    c = extract(vcp_ctx, pts, True, **call)
    for other in (b, c, want):
        assert R.differs(a, other) is None
    pl = R.generic_planes(100, 23)
    s1 = PL.plane_score(pts, pl, 0.012, ctx=vcp_ctx)
    vcp_ctx.dbscan(np.ascontiguousarray(pts[:6000, :2]), 0.05, 5)
    assert np.array_equal(PL.plane_score(pts, pl, 0.012, ctx=vcp_ctx), s1)


# ---- errors -------------------------------------------------------------------------------------------------------------------------
ARG, TOO_LARGE = -1, -5
BIG_N = 0x7FFFFFF0


def test_errors_leave_the_outputs_alone(vcp_ctx):
    L, h = PL._L(), vcp_ctx._h
    n, H = 300, 16
    pts, pl = R.lattice_rows(n, 24), R.generic_planes(H, 25)
    d_pts, d_pl, d_act = dev(pts), dev(pl), dev(np.ones(n, np.uint8))
    d_tri = dev(np.zeros((H, 3), np.int32))
    S = -7
    d_counts = torch.full((H,), S, dtype=torch.int64, device="cuda")
    d_out_pl = torch.full((H, 4), float(S), dtype=torch.float64, device="cuda")
    d_valid = torch.full((H,), 9, dtype=torch.uint8, device="cuda")
    d_lab = torch.full((n,), S, dtype=torch.int32, device="cuda")
    h_counts, h_lab = np.full(H, S, np.int64), np.full(n, S, np.int32)
    r_pl, r_cnt, r_hyp, r_np = np.full((4, 4), float(S)), np.full(4, S, np.int64), np.full(4, S, np.int64), C.c_int32(S)
    k_lab = C.c_int64(S)
    plane = np.array([0.0, 0.0, 1.0, 0.0])
    nan = float("nan")

    def score_dev(ctx=h, p=d_pts, ld=3, n_=n, planes=d_pl, H_=H, thr=0.5, counts=d_counts):
        return L.vcp_plane_score_dev(ctx, ptr(p), ld, n_, ptr(d_act), ptr(planes), H_, thr, ptr(counts))

    def score_host(ctx=h, p=pts, ld=3, n_=n, planes=pl, H_=H, thr=0.5, counts=h_counts):
        return L.vcp_plane_score(ctx, ptr(p), ld, n_, None, ptr(planes), H_, thr, ptr(counts))

    def tri_dev(ctx=h, p=d_pts, ld=3, n_=n, tri=d_tri, H_=H, planes=d_out_pl):
        return L.vcp_planes_from_triples_dev(ctx, ptr(p), ld, n_, ptr(tri), H_, ptr(planes), ptr(d_valid))

    def label_dev(ctx=h, p=d_pts, ld=3, n_=n, pl_=plane, thr=0.5, lab=d_lab, k=k_lab):
        return L.vcp_plane_label_dev(ctx, ptr(p), ld, n_, ptr(d_act), ptr(pl_), thr, 5, ptr(lab), None if k is None else C.byref(k))

    def ransac(dev_form, ctx=h, p=None, ld=3, n_=n, thr=0.5, H_=H, mp=4, mi=0, lab=0, planes=r_pl, cnt=r_cnt, hyp=r_hyp, np_=r_np):
        f = L.vcp_plane_ransac_dev if dev_form else L.vcp_plane_ransac
        p = (d_pts if dev_form else pts) if p is None else p
        lab = (d_lab if dev_form else h_lab) if isinstance(lab, int) else lab
        return f(ctx, ptr(p), ld, n_, None, thr, H_, mp, mi, 1, 1, ptr(lab), ptr(planes), ptr(cnt), ptr(hyp),
                 None if np_ is None else C.byref(np_))

    none = type("Null", (), {"data_ptr": lambda self: None})()                    # ptr(none) is NULL
    for f in (score_dev, score_host):
        for kw, rc in ((dict(ctx=None), ARG), (dict(p=none), ARG), (dict(planes=none), ARG), (dict(counts=none), ARG),
                       (dict(n_=-1), ARG), (dict(ld=2), ARG), (dict(H_=0), ARG), (dict(H_=65537), ARG), (dict(thr=-1e-300), ARG),
                       (dict(thr=nan), ARG), (dict(thr=-np.inf), ARG), (dict(n_=BIG_N), TOO_LARGE)):
            assert f(**kw) == rc, (f.__name__, kw)
    for kw, rc in ((dict(ctx=None), ARG), (dict(p=none), ARG), (dict(tri=none), ARG), (dict(planes=none), ARG), (dict(n_=-1), ARG),
                   (dict(ld=2), ARG), (dict(H_=0), ARG), (dict(H_=65537), ARG), (dict(n_=BIG_N), TOO_LARGE)):
        assert tri_dev(**kw) == rc, kw
    for kw, rc in ((dict(ctx=None), ARG), (dict(p=none), ARG), (dict(pl_=none), ARG), (dict(lab=none), ARG), (dict(k=None), ARG),
                   (dict(n_=-1), ARG), (dict(ld=2), ARG), (dict(thr=nan), ARG), (dict(thr=-1.0), ARG), (dict(n_=BIG_N), TOO_LARGE)):
        assert label_dev(**kw) == rc, kw
    for dev_form in (True, False):
        for kw, rc in ((dict(ctx=None), ARG), (dict(p=none), ARG), (dict(lab=none), ARG), (dict(planes=none), ARG),
                       (dict(cnt=none), ARG), (dict(hyp=none), ARG), (dict(np_=None), ARG), (dict(n_=-1), ARG), (dict(ld=2), ARG),
                       (dict(H_=0), ARG), (dict(H_=65537), ARG), (dict(mp=-1), ARG), (dict(mp=65), ARG), (dict(mi=-1), ARG),
                       (dict(thr=nan), ARG), (dict(thr=-0.5), ARG), (dict(n_=BIG_N), TOO_LARGE)):
            assert ransac(dev_form, **kw) == rc, (dev_form, kw)
    assert L.vcp_plane_score_shape(None, ptr(np.zeros(3, np.int32))) == ARG and L.vcp_plane_score_shape(h, None) == ARG
    # nothing was written
    torch.cuda.synchronize()
    assert (host(d_counts) == S).all() and (host(d_out_pl) == S).all() and (host(d_valid) == 9).all() and (host(d_lab) == S).all()
    assert (h_counts == S).all() and (h_lab == S).all() and (r_pl == S).all() and (r_cnt == S).all() and (r_hyp == S).all()
    assert r_np.value == S and k_lab.value == S
    # ... and the same calls without the fault run
    assert score_dev() == 0 and np.array_equal(host(d_counts), R.score(pts, pl, 0.5))
    assert score_dev(thr=np.inf) == 0 and ransac(True, mp=0, planes=none, cnt=none, hyp=none) == 0 and r_np.value == 0
    assert (host(d_lab) == 0).all()                                                # max_planes == 0: every label 0
