"""vcp_point_features on the MI355X (include/vcp_features.h) against the numpy restatement tests/point_features_ref.py, for
equality: every double output as bits, count and valid as integers.  Host and _dev forms, dim 2 and 3.  The sizes come from
vcp_point_features_shape: the rows per workgroup, the grid's cap and the k classes are where the kernel takes another
path."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import point_features_ref as R
from vtkcloudpoint_amd import features as FT
from vtkcloudpoint_amd import kdist as KD

pytestmark = pytest.mark.gpu

NAN_BITS = 0x7FF8000000000000
KS = (1, 2, 3, 8, 9, 16, 17, 32, 33, 64)                  # both sides of every k class, and of the register / re-gather fork
FORMS = ("host", "dev")
VP = {2: (0.5, -0.25), 3: (0.5, -0.25, 2.0)}


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()                       # a copy: the shared inputs are read-only


def host(t):
    return t.cpu().numpy()


@pytest.fixture(scope="module")
def shape(vcp_ctx):
    rows, grid, classes = FT.point_features_shape(vcp_ctx)
    assert 64 <= rows <= 1024 and rows % 64 == 0 and 1 <= grid <= 8 * 256 and classes == (8, 16, 32, 64)
    return dict(rows=rows, grid=grid)


def run(ctx, form, pts, nbr, vp):
    """point_features with the caller's neighbour rows through one form; the outputs as a dict of numpy arrays."""
    if form == "dev":
        pts, nbr = (pts if torch.is_tensor(pts) else dev(pts)), dev(nbr)
    f = FT.point_features(pts, neighbours=nbr, viewpoint=vp, ctx=ctx)
    assert (torch.is_tensor(f.normal) and f.normal.is_cuda) == (form == "dev")
    return R.as_dict(f)


def check(ctx, pts, nbr, vp, want=None, forms=FORMS):
    want = R.features(pts, nbr, vp) if want is None else want
    for form in forms:
        d = R.differs(run(ctx, form, pts, nbr, vp), want)
        assert d is None, (form, d)
    return want


@functools.lru_cache(maxsize=None)
def _case(n, k, D, seed=3):
    pts, nbr = R.generic_rows(n, D, seed + n + k), R.mixed_nbr(n, k, seed)
    return pts, nbr, R.features(pts, nbr, VP[D])


# ---- sizes ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [2, 3])
@pytest.mark.parametrize("n_case", ("0", "1", "63", "64", "65", "rows-1", "rows", "rows+1"))
def test_row_counts(vcp_ctx, shape, n_case, D):
    n = eval(n_case, dict(shape))
    for k in (5, 16, 17):                                                        # the register road twice, the re-gather road
        pts, nbr, want = _case(n, k, D)
        check(vcp_ctx, pts, nbr, VP[D], want)
        assert n < 63 or (0 < want["valid"].sum() < n and want["count"].min() == 0 and want["count"].max() > 0)


@pytest.mark.parametrize("D", [2, 3])
@pytest.mark.parametrize("k", KS)
def test_every_k_class_from_both_sides(vcp_ctx, shape, k, D):
    n = shape["rows"] + 72                                                       # two workgroups, the second one partly filled
    pts, nbr, want = _case(n, k, D)
    check(vcp_ctx, pts, nbr, VP[D], want)
    assert want["count"].max() == k


@pytest.mark.parametrize("D,k,form", [(3, 3, "dev"), (2, 17, "dev"), (3, 9, "host")])
def test_one_row_past_the_largest_grids_single_trip(vcp_ctx, shape, D, k, form):
    """n = rows * grid + 1: workgroup 0 takes a second trip for one row.  The cloud repeats with a period
    (point_features_ref.tiled_case), so the restatement is needed for one period only; 300 rows, the last ones among them,
    are restated directly as well."""
    n = shape["rows"] * shape["grid"] + 1
    pts, nbr, base, local = R.tiled_case(n, k, D, 21)
    want = R.want_tiled(base, local, n, VP[D])
    sample = np.r_[np.random.default_rng(22).integers(0, n, 280), np.arange(n - 20, n)]
    direct = R.features(pts, nbr, VP[D], rows=sample)
    assert R.differs(direct, {key: want[key][sample] for key in R.KEYS}) is None
    check(vcp_ctx, pts, nbr, VP[D], want, forms=(form,))


# ---- slots, strides, magnitudes -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [2, 3])
def test_rows_without_a_member(vcp_ctx, D):
    n, k = 70, 4
    want = check(vcp_ctx, R.generic_rows(n, D, 30), np.full((n, k), -1, np.int32), VP[D])
    for key in ("normal", "eval", "variation", "mean_dist"):
        assert (R.bits(want[key]) == NAN_BITS).all()
    assert not want["count"].any() and not want["valid"].any()


@pytest.mark.parametrize("D", [2, 3])
def test_strided_views_are_read_in_place_and_the_pad_is_never_read(vcp_ctx, shape, D):
    n, k = shape["rows"] + 9, 12
    pts, nbr, want = _case(n, k, D)
    for ld, col in ((D, 0), (D + 2, 1)):
        wide = np.full((n, ld), np.nan)                                          # a NaN that is read poisons the row's outputs
        wide[:, col:col + D] = pts
        view = wide[:, col:col + D]
        assert R.differs(run(vcp_ctx, "host", view, nbr, VP[D]), want) is None
        t = dev(wide)[:, col:col + D]
        assert t.stride(0) == ld and R.differs(run(vcp_ctx, "dev", t, nbr, VP[D]), want) is None
    assert want["valid"].sum() > n // 2


@pytest.mark.parametrize("D", [2, 3])
def test_a_cloud_far_from_the_origin_keeps_its_digits(vcp_ctx, D):
    n, k = 150, 16
    near, far = R.generic_rows(n, D, 31), R.generic_rows(n, D, 31, offset=1e8)
    nbr = R.mixed_nbr(n, k, 32)
    wf, wn = check(vcp_ctx, far, nbr, VP[D]), R.features(near, nbr, VP[D])
    ok = (wn["valid"] != 0) & (wn["eval"][:, 0] > 0)
    # the centred sums: the largest eigenvalue agrees with the near cloud's to the digits an offset of 1e8 leaves
    assert np.allclose(wf["eval"][ok, 0], wn["eval"][ok, 0], rtol=1e-4, atol=1e-12) and ok.sum() > n // 2


@pytest.mark.parametrize("D", [2, 3])
def test_non_finite_rows_and_neighbours(vcp_ctx, D):
    n, k = 140, 9
    pts = np.array(R.generic_rows(n, D, 33))
    nbr = R.mixed_nbr(n, k, 34)
    pts[7] = np.nan
    pts[11, 1] = np.inf
    pts[20, 0] = -np.inf
    nbr[40, 2], nbr[41, 0], nbr[42, k - 1] = 7, 11, 20                            # rows that are sure to meet them
    want = check(vcp_ctx, pts, nbr, VP[D])
    for i in (40, 41, 42):
        assert want["valid"][i] == 0 and (R.bits(want["eval"][i]) == NAN_BITS).all()
    # the distance to a NaN row is NaN, to an infinite one +inf; a NaN row is at a NaN distance from everything
    assert R.bits(want["mean_dist"])[40] == NAN_BITS and want["mean_dist"][41] == np.inf and want["mean_dist"][42] == np.inf
    assert R.bits(want["mean_dist"])[7] == NAN_BITS and want["valid"].sum() > n // 2


@pytest.mark.parametrize("D", [2, 3])
def test_viewpoints(vcp_ctx, D):
    n, k = 200, 10
    pts, nbr, _ = _case(n, k, D)
    free = check(vcp_ctx, pts, nbr, None)
    flipped = 0
    for vp in (VP[D], tuple(-v for v in VP[D]), (1e12, -1e12, 1e12)[:D], (1e300, 1e300, -1e300)[:D], tuple(pts[37])):
        w = check(vcp_ctx, pts, nbr, vp)
        assert R.differs(w, free, [key for key in R.KEYS if key != "normal"]) is None
        same_or_negated = (R.bits(w["normal"]) == R.bits(free["normal"])).all(1) | (R.bits(w["normal"]) == R.bits(-free["normal"])).all(1)
        assert same_or_negated.all()
        flipped += int((R.bits(w["normal"]) != R.bits(free["normal"])).any(1).sum())
    assert flipped > n // 2
    w = R.features(pts, nbr, tuple(pts[37]))
    assert R.same(w["normal"][37], free["normal"][37])                           # v = 0: s == 0, the normal stays


# ---- NULL outputs, errors, repeatability -------------------------------------------------------------------------------------------
OUT = ("normal", "eval", "variation", "mean_dist", "count", "valid")


def _raw(ctx, form, pts, ld, D, n, nbr, k, vp, outs, h=True):
    """The C entry point itself: pts / nbr / outs are numpy arrays (host form) or tensors (dev form) or None."""
    p = lambda a: None if a is None else (a.ctypes.data if isinstance(a, np.ndarray) else a.data_ptr())
    fn = getattr(FT._L(), "vcp_point_features" if form == "host" else "vcp_point_features_dev")
    vpa = None if vp is None else np.ascontiguousarray(vp, np.float64)
    return fn(ctx._h if h else None, p(pts), C.c_int64(ld), D, C.c_int64(n), p(nbr), k, p(vpa), *[p(outs.get(key)) for key in OUT])


def _fresh(form, n, D):
    o = dict(normal=np.full((n, D), -7.0), eval=np.full((n, D), -7.0), variation=np.full(n, -7.0), mean_dist=np.full(n, -7.0),
             count=np.full(n, -7, np.int32), valid=np.full(n, 9, np.uint8))
    return {key: dev(v) for key, v in o.items()} if form == "dev" else o


def _np(o):
    return {key: (host(v) if torch.is_tensor(v) else v) for key, v in o.items()}


@pytest.mark.parametrize("D", [2, 3])
@pytest.mark.parametrize("form", FORMS)
def test_each_output_may_be_null(vcp_ctx, form, D):
    n, k = 90, 7
    pts, nbr, want = _case(n, k, D)
    a_pts, a_nbr = (dev(pts), dev(nbr)) if form == "dev" else (pts, nbr)
    if form == "dev":
        torch.cuda.synchronize()
    for skip in OUT + ("all",):
        outs = _fresh(form, n, D)
        given = {key: v for key, v in outs.items() if key != skip and skip != "all"}
        assert _raw(vcp_ctx, form, a_pts, D, D, n, a_nbr, k, VP[D], given) == 0
        got = _np(outs)
        for key in OUT:
            if key in given:
                assert R.differs(got, want, [key]) is None, (skip, key)
            else:
                assert (got[key] == (9 if key == "valid" else -7)).all(), (skip, key)   # not handed over: not touched


@pytest.mark.parametrize("form", FORMS)
def test_every_error_code_leaves_the_outputs_alone(vcp_ctx, form):
    n, k, D = 50, 6, 3
    pts, nbr, _ = _case(n, k, D)
    a_pts, a_nbr = (dev(pts), dev(nbr)) if form == "dev" else (pts, nbr)
    outs = _fresh(form, n, D)
    if form == "dev":
        torch.cuda.synchronize()
    ARG, UNSUPPORTED, TOO_LARGE = -1, -8, -5
    cases = [
        (ARG, dict(h=False)), (ARG, dict(n=-1)), (ARG, dict(D=1)), (ARG, dict(D=4)), (ARG, dict(D=0)), (ARG, dict(ld=2)),
        (ARG, dict(D=2, ld=1)), (ARG, dict(k=0)), (ARG, dict(k=-3)), (ARG, dict(pts=None)), (ARG, dict(nbr=None)),
        (UNSUPPORTED, dict(k=65)), (UNSUPPORTED, dict(k=1 << 20)), (TOO_LARGE, dict(n=0x7FFFFFF0)), (TOO_LARGE, dict(n=1 << 40)),
        (ARG, dict(k=65, nbr=None)),                                              # the argument errors come first
    ]
    for code, change in cases:
        a = dict(pts=a_pts, ld=D, D=D, n=n, nbr=a_nbr, k=k, h=True)
        a.update(change)
        assert _raw(vcp_ctx, form, a["pts"], a["ld"], a["D"], a["n"], a["nbr"], a["k"], VP[3], outs, a["h"]) == code, change
    for key, v in _np(outs).items():
        assert (v == (9 if key == "valid" else -7)).all(), key
    # n == 0 is no error, with or without pointers
    assert _raw(vcp_ctx, form, None, D, D, 0, None, k, None, outs) == 0 and _raw(vcp_ctx, form, a_pts, D, D, 0, a_nbr, k, VP[3], outs) == 0
    with pytest.raises(Exception) as e:
        FT.point_features(pts, neighbours=np.zeros((n, 65), np.int32), ctx=vcp_ctx)
    assert getattr(e.value, "code", None) == UNSUPPORTED


@pytest.mark.parametrize("form", FORMS)
def test_two_calls_give_identical_bits_and_the_phase_is_named(vcp_ctx, form):
    pts, nbr, want = _case(400, 33, 3)
    vcp_ctx.timing_enable(True)
    try:
        a = run(vcp_ctx, form, pts, nbr, VP[3])
        assert [name for name, _ in vcp_ctx.timing()] == ["features_rows"]
        vcp_ctx.kdist(pts, 4, 2)                                                  # another entry point in between
        b = run(vcp_ctx, form, pts, nbr, VP[3])
    finally:
        vcp_ctx.timing_enable(False)
    assert R.differs(a, b) is None and R.differs(a, want) is None


# ---- end to end -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
def test_scene_rows_end_to_end(vcp_ctx, form):
    """5000 rows of the scene through point_features(k = 16): the neighbour rows are k_nearest's, every output is the
    restatement's on those rows, and sor_keep and centre_votes give the restatement's bits."""
    pts, kind, _ = R.scene_subset(R.SCENE_SEEDS[0])
    _, knn = KD.k_nearest(pts, 16, "L2_3D", ctx=vcp_ctx)
    f = FT.point_features(dev(pts) if form == "dev" else pts, k=16, ctx=vcp_ctx)
    assert f.knn.dtype == (torch.int32 if form == "dev" else np.int32)
    assert np.array_equal(host(f.knn) if form == "dev" else f.knn, knn) and (knn[:, 0] == np.arange(len(pts))).all()
    want = R.features(pts, knn, (0.0, 0.0, 0.0))
    assert R.differs(R.as_dict(f), want) is None and want["valid"].all()
    wk, wmed, wmad = R.sor_keep(want["mean_dist"], 6.0)
    keep, med, mad = FT.sor_keep(f.mean_dist, 6.0, ctx=vcp_ctx)
    assert (med, mad) == (wmed, wmad) and np.array_equal(host(keep) if form == "dev" else keep, wk) and 0 < (~wk).sum() < 2500
    other = FT.sor_keep(want["mean_dist"] if form == "dev" else dev(want["mean_dist"]), 6.0, floor=0.05, ctx=vcp_ctx)   # the other kind of array
    wo = R.sor_keep(want["mean_dist"], 6.0, floor=0.05)
    assert (other[1], other[2]) == (wo[1], wo[2]) and np.array_equal(other[0] if form == "dev" else host(other[0]), wo[0])
    votes = FT.centre_votes(dev(pts) if form == "dev" else pts, f, R.R_SPHERE)
    assert R.same(R.canon(host(votes) if form == "dev" else votes), R.centre_votes(pts, want["normal"], R.R_SPHERE, want["valid"]))
