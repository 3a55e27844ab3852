"""Anisotropic ICP without a GPU: the three entry points through every layer of the binding, the host step
(vcp_selftest_horn_aniso, compiled from the source the device runs) against its restatement bit for bit, its two exact
invariances, its scales against the exact rational value, and the behaviour scene held to its conditions by the numpy
reference alone (tests/icp_aniso_ref.py) -- the device is held to the same conditions on the same seeds in
tests/test_icp_aniso_gpu.py."""
import ctypes as C
import functools
import inspect
import math
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import icp_aniso_ref as A
import icp_gated_ref as G
import icp_sim_ref as S
import icp_sums_ref as R
from test_abi import _csharp_imports, _declared, _header_prototypes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("vcp_icp_sums_aniso", "vcp_selftest_horn_aniso", "vcp_icp_aniso")
INF, NAN = math.inf, math.nan
LO, HI = (1e-300, 1e-300), (1e300, 1e300)          # bounds that never bind
ONE = (1.0, 1.0)


def _N():
    from vtkcloudpoint_amd import _native
    return _native


def test_abi_has_the_anisotropic_entry_points():
    N = _N()
    lib = N.lib()
    decl = _declared()
    protos = _header_prototypes()
    imports = {name: classes for _, name, classes in _csharp_imports()}
    for name in NAMES:
        assert name in decl and hasattr(lib, name) and name in N.SYMBOLS, name
        assert imports.get(name) == protos[name], name       # the DllImport passes the header's parameters
    assert len(protos["vcp_icp_sums_aniso"]) == 12 and len(protos["vcp_selftest_horn_aniso"]) == 12
    assert len(protos["vcp_icp_aniso"]) == 26
    assert protos["vcp_icp_sums_aniso"] == protos["vcp_icp_sums_sim"]
    sim = protos["vcp_icp_sim"]
    assert protos["vcp_icp_aniso"] == sim[:8] + ["ptr"] + sim[8:]      # init_scale behind init_T, nothing else moves
    assert lib.vcp_version() == 1
    for obj, method, first in ((N.Context, "icp_sums_aniso", ["self", "model", "data", "gate", "A", "T"]),
                               (N.Context, "icp_aniso", ["self", "source", "target", "gates", "ratio_range", "poses",
                                                         "init_T", "init_scale"]),
                               (N, "selftest_horn_aniso", ["sums", "n", "R", "s", "lo", "hi", "V"])):
        params = list(inspect.signature(getattr(obj, method)).parameters)
        assert params[:len(first)] == first, method
    from vtkcloudpoint_amd import icp
    sig = inspect.signature(icp.anisotropic_icp)
    assert list(sig.parameters)[:4] == ["centers", "truths", "scale0", "ratio"]
    assert sig.parameters["scale0"].default is None and sig.parameters["ratio"].default == (0.9, 1.1)
    assert list(inspect.signature(icp.bbox_scale_xy).parameters) == ["centers", "truths"]
    with open(os.path.join(ROOT, "vtkcloudpoint_amd", "host", "csharp", "MainForm.Gpu.cs")) as f:
        src = f.read()
    assert re.search(r"void\s+ICPAnisotropic\s*\(", src) and "VcpNative.vcp_icp_aniso(" in src
    body = src[src.index("void ICPAnisotropic"):]
    body = body[:body.index("\n        }\n")]
    assert "p.tmp_X = p.X * scale[0]" in body and "p.tmp_Y = p.Y * scale[1]" in body
    assert re.search(r"scale\[0\] = fitted\[2 \* best\];\s*scale\[1\] = fitted\[2 \* best \+ 1\];", body)


def test_bbox_scale_xy_is_the_reference_rule():
    from vtkcloudpoint_amd.icp import bbox_scale_xy
    rng = np.random.default_rng(3)
    tgt = rng.uniform(-5.0, 9.0, (50, 3))
    src = rng.uniform(-2.0, 3.0, (70, 3))
    sx, sy = bbox_scale_xy(src, tgt)
    assert sx == (tgt[:, 0].max() - tgt[:, 0].min()) / (src[:, 0].max() - src[:, 0].min())
    assert sy == (tgt[:, 1].max() - tgt[:, 1].min()) / (src[:, 1].max() - src[:, 1].min())
    sc = A.aniso_scene(40, 32, 12, 1, (0.0, 0.0))
    on = sc["centers"][sc["is_true"]] @ G.rz(G.ANGLE).T          # the true centroids alone, turned into the truths' axes
    ex, ey = bbox_scale_xy(on, sc["truths"])
    print("bounding boxes on the true centroids, axes aligned:", ex, ey, "true", A.K_XY)
    assert ex != ey


# ---- the step against its restatement --------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _sums(path, nm, nd, family, pose="generic"):
    Ssum, n, rot = A.case_sums(path, nm, nd, family, pose)
    Ssum.setflags(write=False)
    return Ssum, n, tuple(rot)


def _call(sums, n, Rm, s=ONE, lo=LO, hi=HI, V=None):
    return _N().selftest_horn_aniso(sums, n, Rm, s, lo, hi, V)


def _bits(x):
    return np.asarray(x, np.float64).tobytes()


def _same_step(got, want):
    rc, Rn, Tn, sn, det, _ = want
    assert got["rc"] == rc
    if rc == 0:
        return
    assert _bits(got["R_new"]) == _bits(Rn) and _bits(got["T_new"]) == _bits(Tn), (got, want)
    assert _bits(got["s_new"]) == _bits(sn) and got["determined"] == det, (got, want)


@functools.lru_cache(maxsize=None)
def _fitted(nd, offset, k=(2.5, 2.2), angle=0.3, seed=0):
    """(sums [18], n, rotation [9]): nd planar landmarks round `offset` whose model points are R diag(k, 1) d + t plus
    noise, summed in point order.  Both axes are determined."""
    rng = np.random.default_rng([seed, nd])
    d = np.zeros((nd, 3))
    d[:, :2] = rng.uniform(-10.0, 10.0, (nd, 2)) + offset
    Rm = G.rz(angle)
    y = (d * np.array([k[0], k[1], 1.0])) @ Rm.T + np.array([0.7, -1.1, 0.0])
    y[:, :2] += rng.normal(0.0, 0.01, (nd, 2))
    t = np.empty((nd, 18))
    t[:, 0:3], t[:, 3:6] = d, y
    t[:, 6:15] = (d[:, :, None] * y[:, None, :]).reshape(nd, 9)
    t[:, 15] = 0.0
    t[:, 16], t[:, 17] = d[:, 0] * d[:, 0], d[:, 1] * d[:, 1]
    Ssum = np.zeros(18)
    for row in t:
        Ssum = Ssum + row
    Ssum.setflags(write=False)
    return Ssum, nd, tuple(float(x) for x in G.rz(angle + 0.01).reshape(9))


@pytest.mark.parametrize("pose", R.POSES)
@pytest.mark.parametrize("family", R.FAMILIES)
@pytest.mark.parametrize("path,nm,nd", R.SMALL_SHAPES)
def test_step_is_the_restatement(path, nm, nd, family, pose):
    N = _N()
    sums, n, rot = _sums(path, nm, nd, family, pose)
    assert np.isfinite(sums).all()
    s0 = (0.75, 1.5)
    cold = _call(sums, n, rot, s0)
    want = A.step(N, sums, n, rot, s0, LO, HI)
    assert want[0] == 1
    _same_step(cold, want)
    # A_new of the header from what the call returns
    assert _bits(A.pose_matrix(cold["R_new"].tolist(), cold["s_new"].tolist())) == _bits(want[5])
    # a garbage basis is a cold start; the basis it leaves is a warm one, and the step from it is horn's from it
    V = np.zeros(16)
    assert _bits(_call(sums, n, rot, s0, V=V)["R_new"]) == _bits(cold["R_new"])
    Vw = V.copy()
    warm_want = A.step(N, sums, n, rot, s0, LO, HI, Vw)
    warm = _call(sums, n, rot, s0, V=V)
    assert np.array_equal(V, Vw)
    _same_step(warm, warm_want)
    # an axis that is not determined keeps its scale; a determined one is g / D or the bound it met
    sn, det = cold["s_new"].tolist(), cold["determined"]
    for a in range(2):
        if not det >> a & 1:
            assert sn[a] == s0[a]
            continue
        for lo_a, hi_a, what in ((2 * sn[a], 4 * sn[a], "low"), (sn[a] / 4, sn[a] / 2, "high"), (sn[a], sn[a], "free"),
                                 (np.nextafter(sn[a], INF), 3 * sn[a], "low"), (sn[a] / 3, np.nextafter(sn[a], 0.0), "high")):
            lo, hi = list(LO), list(HI)
            lo[a], hi[a] = lo_a, hi_a
            got = _call(sums, n, rot, s0, lo, hi)
            _same_step(got, A.step(N, sums, n, rot, s0, lo, hi))
            assert got["determined"] == det
            assert got["s_new"][a] == {"low": lo_a, "high": hi_a, "free": sn[a]}[what]
            assert got["s_new"][1 - a] == sn[1 - a]


@pytest.mark.parametrize("nd,offset", [(50, 0.0), (1000, 0.0), (1000, 1e3), (333, 1e5)])
def test_step_on_fitted_pairs_recovers_the_scales(nd, offset):
    N = _N()
    sums, n, rot = _fitted(nd, offset)
    got = _call(sums, n, rot, (2.0, 2.0))
    _same_step(got, A.step(N, sums, n, rot, (2.0, 2.0), LO, HI))
    assert got["determined"] == 3
    assert abs(got["s_new"][0] / 2.5 - 1) < 2e-3 and abs(got["s_new"][1] / 2.2 - 1) < 2e-3
    assert np.allclose(got["R_new"].reshape(3, 3), G.rz(0.3), atol=2e-3)
    # both clamps at once
    got = _call(sums, n, rot, (2.0, 2.0), (2.6, 1.0), (3.0, 2.1))
    _same_step(got, A.step(N, sums, n, rot, (2.0, 2.0), (2.6, 1.0), (3.0, 2.1)))
    assert got["s_new"].tolist() == [2.6, 2.1] and got["determined"] == 3


def test_undetermined_axis():
    N = _N()
    # all kept d share an x: D_0 = 4 - 2 * 2 = 0 exactly; y varies with d_1 alone
    d = np.array([[2.0, -1.0, 0.0], [2.0, 0.0, 0.0], [2.0, 1.0, 0.0], [2.0, 4.0, 0.0]])
    y = d * np.array([1.0, 3.0, 1.0]) + np.array([1.0, 0.5, 0.0])
    s = np.zeros(18)
    s[0:3], s[3:6] = d.sum(axis=0), y.sum(axis=0)
    s[6:15] = (d[:, :, None] * y[:, None, :]).sum(axis=0).reshape(9)
    s[16], s[17] = (d[:, 0] ** 2).sum(), (d[:, 1] ** 2).sum()
    eye = np.eye(3).reshape(9)
    got = _call(s, 4, eye, (1.25, 0.5))
    _same_step(got, A.step(N, s, 4, eye, (1.25, 0.5), LO, HI))
    assert got["rc"] == 1 and got["determined"] == 2
    assert got["s_new"].tolist() == [1.25, 3.0]
    assert np.array_equal(got["R_new"], eye) and got["T_new"].tolist() == [0.5, 0.5, 0.0]     # x keeps 1.25: 3 - 2.5
    # coincident points determine neither axis, and the step is the rigid one on the sums scaled by s
    z = np.zeros(18)
    got = _call(z, 5, eye, (0.8, 1.7))
    assert got["rc"] == 1 and got["determined"] == 0 and got["s_new"].tolist() == [0.8, 1.7]
    assert np.array_equal(got["R_new"], eye) and got["T_new"].tolist() == [0.0, 0.0, 0.0]
    # a rotation that has turned the axis round (g <= 0), an infinite or NaN D or g: comparisons with NaN are false
    sums, n, rot = _fitted(1000, 0.0)
    flip = tuple(float(x) for x in (G.rz(0.3) @ np.diag([-1.0, 1.0, 1.0])).reshape(9))
    got = _call(sums, n, flip, (2.0, 2.0))
    assert got["determined"] == 2 and got["s_new"][0] == 2.0
    _same_step(got, A.step(N, sums, n, flip, (2.0, 2.0), LO, HI))
    for k, v, det in ((16, NAN, 2), (17, NAN, 1), (16, INF, 2), (17, INF, 1), (16, 0.0, 2), (17, -1.0, 1)):
        b = np.array(sums)
        b[k] = v
        got = _call(b, n, rot, (2.0, 2.0))
        assert got["rc"] == 1 and got["determined"] == det, (k, v)
        _same_step(got, A.step(N, b, n, rot, (2.0, 2.0), LO, HI))
    bad_rot = list(rot)
    bad_rot[0] = NAN
    got = _call(sums, n, bad_rot, (2.0, 2.0))
    assert got["determined"] == 2 and got["s_new"][0] == 2.0


@pytest.mark.parametrize("k", range(18))
def test_a_nan_in_each_sum(k):
    """Columns 0..14 reach horn's matrix (NaN: the solve fails, nothing but V written); 15 is read by nothing; 16 and 17
    only undetermine their axis."""
    N = _N()
    sums, n, rot = _fitted(1000, 0.0)
    b = np.array(sums)
    b[k] = NAN
    want = A.step(N, b, n, rot, (2.0, 2.0), LO, HI)
    Rn, Tn, sn = np.full(9, 7.0), np.full(3, 7.0), np.full(2, 7.0)
    det = C.c_int32(7)
    held = [np.array(x, np.float64) for x in (rot, (2.0, 2.0), LO, HI)]
    rc = N.lib().vcp_selftest_horn_aniso(N._ptr(b), C.c_int64(n), None, C.c_int(0), *[N._ptr(x) for x in held], N._ptr(Rn),
                                         N._ptr(Tn), N._ptr(sn), C.byref(det))
    assert rc == want[0] == (1 if k >= 15 else 0)
    if rc == 0:
        assert (Rn == 7).all() and (Tn == 7).all() and (sn == 7).all() and det.value == 7
        assert _call(b, n, rot, (2.0, 2.0))["rc"] == 0
    else:
        assert det.value == {15: 3, 16: 2, 17: 1}[k]
        _same_step(dict(rc=rc, R_new=Rn, T_new=Tn, s_new=sn, determined=det.value), want)


def test_every_argument_error():
    N = _N()
    sums, n, rot = _fitted(1000, 0.0)
    sums = np.array(sums)
    V = np.zeros(16)

    def raw(**kw):
        Rn, Tn, sn = np.full(9, 7.0), np.full(3, 7.0), np.full(2, 7.0)
        det = C.c_int32(7)
        a = dict(sums=sums, n=n, V=V, use_v=1, R=np.array(rot), s=np.array([2.0, 2.0]), lo=np.array([0.5, 0.5]),
                 hi=np.array([4.0, 4.0]), Rn=Rn, Tn=Tn, sn=sn, det=C.byref(det))
        a.update(kw)
        a = {k: np.array(v, np.float64) if isinstance(v, (tuple, list)) else v for k, v in a.items()}   # held to the call
        p = {k: N._ptr(v) if isinstance(v, np.ndarray) else v for k, v in a.items()}
        rc = N.lib().vcp_selftest_horn_aniso(p["sums"], C.c_int64(a["n"]), p["V"], C.c_int(a["use_v"]), p["R"], p["s"],
                                             p["lo"], p["hi"], p["Rn"], p["Tn"], p["sn"], p["det"])
        if rc < 0:
            assert (Rn == 7).all() and (Tn == 7).all() and (sn == 7).all() and det.value == 7
        return rc

    assert raw() == 1 and raw(V=None, use_v=0) == 1
    for kw in (dict(sums=None), dict(R=None), dict(s=None), dict(lo=None), dict(hi=None), dict(Rn=None), dict(Tn=None),
               dict(sn=None), dict(det=None), dict(n=0), dict(n=-3), dict(V=None, use_v=1)):
        assert raw(**kw) == -1, kw
    for a in range(2):
        def two(v, other):
            return [v, other] if a == 0 else [other, v]
        for bad in (NAN, 0.0, -1.0):
            assert raw(s=two(bad, 2.0)) == -1 and raw(lo=two(bad, 0.5)) == -1 and raw(hi=two(bad, 4.0)) == -1, (a, bad)
        assert raw(hi=two(INF, 4.0)) == -1 and raw(lo=two(INF, 0.5), hi=two(INF, 4.0)) == -1
        assert raw(lo=two(1.0, 0.5), hi=two(0.999, 4.0)) == -1
        assert raw(lo=two(1.0, 0.5), hi=two(1.0, 4.0)) == 1
    with pytest.raises(N.VcpError):
        N.selftest_horn_aniso(sums, n, rot, (-1.0, 1.0), (0.5, 0.5), (2.0, 2.0))


# ---- the two exact invariances ---------------------------------------------------------------------------------------
INVARIANCE_INPUTS = [("case", f) for f in ("generic", "offset", "planar", "cancel", "lattice")] + [("fitted", 0.0), ("fitted", 1e3)]


def _inv_sums(kind, what):
    if kind == "case":
        return _sums("pairs", 100, 1000, what, "generic")
    return _fitted(1000, what)


@pytest.mark.parametrize("kind,what", INVARIANCE_INPUTS)
@pytest.mark.parametrize("e", (-40, 1, 40, 100))
def test_power_of_two_scaling_of_everything(kind, what, e):
    sums, n, rot = _inv_sums(kind, what)
    f = 2.0 ** e
    scaled = np.array(sums)
    scaled[0:6] *= f
    scaled[6:18] *= f * f
    for s, lo, hi in (((2.0, 2.0), LO, HI), ((0.75, 1.5), (0.7, 1.4), (0.8, 1.6)), ((1.0, 1.0), ONE, ONE)):
        a, b = _call(sums, n, rot, s, lo, hi), _call(scaled, n, rot, s, lo, hi)
        assert a["rc"] == b["rc"] == 1 and a["determined"] == b["determined"]
        assert _bits(a["R_new"]) == _bits(b["R_new"]) and _bits(a["s_new"]) == _bits(b["s_new"])
        assert _bits(a["T_new"] * f) == _bits(b["T_new"])


@pytest.mark.parametrize("kind,what", INVARIANCE_INPUTS)
@pytest.mark.parametrize("e", (-40, -1, 3, 40))
def test_power_of_two_scaling_of_the_data_x_alone(kind, what, e):
    """The data's x times 2^e, with s_0 and its bounds times 2^-e: R_new, T_new, s'_1 and A_new applied to the scaled data
    are bit-identical, s'_0 is exactly 2^-e times what it was.  No isotropic step passes this."""
    sums, n, rot = _inv_sums(kind, what)
    f = 2.0 ** e
    scaled = np.array(sums)
    scaled[0] *= f
    scaled[6:9] *= f
    scaled[16] *= f * f
    seen = 0
    wide_lo, wide_hi = (2.0 ** -200, 2.0 ** -200), (2.0 ** 200, 2.0 ** 200)      # exact under the scaling
    for s, lo, hi in (((2.0, 2.0), wide_lo, wide_hi), ((0.75, 1.5), (0.7, 1.4), (0.8, 1.6)), ((1.0, 1.0), ONE, ONE)):
        s2, lo2, hi2 = (s[0] / f, s[1]), (lo[0] / f, lo[1]), (hi[0] / f, hi[1])
        a, b = _call(sums, n, rot, s, lo, hi), _call(scaled, n, rot, s2, lo2, hi2)
        assert a["rc"] == b["rc"] == 1 and a["determined"] == b["determined"]
        assert _bits(a["R_new"]) == _bits(b["R_new"]) and _bits(a["T_new"]) == _bits(b["T_new"])
        assert a["s_new"][1] == b["s_new"][1] and b["s_new"][0] == a["s_new"][0] / f
        Aa = np.array(A.pose_matrix(a["R_new"].tolist(), a["s_new"].tolist())).reshape(3, 3)
        Ab = np.array(A.pose_matrix(b["R_new"].tolist(), b["s_new"].tolist())).reshape(3, 3)
        assert _bits(Aa[:, 0]) == _bits(Ab[:, 0] * f) and _bits(Aa[:, 1:]) == _bits(Ab[:, 1:])
        seen += a["determined"] & 1
    if kind == "fitted":
        assert seen == 3                  # the x scale was fitted, not carried


# ---- the scales against the exact rational value ---------------------------------------------------------------------
def _accuracy_inputs():
    out = [("fitted nd %d offset %g" % (nd, off), _fitted(nd, off)) for nd in (50, 1000) for off in (0.0, 1e3, 1e5, 1e6)]
    for path, nm, nd in R.SMALL_SHAPES:
        for family in R.FAMILIES:
            for pose in R.POSES:
                out.append(("%s %d %d %s %s" % (path, nm, nd, family, pose), _sums(path, nm, nd, family, pose)))
    return out


def test_scales_against_the_exact_value():
    """|s^_a / s_a - 1| <= u (3 + 5 q_a + 8 p_a) with s_a = g_a / D_a exactly from the same doubles, while
    u (q_a + p_a) <= 2^-12 and nothing overflows or underflows (derivation in
    tests/icp_aniso_ref.py).  Far-origin clouds (offset 1e3 .. 1e6, the `offset` family at 1e5) are part of the sweep."""
    worst, seen, qmax, outside = 0.0, 0, 0.0, 0
    for name, (sums, n, rot) in _accuracy_inputs():
        ex = A.exact_s(sums, n, rot)
        got = _call(sums, n, rot, (1.0, 1.0))
        if got["rc"] != 1:
            continue
        for a in range(2):
            b = A.s_bound(*ex[a][1:]) if ex[a] else None
            if b is None:
                outside += 1
                continue
            sv, q, p = ex[a]
            assert got["determined"] >> a & 1, (name, a)
            err = abs(Fraction(float(got["s_new"][a])) / sv - 1)
            ratio = float(err / b)
            qmax = max(qmax, float(q))
            print(name, "axis", a, "s", got["s_new"][a], "q %.3g p %.3g" % (float(q), float(p)), "error/bound %.3f" % ratio)
            assert err <= b, (name, a, ratio)
            worst, seen = max(worst, ratio), seen + 1
    print("largest error / bound", worst, "over", seen, "scales;", outside, "outside the domain or not determined")
    assert seen >= 40 and qmax > 1e9


# ---- the behaviour conditions, by the numpy reference alone ----------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _scene(nt, err):
    ntrue, nclutter = {s[0]: s[1:] for s in G.SIZES}[nt]
    return A.aniso_scene(nt, ntrue, nclutter, G.SEEDS[nt], err)


@pytest.mark.parametrize("err", A.START_ERRORS)
@pytest.mark.parametrize("nt,ntrue,nclutter", G.SIZES)
def test_reference_behaviour(nt, ntrue, nclutter, err):
    sc = _scene(nt, err)
    g = A.ref_icp(sc["centers"], sc["truths"], sc["R0"], sc["s0"], sc["T0"], G.schedule(), G.ROUNDS)
    within, perr = G.conditions(sc, g["A"], g["T"])
    print("anisotropic: start errors", err, "within", within, "pose error", perr, "scales", g["s"], "kept", g["kept"],
          "starved", g["starved"], "unscaled", g["unscaled"])
    assert within == 1.0
    assert perr <= 0.02
    assert g["unscaled"] == [0, 0] and g["starved"] == 0


@pytest.mark.parametrize("err", A.START_ERRORS)
@pytest.mark.parametrize("nt,ntrue,nclutter", G.SIZES)
def test_rigid_and_similarity_references_from_the_same_start(nt, ntrue, nclutter, err):
    sc = _scene(nt, err)
    u = G.ref_icp(sc["centers"], sc["truths"], sc["A0"], sc["T0"], G.schedule(), G.ROUNDS)
    v = S.ref_icp(sc["centers"], sc["truths"], sc["A0"], sc["T0"], G.schedule(), G.ROUNDS, A.RATIO)
    pu, pv = G.conditions(sc, u["R"], u["T"])[1], G.conditions(sc, v["R"], v["T"])[1]
    print("start errors", err, "rigid pose error", pu, "similarity pose error", pv)
    if err in A.WRONG_STARTS:
        assert pu > 0.2 and pv > 0.2
    else:
        assert pu <= 0.02 and pv <= 0.02
