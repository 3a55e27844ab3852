"""Similarity ICP without a GPU: the three entry points through every layer of the binding, the host step
(vcp_selftest_horn_sim, compiled from the source the device runs) against its restatement bit for bit and against the
exact rational scale, and the behaviour scene held to its conditions by the numpy reference alone
(tests/icp_sim_ref.py) -- the device is held to the same conditions on the same seeds in tests/test_icp_sim_gpu.py."""
import ctypes as C
import functools
import inspect
import math
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import icp_gated_ref as G
import icp_sim_ref as S
import icp_sums_ref as R
from test_abi import _csharp_imports, _declared, _header_prototypes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("vcp_icp_sums_sim", "vcp_selftest_horn_sim", "vcp_icp_sim")
INF, NAN = math.inf, math.nan
WIDE = (1e-300, 1e300)


def _N():
    from vtkcloudpoint_amd import _native
    return _native


def test_abi_has_the_similarity_entry_points():
    N = _N()
    lib = N.lib()
    decl = _declared()
    protos = _header_prototypes()
    imports = {name: classes for _, name, classes in _csharp_imports()}
    for name in NAMES:
        assert name in decl and hasattr(lib, name) and name in N.SYMBOLS, name
        assert imports.get(name) == protos[name], name       # the DllImport passes the header's parameters
    assert len(protos["vcp_icp_sums_sim"]) == 12 and len(protos["vcp_selftest_horn_sim"]) == 11
    assert len(protos["vcp_icp_sim"]) == 25
    assert protos["vcp_icp_sums_sim"] == protos["vcp_icp_sums_gated"]
    assert protos["vcp_icp_sim"][13:15] == ["f64", "f64"]     # ratio_min, ratio_max, by value
    for obj, method, first in ((N.Context, "icp_sums_sim", ["self", "model", "data", "gate"]),
                               (N.Context, "icp_sim", ["self", "source", "target", "gates", "ratio_range"]),
                               (N, "selftest_horn_sim", ["sums", "n", "c", "ratio_range", "V"])):
        params = list(inspect.signature(getattr(obj, method)).parameters)
        assert params[:len(first)] == first, method
    from vtkcloudpoint_amd import icp
    assert list(inspect.signature(icp.similarity_icp).parameters)[:4] == ["centers", "truths", "gates", "ratio_range"]
    assert list(inspect.signature(icp.global_similarity_icp).parameters)[:7] == \
        ["centers", "truths", "bases", "scale_range", "inlier_dist", "gates", "ratio_range"]
    with open(os.path.join(ROOT, "vtkcloudpoint_amd", "host", "csharp", "MainForm.Gpu.cs")) as f:
        src = f.read()
    assert re.search(r"void\s+ICPSimilarity\s*\(", src) and "VcpNative.vcp_icp_sim(" in src


# ---- the step against its restatement --------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _sums(path, nm, nd, family, pose="generic"):
    Ssum, n = S.case_sums(path, nm, nd, family, pose)
    Ssum.setflags(write=False)
    return Ssum, n


def _call(sums, n, c, rng, V=None):
    return _N().selftest_horn_sim(sums, n, c, rng, V)


def _same_step(got, want):
    rc, R1s, T1, ku, cn = want
    assert got["rc"] == rc
    assert got["R1s"].tolist() == R1s and got["T1"].tolist() == T1, (got, want)
    assert got["k_used"] == ku and got["c_new"] == cn, (got, want)
    assert not any(math.copysign(1.0, a) != math.copysign(1.0, b) for a, b in zip(got["R1s"].tolist(), R1s))


@pytest.mark.parametrize("pose", R.POSES)
@pytest.mark.parametrize("family", R.FAMILIES)
@pytest.mark.parametrize("path,nm,nd", R.SMALL_SHAPES)
def test_step_is_the_restatement(path, nm, nd, family, pose):
    N = _N()
    sums, n = _sums(path, nm, nd, family, pose)
    assert np.isfinite(sums).all()
    c = 0.75
    V = np.zeros(16)
    cold = _call(sums, n, c, WIDE)
    rc0, R1, T1h = S.horn(N, sums, n)
    assert rc0 == 1
    _same_step(cold, S.step(sums, n, R1, c, *WIDE))
    # a garbage basis is a cold start; the basis it leaves is a warm one, and the step from it is horn's from it
    assert _call(sums, n, c, WIDE, V)["R1s"].tolist() == cold["R1s"].tolist()
    Vw = V.copy()
    rcw, R1w, _ = S.horn(N, sums, n, Vw)
    warm = _call(sums, n, c, WIDE, V)
    assert rcw == 1 and np.array_equal(V, Vw)
    _same_step(warm, S.step(sums, n, R1w, c, *WIDE))
    if cold["rc"] == 2:                      # every pair on one model point (nm = 1; the offset family moved by the
        assert nm == 1 or (family, pose) == ("offset", "generic")   # pose): vY cancels, the rigid step
        assert cold["k_used"] == 1.0 and cold["c_new"] == c
        assert cold["R1s"].tolist() == R1 and cold["T1"].tolist() == T1h
        return
    t = cold["c_new"]
    assert t == c * cold["k_used"]
    for rng, what in (((2 * t, 4 * t), "low"), ((t / 4, t / 2), "high"), ((t / 2, 2 * t), "free"), ((t, t), "free"),
                      ((np.nextafter(t, INF), 3 * t), "low"), ((t / 3, np.nextafter(t, 0.0)), "high")):
        got = _call(sums, n, c, rng)
        _same_step(got, S.step(sums, n, R1, c, *rng))
        if what == "low":
            assert got["c_new"] == rng[0] and got["k_used"] == rng[0] / c
        elif what == "high":
            assert got["c_new"] == rng[1] and got["k_used"] == rng[1] / c
        else:
            assert got["c_new"] == t and got["k_used"] == cold["k_used"]
    # k_used == 1.0: the rigid step in every bit
    for cc in (1.0, c):
        got = _call(sums, n, cc, (cc, cc))
        assert got["k_used"] == 1.0 and got["c_new"] == cc and got["rc"] == 1
        assert got["R1s"].tobytes() == np.array(R1).tobytes() and got["T1"].tobytes() == np.array(T1h).tobytes()


def test_undetermined_scale():
    N = _N()
    z = np.zeros(18)
    got = _call(z, 5, 0.8, (0.5, 2.0))       # coincident points: horn's R1 = I, T1 = 0
    assert got["rc"] == 2 and got["k_used"] == 1.0 and got["c_new"] == 0.8
    assert got["R1s"].tolist() == np.eye(3).reshape(9).tolist() and got["T1"].tolist() == [0.0, 0.0, 0.0]
    # every pair on one target, exactly: vY = 56/4 - 14 = 0
    P = np.array([[1.0, 0.0, 0.0], [0.0, 2.0, 0.0], [0.0, 0.0, 3.0], [1.0, 1.0, 1.0]])
    y = np.array([1.0, 2.0, 3.0])
    s = np.zeros(18)
    s[0:3], s[3:6] = P.sum(axis=0), 4 * y
    s[6:15] = (P[:, :, None] * y[None, None, :]).sum(axis=0).reshape(9)
    s[15], s[16], s[17] = ((P - y) ** 2).sum(), (P * P).sum(), 4 * (y * y).sum()
    rc, R1, T1 = S.horn(N, s, 4)
    got = _call(s, 4, 1.25, (0.5, 2.0))
    assert rc == 1 and got["rc"] == 2 and got["k_used"] == 1.0 and got["c_new"] == 1.25
    assert got["R1s"].tolist() == R1 and got["T1"].tolist() == T1
    # the same with vP = 0 (the two columns swapped), and a NaN or an infinity in either: comparisons with NaN are false
    sums, n = _sums("pairs", 100, 129, "generic")
    rc, R1, T1 = S.horn(N, sums, n)
    for k, v in ((16, NAN), (17, NAN), (16, INF), (17, INF), (16, 0.0), (17, 0.0), (16, -1.0)):
        b = np.array(sums)
        b[k] = v
        got = _call(b, n, 1.0, (0.5, 2.0))
        assert got["rc"] == 2 and got["k_used"] == 1.0 and got["c_new"] == 1.0, (k, v)
        assert got["R1s"].tolist() == R1 and got["T1"].tolist() == T1
        _same_step(got, S.step(b, n, R1, 1.0, 0.5, 2.0))


def test_failed_solve_writes_nothing():
    N = _N()
    sums, n = _sums("pairs", 100, 129, "generic")
    for k, v in ((0, NAN), (7, INF), (4, -INF)):
        b = np.array(sums)
        b[k] = v
        assert S.horn(N, b, n)[0] == 0
        R1s, T1 = np.full(9, 7.0), np.full(3, 7.0)
        ku, cn = C.c_double(7.0), C.c_double(7.0)
        rc = N.lib().vcp_selftest_horn_sim(N._ptr(b), C.c_int64(n), None, C.c_int(0), C.c_double(1.0), C.c_double(0.5),
                                           C.c_double(2.0), N._ptr(R1s), N._ptr(T1), C.byref(ku), C.byref(cn))
        assert rc == 0 and (R1s == 7).all() and (T1 == 7).all() and ku.value == 7.0 and cn.value == 7.0
        assert _call(b, n, 1.0, (0.5, 2.0))["rc"] == 0


def test_every_argument_error():
    N = _N()
    sums, n = _sums("pairs", 100, 129, "generic")
    sums = np.array(sums)
    V = np.zeros(16)

    def raw(**kw):
        R1s, T1 = np.full(9, 7.0), np.full(3, 7.0)
        ku, cn = C.c_double(7.0), C.c_double(7.0)
        a = dict(sums=N._ptr(sums), n=n, V=N._ptr(V), use_v=1, c=1.0, lo=0.5, hi=2.0, R1s=N._ptr(R1s), T1=N._ptr(T1),
                 ku=C.byref(ku), cn=C.byref(cn))
        a.update(kw)
        rc = N.lib().vcp_selftest_horn_sim(a["sums"], C.c_int64(a["n"]), a["V"], C.c_int(a["use_v"]), C.c_double(a["c"]),
                                           C.c_double(a["lo"]), C.c_double(a["hi"]), a["R1s"], a["T1"], a["ku"], a["cn"])
        if rc < 0:
            assert (R1s == 7).all() and (T1 == 7).all() and ku.value == 7.0 and cn.value == 7.0
        return rc

    assert raw() == 1 and raw(V=None, use_v=0) == 1
    for kw in (dict(sums=None), dict(R1s=None), dict(T1=None), dict(ku=None), dict(cn=None), dict(n=0), dict(n=-3),
               dict(V=None, use_v=1), dict(c=NAN), dict(c=0.0), dict(c=-1.0), dict(lo=NAN), dict(lo=0.0), dict(lo=-0.5),
               dict(hi=NAN), dict(hi=INF), dict(lo=1.0, hi=0.999), dict(lo=INF, hi=INF)):
        assert raw(**kw) == -1, kw
    assert raw(lo=1.0, hi=1.0) == 1 and raw(c=INF) == 1      # c = +inf is > 0: every factor clamps to 0
    with pytest.raises(N.VcpError):
        N.selftest_horn_sim(sums, n, -1.0, (0.5, 2.0))


@pytest.mark.parametrize("family", ("generic", "offset", "planar", "cancel", "lattice"))
@pytest.mark.parametrize("e", (-40, 1, 40, 100))
def test_power_of_two_invariance(family, e):
    sums, n = _sums("pairs", 100, 1000, family, "none")
    f = 2.0 ** e
    scaled = np.array(sums)
    scaled[0:6] *= f
    scaled[6:18] *= f * f
    for c, rng in ((1.0, WIDE), (0.75, (0.9, 1.1)), (1.0, (1.0, 1.0))):
        a, b = _call(sums, n, c, rng), _call(scaled, n, c, rng)
        assert a["rc"] == b["rc"] == 1
        assert a["R1s"].tobytes() == b["R1s"].tobytes() and a["k_used"] == b["k_used"] and a["c_new"] == b["c_new"]
        assert (a["T1"] * f).tobytes() == b["T1"].tobytes()


# ---- k against the exact rational value ------------------------------------------------------------------------------
@pytest.mark.parametrize("family", R.FAMILIES)
def test_k_against_the_exact_scale(family):
    """|k^ / k - 1| <= u (a + b (qP + qY)), k = sqrt(vY / vP) exactly from the same sums, tested
    on the squares: k^2 (1 - bound)^2 <= k^^2 <= k^2 (1 + bound)^2 in rational arithmetic."""
    worst, seen, qmax = 0.0, 0, 0.0
    for path, nm, nd, pose in [s + (p,) for s in R.SMALL_SHAPES for p in R.POSES]:
        sums, n = _sums(path, nm, nd, family, pose)
        ex = S.exact_k2(sums, n)
        b = S.k_bound(*ex[1:]) if ex else None
        if b is None:            # every pair on one model point: vY is zero or what the roundings left of it
            assert nm == 1 or (family, pose) == ("offset", "generic"), (family, path, nm, nd, pose)
            continue
        r, qP, qY = ex
        qmax = max(qmax, float(qP), float(qY))
        got = _call(sums, n, 1.0, WIDE)
        assert got["rc"] == 1 and got["c_new"] == got["k_used"]
        k2 = Fraction(got["k_used"]) ** 2
        ratio = abs(float(k2 / r - 1)) / 2 / float(b)         # |k^/k - 1| / bound to first order
        print(family, path, nm, nd, pose, "k", got["k_used"], "qP %.3g qY %.3g" % (float(qP), float(qY)), "error/bound %.3f" % ratio)
        assert r * (1 - b) ** 2 <= k2 <= r * (1 + b) ** 2, (family, path, nm, nd, ratio)
        worst, seen = max(worst, ratio), seen + 1
    print(family, "largest error / bound", worst)
    assert seen >= (len(R.SMALL_SHAPES) - 3) * (1 if family == "offset" else 2)
    if family == "offset":                                   # the sums cancel hard: the bound is dominated by q
        assert qmax > 1e6


# ---- the behaviour conditions, by the numpy reference alone ----------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _ref(nt, err, rng):
    ntrue, nclutter = {s[0]: s[1:] for s in G.SIZES}[nt]
    sc = S.scaled_scene(nt, ntrue, nclutter, G.SEEDS[nt], err)
    return sc, S.ref_icp(sc["centers"], sc["truths"], sc["R0"], sc["T0"], G.schedule(), G.ROUNDS, rng)


@pytest.mark.parametrize("err", S.START_ERRORS)
@pytest.mark.parametrize("nt,ntrue,nclutter", G.SIZES)
def test_reference_behaviour(nt, ntrue, nclutter, err):
    sc, g = _ref(nt, err, S.RATIO_RANGE)
    within, perr = G.conditions(sc, g["R"], g["T"])
    k = S.linear_scale(g["R"])
    print("similarity: start error", err, "within", within, "pose error", perr, "k", k, "ratio", g["ratio"], "kept",
          g["kept"], "starved", g["starved"], "unscaled", g["unscaled"])
    assert within == 1.0
    assert perr < 0.01
    assert abs(k / S.K_UNIT - 1.0) < 1e-3
    assert g["unscaled"] == 0
    # ratio is the nominal product of the factors: the pose's scale is the start's times it, to roundings
    assert abs(k / (S.K_UNIT * (1.0 + err) * g["ratio"]) - 1.0) < 1e-12


@pytest.mark.parametrize("nt,ntrue,nclutter", G.SIZES)
def test_rigid_reference_loses_the_field_at_two_percent(nt, ntrue, nclutter):
    sc = S.scaled_scene(nt, ntrue, nclutter, G.SEEDS[nt], 0.02)
    u = G.ref_icp(sc["centers"], sc["truths"], sc["R0"], sc["T0"], G.schedule(), G.ROUNDS)
    within, perr = G.conditions(sc, u["R"], u["T"])
    print("rigid at 2 %: within", within, "pose error", perr)
    assert within < 0.5
    # and the similarity reference whose range is closed is that rigid loop
    s = S.ref_icp(sc["centers"], sc["truths"], sc["R0"], sc["T0"], G.schedule(), G.ROUNDS, (1.0, 1.0))
    assert s["ratio"] == 1.0 and np.allclose(s["R"], u["R"], atol=1e-12) and np.allclose(s["T"], u["T"], atol=1e-12)


@pytest.mark.parametrize("nt,ntrue,nclutter", G.SIZES)
def test_reference_ratio_ends_on_the_bound(nt, ntrue, nclutter):
    sc, g = _ref(nt, 0.05, (0.99, 1.01))
    print("5 % start, range (0.99, 1.01): ratio", g["ratio"])
    assert g["ratio"] == 0.99
