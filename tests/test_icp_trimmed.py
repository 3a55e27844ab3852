"""Trimmed ICP without a GPU: the two entry points through every layer of the binding, trim_schedule and
expected_share, the rule of the select on ties, +inf and NaN, and the behaviour scene held to its conditions by the numpy
reference alone (tests/icp_trimmed_ref.py) -- the device is held to the same conditions on the same seeds in
tests/test_icp_trimmed_gpu.py."""
import inspect
import math
import os
import re

import numpy as np
import pytest

import icp_gated_ref as G
import icp_trimmed_ref as TR
from test_abi import _csharp_imports, _declared, _header_prototypes
from vtkcloudpoint_amd import _native
from vtkcloudpoint_amd.icp import expected_share, trim_schedule, trimmed_icp   # noqa: F401  (the parent lacks them)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("vcp_icp_sums_trimmed", "vcp_icp_trimmed")
assert all(n in _native.SYMBOLS for n in NAMES)     # every test of this file fails without the feature


def test_abi_has_the_trimmed_entry_points():
    lib = _native.lib()
    decl = _declared()
    protos = _header_prototypes()
    imports = {name: classes for _, name, classes in _csharp_imports()}
    for name in NAMES:
        assert name in decl and hasattr(lib, name) and name in _native.SYMBOLS, name
        assert imports.get(name) == protos[name], name       # the DllImport passes the header's parameters
    assert len(protos["vcp_icp_sums_trimmed"]) == 12 and len(protos["vcp_icp_trimmed"]) == 22
    assert protos["vcp_icp_sums_trimmed"][7] == "i64"         # m, by value
    # the gated call's parameters, then trim_dist
    assert protos["vcp_icp_trimmed"][:21] == protos["vcp_icp_gated"] and protos["vcp_icp_trimmed"][21] == "ptr"
    for method, first in (("icp_sums_trimmed", ["self", "model", "data", "m", "R", "T"]),
                          ("icp_trimmed", ["self", "source", "target", "keep", "poses"])):
        params = list(inspect.signature(getattr(_native.Context, method)).parameters)
        assert params[:len(first)] == first, method
    assert list(inspect.signature(trimmed_icp).parameters) == [
        "centers", "truths", "keep", "n_angles", "mirror", "init_T", "max_iter", "max_landmarks", "min_pairs",
        "inlier_dist", "ctx"]
    from vtkcloudpoint_amd.icp import global_icp
    assert list(inspect.signature(global_icp).parameters)[-1] == "keep"      # appended: positional callers are unchanged
    assert inspect.signature(global_icp).parameters["keep"].default is None
    with open(os.path.join(ROOT, "vtkcloudpoint_amd", "host", "csharp", "MainForm.Gpu.cs")) as f:
        src = f.read()
    assert re.search(r"void\s+ICPTrimmed\s*\(\s*int\s+angles\s*,\s*bool\s+mirror\s*,\s*double\s+keepShare\s*,\s*double\s+"
                     r"matchDistance\s*\)", src)
    with open(os.path.join(ROOT, "include", "vcp.h")) as f:
        hdr = f.read()
    assert re.search(r"#define\s+VCP_ICPT_SELECT_WG_MAX\s+%d\b" % TR.SELECT_WG_MAX, hdr)


@pytest.mark.parametrize("start,end,rounds", [(1.0, 0.6, 10), (1.0, 0.75, 2), (0.9, 1e-3, 37), (0.7, 0.7, 5),
                                              (1.0, 5e-324, 100), (0.1 + 0.2, 0.1, 3), (1.0, 1.0, 4)])
def test_trim_schedule(start, end, rounds):
    f = trim_schedule(start, end, rounds)
    assert f.dtype == np.float64 and f.shape == (rounds,)
    assert f[0] == start and f[-1] == end                     # exact endpoints
    assert (np.diff(f) <= 0).all() and (f > 0).all() and (f <= 1).all()
    if rounds > 2:                                            # linear: constant steps, to rounding
        d = np.diff(f)
        assert np.allclose(d, (end - start) / (rounds - 1), rtol=1e-9, atol=1e-15)
    assert np.array_equal(trim_schedule(start, end, 1), [end])


def test_trim_schedule_refuses_nonsense():
    for bad in ((0.6, 0.9, 5), (0.6, 0.0, 5), (0.6, -1.0, 5), (0.6, 0.1, 0), (np.nan, 0.1, 3), (1.5, 0.5, 3),
                (0.5, np.nan, 3), (math.inf, 0.5, 3)):
        with pytest.raises(ValueError):
            trim_schedule(*bad)


def test_expected_share():
    assert expected_share(320, 300, 0.8) == min(1.0, 0.8 * 300 / 320) == 0.75
    assert expected_share(100, 300) == 1.0 and expected_share(300, 300) == 1.0
    assert expected_share(400, 100) == 0.25 and expected_share(400, 100, 0.5) == 0.125
    for bad in ((0, 10, 1.0), (10, 0, 1.0), (10, 10, 0.0), (10, 10, 1.5), (10, 10, math.nan)):
        with pytest.raises(ValueError):
            expected_share(*bad)


def test_keep_count():
    assert TR.keep_count(1.0, 7) == 7 and TR.keep_count(0.5, 7) == 4 and TR.keep_count(0.5, 8) == 4
    assert TR.keep_count(5e-324, 1000) == 1 and TR.keep_count(0.75, 320) == 240
    assert TR.keep_count(240 / 320, 320) == 240


def test_trim_mask():
    inf, nan = math.inf, math.nan
    # ties go to the lower index
    dd = np.array([4.0, 1.0, 4.0, 1.0, 4.0, 0.0])
    for m, want, thr in ((1, [5], 0.0), (2, [1, 5], 1.0), (3, [1, 3, 5], 1.0), (4, [0, 1, 3, 5], 4.0),
                         (5, [0, 1, 2, 3, 5], 4.0), (6, [0, 1, 2, 3, 4, 5], 4.0)):
        keep, t = TR.trim_mask(dd, m)
        assert np.flatnonzero(keep).tolist() == want and t == thr, m
    # +inf before NaN, NaN last; among NaNs the lower index first (whatever their payload or sign)
    dd = np.array([nan, inf, 2.0, -nan, inf, 0.5])
    order = [5, 2, 1, 4, 0, 3]
    for m in range(1, 7):
        keep, t = TR.trim_mask(dd, m)
        assert sorted(np.flatnonzero(keep).tolist()) == sorted(order[:m]), m
        assert TR.same_float(t, float(dd[order[m - 1]])), m
    assert TR.keys(np.array([nan, -nan])).tolist() == [0xFFFFFFFFFFFFFFFF] * 2
    assert TR.keys(np.array([0.0, 1.0, inf])).tolist() == [0, 0x3FF0000000000000, 0x7FF0000000000000]
    # the order of the keys is the order of the numbers, denormals included
    x = np.array([0.0, 5e-324, 2.2e-308, 1.0, np.nextafter(1.0, 2.0), 1e308, inf])
    assert (np.diff(TR.keys(x).astype(object)) > 0).all()
    for bad in (0, 7):
        with pytest.raises(ValueError):
            TR.trim_mask(dd, bad)


@pytest.mark.parametrize("nt,ntrue,nclutter", G.SIZES)
def test_reference_behaviour(nt, ntrue, nclutter):
    """The scene of the gated tests, by the reference alone: trimmed at the share of true centroids, at 0.6 and -- share
    1.0 -- not at all, from the scene's own start."""
    sc = G.scene(nt, ntrue, nclutter, G.SEEDS[nt])
    n = len(sc["centers"])
    assert sc["is_true"].sum() == ntrue and n == ntrue + nclutter
    g = TR.ref_trimmed_icp(sc["centers"], sc["truths"], sc["R0"], sc["T0"], [ntrue / n], G.ROUNDS)
    within, err = G.conditions(sc, g["R"], g["T"])
    print("share ntrue/n: within", within, "pose error", err, "kept", g["kept"], "trim_dist", g["trim_dist"])
    assert within == 1.0
    assert err < 0.01
    assert g["kept"] == ntrue
    g = TR.ref_trimmed_icp(sc["centers"], sc["truths"], sc["R0"], sc["T0"], [0.6], G.ROUNDS)
    within, err = G.conditions(sc, g["R"], g["T"])
    print("share 0.6: within", within, "pose error", err, "kept", g["kept"])
    assert within == 1.0
    assert err < 0.01
    u = TR.ref_trimmed_icp(sc["centers"], sc["truths"], sc["R0"], sc["T0"], [1.0], G.ROUNDS)
    within_u, err_u = G.conditions(sc, u["R"], u["T"])
    print("share 1.0: within", within_u, "pose error", err_u)
    assert within_u < 0.5
    assert u["kept"] == n
