"""Unique-correspondence ICP without a GPU: the two entry points through every layer of the binding, the winner rule on
ties, +inf and NaN, and the ghost scene held to its conditions by the numpy references alone
(tests/icp_unique_ref.py) -- the device is held to the same conditions on the same seeds in
tests/test_icp_unique_gpu.py."""
import inspect
import math
import os
import re

import numpy as np
import pytest

import icp_gated_ref as G
import icp_unique_ref as U
from test_abi import _csharp_imports, _declared, _header_prototypes
from vtkcloudpoint_amd import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("vcp_icp_sums_unique", "vcp_icp_unique")
assert all(n in _native.SYMBOLS for n in NAMES)     # every test of this file fails without the feature


def test_abi_has_the_unique_entry_points():
    from vtkcloudpoint_amd.icp import global_icp, global_unique_icp, unique_icp
    lib = _native.lib()
    decl = _declared()
    protos = _header_prototypes()
    imports = {name: classes for _, name, classes in _csharp_imports()}
    for name in NAMES:
        assert name in decl and hasattr(lib, name) and name in _native.SYMBOLS, name
        assert imports.get(name) == protos[name], name       # the DllImport passes the header's parameters
    assert len(protos["vcp_icp_sums_unique"]) == 13 and len(protos["vcp_icp_unique"]) == 22
    # the gated forms' parameters, then lost
    assert protos["vcp_icp_sums_unique"][:12] == protos["vcp_icp_sums_gated"] and protos["vcp_icp_sums_unique"][12] == "ptr"
    assert protos["vcp_icp_unique"][:21] == protos["vcp_icp_gated"] and protos["vcp_icp_unique"][21] == "ptr"
    sig = inspect.signature(_native.Context.icp_sums_unique)
    assert list(sig.parameters) == ["self", "model", "data", "gate", "R", "T", "want_nn", "want_keep"]
    assert [sig.parameters[k].default for k in ("R", "T", "want_nn", "want_keep")] == [None, None, True, True]
    sig = inspect.signature(_native.Context.icp_unique)
    assert list(sig.parameters) == ["self", "source", "target", "gates", "poses", "init_T", "max_iter", "max_landmarks",
                                    "min_pairs", "inlier_dist"]
    assert [p.default for p in list(sig.parameters.values())[4:]] == [1, None, 100, 200, 3, np.inf]
    assert sig == inspect.signature(_native.Context.icp_gated)
    sig = inspect.signature(unique_icp)
    assert list(sig.parameters) == ["centers", "truths", "gates", "n_angles", "mirror", "init_T", "max_iter",
                                    "max_landmarks", "min_pairs", "inlier_dist", "ctx"]
    assert [p.default for p in list(sig.parameters.values())[3:]] == [1, False, None, 100, 200, 3, np.inf, None]
    sig = inspect.signature(global_unique_icp)
    assert list(sig.parameters) == ["centers", "truths", "bases", "len_tol", "inlier_dist", "gates", "mirror", "max_iter",
                                    "max_landmarks", "min_pairs", "ctx"]
    assert [p.default for p in list(sig.parameters.values())[6:]] == [False, 20, 200, 3, None]
    assert list(inspect.signature(global_icp).parameters)[-1] == "keep"       # global_icp stays as it was
    with open(os.path.join(ROOT, "vtkcloudpoint_amd", "host", "csharp", "MainForm.Gpu.cs")) as f:
        src = f.read()
    assert re.search(r"void\s+ICPUnique\s*\(\s*int\s+angles\s*,\s*bool\s+mirror\s*,\s*double\s+gateStart\s*,\s*double\s+"
                     r"gateEnd\s*,\s*double\s+matchDistance\s*\)", src)
    assert "VcpNative.vcp_icp_unique(" in src


def test_unique_mask():
    inf, nan = math.inf, math.nan
    # two landmarks with bit-equal dd on one target: the lower index wins
    assert U.unique_mask([3, 3], [0.25, 0.25]).tolist() == [True, False]
    assert U.unique_mask([3, 0, 3, 3], [0.5, 9.0, 0.25, 0.25]).tolist() == [False, True, True, False]
    # the smaller distance wins whatever its index; -0.0 does not occur (dd is a sum of squares)
    assert U.unique_mask([1, 1, 1], [2.0, 1.0, 3.0]).tolist() == [False, True, False]
    # +inf before NaN
    assert U.unique_mask([0, 0], [nan, inf]).tolist() == [False, True]
    assert U.unique_mask([0, 0, 0], [nan, inf, 1e308]).tolist() == [False, False, True]
    # a target with only NaN pairs keeps the lowest index (whatever the payload or sign of the NaN)
    assert U.unique_mask([2, 2, 2, 5], [nan, -nan, nan, nan]).tolist() == [True, False, False, True]
    # all landmarks on one target: one kept
    rng = np.random.default_rng(5)
    dd = rng.random(100)
    win = U.unique_mask(np.zeros(100, int), dd)
    assert win.sum() == 1 and win[np.argmin(dd)]
    # injective nn: all kept
    assert U.unique_mask(rng.permutation(50), rng.random(50)).all()
    # denormal distances order as numbers
    assert U.unique_mask([0, 0, 0], [1e-310, 5e-324, 0.5]).tolist() == [False, True, False]


def test_keep_codes():
    """The gate plays no part in the choice of the winner: a winner it drops leaves its target empty."""
    nan = math.nan
    nn = [0, 0, 1, 1, 2]
    dd = [0.01, 0.04, 1.0, 0.81, nan]
    assert U.keep_codes(nn, dd, math.inf).tolist() == [1, 2, 2, 1, 1]
    assert U.keep_codes(nn, dd, 0.9).tolist() == [1, 2, 2, 0, 1]          # sqrt(0.81) = 0.9 >= 0.9: dropped
    assert U.keep_codes(nn, dd, 0.15).tolist() == [1, 2, 2, 0, 1]         # the loser at 0.2 lies outside, the winner inside
    assert U.keep_codes(nn, dd, 0.05).tolist() == [0, 2, 2, 0, 1]         # a NaN winner is kept by any gate
    # a loser inside the gate stays lost (a winner is never farther than its loser, so the gate cannot drop the winner
    # and admit the loser: what it can do is drop both, and the target then stays empty)
    assert U.keep_codes([4, 4], [0.0001, 0.0004], 0.05).tolist() == [1, 2]
    assert U.keep_codes([4, 4], [0.0001, 0.0004], 0.01).tolist() == [0, 2]


@pytest.mark.parametrize("nt,ntrue,nclutter", G.SIZES)
def test_reference_behaviour(nt, ntrue, nclutter):
    """The gated scene with ghosts beside 40 % of the true centroids, all on the same side, by the references alone:
    the gated loop ends at the predicted bias, the same loop with one centroid per truth well below it."""
    for seed in U.SEEDS[nt]:
        sc = U.ghost_scene(nt, ntrue, nclutter, seed)
        g = sc["n_ghost"]
        assert g == round(0.4 * ntrue) and len(sc["centers"]) == ntrue + nclutter + g
        assert sc["is_true"].sum() == ntrue and sc["is_ghost"].sum() == g and not (sc["is_true"] & sc["is_ghost"]).any()
        bias = sc["bias"]
        assert bias == 0.07 * g / (ntrue + g) and abs(bias - 0.02) < 3e-4
        # a ghost lies 0.07 from a truth that has a true centroid of its own
        x = sc["centers"] @ sc["R_true"].T + sc["T_true"]
        nn, dd = G.brute_nn(sc["truths"], x[sc["is_ghost"]])
        assert (np.abs(np.sqrt(dd) - 0.07) < 5 * G.NOISE).all() and np.isin(nn, sc["truth_of"][sc["is_true"]]).all()
        gates = G.schedule()
        a = G.ref_icp(sc["centers"], sc["truths"], sc["R0"], sc["T0"], gates, G.ROUNDS)
        within_a, err_a = G.conditions(sc, a["R"], a["T"])
        u = U.ref_unique_icp(sc["centers"], sc["truths"], sc["R0"], sc["T0"], gates, G.ROUNDS)
        within_u, err_u = G.conditions(sc, u["R"], u["T"])
        print("seed", seed, "bias", bias, "gated: within", within_a, "pose error", err_a, "kept", a["kept"],
              "| unique: within", within_u, "pose error", err_u, "kept", u["kept"], "lost", u["lost"])
        assert within_a == 1.0 and within_u == 1.0
        assert err_a >= 0.75 * bias
        assert err_u <= 0.5 * bias
        assert u["kept"] == ntrue and u["lost"] >= g and u["starved"] == 0
        assert a["kept"] == ntrue + g
