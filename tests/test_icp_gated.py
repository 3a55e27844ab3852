"""Gated ICP without a GPU: the two entry points through every layer of the binding, gate_schedule, and the behaviour
scene held to its conditions by the numpy reference alone (tests/icp_gated_ref.py) -- the device is held to the same
conditions on the same seeds in tests/test_icp_gated_gpu.py."""
import inspect
import os
import re

import numpy as np
import pytest

import icp_gated_ref as G
from test_abi import _csharp_imports, _declared, _header_prototypes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("vcp_icp_sums_gated", "vcp_icp_gated")


def test_abi_has_the_gated_entry_points():
    from vtkcloudpoint_amd import _native
    lib = _native.lib()
    decl = _declared()
    protos = _header_prototypes()
    imports = {name: classes for _, name, classes in _csharp_imports()}
    for name in NAMES:
        assert name in decl and hasattr(lib, name) and name in _native.SYMBOLS, name
        assert imports.get(name) == protos[name], name       # the DllImport passes the header's parameters
    assert len(protos["vcp_icp_sums_gated"]) == 12 and len(protos["vcp_icp_gated"]) == 21
    assert protos["vcp_icp_sums_gated"][7] == "f64"           # gate, by value
    for method, first in (("icp_sums_gated", ["self", "model", "data", "gate"]),
                          ("icp_gated", ["self", "source", "target", "gates"])):
        params = list(inspect.signature(getattr(_native.Context, method)).parameters)
        assert params[:4] == first, method
    with open(os.path.join(ROOT, "vtkcloudpoint_amd", "host", "csharp", "MainForm.Gpu.cs")) as f:
        src = f.read()
    assert re.search(r"void\s+ICPGated\s*\(\s*int\s+angles\s*,\s*bool\s+mirror\s*,\s*double\s+gateStart\s*,\s*double\s+"
                     r"gateEnd\s*,\s*double\s+matchDistance\s*\)", src)


@pytest.mark.parametrize("start,end,rounds", [(0.6, 0.1, 10), (0.6, 0.1, 2), (3.0, 1e-3, 37), (0.7, 0.7, 5),
                                              (1e300, 1e-300, 100), (0.1 + 0.2, 0.1, 3)])
def test_gate_schedule(start, end, rounds):
    from vtkcloudpoint_amd.icp import gate_schedule
    g = gate_schedule(start, end, rounds)
    assert g.dtype == np.float64 and g.shape == (rounds,)
    assert g[0] == start and g[-1] == end                     # exact endpoints
    assert (np.diff(g) <= 0).all() and (g > 0).all()
    if start > end and rounds > 2:                            # geometric: a constant ratio, to rounding
        q = g[1:] / g[:-1]
        assert np.allclose(q, q[0], rtol=1e-9)
    assert np.array_equal(gate_schedule(start, end, 1), [end])


def test_gate_schedule_refuses_nonsense():
    from vtkcloudpoint_amd.icp import gate_schedule
    for bad in ((0.1, 0.6, 5), (0.6, 0.0, 5), (0.6, -1.0, 5), (0.6, 0.1, 0), (np.nan, 0.1, 3)):
        with pytest.raises(ValueError):
            gate_schedule(*bad)


@pytest.mark.parametrize("nt,ntrue,nclutter", G.SIZES)
def test_reference_behaviour(nt, ntrue, nclutter):
    """The scene shows what the gate is for, by the reference alone: gated, every true centroid ends on its truth;
    ungated from the same start, the clutter band walks the pose away."""
    sc = G.scene(nt, ntrue, nclutter, G.SEEDS[nt])
    assert sc["is_true"].sum() == ntrue and len(sc["centers"]) == ntrue + nclutter
    t = sc["truths"][:, :2]
    d2 = ((t[:, None, :] - t[None, :, :]) ** 2).sum(axis=2) + np.eye(nt) * 1e9
    assert d2.min() > G.SEPARATION ** 2
    gates = G.schedule()
    g = G.ref_icp(sc["centers"], sc["truths"], sc["R0"], sc["T0"], gates, G.ROUNDS)
    within, err = G.conditions(sc, g["R"], g["T"])
    print("gated: within", within, "pose error", err, "kept", g["kept"], "starved", g["starved"])
    assert within == 1.0
    assert err < 0.01
    assert g["kept"] == ntrue
    u = G.ref_icp(sc["centers"], sc["truths"], sc["R0"], sc["T0"], None, G.ROUNDS)
    within_u, err_u = G.conditions(sc, u["R"], u["T"])
    print("ungated: within", within_u, "pose error", err_u)
    assert within_u < 0.5
