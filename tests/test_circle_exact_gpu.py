"""vcp_mcc and vcp_cluster_shapes on the families of shape_families.py, on the MI355X: bit for bit the oracle (host and
device forms, twice in a row), and -- not taken on trust from the oracle -- the device's own circle, hull and rectangle
held to the exact references of circle_ref.py with the bounds of test_circle_exact.py."""
import numpy as np
import pytest

import shape_families as SF

pytestmark = pytest.mark.gpu

CIRCLE = ("centers", "radius", "valid", "hull_n")
RECT = ("rect_valid", "rect_edge", "rect_len", "rect_xy")


def _same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


def _host(vcp_ctx, c):
    if "gpu" not in c:
        c["gpu"] = vcp_ctx.cluster_shapes(c["xy"], c["labels"], c["K"], c["order"])
    return c["gpu"]


def _dev(vcp_ctx, c):
    import torch
    K, n, order = c["K"], len(c["labels"]), c["order"]
    m = n if order is None else len(order)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    xy, lab = dev(c["xy"]), dev(c["labels"])
    od = None if order is None else dev(order)
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device="cuda")
    o = dict(centers=z((K, 2), torch.float64), radius=z(K, torch.float64), valid=z(K, torch.uint8), hull_n=z(K, torch.int32),
             rect_xy=z((K, 4, 2), torch.float64), rect_len=z((K, 2), torch.float64), rect_edge=z(K, torch.int32),
             rect_valid=z(K, torch.uint8), hull_off=z(K + 1, torch.int32), hull_idx=z(max(m, 1), torch.int32))
    torch.cuda.synchronize()
    p = {k: v.data_ptr() for k, v in o.items()}
    vcp_ctx.cluster_shapes_dev(xy.data_ptr(), lab.data_ptr(), None if od is None else od.data_ptr(), m, n, K, p["centers"],
                               p["radius"], p["valid"], p["hull_n"], p["rect_xy"], p["rect_len"], p["rect_edge"],
                               p["rect_valid"], p["hull_off"], p["hull_idx"])
    r = {k: v.cpu().numpy() for k, v in o.items()}
    r["hull_idx"] = r["hull_idx"][: r["hull_off"][K]]
    return r


def _hull_xy(c, got, k):
    return c["xy"][got["hull_idx"][got["hull_off"][k]:got["hull_off"][k + 1]]]


@pytest.mark.parametrize("name", sorted(SF.ALL))
def test_equals_the_oracle(vcp_ctx, oracle, name):
    """Circle, hull and rectangle of both entry points, host and device forms, each twice: the oracle's bits."""
    c = SF.family(name)
    ref = SF.oracle_shapes(oracle, c)
    assert ref["valid"].sum() >= c["K"] - 1
    runs = [_host(vcp_ctx, c), vcp_ctx.cluster_shapes(c["xy"], c["labels"], c["K"], c["order"]), _dev(vcp_ctx, c), _dev(vcp_ctx, c)]
    for got in runs:
        for key in CIRCLE + RECT:
            assert _same(got[key], ref[key]), (name, key, np.flatnonzero([not _same(a, b) for a, b in zip(got[key], ref[key])]))
        assert got["hull_off"][0] == 0 and _same(np.diff(got["hull_off"]), np.where(ref["valid"] == 1, ref["hull_n"], 0))
        for k in range(c["K"]):
            if ref["valid"][k] == 1:
                assert _same(_hull_xy(c, got, k), ref["hull_xy"][k]), (name, k)
        assert _same(got["hull_idx"], runs[0]["hull_idx"])
    for _ in range(2):
        mcc = vcp_ctx.mcc(c["xy"], c["labels"], c["K"], c["order"])
        for key in CIRCLE:
            assert _same(mcc[key], ref[key]), (name, key)


@pytest.mark.parametrize("name", sorted(SF.FINITE))
def test_device_against_exact_geometry(vcp_ctx, oracle, name):
    """The device's own outputs against exact geometry: how far a member lies beyond the circle, |r - r_exact|,
    |c - c_exact| and how far a member lies outside the rectangle, within twice the figures recorded for the family;
    the hull is the exact hull (members on its edges allowed) wherever the wrap is not exempt."""
    c = SF.family(name)
    got = _host(vcp_ctx, c)
    w = SF.figures(c, got)
    print("%-15s clusters %3d  beyond %.3g  |r - r_exact| %.3g  |c - c_exact| %.3g  outside the rectangle %.3g (%d)"
          % (name, w["checked"], w["beyond"], w["r"], w["c"], w["rect"], w["rect_checked"]))
    SF.check_bounds(name, w)
    assert w["rect_checked"] > 0
    n_hull = 0
    for k, kind in enumerate(c["kinds"]):
        if got["valid"][k] == 1 and kind not in SF.HULL_EXEMPT:
            assert SF.hull_is_exact(c, k, _hull_xy(c, got, k)), (name, k, kind)
            n_hull += 1
    assert n_hull > 0
    # where the insertion rule fires: read from the oracle's literal against its repaired result
    lit = oracle.get_circles(c["xy"], c["labels"], c["K"], c["order"], literal=True)
    rep = SF.oracle_shapes(oracle, c)
    fired = (rep["inserted"] > 0)
    assert _same(fired, (lit["radius"] != rep["radius"]) & (lit["radius"] > 0))
    if name in SF.NEVER_FIRES:
        assert not fired.any()
    if name in SF.MUST_FIRE:
        assert fired.any() and (got["radius"][fired] > lit["radius"][fired]).all()
