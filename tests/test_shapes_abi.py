"""Cluster shapes and the radius / aspect filter without a GPU: the four entry points exist in the library, the header,
the Python binding and the C# imports with matching arity; the numpy restatement of the rectangle and the filter
(tests/shapes_ref.py) on hand-built cases whose answers are known; the host-side removal keeps order."""
import math

import numpy as np

import shapes_ref as S
from test_abi import _csharp_imports, _header_prototypes

NAMES = ["vcp_cluster_shapes", "vcp_cluster_shapes_dev", "vcp_cluster_filter", "vcp_cluster_filter_dev"]


def test_the_four_symbols_everywhere_with_matching_arity():
    from vtkcloudpoint_amd import _native
    lib = _native.lib()
    protos = _header_prototypes()
    cs = {name: classes for _, name, classes in _csharp_imports()}
    for nm in NAMES:
        assert hasattr(lib, nm), nm
        assert nm in protos and nm in _native.SYMBOLS, nm
        assert cs.get(nm) == protos[nm], (nm, cs.get(nm), protos[nm])
    assert len(protos["vcp_cluster_shapes"]) == len(protos["vcp_cluster_shapes_dev"]) == 17
    assert len(protos["vcp_cluster_filter"]) == len(protos["vcp_cluster_filter_dev"]) == 15
    for meth in ("cluster_shapes", "cluster_shapes_dev", "cluster_filter", "cluster_filter_dev"):
        assert callable(getattr(_native.Context, meth))


def _hull(oracle, pts):
    return oracle.min_circle(np.asarray(pts, np.float64))[2]


def test_unit_square_turned_by_30_degrees(oracle):
    rng = np.random.default_rng(3)
    c, s = math.cos(math.radians(30)), math.sin(math.radians(30))
    sq = np.array([[0, 0], [1, 0], [1, 1], [0, 1]], float)
    pts = np.r_[sq, rng.uniform(0.1, 0.9, (40, 2))] @ np.array([[c, s], [-s, c]]) + (5.0, -2.0)
    hull = _hull(oracle, pts[rng.permutation(len(pts))])
    assert len(hull) == 4
    r = S.rectangle(hull)
    assert r["valid"] == 1 and 0 <= r["edge"] < 4  # which of the four edges wins is rounding
    assert np.allclose(r["len"], [1.0, 1.0], rtol=0, atol=1e-14)
    assert abs(r["len"][0] * r["len"][1] - 1.0) <= 1e-14
    # the corners are the square's corners
    d = np.abs(r["xy"][:, None, :] - hull[None, :, :]).max(2).min(1)
    assert d.max() < 1e-13


def test_integer_rectangle_is_exact(oracle):
    pts = np.array([[0, 0], [3, 0], [3, 1], [0, 1], [1, 0.5], [2, 0.5], [1.5, 0.25], [2.5, 0.75]], float)
    hull = _hull(oracle, pts)
    assert hull[0].tolist() == [0.0, 0.0] and hull[1].tolist() == [3.0, 0.0]
    r = S.rectangle(hull)
    assert r["valid"] == 1 and r["edge"] == 0  # edges 0 and 2 tie at area 3: the lower index wins
    assert r["len"].tolist() == [3.0, 1.0]
    assert r["areas"][0] == r["areas"][2] == 3.0
    assert r["xy"].tolist() == [[0.0, 0.0], [3.0, 0.0], [3.0, 1.0], [0.0, 1.0]]
    f = S.cluster_filter(np.ones(len(pts), np.int32), 1, [2.0], [1], r["len"][None], [1], np.inf, 2.0)
    assert f["filtered"].tolist() == [1] and f["n_kept"] == 0
    f = S.cluster_filter(np.ones(len(pts), np.int32), 1, [2.0], [1], r["len"][None], [1], np.inf, 3.0)
    assert f["filtered"].tolist() == [0] and f["n_kept"] == len(pts)  # strict comparison: 3 > 3 * 1 is false


def test_points_on_a_line_have_zero_width_and_any_finite_aspect_filters_them(oracle):
    pts = np.array([[i, 2 * i] for i in range(6)], float)
    hull = _hull(oracle, pts)
    r = S.rectangle(hull)
    assert r["valid"] == 1 and r["len"][1] == 0.0 and r["len"][0] > 0
    assert all(a == 0.0 for a in r["areas"] if a is not None)
    lab = np.ones(6, np.int32)
    f = S.cluster_filter(lab, 1, [1.0], [1], r["len"][None], [1], np.inf, 1e300)
    assert f["filtered"].tolist() == [1] and f["keep"].tolist() == [0] * 6 and f["n_kept"] == 0
    f = S.cluster_filter(lab, 1, [1.0], [1], r["len"][None], [1], np.inf, np.inf)  # inf * 0 = NaN: criterion off
    assert f["filtered"].tolist() == [0]


def test_coincident_points_have_no_rectangle_and_are_kept(oracle):
    pts = np.tile([[2.5, -1.0]], (5, 1))
    c, rad, hull = oracle.min_circle(pts)
    assert len(hull) == 1 and rad == 0.0
    r = S.rectangle(hull)
    assert r["valid"] == 0 and r["edge"] == -1 and r["len"].tolist() == [0.0, 0.0]
    assert r["xy"].tolist() == [[2.5, -1.0]] * 4
    f = S.cluster_filter(np.ones(5, np.int32), 1, [rad], [1], r["len"][None], [r["valid"]], 0.0, 0.0)
    assert f["filtered"].tolist() == [0] and f["keep"].tolist() == [1] * 5


def test_filter_expression_edges():
    lab = np.array([0, 1, 2, 3, 0, 2, 1, 3], np.int32)
    rad, val = [1.0, 5.0, 9.0], [1, 1, 0]
    f = S.cluster_filter(lab, 3, rad, val, None, None, 2.0, np.nan)
    assert f["filtered"].tolist() == [0, 1, 0] and f["kept_idx"].tolist() == [0, 1, 3, 4, 6, 7]  # cluster 3 is not valid
    assert S.cluster_filter(lab, 3, rad, val, None, None, np.nan, np.nan)["n_filtered"] == 0
    assert S.cluster_filter(lab, 3, rad, val, None, None, -1.0, np.inf)["filtered"].tolist() == [1, 1, 0]


def test_remove_filter_points_keeps_order():
    from vtkcloudpoint_amd.datamodel import Point3D
    from vtkcloudpoint_amd.tools import Tools
    ids = [0, 3, 1, 2, 3, 0, 5, 2, 1, 4]
    data = [Point3D(float(i), 0.0, 0.0, c, True) for i, c in enumerate(ids)]
    same = list(data)
    Tools.removeFilterPointFromClustering(data, [])
    assert data == same
    held = data
    Tools.removeFilterPointFromClustering(data, [3, 2, 7])
    assert data is held  # in place, like the C#'s ref list
    assert [p.X for p in data] == [0.0, 2.0, 5.0, 6.0, 8.0, 9.0]
    assert [p.clusterId for p in data] == [0, 1, 0, 5, 1, 4]
    lab = np.array(ids, np.int32)
    f = S.cluster_filter(lab, 5, [1.0] * 5, [0, 1, 1, 0, 0], None, None, 0.0, np.inf)
    assert f["kept_idx"].tolist() == [int(p.X) for p in data]
