"""The exact references of circle_ref.py on hand cases and against each other, and the CPU oracle's circle, hull and
rectangle held to them on every finite family of shape_families.py.  The figures are printed before they are asserted
(pytest -s shows them): twice shape_families.BOUNDS, the worst figures recorded from this very measurement."""
from fractions import Fraction as F

import numpy as np
import pytest

import circle_ref as CR
import shape_families as SF
import shapes_ref as S


def _mec(pts):
    return CR.min_circle(CR.convex_hull(CR.fractions_of(np.asarray(pts, float))))


def test_references_on_hand_cases():
    sq = [[0, 0], [2, 0], [2, 2], [0, 2], [1, 1], [2, 2], [1, 0], [0.5, 2]]
    H = CR.convex_hull(CR.fractions_of(sq))
    assert H == [(F(0), F(0)), (F(2), F(0)), (F(2), F(2)), (F(0), F(2))]  # duplicates merged, edge points left out
    assert _mec(sq) == (F(1), F(1), F(2))
    assert _mec([[0, 0], [4, 0], [0, 3]]) == (F(2), F(3, 2), F(25, 4))           # 3-4-5: the hypotenuse is a diameter
    assert _mec([[0, 0], [4, 0], [2, 0.25], [1, 0.125]]) == (F(2), F(0), F(4))   # obtuse: the long side is a diameter
    assert _mec([[0, 0], [4, 0], [2, 3]]) == (F(2), F(5, 6), F(169, 36))         # acute: the circumcircle
    assert _mec(SF.lattice_circle(50)) == (F(0), F(0), F(50))
    assert _mec(SF.lattice_circle(50) * 0.5 + [1000.5, 7]) == (F(2001, 2), F(7), F(25, 2))
    assert _mec([[3, 3]] * 4) == (F(3), F(3), F(0))
    assert _mec([[0, 0], [1, 2], [2, 4], [3, 6]]) == (F(3, 2), F(3), F(45, 4))
    assert len(CR.convex_hull(CR.fractions_of([[0, 0], [1, 2], [2, 4], [3, 6]]))) == 2
    # the predicates
    P = CR.fractions_of(sq)
    assert CR.max_dist2(P, 1.0, 1.0) == 2 and CR.max_dist2(P, 0.0, 0.0) == 8
    box = np.array([[0, 0], [2, 0], [2, 2], [0, 2]], float)
    assert CR.outside_rectangle(P, box) == 0.0
    assert CR.outside_rectangle(CR.fractions_of([[1, 1]]), box) == -1.0
    assert CR.outside_rectangle(CR.fractions_of([[1, 2.5], [1, 1]]), box) == 0.5
    assert CR.outside_rectangle(CR.fractions_of([[-0.25, 1]]), box) == 0.25
    seg = np.array([[0, 0], [4, 0], [4, 0], [0, 0]], float)  # the rectangle of a line
    assert CR.outside_rectangle(CR.fractions_of([[1, 0], [4, 0]]), seg) == 0.0
    assert CR.outside_rectangle(CR.fractions_of([[1, -0.5]]), seg) == 0.5
    assert CR.beyond(F(25, 4), 2.5) == 0.0 and CR.beyond(F(9), 2.0) == 1.0
    tiny = CR.beyond(F(1) + F(1, 2 ** 60), 1.0)
    assert abs(tiny - 2.0 ** -61) < 2.0 ** -100


@pytest.mark.parametrize("name", sorted(SF.FINITE))
def test_search_and_welzl_agree(name):
    n = 0
    for e in SF.exact(SF.family(name)):
        if e is not None and len(e["H"]) <= CR.SEARCH_MAX:
            assert CR.min_circle_welzl(e["H"], seed=n) == (e["cx"], e["cy"], e["r2"])
            n += 1
    assert n > 0 or name == "long_hull"
    if name == "long_hull":  # above SEARCH_MAX only Welzl runs: two shuffles of it agree, and the circle holds the hull
        for e in SF.exact(SF.family(name)):
            assert CR.min_circle_welzl(e["H"], seed=5) == (e["cx"], e["cy"], e["r2"])
            assert CR.max_dist2(e["H"], e["cx"], e["cy"]) == e["r2"]


@pytest.mark.parametrize("name", sorted(SF.FINITE))
def test_oracle_against_exact_geometry(oracle, name):
    c = SF.family(name)
    res = SF.oracle_shapes(oracle, c)
    w = SF.figures(c, res)
    fired = int((res["inserted"] > 0).sum())
    lit = oracle.get_circles(c["xy"], c["labels"], c["K"], c["order"], literal=True)
    covered = int(((lit["valid"] == 1) & (lit["hull_n"] > 2) & (lit["radius"] == 0)).sum())  # the C# found no circle
    print("%-15s clusters %3d  beyond %.3g  |r - r_exact| %.3g  |c - c_exact| %.3g  outside the rectangle %.3g (%d)"
          "  insertion fired on %d (most insertions %d), covering on %d"
          % (name, w["checked"], w["beyond"], w["r"], w["c"], w["rect"], w["rect_checked"], fired, res["inserted"].max(),
             covered))
    SF.check_bounds(name, w)
    if name in SF.NEVER_FIRES:
        assert fired == 0
    if name in SF.MUST_FIRE:
        assert fired > 0
    n_hull = 0
    for k, kind in enumerate(c["kinds"]):
        if res["valid"][k] == 1 and kind not in SF.HULL_EXEMPT:
            assert SF.hull_is_exact(c, k, res["hull_xy"][k]), (k, kind)
            assert res["inserted"][k] == 0, (k, kind)  # an exact hull leaves the rule nothing to add
            n_hull += 1
    assert n_hull > 0
    assert np.array_equal(lit["valid"], res["valid"]) and np.array_equal(lit["hull_n"], res["hull_n"])
    if name != "long_hull":  # (its search is the slow one, and get_circles is the same code cluster by cluster)
        rep = oracle.get_circles(c["xy"], c["labels"], c["K"], c["order"])
        for key in ("centers", "radius", "valid", "hull_n", "inserted"):
            assert np.array_equal(rep[key], res[key]), key
    if name in SF.NEVER_FIRES:  # where no rule acts the result is the reference's, bit for bit
        same = ~((lit["valid"] == 1) & (lit["hull_n"] > 2) & (lit["radius"] == 0))
        for key in ("centers", "radius"):
            assert np.array_equal(lit[key][same], res[key][same]), key


def test_seven_point_cluster(oracle):
    """The reference's own result is pinned (hull of 5, a circle that leaves the seventh point 1.105 from its centre),
    and beside it the repaired one."""
    pts = SF.verbatim7()
    lit = oracle.min_circle_ex(pts, literal=True)
    assert len(lit["hull"]) == 5 and lit["inserted"] == 0
    assert lit["radius"] == 0.855438099596984
    assert lit["center"].tolist() == [0.4683115402080905, -1.3274474883893967]
    assert float(np.hypot(*(pts[6] - lit["center"]))) == pytest.approx(1.1054554311943505, rel=1e-15)
    P = CR.fractions_of(pts)
    H = CR.convex_hull(P)
    cx, cy, r2 = CR.min_circle(H)
    r_exact = CR._sqrt(r2)
    assert r_exact == pytest.approx(0.98045, abs=1e-5)
    assert CR.max_dist2(P, *lit["center"]) > F(1.1) ** 2 > r2
    rep = oracle.min_circle_ex(pts)
    assert rep["inserted"] == 1 and np.array_equal(rep["hull"], lit["hull"])  # the hull output stays the wrap's
    u = SF.unit(pts, r_exact)
    b = SF.BOUNDS["near_collinear"]
    assert abs(CR.beyond(r2, rep["radius"])) <= 2 * b["r"] * u
    assert CR.beyond(CR.max_dist2(P, *rep["center"]), rep["radius"]) <= 2 * b["beyond"] * u
    # the rectangle: on the truncated hull alone it leaves members outside; over the members it holds them
    short = S.rectangle(lit["hull"])
    full = S.rectangle(rep["hull"], pts)
    assert short["edge"] >= 0 and full["edge"] >= 0
    ur = SF.unit(pts, float(full["len"].max()))
    assert CR.outside_rectangle(P, short["xy"]) > 0.1
    assert CR.outside_rectangle(P, full["xy"]) <= 2 * b["rect"] * ur
    # get_circles goes through the same code
    g = oracle.get_circles(pts, np.ones(7, np.int32), 1)
    assert g["radius"][0] == rep["radius"] and g["centers"][0].tolist() == rep["center"].tolist() and g["inserted"][0] == 1
    gl = oracle.get_circles(pts, np.ones(7, np.int32), 1, literal=True)
    assert gl["radius"][0] == lit["radius"] and gl["hull_n"][0] == 5
