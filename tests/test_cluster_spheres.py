"""vcp_cluster_spheres without a GPU: the solve of csrc/spdsolve.hpp (run on the host through vcp_selftest_spd_solve)
against the replay of its operation sequence; the numpy restatement of the definition (tests/cluster_spheres_ref.py) on the
families whose centre and radius are exact, against the 60-digit minimiser with a plain numpy Gauss-Newton as the
yardstick, and on what the fit is for: caps seen from one side, reduced caps, a field at 1e8."""
import ctypes as C

import numpy as np
import pytest

import cluster_spheres_ref as R
from vtkcloudpoint_amd import _native as N

N_BITS = 300        # systems per family and dimension, bit for bit against the replay
# Gauss-Newton rounds of the accuracy tests: the smallest count at which the reported step has stopped shrinking on every
# case below.  The slowest (distance 5, noise 0.005, free radius, 3-D) contracts by about 40 a round from 3e-3 and is at
# its floor of a few 1e-16 in round 9 or 10; the fixed radius is there by round 7.  test_accuracy asserts the floor.
ROUNDS = 10
STEP_FLOOR = 1e-14
RT = R.R_TARGET


def one(x, fixed_radius=0.0, rounds=ROUNDS, w=None, **kw):
    """The restatement on one cluster: the dict with the leading axis dropped."""
    r = R.spheres(x, np.ones(len(x), np.int32), 1, w, fixed_radius, rounds, **kw)
    return {k: v[0] for k, v in r.items()}


# ---- the solve against the replay ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("family", R.SPD_FAMILIES)
def test_solve_equals_the_replay_bit_for_bit(family, dim):
    sys_ = R.spd_family(family, dim, N_BITS)
    assert len(sys_) >= 2
    oks = []
    for S, b in sys_:
        x, ok = N.selftest_spd_solve(S, b)
        rx, rok = R.spd_solve(S[np.triu_indices(dim)], b)
        # a NaN that a non-finite b leaves in x keeps the sign the arithmetic gave it: compared as NaN, not by payload
        assert ok == rok and R.same(R.canon(x), R.canon(rx)), (family, dim, S.tolist(), b.tolist())
        assert R.same(N.selftest_spd_solve(S[np.triu_indices(dim)], b)[0], x)      # the packed form is the same call
        oks.append(ok)
        if not ok:
            assert (R.bits(x) == 0x7FF8000000000000).all()
    if family in ("random", "graded", "scaled_up", "scaled_down", "identity", "nonfinite_rhs"):
        assert all(oks)
    if family in ("indefinite", "semidefinite", "zero", "nonfinite"):
        assert not any(oks)
    if family in ("random", "graded", "scaled_up"):
        for S, b in sys_[:50]:
            x, _ = N.selftest_spd_solve(S, b)
            assert np.abs(S @ x - b).max() <= 1e-9 * np.abs(b).max() * np.linalg.cond(S)
    if family == "identity":
        assert all(R.same(N.selftest_spd_solve(S, b)[0], b) for S, b in sys_[:20])
    if family == "nonfinite_rhs":
        assert not any(np.isfinite(N.selftest_spd_solve(S, b)[0]).all() for S, b in sys_)


def test_selftest_arguments():
    f = N.lib().vcp_selftest_spd_solve
    s, b, x, ok = np.eye(3)[np.triu_indices(3)].copy(), np.ones(3), np.full(3, -7.0), C.c_int(-7)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    for dim in (0, 1, 4, -2):
        assert f(C.c_int(dim), p(s), p(b), p(x), C.byref(ok)) == -1
    assert f(C.c_int(3), None, p(b), p(x), C.byref(ok)) == -1 and f(C.c_int(3), p(s), None, p(x), C.byref(ok)) == -1
    assert f(C.c_int(3), p(s), p(b), None, C.byref(ok)) == -1
    assert (x == -7.0).all() and ok.value == -7
    assert f(C.c_int(3), p(s), p(b), p(x), None) == 1 and R.same(x, np.ones(3))    # ok may be NULL


# ---- the families whose centre and radius are exact -------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [2, 3])
def test_lattice_points_give_centre_and_radius_exactly(dim):
    x, c, r = R.exact_family(dim)
    assert len(x) == (12 if dim == 2 else 24)
    assert (c.tolist(), r) == (([1000.25, -77.5], 0.625) if dim == 2 else ([3.5, 100.125, -9.0], 0.1875))
    for fixed in (0.0, r):
        for rounds in (0, 1, 3, ROUNDS):
            o = one(x, fixed, rounds)
            assert o["valid"] == 1 and o["counts"] == len(x)
            assert o["centre"].tolist() == c.tolist() and o["radius"] == r, (fixed, rounds)
            assert o["alg"].tolist() == c.tolist() + [r]
            assert o["rms"] <= 1e-15 * r and o["cap"] <= 1e-15 and o["step"] <= 1e-15 * r


@pytest.mark.parametrize("dim", [2, 3])
def test_a_member_at_the_centre_has_no_direction(dim):
    """rho == 0: nu = 0, and the member adds fl(w * 0) to the sums with nu in them (without the rule, 0 / 0 = NaN would
    reach every sum, also through a weight of 0).  With weight 0 the member changes nothing: centre and radius stay exact
    through every round.  With weight 1 it is an outlier at distance r: in the first round, where rho is exactly 0, the
    centre stays exact and the free radius becomes the mean of rho, r m / (m + 1)."""
    x, c, r = R.exact_family(dim)
    m = len(x)
    x1 = np.vstack([x, c])
    w0 = np.ones(m + 1, np.int32)
    w0[-1] = 0
    for fixed in (0.0, r):
        for rounds in (0, 1, ROUNDS):
            o = one(x1, fixed, rounds, w0)
            assert o["valid"] == 1 and o["counts"] == m
            assert o["centre"].tolist() == c.tolist() and o["radius"] == r
    o = one(x1, 0.0, 1)
    assert o["valid"] == 1 and o["counts"] == m + 1 and o["centre"].tolist() == c.tolist()
    assert abs(o["radius"] - r * m / (m + 1)) <= 4 * np.spacing(r)
    assert abs(o["rms"] - r * np.sqrt(m) / (m + 1)) <= 1e-14 * r           # the residuals: m of r / (m + 1), one of -r m / (m + 1)
    o = one(x1, r, 1)
    assert o["valid"] == 1 and o["centre"].tolist() == c.tolist() and o["radius"] == r
    assert abs(o["rms"] - r / np.sqrt(m + 1)) <= 1e-14 * r


def test_degenerate_clusters_are_invalid():
    nan = 0x7FF8000000000000
    cases = {
        "coincident": np.tile([1.5, -2.25, 4.0], (6, 1)),
        "collinear": np.outer(np.arange(6.0), [1.0, 2.0, -1.0]) + [0.5, 0.25, 8.0],
        "coplanar": np.array([[a, b, 3.0] for a in range(3) for b in range(3)], np.float64),
        "nan": np.vstack([R.exact_family(3)[0], [np.nan, 0, 0]]),
        "inf": np.vstack([R.exact_family(3)[0], [0, np.inf, 0]]),
    }
    for name, x in cases.items():
        for dim in (2, 3):
            if name == "coplanar" and dim == 2:
                continue                               # a grid in the plane: a fine circle fit
            for fixed in (0.0, 0.5):
                o = one(x[:, :dim], fixed, 3)
                assert o["valid"] == 0 and o["counts"] == len(x), (name, dim, fixed)
                for k in ("centre", "radius", "rms", "cap", "step", "alg"):
                    assert (R.bits(o[k]) == nan).all(), (name, dim, fixed, k)
    x, _, r = R.exact_family(3)
    for m in range(0, 6):                              # the limits of both forms: dim + 1 members free, dim fixed
        for dim in (2, 3):
            for fixed in (0.0, r):
                o = one(x[:m, :dim], fixed, 2)
                if m < (dim if fixed else dim + 1):
                    assert o["valid"] == 0 and o["counts"] == m and np.isnan(o["centre"]).all()


# ---- accuracy -----------------------------------------------------------------------------------------------------------
_ACC = {}


def _accuracy(family, dim, fixed):
    """Per case of the family: (the restatement's (centre, radius) errors against the 60-digit minimiser, the yardstick's,
    the last step); computed once."""
    key = (family, dim, fixed)
    if key not in _ACC:
        rows = []
        for x, _ in R.accuracy_cases(family, dim):
            o = one(x, RT if fixed else 0.0)
            assert o["valid"] == 1
            cm, rm = R.minimiser(x, o["centre"], RT if fixed else 0.0)
            pc, pr = R.plain_gn(x, RT if fixed else 0.0, ROUNDS)
            rows.append((R.error_to(cm, rm, o["centre"], o["radius"]), R.error_to(cm, rm, pc, pr), o["step"]))
        _ACC[key] = rows
    return _ACC[key]


@pytest.mark.parametrize("fixed", [False, True], ids=["free", "fixed"])
@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("family", R.ACC_FAMILIES)
def test_accuracy_against_the_60_digit_minimiser(family, dim, fixed):
    """The restatement's worst distance from the minimiser, centre and radius each, is at most twice that of a plain numpy
    Gauss-Newton (np.sum, np.linalg.solve) of the same rounds: the margin the Jacobi solver has over LAPACK."""
    rows = _accuracy(family, dim, fixed)
    ec, er = max(r[0][0] for r in rows), max(r[0][1] for r in rows)
    yc, yr = max(r[1][0] for r in rows), max(r[1][1] for r in rows)
    st = max(r[2] for r in rows)
    print("\n%s dim %d %s: centre %.2e (numpy %.2e), radius %.2e (numpy %.2e), last step %.1e"
          % (family, dim, "fixed" if fixed else "free", ec, yc, er, yr, st))
    assert st <= STEP_FLOOR                            # ROUNDS is past the last shrinking round
    assert ec <= 2 * yc and er <= 2 * yr


def test_the_step_has_stopped_shrinking_at_ROUNDS_and_not_two_rounds_before():
    """ROUNDS is the smallest count that serves every case: two rounds earlier the slowest case still moves."""
    worst_before, worst_at = 0.0, 0.0
    for dim in (2, 3):
        for x, _ in R.accuracy_cases("near", dim):
            tr = []
            one(x, 0.0, ROUNDS, trace=tr)
            worst_before = max(worst_before, float(tr[ROUNDS - 3][0]))
            worst_at = max(worst_at, float(tr[ROUNDS - 1][0]))
    print("\nstep in round %d: %.1e; in round %d: %.1e" % (ROUNDS - 2, worst_before, ROUNDS, worst_at))
    assert worst_before > STEP_FLOOR >= worst_at


# ---- what the fit is for -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [2, 3])
def test_the_mean_sits_in_front_of_the_centre_and_the_fit_does_not(dim):
    for x, c in R.accuracy_cases("clean", dim):
        o = one(x)
        em, ef = np.linalg.norm(x.mean(0) - c), np.linalg.norm(o["centre"] - c)
        assert em > RT / 2 and ef <= em / 100 and abs(o["radius"] - RT) <= 1e-4 * RT
        assert np.dot(x.mean(0) - c, -c) > 0           # towards the instrument
        assert ef <= 1e-4 * RT
        assert 0.55 < o["cap"] < 0.85                  # 2/3 for the sphere's cap, pi/4 for the rim's arc


def test_reduced_caps_fixed_beats_free_beats_algebraic():
    """The inner 60 % of the cap with a range noise of 0.0005 (R / 145), 12 seeded spheres: root-mean-square distance to
    the true centre of the fixed-radius fit < of the free fit < of the algebraic start."""
    rng = np.random.default_rng(5)
    e = {"fixed": [], "free": [], "alg": []}
    for _ in range(12):
        v = rng.normal(size=3)
        c = rng.uniform(5, 20) * v / np.linalg.norm(v)
        x = R.cap_points(rng, c, 300, inner=0.6, noise=0.0005)
        free, fixed = one(x), one(x, RT)
        e["fixed"].append(np.linalg.norm(fixed["centre"] - c))
        e["free"].append(np.linalg.norm(free["centre"] - c))
        e["alg"].append(np.linalg.norm(free["alg"][:3] - c))
    rms = {k: float(np.sqrt(np.mean(np.square(v)))) / RT for k, v in e.items()}
    print("\ninner 60 %%: fixed %.4f R, free %.4f R, algebraic %.4f R" % (rms["fixed"], rms["free"], rms["alg"]))
    assert rms["fixed"] < rms["free"] < rms["alg"]


def test_a_field_at_1e8_keeps_its_digits_in_the_centred_form_only():
    """The caps shifted by 1e8 on every axis (the rounded coordinates are the input).  The centre can be no better than
    the spacing of doubles there (1.5e-8) in any form; the radius is a difference and can.  The definition's radius stays
    within twice the yardstick's error; the variant that forms e from raw coordinates and fl(m + u) loses it."""
    worst = {"def": 0.0, "raw": 0.0, "numpy": 0.0, "def_c": 0.0, "numpy_c": 0.0}
    for x, _ in R.accuracy_cases("noisy", 3):
        x = x + 1e8
        o, q = one(x), one(x, raw=True)
        cm, rm = R.minimiser(x, o["centre"])
        pc, pr = R.plain_gn(x, 0.0, ROUNDS)
        for name, (cc, rr) in (("def", (o["centre"], o["radius"])), ("raw", (q["centre"], q["radius"])), ("numpy", (pc, pr))):
            ec, er = R.error_to(cm, rm, cc, rr)
            worst[name] = max(worst[name], er)
            if name + "_c" in worst:
                worst[name + "_c"] = max(worst[name + "_c"], ec)
    print("\nat 1e8: radius error %.2e (numpy %.2e), from raw coordinates %.2e; centre %.2e (numpy %.2e)"
          % (worst["def"], worst["numpy"], worst["raw"], worst["def_c"], worst["numpy_c"]))
    assert worst["def"] <= 2 * worst["numpy"] and worst["def_c"] <= 2 * worst["numpy_c"]
    assert worst["raw"] > 2 * worst["numpy"] and worst["raw"] > 100 * worst["def"]
