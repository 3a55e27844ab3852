"""vcp_cluster_moments without a GPU: the eigen-solver of csrc/symeig.hpp (run on the host through vcp_selftest_sym_eig)
against the replay of its operation sequence and against 60-digit eigenvalues with LAPACK as the yardstick; the numpy
restatement of the definition (tests/cluster_moments_ref.py) against the exact rational covariance and the bound of
DESIGN.md section 33; the family on which the sums are exact."""
import ctypes as C
from fractions import Fraction

import mpmath
import numpy as np
import pytest

import centroid_ref as CR
import cluster_moments_ref as R
from vtkcloudpoint_amd import _native as N

N_BITS = 300        # matrices per family and dimension, bit for bit against the replay
N_ACC = 500         # matrices per family and dimension in the accuracy measures


# ---- the solver against the replay ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("family", R.EIG_FAMILIES)
def test_solver_equals_the_replay_bit_for_bit(family, dim):
    mats = R.eig_family(family, dim, N_BITS)
    assert len(mats) >= 2
    sweeps = []
    for S in mats:
        ev, vec, sw = N.selftest_sym_eig(S)
        rv, rvec, rsw = R.sym_eig(S)
        assert sw == rsw and R.same(ev, R.canon(rv)) and R.same(vec, R.canon(rvec)), (family, dim, S.tolist())
        assert R.same(N.selftest_sym_eig(R.pack(S))[0], ev)                  # the packed form is the same call
        sweeps.append(sw)
        if family == "nonfinite":
            assert np.isnan(ev).all() and np.isnan(vec).all() and sw == 0
            assert (R.bits(ev) == 0x7FF8000000000000).all() and (R.bits(vec) == 0x7FF8000000000000).all()
            continue
        assert np.all(ev[:-1] >= ev[1:])                                     # descending
        big = np.abs(vec).argmax(axis=1)
        assert all(vec[j, big[j]] > 0 for j in range(dim))                   # the sign rule
        if family == "zero":
            assert R.same(ev, np.zeros(dim)) and R.same(vec, np.eye(dim)) and sw == 0
        if family == "diagonal":
            assert sw == 0 and sorted(ev.tolist()) == sorted(np.diag(S).tolist()) and set(np.abs(vec).ravel()) == {0.0, 1.0}
    assert max(sweeps) < R.SWEEPS                                            # the stop at exact zeros was reached
    if dim == 2:
        assert max(sweeps) <= 1                                              # a 2x2 needs one rotation
    print("\n%s dim %d: sweeps %d..%d" % (family, dim, min(sweeps), max(sweeps)))


def test_equal_eigenvalues_keep_their_diagonal_order_and_determinant_may_be_minus_one():
    ev, vec, _ = N.selftest_sym_eig(np.diag([2.0, 5.0, 2.0]))
    assert ev.tolist() == [5.0, 2.0, 2.0] and R.same(vec, np.array([[0.0, 1, 0], [1, 0, 0], [0, 0, 1]]))
    assert np.linalg.det(vec) == -1.0
    ev, vec, _ = N.selftest_sym_eig(np.array([[-1.0, 0.0], [0.0, -3.0]]))      # negative eigenvalues: as computed
    assert ev.tolist() == [-1.0, -3.0]


def test_selftest_arguments():
    f = N.lib().vcp_selftest_sym_eig
    s, ev, vec = np.zeros(6), np.full(3, -7.0), np.full(9, -7.0)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    for dim in (0, 1, 4, -2):
        assert f(C.c_int(dim), p(s), p(ev), p(vec), None) == -1
    assert f(C.c_int(3), None, p(ev), p(vec), None) == -1 and f(C.c_int(3), p(s), None, p(vec), None) == -1
    assert f(C.c_int(3), p(s), p(ev), None, None) == -1
    assert (ev == -7.0).all() and (vec == -7.0).all()
    assert f(C.c_int(3), p(s), p(ev), p(vec), None) == 1 and R.same(ev, np.zeros(3))   # sweeps may be NULL


# ---- the solver's accuracy -----------------------------------------------------------------------------------------------------
def _measures(S, ev, vec):
    """(eigenvalue error, residual) in units of u |S|_F and |V V^T - I|_max in units of u, in 60-digit arithmetic;
    ev descending, eigenvector j = vec[j]."""
    D = len(ev)
    with mpmath.workdps(60):
        M = mpmath.matrix(S.tolist())
        u = mpmath.mpf(2) ** -53
        nrm = mpmath.sqrt(sum(M[i, j] ** 2 for i in range(D) for j in range(D)))
        exact = sorted(mpmath.eigsy(M, eigvals_only=True), reverse=True)
        e_val = max(abs(mpmath.mpf(float(ev[j])) - exact[j]) for j in range(D)) / (u * nrm)
        Vm = mpmath.matrix(vec.tolist())
        res = 0
        for j in range(D):
            v = Vm[j, :].T
            r = M * v - mpmath.mpf(float(ev[j])) * v
            res = max(res, mpmath.sqrt(sum(x * x for x in r)))
        G = Vm * Vm.T - mpmath.eye(D)
        orth = max(abs(G[i, j]) for i in range(D) for j in range(D)) / u
        return float(e_val), float(res / (u * nrm)), float(orth)


@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("family", R.EIG_ACCURACY)
def test_solver_accuracy_against_60_digits_with_lapack_as_the_yardstick(family, dim):
    """Per family the worst eigenvalue error, residual |S v - lambda v| and |V V^T - I| of the Jacobi solve may be at most
    twice LAPACK's (numpy.linalg.eigh) on the same matrices.  The figures are printed; DESIGN.md section 33 records them."""
    worst_j, worst_l = np.zeros(3), np.zeros(3)
    for S in R.eig_family_in_range(family, dim, N_ACC):
        ev, vec, _ = N.selftest_sym_eig(S)
        worst_j = np.maximum(worst_j, _measures(S, ev, vec))
        lw, lv = np.linalg.eigh(S)
        worst_l = np.maximum(worst_l, _measures(S, lw[::-1], lv[:, ::-1].T))
    print("\n%s dim %d: jacobi (eval %.2f, resid %.2f, orth %.2f) u; lapack (eval %.2f, resid %.2f, orth %.2f) u"
          % ((family, dim) + tuple(worst_j) + tuple(worst_l)))
    assert np.all(worst_j <= 2.0 * worst_l), (family, dim, worst_j.tolist(), worst_l.tolist())


# ---- the restatement against exact arithmetic ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def labels():
    return CR.case_labels()


@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("family", CR.INEXACT)
def test_restatement_within_the_bound_of_the_exact_covariance(labels, family, dim):
    K = max(CR.SLOTS)
    pts = CR.case_values(family, labels, dim)
    r = R.moments(pts, labels, K)
    ex = R.exact_cov(pts, labels, K)
    bnd = R.cov_bound(pts, labels, K, ex=ex)
    raw = R.raw_moment_cov(pts, labels, K)
    pairs = [(a, b) for a in range(dim) for b in range(a, dim)]
    worst, raw_breaks = Fraction(0), []
    for k in range(K):
        if ex[k] is None:
            assert r["counts"][k] == 0 and np.isnan(r["cov"][k]).all()
            continue
        W, _, Cx = ex[k]
        assert W == r["counts"][k]
        for j, ab in enumerate(pairs):
            err = abs(Fraction(float(r["cov"][k, j])) - Cx[ab])
            assert err <= bnd[k][ab], (family, dim, k, ab, float(err), float(bnd[k][ab]))
            if bnd[k][ab] > 0:
                worst = max(worst, err / bnd[k][ab])
        if W >= 63:
            raw_breaks.append(any(abs(Fraction(float(raw[k, j])) - Cx[ab]) > bnd[k][ab] for j, ab in enumerate(pairs)))
    print("\n%s dim %d: worst error / bound %.3g" % (family, dim, float(worst)))
    assert len(raw_breaks) == len([s for s in CR.SIZES if s >= 63])
    if family == "offset":      # the bound is not vacuous: the raw-moment form breaks it on every such cluster
        assert all(raw_breaks)


def test_sums_are_exact_on_the_grid_family():
    """Multiples of 2^-10 below 100 in clusters of 2^j points, j <= 6: the mean is a multiple of 2^-(10 + j), the
    differences and their products are exact, and so is every partial sum (34 + 3 j bits at most): S equals the rational
    sum, and the mean the rational mean."""
    sizes = [1, 2, 4, 8, 16, 32, 64]
    K = len(sizes)
    rng = np.random.default_rng(3)
    lab = np.repeat(np.arange(1, K + 1, dtype=np.int32), sizes)
    lab = np.concatenate([lab, np.zeros(50, np.int32)])[rng.permutation(len(lab) + 50)]
    for dim in (2, 3):
        pts = CR.case_values("grid", lab, dim)
        r = R.moments(pts, lab, K)
        ex = R.exact_cov(pts, lab, K)
        for k in range(K):
            W, mu, Cx = ex[k]
            assert W == sizes[k] and [Fraction(float(x)) for x in r["mean"][k]] == mu
            want = [Cx[(a, b)] * W for a in range(dim) for b in range(a, dim)]
            assert [Fraction(float(x)) for x in r["S"][k]] == want
