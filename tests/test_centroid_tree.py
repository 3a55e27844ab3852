"""The replay of the centroid kernels' summation tree (tests/centroid_ref.py) on the CPU: it meets its derived bound
against the exact means, it is exact where every partial sum is, it agrees with the oracle's sequential sums within
the sum of both a-priori bounds, every way of getting the tree wrong changes its bits on the shared input set (so the
bit-for-bit GPU test, tests/test_centroid_replay_gpu.py, would notice), and the inputs on which the tree and a
sequential sum differ in kind are written down as assertions."""
from fractions import Fraction

import numpy as np
import pytest

import centroid_ref as R

CH = R.CH
MULTI = [k for k, s in zip(R.SLOTS, R.SIZES) if s > CH]          # labels whose cluster spans more than one chunk
THREE = [k for k, s in zip(R.SLOTS, R.SIZES) if s > 2 * CH]      # ... three chunks or more
K = 257


@pytest.fixture(scope="module")
def cases():
    return {f: R.case(f) for f in R.FAMILIES}


def _within(c, means, bounds, k, a):
    return abs(Fraction(float(c)) - means[k][a]) <= bounds[k][a]


def test_input_set_is_what_it_claims():
    lab = R.case_labels()
    cnt = np.bincount(lab, minlength=K + 1)
    assert len(lab) == R.N_POINTS and [int(cnt[s]) for s in R.SLOTS] == R.SIZES
    assert cnt[1:].sum() == sum(R.SIZES) and cnt[1] == 0 and cnt[255] == cnt[256] == cnt[257] == 0
    # scattered: the members of the largest cluster are not a contiguous run of the array
    ix = np.flatnonzero(lab == R.SLOTS[-1])
    assert ix[-1] - ix[0] > 4 * len(ix) and len(MULTI) == 5 and len(THREE) == 2


def test_replay_within_bound_of_exact_mean(cases):
    worst = 0.0
    for fam, (xyz, motor, lab) in cases.items():
        vals = np.concatenate([xyz, motor], 1)
        c3, c2, cnt = R.tree_centroids(xyz, motor, lab, K)
        c = np.concatenate([c3, c2], 1)
        means, bounds = R.exact_means(vals, lab, K), R.bound(vals, lab, K)
        for k in range(K):
            if means[k] is None:
                assert cnt[k] == 0 and np.isnan(c[k]).all()
                continue
            for a in range(5):
                assert _within(c[k, a], means, bounds, k, a), (fam, k + 1, a)
                if bounds[k][a]:
                    worst = max(worst, float(abs(Fraction(float(c[k, a])) - means[k][a]) / bounds[k][a]))
        if fam == "grid":  # every partial sum is a multiple of 2^-10 below 2^53 units: the only rounding is the division
            for k in range(K):
                if means[k] is not None:
                    want = [float(m) for m in means[k]]  # Fraction -> float rounds correctly
                    assert c[k].tolist() == want, (k + 1)
    print("replay error / a-priori bound, worst over the input set: %.3g" % worst)
    assert worst < 1.0


def test_replay_exact_on_small_integers():
    rng = np.random.default_rng(3)
    n = 3 * CH + 5
    xyz = rng.integers(-1000, 1000, (n, 3)).astype(np.float64)
    motor = rng.integers(-9, 9, (n, 2)).astype(np.float64)
    lab = rng.integers(0, 3, n).astype(np.int32)
    lab[: 2 * CH + 3] = 2
    c3, c2, cnt = R.tree_centroids(xyz, motor, lab, 2)
    means = R.exact_means(np.concatenate([xyz, motor], 1), lab, 2)
    assert cnt[1] > 2 * CH
    for k in range(2):
        assert np.concatenate([c3[k], c2[k]]).tolist() == [float(m) for m in means[k]]


def test_exact_sum_equals_a_plain_fraction_sum():
    """exact_means adds split mantissas per exponent for speed; the same sums from fractions.Fraction one by one."""
    rng = np.random.default_rng(8)
    x = np.concatenate([rng.uniform(-100, 100, 200), 10.0 ** rng.uniform(-300, 300, 200) * rng.choice([-1, 1], 200),
                        np.array([R.SUB, -3 * R.SUB, 2.2250738585072014e-308, -1e-310, 0.0, -0.0, R.BIG, -R.BIG, 1.0])])
    w = rng.integers(0, 2 ** 20, len(x))
    assert R._exact_int_sum(x) == sum(Fraction(float(v)) for v in x)
    assert R._exact_int_sum(x, w) == sum(Fraction(float(v)) * int(k) for v, k in zip(x, w))
    lab = rng.integers(0, 4, len(x)).astype(np.int32)
    m = R.exact_means(x[:, None], lab, 3, w)
    for k in (1, 2, 3):
        sel = lab == k
        assert m[k - 1][0] == sum(Fraction(float(v)) * int(c) for v, c in zip(x[sel], w[sel])) / int(w[sel].sum())


def test_weighted_replay_within_bound_of_exact_mean(cases):
    for fam, (xyz, _, lab) in cases.items():
        grp, Kc = R.compact(lab)
        cid, pts = R.case_weights(grp)
        for ignore in (False, True):
            for c in (cid, None):
                w = R.weights_of(grp, c, pts, ignore)
                c3, inside = R.tree_centroids_weighted(xyz, grp, c, pts, Kc, ignore)
                assert inside.tolist() == [int(w[grp == k].sum()) for k in range(1, Kc + 1)] and inside.max() < 2 ** 31
                means, bounds = R.exact_means(xyz, grp, Kc, w), R.bound(xyz, grp, Kc, w)
                for k in range(Kc):
                    for a in range(3):
                        assert _within(c3[k, a], means, bounds, k, a), (fam, ignore, c is None, k + 1, a)
                if not ignore:
                    assert inside.max() > 2 ** 27  # the heavy cluster is there


def test_replay_against_oracle(cases, oracle):
    """Two rounded sums of the same members: they differ by at most the sum of their a-priori bounds (the tree's, and
    gamma_(n-1) sum|x| / n for the sequential sum); everything integral is equal."""
    for fam, (xyz, motor, lab) in cases.items():
        vals = np.concatenate([xyz, motor], 1)
        for Kc in (255, 256, 257):
            t3, t2, tc = R.tree_centroids(xyz, motor, lab, Kc)
            o3, o2, oc = oracle.centroids(xyz, motor, lab, Kc)
            assert np.array_equal(tc, oc)
            if Kc != K:
                assert np.array_equal(t3, R.tree_centroids(xyz, motor, lab, K)[0][:Kc], equal_nan=True)
                continue
            bt, bs = R.bound(vals, lab, Kc), R.bound(vals, lab, Kc, sequential=True)
            t, o = np.concatenate([t3, t2], 1), np.concatenate([o3, o2], 1)
            for k in range(Kc):
                if bt[k] is None:
                    assert np.isnan(t[k]).all() and np.isnan(o[k]).all()
                    continue
                for a in range(5):
                    assert abs(Fraction(float(t[k, a])) - Fraction(float(o[k, a]))) <= bt[k][a] + bs[k][a], (fam, k + 1, a)
        # refresh_by_dictionary: labels, K' and counts equal; the oracle appends merged members, the kernel re-sorts them
        m = R.case_dictionary(K)
        tl, tk, t3, t2, tc = R.tree_refresh(xyz, motor, lab, K, m)
        ol, ok, o3, o2, oc = oracle.refresh_by_dictionary(xyz, motor, lab, K, m)
        assert tk == ok == len(R.SLOTS) - 3 and np.array_equal(tl, ol) and np.array_equal(tc, oc)
        assert tc.tolist() == [64, 65, 255, 256, 257, CH, CH, CH + 64, 2 * CH + 1, 2 * CH, 2 * CH + 1, 3 * CH + 17]
        bt, bs = R.bound(vals, tl, tk), R.bound(vals, tl, tk, sequential=True)
        t, o = np.concatenate([t3, t2], 1), np.concatenate([o3, o2], 1)
        for k in range(tk):
            for a in range(5):
                assert abs(Fraction(float(t[k, a])) - Fraction(float(o[k, a]))) <= bt[k][a] + bs[k][a], (fam, k + 1, a)
        # getFixedPtsCentroid
        grp, Kc = R.compact(lab)
        cid, pts = R.case_weights(grp)
        for ignore in (False, True):
            for c in (cid, None):
                w = R.weights_of(grp, c, pts, ignore)
                t3, ti = R.tree_centroids_weighted(xyz, grp, c, pts, Kc, ignore)
                o3, oi = oracle.fixed_centroids(xyz, grp, c, pts, Kc, ignore)
                assert np.array_equal(ti, oi)
                bt, bs = R.bound(xyz, grp, Kc, w), R.bound(xyz, grp, Kc, w, sequential=True)
                for k in range(Kc):
                    for a in range(3):
                        assert abs(Fraction(float(t3[k, a])) - Fraction(float(o3[k, a]))) <= bt[k][a] + bs[k][a]


def _differs(a, b):
    """per label: any bit of the row differs (NaN rows of empty labels compare equal)"""
    return ~((a == b) | (np.isnan(a) & np.isnan(b))).all(axis=1)


@pytest.mark.parametrize("knob", sorted(R.KNOBS))
def test_every_knob_changes_bits(cases, knob):
    """A replay with one property of the kernel's order broken differs in bits from the true replay, on every family
    whose sums round.  This is the proof, without a GPU, that the bit-for-bit GPU comparison notices that defect."""
    hits = {}
    for fam in R.INEXACT:
        xyz, motor, lab = cases[fam]
        t3, t2, _ = R.tree_centroids(xyz, motor, lab, K)
        m3, m2, _ = R.tree_centroids(xyz, motor, lab, K, **R.KNOBS[knob])
        diff = _differs(np.concatenate([t3, t2], 1), np.concatenate([m3, m2], 1))
        hits[fam] = {int(k) + 1 for k in np.flatnonzero(diff)}
        assert hits[fam], (knob, fam)
    # per cluster the requirement is on the input set as a whole: some family tells the mutant apart.  (On the 1e8 family
    # a cluster's sum has an ulp thousands of times the members', so many reorderings round to the same sum there.)
    union = set().union(*hits.values())
    if knob == "chunk_reversed":
        # a + b == b + a: two chunks reversed are the same sum, bit for bit, in every family; three chunks or more tell
        assert union == set(THREE), (knob, hits)
    elif knob.startswith("chunk_len"):
        assert set(MULTI) <= union, (knob, hits)
        assert not union & {k for k, s in zip(R.SLOTS, R.SIZES) if s < CH - 1}   # one chunk either way
    elif knob == "members_descending":
        assert set(MULTI) <= union, (knob, hits)
        # the weighted kernel shares the fold; its replay shares the code, one family is enough
    xyz, _, lab = cases["uniform"]
    grp, Kc = R.compact(lab)
    cid, pts = R.case_weights(grp)
    a = R.tree_centroids_weighted(xyz, grp, cid, pts, Kc, False)[0]
    b = R.tree_centroids_weighted(xyz, grp, cid, pts, Kc, False, **R.KNOBS[knob])[0]
    assert _differs(a, b).any()


def test_grid_family_hides_every_knob(cases):
    """The counterpart: where all partial sums are exact no order can be told apart, which is why the benchmark clouds
    (multiples of 2^-10) never exercised the order."""
    xyz, motor, lab = cases["grid"]
    t3, t2, _ = R.tree_centroids(xyz, motor, lab, K)
    for knob, kw in R.KNOBS.items():
        m3, m2, _ = R.tree_centroids(xyz, motor, lab, K, **kw)
        assert np.array_equal(t3, m3, equal_nan=True) and np.array_equal(t2, m2, equal_nan=True), knob


# ---- differences in kind --------------------------------------------------------------------------------------------
def _both(oracle, name):
    xyz, motor, lab = R.kind_arrays(R.kind_cases()[name])
    t3, t2, tc = R.tree_centroids(xyz, motor, lab, 1)
    o3, o2, oc = oracle.centroids(xyz, motor, lab, 1)
    assert np.array_equal(tc, oc)
    assert (t3 == t3[0, 0]).all() | np.isnan(t3).all() and (o3 == o3[0, 0]).all() | np.isnan(o3).all()
    assert np.array_equal(t3[0, :2], t2[0], equal_nan=True) and np.array_equal(o3[0, :2], o2[0], equal_nan=True)
    return float(t3[0, 0]), float(o3[0, 0])


def test_kind_overflow(oracle):
    # the true mean is 0 in both; whoever adds two 1e308 of one sign first overflows
    t, o = _both(oracle, "overflow_sequential_only")
    assert t == 0.0 and o == np.inf            # tree: (1e308 - 1e308) + (1e308 - 1e308); C#: 1e308 + 1e308 = inf
    t, o = _both(oracle, "overflow_tree_only")
    assert np.isnan(t) and o == 0.0            # tree: (1e308 + 1e308) + (-1e308 - 1e308) = inf - inf; C#: alternates


def test_kind_negative_zero(oracle):
    t, o = _both(oracle, "negative_zero")
    assert t == 0.0 and o == 0.0 and not np.signbit(t) and not np.signbit(o)   # both sums start at +0.0


def test_kind_subnormal(oracle):
    """Sums of subnormals are exact; the division rounds to the 2^-1074 grid, which the relative bound does not
    cover: the absolute term 2^-1075 does."""
    t, o = _both(oracle, "subnormal")
    assert t == o == 2 * R.SUB                 # 5 units / 3 = 1.67 units -> 2 units
    col = R.kind_cases()["subnormal"][:, None]
    lab = np.ones(3, np.int32)
    mean, b = R.exact_means(col, lab, 1)[0][0], R.bound(col, lab, 1)[0][0]
    err = abs(Fraction(t) - mean)
    assert err > b and err <= Fraction(1, 2 ** 1075)


def test_kind_non_finite(oracle):
    t, o = _both(oracle, "inf_member")
    assert t == o == np.inf
    t, o = _both(oracle, "inf_both_signs")
    assert np.isnan(t) and np.isnan(o)
    t, o = _both(oracle, "nan_member")
    assert np.isnan(t) and np.isnan(o)         # payloads are not pinned
