"""vcp_match_unique without a GPU: the two entry points exist in the header, the Python binding, the library and the C#
imports with matching arity; the numpy restatement of the definition (tests/match_unique_ref.py) on hand-checked cases; the
two properties that tie it to vcp_match (P1, P2 of DESIGN.md section 15) on random inputs; the rounds of locally dominant
pairs against the sequential walk."""
import numpy as np

import match_unique_ref as R
from test_abi import _csharp_imports, _header_prototypes

NAMES = ["vcp_match_unique", "vcp_match_unique_dev"]
I4 = np.eye(4)


def test_the_two_symbols_everywhere_with_matching_arity():
    from vtkcloudpoint_amd import _native
    lib = _native.lib()
    protos = _header_prototypes()
    cs = {name: classes for _, name, classes in _csharp_imports()}
    for nm in NAMES:
        assert hasattr(lib, nm), nm
        assert nm in protos and nm in _native.SYMBOLS, nm
        assert cs.get(nm) == protos[nm], (nm, cs.get(nm), protos[nm])
    assert len(protos["vcp_match_unique"]) == len(protos["vcp_match_unique_dev"]) == 13
    assert protos["vcp_match_unique"] == ["ptr", "ptr", "i32", "ptr", "i32", "ptr", "f64"] + ["ptr"] * 6
    for meth in ("match_unique", "match_unique_dev"):
        assert callable(getattr(_native.Context, meth))
    from vtkcloudpoint_amd.tools import Matcher
    assert callable(Matcher.MatchOneToOne)


def _same(a, b):
    for k in ("truth_of", "center_of", "pair_dist"):
        assert np.array_equal(a[k], b[k]), k
    assert a["count"] == b["count"]


def test_the_second_centroid_wins_the_contested_truth():
    # c0 at 0.3 and c1 at 0.2 from t0; c0 also 0.5 from t1 (exact in binary: multiples of 1/8 scaled)
    t = np.array([[0.0, 0, 0], [0.0, 0.875, 0]])
    c = np.array([[0.0, 0.375, 0], [0.25, 0, 0]])   # d(c0,t0) = 0.375, d(c1,t0) = 0.25, d(c0,t1) = 0.5
    r = R.greedy_matching(c, t, I4, 1.0)
    assert r["truth_of"].tolist() == [1, 0] and r["center_of"].tolist() == [1, 0] and r["count"] == 2
    assert r["pair_dist"].tolist() == [0.5, 0.25]
    r = R.greedy_matching(c, t, I4, 0.5)            # d(c0,t1) >= max_dist: c0 stays unpaired
    assert r["truth_of"].tolist() == [-1, 0] and r["center_of"].tolist() == [1, -1] and r["count"] == 1
    assert r["pair_dist"].tolist() == [np.inf, 0.25]
    n = R.nearest_match(c, t, I4, 1.0)              # vcp_match gives t0 to both
    assert n["nearest"].tolist() == [0, 0] and n["count"] == 2


def test_an_exact_tie_goes_to_the_lower_centroid_then_the_lower_truth():
    # c0 and c1 both exactly 1 from t0: c0 (lower j) takes it; c1 has nothing else
    r = R.greedy_matching([[1.0, 0, 0], [-1.0, 0, 0]], [[0.0, 0, 0]], I4, 2.0)
    assert r["truth_of"].tolist() == [0, -1]
    # one centroid exactly 1 from t0 and t1: the lower truth index
    r = R.greedy_matching([[0.0, 0, 0]], [[1.0, 0, 0], [-1.0, 0, 0]], I4, 2.0)
    assert r["truth_of"].tolist() == [0] and r["center_of"].tolist() == [0, -1]
    # j decides before i: all four distances are 1; (c0,t0) first, then (c1,t1)
    r = R.greedy_matching([[0.0, 1, 0], [0.0, -1, 0]], [[1.0, 0, 0], [-1.0, 0, 0]], I4, 9.0)
    assert np.all(R.distances(R.transform([[0.0, 1, 0], [0.0, -1, 0]], I4)[:, None], np.array([[1.0, 0, 0], [-1.0, 0, 0]])[None])
                  == np.sqrt(2.0))
    assert r["truth_of"].tolist() == [0, 1]


def test_a_distance_of_exactly_max_dist_is_excluded_and_odd_thresholds_give_nothing():
    c, t = [[0.0, 0, 0]], [[0.5, 0, 0]]
    assert R.greedy_matching(c, t, I4, 0.5)["count"] == 0
    assert R.greedy_matching(c, t, I4, np.nextafter(0.5, 1))["count"] == 1
    for md in (np.nan, 0.0, -1.0):
        r = R.greedy_matching(c, t, I4, md)
        assert r["count"] == 0 and r["truth_of"].tolist() == [-1] and r["center_of"].tolist() == [-1]
    # non-finite points pair with nobody, not even at max_dist = +inf
    c = [[np.nan, 0, 0], [np.inf, 0, 0], [0.0, 0, 0]]
    t = [[0.0, np.nan, 0], [1.0, 0, 0]]
    r = R.greedy_matching(c, t, I4, np.inf)
    assert r["truth_of"].tolist() == [-1, -1, 1] and r["center_of"].tolist() == [-1, 2]


def _random_case(rng):
    T, K = int(rng.integers(1, 60)), int(rng.integers(1, 60))
    t = rng.uniform(0, 4, (T, 3))
    k = min(K, T)
    c = np.r_[t[rng.permutation(T)[:k]] + rng.normal(0, 0.05, (k, 3)), rng.uniform(0, 4, (K - k, 3))]
    if rng.random() < 0.5:  # a lattice: exact ties
        t, c = np.round(t * 2) / 2, np.round(c * 4) / 4
    M = np.eye(4)
    M[:3, 3] = rng.normal(0, 0.01, 3)
    return c, t, M, float(rng.choice([0.1, 0.3, 0.75, 5.0]))


def test_p1_every_truth_vcp_match_gives_away_is_paired():
    rng = np.random.default_rng(21)
    for _ in range(300):
        c, t, M, md = _random_case(rng)
        n, u = R.nearest_match(c, t, M, md), R.greedy_matching(c, t, M, md)
        given = set(n["nearest"][n["is_matched"] == 1].tolist())
        assert given <= set(np.flatnonzero(u["center_of"] >= 0).tolist())
        assert len(given) <= u["count"] <= n["count"]
        js = np.flatnonzero(u["truth_of"] >= 0)
        assert len(set(u["truth_of"][js].tolist())) == len(js)  # a pairing


def test_p2_where_nearest_is_injective_the_two_calls_agree():
    rng = np.random.default_rng(22)
    seen = 0
    for _ in range(600):
        c, t, M, md = _random_case(rng)
        n = R.nearest_match(c, t, M, md)
        got = n["nearest"][n["is_matched"] == 1]
        if len(set(got.tolist())) != len(got):
            continue
        seen += 1
        u = R.greedy_matching(c, t, M, md)
        assert np.array_equal(u["truth_of"], np.where(n["is_matched"] == 1, n["nearest"], -1))
        assert u["count"] == n["count"]
    assert seen >= 50


def test_rounds_of_locally_dominant_pairs_equal_the_walk():
    c, t = R.lattice(seed=7, T=300, K=330)
    for md in (0.6, 0.5):
        g, r = R.greedy_matching(c, t, I4, md), R.rounds_matching(c, t, I4, md)
        _same(g, r)
        assert g["count"] > 50 and r["rounds"] >= 2  # not vacuous: pairs exist, and not all in one round
    c, t = R.chain(300)
    g, r = R.greedy_matching(c, t, I4, 2.0), R.rounds_matching(c, t, I4, 2.0)
    _same(g, r)
    assert g["count"] == 300 and r["rounds"] == 300
    n = R.nearest_match(c, t, I4, 2.0)  # nearest is injective here, yet one pair per round
    assert n["nearest"].tolist() == list(range(300)) and g["truth_of"].tolist() == list(range(300))
    rng = np.random.default_rng(23)
    for _ in range(100):
        c, t, M, md = _random_case(rng)
        _same(R.greedy_matching(c, t, M, md), R.rounds_matching(c, t, M, md))
    c, t, M, _ = _random_case(rng)
    _same(R.greedy_matching(c, t, M, np.inf), R.rounds_matching(c, t, M, np.inf))


def test_the_sparse_candidate_search_equals_the_dense_one():
    c, t = R.field(seed=5, T=3000, n_det=2600, n_clutter=400)
    m = R.transform(c, I4)
    a = R.candidates(m, t, 0.1, dense_limit=0)
    b = R.candidates(m, t, 0.1, dense_limit=10 ** 9)
    ka, kb = np.lexsort((a[1], a[0])), np.lexsort((b[1], b[0]))
    assert len(a[0]) > 2600 and all(np.array_equal(x[ka], y[kb]) for x, y in zip(a, b))
