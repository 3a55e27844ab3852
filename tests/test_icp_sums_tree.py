"""The replay of the ICP moment sums' reduction tree (tests/icp_sums_ref.py) on the CPU: its launch plans are the ones
icp_run's arithmetic gives, it meets its derived bound against the exact sums, it is exact where every partial sum is,
it agrees with a plain sequential sum (and the oracle's) within the sum of both a-priori bounds, and every way of
getting the tree wrong changes its bits on the shared input set -- so the bit-for-bit GPU test,
tests/test_icp_sums_replay_gpu.py, would notice."""
from fractions import Fraction

import numpy as np
import pytest

import icp_sums_ref as S

ORDER_KNOBS = [k for k in S.KNOBS if k not in ("tail_dropped", "tail_counted")]   # those two change WHICH points are added


def _cases():
    """(path, nm, nd, family, pose): every shape on the generic family; every family at every shape, with both poses at
    the small ones."""
    out = []
    for path, nm, nd in S.SHAPES + S.SMALL_SHAPES:
        for fam in S.FAMILIES:
            for pose in S.POSES if nd <= 1000 else ("generic",):
                out.append((path, nm, nd, fam, pose))
    return out


def _digest(oracle, model, data, R, T, knobs, exact=True, contraction=True):
    """Everything the assertions need of one case, without keeping its [nd, 16] terms."""
    nm, nd = len(model), len(data)
    pl = S.plan(nm, nd, np.isfinite(model).all())
    p = S.transform(data, R, T)
    nn = oracle.find_closest(model, p)
    t = S.terms(model, data, R, T, nn)
    r = dict(pl=pl, nd=nd, sums=S.replay(t, nd, pl), seq=0.0 + np.add.accumulate(t, axis=0)[-1],
             oracle=oracle.icp_sums(model, p), mut={})
    if exact:
        sabs = S.abs_sums(t)
        r.update(exact=S._exact_columns(t), bound=S.bound(pl, t, sabs=sabs),
                 bound_seq=S.bound(pl, t, sequential=True, sabs=sabs))
    for knob in knobs:
        if knob in ("fma_products", "sse_contracted") and (nd > S.FMA_MAX_POINTS or not contraction):
            continue
        tk = S.terms(model, data, R, T, nn, sse_contracted=True) if knob == "sse_contracted" else t
        r["mut"][knob] = S.replay(tk, nd, pl, **S.KNOBS[knob])
    return r


@pytest.fixture(scope="module")
def results(oracle):
    # the contraction mutants cost a rational operation per point: beyond 1000 points on two families only
    return {c: _digest(oracle, *S.case(*c), S.KNOBS, contraction=c[2] <= 1000 or c[3] in ("generic", "lattice"))
            for c in _cases()}


@pytest.fixture(scope="module")
def probe_results(oracle):
    return {f: [_digest(oracle, *c, ("fma_products", "sse_contracted"), exact=False) for c in S.probes(f)]
            for f in S.INEXACT}


def test_plans_are_icp_runs():
    """The launch of every shape of the input set, written out: what icp_run computes from ICP_MAX_BLOCKS = 1024,
    nng::NNG = 8, the nm > 512 switch and tb = 64 / 256."""
    want = {
        ("pairs", 100): {1: (64, 1, 1), 2: (64, 1, 1), 3: (64, 1, 1), 127: (64, 1, 1), 128: (64, 1, 1), 129: (64, 2, 1),
                         65535: (64, 512, 1), 65536: (64, 512, 1), 65537: (256, 129, 1), 524288: (256, 1024, 1),
                         524289: (256, 1024, 2), 600001: (256, 1024, 2)},
        ("tiled", 600): {1: (64, 1, 1), 65: (64, 2, 1), 65536: (64, 1024, 1), 65537: (256, 257, 1),
                         262145: (256, 1024, 2), 300001: (256, 1024, 2)},
        ("grid", 600): {1: (64, 1, 1), 9: (64, 2, 1), 8192: (64, 1024, 1), 8193: (256, 257, 1), 32769: (256, 1024, 2),
                        40001: (256, 1024, 2)},
    }
    assert sorted((p, nm, nd) for (p, nm), v in want.items() for nd in v) == sorted(S.SHAPES)
    for path, nm, nd in S.SHAPES:
        pl = S.plan(nm, nd, path != "tiled")
        assert (pl["path"], pl["tb"], pl["nb"], pl["trips"]) == (path,) + want[(path, nm)][nd], (path, nm, nd)
    assert [S.plan(nm, 1000)["path"] for nm in (1, 2, 512, 513)] == ["pairs"] * 3 + ["grid"]
    assert S.plan(513, 1000, False)["path"] == "tiled" and S.plan(512, 1000, False)["path"] == "pairs"
    assert S.depth(S.plan(100, 600001)) == 4 + 9 + 13 and S.depth(S.plan(600, 1, False)) == 1 + 6 + 10


def test_terms_are_the_oracles(results):
    """The replay's terms summed one after the other ARE the oracle's sums, bit for bit: the same TransPoint, products and
    SSE expression (the oracle is built without contraction too)."""
    for c, r in results.items():
        assert np.array_equal(r["seq"], r["oracle"]), c


def test_two_product_is_exact():
    rng = np.random.default_rng(11)
    a = np.concatenate([rng.uniform(-10, 10, 300), 1e5 + rng.uniform(-10, 10, 300), rng.uniform(-10, 10, 300) * 2.0 ** 40,
                        np.array([0.0, -0.0, 1.0, 3.0 / 1024])])
    b = rng.permutation(a)
    x, e = S._two_prod(a, b)
    for i in range(len(a)):
        assert Fraction(float(x[i])) + Fraction(float(e[i])) == Fraction(float(a[i])) * Fraction(float(b[i]))
    assert S._exact_dot(a, b) == sum(Fraction(float(u)) * Fraction(float(v)) for u, v in zip(a, b))
    x = np.concatenate([a, 10.0 ** rng.uniform(-300, 300, 200) * rng.choice([-1, 1], 200),
                        np.array([5e-324, -1.5e-323, 2.2250738585072014e-308, -1e-310, 1e308, -1e308])])
    assert S._exact_sum(x) == sum(Fraction(float(v)) for v in x)
    assert S._fma(3.0, 1.0 + 2.0 ** -52, -3.0) == 3 * 2.0 ** -52 and S._fma(0.1, 10.0, -1.0) == 2.0 ** -54


def test_replay_within_bound_of_exact_sums(results):
    worst = 0.0
    for c, r in results.items():
        for k in range(16):
            err = abs(Fraction(float(r["sums"][k])) - r["exact"][k])
            assert err <= r["bound"][k], (c, k)
            if r["bound"][k]:
                worst = max(worst, float(err / r["bound"][k]))
    print("replay error / a-priori bound, worst over the input set: %.3g" % worst)
    assert 0.0 < worst < 1.0


def test_replay_against_sequential_sum(results):
    """Two rounded sums of the same terms differ by at most the sum of their a-priori bounds."""
    for c, r in results.items():
        for k in range(16):
            d = abs(Fraction(float(r["sums"][k])) - Fraction(float(r["seq"][k])))
            assert d <= r["bound"][k] + r["bound_seq"][k], (c, k)


@pytest.mark.parametrize("knob", [k for k in S.KNOBS if k not in ("fma_products", "sse_contracted")])
def test_every_knob_changes_bits(results, knob):
    """A replay with one property of the kernels' order broken differs in bits from the true replay in at least one of
    the 16 sums, on every family whose sums round, at every shape where S.shows() demands it; where the property is not
    in play the mutant IS the replay.  This is the proof, without a GPU, that the bit-for-bit GPU comparison notices."""
    demanded = 0
    for (path, nm, nd, fam, pose), r in results.items():
        same = np.array_equal(r["mut"][knob], r["sums"], equal_nan=True)
        if not S.in_play(knob, r["pl"], nd):
            assert same, (knob, path, nm, nd, fam, pose)
        elif S.shows(knob, r["pl"], nd) and fam in S.INEXACT:
            assert not same, (knob, path, nm, nd, fam, pose)
            demanded += 1
    assert demanded >= (10 if knob == "cap_2048" else 30)
    if knob == "cap_2048":   # it can only show where the cap binds
        assert all(r["pl"]["nb"] == 1024 and r["pl"]["trips"] == 2 for c, r in results.items()
                   if S.in_play(knob, r["pl"], r["nd"]))


@pytest.mark.parametrize("knob", ["fma_products", "sse_contracted"])
def test_contraction_changes_bits_on_the_probes(probe_results, results, knob):
    """Contracting s += p * y or the SSE expression changes the bits of some probe on every family whose sums round and
    on every kernel it can act in: k_icp_pass_small (both mutants), and the SSE term of k_icp_pass on the tiled and
    the grid path.  (An accumulate onto a non-zero sum in k_icp_pass needs a second trip, 262 145 slots: not probed.)"""
    n = S.N_PROBES
    for fam, rs in probe_results.items():
        groups = {"pairs": rs[:n], "tiled": rs[n:2 * n], "grid": rs[2 * n:]}
        for path, g in groups.items():
            assert all(r["pl"]["path"] == path and r["pl"]["tb"] == 64 for r in g)
            hits = sum(not np.array_equal(r["mut"][knob], r["sums"]) for r in g)
            if knob == "fma_products" and path != "pairs":
                assert hits == 0, (fam, path)      # one point, one add from +0.0: nothing to contract
            else:
                assert hits >= 1, (knob, fam, path, hits)
    # in the long sums it is a matter of luck, which is why the probes exist: some sum of 1000 terms or more hides it
    long_sums = [np.array_equal(r["mut"][knob], r["sums"]) for c, r in results.items()
                 if c[2] >= 1000 and c[3] in S.INEXACT and knob in r["mut"] and S.in_play(knob, r["pl"], c[2])]
    assert len(long_sums) >= 10 and any(long_sums)


def test_lattice_family_hides_every_order_knob(results):
    """The counterpart: on multiples of 2^-10 every partial sum is exact, the replay IS the exact sum and no order or
    contraction mutant can be told apart -- that family (what synth and the benchmark are made of) is no evidence of
    order.  The two tail mutants lose or double a point and show there too."""
    seen = 0
    for (path, nm, nd, fam, pose), r in results.items():
        if fam != "lattice":
            continue
        assert r["sums"].tolist() == [float(x) for x in r["exact"]], (path, nm, nd, pose)
        for knob in ORDER_KNOBS:
            if knob in r["mut"]:
                assert np.array_equal(r["mut"][knob], r["sums"]), (knob, path, nm, nd, pose)
                seen += 1
        for knob in ("tail_dropped", "tail_counted"):
            assert np.array_equal(r["mut"][knob], r["sums"]) == (not S.in_play(knob, r["pl"], nd)), (knob, path, nm, nd)
    assert seen > 200


def test_signed_zero_and_nan():
    """A sum is never -0.0, whatever the terms; a NaN term makes its sums NaN and no other."""
    pl = S.plan(100, 5)
    t = np.full((5, 16), -0.0)
    s = S.replay(t, 5, pl)
    assert (s == 0.0).all() and not np.signbit(s).any()
    t = np.ones((5, 16))
    t[3, 7] = np.nan
    s = S.replay(t, 5, pl)
    assert np.isnan(s[7]) and (np.delete(s, 7) == 5.0).all()
    with pytest.raises(TypeError):
        S.replay(t, 5, pl, no_such_knob=1)
