"""What keeps tests/fuzz_queries.py from passing by being empty, without a GPU: the case lists that
tests/test_fuzz_queries_gpu.py runs (same seeds, same counts, built by make_<family> alone) held to conditions computed
from the references -- few degenerate cases, thresholds taken from the case's own distances in all three variants, every
frame transform, DBSCAN cases with several clusters, with border points and with a pair at exactly eps that decides a
core flag, contested truths and a pair dropped only because d == max_dist -- and the restatements themselves held to the
oracle, to nearthr's exact pair count and to each other on these far-origin and scaled inputs."""
import math

import numpy as np
import pytest

import fuzz_queries as F
import gdbscan_ref as GD
import match_unique_ref as MU
import nearthr as NT

DBSCAN_LIKE = ("kdist", "eps_tree", "gdbscan")
_LISTS = {}


def case_list(family):
    """The family's committed case list, built once per process."""
    if family not in _LISTS:
        count, seed = F.SUITE[family]
        _LISTS[family] = list(F.case_list(family, count, seed))
    return _LISTS[family]


def problems(family, cases):
    """The conditions on a case list that fail, as a list of strings (empty: all hold)."""
    n = len(cases)
    third = math.ceil(n / 3)
    bad = []
    degenerate = sum(c["degenerate"] for c in cases)
    if degenerate * 10 > n:
        bad.append("%d of %d cases degenerate" % (degenerate, n))
    own = [c for c in cases if c["mode"] == "own"]
    if len(own) < third:
        bad.append("%d of %d thresholds from the case's own distances" % (len(own), n))
    for v in F.VARIANTS:
        if not any(c["variant"] == v for c in own):
            bad.append("no own threshold taken %s" % v)
    for t in ("shift", "scale", "outliers"):
        if not any(c["transform"] == t for c in cases):
            bad.append("no case with the transform %s" % t)
    if family in DBSCAN_LIKE:
        if "nearthr" not in {c["transform"] for c in cases}:
            bad.append("no near-threshold frame")
        if sum(c["clusters"] >= 2 for c in cases) < third:
            bad.append("%d cases with two or more clusters" % sum(c["clusters"] >= 2 for c in cases))
        if sum(c["border"] for c in cases) < third:
            bad.append("%d cases with a non-core labelled point" % sum(c["border"] for c in cases))
        if not any(c["decides"] for c in cases):
            bad.append("no pair at exactly eps decides a core flag")
    if family == "match_unique":
        if sum(c["contested"] for c in cases) < third:
            bad.append("%d cases with a contested truth" % sum(c["contested"] for c in cases))
        if not any(c["dropped"] for c in cases):
            bad.append("no pair dropped only because d == max_dist")
    if family in F.HALF:            # a case without a hypothesis compares nothing but zeros
        if sum(c["hypotheses"] > 0 and c["best"] >= 0 for c in cases) < third:
            bad.append("%d cases with a scored hypothesis" % sum(c["hypotheses"] > 0 and c["best"] >= 0 for c in cases))
    if family == "assign_truths":   # a case in which nothing is assigned compares nothing but zeros
        if sum(c["assigned"] > 0 for c in cases) < third:
            bad.append("%d cases with an assigned point" % sum(c["assigned"] > 0 for c in cases))
    return bad


@pytest.mark.parametrize("family", F.FAMILIES)
def test_the_case_list_is_not_empty_handed(oracle, family):
    cases = case_list(family)
    assert len(cases) == F.SUITE[family][0]
    assert problems(family, cases) == []


def test_the_case_list_is_a_function_of_the_seed():
    a = list(F.case_list("assign_truths", 6, 77))
    b = list(F.case_list("assign_truths", 6, 77))
    for x, y in zip(a, b):
        assert x["tag"] == y["tag"] and x["radius"] == y["radius"] and x["motor"].tobytes() == y["motor"].tobytes()
        assert np.array_equal(x["want_ids"], y["want_ids"])


def test_gdbscan_restatement_is_the_oracle_on_these_clouds(oracle):
    """gdbscan_ref with neither weights nor aux against oracle.dbscan: labels, core flags and count, on the clouds and
    thresholds of the kdist and gdbscan lists (far origins, scaled frames, own distances)."""
    compared = 0
    for family in ("kdist", "gdbscan"):
        for c in case_list(family):
            mp = c["k"] if family == "kdist" else c["mw"]
            r = c["ref"] if family == "kdist" else GD.gdbscan(c["c"], c["eps"], mp, c["metric"])
            o = oracle.dbscan(c["c"], c["eps"], mp, c["metric"])
            what = "%s case %d %s" % (family, c["index"], c["tag"])
            assert np.array_equal(r["labels"], o["labels"]), what
            assert np.array_equal(r["is_core"], o["is_key"]) and r["cf"] == o["cf"], what
            compared += 1
    assert compared == F.SUITE["kdist"][0] + F.SUITE["gdbscan"][0]


def test_brute_force_kdist_is_the_exact_core_count():
    """kd <= eps <=> nearthr.exact_core (every pair within eps counted in binary64 from a k-d tree's candidates)."""
    compared = 0
    for c in case_list("kdist"):
        for eps in c["eps_list"].tolist():
            with np.errstate(invalid="ignore"):
                want = (c["kd"] <= eps).astype(np.uint8)
            assert np.array_equal(want, NT.exact_core(c["c"], c["metric"], eps, c["k"])), (c["index"], c["tag"], eps)
            compared += 1
    assert compared >= 2 * F.SUITE["kdist"][0]


def test_greedy_walk_is_the_rounds():
    for c in case_list("match_unique"):
        r = MU.rounds_matching(c["centers"], c["truths"], c["M"], c["max_dist"])
        g = c["ref"]
        what = "case %d %s" % (c["index"], c["tag"])
        assert np.array_equal(r["truth_of"], g["truth_of"]) and np.array_equal(r["center_of"], g["center_of"]), what
        assert F.same_doubles(r["pair_dist"], g["pair_dist"]) and r["count"] == g["count"], what
