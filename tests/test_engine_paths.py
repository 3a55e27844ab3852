"""The case table of the DBSCAN engine's paths (tests/engine_path_cases.py) held to the source and to the oracle, without
a GPU: every launch site of csrc/dbscan.hip is expected by some case, every case is on the 2^-10 lattice and small, and the
oracle's result has the structure the case's docstring promises -- core, border and noise points where the case needs them,
the re-scan probe a border point, the clumps of the sizes stated.  tests/test_engine_paths_gpu.py runs the same table on
the device."""
import os
import re

import numpy as np
import pytest

import engine_path_cases as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def launch_sites(path):
    """The kernel argument of every `VCP_LAUNCH(ctx, ...` in a source file, whitespace collapsed as the trace prints it."""
    with open(path) as f:
        text = f.read()
    out = []
    for m in re.finditer(r"\bVCP_LAUNCH\(ctx,", text):
        i, depth, angle = m.end(), 0, 0
        start = i
        while True:
            ch = text[i]
            if ch == "(":
                depth += 1
            elif ch == ")":
                depth -= 1
            elif ch == "<":
                angle += 1
            elif ch == ">":
                angle -= 1
            elif ch == "," and depth == 0 and angle == 0:
                break
            i += 1
        out.append(" ".join(text[start:i].split()))
    return out


def test_every_launch_site_of_the_engine_is_in_the_table():
    found = launch_sites(os.path.join(ROOT, "vtkcloudpoint_amd", "csrc", "dbscan.hip"))
    assert len(found) >= 30
    assert set(found) == set(T.SITES), "engine_path_cases.SITES against dbscan.hip: %r" % (set(found) ^ set(T.SITES))
    expected = set()
    for c in T.CASES:
        must, must_not = c.expect()
        assert must <= T.SITES and not (must & must_not)
        expected |= must
    # the two sites only a switch reaches: VCP_CORE_GLOBAL on the grouped case, VCP_JOIN_ALL on any case with lists
    expected |= T.BY_NAME["grouped_blocks"].expect(core_global=True)[0]
    # regime-dependent sites are left open on the grouped and staged cases; the plain cases demand each of them
    missing = T.SITES - expected
    assert not missing, "launch sites no case expects: %r" % sorted(missing)


def test_the_model_of_the_driver_covers_both_sides_of_every_fork():
    seen = {}
    for c in T.CASES:
        if c.kind == "engine":
            for s in c.expect()[0]:
                seen.setdefault(s, set()).add(c.params["gd"])
    for s in ("k_flatten0<2>", "k_flatten0<1>", "k_flatten<true>", "k_flatten<false>", "k_chunkroot", T.UNION_DENSE,
              T.UNION_PRE, T.BORDER, T.BORDER_LIST, "k_union_init_list"):
        assert seen.get(s) == {2, 3}, "%s is expected in %r-D only" % (s, seen.get(s))
    assert seen[T.UNION_INIT] == {2} and seen[T.UNION_PLAIN] == {3} and seen[T.CORE_LDS] == {2} and seen[T.CORE_GLOBAL] == {3}


def _structure(inp, o):
    core = o["is_key"].astype(bool)
    entered = inp.get("in_classed")
    entered = np.zeros(len(core), bool) if entered is None else np.asarray(entered).astype(bool)
    return {"core": core.any(), "border": ((o["labels"] != 0) & ~core & ~entered).any(), "noise": (o["labels"] == 0).any()}


@pytest.mark.parametrize("case", T.CASES, ids=lambda c: c.name)
def test_case_is_small_exact_and_means_what_it_says(case, oracle):
    assert case.__doc__ and len(case.__doc__) > 80, "every case says why its path is reached"
    inp = case.build()
    again = case.build()
    c = inp["motor"] if case.kind == "blocks" else inp["coords"]
    assert np.array_equal(c, again["motor" if case.kind == "blocks" else "coords"], equal_nan=True), "fixed seed"
    assert len(c) <= 3000
    fin = c[np.isfinite(c)]
    assert np.array_equal(fin * T.Q, np.round(fin * T.Q)), "coordinates on the 2^-10 lattice"
    if case.kind == "blocks":
        o = oracle.block_pipeline(inp["motor"], inp["eps"], inp["min_pts"], inp["pts_in_cell"], 3)
        sizes = np.bincount(o["block_of"][o["block_of"] >= 0])
        assert (sizes > 1024).any() and (sizes <= 1024).any() and o["cluster_amount"] > 3, sizes
        return
    o = oracle.dbscan(c, inp["eps"], inp["min_pts"], inp["metric"], inp.get("cf_in", 0), inp.get("in_classed"),
                      inp.get("labels"))
    have = _structure(inp, o)
    for k in case.needs:
        assert have[k], "the case needs %s points" % k
    if case.claim:
        case.claim(inp, T.neighbour_counts(c, inp["eps"], inp["metric"]), o)


def test_trace_line_parser():
    what, d = T.parse_trace_line("vcp-trace dbscan n=12 gd=2 ncells=1 D=1,1,1 cellw=inf sc.lo=-1 sc.hi=inf dense=0")
    assert what == "dbscan" and d["n"] == 12 and d["D"] == [1, 1, 1] and d["cellw"] == float("inf") and d["sc.lo"] == -1
    assert T.parse_trace_line("vcp-trace launch (k_union<GD, METRIC, GROUPED, true, true>)") == \
        ("launch", "(k_union<GD, METRIC, GROUPED, true, true>)")
    assert T.parse_trace_line("vcp-trace dbscan all_pairs n=3 metric=0 min_pts=2")[1]["_words"] == ["all_pairs"]
