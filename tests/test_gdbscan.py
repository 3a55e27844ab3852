"""vcp_gdbscan without a GPU: the two entry points in the header, the library, the Python binding, the C# imports and the
C++ mirror with matching arity; the numpy restatement of the definition (tests/gdbscan_ref.py) held to the project's oracle
(the literal DBImproved) in three forms -- unit weights, integer weights against the expanded cloud, a gate on a group
number against one run per group -- and to scikit-learn's DBSCAN with sample_weight; hand cases; multiplicity().  The
device is held to equality with the restatement in tests/test_gdbscan_gpu.py.  Every comparison is equality."""
import inspect
import os
import re

import numpy as np
import pytest

import gdbscan_ref as R
from test_abi import _csharp_imports, _declared, _header_prototypes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("vcp_gdbscan", "vcp_gdbscan_dev")
N_CLOUDS = 300


def test_the_two_symbols_everywhere_with_matching_arity():
    from vtkcloudpoint_amd import _native, dbscan, gdbscan
    lib = _native.lib()
    decl, protos = _declared(), _header_prototypes()
    cs = {name: classes for _, name, classes in _csharp_imports()}
    for nm in NAMES:
        assert nm in decl and hasattr(lib, nm) and nm in _native.SYMBOLS, nm
        assert cs.get(nm) == protos[nm], (nm, cs.get(nm), protos[nm])
        assert len(protos[nm]) == 15
    assert protos["vcp_gdbscan"] == ["ptr", "ptr", "i64", "i32", "i32", "f64", "ptr", "f64", "ptr", "i64", "i32"] + ["ptr"] * 4
    assert protos["vcp_gdbscan_dev"] == protos["vcp_gdbscan"]
    assert list(inspect.signature(_native.Context.gdbscan).parameters) == \
        ["self", "coords", "eps", "min_weight", "metric", "weights", "aux", "gate", "cf_in", "want_wsum"]
    assert callable(_native.Context.gdbscan_dev)
    assert list(inspect.signature(gdbscan.gdbscan).parameters)[:9] == \
        ["points", "eps", "min_weight", "weights", "aux", "gate", "metric", "cf_in", "ctx"]
    assert list(inspect.signature(gdbscan.multiplicity).parameters) == ["rows"]
    assert list(inspect.signature(dbscan.DBImproved.dbscanGeneral).parameters) == \
        ["self", "lst", "e", "minWeight", "gate", "usePtsCount"]
    host = os.path.join(ROOT, "vtkcloudpoint_amd", "host")
    with open(os.path.join(host, "csharp", "DBImproved.cs")) as f:
        assert re.search(r"public\s+void\s+dbscanGeneral\s*\(", f.read())
    with open(os.path.join(host, "cpp", "vcp_host.hpp")) as f:
        src = f.read()
    m = re.search(r"vcp_gdbscan\(([^;]*)\)\);", src, re.S)
    assert m and re.search(r"namespace vcp\s*\{", src) and "gdbscan(Context&" in src and "dbscanGeneral(" in src
    depth, args = 0, 1                       # arguments of the mirror's call: commas outside brackets
    for ch in m.group(1):
        depth += ch in "(["
        depth -= ch in ")]"
        args += ch == "," and depth == 0
    assert args == 15


def _clouds():
    """300 seeded clouds, n in 1..119, the three metrics; every other one on a 1/8 lattice (exact ties).  Per cloud:
    integer weights 1..3, a group number 0..2, eps, min_weight."""
    rng = np.random.default_rng(1998)
    for t in range(N_CLOUDS):
        n = int(rng.integers(1, 120))
        metric = t % 3
        c = rng.uniform(0, 1, (n, 3 if metric == R.L2_3D else 2))
        if t % 2:
            c = np.round(c * 8) / 8
        w = rng.integers(1, 4, n).astype(np.int32)
        grp = rng.integers(0, 3, n).astype(np.float64)
        eps = (0.125, 0.2, 0.3)[(t // 3) % 3] * (1.5 if metric == R.L2_3D else 1.0)
        yield t, c, metric, eps, (2, 4, 7)[(t // 9) % 3], w, grp


@pytest.fixture(scope="module")
def sweep():
    """The restatement's results on the seeded clouds, computed once: plain, weighted, gated."""
    out = []
    for t, c, metric, eps, mw, w, grp in _clouds():
        out.append(dict(t=t, c=c, metric=metric, eps=eps, mw=mw, w=w, grp=grp,
                        plain=R.gdbscan(c, eps, mw, metric),
                        weighted=R.gdbscan(c, eps, mw, metric, weights=w),
                        gated=R.gdbscan(c, eps, mw, metric, aux=grp, gate=0.5)))
    return out


def test_unit_weights_no_gate_is_the_oracle(oracle, sweep):
    for s in sweep:
        o = oracle.dbscan(s["c"], s["eps"], s["mw"], s["metric"], literal=True)
        r = s["plain"]
        assert np.array_equal(r["labels"], o["labels"]) and np.array_equal(r["is_core"], o["is_key"]), s["t"]
        assert r["cf"] == o["cf"], s["t"]


def test_integer_weights_are_the_oracle_on_the_expanded_cloud(oracle, sweep):
    rng = np.random.default_rng(3)
    for s in sweep:
        n = len(s["c"])
        big = R.expand(s["c"], s["w"])
        tail = n + rng.permutation(len(big) - n)              # the copies in any order
        big = np.concatenate([big[:n], big[tail]])
        o = oracle.dbscan(big, s["eps"], s["mw"], s["metric"], literal=True)
        r = s["weighted"]
        assert np.array_equal(r["labels"], o["labels"][:n]) and np.array_equal(r["is_core"], o["is_key"][:n]), s["t"]
        assert r["cf"] == o["cf"], s["t"]


def test_a_gate_on_a_group_number_is_one_oracle_run_per_group(oracle, sweep):
    for s in sweep:
        n = len(s["c"])
        labels, core, off = np.zeros(n, np.int32), np.zeros(n, np.uint8), 0
        for g in range(3):
            idx = np.nonzero(s["grp"] == g)[0]
            if len(idx) == 0:
                continue
            o = oracle.dbscan(s["c"][idx], s["eps"], s["mw"], s["metric"], literal=True)
            labels[idx] = np.where(o["labels"] != 0, o["labels"] + off, 0)
            core[idx] = o["is_key"]
            off += o["cf"]
        labels, k = R.renumber(labels, core)
        r = s["gated"]
        assert np.array_equal(r["labels"], labels) and np.array_equal(r["is_core"], core) and r["cf"] == k, s["t"]


def test_the_sweep_is_not_vacuous(sweep):
    two, gate_matters, weights_matter = 0, 0, 0
    for s in sweep:
        for key, kw in (("plain", {}), ("weighted", {}), ("gated", dict(aux=s["grp"], gate=0.5))):
            r = s[key]
            core = r["is_core"].astype(bool)
            N = R.neighbourhoods(s["c"], s["eps"], s["metric"], **kw)
            for i in np.nonzero(~core & (r["labels"] != 0))[0]:
                two += len(np.unique(r["labels"][N[i] & core])) >= 2
        gate_matters += not np.array_equal(s["gated"]["labels"], s["plain"]["labels"])
        weights_matter += not np.array_equal(s["weighted"]["is_core"], s["plain"]["is_core"])
    assert two >= 10 and gate_matters >= 50 and weights_matter >= 50, (two, gate_matters, weights_matter)


def test_restatement_against_scikit_learn():
    cluster = pytest.importorskip("sklearn.cluster")
    rng = np.random.default_rng(11)
    checked = 0
    for t in range(30):
        n = int(rng.integers(20, 150))
        metric = t % 3
        c = rng.uniform(0, 1, (n, 3 if metric == R.L2_3D else 2))
        if t % 2:
            c = np.round(c * 8) / 8
        w = rng.integers(0, 4, n)                                 # zeros included
        aux = rng.integers(0, 3, n).astype(np.float64) if t % 4 != 1 else None
        eps, mw = 0.2 * (1.5 if metric == R.L2_3D else 1.0), 5
        r = R.gdbscan(c, eps, mw, metric, weights=w, aux=aux, gate=None if aux is None else 1.0)
        D = R.dist_matrix(c, metric)
        if aux is not None:
            D = np.where(np.abs(aux[:, None] - aux[None, :]) <= 1.0, D, 1e9)   # gated-out pairs set far
        sk = cluster.DBSCAN(eps=eps, min_samples=mw, metric="precomputed").fit(D, sample_weight=w)
        core = np.zeros(n, bool)
        core[sk.core_sample_indices_] = True
        assert np.array_equal(core, r["is_core"].astype(bool)), t
        a, b = sk.labels_[core], r["labels"][core]
        assert (a >= 0).all() and (b > 0).all()
        assert np.array_equal(a[:, None] == a[None, :], b[:, None] == b[None, :]), t    # the same partition of the cores
        assert len(np.unique(b)) == r["cf"]
        checked += core.any()
    assert checked >= 20


def test_hand_cases():
    # a border point between two clusters takes the higher id
    left = [[0.0, 0.0], [0.0, 0.05], [0.0, -0.05]]
    right = [[1.0, 0.0], [1.0, 0.05], [1.0, -0.05]]
    c = np.array(left + [[0.5, 0.0]] + right)
    r = R.gdbscan(c, 0.5, 4, R.L1_2D)
    assert r["is_core"].tolist() == [1, 0, 0, 0, 1, 0, 0] and r["cf"] == 2
    assert r["labels"].tolist() == [1, 1, 1, 2, 2, 2, 2] and r["wsum"].tolist() == [4, 3, 3, 3, 4, 3, 3]
    r = R.gdbscan(c[::-1], 0.5, 4, R.L1_2D, cf_in=5)             # the other cluster comes first now: still the higher id
    assert r["labels"].tolist() == [6, 6, 6, 7, 7, 7, 7] and r["cf"] == 7
    # |aux difference| exactly equal to the gate is inside, one ulp above it is outside
    c = np.zeros((3, 2))
    assert R.gdbscan(c, 0.0, 3, R.L2_2D, aux=[1.0, 1.5, 2.0], gate=0.5)["wsum"].tolist() == [2, 3, 2]
    assert R.gdbscan(c, 0.0, 2, R.L2_2D, aux=[1.0, 1.5, 2.0], gate=0.5)["labels"].tolist() == [1, 1, 1]
    up = np.nextafter(1.5, 2.0)
    assert R.gdbscan(c, 0.0, 2, R.L2_2D, aux=[1.0, up, 2.0], gate=0.5)["labels"].tolist() == [0, 1, 1]
    # a weight-0 row within eps of a core point is labelled and adds nothing
    c = np.array([[0.0, 0.0], [0.1, 0.0], [0.2, 0.0]])
    r = R.gdbscan(c, 0.1, 3, R.L1_2D, weights=[2, 0, 1])
    assert r["wsum"].tolist() == [2, 3, 1] and r["is_core"].tolist() == [0, 1, 0] and r["labels"].tolist() == [1, 1, 1]
    r = R.gdbscan(c, 0.1, 3, R.L1_2D, weights=[3, 0, 0])
    assert r["wsum"].tolist() == [3, 3, 0] and r["is_core"].tolist() == [1, 1, 0] and r["labels"].tolist() == [1, 1, 1]
    # three rows of weight 2^30: 3 * 2^30 does not fit an int32
    r = R.gdbscan(np.zeros((3, 2)), 0.5, 3 << 30, R.L1_2D, weights=[1 << 30] * 3)
    assert r["wsum"].tolist() == [3 << 30] * 3 and r["is_core"].tolist() == [1, 1, 1] and r["cf"] == 1
    assert not R.gdbscan(np.zeros((3, 2)), 0.5, (3 << 30) + 1, R.L1_2D, weights=[1 << 30] * 3)["is_core"].any()
    # non-finite rows: an empty neighbourhood, in nobody's; with min_weight <= 0 a cluster each
    c = np.array([[0.0, 0.0], [np.nan, 0.0], [0.0, 0.0], [np.inf, 0.0]])
    r = R.gdbscan(c, 1.0, 2, R.L1_2D)
    assert r["labels"].tolist() == [1, 0, 1, 0] and r["wsum"].tolist() == [2, 0, 2, 0]
    r = R.gdbscan(c, 1.0, 0, R.L1_2D)
    assert r["labels"].tolist() == [1, 2, 1, 3] and r["is_core"].all() and r["cf"] == 3
    r = R.gdbscan(c[[0, 2]], 1.0, 2, R.L1_2D, aux=[1.0, np.nan], gate=np.inf)
    assert r["labels"].tolist() == [0, 0] and r["wsum"].tolist() == [1, 0]
    # eps NaN or < 0: every neighbourhood is empty
    for eps in (np.nan, -1.0):
        r = R.gdbscan(np.zeros((3, 2)), eps, 1, R.L1_2D)
        assert not r["labels"].any() and not r["wsum"].any() and r["cf"] == 0
        assert R.gdbscan(np.zeros((3, 2)), eps, 0, R.L1_2D)["labels"].tolist() == [1, 2, 3]


def test_multiplicity_on_shuffled_duplicates():
    from vtkcloudpoint_amd.gdbscan import multiplicity
    rng = np.random.default_rng(21)
    base = np.round(rng.uniform(0, 1, (200, 3)) * 64) / 64
    counts = rng.integers(1, 4, 200)
    rows = np.repeat(base, counts, axis=0)[rng.permutation(int(counts.sum()))]
    first, cnt = multiplicity(rows)
    seen, want_first, want_cnt = {}, [], []
    for i, row in enumerate(map(bytes, rows)):                    # the import's dedupe with the count kept
        if row in seen:
            want_cnt[seen[row]] += 1
        else:
            seen[row] = len(want_first)
            want_first.append(i)
            want_cnt.append(1)
    assert first.tolist() == want_first and cnt.tolist() == want_cnt
    assert first.dtype == np.int64 and cnt.dtype == np.int32 and cnt.sum() == len(rows)
    # the raw cloud's clustering, restricted to the first occurrences, is the weighted clustering of the distinct rows
    raw = R.gdbscan(rows[:, :2], 0.08, 6, R.L1_2D)
    # ids are numbered by smallest member index, and the first occurrences keep the raw cloud's order
    w = R.gdbscan(rows[first][:, :2], 0.08, 6, R.L1_2D, weights=cnt)
    assert np.array_equal(w["labels"], raw["labels"][first]) and np.array_equal(w["is_core"], raw["is_core"][first])
    assert w["cf"] == raw["cf"] and np.array_equal(w["wsum"], raw["wsum"][first])
    e_first, e_cnt = multiplicity(np.zeros((0, 3)))
    assert len(e_first) == 0 and len(e_cnt) == 0
