"""vcp_eps_tree without a GPU: the two entry points in the header, the Python binding, the library, the C# imports and the
C++ mirror with matching arity; the numpy restatement of the definition (tests/eps_tree_ref.py) held to the project's
oracle (the literal DBImproved) at every breakpoint and midpoint, and to scipy's minimum spanning tree; the host emulation
of the device's rounds held to the walk; hand-checked cases; the numpy helpers of vtkcloudpoint_amd/epstree.py.  The device
is held to equality with the restatement in tests/test_eps_tree_gpu.py."""
import inspect
import os
import re

import numpy as np
import pytest

import eps_tree_ref as R
from test_abi import _csharp_imports, _declared, _header_prototypes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("vcp_eps_tree", "vcp_eps_tree_dev")


def _tree(c, k, eps_max, metric):
    from vtkcloudpoint_amd.epstree import EpsTree
    r = R.eps_tree(np.asarray(c, np.float64), k, eps_max, metric)
    return EpsTree(r["kdist"], r["reach"], r["merge_w"], r["merge_a"], r["merge_b"], eps_max, k), r


def test_the_two_symbols_everywhere_with_matching_arity():
    from vtkcloudpoint_amd import _native, epstree
    lib = _native.lib()
    decl, protos = _declared(), _header_prototypes()
    cs = {name: classes for _, name, classes in _csharp_imports()}
    for nm in NAMES:
        assert nm in decl and hasattr(lib, nm) and nm in _native.SYMBOLS, nm
        assert cs.get(nm) == protos[nm], (nm, cs.get(nm), protos[nm])
        assert len(protos[nm]) == 15
    assert protos["vcp_eps_tree"] == ["ptr", "ptr", "i64", "i32", "i32", "i32", "f64", "i32"] + ["ptr"] * 7
    assert protos["vcp_eps_tree_dev"] == protos["vcp_eps_tree"]
    assert list(inspect.signature(_native.Context.eps_tree).parameters) == \
        ["self", "coords", "k", "eps_max", "metric", "kdist", "want_edges"]
    assert callable(_native.Context.eps_tree_dev)
    assert list(inspect.signature(epstree.eps_tree).parameters) == ["points", "min_pts", "eps_max", "metric", "ctx", "kd"]
    for fn in (epstree.counts_at, epstree.cluster_count_steps, epstree.eps_for_clusters, epstree.core_labels_at):
        assert callable(fn)
    host = os.path.join(ROOT, "vtkcloudpoint_amd", "host")
    with open(os.path.join(host, "csharp", "Tools.Gpu.cs")) as f:
        assert re.search(r"public\s+static\s+[\w\[\],<> ]+\s+EpsForClusters\s*\(", f.read())
    with open(os.path.join(host, "cpp", "vcp_host.hpp")) as f:
        src = f.read()
    m = re.search(r"vcp_eps_tree\(([^;]*)\)\);", src, re.S)
    assert m and "EpsTree(" in src
    depth, args = 0, 1                       # arguments of the mirror's call: commas outside brackets
    for ch in m.group(1):
        depth += ch in "(["
        depth -= ch in ")]"
        args += ch == "," and depth == 0
    assert args == 15


def _clouds():
    """40 seeded clouds, n in 2..150, the three metrics, k in {1, 2, 4, 7}; every other one on a 1/8 lattice."""
    rng = np.random.default_rng(2024)
    for t in range(40):
        n = int(rng.integers(2, 151))
        metric = t % 3
        c = rng.uniform(0, 1, (n, 3 if metric == R.L2_3D else 2))
        if t % 2:
            c = np.round(c * 8) / 8
        yield t, c, metric, (1, 2, 4, 7)[(t // 3) % 4], (0.2, 0.35, 0.6)[t % 3] * (1.5 if metric == R.L2_3D else 1.0)


def test_restatement_against_the_oracle_at_every_breakpoint(oracle):
    from vtkcloudpoint_amd import epstree as ET
    probes = 0
    for t, c, metric, k, eps_max in _clouds():
        tree, r = _tree(c, k, eps_max, metric)
        breaks, _ = ET.cluster_count_steps(tree)
        reach = np.unique(r["reach"][r["reach"] <= eps_max])
        breaks = np.unique(np.concatenate([breaks, reach]))
        eps_list = np.unique(np.concatenate([breaks, 0.5 * (breaks[1:] + breaks[:-1]), [eps_max]]))
        for eps in eps_list[eps_list <= eps_max].tolist():
            o = oracle.dbscan(c, eps, k, metric, literal=True)
            core = o["is_key"].astype(bool)
            cores, clusters, labelled = ET.counts_at(tree, eps)
            assert (cores, clusters, labelled) == (int(core.sum()), o["cf"], int((o["labels"] != 0).sum())), (t, eps)
            lab = ET.core_labels_at(tree, eps)
            assert np.array_equal(lab[core], o["labels"][core]) and not lab[~core].any(), (t, eps)
            probes += 1
    assert probes > 2000


def test_restatement_against_scipy():
    csgraph = pytest.importorskip("scipy.sparse.csgraph")
    rng = np.random.default_rng(7)
    for metric in (R.L1_2D, R.L2_2D, R.L2_3D):
        c = rng.uniform(0, 1, (120, 3))
        w, kd = R.w_matrix(c, 1, metric)                       # k = 1: kdist 0, w = d > 0 off the diagonal, all distinct
        off = w[np.triu_indices(120, 1)]
        assert (off > 0).all() and len(np.unique(off)) == len(off)
        r = R.eps_tree(c, 1, 10.0, metric)
        mst = csgraph.minimum_spanning_tree(np.triu(w, 1)).tocoo()
        assert np.array_equal(np.sort(mst.data), r["merge_w"]) and r["n_merge"] == 119


def test_the_emulated_rounds_equal_the_walk():
    """The device's round structure, emulated on the host slot for slot (eps_tree_ref.boruvka): the same forest as the
    Kruskal walk whatever the slot order, within floor(log2 |P|) rounds, with no cycle of hooks."""
    for t, c, metric, k, eps_max in _clouds():
        ref = R.eps_tree(c, k, eps_max, metric)
        for seed in (t, t + 100):
            w, a, b, rounds = R.boruvka(c, k, eps_max, metric, seed)
            assert np.array_equal(w.view(np.uint64), ref["merge_w"].view(np.uint64)), t
            assert np.array_equal(a, ref["merge_a"]) and np.array_equal(b, ref["merge_b"]), t
            assert rounds <= R.round_bound(ref["n_p"]) and (rounds == 0) == (ref["n_merge"] == 0), t


def test_hand_cases():
    from vtkcloudpoint_amd import epstree as ET
    # two points
    r = R.eps_tree([[0.0, 0.0], [3.0, 4.0]], 1, 10.0, R.L2_2D)
    assert r["merge_w"].tolist() == [5.0] and r["merge_a"].tolist() == [0] and r["merge_b"].tolist() == [1]
    assert r["kdist"].tolist() == [0.0, 0.0] and r["reach"].tolist() == [0.0, 0.0]
    r = R.eps_tree([[0.0, 0.0], [3.0, 4.0]], 2, 10.0, R.L1_2D)                 # k = 2: both turn core at 7
    assert r["kdist"].tolist() == [7.0, 7.0] and r["merge_w"].tolist() == [7.0] and r["reach"].tolist() == [7.0, 7.0]
    assert R.eps_tree([[0.0, 0.0], [3.0, 4.0]], 1, 4.5, R.L2_2D)["n_merge"] == 0
    # three collinear points, gaps 1 and 2
    tree, r = _tree([[0.0, 0.0], [1.0, 0.0], [3.0, 0.0]], 2, 5.0, R.L1_2D)
    assert r["kdist"].tolist() == [1.0, 1.0, 2.0]
    assert (r["merge_w"].tolist(), r["merge_a"].tolist(), r["merge_b"].tolist()) == ([1.0, 2.0], [0, 1], [1, 2])
    assert ET.counts_at(tree, 0.5) == (0, 0, 0) and ET.counts_at(tree, 1.0) == (2, 1, 2)
    assert ET.counts_at(tree, 2.0) == (3, 1, 3) and ET.counts_at(tree, 5.0) == (3, 1, 3)
    assert r["reach"].tolist() == [1.0, 1.0, 2.0]
    # identical points: a star on index 0, every w = 0
    r = R.eps_tree(np.full((6, 3), 2.5), 4, 1.0, R.L2_3D)
    assert not r["merge_w"].any() and r["merge_a"].tolist() == [0] * 5 and r["merge_b"].tolist() == [1, 2, 3, 4, 5]
    # a point that is never core below eps_max and still gets a label from a neighbour
    c = [[0.0, 0.0], [0.1, 0.0], [0.0, 0.1], [0.5, 0.0]]
    tree, r = _tree(c, 3, 0.45, R.L1_2D)
    assert r["kdist"][3] > 0.45 and r["reach"][3] == 0.4 and r["n_p"] == 3
    assert ET.counts_at(tree, 0.4) == (3, 1, 4) and ET.counts_at(tree, 0.39) == (3, 1, 3)
    assert ET.core_labels_at(tree, 0.4).tolist() == [1, 1, 1, 0]


def test_eps_for_clusters_on_a_tree_written_by_hand():
    from vtkcloudpoint_amd import epstree as ET
    # six points turn core at 1 1 1 1 2 2; merges at 3, 3.5, 6 and 7:
    # eps      [0,1) [1,2) [2,3) [3,3.5) [3.5,6) [6,7) [7,10]
    # clusters   0     4     6      5       4      3      2
    kd = [1.0, 1.0, 1.0, 1.0, 2.0, 2.0, np.inf]
    tree = ET.EpsTree(kd, kd, [3.0, 3.5, 6.0, 7.0], [0, 2, 0, 0], [1, 3, 2, 4], 10.0)
    breaks, clusters = ET.cluster_count_steps(tree)
    assert breaks.tolist() == [0.0, 1.0, 2.0, 3.0, 3.5, 6.0, 7.0] and clusters.tolist() == [0, 4, 6, 5, 4, 3, 2]
    assert ET.eps_for_clusters(tree, 4) == [(3.5, 6.0), (1.0, 2.0)]           # two plateaus, widest first
    assert ET.eps_for_clusters(tree, 2) == [(7.0, 10.0)]                      # the last one runs to eps_max
    assert ET.eps_for_clusters(tree, 5, tol=1) == [(1.0, 6.0)]                # 4 6 5 4: four steps, one interval
    assert ET.eps_for_clusters(tree, 6, tol=1) == [(2.0, 3.5)]
    assert ET.eps_for_clusters(tree, 1) == [] and ET.eps_for_clusters(tree, 9, tol=2) == []
    tie = ET.EpsTree([1.0, 1.0, 3.0], [1.0, 1.0, 3.0], [2.0, 4.0], [0, 0], [1, 2], 5.0)   # 0 2 1 2 1 on [0,1,2,3,4,5]
    assert ET.eps_for_clusters(tie, 1) == [(2.0, 3.0), (4.0, 5.0)]            # equal widths: the lower lo first
    c, m, lab = ET.counts_at(tree, np.array([0.5, 1.0, 3.25, 10.0]))
    assert c.tolist() == [0, 4, 6, 6] and m.tolist() == [0, 4, 5, 2] and lab.tolist() == [0, 4, 6, 6]
    assert ET.core_labels_at(tree, 6.5).tolist() == [1, 1, 1, 1, 2, 3, 0]
    for bad in (10.5, np.array([1.0, 11.0]), np.nan):
        with pytest.raises(ValueError):
            ET.counts_at(tree, bad)
    with pytest.raises(ValueError):
        ET.core_labels_at(tree, 10.5)
