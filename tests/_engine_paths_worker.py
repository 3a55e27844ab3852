"""Worker of tests/test_engine_paths_gpu.py: the whole case table (tests/engine_path_cases.py) on the device, in a process
of its own because the engine's switches are read once per process.  The parent sets VCP_TRACE and the switch under test.

For every case: `@@ begin NAME` on stderr, the call (whose trace lines follow on stderr, each written whole), the
comparison of labels, is_core, is_classed, cf and evals with the CPU oracle for equality, then `@@ end NAME ok` or
`@@ end NAME FAIL <what differed>`.  The markers go through the same unbuffered descriptor as the trace, so the parent
reads which launches belong to which case.

usage: _engine_paths_worker.py [SUBSTRING ...]    (only the cases whose name contains one of the substrings)
exit status: 0 = every comparison held, 1 = some case differs from the oracle; anything else ends the parent's module (a
HIP error ends the worker at once, with status 3: nothing more is started on a device that reported one)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import engine_path_cases as T  # noqa: E402


def mark(text):
    os.write(2, (text + "\n").encode())


def same(g, o, core="is_core", classed="is_classed"):
    assert np.array_equal(g["labels"], o["labels"]), "labels differ at %d points (first: %r)" % (
        int((g["labels"] != o["labels"]).sum()), np.flatnonzero(g["labels"] != o["labels"])[:5].tolist())
    assert np.array_equal(g[core], o["is_key"]), "is_core differs at %d points" % int((g[core] != o["is_key"]).sum())
    assert np.array_equal(g[classed], o["classed"]), "is_classed differs at %d points" % int(
        (g[classed] != o["classed"]).sum())
    assert g["cf"] == o["cf"], "cf %d != %d" % (g["cf"], o["cf"])
    assert g["evals"] == o["evals"], "evals %d != %d" % (g["evals"], o["evals"])


def run_engine(inp, ctxs, O, N):
    kw = dict(cf_in=inp.get("cf_in", 0), in_classed=inp.get("in_classed"), labels=inp.get("labels"))
    g = ctxs[0].dbscan(inp["coords"], inp["eps"], inp["min_pts"], inp["metric"], **kw)
    o = O.dbscan(inp["coords"], inp["eps"], inp["min_pts"], inp["metric"], kw["cf_in"], kw["in_classed"], kw["labels"])
    same(g, o)


def run_blocks(inp, ctxs, O, N):
    g = ctxs[0].dbscan_blocks(inp["motor"], inp["eps"], inp["min_pts"], inp["pts_in_cell"], 3)
    o = O.block_pipeline(inp["motor"], inp["eps"], inp["min_pts"], inp["pts_in_cell"], 3)
    for k in ("labels", "block_of", "order"):
        assert np.array_equal(g[k], o[k]), "%s differs" % k
    for k in ("rows", "cols", "kept", "del_sum", "cluster_amount", "evals"):
        assert g[k] == o[k], "%s %r != %r" % (k, g[k], o[k])


def run_slabs(inp, ctxs, O, N):
    import torch
    from vtkcloudpoint_amd import distributed as D
    if len(ctxs) < 2:
        ctxs.append(N.Context(0))
    pts, cuts = inp["coords"], inp["cuts"]
    parts = [torch.from_numpy(np.ascontiguousarray(pts[a:b])).cuda() for a, b in zip(cuts, cuts[1:])]
    res = D.exact_slabs_local(ctxs[:2], parts, inp["eps"], inp["min_pts"], inp["metric"], 0)
    o = O.dbscan(pts, inp["eps"], inp["min_pts"], inp["metric"])
    whole = {k: np.concatenate([r[k].cpu().numpy() for r in res]) for k in ("labels", "is_core", "is_classed")}
    for r in res:  # every rank reports the totals of the whole list
        same(dict(whole, cf=r["cf"], evals=r["dist_evals"]), o)


RUN = {"engine": run_engine, "blocks": run_blocks, "slabs": run_slabs}


def main():
    from oracle import binding as O
    from vtkcloudpoint_amd import _native as N
    O.build()
    only = sys.argv[1:]
    ctxs = [N.Context(0)]
    bad = 0
    for case in T.CASES:
        if only and not any(s in case.name for s in only):
            continue
        mark("@@ begin " + case.name)
        try:
            RUN[case.kind](case.build(), ctxs, O, N)
            mark("@@ end %s ok" % case.name)
        except AssertionError as e:
            bad += 1
            mark("@@ end %s FAIL %s" % (case.name, " ".join(str(e).split())))
        except N.VcpError as e:
            mark("@@ end %s FAIL %s" % (case.name, " ".join(str(e).split())))
            if e.code == -7:  # VCP_ERR_HIP: the device reported an error; nothing more runs on it from here
                os._exit(3)
            bad += 1
    for c in ctxs:
        c.close()
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
