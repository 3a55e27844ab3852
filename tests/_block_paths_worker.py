"""Worker of tests/test_block_paths_gpu.py: the whole case table (tests/block_path_cases.py) on the device, in a process of
its own because the pipeline's switches are read once per process.  The parent sets VCP_TRACE and the switch under test.

Every case runs twice on one context.  `@@ begin NAME` ... `@@ end NAME ok`: the one public call, Context.dbscan_blocks.
`@@ begin NAME/staged` ... `@@ end NAME/staged ok`: the stages one by one -- blocks_begin, blocks_share for a world of three
with blocks_cluster_dev on every share, blocks_finish_local (the sharded finish's first stage, whose loop repeats the final
order itself when a block's ids overflow the table) and blocks_finish_dev (the whole finish, which repeats it through its
`again` path).  Both forms are compared with the CPU oracle for equality: labels, block_of, order, rows, cols, kept, del_sum,
cluster_amount and evals; the position cases also with the numpy restatement's block_of, order and position labels; an error
case by its error code.  The trace lines of a call follow its `begin` marker on the same unbuffered descriptor, so the
parent reads which lines belong to which case.

usage: _block_paths_worker.py [SUBSTRING ...]    (only the cases whose name contains one of the substrings)
exit status: 0 = every comparison held, 1 = some case differs; anything else ends the parent's module (a HIP error ends the
worker at once, with status 3: nothing more is started on a device that reported one)."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import block_path_cases as T  # noqa: E402

ARRAYS, SCALARS = ("labels", "block_of", "order"), ("rows", "cols", "kept", "del_sum", "cluster_amount", "evals")


def mark(text):
    os.write(2, (text + "\n").encode())


def same(g, o):
    for k in ARRAYS:
        assert np.array_equal(g[k], o[k]), "%s differs from the oracle at %d places (first: %r)" % (
            k, int((g[k] != o[k]).sum()) if g[k].shape == o[k].shape else -1,
            np.flatnonzero(g[k] != o[k])[:5].tolist() if g[k].shape == o[k].shape else [g[k].shape, o[k].shape])
    for k in SCALARS:
        assert g[k] == o[k], "%s %r != %r" % (k, g[k], o[k])


def same_positions(g, inp):
    P = T.ref_partition(inp.get("key_xy", inp["motor"]), inp["pts_in_cell"])
    assert np.array_equal(g["block_of"], P["block_of"]), "block_of differs from the restated partition"
    assert np.array_equal(g["order"], P["order"]), "order is not the block-major list by (block, d, index)"
    lab = T.position_labels(P, len(inp["motor"]))
    assert np.array_equal(g["labels"], lab), "labels != 1 + position at %d points (first: %r)" % (
        int((g["labels"] != lab).sum()), np.flatnonzero(g["labels"] != lab)[:5].tolist())


def one_shot(ctx, inp):
    return ctx.dbscan_blocks(inp["motor"], inp["eps"], inp["min_pts"], inp["pts_in_cell"], inp["small_max"],
                             key_xy=inp.get("key_xy"))


def staged(ctx, inp):
    import torch
    info = ctx.blocks_begin(inp["motor"], inp["eps"], inp["min_pts"], inp["pts_in_cell"], inp["small_max"],
                            key_xy=inp.get("key_xy"))
    m, n = info["m"], len(inp["motor"])
    local = torch.zeros(max(m, 1), dtype=torch.int32, device="cuda")
    evals = covered = 0
    for r in range(3):  # three "ranks" on one GPU: contiguous block ranges balanced on the point count
        lo, hi, plo, phi = ctx.blocks_share(r, 3)
        assert plo == covered, "the shares do not adjoin"
        covered = phi
        evals += ctx.blocks_cluster_dev(lo, hi, local.data_ptr())
    assert covered == m
    first = ctx.blocks_finish_local(local.data_ptr())
    labels = torch.zeros(n, dtype=torch.int32, device="cuda")
    block_of = torch.zeros(n, dtype=torch.int32, device="cuda")
    order = torch.zeros(max(m, 1), dtype=torch.int64, device="cuda")
    out = ctx.blocks_finish_dev(local.data_ptr(), evals, labels.data_ptr(), block_of.data_ptr(), order.data_ptr())
    assert first["kept"] == out["kept"] and first["clusters"] == out["kept"] + out["del_sum"] and first["m"] == m, \
        "the sharded finish's first stage and the whole finish disagree: %r, %r" % (first, out)
    out.update(labels=labels.cpu().numpy(), block_of=block_of.cpu().numpy(), order=order.cpu().numpy()[:m],
               rows=info["rows"], cols=info["cols"])
    return out


def run(ctx, inp, o, call, N, O):
    if isinstance(o, O.OracleError):
        try:
            call(ctx, inp)
        except N.VcpError as e:
            if e.code == -7:
                raise
            assert e.code == o.code, "error code %d, the oracle's is %d" % (e.code, o.code)
            return
        raise AssertionError("no error, the oracle's is %d" % o.code)
    g = call(ctx, inp)
    same(g, o)
    if inp["kind"] == "position":
        same_positions(g, inp)


def main():
    from oracle import binding as O
    from vtkcloudpoint_amd import _native as N
    O.build()
    only = sys.argv[1:]
    ctx = N.Context(0)
    bad = 0
    t0 = time.time()
    for case in T.CASES:
        if only and not any(s in case.name for s in only):
            continue
        inp = case.build()
        try:
            o = O.block_pipeline(inp["motor"], inp["eps"], inp["min_pts"], inp["pts_in_cell"], inp["small_max"],
                                 key_xy=inp.get("key_xy"))
        except O.OracleError as e:
            o = e
        for name, call in ((case.name, one_shot), (case.name + "/staged", staged)):
            mark("@@ begin " + name)
            try:
                run(ctx, inp, o, call, N, O)
                mark("@@ end %s ok" % name)
            except AssertionError as e:
                bad += 1
                mark("@@ end %s FAIL %s" % (name, " ".join(str(e).split())))
            except N.VcpError as e:
                mark("@@ end %s FAIL %s" % (name, " ".join(str(e).split())))
                if e.code == -7:  # VCP_ERR_HIP: the device reported an error; nothing more runs on it from here
                    os._exit(3)
                bad += 1
    ctx.close()
    mark("@@ wall %.1f" % (time.time() - t0))
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
