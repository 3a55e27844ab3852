"""Timing of vcp_gdbscan_dev (DBSCAN with point weights and a range gate) beside vcp_dbscan_dev on the same cloud.

The C4 cloud (10 M points, L1_2D on motor, the headline eps 0.1 and minPts 10), inputs resident on the device.  Four runs:
unit weights and no gate (what vcp_dbscan_dev computes: labels and core flags are compared), weights 1..3, a gate of 0.5 on
a synthetic Distance in two range layers (5 + u/2 and 9 + u/2), and both.  Per run a warm-up call, then --reps calls timed by
host wall clock around the blocking call, median reported, plus the vcp_timing phases of the last call.  vcp_dbscan_dev is
timed the same way (dbscan.hip is the engine this project's bench.py measures; this change does not touch it).  One JSON
line per run, appended to --out as well.
usage: python tools/bench_gdbscan.py [--n 10000000] [--reps 3] [--out profiles/gdbscan_bench.txt]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from vtkcloudpoint_amd import _native as N  # noqa: E402
from vtkcloudpoint_amd import synth  # noqa: E402


def _median_ms(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gdbscan_bench.txt"))
    args = ap.parse_args()
    ctx = N.Context(0)
    cloud = synth.config_cloud(args.n)
    eps, min_pts = cloud["eps_l1"], cloud["min_pts"]
    n = args.n
    t = torch.from_numpy(np.ascontiguousarray(cloud["motor"])).cuda()
    w = torch.from_numpy((1 + (synth.splitmix64(91, 0, n) % np.uint64(3))).astype(np.int32)).cuda()
    layer = np.where(synth.uniform01(92, 0, n) < 0.5, 5.0, 9.0) + 0.5 * synth.uniform01(93, 0, n)
    aux = torch.from_numpy(layer).cuda()
    lab = torch.empty(n, dtype=torch.int32, device="cuda")
    core = torch.empty(n, dtype=torch.uint8, device="cuda")
    lab0 = torch.empty(n, dtype=torch.int32, device="cuda")
    core0 = torch.empty(n, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    res = {}

    def engine():
        res["cf"] = ctx.dbscan_dev(t.data_ptr(), n, 2, eps, min_pts, N.L1_2D, d_labels=lab0.data_ptr(),
                                   d_is_core=core0.data_ptr())[0]

    ctx.timing_enable(True)
    db_ms = _median_ms(engine, args.reps)
    line = dict(cloud="C4", n=n, metric="L1_2D", eps=eps, min_pts=min_pts, run="vcp_dbscan_dev", ms=round(db_ms, 3),
                clusters=res["cf"], phases={p: round(v, 3) for p, v in ctx.timing()})
    print(json.dumps(line), flush=True)
    lines = [json.dumps(line)]
    for name, dw, da in (("unit weights, no gate", None, None), ("weights 1..3", w, None), ("gate 0.5 on Distance", None, aux),
                         ("weights 1..3 and gate", w, aux)):
        def call():
            res["cf"] = ctx.gdbscan_dev(t.data_ptr(), n, 2, eps, min_pts, lab.data_ptr(), N.L1_2D,
                                        d_weights=None if dw is None else dw.data_ptr(),
                                        d_aux=None if da is None else da.data_ptr(), gate=0.5, d_is_core=core.data_ptr())

        ms = _median_ms(call, args.reps)
        line = dict(cloud="C4", n=n, metric="L1_2D", eps=eps, min_weight=min_pts, run=name, ms=round(ms, 3),
                    ratio_to_vcp_dbscan_dev=round(ms / db_ms, 3), clusters=res["cf"], cores=int(core.sum().item()),
                    phases={p: round(v, 3) for p, v in ctx.timing()})
        if dw is None and da is None:
            line["equals_vcp_dbscan_dev"] = bool(torch.equal(lab, lab0) and torch.equal(core, core0))
        print(json.dumps(line), flush=True)
        lines.append(json.dumps(line))
    ctx.close()
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
