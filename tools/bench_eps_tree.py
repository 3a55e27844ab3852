"""Timing of vcp_eps_tree_dev (DBSCAN's cluster count at every eps <= eps_max in one call) beside what the library offered
for the same question before: vcp_kdist_dev once plus one vcp_dbscan_dev per eps.

The C4 family of tools/bench_kdist.py at 1 M and 10 M points: L1_2D on motor with eps_max 0.2 and L2_3D on xyz with eps_max
1.0, k = 7.  Inputs on the device once; per case a warm-up call, then --reps calls timed by host wall clock around the
blocking call, median reported, plus the vcp_timing phases and `rounds` of the last call.  Beside it vcp_kdist_dev and
vcp_dbscan_dev at E = --eps-count values of eps spread evenly up to eps_max, and the E at which the two cost the same:
(tree - kdist) / (mean dbscan call).  One JSON line per case, appended to --out as well.
usage: python tools/bench_eps_tree.py [--sizes 1000000,10000000] [--reps 3] [--out profiles/eps_tree_bench.txt]"""
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


def _median_ms(fn, reps, warm=True):
    if warm:
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1000000,10000000")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--k", type=int, default=7)
    ap.add_argument("--eps-count", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eps_tree_bench.txt"))
    args = ap.parse_args()
    ctx = N.Context(0)
    k = args.k
    lines = []
    for n in [int(v) for v in args.sizes.split(",")]:
        cloud = synth.config_cloud(n)
        for mname, coords, metric, eps_max in (("L1_2D", cloud["motor"], N.L1_2D, 0.2), ("L2_3D", cloud["xyz"], N.L2_3D, 1.0)):
            t = torch.from_numpy(np.ascontiguousarray(coords)).cuda()
            n, dim = t.shape
            kd = torch.empty(n, dtype=torch.float64, device="cuda")
            reach = torch.empty(n, dtype=torch.float64, device="cuda")
            mw = torch.empty(n, dtype=torch.float64, device="cuda")
            ma = torch.empty(n, dtype=torch.int32, device="cuda")
            mb = torch.empty(n, dtype=torch.int32, device="cuda")
            lab = torch.empty(n, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            out = {}

            def tree():
                out["m"], out["rounds"] = ctx.eps_tree_dev(t.data_ptr(), n, dim, k, eps_max, mw.data_ptr(), ma.data_ptr(),
                                                           mb.data_ptr(), kd.data_ptr(), reach.data_ptr(), metric=metric)

            ctx.timing_enable(True)
            tree_ms = _median_ms(tree, args.reps)
            phases = {p: round(v, 3) for p, v in ctx.timing()}
            ctx.timing_enable(False)
            kd_ms = _median_ms(lambda: ctx.kdist_dev(t.data_ptr(), n, dim, k, kd.data_ptr(), metric=metric), args.reps)
            eps_list = [eps_max * (i + 1) / args.eps_count for i in range(args.eps_count)]
            db_ms, cf = [], []
            for eps in eps_list:
                res = {}

                def db():
                    res["cf"] = ctx.dbscan_dev(t.data_ptr(), n, dim, eps, k, metric, d_labels=lab.data_ptr())[0]

                db_ms.append(_median_ms(db, 1))
                cf.append(res["cf"])
            # the same counts from the tree's arrays
            kdh, mwh = kd.cpu().numpy(), mw[: out["m"]].cpu().numpy()
            tree_cf = [int((kdh <= e).sum() - (mwh <= e).sum()) for e in eps_list]
            mean_db = float(np.mean(db_ms))
            line = dict(cloud="C4", metric=mname, n=int(n), k=k, eps_max=eps_max, eps_tree_ms=round(tree_ms, 3),
                        phases=phases, rounds=out["rounds"], n_merge=int(out["m"]), kdist_ms=round(kd_ms, 3),
                        dbscan_eps=[round(e, 6) for e in eps_list], dbscan_ms=[round(v, 3) for v in db_ms],
                        per_eps_path_ms=round(kd_ms + sum(db_ms), 3), break_even_E=round((tree_ms - kd_ms) / mean_db, 2),
                        clusters=cf, counts_agree=tree_cf == cf)
            print(json.dumps(line), flush=True)
            lines.append(json.dumps(line))
            del t, kd, reach, mw, ma, mb, lab
            torch.cuda.empty_cache()
    ctx.close()
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
