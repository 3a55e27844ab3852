"""Timing of vcp_kdist_dev (exact k-distance) beside vcp_dbscan_dev on the same clouds.

Inputs on the device once; per case a warm-up call, then --reps calls each timed by host wall clock around the blocking
call (the library synchronises its stream before returning), median reported, plus the vcp_timing phases of the last
call.  Cases: C4 (10 M) L1_2D on motor and L2_3D on xyz for k in 4 / 7 / 10 / 32 / 64, a 10 M C5-shaped cloud, and
C4 plus six points at +-1e12.  One JSON line per case.
usage: python tools/bench_kdist.py [--n 10000000] [--reps 5]"""
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
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--ks", default="4,7,10,32,64")
    args = ap.parse_args()
    ctx = N.Context(0)
    ctx.timing_enable(True)
    c4 = synth.config_cloud(args.n)
    c5 = synth.config_c5(args.n)
    far = np.array([[1e12, 1e12], [-1e12, 1e12], [1e12, -1e12], [-1e12, -1e12], [1e12, 0.0], [5.0, -1e12]])
    cases = []
    for k in [int(v) for v in args.ks.split(",")]:
        cases.append(("C4", "L1_2D", c4["motor"], N.L1_2D, k, c4["eps_l1"]))
        cases.append(("C4", "L2_3D", c4["xyz"], N.L2_3D, k, c4["eps_l2"]))
    cases.append(("C5", "L1_2D", c5["motor"], N.L1_2D, 10, c5["eps_l1"]))
    cases.append(("C5", "L2_3D", c5["xyz"], N.L2_3D, 10, c5["eps_l2"]))
    cases.append(("C4+far", "L1_2D", np.concatenate([c4["motor"], far]), N.L1_2D, 10, c4["eps_l1"]))
    for name, mname, coords, metric, k, eps in cases:
        t = torch.from_numpy(np.ascontiguousarray(coords)).cuda()
        n, dim = t.shape
        kd = torch.empty(n, dtype=torch.float64, device="cuda")
        lab = torch.empty(n, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        ms = _median_ms(lambda: ctx.kdist_dev(t.data_ptr(), n, dim, k, kd.data_ptr(), metric=metric), args.reps)
        phases = {p: round(v, 4) for p, v in ctx.timing()}
        db = _median_ms(lambda: ctx.dbscan_dev(t.data_ptr(), n, dim, eps, k, metric, d_labels=lab.data_ptr()), args.reps)
        print(json.dumps(dict(cloud=name, metric=mname, n=int(n), k=k, kdist_ms=round(ms, 3), phases=phases,
                              dbscan_eps=eps, dbscan_ms=round(db, 3))), flush=True)
        del t, kd, lab
        torch.cuda.empty_cache()
    ctx.close()


if __name__ == "__main__":
    main()
