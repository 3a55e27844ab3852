"""Timing of the cluster shapes and the cluster filter beside vcp_mcc on the headline workload.

synth.config_cloud(n) clustered by vcp_dbscan_blocks at the bench's parameters (eps 0.07, minPts 7, 200 points per
block); then per case a warm-up call and the median of --reps blocking calls (host wall clock around the call: the
library synchronises its stream before returning), plus the vcp_timing phases of the last call:
  mcc_host      vcp_mcc from host arrays (uploads the points, labels and order)
  shapes_dev    vcp_cluster_shapes_dev from device arrays, every output
  circles_dev   the same without rectangle and hull outputs
  filter_dev    vcp_cluster_filter_dev (median radius, aspect 2), keep and kept_idx written
  label_copy    a plain device copy of the label array, for scale
One JSON line per case.
usage: python tools/bench_shapes.py [--n 10000000] [--reps 5]"""
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
    return float(np.median(ts)), [round(t, 3) for t in ts]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    ctx = N.Context(0)
    ctx.timing_enable(True)
    motor = np.ascontiguousarray(synth.config_cloud(args.n)["motor"])
    r = ctx.dbscan_blocks(motor, 0.07, 7, 200, 3)
    labels, order, K = r["labels"], r["order"], r["cluster_amount"]
    n, m = len(labels), len(order)
    base = dict(n=n, m=m, K=K)

    def report(case, fn, **extra):
        ms, all_ms = _median_ms(fn, args.reps)
        phases = {p: round(v, 4) for p, v in ctx.timing()}
        print(json.dumps(dict(case=case, ms=round(ms, 3), runs=all_ms, phases=phases, **base, **extra)), flush=True)
        return ms

    a = report("mcc_host", lambda: ctx.mcc(motor, labels, K, order))

    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    d_xy, d_lab, d_ord = dev(motor), dev(labels), dev(order)
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device="cuda")
    cen, rad, val, hn = z((K, 2), torch.float64), z(K, torch.float64), z(K, torch.uint8), z(K, torch.int32)
    rxy, rlen, redge, rval = z((K, 8), torch.float64), z((K, 2), torch.float64), z(K, torch.int32), z(K, torch.uint8)
    hoff, hidx = z(K + 1, torch.int32), z(max(m, 1), torch.int32)
    torch.cuda.synchronize()
    head = (d_xy.data_ptr(), d_lab.data_ptr(), d_ord.data_ptr(), m, n, K, cen.data_ptr(), rad.data_ptr(), val.data_ptr(),
            hn.data_ptr())
    b = report("shapes_dev", lambda: ctx.cluster_shapes_dev(*head, rxy.data_ptr(), rlen.data_ptr(), redge.data_ptr(),
                                                             rval.data_ptr(), hoff.data_ptr(), hidx.data_ptr()))
    print(json.dumps(dict(case="mcc_host - shapes_dev", ms=round(a - b, 3))), flush=True)
    report("circles_dev", lambda: ctx.cluster_shapes_dev(*head))

    v = val.cpu().numpy() == 1
    med = float(np.median(rad.cpu().numpy()[v])) if v.any() else 0.0
    filt, keep, kidx = z(K, torch.uint8), z(n, torch.uint8), z(max(n, 1), torch.int32)
    torch.cuda.synchronize()
    counts = []
    f = report("filter_dev", lambda: counts.append(ctx.cluster_filter_dev(
        d_lab.data_ptr(), n, K, rad.data_ptr(), val.data_ptr(), rlen.data_ptr(), rval.data_ptr(), med, 2.0, filt.data_ptr(),
        keep.data_ptr(), kidx.data_ptr())), max_radius=med, max_aspect=2.0)
    d_copy = torch.empty_like(d_lab)

    def copy():
        d_copy.copy_(d_lab)
        torch.cuda.synchronize()

    c, runs = _median_ms(copy, args.reps)
    print(json.dumps(dict(case="label_copy", ms=round(c, 3), runs=runs, filter_over_copy=round(f / c, 2),
                          n_filtered=counts[-1][0], n_kept=counts[-1][1], **base)), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
