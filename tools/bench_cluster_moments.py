"""Timing of vcp_cluster_moments_dev beside vcp_centroids_dev and vcp_cluster_shapes_dev on the same labels.

One case, inputs resident on the device: the bench cloud (10 M points), labels from vcp_dbscan_dev (L1_2D on motor, the
headline eps and minPts): tens of thousands of clusters, most of them small, a few beyond one chunk of the summation tree.
Calls timed: centroids_dev (xyz and motor: what the pipeline runs today), cluster_shapes_dev on motor (circle, rectangle and
hull: the description the moments stand beside), cluster_moments_dev with dim 2 on motor, with dim 3 on xyz, with dim 2 on
the (X, Y) columns of xyz read in place (ld 3), and with dim 3 and int32 weights.  Per call a warm-up, then --reps timed
calls.  ms_events is the median of the sum of the call's vcp_timing phases (hipEvents on the stream the kernels run on);
ms_wall is the median host clock around the blocking call (read-backs and the final synchronise included).  gb_s is the
algorithmic bytes of the call (per labelled point 4 + 2 * 8 * dim, + 8 with weights; per point 4 for
its label and 4 for its slot in the sorted order) over ms_events: a figure for the whole call, grouping sort included, not a
kernel's share of peak.  One JSON line per call, appended to --out as well.
usage: python tools/bench_cluster_moments.py [--n 10000000] [--reps 5] [--out profiles/cluster_moments_bench.txt]"""
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


def _lib_ms(ctx, fn, reps):
    fn()
    ev, wall = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        wall.append((time.perf_counter() - t0) * 1e3)
        ev.append(sum(ms for _, ms in ctx.timing()))
    return float(np.median(ev)), float(np.median(wall)), {p: round(v, 3) for p, v in ctx.timing()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cluster_moments_bench.txt"))
    args = ap.parse_args()
    ctx = N.Context(0)
    ctx.timing_enable(True)
    n = args.n
    cloud = synth.config_cloud(n)
    motor = torch.from_numpy(np.ascontiguousarray(cloud["motor"])).cuda()
    xyz = torch.from_numpy(np.ascontiguousarray(cloud["xyz"])).cuda()
    labels = torch.empty(n, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    K = ctx.dbscan_dev(motor.data_ptr(), n, 2, cloud["eps_l1"], cloud["min_pts"], N.L1_2D, d_labels=labels.data_ptr())[0]
    weights = (1 + (torch.arange(n, device="cuda", dtype=torch.int64) * 2654435761 >> 7) % 5).to(torch.int32)
    z = lambda shape, dt=torch.float64: torch.empty(shape, dtype=dt, device="cuda")
    c3, c2, cc = z((K, 3)), z((K, 2)), z(K, torch.int64)
    cen, rad, val, hn = z((K, 2)), z(K), z(K, torch.uint8), z(K, torch.int32)
    rxy, rlen, redge, rval = z((K, 4, 2)), z((K, 2)), z(K, torch.int32), z(K, torch.uint8)
    hoff, hidx = z(K + 1, torch.int32), z(n, torch.int32)
    out = {d: dict(d_mean=z((K, d)), d_cov=z((K, d * (d + 1) // 2)), d_eval=z((K, d)), d_evec=z((K, d, d)), d_shape=z((K, 4)),
                   d_valid=z(K, torch.uint8), d_counts=z(K, torch.int64)) for d in (2, 3)}
    torch.cuda.synchronize()

    def moments(src, ld, dim, w=None):
        return lambda: ctx.cluster_moments_dev(src.data_ptr(), ld, dim, labels.data_ptr(), None if w is None else w.data_ptr(),
                                               n, K, **{k: v.data_ptr() for k, v in out[dim].items()})

    calls = [
        ("vcp_centroids_dev (xyz + motor)", None, lambda: ctx.centroids_dev(xyz.data_ptr(), motor.data_ptr(), labels.data_ptr(), n, K,
                                                                           c3.data_ptr(), c2.data_ptr(), cc.data_ptr())),
        ("vcp_cluster_shapes_dev (motor; circle, rectangle, hull)", None,
         lambda: ctx.cluster_shapes_dev(motor.data_ptr(), labels.data_ptr(), None, n, n, K, cen.data_ptr(), rad.data_ptr(),
                                        val.data_ptr(), hn.data_ptr(), rxy.data_ptr(), rlen.data_ptr(), redge.data_ptr(),
                                        rval.data_ptr(), hoff.data_ptr(), hidx.data_ptr())),
        ("vcp_cluster_moments_dev dim 2 (motor)", (2, 0), moments(motor, 2, 2)),
        ("vcp_cluster_moments_dev dim 2 (X, Y of xyz, ld 3)", (2, 0), moments(xyz, 3, 2)),
        ("vcp_cluster_moments_dev dim 3 (xyz)", (3, 0), moments(xyz, 3, 3)),
        ("vcp_cluster_moments_dev dim 3 (xyz), int32 weights", (3, 8), moments(xyz, 3, 3, weights)),
    ]
    lines, base = [], None
    head = dict(case="C4", n=n, K=K)
    for name, alg, fn in calls:
        try:
            ev, wall, ph = _lib_ms(ctx, fn, args.reps)
        except N.VcpError as e:
            lines.append(dict(head, run=name, error=str(e)))
            print(json.dumps(lines[-1]), flush=True)
            if e.code == -7:
                break              # a HIP runtime error: nothing more is started on this device
            continue
        ln = dict(head, run=name, ms_events=round(ev, 3), ms_wall=round(wall, 3), phases=ph)
        if base is None:
            base = ev
            sizes = cc.cpu().numpy()
            head["sizes"] = dict(min=int(sizes.min()), median=float(np.median(sizes)), max=int(sizes.max()),
                                 in_no_cluster=int(n - sizes.sum()))
            ln["sizes"] = head["sizes"]
        else:
            ln["ratio_to_centroids_dev"] = round(ev / base, 3)
        if alg is not None:
            members = int(n - head["sizes"]["in_no_cluster"])
            nbytes = 8 * n + members * (4 + 2 * 8 * alg[0] + alg[1])
            ln["algorithmic_bytes"] = nbytes
            ln["gb_s"] = round(nbytes / (ev * 1e-3) / 1e9, 1)
        lines.append(ln)
        print(json.dumps(ln), flush=True)
    ctx.close()
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(json.dumps(ln) for ln in lines) + "\n")


if __name__ == "__main__":
    main()
