"""Timing of vcp_cluster_quantiles_dev and vcp_cluster_mad_dev beside vcp_centroids_dev on the same labels, and beside the
alternative that needs no select: a device sort of (label, key) pairs.

Two cases, inputs resident on the device:
  C4       the bench cloud (10 M points), labels from vcp_dbscan_dev (L1_2D on motor, the headline eps and minPts), the
           value = the Distance |xyz| of every point: tens of thousands of clusters of a few hundred points
  files    20 groups of 500 000 rows (fixed-point files): every group in the large class
Calls timed: cluster_quantiles_dev with q = (0, 0.5, 1), cluster_mad_dev (c = 3, floor = 0), centroids_dev (xyz and motor),
and the sort route in torch: the key map, torch.sort of the keys, a stable torch.sort of the labels in that order,
torch.bincount and one gather per rank -- whose result is compared with cluster_quantiles_dev's bit for bit.
Per call a warm-up, then --reps timed calls.  ms_events is the median of the sum of the call's vcp_timing phases (hipEvents
on the stream the kernels run on) for the library calls and of torch.cuda.Event pairs for the sort route; ms_wall is the
median host clock around the blocking call (the read-backs and, for the library, the final synchronise included).  One JSON
line per call, appended to --out as well.
usage: python tools/bench_cluster_quantiles.py [--n 10000000] [--reps 5] [--out profiles/cluster_quantiles_bench.txt]"""
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

Q = [0.0, 0.5, 1.0]
SIGN = -(1 << 63)


def _lib_ms(ctx, fn, reps):
    fn()
    ev, wall = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        wall.append((time.perf_counter() - t0) * 1e3)
        ev.append(sum(ms for _, ms in ctx.timing()))
    return float(np.median(ev)), float(np.median(wall)), {p: round(v, 3) for p, v in ctx.timing()}


def _torch_ms(fn, reps):
    fn()
    torch.cuda.synchronize()
    ev, wall = [], []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
        ev.append(a.elapsed_time(b))
    return float(np.median(ev)), float(np.median(wall))


def sort_route(values, labels, K):
    """out [K, 3] by sorting: the keys as int64 in the order of vcp.h, sorted; the labels in that order, sorted stably;
    the rank floor(q (c - 1)) of every group read from its segment."""
    u = values.view(torch.int64)
    key = torch.where(u < 0, ~u, u ^ SIGN) ^ SIGN                    # unsigned key order as signed int64 order
    key = torch.where(torch.isnan(values), torch.full_like(key, (1 << 63) - 1), key)
    skey, idx = torch.sort(key)
    slab, idx2 = torch.sort(labels[idx].to(torch.int64), stable=True)
    skey = skey[idx2]
    counts = torch.bincount(slab, minlength=K + 1)[: K + 1]
    start = torch.cumsum(counts, 0) - counts
    c = counts[1:].to(torch.float64)
    out = torch.full((K, len(Q)), float("nan"), dtype=torch.float64, device=values.device)
    has = counts[1:] > 0
    for j, q in enumerate(Q):
        r = torch.floor(q * (c - 1)).to(torch.int64).clamp(min=0)
        k = skey[(start[1:] + r).clamp(max=len(skey) - 1)] ^ SIGN      # back to the unsigned key
        v = torch.where(k < 0, k ^ SIGN, ~k).view(torch.float64)
        v = torch.where(k == -1, torch.full_like(v, float("nan")), v)
        out[:, j] = torch.where(has, v, out[:, j])
    return out


def run_case(ctx, name, values, labels, K, xyz, motor, reps):
    n = labels.numel()
    nq = len(Q)
    out = torch.empty((K, nq), dtype=torch.float64, device="cuda")
    cnt = torch.empty(K, dtype=torch.int64, device="cuda")
    med, mad, thr = (torch.empty(K, dtype=torch.float64, device="cuda") for _ in range(3))
    rej = torch.empty(n, dtype=torch.uint8, device="cuda")
    kept = torch.empty(K, dtype=torch.int64, device="cuda")
    c3 = torch.empty((K, 3), dtype=torch.float64, device="cuda")
    c2 = torch.empty((K, 2), dtype=torch.float64, device="cuda")
    cc = torch.empty(K, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    res = {}

    def quant():
        ctx.cluster_quantiles_dev(values.data_ptr(), 1, labels.data_ptr(), n, K, Q, out.data_ptr(), cnt.data_ptr())

    def madc():
        res["nr"] = ctx.cluster_mad_dev(values.data_ptr(), 1, labels.data_ptr(), n, K, 3.0, 0.0, med.data_ptr(),
                                        mad.data_ptr(), thr.data_ptr(), rej.data_ptr(), kept.data_ptr())

    def cent():
        ctx.centroids_dev(xyz.data_ptr(), None if motor is None else motor.data_ptr(), labels.data_ptr(), n, K,
                          c3.data_ptr(), None if motor is None else c2.data_ptr(), cc.data_ptr())

    def sortr():
        res["sorted"] = sort_route(values, labels, K)

    head = dict(case=name, n=n, K=K, q=Q)
    ce, cw, cph = _lib_ms(ctx, cent, reps)
    qe, qw, qph = _lib_ms(ctx, quant, reps)
    me, mw, mph = _lib_ms(ctx, madc, reps)
    se, sw = _torch_ms(sortr, reps)
    sizes = cnt.cpu().numpy()
    head["sizes"] = dict(min=int(sizes.min()), median=float(np.median(sizes)), max=int(sizes.max()),
                         in_no_group=int(n - sizes.sum()))
    same = bool(torch.equal(res["sorted"].view(torch.int64), out.view(torch.int64)))
    lines = [
        dict(head, run="vcp_centroids_dev", ms_events=round(ce, 3), ms_wall=round(cw, 3), phases=cph),
        dict(head, run="vcp_cluster_quantiles_dev", ms_events=round(qe, 3), ms_wall=round(qw, 3), phases=qph,
             ratio_to_centroids_dev=round(qe / ce, 3), ratio_to_sort_route=round(qe / se, 3)),
        dict(head, run="vcp_cluster_mad_dev", ms_events=round(me, 3), ms_wall=round(mw, 3), phases=mph,
             ratio_to_centroids_dev=round(me / ce, 3), rejected=int(res["nr"])),
        dict(head, run="sort route (torch.sort x 2, bincount, gathers)", ms_events=round(se, 3), ms_wall=round(sw, 3),
             equals_cluster_quantiles_dev=same, select_beats_sort=bool(qe < se)),
    ]
    for ln in lines:
        print(json.dumps(ln), flush=True)
    return [json.dumps(ln) for ln in lines]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--files", type=int, default=20)
    ap.add_argument("--rows", type=int, default=500_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cluster_quantiles_bench.txt"))
    args = ap.parse_args()
    ctx = N.Context(0)
    ctx.timing_enable(True)
    lines = []
    # C4: the bench cloud with its DBSCAN labels
    n = args.n
    cloud = synth.config_cloud(n)
    motor = torch.from_numpy(np.ascontiguousarray(cloud["motor"])).cuda()
    xyz = torch.from_numpy(np.ascontiguousarray(cloud["xyz"])).cuda()
    labels = torch.empty(n, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    K = ctx.dbscan_dev(motor.data_ptr(), n, 2, cloud["eps_l1"], cloud["min_pts"], N.L1_2D, d_labels=labels.data_ptr())[0]
    dist = torch.linalg.vector_norm(xyz, dim=1).contiguous()
    lines += run_case(ctx, "C4", dist, labels, K, xyz, motor, args.reps)
    del motor, xyz, labels, dist
    # files: groups of one fixed target each, at different ranges, 2 % far rows
    F, m = args.files, args.rows
    g = np.repeat(np.arange(1, F + 1, dtype=np.int32), m)
    d = 5.0 + 30.0 * (g - 1) + 0.02 * synth.normal(71, 0, F * m)
    far = synth.uniform01(72, 0, F * m) < 0.02
    d[far] += 3.0 + 5.0 * synth.uniform01(73, 0, F * m)[far]
    pxyz = np.c_[d, 0.5 * d, 0.25 * d]
    lines += run_case(ctx, "files", torch.from_numpy(d).cuda(), torch.from_numpy(g).cuda(), F,
                      torch.from_numpy(np.ascontiguousarray(pxyz)).cuda(), None, args.reps)
    ctx.close()
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
