"""Timing of vcp_cluster_spheres_dev beside vcp_centroids_dev and vcp_cluster_moments_dev on the same labels, in one run.

One case, inputs resident on the device: the bench cloud (10 M points), labels from vcp_dbscan_dev (L1_2D on motor, the
headline eps and minPts): tens of thousands of clusters, most of them small, a few beyond one chunk of the summation tree.
Calls timed: centroids_dev (xyz and motor), cluster_moments_dev with dim 2 on motor and dim 3 on xyz, then
cluster_spheres_dev with dim 2 on motor and dim 3 on xyz, the radius free and fixed, at rounds 0, 4 and 12.  The clusters of
the bench cloud are not spheres and the fixed radius is an arbitrary 0.05: every cluster runs every round whatever its
data, so the time does not depend on what is fitted.  Per call a warm-up, then --reps timed calls.  ms_events is the median
of the sum of the call's vcp_timing phases (hipEvents on the stream the kernels run on); ms_wall is the median host clock
around the blocking call.  After the calls one line per (dim, radius) gives ms_per_round = (ms_events at 12 rounds - at 0) /
12 and the same from 4 rounds, beside the moments_cov phase of cluster_moments_dev of the same dim: that phase is one
gather pass through sorted[] over the same members with one per-cluster kernel behind it, a round is one contiguous pass
over d with one per-cluster kernel behind it.  One JSON line per call, appended to --out as well.
usage: python tools/bench_cluster_spheres.py [--n 10000000] [--reps 5] [--out profiles/cluster_spheres_bench.txt]"""
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

ROUNDS = (0, 4, 12)
FIXED = 0.05


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cluster_spheres_bench.txt"))
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
    z = lambda shape, dt=torch.float64: torch.empty(shape, dtype=dt, device="cuda")
    c3, c2, cc = z((K, 3)), z((K, 2)), z(K, torch.int64)
    mom = {d: dict(d_mean=z((K, d)), d_cov=z((K, d * (d + 1) // 2)), d_eval=z((K, d)), d_evec=z((K, d, d)), d_shape=z((K, 4)),
                   d_valid=z(K, torch.uint8), d_counts=z(K, torch.int64)) for d in (2, 3)}
    sph = {d: dict(d_centre=z((K, d)), d_radius=z(K), d_rms=z(K), d_cap=z(K), d_step=z(K), d_alg=z((K, d + 1)),
                   d_valid=z(K, torch.uint8), d_counts=z(K, torch.int64)) for d in (2, 3)}
    src = {2: (motor, 2), 3: (xyz, 3)}
    torch.cuda.synchronize()

    def moments(dim):
        a, ld = src[dim]
        return lambda: ctx.cluster_moments_dev(a.data_ptr(), ld, dim, labels.data_ptr(), None, n, K,
                                               **{k: v.data_ptr() for k, v in mom[dim].items()})

    def spheres(dim, fixed, rounds):
        a, ld = src[dim]
        return lambda: ctx.cluster_spheres_dev(a.data_ptr(), ld, dim, labels.data_ptr(), None, n, K, fixed, rounds,
                                               **{k: v.data_ptr() for k, v in sph[dim].items()})

    calls = [("vcp_centroids_dev (xyz + motor)", None,
              lambda: ctx.centroids_dev(xyz.data_ptr(), motor.data_ptr(), labels.data_ptr(), n, K, c3.data_ptr(), c2.data_ptr(),
                                        cc.data_ptr()))]
    calls += [("vcp_cluster_moments_dev dim %d" % d, ("moments", d), moments(d)) for d in (2, 3)]
    for d in (2, 3):
        for fixed in (0.0, FIXED):
            for r in ROUNDS:
                calls.append(("vcp_cluster_spheres_dev dim %d, radius %s, rounds %d" % (d, "fixed" if fixed else "free", r),
                              ("spheres", d, fixed, r), spheres(d, fixed, r)))
    lines, base, seen = [], None, {}
    head = dict(case="C4", n=n, K=K)
    for name, key, fn in calls:
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
        seen[key] = (ev, ph)
        lines.append(ln)
        print(json.dumps(ln), flush=True)
    for d in (2, 3):
        for fixed in (0.0, FIXED):
            k0, k4, k12 = (("spheres", d, fixed, r) for r in ROUNDS)
            if not all(k in seen for k in (k0, k4, k12, ("moments", d))):
                continue
            cov = seen[("moments", d)][1].get("moments_cov")
            per12, per4 = (seen[k12][0] - seen[k0][0]) / 12, (seen[k4][0] - seen[k0][0]) / 4
            ln = dict(head, run="per round, dim %d, radius %s" % (d, "fixed" if fixed else "free"),
                      ms_per_round_from_12=round(per12, 4), ms_per_round_from_4=round(per4, 4), moments_cov_ms=cov,
                      round_over_moments_cov=round(per12 / cov, 3) if cov else None)
            lines.append(ln)
            print(json.dumps(ln), flush=True)
    ctx.close()
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(json.dumps(ln) for ln in lines) + "\n")


if __name__ == "__main__":
    main()
