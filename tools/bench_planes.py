"""Timing of the plane extraction (include/vcp_planes.h) on a resident cloud, and of vcp_dbscan_dev before and after it.

The cloud (--n rows, generated on the device from a seed, on the 2^-20 lattice, shuffled): three planes holding 60 % of the
rows (normals (0,0,1), (1,0,0), (0.6,0.75,0.28); uniform in +-4 along two in-plane axes, normal noise sigma 0.004), sphere
targets of radius 0.0725 with 1000 rows each holding 20 %, uniform background in [-5, 7]^3 for the rest.
Timed, each after a warm-up, median of --reps calls:
  score      vcp_plane_score_dev alone at H = 256, 1024, 4096 (planes of random triples of the cloud: most cross it).
             ms_events is the call's planes_score phase (hipEvents on the stream the kernel runs on, the memset of the
             counts included); gop_s = 7 n H / ms_events, the binary64 operations of the definition (3 multiplies, 3 adds,
             1 compare per residual) per second: a figure for the kernel.
  extract    the whole extract_planes call (thr 0.012, H 1024, up to 5 planes, min_inliers n / 100, refit): ms_wall is the
             host clock around the blocking call, read-backs included; phases sums the vcp_timing phases by name.
  dbscan     vcp_dbscan_dev (L2_3D, --eps, --min-pts) on the whole cloud, and on the rows extract_planes left (compacted
             by torch, not timed): ms_events is the sum of its phases.
One JSON line per measurement, appended to --out as well.  --lib times another build of the library (the same sources
with -DPL_PLANES_IN_LDS=0, say) instead of the package's.
usage: python tools/bench_planes.py [--n 10000000] [--reps 5] [--out profiles/planes_bench.txt] [--lib path] [--no-dbscan]"""
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

TRUE_PLANES = (((0.0, 0.0, 1.0), -1.5), ((1.0, 0.0, 0.0), 5.0), ((0.6, 0.75, 0.28), 6.0))


def cloud(n, seed):
    """[n, 3] float64 on the device, and the number of rows drawn on the planes."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    f64 = dict(dtype=torch.float64, device="cuda", generator=g)
    per_plane, n_sph = n // 5, max(n // 5000, 1)
    per_sph = (n // 5) // n_sph
    parts = []
    for nv, off in TRUE_PLANES:
        nv = np.asarray(nv) / np.linalg.norm(nv)
        e1 = np.cross(nv, [0.3, 0.5, 0.8])
        e1 /= np.linalg.norm(e1)
        e2 = np.cross(nv, e1)
        nv, e1, e2 = (torch.tensor(v, dtype=torch.float64, device="cuda") for v in (nv, e1, e2))
        s = torch.rand((per_plane, 2), **f64) * 8.0 - 4.0
        w = torch.randn((per_plane, 1), **f64) * 0.004
        parts.append(off * nv + s[:, :1] * e1 + s[:, 1:] * e2 + w * nv)
    c = torch.rand((n_sph, 1, 3), **f64) * 6.0 - 3.0
    v = torch.randn((n_sph, per_sph, 3), **f64)
    parts.append((c + 0.0725 * v / v.norm(dim=2, keepdim=True)).reshape(-1, 3))
    rest = n - sum(len(p) for p in parts)
    parts.append(torch.rand((rest, 3), **f64) * 12.0 - 5.0)
    pts = torch.round(torch.cat(parts) * 2.0 ** 20) / 2.0 ** 20
    return pts[torch.randperm(n, device="cuda", generator=g)].contiguous(), 3 * per_plane


def timed(ctx, fn, reps):
    """(median of the summed phases, median wall, the phases of the last call summed by name) after one warm-up."""
    fn()
    ev, wall = [], []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        wall.append((time.perf_counter() - t0) * 1e3)
        ev.append(sum(ms for _, ms in ctx.timing()))
    ph = {}
    for name, ms in ctx.timing():
        ph[name] = round(ph.get(name, 0.0) + ms, 3)
    return float(np.median(ev)), float(np.median(wall)), ph


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--eps", type=float, default=0.02)
    ap.add_argument("--min-pts", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "planes_bench.txt"))
    ap.add_argument("--lib", default=None)
    ap.add_argument("--no-dbscan", action="store_true")
    args = ap.parse_args()
    if args.lib:
        N.LIB_PATH = os.path.abspath(args.lib)
    from vtkcloudpoint_amd import planes as PL
    ctx = N.Context(0)
    ctx.timing_enable(True)
    n = args.n
    pts, on_planes = cloud(n, args.seed)
    head = dict(n=n, lib=os.path.relpath(N.LIB_PATH, ROOT), shape=PL.plane_score_shape(ctx), rows_on_planes=on_planes)
    lines = []

    def emit(**kw):
        lines.append(dict(head, **kw))
        print(json.dumps(lines[-1]), flush=True)

    try:
        g = torch.Generator(device="cuda").manual_seed(args.seed + 1)
        for H in (256, 1024, 4096):
            tri = torch.randint(0, n, (H, 3), dtype=torch.int32, device="cuda", generator=g)
            planes, valid = PL.planes_from_triples(pts, tri, ctx=ctx)
            counts = [None]

            def score():
                counts[0] = PL.plane_score(pts, planes, 0.012, ctx=ctx)

            ev, wall, ph = timed(ctx, score, args.reps)
            emit(run="score", H=H, ms_events=round(ev, 3), ms_wall=round(wall, 3), ops=7 * n * H,
                 gop_s=round(7 * n * H / (ev * 1e-3) / 1e9, 1), valid=int(valid.sum()), inliers_max=int(counts[0].max()),
                 inliers_mean=float(counts[0].double().mean()))
        fit = [None]

        def extract():
            fit[0] = PL.extract_planes(pts, 0.012, hypotheses=1024, max_planes=5, min_inliers=n // 100, seed=args.seed, ctx=ctx)

        ev, wall, ph = timed(ctx, extract, args.reps)
        emit(run="extract", H=1024, ms_events=round(ev, 3), ms_wall=round(wall, 3), phases=ph, n_planes=fit[0].n_planes,
             counts=fit[0].counts.tolist(), hyp_counts=fit[0].hyp_counts.tolist())
        if not args.no_dbscan:
            keep, idx = PL.remove_planes(fit[0])
            rest = pts[idx.long()].contiguous()
            for name, coords in (("dbscan, whole cloud", pts), ("dbscan, planes removed", rest)):
                m = coords.shape[0]
                labels = torch.empty(m, dtype=torch.int32, device="cuda")
                torch.cuda.synchronize()
                res = [None]

                def db():
                    res[0] = ctx.dbscan_dev(coords.data_ptr(), m, 3, args.eps, args.min_pts, N.L2_3D, d_labels=labels.data_ptr())

                ev, wall, ph = timed(ctx, db, max(1, args.reps // 2))
                sizes = torch.bincount(labels[labels > 0].long()) if res[0][0] > 0 else torch.zeros(1)
                emit(run=name, rows=m, eps=args.eps, min_pts=args.min_pts, ms_events=round(ev, 3), ms_wall=round(wall, 3),
                     phases=ph, clusters=res[0][0], largest_cluster=int(sizes.max()))
    except N.VcpError as e:
        emit(error=str(e))                 # a library error: nothing more is started on this device
    ctx.close()
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(json.dumps(ln) for ln in lines) + "\n")


if __name__ == "__main__":
    main()
