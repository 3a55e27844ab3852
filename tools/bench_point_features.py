"""Timing of vcp_point_features_dev (include/vcp_features.h) beside the vcp_kdist_dev call that feeds it, on a resident cloud.

The cloud is the 10 M-row 3-D cloud of tools/bench_kdist.py (synth.config_cloud(--n)["xyz"]), on the device once.  Runs:
  k = 8, 16, 32    the rows in the cloud's own order
  k = 16           the same rows in Morton order (a 60-bit key of 2^20 cubic cells per axis over the bounding box, the
                   order vcp_kdist sorts its queries in; its 8-sigma trim of the box is left out, this cloud has no far
                   outliers)
  k = 16           the same rows after a random permutation
Per run, after a warm-up, the median of --reps calls of each:
  kdist_ms         vcp_kdist_dev with the knn rows at that k: the sum of its phases (hipEvents on its stream)
  features_ms      the features_rows phase of vcp_point_features_dev on those knn rows, every output asked for
  gb_s             bytes / features_ms with bytes = n (4 k the index read + 24 k the k gathered rows, counted once + 69 the
                   outputs): the bytes the definition needs, so a figure for the kernel, not a measured traffic
  share            features_ms / kdist_ms
One JSON line per run, appended to --out as well.
usage: python tools/bench_point_features.py [--n 10000000] [--reps 5] [--out profiles/point_features_bench.txt]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from vtkcloudpoint_amd import _native as N  # noqa: E402
from vtkcloudpoint_amd import synth  # noqa: E402


def _spread3(x):
    """Bit j of x (20 bits) to bit 3 j, as csrc/kdist.hip's spread3."""
    x = x & 0xFFFFF
    x = (x | (x << 32)) & 0x1F00000000FFFF
    x = (x | (x << 16)) & 0x1F0000FF0000FF
    x = (x | (x << 8)) & 0x100F00F00F00F00F
    x = (x | (x << 4)) & 0x10C30C30C30C30C3
    x = (x | (x << 2)) & 0x1249249249249249
    return x


def morton_order(pts):
    lo = pts.min(dim=0).values
    scale = (2 ** 20 - 1) / float((pts.max(dim=0).values - lo).max())
    c = ((pts - lo) * scale).to(torch.int64).clamp_(0, 2 ** 20 - 1)
    key = _spread3(c[:, 0]) | (_spread3(c[:, 1]) << 1) | (_spread3(c[:, 2]) << 2)
    return torch.argsort(key, stable=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "point_features_bench.txt"))
    args = ap.parse_args()
    from vtkcloudpoint_amd import features as FT
    ctx = N.Context(0)
    ctx.timing_enable(True)
    base = torch.from_numpy(np.ascontiguousarray(synth.config_cloud(args.n)["xyz"])).cuda()
    n = base.shape[0]
    head = dict(n=n, shape=FT.point_features_shape(ctx))
    lines = []
    runs = [("own", 8), ("own", 16), ("own", 32), ("morton", 16), ("random", 16)]
    try:
        for order, k in runs:
            if order == "own":
                pts = base
            elif order == "morton":
                pts = base[morton_order(base)].contiguous()
            else:
                pts = base[torch.randperm(n, device="cuda", generator=torch.Generator(device="cuda").manual_seed(args.seed))].contiguous()
            kd = torch.empty(n, dtype=torch.float64, device="cuda")
            knn = torch.empty((n, k), dtype=torch.int32, device="cuda")
            out = [torch.empty((n, 3), dtype=torch.float64, device="cuda") for _ in range(2)] + \
                  [torch.empty(n, dtype=torch.float64, device="cuda") for _ in range(2)] + \
                  [torch.empty(n, dtype=torch.int32, device="cuda"), torch.empty(n, dtype=torch.uint8, device="cuda")]
            vp = np.zeros(3)
            torch.cuda.synchronize()
            t_kd, t_pf = [], []
            for rep in range(args.reps + 1):                 # the first call of each is the warm-up
                ctx.kdist_dev(pts.data_ptr(), n, 3, k, kd.data_ptr(), knn.data_ptr(), metric=N.L2_3D)
                t_kd.append(sum(ms for _, ms in ctx.timing()))
                ctx._chk(FT._L().vcp_point_features_dev(ctx._h, pts.data_ptr(), 3, 3, n, knn.data_ptr(), k, vp.ctypes.data,
                                                        *[o.data_ptr() for o in out]))
                t_pf.append(dict(ctx.timing())["features_rows"])
            kd_ms, pf_ms = float(np.median(t_kd[1:])), float(np.median(t_pf[1:]))
            nbytes = n * (4 * k + 24 * k + 69)
            lines.append(dict(head, order=order, k=k, kdist_ms=round(kd_ms, 3), features_ms=round(pf_ms, 3),
                              features_ms_all=[round(v, 3) for v in t_pf[1:]], bytes=nbytes,
                              gb_s=round(nbytes / (pf_ms * 1e-3) / 1e9, 1), share=round(pf_ms / kd_ms, 4),
                              valid=int(out[5].sum()), mean_dist_median=float(out[3][torch.isfinite(out[3])].median())))
            print(json.dumps(lines[-1]), flush=True)
            del pts, kd, knn, out
            torch.cuda.empty_cache()
    except N.VcpError as e:
        lines.append(dict(head, error=str(e)))               # a library error: nothing more is started on this device
        print(json.dumps(lines[-1]), flush=True)
    ctx.close()
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(json.dumps(ln) for ln in lines) + "\n")


if __name__ == "__main__":
    main()
