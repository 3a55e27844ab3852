"""Timing of vcp_match_unique beside vcp_match on the same input, in the same run.

Inputs (K centroids against T truths, identity M):
  field   T truths on a jittered 2-D field of unit pitch (z = 0, as the reference feeds them), 0.87 T detections
          (truth + sigma 0.02 noise), the remaining centroids clutter, a quarter of it beside a detection; max_dist =
          five sigmas.  The centroid workload the README quotes vcp_match for.
  chain   centroids and truths alternating on a line with strictly decreasing gaps: nearest is injective, yet only one
          pair is locally dominant per round, so the rounds number min(K, T).  The declared worst case.
Per case a warm-up call and the median of --reps blocking calls (host wall clock around the call; the library
synchronises its stream before returning), the vcp_timing phases of the last call, rounds, count_pairs and vcp_match's
count.  One JSON line per case.
usage: python tools/bench_match_unique.py [--n 27000] [--reps 7] [--chain-reps 3]"""
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


def _median_ms(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), [round(t, 3) for t in ts]


def field(n, seed=41, sigma=0.02):
    rng = np.random.default_rng(seed)
    side = int(np.ceil(np.sqrt(n)))
    g = np.stack(np.meshgrid(np.arange(side), np.arange(side), indexing="ij"), -1).reshape(-1, 2)[:n] * 1.0
    truths = np.c_[g + rng.uniform(-0.2, 0.2, (n, 2)), np.zeros(n)]
    n_det = int(0.87 * n)
    n_near = (n - n_det) // 4
    n_far = n - n_det - n_near
    det = truths[rng.choice(n, n_det, replace=False)] + np.c_[rng.normal(0, sigma, (n_det, 2)), np.zeros(n_det)]
    near = det[rng.integers(0, n_det, n_near)] + np.c_[rng.normal(0, 2 * sigma, (n_near, 2)), np.zeros(n_near)]
    far = np.c_[rng.uniform(-1, side, (n_far, 2)), np.zeros(n_far)]
    centers = np.r_[det, near, far]
    return centers[rng.permutation(n)], truths, 5 * sigma


def chain(n):
    gaps = 1.0 - (0.5 / (2 * n)) * np.arange(2 * n - 1)
    x = np.concatenate([[0.0], np.cumsum(gaps)])
    z = np.zeros(n)
    return np.c_[x[0::2], z, z], np.c_[x[1::2], z, z], 2.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=27000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--chain-reps", type=int, default=3)
    args = ap.parse_args()
    ctx = N.Context(0)
    ctx.timing_enable(True)
    M = np.eye(4)
    for name, (c, t, md), reps in (("field", field(args.n), args.reps), ("chain", chain(args.n), args.chain_reps)):
        K, T = len(c), len(t)
        base = dict(input=name, K=K, T=T, max_dist=md)
        out = {}

        def report(case, fn, extra):
            ms, runs = _median_ms(fn, reps)
            # vcp_match records no phases: the context would still hold those of an earlier call
            phases = {p: round(v, 4) for p, v in ctx.timing()} if case != "match_host" else {}
            print(json.dumps(dict(case=case, ms=round(ms, 3), runs=runs, phases=phases, **base, **extra())), flush=True)
            return ms

        a = report("match_host", lambda: out.update(m=ctx.match(c, t, M, md)), extra=lambda: dict(count_matched=out["m"]["count"]))
        b = report("match_unique_host", lambda: out.update(u=ctx.match_unique(c, t, M, md)),
                   extra=lambda: dict(count_pairs=out["u"]["count"], rounds=out["u"]["rounds"],
                                      count_matched=out["m"]["count"],
                                      distinct_truths_of_match=int(len(set(out["m"]["nearest"][out["m"]["is_matched"] == 1].tolist())))))
        d_c, d_t = torch.from_numpy(np.ascontiguousarray(c)).cuda(), torch.from_numpy(np.ascontiguousarray(t)).cuda()
        to = torch.zeros(K, dtype=torch.int32, device="cuda")
        co = torch.zeros(T, dtype=torch.int32, device="cuda")
        pd = torch.zeros(K, dtype=torch.float64, device="cuda")
        mx = torch.zeros((K, 3), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        d = report("match_unique_dev", lambda: out.update(d=ctx.match_unique_dev(
            d_c.data_ptr(), K, d_t.data_ptr(), T, M, md, to.data_ptr(), co.data_ptr(), pd.data_ptr(), mx.data_ptr())),
            extra=lambda: dict(count_pairs=out["d"]["count"], rounds=out["d"]["rounds"]))
        print(json.dumps(dict(case="ratios", unique_host_over_match_host=round(b / a, 2), unique_dev_ms=round(d, 3), **base)),
              flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
