"""Congruent-pair registration (vcp_register_pairs) next to vcp_icp_multistart (H = 36, 100 rounds) on the same
partial-overlap input, in the same process: a scan that sees a window of the truth field (truths uniform in a square,
the source = the truths inside the lower-left window, 90 % kept, noise sigma 0.01, 10 clutter points, moved back by a
planted pose), 8 bases of length 2..5, len_tol 0.03, inlier_dist 0.1.  The two calls alternate; median and spread
(min .. max) of `--reps` blocking calls each after a warm-up.  Both inlier counts are printed beside the planted pose's:
the timing compares a call that finds the pose with one that cannot.  One line per case and a JSON summary line.

usage: python tools/bench_register.py [--reps 7]"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vtkcloudpoint_amd import _native as N  # noqa: E402
from vtkcloudpoint_amd.icp import choose_bases  # noqa: E402

ANGLE, SHIFT = 2.0, np.array([1.5, -0.8, 0.0])
LEN_TOL, INLIER = 0.03, 0.1


def scene(n_truths, field, window, seed):
    rng = np.random.default_rng([seed, n_truths])
    truths = np.zeros((n_truths, 3))
    truths[:, :2] = rng.uniform(0.0, field, (n_truths, 2))
    seen = truths[(truths[:, 0] <= window) & (truths[:, 1] <= window)]
    seen = seen[rng.random(len(seen)) < 0.9].copy()
    seen[:, :2] += rng.normal(0.0, 0.01, (len(seen), 2))
    clutter = np.zeros((10, 3))
    clutter[:, :2] = rng.uniform(0.0, window, (10, 2))
    x = np.concatenate([seen, clutter])
    x = x[rng.permutation(len(x))]
    c, s = math.cos(ANGLE), math.sin(ANGLE)
    Rz = np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])
    src = np.ascontiguousarray((x - SHIFT) @ Rz)
    src[:, 2] = 0.0
    M = np.eye(4)
    M[:3, :3], M[:3, 3] = Rz, SHIFT
    return truths, src, M


def alternate(f, g, reps):
    f(), g()  # warm-up
    tf, tg = [], []
    for _ in range(reps):
        for fn, ts in ((f, tf), (g, tg)):
            t = time.perf_counter()
            fn()
            ts.append((time.perf_counter() - t) * 1e3)
    return tf, tg


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    ctx = N.Context(0)
    rows = []
    # (truths, field edge, window edge): the scene of the tests, then the same density on larger fields
    for n_truths, field, window in ((400, 20.0, 10.0), (4000, 63.2, 10.0), (4000, 63.2, 31.6), (27380, 165.5, 31.6)):
        truths, src, P = scene(n_truths, field, window, 5)
        bases = choose_bases(src, 8, 2.0, 5.0, 1)
        planted = ctx.match(src, truths, P, INLIER)["count"]
        tr, tm = alternate(lambda: ctx.register_pairs(src, truths, bases, LEN_TOL, INLIER),
                           lambda: ctx.icp_multistart(src, truths, 36, None, 100, 200, INLIER), a.reps)
        r = ctx.register_pairs(src, truths, bases, LEN_TOL, INLIER)
        m = ctx.icp_multistart(src, truths, 36, None, 100, 200, INLIER)
        ctx.timing_enable(True)
        ctx.register_pairs(src, truths, bases, LEN_TOL, INLIER)
        phases = {k: round(v, 3) for k, v in ctx.timing()}
        ctx.timing_enable(False)
        row = dict(truths=n_truths, source=len(src), planted_inliers=int(planted), hypotheses=int(r["n_hyp"].sum()),
                   register_ms=round(float(np.median(tr)), 3), register_min_max=[round(min(tr), 3), round(max(tr), 3)],
                   register_inliers=int(r["inliers"][r["best"]]) if r["best"] >= 0 else 0, register_phases_ms=phases,
                   multistart_ms=round(float(np.median(tm)), 3), multistart_min_max=[round(min(tm), 3), round(max(tm), 3)],
                   multistart_inliers=int(m["inliers"][m["best"]]))
        rows.append(row)
        print("truths=%d source=%d planted %d: register_pairs %.3f ms (%.3f .. %.3f), %d hypotheses, %d inliers, phases %s; "
              "icp_multistart H=36 %.3f ms (%.3f .. %.3f), %d inliers"
              % (n_truths, len(src), planted, row["register_ms"], min(tr), max(tr), row["hypotheses"],
                 row["register_inliers"], phases, row["multistart_ms"], min(tm), max(tm), row["multistart_inliers"]),
              flush=True)
    print(json.dumps(dict(bench="register_pairs", reps=a.reps, rows=rows)))


if __name__ == "__main__":
    main()
