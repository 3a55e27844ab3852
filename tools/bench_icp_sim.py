"""Similarity ICP (vcp_icp_sim) next to vcp_icp_gated on the same inputs, in the same process: what the two further
columns of the pass and the scale of the step cost, at the (K, landmarks) rows of tools/bench_icp_gated.py with H = 1
and H = 36, the same schedule (wider than the scene: nothing is dropped) and the same poses.  The similarity call runs
twice: with the ratio range closed to (1, 1), where every round's pose is the gated call's bit for bit (checked once per
case), so that the difference in time is the 18-wide pass and step and nothing else; and with the range open, (0.9,
1.1), where the rounds fit and apply a scale and the poses, and with them the cost of the neighbour search, go their
own way.  The three calls alternate; median and spread (min .. max) of 5 blocking calls each after a warm-up; prints one
line per case and a JSON summary line."""
import json
import math
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vtkcloudpoint_amd import _native as N  # noqa: E402

GATES = [4000.0, 2000.0, 1000.0]   # finite, and beyond every distance in a scene of 215 x 215: nothing is dropped
RANGE = (0.9, 1.1)


def alternate(fns, reps=5):
    for fn in fns:  # warm-up
        fn()
    out = [[] for _ in fns]
    for _ in range(reps):
        for fn, ts in zip(fns, out):
            t = time.perf_counter()
            fn()
            ts.append((time.perf_counter() - t) * 1e3)
    return out


ctx = N.Context(0)
rows = []
for K in (4000, 27380):
    rng = np.random.default_rng(K)
    truth = np.c_[rng.uniform(0.0, 215.0, (K, 2)), np.zeros(K)]
    th = math.radians(150.0)
    c, s = math.cos(th), math.sin(th)
    cen = (truth - [3.0, -2.0, 0.0]) @ np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])
    cen[:, :2] += rng.normal(0.0, 0.01, (K, 2))
    for ml in (200, K):
        for H in (1, 36):
            tg, tc, ts = alternate([lambda: ctx.icp_gated(cen, truth, GATES, H, None, 100, ml, 3, 0.05),
                                    lambda: ctx.icp_sim(cen, truth, GATES, (1.0, 1.0), H, None, 100, ml, 3, 0.05),
                                    lambda: ctx.icp_sim(cen, truth, GATES, RANGE, H, None, 100, ml, 3, 0.05)])
            g = ctx.icp_gated(cen, truth, GATES, H, None, 100, ml, 3, 0.05)
            one = ctx.icp_sim(cen, truth, GATES, (1.0, 1.0), H, None, 100, ml, 3, 0.05)
            same = all(np.array_equal(g[k], one[k]) for k in ("M_all", "mean_dist", "inliers", "kept", "starved"))
            L = K // (K // ml) if K > ml else K   # the landmarks of the call: every (K / ml)-th centroid
            assert (one["kept"] == L).all() and (one["starved"] == 0).all()
            row = dict(K=K, landmarks=L, H=H, gated_ms=round(float(np.median(tg)), 3),
                       gated_min_max=[round(min(tg), 3), round(max(tg), 3)],
                       closed_ms=round(float(np.median(tc)), 3), closed_min_max=[round(min(tc), 3), round(max(tc), 3)],
                       open_ms=round(float(np.median(ts)), 3), open_min_max=[round(min(ts), 3), round(max(ts), 3)],
                       ratio_closed=round(float(np.median(tc) / np.median(tg)), 3),
                       ratio_open=round(float(np.median(ts) / np.median(tg)), 3), same_bits_closed_range=bool(same))
            rows.append(row)
            print("K=%d landmarks=%d H=%d: gated %.2f ms (%.2f .. %.2f); similarity, closed range %.2f ms (%.2f .. %.2f), "
                  "x%.3f, same bits: %s; open range %.2f ms (%.2f .. %.2f), x%.3f"
                  % (K, L, H, row["gated_ms"], min(tg), max(tg), row["closed_ms"], min(tc), max(tc), row["ratio_closed"],
                     same, row["open_ms"], min(ts), max(ts), row["ratio_open"]), flush=True)
ctx.timing_enable(True)
ctx.icp_sim(cen, truth, GATES, RANGE, 36, None, 100, 200, 3, 0.05)
print(json.dumps(dict(bench="icp_sim", rows=rows, phases_K27380_H36=ctx.timing())))
