"""Gated ICP (vcp_icp_gated) next to vcp_icp_multistart on the same inputs, in the same process: what the gate costs
when it drops nothing (a finite schedule wider than the scene), at the (K, landmarks) rows of tools/
bench_icp_multistart.py with H = 1 and H = 36.  The two calls alternate; median and spread (min .. max) of 5 blocking
calls each after a warm-up; prints one line per case and a JSON summary line."""
import json
import math
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vtkcloudpoint_amd import _native as N  # noqa: E402

GATES = [4000.0, 2000.0, 1000.0]   # finite, and beyond every distance in a scene of 215 x 215: nothing is dropped


def alternate(f, g, reps=5):
    f(), g()  # warm-up
    tf, tg = [], []
    for _ in range(reps):
        for fn, ts in ((f, tf), (g, tg)):
            t = time.perf_counter()
            fn()
            ts.append((time.perf_counter() - t) * 1e3)
    return tf, tg


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
            tm, tg = alternate(lambda: ctx.icp_multistart(cen, truth, H, None, 100, ml, 0.05),
                               lambda: ctx.icp_gated(cen, truth, GATES, H, None, 100, ml, 3, 0.05))
            m = ctx.icp_multistart(cen, truth, H, None, 100, ml, 0.05)
            g = ctx.icp_gated(cen, truth, GATES, H, None, 100, ml, 3, 0.05)
            same = all(np.array_equal(m[k], g[k]) for k in ("M_all", "mean_dist", "inliers"))
            L = K // (K // ml) if K > ml else K   # the landmarks of the call: every (K / ml)-th centroid
            assert (g["kept"] == L).all() and (g["starved"] == 0).all()
            row = dict(K=K, landmarks=L, H=H, multistart_ms=round(float(np.median(tm)), 3),
                       multistart_min_max=[round(min(tm), 3), round(max(tm), 3)],
                       gated_ms=round(float(np.median(tg)), 3), gated_min_max=[round(min(tg), 3), round(max(tg), 3)],
                       ratio=round(float(np.median(tg) / np.median(tm)), 3), same_bits=bool(same))
            rows.append(row)
            print("K=%d landmarks=%d H=%d: gated %.2f ms (%.2f .. %.2f), multistart %.2f ms (%.2f .. %.2f), x%.3f; "
                  "same bits: %s" % (K, L, H, row["gated_ms"], min(tg), max(tg), row["multistart_ms"], min(tm),
                                     max(tm), row["ratio"], same), flush=True)
ctx.timing_enable(True)
ctx.icp_gated(cen, truth, GATES, 36, None, 100, 200, 3, 0.05)
print(json.dumps(dict(bench="icp_gated", rows=rows, phases_K27380_H36=ctx.timing())))
