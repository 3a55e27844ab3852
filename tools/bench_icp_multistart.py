"""Multi-start ICP (vcp_icp_multistart) of K centroids against K truths, MainForm.ICP's real use: H start rotations in
one call next to one vcp_icp_vtklike call and 36 sequential ones on the same inputs.  Median of 5 blocking calls after
a warm-up; prints one line per case and a JSON summary line."""
import json
import math
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vtkcloudpoint_amd import _native as N  # noqa: E402


def med(f, reps=5):
    f()  # warm-up
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        f()
        ts.append(time.perf_counter() - t)
    return float(np.median(ts)) * 1e3


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
        one = med(lambda: ctx.icp_vtklike(cen, truth, 100, ml, True))
        seq36 = med(lambda: [ctx.icp_vtklike(cen, truth, 100, ml, True) for _ in range(36)], reps=3)
        for H in (1, 36, 360):
            t = med(lambda: ctx.icp_multistart(cen, truth, H, None, 100, ml, 0.05))
            r = ctx.icp_multistart(cen, truth, H, None, 100, ml, 0.05)
            row = dict(K=K, landmarks=min(ml, K), H=H, ms=round(t, 3), vtklike_ms=round(one, 3),
                       vtklike_x36_ms=round(seq36, 3), ratio=round(t / one, 2), best_inliers=int(r["inliers"][r["best"]]))
            rows.append(row)
            print("K=%d landmarks=%d H=%d: %.2f ms (one vtklike %.2f ms, 36 sequential %.2f ms, x%.2f of one); "
                  "best %d / %d inliers" % (K, min(ml, K), H, t, one, seq36, t / one, row["best_inliers"], K), flush=True)
ctx.timing_enable(True)
ctx.icp_multistart(cen, truth, 360, None, 100, 200, 0.05)
print(json.dumps(dict(bench="icp_multistart", rows=rows, phases_K27380_H360=ctx.timing())))
