"""Anisotropic ICP (vcp_icp_aniso) next to vcp_icp_sim on the same inputs, in the same process, at the (K, landmarks)
rows of tools/bench_icp_sim.py with H = 1 and H = 36, the same schedule (wider than the scene: nothing is dropped) and the
same poses.  Both passes are 18 columns wide and both steps hold one Horn solve, so the figure of interest is the ratio
of the two.  Each call runs twice: with the ratio range closed to (1, 1), where both loops are the rigid fit and their
poses agree to rounding (checked once per case), so that the two walk the same neighbour searches and the difference in
time is the pass and the step alone; and with the range open, (0.9, 1.1), where each fits its own scales and the poses,
and with them the cost of the neighbour search, go their own way.  The four calls alternate; median and spread
(min .. max) of 5 blocking calls each after a warm-up; 100 rounds a call, so a round's time is the call's over 100 (the
score and the transfers included).  Prints one line per case and a JSON summary line."""
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
ROUNDS = 100


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


def med(ts):
    return round(float(np.median(ts)), 3)


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
            calls = [lambda: ctx.icp_sim(cen, truth, GATES, (1.0, 1.0), H, None, ROUNDS, ml, 3, 0.05),
                     lambda: ctx.icp_aniso(cen, truth, GATES, (1.0, 1.0), H, None, None, ROUNDS, ml, 3, 0.05),
                     lambda: ctx.icp_sim(cen, truth, GATES, RANGE, H, None, ROUNDS, ml, 3, 0.05),
                     lambda: ctx.icp_aniso(cen, truth, GATES, RANGE, H, None, None, ROUNDS, ml, 3, 0.05)]
            sc, ac, so, ao = alternate(calls)
            a, b = calls[0](), calls[1]()
            close = bool(np.abs(a["M_all"] - b["M_all"]).max() < 1e-6 and np.array_equal(a["inliers"], b["inliers"]))
            L = K // (K // ml) if K > ml else K   # the landmarks of the call: every (K / ml)-th centroid
            assert (b["kept"] == L).all() and (b["starved"] == 0).all() and (b["scale"] == 1.0).all()
            row = dict(K=K, landmarks=L, H=H, sim_closed_ms=med(sc), sim_closed_min_max=[round(min(sc), 3), round(max(sc), 3)],
                       aniso_closed_ms=med(ac), aniso_closed_min_max=[round(min(ac), 3), round(max(ac), 3)],
                       sim_open_ms=med(so), sim_open_min_max=[round(min(so), 3), round(max(so), 3)],
                       aniso_open_ms=med(ao), aniso_open_min_max=[round(min(ao), 3), round(max(ao), 3)],
                       aniso_round_us=round(1e3 * med(ac) / ROUNDS, 2),
                       ratio_closed=round(float(np.median(ac) / np.median(sc)), 3),
                       ratio_open=round(float(np.median(ao) / np.median(so)), 3), same_poses_closed_range=close)
            rows.append(row)
            print("K=%d landmarks=%d H=%d: closed range: similarity %.2f ms (%.2f .. %.2f), anisotropic %.2f ms (%.2f .. %.2f), "
                  "x%.3f, %.1f us a round, poses agree: %s; open range: similarity %.2f ms (%.2f .. %.2f), anisotropic "
                  "%.2f ms (%.2f .. %.2f), x%.3f"
                  % (K, L, H, row["sim_closed_ms"], min(sc), max(sc), row["aniso_closed_ms"], min(ac), max(ac),
                     row["ratio_closed"], row["aniso_round_us"], close, row["sim_open_ms"], min(so), max(so),
                     row["aniso_open_ms"], min(ao), max(ao), row["ratio_open"]), flush=True)
ctx.timing_enable(True)
ctx.icp_aniso(cen, truth, GATES, RANGE, 36, None, None, ROUNDS, 200, 3, 0.05)
print(json.dumps(dict(bench="icp_aniso", rows=rows, phases_K27380_H36=ctx.timing())))
