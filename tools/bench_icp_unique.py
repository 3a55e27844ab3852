"""Unique-correspondence ICP (vcp_icp_unique) next to vcp_icp_gated on the same inputs, in the same process: what the
winner rule costs -- per round a distance pass that stores keys and takes the per-target minimum, the tie pass and a sums
pass that reads both back, where the gated round runs one pass -- at the (K, landmarks) rows of tools/bench_icp_gated.py
with H = 1 and H = 36, the same schedule (wider than the scene: the gate drops nothing) and the same poses.  The poses of
the two calls differ wherever two landmarks share a truth, so the neighbour searches do not see the same points; `lost`
says how many landmarks the last round left out.  The two calls alternate; median and spread (min .. max) of 5 blocking
calls each after a warm-up; prints one line per case and a JSON summary line, and writes both to
profiles/icp_unique_bench.txt (or the path given as the first argument)."""
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from vtkcloudpoint_amd import _native as N  # noqa: E402

GATES = [4000.0, 2000.0, 1000.0]   # finite, and beyond every distance in a scene of 215 x 215: nothing is dropped
ROUNDS = 100


def alternate(f, g, reps=5):
    f(), g()  # warm-up
    tf, tg = [], []
    for _ in range(reps):
        for fn, ts in ((f, tf), (g, tg)):
            t = time.perf_counter()
            fn()
            ts.append((time.perf_counter() - t) * 1e3)
    return tf, tg


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "icp_unique_bench.txt")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

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
                tg, tu = alternate(lambda: ctx.icp_gated(cen, truth, GATES, H, None, ROUNDS, ml, 3, 0.05),
                                   lambda: ctx.icp_unique(cen, truth, GATES, H, None, ROUNDS, ml, 3, 0.05))
                g = ctx.icp_gated(cen, truth, GATES, H, None, ROUNDS, ml, 3, 0.05)
                u = ctx.icp_unique(cen, truth, GATES, H, None, ROUNDS, ml, 3, 0.05)
                L = K // (K // ml) if K > ml else K   # the landmarks of the call: every (K / ml)-th centroid
                assert (g["kept"] == L).all() and (u["kept"] + u["lost"] == L).all()
                row = dict(K=K, landmarks=L, H=H, gated_ms=round(float(np.median(tg)), 3),
                           gated_min_max=[round(min(tg), 3), round(max(tg), 3)],
                           unique_ms=round(float(np.median(tu)), 3), unique_min_max=[round(min(tu), 3), round(max(tu), 3)],
                           ratio=round(float(np.median(tu) / np.median(tg)), 3),
                           lost_best=int(u["lost"][u["best"]]), lost_max=int(u["lost"].max()),
                           inliers_gated=int(g["inliers"][g["best"]]), inliers_unique=int(u["inliers"][u["best"]]))
                rows.append(row)
                say("K=%d landmarks=%d H=%d: unique %.2f ms (%.2f .. %.2f), gated %.2f ms (%.2f .. %.2f), x%.3f; lost %d "
                    "(best pose) .. %d; inliers %d (unique) %d (gated)"
                    % (K, L, H, row["unique_ms"], min(tu), max(tu), row["gated_ms"], min(tg), max(tg), row["ratio"],
                       row["lost_best"], row["lost_max"], row["inliers_unique"], row["inliers_gated"]))
    ctx.timing_enable(True)
    ctx.icp_gated(cen, truth, GATES, 36, None, ROUNDS, 200, 3, 0.05)
    pg = ctx.timing()
    ctx.icp_unique(cen, truth, GATES, 36, None, ROUNDS, 200, 3, 0.05)
    pu = ctx.timing()
    say(json.dumps(dict(bench="icp_unique", rounds=ROUNDS, rows=rows, phases_gated_K27380_H36=pg,
                        phases_unique_K27380_H36=pu)))
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
