"""Trimmed ICP (vcp_icp_trimmed, share 0.75) next to vcp_icp_gated (a finite schedule that drops nothing) and
vcp_icp_multistart on the same inputs, in the same process, at the (K, landmarks) rows of tools/bench_icp_multistart.py
with H = 1 and H = 36.  The three calls alternate; median and spread (min .. max) of 5 blocking calls each after a
warm-up; prints one line per case and a JSON summary line, and writes both to profiles/icp_trimmed_bench.txt (or the
file given as the first argument)."""
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
SHARE = [0.75]
ROUNDS = 100


def alternate(fns, reps=5):
    for f in fns:  # warm-up
        f()
    ts = [[] for _ in fns]
    for _ in range(reps):
        for f, t in zip(fns, ts):
            t0 = time.perf_counter()
            f()
            t.append((time.perf_counter() - t0) * 1e3)
    return ts


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "icp_trimmed_bench.txt")
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
            L = K // (K // ml) if K > ml else K   # the landmarks of the call: every (K / ml)-th centroid
            for H in (1, 36):
                tm, tg, tt = alternate((lambda: ctx.icp_multistart(cen, truth, H, None, ROUNDS, ml, 0.05),
                                        lambda: ctx.icp_gated(cen, truth, GATES, H, None, ROUNDS, ml, 3, 0.05),
                                        lambda: ctx.icp_trimmed(cen, truth, SHARE, H, None, ROUNDS, ml, 3, 0.05)))
                g = ctx.icp_gated(cen, truth, GATES, H, None, ROUNDS, ml, 3, 0.05)
                t = ctx.icp_trimmed(cen, truth, SHARE, H, None, ROUNDS, ml, 3, 0.05)
                assert (g["kept"] == L).all() and (g["starved"] == 0).all()
                assert (t["kept"] == math.ceil(0.75 * L)).all() and (t["starved"] == 0).all()
                med = [float(np.median(x)) for x in (tm, tg, tt)]
                row = dict(K=K, landmarks=L, H=H, multistart_ms=round(med[0], 3),
                           multistart_min_max=[round(min(tm), 3), round(max(tm), 3)], gated_ms=round(med[1], 3),
                           gated_min_max=[round(min(tg), 3), round(max(tg), 3)], trimmed_ms=round(med[2], 3),
                           trimmed_min_max=[round(min(tt), 3), round(max(tt), 3)],
                           trimmed_over_multistart=round(med[2] / med[0], 3), trimmed_over_gated=round(med[2] / med[1], 3),
                           gated_over_multistart=round(med[1] / med[0], 3))
                rows.append(row)
                say("K=%d landmarks=%d H=%d: trimmed %.2f ms (%.2f .. %.2f), gated %.2f ms (%.2f .. %.2f), multistart "
                    "%.2f ms (%.2f .. %.2f); trimmed/multistart x%.3f, trimmed/gated x%.3f, gated/multistart x%.3f"
                    % (K, L, H, med[2], min(tt), max(tt), med[1], min(tg), max(tg), med[0], min(tm), max(tm),
                       row["trimmed_over_multistart"], row["trimmed_over_gated"], row["gated_over_multistart"]))
    ctx.timing_enable(True)
    phases = {}
    for ml in (200, 27380):     # the last K: per-phase device time of the three calls at H = 36
        ctx.icp_multistart(cen, truth, 36, None, ROUNDS, ml, 0.05)
        phases["multistart_L%d" % ml] = ctx.timing()
        ctx.icp_gated(cen, truth, GATES, 36, None, ROUNDS, ml, 3, 0.05)
        phases["gated_L%d" % ml] = ctx.timing()
        ctx.icp_trimmed(cen, truth, SHARE, 36, None, ROUNDS, ml, 3, 0.05)
        phases["trimmed_L%d" % ml] = ctx.timing()
    say(json.dumps(dict(bench="icp_trimmed", rounds=ROUNDS, share=SHARE[0], rows=rows, phases_K27380_H36=phases)))
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
