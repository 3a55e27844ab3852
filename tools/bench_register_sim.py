"""Similarity-pair registration (vcp_register_sim) next to congruent-pair registration (vcp_register_pairs) in the same
process, on tools/bench_register.py's partial-overlap scenes at 400, 4000 and 27 380 truths.  vcp_register_sim gets the
source divided by 2.5, 8 bases of length 2/2.5 .. 5/2.5 and the range [2.2, 2.8]; vcp_register_pairs gets the source in
the truths' unit, the same index pairs and len_tol 0.03, inlier_dist 0.1 for both.  The range admits far more target pairs
per base than len_tol does, so the two calls do different amounts of work: the hypothesis counts are printed beside the
times.  The two calls alternate; median and spread (min .. max) of `--reps` blocking calls each after a warm-up.  One line
per case and a JSON summary line.

usage: python tools/bench_register_sim.py [--reps 7]"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_register import INLIER, LEN_TOL, alternate, scene  # noqa: E402
from vtkcloudpoint_amd import _native as N  # noqa: E402
from vtkcloudpoint_amd.icp import choose_bases  # noqa: E402

SCALE, RANGE = 2.5, (2.2, 2.8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    ctx = N.Context(0)
    rows = []
    for n_truths, field, window in ((400, 20.0, 10.0), (4000, 63.2, 10.0), (27380, 165.5, 31.6)):
        truths, src, P = scene(n_truths, field, window, 5)
        small = np.ascontiguousarray(src / SCALE)
        bases = choose_bases(small, 8, 2.0 / SCALE, 5.0 / SCALE, 1)
        Ps = P.copy()
        Ps[:3, :3] *= SCALE
        planted = ctx.match(small, truths, Ps, INLIER)["count"]
        ts, tr = alternate(lambda: ctx.register_sim(small, truths, bases, RANGE[0], RANGE[1], INLIER),
                           lambda: ctx.register_pairs(src, truths, bases, LEN_TOL, INLIER), a.reps)
        s = ctx.register_sim(small, truths, bases, RANGE[0], RANGE[1], INLIER)
        r = ctx.register_pairs(src, truths, bases, LEN_TOL, INLIER)
        ctx.timing_enable(True)
        ctx.register_sim(small, truths, bases, RANGE[0], RANGE[1], INLIER)
        phases = {k: round(v, 3) for k, v in ctx.timing()}
        ctx.timing_enable(False)
        row = dict(truths=n_truths, source=len(src), planted_inliers=int(planted),
                   sim_hypotheses=int(s["n_hyp"].sum()), sim_ms=round(float(np.median(ts)), 3),
                   sim_min_max=[round(min(ts), 3), round(max(ts), 3)],
                   sim_inliers=int(s["inliers"][s["best"]]) if s["best"] >= 0 else 0,
                   sim_scale=float(s["scale"][s["best"]]) if s["best"] >= 0 else 0.0, sim_phases_ms=phases,
                   pairs_hypotheses=int(r["n_hyp"].sum()), pairs_ms=round(float(np.median(tr)), 3),
                   pairs_min_max=[round(min(tr), 3), round(max(tr), 3)],
                   pairs_inliers=int(r["inliers"][r["best"]]) if r["best"] >= 0 else 0)
        rows.append(row)
        print("truths=%d source=%d planted %d: register_sim %.3f ms (%.3f .. %.3f), %d hypotheses, %d inliers, scale %.5f, "
              "phases %s; register_pairs %.3f ms (%.3f .. %.3f), %d hypotheses, %d inliers"
              % (n_truths, len(src), planted, row["sim_ms"], min(ts), max(ts), row["sim_hypotheses"], row["sim_inliers"],
                 row["sim_scale"], phases, row["pairs_ms"], min(tr), max(tr), row["pairs_hypotheses"], row["pairs_inliers"]),
              flush=True)
    print(json.dumps(dict(bench="register_sim", reps=a.reps, rows=rows)))


if __name__ == "__main__":
    main()
