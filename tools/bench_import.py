"""AddFolder's row work at 10 M rows, from the parsed rows on the host to the point where vcp_gdbscan_dev could start
(motor, dist and count resident), two ways:

  (a) host route      Context.import_convert (H2D rows, D2H xyz + state), selection of the kept rows on the host,
                      gdbscan.multiplicity on the converted triples, upload of motor / dist / count
  (b) resident route  one upload of rows, Context.import_compact_dev

Every distinct row occurs three times on average and 5 % of the rows are filtered.  Each route is warmed up once and timed
REPS times, alternating, with a host clock around work that ends in a device synchronise; the median and the spread are
printed, then the per-phase device times of (b) (hipEvents, vcp_timing), the achieved bytes per second of its passes from
the bytes the algorithm moves (counted below from the shapes), and vcp_dbscan_dev on the result for scale.
usage: python tools/bench_import.py [n] [reps] > profiles/import_compact_bench.txt"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vtkcloudpoint_amd import _native as N  # noqa: E402
from vtkcloudpoint_amd.gdbscan import multiplicity  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000_000
REPS = int(sys.argv[2]) if len(sys.argv) > 2 else 5
XA, YA = 1.51, -0.53

rng = np.random.default_rng(1)
k = max(1, int(n * 0.95 / 3))
base = np.c_[rng.random((k, 2)) * 40, 1 + rng.random(k) * 900]
rows = base[rng.integers(0, k, n)]
rows[rng.random(n) < 0.05, 2] = 1100.0
rows = np.ascontiguousarray(rows)

ctx = N.Context(0)
dev = torch.device("cuda", 0)


def route_a():
    r = ctx.import_convert(rows, XA, YA, 2, 1, dedupe=False)
    unf = np.nonzero(r["state"] != 0)[0]
    first, cnt = multiplicity(r["xyz"][unf])
    src = unf[first]
    motor = torch.from_numpy(np.ascontiguousarray(rows[src, :2])).to(dev)
    dist = torch.from_numpy(np.ascontiguousarray(rows[src, 2])).to(dev)
    count = torch.from_numpy(cnt).to(dev)
    torch.cuda.synchronize()
    return len(src), len(unf) - len(src), (motor, dist, count)


out = dict(motor=torch.empty((n, 2), dtype=torch.float64, device=dev), xyz=torch.empty((n, 3), dtype=torch.float64, device=dev),
           dist=torch.empty(n, dtype=torch.float64, device=dev))
out.update({key: torch.empty(n, dtype=torch.int32, device=dev) for key in ("src", "count", "group", "row_to")})


def route_b():
    d_rows = torch.from_numpy(rows).to(dev)
    torch.cuda.synchronize()
    m, dup = ctx.import_compact_dev(d_rows.data_ptr(), n, None, XA, YA, 2, 1, True, out["motor"].data_ptr(),
                                    out["xyz"].data_ptr(), out["dist"].data_ptr(), out["src"].data_ptr(),
                                    out["count"].data_ptr(), out["group"].data_ptr(), out["row_to"].data_ptr())
    return m, dup, d_rows


def timed(fn):
    t = time.perf_counter()
    r = fn()
    return time.perf_counter() - t, r


ra, rb = route_a(), route_b()                       # warm-up of every shape, and the two routes agree
assert ra[:2] == rb[:2], (ra[:2], rb[:2])
m, dup = rb[:2]
assert torch.equal(ra[2][0], out["motor"][:m]) and torch.equal(ra[2][1], out["dist"][:m]) and torch.equal(ra[2][2], out["count"][:m])
ta, tb = [], []
for _ in range(REPS):                               # alternating
    ta.append(timed(route_a)[0])
    tb.append(timed(route_b)[0])
print("n = %d rows, %d kept, %d duplicates, %d filtered; %d timed repetitions of each route, alternating" %
      (n, m, dup, n - m - dup, REPS))
for name, t in (("(a) host route: import_convert + host selection + multiplicity + upload", ta),
                ("(b) resident route: upload of rows + import_compact_dev", tb)):
    print("%-75s median %8.1f ms   min %8.1f   max %8.1f" % (name, np.median(t) * 1e3, min(t) * 1e3, max(t) * 1e3))
print("(a) / (b), medians: %.1f" % (np.median(ta) / np.median(tb)))

# (b) without the upload, and its phases
d_rows = rb[2]
ctx.timing_enable(True)
td, phases = [], []
for _ in range(REPS + 1):
    torch.cuda.synchronize()
    t = time.perf_counter()
    ctx.import_compact_dev(d_rows.data_ptr(), n, None, XA, YA, 2, 1, True, out["motor"].data_ptr(), out["xyz"].data_ptr(),
                           out["dist"].data_ptr(), out["src"].data_ptr(), out["count"].data_ptr(), out["group"].data_ptr(),
                           out["row_to"].data_ptr())
    td.append(time.perf_counter() - t)
    phases.append(dict(ctx.timing()))
ctx.timing_enable(False)
td, phases = td[1:], phases[1:]
print("import_compact_dev alone (rows resident): median %.2f ms   min %.2f   max %.2f" %
      (np.median(td) * 1e3, min(td) * 1e3, max(td) * 1e3))
cap = 1
while cap < 2 * n + 16:
    cap <<= 1
unf = m + dup
# bytes each phase moves, from the shapes (random table accesses counted at their 8-byte entries, not at sector size)
moved = dict(
    impc_convert=n * (24 + 24 + 24 + 1),                    # rows in; xyz, the triple and state out
    impc_dedupe=cap * 8 + n * 1 + unf * (24 + 4 + 16),      # clear; state, triple in, slot out, two table words twice
    impc_compact=(n * (1 + 4 + 4) + unf * 8                 # flags: state, slot in, keep out, the table entry
                  + n * 8                                   # scan: keep in, pos out
                  + n * (1 + 4 + 4) + unf * (8 + 4)         # scatter: state, slot in, row_to out; the entry and its pos
                  + m * (24 + 24 + 60)))                    # a kept row: rows and xyz in, 60 bytes in seven arrays out
for name in ("impc_convert", "impc_dedupe", "impc_compact"):
    ms = float(np.median([p[name] for p in phases]))
    print("  %-13s median %7.3f ms   %6.1f bytes/row   %7.1f GB/s" % (name, ms, moved[name] / n, moved[name] / ms / 1e6))
print("  all passes    %6.1f bytes/row; table: %d entries of 8 bytes (%.0f MB), 2 atomics per unfiltered row" %
      (sum(moved.values()) / n, cap, cap * 8 / 1e6))

# for scale: vcp_dbscan_dev on the compacted motor coordinates
lab = torch.zeros(m, dtype=torch.int32, device=dev)
torch.cuda.synchronize()
ts = []
for _ in range(3):
    t = time.perf_counter()
    cf, _ = ctx.dbscan_dev(out["motor"].data_ptr(), m, 2, 0.06, 10, N.L1_2D, d_labels=lab.data_ptr())
    ts.append(time.perf_counter() - t)
print("vcp_dbscan_dev on the %d kept rows (L1, eps 0.06, min_pts 10): median %.1f ms, %d clusters" %
      (m, np.median(ts[1:]) * 1e3, cf))
