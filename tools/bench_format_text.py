"""Resident rows -> export text at 1 M and 10 M rows of the import bench's cloud (tools/bench_import.py), F6, both exports:
the scan export (`motor_x TAB motor_y TAB Distance`, every row in turn) and the cluster export (`clusterId TAB ...`, the
labelled rows stably sorted by label; the labels are synthetic, uniform in 0..1000, so that all but 0.1 % of the rows are
written).

  * the host path, write_scan_text / write_clusters_text style ('%.6f' per number, one line per row, joined and encoded), on
    the same arrays, in full at 1 M rows; its 10 M figure is that time x 10, labelled as extrapolated
  * Context.format_rows_dev per phase (hipEvents, vcp_timing) and as a whole (host clock around the blocking call, the text
    landing in a numpy buffer that exists already), with the staged k_fmt_write (lines built in LDS, 16-byte stores) and
    the direct one (VCP_FMT_DIRECT=1, every lane stores its own bytes), alternating in one process; the count-only call
  * the 1 M texts are compared with the host path's, byte for byte
Every shape is warmed up twice per kernel; REPS timed repetitions, median / min / max.
usage: python tools/bench_format_text.py [reps] > profiles/format_rows_bench.txt"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vtkcloudpoint_amd import _native as N  # noqa: E402
from vtkcloudpoint_amd import io as vio  # noqa: E402

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 5
M1 = 1_000_000


def cloud(n):
    rng = np.random.default_rng(1)
    k = n // 3
    base = np.c_[rng.random((k, 2)) * 40, 1 + rng.random(k) * 900]
    rows = base[rng.integers(0, k, n)]                   # every distinct row three times on average
    rows[rng.random(n) < 0.05, 2] = 1100.0
    return rows, rng.integers(0, 1001, n).astype(np.int32)


def stats(t):
    return "median %9.2f ms   min %9.2f   max %9.2f" % (np.median(t) * 1e3, min(t) * 1e3, max(t) * 1e3)


def host_text(rows, labels, order):
    """(seconds, bytes): the Python writers' formatting of the same arrays."""
    t = time.perf_counter()
    if labels is None:
        text = "".join(["%.6f\t%.6f\t%.6f\r\n" % (a, b, c) for a, b, c in rows.tolist()]).encode("ascii")
    else:
        sel = rows[order]
        text = "".join(["%d\t%.6f\t%.6f\t%.6f\r\n" % (i, a, b, c)
                        for i, (a, b, c) in zip(labels[order].tolist(), sel.tolist())]).encode("ascii")
    return time.perf_counter() - t, text


ctx = N.Context(0)
print("the import bench's cloud; F6, \"\\r\\n\".  %d timed repetitions, two warm-ups per kernel" % REPS)
for n in (M1, 10 * M1):
    rows, labels = cloud(n)
    t_rows, t_lab = torch.from_numpy(rows).cuda(), torch.from_numpy(labels).cuda()
    t_sort = []
    for rep in range(REPS + 1):                          # the first run warms torch's sort up
        torch.cuda.synchronize()
        t = time.perf_counter()
        t_order = vio.cluster_order(t_lab)
        torch.cuda.synchronize()
        t_sort.append(time.perf_counter() - t)
    for export, ids, order in (("scan export", None, None), ("cluster export", t_lab, t_order)):
        m = n if order is None else len(order)
        want = None
        print("\n%s, %d rows, %d lines" % (export, n, m))
        if n == M1:
            t_py, want = host_text(rows, None if ids is None else labels, None if order is None else order.cpu().numpy())
            print("  host path ('%%.6f' per number), in full (one run)              %9.0f ms, %d bytes" % (t_py * 1e3, len(want)))
            print("  host path, 10 M rows, EXTRAPOLATED (x 10)                     %9.0f ms" % (t_py * 1e4))
            t_host = t_py
        if order is not None:
            print("  io.cluster_order on the device (torch: nonzero, stable sort)    %s" % stats(t_sort[1:]))
        p = t_rows.data_ptr()
        args = (p, 3, p + 8, 3, p + 16, 3, n, None if ids is None else ids.data_ptr(),
                None if order is None else order.data_ptr(), m)
        tc = []
        for rep in range(REPS + 1):
            t = time.perf_counter()
            nbytes = ctx.format_rows_dev(*args, bit=6, eol=1)
            tc.append(time.perf_counter() - t)
        out = np.empty(nbytes, np.uint8)
        out[:] = 0                                       # the pages exist before the first timed copy
        res = {}
        for mode in ("staged", "direct", "staged", "direct") + ("staged", "direct") * REPS:
            os.environ["VCP_FMT_DIRECT"] = "1" if mode == "direct" else "0"
            ctx.timing_enable(True)
            t = time.perf_counter()
            k = ctx.format_rows_dev(*args, bit=6, eol=1, out=out)
            dt = time.perf_counter() - t
            res.setdefault(mode, []).append((dt, dict(ctx.timing())))
            assert k == nbytes
            if want is not None and len(res[mode]) == 1:
                assert out.tobytes() == want, "differs from the host path"
        ctx.timing_enable(False)
        os.environ.pop("VCP_FMT_DIRECT")
        print("  format_rows_dev, %d bytes (%.1f per line); count-only call      %s" % (nbytes, nbytes / max(m, 1), stats(tc[1:])))
        for mode in ("staged", "direct"):
            runs = res[mode][2:]
            print("    %-6s whole call (host clock)   %s" % (mode, stats([x[0] for x in runs])))
            for ph in ("fmt_len", "fmt_write", "fmt_download"):
                print("    %-6s   %-12s (device)    %s" % (mode, ph, stats([x[1].get(ph, 0.0) * 1e-3 for x in runs])))
        if n == M1:
            for mode in ("staged", "direct"):
                print("    %-6s host path / whole call (medians)   %.1f x" %
                      (mode, t_host / np.median([x[0] for x in res[mode][2:]])))
    del t_rows, t_lab, t_order
ctx.close()
