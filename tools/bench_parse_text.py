"""Scan text -> resident rows at 1 M and 10 M rows, F6 text (what the reference writes, class 1) and 17-digit text ("%.17g",
class 2), generated in memory: 1 M distinct lines, the 10 M text is that text ten times over.

  * io.read_scan_text (the Python reader) in full at 1 M rows; its 10 M figure is that time x 10, labelled as extrapolated
  * Context.parse_scan_text_dev per phase (hipEvents, vcp_timing) and as a whole (host clock around the blocking call),
    with the staged parse kernel (a workgroup's lines copied to LDS first) and the direct one (VCP_TXT_DIRECT=1, bytes
    read from global memory), alternating; n_host = the lines the host had to parse
  * io.read_folder_resident on four files through import_compact_dev, then vcp_dbscan_dev on the kept rows
Every shape is warmed up once; REPS timed repetitions, median / min / max.
usage: python tools/bench_parse_text.py [reps] > profiles/parse_text_bench.txt"""
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vtkcloudpoint_amd import _native as N  # noqa: E402
from vtkcloudpoint_amd import io as vio  # noqa: E402

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 5
M1 = 1_000_000

rng = np.random.default_rng(1)
k = M1 // 3
base = np.c_[rng.random((k, 2)) * 40, 1 + rng.random(k) * 900]
rows1 = base[rng.integers(0, k, M1)]                     # every distinct row three times on average
rows1[rng.random(M1) < 0.05, 2] = 1100.0                 # 5 % filtered by the import
TEXT = {}
for kind, fmt in (("F6", "%.6f\t%.6f\t%.6f\r\n"), ("17-digit", "%.17g\t%.17g\t%.17g\r\n")):
    TEXT[kind, M1] = "".join([fmt % (a, b, c) for a, b, c in rows1.tolist()]).encode()
    TEXT[kind, 10 * M1] = TEXT[kind, M1] * 10

ctx = N.Context(0)
dev = torch.device("cuda", 0)


def stats(t):
    return "median %9.2f ms   min %9.2f   max %9.2f" % (np.median(t) * 1e3, min(t) * 1e3, max(t) * 1e3)


tmp = tempfile.mkdtemp()
print("1 M distinct rows; the 10 M text is the 1 M text ten times.  %d timed repetitions, one warm-up" % REPS)
for kind in ("F6", "17-digit"):
    path = os.path.join(tmp, "one.txt")
    with open(path, "wb") as f:
        f.write(TEXT[kind, M1])
    t = time.perf_counter()
    want = vio.read_scan_text(path)
    t_py = time.perf_counter() - t
    print("\n%s text, %.1f bytes per line" % (kind, len(TEXT[kind, M1]) / M1))
    print("  io.read_scan_text, 1 M rows, in full (one run)          %9.0f ms" % (t_py * 1e3))
    print("  io.read_scan_text, 10 M rows, EXTRAPOLATED (x 10)       %9.0f ms" % (t_py * 1e4))
    for n in (M1, 10 * M1):
        text = TEXT[kind, n]
        d_rows = torch.empty((n, 3), dtype=torch.float64, device=dev)
        d_group = torch.empty(n, dtype=torch.int32, device=dev)
        res = {}
        for mode in ("staged", "direct", "staged", "direct") + ("staged", "direct") * REPS:    # two warm-ups each
            os.environ["VCP_TXT_DIRECT"] = "1" if mode == "direct" else "0"
            ctx.timing_enable(True)
            torch.cuda.synchronize()
            t = time.perf_counter()
            r = ctx.parse_scan_text_dev(text, n, d_rows.data_ptr(), d_group.data_ptr())
            dt = time.perf_counter() - t
            res.setdefault(mode, []).append((dt, dict(ctx.timing()), r["n_host"]))
            assert r["n"] == n
        ctx.timing_enable(False)
        os.environ["VCP_TXT_DIRECT"] = "0"
        if n == M1:
            assert np.array_equal(d_rows.cpu().numpy().view(np.uint64), want.view(np.uint64)), "differs from read_scan_text"
        print("  parse_scan_text_dev, %d rows, %d bytes; lines parsed on the host (n_host): %d of %d" %
              (n, len(text), res["staged"][-1][2], n))
        for mode in ("staged", "direct"):
            runs = res[mode][2:]
            print("    %-6s whole call (host clock)   %s" % (mode, stats([x[0] for x in runs])))
            for ph in ("txt_upload", "txt_index", "txt_parse", "txt_patch"):
                print("    %-6s   %-10s (device)      %s" % (mode, ph, stats([x[1].get(ph, 0.0) * 1e-3 for x in runs])))
        del d_rows, d_group

# end to end: four files -> read_folder_resident -> dbscan_dev
for kind in ("F6", "17-digit"):
    text = TEXT[kind, 10 * M1]
    cut = [0]
    for q in (1, 2, 3):
        cut.append(text.index(b"\n", len(text) * q // 4) + 1)
    cut.append(len(text))
    paths = []
    for q in range(4):
        paths.append(os.path.join(tmp, "part%d.txt" % q))
        with open(paths[-1], "wb") as f:
            f.write(text[cut[q]:cut[q + 1]])
    te, td = [], []
    for rep in range(REPS + 1):
        torch.cuda.synchronize()
        t = time.perf_counter()
        r = vio.read_folder_resident(paths, 1.51, -0.53, ctx=ctx)
        torch.cuda.synchronize()
        te.append(time.perf_counter() - t)
        lab = torch.zeros(r["m"], dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        t = time.perf_counter()
        cf, _ = ctx.dbscan_dev(r["motor"].data_ptr(), r["m"], 2, 0.06, 10, N.L1_2D, d_labels=lab.data_ptr())
        td.append(time.perf_counter() - t)
    print("\n%s text, 10 M rows in four files (page cache): read_folder_resident (read, upload, parse, import_compact_dev)"
          % kind)
    print("    files -> resident kept rows     %s   (%d rows, %d kept, %d duplicates, n_host %d)" %
          (stats(te[1:]), r["n"], r["m"], r["duplicates"], r["n_host"]))
    print("    vcp_dbscan_dev on the kept rows %s   (L1, eps 0.06, min_pts 10, %d clusters)" % (stats(td[1:]), cf))
    for p in paths:
        os.remove(p)
os.remove(os.path.join(tmp, "one.txt"))
os.rmdir(tmp)
