"""Runs the source of k_regp_search and of k_regs_search on the host (tools/regp_host_emulation.cpp: real threads, barriers,
wave collectives) and compares the winners' words and the hypothesis counts with tests/register_ref.py and
tests/register_sim_ref.py, for equality.  No GPU needed.

usage: python tools/regp_host_emulation.py [--sanitize] [--quick]"""
import argparse
import os
import struct
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import register_ref as R  # noqa: E402
import register_sim_ref as S  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--sanitize", action="store_true", help="build with -fsanitize=address,undefined")
ap.add_argument("--quick", action="store_true", help="leave the two larger scenes out")
args = ap.parse_args()
WORK = tempfile.mkdtemp(prefix="regp_emu_")
CSRC = os.path.join(ROOT, "vtkcloudpoint_amd", "csrc")
with open(os.path.join(CSRC, "epsgrid.hpp")) as f:
    grid = f.read()
with open(os.path.join(CSRC, "register.hip")) as f:
    text = f.read()
with open(os.path.join(WORK, "kernels.inc"), "w") as f:
    f.write(grid[grid.index("struct EpsGrid {"):grid.index("// ---- binning")])          # the grid, its cells and row ranges
    f.write(text[text.index("struct RGScan {"):text.index("// grid (source points, bases)")])  # the first struct .. the search kernels
subprocess.run(["g++", "-std=c++20", "-O1", "-g", "-pthread", "-ffp-contract=off", "-I" + WORK]
               + (["-fsanitize=address,undefined"] if args.sanitize else [])
               + [os.path.join(ROOT, "tools", "regp_host_emulation.cpp"), "-o", os.path.join(WORK, "harness")], check=True)
FAILED = []
LOW = (1 << 33) - 1
def run(name, src, tgt, bases, tol, inlier, mirror=False, ml=200, grid=True, sim=None):
    """tol: len_tol of the rigid kernel; sim = (scale_min, scale_max) runs the similarity kernel instead."""
    src = np.ascontiguousarray(src, np.float64).reshape(-1, 3); tgt = np.ascontiguousarray(tgt, np.float64).reshape(-1, 3)
    bases = np.ascontiguousarray(bases, np.int32).reshape(-1, 2)
    ns, nt, nb = len(src), len(tgt), len(bases)
    step = ns // ml if ns > ml else 1
    h = inlier * (1 + 2.0 ** -20) if (grid and np.isfinite(inlier)) else 0.0
    with open(os.path.join(WORK, 'in.bin'), 'wb') as f:
        f.write(struct.pack('6q5d', ns, nt, nb, step, int(mirror), int(sim is not None), tol, inlier, h, *(sim or (0.0, 0.0))))
        f.write(src.tobytes()); f.write(tgt.tobytes()); f.write(bases.tobytes())
    t = time.time()
    subprocess.run([os.path.join(WORK, 'harness'), os.path.join(WORK, 'in.bin'), os.path.join(WORK, 'out.bin')], check=True)
    out = np.fromfile(os.path.join(WORK, 'out.bin'), np.uint64)
    key, nh = out[:nb], out[nb:]
    score = np.where(key == 0, -1, (key >> np.uint64(33)).astype(np.int64))
    pk = LOW - (key & np.uint64(LOW)).astype(np.int64)
    pick = np.stack([pk >> 32, (pk >> 16) & 0xFFFF, pk & 0xFFFF], 1)
    pick[key == 0] = (0, -1, -1)
    if sim is None:
        ref = R.register(src, tgt, bases, tol, inlier, mirror, ml)
    else:
        ref = S.register(src, tgt, bases, sim[0], sim[1], inlier, mirror, ml)
    ok = np.array_equal(score, ref["score"]) and np.array_equal(pick, ref["pick"]) and np.array_equal(nh.astype(np.int64), ref["n_hyp"])
    print("ok  " if ok else "FAIL", name, "hyps", int(ref["n_hyp"].sum()), "%.1fs" % (time.time() - t), flush=True)
    if not ok:
        FAILED.append(name)
        print(score, ref["score"], pick.tolist(), ref["pick"].tolist(), nh, ref["n_hyp"])
rng = np.random.default_rng(12)
for nt, n_bases in ((70, 4), (40, 16)):
    rng = np.random.default_rng(12)
    tgt = np.c_[rng.uniform(0, 8, (nt, 2)), np.zeros(nt)]
    src = np.c_[rng.uniform(0, 8, (16, 2)), np.zeros(16)]
    src[:10] = (tgt[:10] - R.planted()[:3, 3]) @ R.planted()[:3, :3]
    bases = np.array([(a, b) for a in range(16) for b in range(16) if a != b])[rng.permutation(240)[:n_bases]]
    run("queue %d x %d" % (nt, n_bases), src, tgt, bases, np.inf, 0.1)
    run("queue %d x %d mirror" % (nt, n_bases), src, tgt, bases, np.inf, 0.1, True)
    run("sim queue %d x %d" % (nt, n_bases), src, tgt, bases, 0.0, 0.1, sim=(1e-3, 1e3))
    run("sim queue %d x %d mirror" % (nt, n_bases), src, tgt, bases, 0.0, 0.1, True, sim=(1e-3, 1e3))
xy = np.array([[x, y, 0.0] for y in range(4) for x in range(4)])
run("lattice mirror", xy, xy, [[0, 1], [0, 5], [0, 3], [5, 10], [15, 0], [1, 7], [6, 6]], 0.0, 0.5, True)
LATTICE = [[0, 1], [0, 5], [0, 3], [5, 10], [15, 0], [1, 7], [6, 6]]
for rng_ in ((1.0, 1.0), (2.0, 2.0), (0.5, 2.0)):
    run("sim lattice mirror [%g, %g]" % rng_, xy, xy, LATTICE, 0.0, 0.5, True, sim=rng_)
tgt = np.array([[0.0, 0, 0], [1.0, 0, 0], [1.0, 0, 0], [0.0, 2, 0], [np.inf, 0, 0], [3.0, np.nan, 0]])
src = np.array([[0.0, 0, 0], [1.0, 0, 0], [np.nan, 0, 0]])
run("degenerate", src, tgt, [[1, 1], [0, 2], [0, 1]], np.inf, 0.25, True)
run("inf inlier", src, tgt, [[0, 1]], 0.0, np.inf)
run("sim degenerate", src, tgt, [[1, 1], [0, 2], [0, 1]], 0.0, 0.25, True, sim=(1e-300, 1e300))
run("sim inf inlier", src, tgt, [[0, 1]], 0.0, np.inf, sim=(0.5, 2.0))
if args.quick:
    sys.exit(1 if FAILED else 0)
# 300 blocks, landmark step 2, multi-cell grid
rng = np.random.default_rng(13)
tgt = np.c_[rng.uniform(0, 12, (300, 2)), np.zeros(300)]
src = np.r_[tgt[:250], np.c_[rng.uniform(0, 12, (200, 2)), np.zeros(200)]]
src = np.ascontiguousarray((src[rng.permutation(450)] - R.planted()[:3, 3]) @ R.planted()[:3, :3])
from vtkcloudpoint_amd.icp import choose_bases
run("landmark step", src, tgt, choose_bases(src, 3, 3.0, 5.0, 2), 1e-3, 0.05, False, 200)
sc, bases, ref = R.scene_case("third")
run("third scene", sc["source"], sc["truths"], bases, R.LEN_TOL, R.INLIER, True)
sc, bases = S.scaled_scene("third")
run("sim third scene", sc["source"], sc["truths"], bases, 0.0, R.INLIER, True, sim=S.RANGE)
sys.exit(1 if FAILED else 0)
