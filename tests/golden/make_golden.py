#!/usr/bin/env python3
"""Regenerates tests/golden/*.npz.

The reference (C# / .NET 3.5) cannot run here and ships no fixtures, so these are REGRESSION vectors of
the oracle itself (oracle/vcp_oracle.cpp, literal transcription) on the deterministic synthetic clouds of
vtkcloudpoint_amd/synth.py -- they pin the oracle against accidental change; the hand-derived
known-answer cases live in micro_cases.json.  Inputs are not stored (they are regenerated from the seed);
a checksum of the inputs is.

import_rows.npz is of another kind: rows for the import conversion (MainForm.AddFolder, csrc/import.hip) with the TRUE
tmpx, tmpy, tmpz of every row, evaluated with mpmath at 60 digits and stored as hi + lo, so that the GPU test needs no
mpmath.  It is written with fixed zip timestamps and no compression: regenerating it gives the same bytes.
usage: make_golden.py [oracle] [import]   (default: both)
"""
import hashlib
import io
import os
import sys
import zipfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle import binding as O  # noqa: E402
from vtkcloudpoint_amd import synth  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


IMPORT_X_ANGLE, IMPORT_Y_ANGLE = 1.5, -0.5
PI = 3.14159265358979323846  # Math.PI


def import_rows():
    """[n, 3] (motor_x, motor_y, Distance): random rows as tests/test_tools_gpu.py draws them, the zeros of cos and sin
    of both angles, angle 0, angles up to 1e6 and 1e9 degrees, Distance at 0, 1000, the next double after 1000 and tiny
    values down into the subnormals, and a block of exact duplicates of earlier rows at the end."""
    rng = np.random.default_rng(20261017)
    xa, ya = IMPORT_X_ANGLE, IMPORT_Y_ANGLE
    n = 1200
    blocks = [np.c_[rng.random(n) * 40, rng.random(n) * 40, rng.random(n) * 1100]]
    z = []
    for k in range(-8, 9):
        mxs = (xa - 45.0 * (2 * k + 1), xa - 90.0 * k)      # cos(yangjiao) = 0, sin(yangjiao) = 0
        mys = (ya + 90.0 * k, ya + 45.0 * (2 * k + 1))      # sin(fangweijiao) = 0, cos(fangweijiao) = 0
        for mx in mxs:
            z.append((mx, rng.random() * 40, rng.uniform(1, 1000)))
            for my in mys:
                z.append((mx, my, rng.uniform(1, 1000)))
        for my in mys:
            z.append((rng.random() * 40, my, rng.uniform(1, 1000)))
    blocks.append(np.array(z))
    blocks.append(np.array([(xa, ya, 1.0), (xa, ya, 777.25), (xa, 17.0, 3.5), (12.0, ya, 3.5), (xa, ya, 1000.0)]))
    for top in (1e6, 1e9):
        m = 180
        blocks.append(np.c_[rng.uniform(-top, top, m), rng.uniform(-top, top, m), rng.uniform(1, 1000, m)])
        blocks.append(np.c_[rng.uniform(-top, top, 20), rng.random(20) * 40, rng.uniform(1, 1000, 20)])
        blocks.append(np.c_[rng.random(20) * 40, rng.uniform(-top, top, 20), rng.uniform(1, 1000, 20)])
    edge = [0.0, -0.0, 1000.0, np.nextafter(1000.0, np.inf), 1e-300, 1e-305, 2.2250738585072014e-308, 1e-310, 1e-320,
            -5.0, -1e-300]                                   # (negative distances pass the C#'s filter)
    blocks.append(np.c_[5 + rng.random(len(edge)) * 30, 5 + rng.random(len(edge)) * 30, edge])
    rows = np.concatenate(blocks)
    dup = rng.integers(0, len(rows), 2000 - len(rows))
    assert len(dup) >= 100
    return np.ascontiguousarray(np.concatenate([rows, rows[dup]]))


def import_angles(rows, xa=IMPORT_X_ANGLE, ya=IMPORT_Y_ANGLE):
    """The two binary64 angles in the C#'s operation order (FrmMain.cs:1025-1026), which is part of the contract:
    near a zero of cos a re-ordered expression gives another double and a tmpz wrong in every digit."""
    a = (-2) * (rows[:, 0] - xa) / 180 * PI
    b = 2 * (rows[:, 1] - ya) / 180 * PI
    return a, b


def import_reference(rows):
    """dict(hi, lo [n, 3], kept [n], host_sincos_units): hi + lo = the 60-digit tmpx, tmpy, tmpz = D cos a sin b,
    D sin a cos b, D cos a at the binary64 angles (0 for the rows the Distance filter drops, FrmMain.cs:1011);
    host_sincos_units = the worst error of numpy's (the host libm's) sin and cos ALONE on those angles, in units of
    2^-52 relative -- tests/test_import_accuracy.py checks tests/import_ref.py's HOST_SINCOS_UNITS against it."""
    from mpmath import mp, mpf
    mp.dps = 60
    a, b = import_angles(rows)
    kept = ~((rows[:, 2] == 0) | (rows[:, 2] > 1000))
    hi = np.zeros((len(rows), 3))
    lo = np.zeros((len(rows), 3))
    worst = mpf(0)
    for i in np.flatnonzero(kept):
        D, ma, mb = mpf(float(rows[i, 2])), mpf(float(a[i])), mpf(float(b[i]))
        ca, sa, cb, sb = mp.cos(ma), mp.sin(ma), mp.cos(mb), mp.sin(mb)
        for j, v in enumerate((D * ca * sb, D * sa * cb, D * ca)):
            hi[i, j] = float(v)
            lo[i, j] = float(v - mpf(hi[i, j]))
        for true, got in ((ca, np.cos(a[i])), (sa, np.sin(a[i])), (cb, np.cos(b[i])), (sb, np.sin(b[i]))):
            if true != 0:
                worst = max(worst, abs(mpf(float(got)) - true) / abs(true) * mpf(2) ** 52)
            else:
                assert got == 0
    return dict(hi=hi, lo=lo, kept=kept, host_sincos_units=np.float64(float(worst)))


def write_npz_fixed(path, arrays):
    """np.savez with the zip timestamps pinned and no compression: the same arrays give the same bytes."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_STORED) as zf:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[name]), version=(1, 0), allow_pickle=False)
            zf.writestr(zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue())


def import_fixture():
    rows = import_rows()
    ref = import_reference(rows)
    # (the host libm's own error, ref["host_sincos_units"], is a property of the machine and stays out of the file)
    return dict(rows=rows, angles=np.array([IMPORT_X_ANGLE, IMPORT_Y_ANGLE]), hi=ref["hi"], lo=ref["lo"])


def main():
    which = sys.argv[1:] or ["oracle", "import"]
    if "import" in which:
        write_npz_fixed(os.path.join(HERE, "import_rows.npz"), import_fixture())
        print("import_rows.npz written")
    if "oracle" not in which:
        return
    d = synth.config_c1()
    l1 = O.dbscan(d["motor"], d["eps_l1"], d["min_pts"], O.L1_2D, literal=True)
    l2 = O.dbscan(d["xyz"], d["eps_l2"], d["min_pts"], O.L2_3D, literal=True)
    bp = O.block_pipeline(d["motor"], 0.3, 5, 200, 3, canonical=False, brute=True)
    K = bp["cluster_amount"]
    c3, c2, cnt = O.centroids(d["xyz"], d["motor"], bp["labels"], K, bp["order"])
    np.savez_compressed(os.path.join(HERE, "c1_dbscan.npz"), motor_sha=sha(d["motor"]), xyz_sha=sha(d["xyz"]),
                        l1_labels=l1["labels"], l1_key=l1["is_key"], l1_cf=l1["cf"], l1_evals=l1["evals"],
                        l2_labels=l2["labels"], l2_key=l2["is_key"], l2_cf=l2["cf"], l2_evals=l2["evals"],
                        bp_labels=bp["labels"], bp_block_of=bp["block_of"], bp_order=bp["order"],
                        bp_meta=np.array([bp["rows"], bp["cols"], bp["kept"], bp["del_sum"], bp["cluster_amount"]]),
                        bp_evals=bp["evals"], c3=c3, c2=c2, counts=cnt)
    c = synth.config_icp(nd=5000, nm=100, jitter=0.05)
    r = O.icp(c["model"], c["data"], 1e-4, 100, O.STOP_SSE_DELTA)
    r0 = O.icp(synth.config_icp(nd=5000, nm=100, jitter=0.0)["model"], synth.config_icp(nd=5000, nm=100, jitter=0.0)["data"],
               1e-4, 100, O.STOP_RMSE)
    np.savez_compressed(os.path.join(HERE, "icp_5k.npz"), model_sha=sha(c["model"]), data_sha=sha(c["data"]),
                        R=r["R"], T=r["T"], sse=r["sse"], rmse=r["rmse"], iters=r["iters"],
                        nn0=O.find_closest(c["model"], c["data"]), R0=r0["R"], T0=r0["T"], iters0=r0["iters"])
    print("golden written")


if __name__ == "__main__":
    main()
