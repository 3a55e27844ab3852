"""Reading tests/golden/import_rows.npz (written by tests/golden/make_golden.py) and measuring an import conversion
against it.  No mpmath here: the fixture carries the 60-digit values as hi + lo."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "import_rows.npz")
UNIT = 2.0 ** -52
SPACING = 2.0 ** -1074   # below the normal range a product rounds to this grid: the unit cannot get smaller
# The worst error of the host libm's sin and cos alone on the fixture's angles against mpmath, in units of 2^-52
# relative (measured 0.4938 with glibc; tests/test_import_accuracy.py re-measures it and fails if it is larger or
# much smaller).  The device libm's bound L is 4 times this (tests/test_import_accuracy_gpu.py).
HOST_SINCOS_UNITS = 0.494


def load():
    z = np.load(GOLDEN)
    f = {k: z[k] for k in z.files}
    f["x_angle"], f["y_angle"] = (float(v) for v in f["angles"])
    f["kept"] = ~((f["rows"][:, 2] == 0) | (f["rows"][:, 2] > 1000))   # FrmMain.cs:1011
    return f


def tmp_of(xyz, xdir, ydir):
    """(tmpx, tmpy, tmpz) back from the direction-mapped X, Y, Z: 1 = tmpy, 2 = tmpx, 3 = -tmpy, 4 = -tmpx."""
    out = np.full(xyz.shape, np.nan)
    for col, d in ((0, xdir), (1, ydir)):
        out[:, {1: 1, 2: 0, 3: 1, 4: 0}[d]] = xyz[:, col] * (1.0 if d < 3 else -1.0)
    out[:, 2] = xyz[:, 2]
    return out


def error_units(tmp, f):
    """[n, 3]: |tmp - (hi + lo)| in units of 2^-52 |true value| (of the subnormal spacing where that is larger)."""
    unit = np.maximum(np.abs(f["hi"]) * UNIT, SPACING)
    return np.abs((tmp - f["hi"]) - f["lo"]) / unit
