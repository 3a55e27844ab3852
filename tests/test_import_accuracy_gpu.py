"""The device's import conversion (k_import_convert, csrc/import.hip) against the 60-digit values of
tests/golden/import_rows.npz (no mpmath needed here), with the default directions and with xdir = 4, ydir = 3.

The bound.  tmpx = D cos a sin b: two library functions, each within L units of 2^-52 relative, and two product
roundings of half a unit each -> 2 L + 1 units; tmpy alike; tmpz = D cos a -> L + 0.5.  No statement of the device
libm's accuracy for binary64 sin and cos ships with the ROCm installation, so L = 4 x the worst error of the HOST
libm's sin and cos alone on the fixture's angles against mpmath (import_ref.HOST_SINCOS_UNITS = 0.494, re-measured by
tests/test_import_accuracy.py -> L = 1.976).  The factor lets a correct but less tight libm pass; it
still rejects a binary32 intermediate (1e8 units), poor argument reduction at large angles or near the zeros (errors
of the order of the value) and a re-ordered angle expression (unbounded near the zeros)."""
import numpy as np
import pytest

import import_ref as I

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("xdir,ydir,dedupe", [(2, 1, True), (4, 3, False)])
def test_device_conversion_within_bound(vcp_ctx, oracle, xdir, ydir, dedupe):
    f = I.load()
    L = 4.0 * I.HOST_SINCOS_UNITS
    bound = (2 * L + 1, 2 * L + 1, L + 0.5)
    g = vcp_ctx.import_convert(f["rows"], f["x_angle"], f["y_angle"], xdir, ydir, dedupe)
    o = oracle.import_convert(f["rows"], f["x_angle"], f["y_angle"], xdir, ydir, dedupe)
    # the decisions are bit-exact: filter, first-occurrence duplicate removal, counters
    assert np.array_equal(g["state"], o["state"]) and g["kept"] == o["kept"] and g["duplicates"] == o["duplicates"]
    assert np.array_equal(g["state"] != 0, f["kept"])
    if dedupe:
        assert g["duplicates"] >= 100 and (g["state"] == 2).sum() == g["duplicates"]
    tmp = I.tmp_of(g["xyz"], xdir, ydir)
    e = I.error_units(tmp, f)
    print("device, xdir=%d ydir=%d: worst error %.3f %.3f %.3f units of 2^-52 (bound %.2f %.2f %.2f, L = %.3f)"
          % ((xdir, ydir) + tuple(e.max(axis=0)) + bound + (L,)))
    for j in range(3):
        i = int(e[:, j].argmax())
        assert e[i, j] <= bound[j], (j, i, f["rows"][i].tolist(), float(e[i, j]))
    zero = f["hi"] == 0   # sin(0) = 0 and the filtered rows
    assert (tmp[zero] == 0).all()
