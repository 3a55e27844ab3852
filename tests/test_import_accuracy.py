"""The import conversion (tmpx = D cos a sin b, tmpy = D sin a cos b, tmpz = D cos a; FrmMain.cs:1025-1062) against
the truth: tests/golden/import_rows.npz holds, for ~2000 rows -- random ones, the zeros of cos and sin, angle 0, angles
up to 1e9 degrees, distances at the filter's edges and down into the subnormals -- the 60-digit values at the binary64
angles.  Here, on the CPU: the fixture is what its generator produces, and the host oracle meets the budget derived
for the host: glibc's sin and cos are within 1 ulp (<= 1 unit of 2^-52 relative), tmpx and tmpy add two product
roundings of half a unit each -> 1 + 1 + 2 * 0.5 = 3 units; tmpz has one function and one rounding -> 1.5 units.
tests/test_import_accuracy_gpu.py holds the device to the same fixture."""
import importlib.util
import os

import numpy as np
import pytest

import import_ref as I

HOST_BUDGET = (3.0, 3.0, 1.5)


@pytest.fixture(scope="module")
def make_golden():
    pytest.importorskip("mpmath")
    path = os.path.join(os.path.dirname(I.GOLDEN), "make_golden.py")
    spec = importlib.util.spec_from_file_location("make_golden", path)
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_fixture_is_what_the_generator_writes(make_golden, tmp_path):
    f = I.load()
    g = make_golden.import_fixture()
    for k in ("rows", "angles", "hi", "lo"):
        assert g[k].tobytes() == f[k].tobytes(), k
    p = str(tmp_path / "again.npz")
    make_golden.write_npz_fixed(p, g)
    assert open(p, "rb").read() == open(I.GOLDEN, "rb").read()
    assert os.path.getsize(I.GOLDEN) <= os.path.getsize(os.path.join(os.path.dirname(I.GOLDEN), "horn_step_rows.npz"))


def test_host_libm_error_is_the_recorded_constant(make_golden):
    """L of the GPU test is 4 x I.HOST_SINCOS_UNITS: the constant is the host libm's measured worst error (glibc
    documents 1 ulp) rounded up (glibc picks its sin / cos build by CPU: a last bit on a few
    angles may differ between machines, which the constant's rounding up absorbs)."""
    m = float(make_golden.import_reference(I.load()["rows"])["host_sincos_units"])
    print("host sin/cos worst error: %.4f units of 2^-52 (constant %.4f)" % (m, I.HOST_SINCOS_UNITS))
    assert m <= I.HOST_SINCOS_UNITS <= 1.0   # (a tighter host libm only leaves the constant, and so L, where it is)


def test_fixture_rows_cover_what_they_claim():
    f = I.load()
    rows, kept = f["rows"], f["kept"]
    a = (-2) * (rows[:, 0] - f["x_angle"]) / 180 * np.pi   # FrmMain.cs:1025-1026, Math.PI == np.pi
    b = 2 * (rows[:, 1] - f["y_angle"]) / 180 * np.pi
    assert len(rows) == 2000 and (~kept).sum() > 100
    ca = np.abs(f["hi"][:, 2] / np.where(kept, rows[:, 2], 1.0))   # |cos a|
    near_zero_cos = kept & (np.abs(np.abs(a) / np.pi % 1 - 0.5) < 1e-12)
    assert near_zero_cos.sum() >= 17 * 3 and (ca[near_zero_cos] < 1e-14).all() and (ca[near_zero_cos] > 0).all()
    assert (kept & (a == 0) & (b == 0)).sum() >= 3
    assert (np.abs(a) > 1e7).sum() > 100 and (np.abs(b) > 1e7).sum() > 100
    for D in (1000.0, 1e-300, 2.2250738585072014e-308, 1e-310, 1e-320):
        assert (kept & (rows[:, 2] == D)).any()
    assert not kept[rows[:, 2] == np.nextafter(1000.0, np.inf)].any() and not kept[rows[:, 2] == 0].any()
    # the last block repeats earlier rows exactly
    first = {r.tobytes(): i for i, r in reversed(list(enumerate(rows)))}
    assert sum(first[r.tobytes()] != i for i, r in enumerate(rows)) >= 100


def test_host_oracle_within_the_host_budget(oracle):
    f = I.load()
    worst = {}
    for xdir, ydir, dedupe in ((2, 1, True), (4, 3, False)):
        o = oracle.import_convert(f["rows"], f["x_angle"], f["y_angle"], xdir, ydir, dedupe)
        assert np.array_equal(o["state"] != 0, f["kept"])
        tmp = I.tmp_of(o["xyz"], xdir, ydir)
        e = I.error_units(tmp, f)
        worst[(xdir, ydir)] = e.max(axis=0)
        print("host oracle, xdir=%d ydir=%d: worst error %.3f %.3f %.3f units of 2^-52" % ((xdir, ydir) + tuple(e.max(axis=0))))
        for j in range(3):
            assert e[:, j].max() <= HOST_BUDGET[j], (j, int(e[:, j].argmax()), f["rows"][e[:, j].argmax()])
        # exact zeros come back as zeros: sin(0) = 0, a filtered row is all zero
        zero = f["hi"] == 0
        assert zero[f["kept"]].any() and (tmp[zero] == 0).all()
    assert np.array_equal(worst[(2, 1)], worst[(4, 3)])   # the directions only swap and negate
