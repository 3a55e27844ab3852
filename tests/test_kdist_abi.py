"""k-distance on a CPU-only box: the C-ABI symbols exist in the library, the header and the C# binding, and the
knee rule of suggest_eps gives its documented answers on hand-built curves.  No compute calls on a device."""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    with open(os.path.join(ROOT, "include", "vcp.h")) as f:
        return re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)


def _params(proto):
    proto = re.sub(r"\s+", " ", proto).strip()
    return [p for p in proto.split(",") if p.strip()]


def test_library_and_header_have_kdist():
    from vtkcloudpoint_amd import _native
    lib = _native.lib()
    src = _header()
    for name in ("vcp_kdist", "vcp_kdist_dev"):
        assert hasattr(lib, name), name
        assert re.search(r"\bint %s\s*\(" % name, src), name
        assert name in _native.SYMBOLS


def test_csharp_dllimports_match_the_header():
    src = _header()
    with open(os.path.join(ROOT, "vtkcloudpoint_amd", "host", "csharp", "VcpNative.cs")) as f:
        cs = f.read()
    for name in ("vcp_kdist", "vcp_kdist_dev"):
        c = re.search(r"\bint %s\s*\(([^)]*)\)" % name, src)
        d = re.search(r"extern int %s\s*\(([^)]*)\)" % name, cs)
        assert c and d, name
        assert len(_params(c.group(1))) == len(_params(d.group(1))) == 8, name


def test_eps_from_curve_step():
    from vtkcloudpoint_amd.kdist import eps_from_curve, suggest_eps
    curve = np.array([0.5] * 80 + [10.0] * 20)
    assert eps_from_curve(curve) == 0.5
    assert suggest_eps(None, 7, kd=curve[::-1].copy()) == 0.5  # order of kd does not matter


def test_eps_from_curve_convex_with_outlier_tail():
    from vtkcloudpoint_amd.kdist import eps_from_curve
    x = np.linspace(0.0, 1.0, 1000)
    curve = np.concatenate([0.1 + 0.05 * x, 0.15 + 3.0 * x[:200] ** 2, [1e9] * 5])  # knee at 0.15, five far points
    e = eps_from_curve(curve)
    assert 0.15 <= e <= 0.2, e
    # without the quantile clip the 1e9 tail flattens everything: the knee moves to the last non-outlier value
    assert eps_from_curve(curve, top_quantile=1.0) == curve[-6]
    # non-finite values (NaN rows, +inf rows) are not part of the curve
    assert eps_from_curve(np.concatenate([curve, [np.nan, np.inf]])) == e


def test_eps_from_curve_constant_and_empty():
    from vtkcloudpoint_amd.kdist import eps_from_curve, k_distance_curve
    assert eps_from_curve(np.full(50, 0.25)) == 0.25
    assert eps_from_curve(np.array([3.0])) == 3.0
    assert np.isnan(eps_from_curve(np.array([np.nan, np.inf])))
    assert np.array_equal(k_distance_curve([3.0, np.nan, 1.0, np.inf, 2.0]), [1.0, 2.0, 3.0])
