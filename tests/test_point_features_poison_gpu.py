"""The entry points of include/vcp_features.h under an overwritten workspace, as tests/test_planes_poison_gpu.py holds those
of vcp_planes.h: vcp_selftest_poison fills every workspace buffer the context lists (the b_pf_* of csrc/point_features.hip
are listed like the others), the pinned scratch and the staging area with a known word before each call, and every output
is compared with the restatement tests/point_features_ref.py.  Words 0x00000000, 0x00000001, then 0xFFFFFFFF (NaN as a
double, -1 as an index).  The module has a context of its own; the session's is never armed.

Without a GPU: the case list names every function of the header whose first parameter is a vcp_ctx*."""
import os
import re

import numpy as np
import pytest

import point_features_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORDS = (0x00000000, 0x00000001, 0xFFFFFFFF)


def _dev(a):
    import torch
    return torch.from_numpy(np.array(a, order="C")).cuda()


_want = {}


def _features(on_device, D, k):
    def check(ctx):
        from vtkcloudpoint_amd import features as FT
        rows, _, _ = FT.point_features_shape(ctx)
        n = 2 * rows + 3
        if (D, k) not in _want:
            pts, nbr = R.generic_rows(n, D, 50 + k), R.mixed_nbr(n, k, 51)
            _want[D, k] = (pts, nbr, R.features(pts, nbr, (0.25, 0.5, -1.0)[:D]))
        pts, nbr, want = _want[D, k]
        f = FT.point_features(_dev(pts) if on_device else pts, neighbours=_dev(nbr) if on_device else nbr,
                              viewpoint=(0.25, 0.5, -1.0)[:D], ctx=ctx)
        d = R.differs(R.as_dict(f), want)
        assert d is None and want["valid"].sum() > n // 2, d
    return check


def _own_neighbours(on_device):
    """neighbours=None: vcp_kdist's workspace is in play between the poison and the feature pass."""
    def check(ctx):
        from vtkcloudpoint_amd import features as FT
        import kdist_ref
        if "knn" not in _want:
            pts = R.generic_rows(700, 3, 52)
            knn = kdist_ref.brute_rows(pts, 9, kdist_ref.L2_3D, np.arange(700))[1]
            _want["knn"] = (pts, knn, R.features(pts, knn, (0.0, 0.0, 0.0)))
        pts, knn, want = _want["knn"]
        f = FT.point_features(_dev(pts) if on_device else pts, k=9, ctx=ctx)
        assert np.array_equal(f.knn.cpu().numpy() if on_device else f.knn, knn) and R.differs(R.as_dict(f), want) is None
    return check


def _shape(ctx):
    from vtkcloudpoint_amd import features as FT
    a = FT.point_features_shape(ctx)
    assert a == FT.point_features_shape(ctx) and a[0] >= 64 and a[1] >= 1


CASES = [
    ("features/host/3d/k9", ("vcp_point_features",), _features(False, 3, 9)),
    ("features/dev/3d/k9", ("vcp_point_features_dev",), _features(True, 3, 9)),
    ("features/host/2d/k33", ("vcp_point_features",), _features(False, 2, 33)),
    ("features/dev/2d/k33", ("vcp_point_features_dev",), _features(True, 2, 33)),
    ("features/host/own_neighbours", ("vcp_point_features",), _own_neighbours(False)),
    ("features/dev/own_neighbours", ("vcp_point_features_dev",), _own_neighbours(True)),
    ("shape", ("vcp_point_features_shape",), _shape),
]


def context_functions():
    """Every function of vcp_features.h whose first parameter is a vcp_ctx* (the regex of tests/test_poison_cases.py)."""
    with open(os.path.join(ROOT, "include", "vcp_features.h")) as f:
        src = f.read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    src = re.sub(r"//[^\n]*", "", src)
    return sorted(set(re.findall(r"\b(vcp_[a-z0-9_]+)\s*\(\s*(?:const\s+)?vcp_(?:ctx|multi)\s*\*", src)))


def test_the_case_list_names_every_context_entry_point():
    funcs = context_functions()
    named = {f for _, fs, _ in CASES for f in fs}
    assert funcs == ["vcp_point_features", "vcp_point_features_dev", "vcp_point_features_shape"]
    assert sorted(named) == funcs
    assert len({name for name, _, _ in CASES}) == len(CASES)


_state = dict(fatal=None, most=0)


@pytest.fixture(scope="module")
def ctx():
    from vtkcloudpoint_amd import _native as N
    c = N.Context(0)
    yield c
    c.selftest_poison(0, armed=False)
    c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", [c[0] for c in CASES])
def test_case_under_every_word(ctx, name):
    if _state["fatal"]:                                  # the device reported an error: nothing more runs on it from here
        pytest.fail("not started: " + _state["fatal"])
    check = {c[0]: c[2] for c in CASES}[name]
    try:
        try:
            check(ctx)                                   # unpoisoned: the case is sound
            for word in WORDS:                           # 0xFFFFFFFF only after 0 and 1 have passed
                _, nbufs = ctx.selftest_poison(word)
                _state["most"] = max(_state["most"], nbufs)
                try:
                    check(ctx)
                except AssertionError as e:
                    raise AssertionError("under the word 0x%08X: %s" % (word, e)) from e
        finally:
            ctx.selftest_poison(0, armed=False)
    except AssertionError:
        raise
    except BaseException as e:                           # VcpError, a torch RuntimeError, ...: nothing more runs on the device
        _state["fatal"] = "%s ended with %s: %s" % (name, type(e).__name__, " ".join(str(e).split())[:300])
        raise


@pytest.mark.gpu
def test_the_fill_reaches_the_features_buffers(ctx):
    """After the cases the context lists the two b_pf_* buffers of csrc/point_features.hip beside those of vcp_kdist, and
    the hook fills them."""
    if _state["fatal"]:
        pytest.fail("not started: " + _state["fatal"])
    with open(os.path.join(ROOT, "vtkcloudpoint_amd", "csrc", "point_features.hip")) as f:
        members = re.findall(r"^\s*DevBuf\s+([^;]+);", f.read(), flags=re.M)
    names = [m.strip() for d in members for m in d.split(",")]
    assert len(names) == 2 and all(re.fullmatch(r"b_pf_\w+", m) for m in names)
    {c[0]: c[2] for c in CASES}["features/host/3d/k9"](ctx)
    try:
        _, nbufs = ctx.selftest_poison(WORDS[0])
    finally:
        ctx.selftest_poison(0, armed=False)
    assert max(nbufs, _state["most"]) >= len(names) + 2         # + the buffers of vcp_kdist at the least
