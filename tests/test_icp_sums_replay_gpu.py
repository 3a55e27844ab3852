"""vcp_icp_sums (csrc/icp.hip: k_icp_pass / k_icp_pass_small folded by k_icp_step) against the numpy replay of the stated
reduction tree (tests/icp_sums_ref.py), BIT FOR BIT: the 16 moment sums (NaN as NaN, the sign of zero included) and the
nearest-neighbour indices, which come from the oracle's FindClosestPointSet on the replay's transformed points.  Every
case is one pass (MODE_SUMS_ONLY).  The shapes are the smallest at which each property of the partition can go wrong:
all three paths, both workgroup sizes, one wave / one workgroup / 129 / 257 / 1024 workgroups, a partly filled second
trip, odd and even nd; at the small shapes six value families, both poses, nm at and next to the path switch, a NaN data
point, a fresh context and one on which a 1024-workgroup call has just run.  tests/test_icp_sums_tree.py proves on the
CPU that every way of getting the order wrong changes these bits."""
import numpy as np
import pytest

import icp_sums_ref as S
from test_centroid_replay_gpu import same
from vtkcloudpoint_amd import _native as N

pytestmark = pytest.mark.gpu


def check(ctx, oracle, model, data, R, T, tag):
    nn = oracle.find_closest(model, S.transform(data, R, T))
    want = S.sums(model, data, R, T, nn)
    got, gnn = ctx.icp_sums(model, data, R, T)
    assert np.array_equal(gnn, nn), (tag, "nn", np.flatnonzero(gnn != nn)[:8])
    assert same(got, want), (tag, "sums", np.flatnonzero(~((got == want) | np.isnan(want))), got, want)
    again, none = ctx.icp_sums(model, data, R, T, want_nn=False)   # the same call twice, and without the index output
    assert none is None and same(again, got), (tag, "second call")
    return got


@pytest.mark.parametrize("path,nm,nd", S.SHAPES)
def test_shapes_bit_exact(vcp_ctx, oracle, path, nm, nd):
    for pose in S.POSES if nd <= 1000 else ("generic",):
        model, data, R, T = S.case(path, nm, nd, "generic", pose)
        check(vcp_ctx, oracle, model, data, R, T, (path, nm, nd, pose))


@pytest.mark.parametrize("family", S.FAMILIES)
def test_families_at_small_shapes(vcp_ctx, oracle, family):
    for path, nm, nd in [s for s in S.SHAPES if s[2] <= 1000] + S.SMALL_SHAPES:
        for pose in S.POSES:
            model, data, R, T = S.case(path, nm, nd, family, pose)
            got = check(vcp_ctx, oracle, model, data, R, T, (family, path, nm, nd, pose))
            assert not np.signbit(got[got == 0.0]).any()   # a sum is never -0.0
            if family == "planar":                         # z = 0: products with a signed zero, sums +0.0
                assert (got[[2, 5, 8, 11, 12, 13, 14]] == 0.0).all()


@pytest.mark.parametrize("family", S.INEXACT)
def test_probes_bit_exact(vcp_ctx, oracle, family):
    """One and two points per call: the sum IS the term (or one accumulate onto it), which is where a contracted product
    accumulate or SSE expression shows (test_icp_sums_tree.py: in a long sum of squares it drowns)."""
    for k, (model, data, R, T) in enumerate(S.probes(family)):
        check(vcp_ctx, oracle, model, data, R, T, (family, "probe", k))


@pytest.mark.parametrize("path,nm,nd", [("pairs", 100, 1000), ("tiled", 600, 1000), ("grid", 600, 1000)])
def test_nan_data_point(vcp_ctx, oracle, path, nm, nd):
    """A NaN coordinate makes all of p NaN (0 * NaN in TransPoint): every sum p feeds is NaN, the sums of y are the
    replay's (FindClosestPointSet keeps model[0] for such a point)."""
    for pose in S.POSES:
        model, data, R, T = S.case(path, nm, nd, "generic", pose)
        data[nd // 3, 1] = np.nan
        got = check(vcp_ctx, oracle, model, data, R, T, (path, pose, "nan"))
        assert np.isnan(got).tolist() == [True] * 3 + [False] * 3 + [True] * 10


def test_fresh_context_and_after_a_larger_call(vcp_ctx, oracle):
    """k_icp_step reads its own launch's partial rows only: a fresh context, and the session's context right after a
    call that filled 1024 rows, followed by calls that write 1 and 13."""
    small = S.case("pairs", 100, 100, "generic")
    ctx = N.Context(0)
    try:
        check(ctx, oracle, *small, "fresh")
    finally:
        ctx.close()
    assert S.plan(100, 100)["nb"] == 1 and S.plan(600, 100)["nb"] == 13
    for path, nm, nd in (("pairs", 100, 600001), ("grid", 600, 40001)):
        big = S.case(path, nm, nd, "offset")
        assert S.plan(nm, nd)["nb"] == 1024
        check(vcp_ctx, oracle, *big, ("big", path))
        check(vcp_ctx, oracle, *S.case(path, nm, 100, "generic"), ("after big", path))
    check(vcp_ctx, oracle, *small, "small again")
