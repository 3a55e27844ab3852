"""The centroid kernels (csrc/centroids.hip) against the numpy replay of their stated summation tree
(tests/centroid_ref.py), BIT FOR BIT: c3, c2, counts, inside_num, the relabelled labels and new_k, through
Context.centroids, centroids_dev (torch device tensors), centroids_weighted and refresh_by_dictionary, on the shared
input set -- cluster sizes at and next to the wave, workgroup and chunk boundaries, empty labels in between, members
scattered over the array, K at 255 / 256 / 257 -- and on the inputs where the tree differs in kind from a sequential
sum.  tests/test_centroid_tree.py proves on the CPU that every way of getting the order wrong changes these bits.

Weighted sums: sum(w) stays below 2^31 (the C#'s insideNum is a 32-bit int); larger totals are out of scope."""
import numpy as np
import pytest

import centroid_ref as R
from vtkcloudpoint_amd import _native as N
from vtkcloudpoint_amd import synth

pytestmark = pytest.mark.gpu


def same(a, b):
    num = ~np.isnan(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b, equal_nan=True) \
        and np.array_equal(np.signbit(a)[num], np.signbit(b)[num])   # -0.0 is not +0.0 here


def check_plain(ctx, xyz, motor, lab, K, tag):
    g3, g2, gc = ctx.centroids(xyz, motor, lab, K)
    t3, t2, tc = R.tree_centroids(xyz, motor, lab, K)
    assert np.array_equal(gc, tc), tag
    assert same(g3, t3), (tag, "c3", np.flatnonzero(~((g3 == t3) | np.isnan(t3)).all(1)) + 1)
    assert same(g2, t2), (tag, "c2", np.flatnonzero(~((g2 == t2) | np.isnan(t2)).all(1)) + 1)
    return g3, g2, gc


@pytest.mark.parametrize("family", R.FAMILIES)
def test_centroids_bit_exact(vcp_ctx, family):
    xyz, motor, lab = R.case(family)
    for K in (255, 256, 257):   # the thread guards of k_nchunks (K + 1 entries) and k_centroid_final (K)
        check_plain(vcp_ctx, xyz, motor, lab, K, (family, K))
    check_plain(vcp_ctx, xyz, None, lab, 257, (family, "xyz only"))
    check_plain(vcp_ctx, None, motor, lab, 257, (family, "motor only"))


@pytest.mark.parametrize("family", R.FAMILIES)
def test_centroids_dev_bit_exact(vcp_ctx, family):
    import torch
    xyz, motor, lab = R.case(family)
    K = 256
    dx, dm, dl = (torch.from_numpy(a).cuda() for a in (xyz, motor, lab))
    d3 = torch.full((K, 3), 7.0, dtype=torch.float64, device="cuda")
    d2 = torch.full((K, 2), 7.0, dtype=torch.float64, device="cuda")
    dc = torch.full((K,), -1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    vcp_ctx.centroids_dev(dx.data_ptr(), dm.data_ptr(), dl.data_ptr(), len(lab), K, d3.data_ptr(), d2.data_ptr(),
                          dc.data_ptr())
    t3, t2, tc = R.tree_centroids(xyz, motor, lab, K)
    assert np.array_equal(dc.cpu().numpy(), tc)
    assert same(d3.cpu().numpy(), t3) and same(d2.cpu().numpy(), t2)


@pytest.mark.parametrize("family", R.FAMILIES)
def test_centroids_weighted_bit_exact(vcp_ctx, family):
    xyz, _, lab = R.case(family)
    grp, K = R.compact(lab)   # an empty list is an error in this entry point (test_tools_gpu.py covers it)
    cid, pts = R.case_weights(grp)
    for ignore in (False, True):
        for c in (cid, None):
            g3, gi = vcp_ctx.centroids_weighted(xyz, grp, c, pts, K, ignore)
            t3, ti = R.tree_centroids_weighted(xyz, grp, c, pts, K, ignore)
            assert np.array_equal(gi, ti) and gi.max() < 2 ** 31, (family, ignore, c is None)
            assert same(g3, t3), (family, ignore, c is None, np.flatnonzero((g3 != t3).any(1)) + 1)


@pytest.mark.parametrize("family", R.FAMILIES)
def test_refresh_by_dictionary_bit_exact(vcp_ctx, family):
    xyz, motor, lab = R.case(family)
    for K in (255, 256, 257):
        m = R.case_dictionary(K)
        gl, gk, g3, g2, gc = vcp_ctx.refresh_by_dictionary(xyz, motor, lab, K, m)
        tl, tk, t3, t2, tc = R.tree_refresh(xyz, motor, lab, K, m)
        assert gk == tk == 12 and np.array_equal(gl, tl) and gl.dtype == tl.dtype and np.array_equal(gc, tc)
        assert same(g3, t3) and same(g2, t2), (family, K)
    assert R.CH in gc and 2 * R.CH + 1 in gc   # merged sizes sit on chunk boundaries


@pytest.mark.parametrize("name", sorted(R.kind_cases()))
def test_differences_in_kind(vcp_ctx, name):
    """Overflow placed for or against the tree, -0.0, subnormal, inf and NaN members: the device does what the replay
    says (NaN compared as NaN, payloads not pinned); what the C# does instead is in tests/test_centroid_tree.py."""
    col = R.kind_cases()[name]
    xyz, motor, lab = R.kind_arrays(col)
    g3, _, _ = check_plain(vcp_ctx, xyz, motor, lab, 1, name)
    w3, wi = vcp_ctx.centroids_weighted(xyz, lab, None, np.ones(len(lab), np.int32), 1, False)
    t3, ti = R.tree_centroids_weighted(xyz, lab, None, np.ones(len(lab), np.int32), 1, False)
    assert np.array_equal(wi, ti) and same(w3, t3) and same(w3, g3)   # weight 1: x * 1.0 is x
    # the same members behind three full chunks of zeros: the chunk loop carries the special value through
    pad = 3 * R.CH
    xyz2 = np.concatenate([np.zeros((pad, 3)), xyz])
    motor2 = np.concatenate([np.zeros((pad, 2)), motor])
    check_plain(vcp_ctx, xyz2, motor2, np.ones(pad + len(lab), np.int32), 1, (name, "padded"))


def test_degenerate_sizes(vcp_ctx):
    c3, c2, cnt = vcp_ctx.centroids(np.zeros((0, 3)), np.zeros((0, 2)), np.zeros(0, np.int32), 3)
    assert c3.shape == (3, 3) and np.isnan(c3).all() and np.isnan(c2).all() and cnt.tolist() == [0, 0, 0]
    t3, t2, tc = R.tree_centroids(np.zeros((0, 3)), np.zeros((0, 2)), np.zeros(0, np.int32), 3)
    assert same(c3, t3) and same(c2, t2) and np.array_equal(cnt, tc)
    xyz, motor, lab = R.case("uniform")
    c3, c2, cnt = vcp_ctx.centroids(xyz, motor, np.zeros_like(lab), 0)
    assert c3.shape == (0, 3) and c2.shape == (0, 2) and cnt.shape == (0,)


def test_fresh_context_and_after_a_larger_call(vcp_ctx):
    """The result does not depend on what the context's buffers held: a fresh context, and the session's context right
    after a larger unrelated call that leaves the shared work buffers full of something else."""
    xyz, motor, lab = R.case("uniform")
    t3, t2, tc = R.tree_centroids(xyz, motor, lab, 257)
    ctx = N.Context(0)
    try:
        g3, g2, gc = ctx.centroids(xyz, motor, lab, 257)
    finally:
        ctx.close()
    assert same(g3, t3) and same(g2, t2) and np.array_equal(gc, tc)
    d = synth.config_cloud(1_000_000)
    big = vcp_ctx.dbscan(d["motor"], d["eps_l1"], d["min_pts"], N.L1_2D)
    vcp_ctx.centroids(d["xyz"], d["motor"], big["labels"], big["cf"])
    check_plain(vcp_ctx, xyz, motor, lab, 257, "after a larger call")
    grp, K = R.compact(lab)
    cid, pts = R.case_weights(grp)
    g3, gi = vcp_ctx.centroids_weighted(xyz, grp, cid, pts, K, False)
    t3, ti = R.tree_centroids_weighted(xyz, grp, cid, pts, K, False)
    assert same(g3, t3) and np.array_equal(gi, ti)
