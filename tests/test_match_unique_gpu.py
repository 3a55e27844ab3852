"""vcp_match_unique on the device against the sequential greedy walk of tests/match_unique_ref.py: truth_of, center_of,
pair_dist and the count for exact equality, matched_xyz against vcp_match."""
import numpy as np
import pytest

import match_unique_ref as R
from vtkcloudpoint_amd import _native, synth

pytestmark = pytest.mark.gpu
I4 = np.eye(4)


def _check(ctx, c, t, M, md, ref=None):
    c, t = np.asarray(c, np.float64).reshape(-1, 3), np.asarray(t, np.float64).reshape(-1, 3)
    g = ctx.match_unique(c, t, M, md)
    ref = ref or R.greedy_matching(c, t, M, md)
    for k in ("truth_of", "center_of", "pair_dist"):
        assert np.array_equal(g[k], ref[k]), (k, int((g[k] != ref[k]).sum()))
    assert g["count"] == ref["count"]
    assert 0 <= g["rounds"] <= min(len(c), len(t)) and (g["rounds"] > 0) == (g["count"] > 0)
    v = ctx.match(c, t, M, md)
    assert np.array_equal(g["matched_xyz"].view(np.uint64), v["matched_xyz"].view(np.uint64))
    return g, v


def test_one_and_one(vcp_ctx):
    g, _ = _check(vcp_ctx, [[0.0, 0, 0]], [[0.25, 0, 0]], I4, 1.0)
    assert g["truth_of"].tolist() == [0] and g["pair_dist"].tolist() == [0.25] and g["rounds"] == 1
    g, _ = _check(vcp_ctx, [[0.0, 0, 0]], [[0.25, 0, 0]], I4, 0.25)
    assert g["truth_of"].tolist() == [-1] and g["count"] == 0


def test_three_and_two_two_and_three(vcp_ctx):
    t = np.array([[0.0, 0, 0], [0.0, 0.875, 0]])
    c = np.array([[0.0, 0.375, 0], [0.25, 0, 0], [5.0, 5, 5]])
    g, v = _check(vcp_ctx, c, t, I4, 1.0)
    assert g["truth_of"].tolist() == [1, 0, -1] and v["nearest"][:2].tolist() == [0, 0] and v["count"] == 2
    g, _ = _check(vcp_ctx, c, t, I4, 0.5)
    assert g["truth_of"].tolist() == [-1, 0, -1] and g["center_of"].tolist() == [1, -1]
    # ties: by j, then by i
    g, _ = _check(vcp_ctx, [[0.0, 1, 0], [0.0, -1, 0]], [[1.0, 0, 0], [-1.0, 0, 0], [0.0, 0, 1]], I4, 9.0)
    assert g["truth_of"].tolist() == [0, 1] and g["center_of"].tolist() == [0, 1, -1]
    g, _ = _check(vcp_ctx, [[1.0, 0, 0], [-1.0, 0, 0], [0.0, 3, 0]], [[0.0, 0, 0], [0.0, 2, 0]], I4, 2.0)
    assert g["truth_of"].tolist() == [0, -1, 1]


@pytest.mark.parametrize("md", [0.6, 0.5])
def test_lattice_with_exact_ties_and_duplicates(vcp_ctx, md):
    c, t = R.lattice()
    assert len(c) == 2200 and len(t) == 2000 and len(np.unique(t, axis=0)) < len(t) and len(np.unique(c, axis=0)) < len(c)
    g, v = _check(vcp_ctx, c, t, I4, md)
    assert g["count"] < v["count"] and g["rounds"] >= 2


def test_chain_takes_many_rounds(vcp_ctx):
    c, t = R.chain(300)
    g, v = _check(vcp_ctx, c, t, I4, 2.0)
    assert g["truth_of"].tolist() == list(range(300)) and v["nearest"].tolist() == list(range(300))
    assert 1 <= g["rounds"] <= 300


def _edge_case():
    md = 0.5
    h = md * (1.0 + 2.0 ** -20)
    rng = np.random.default_rng(31)
    t = np.c_[rng.uniform(0, 10, (2994, 2)), rng.uniform(0, 1, 2994)]
    corners = np.array([[0.0, 0, 0], [10.0, 10, 1]])                     # the box's minimum and maximum corner
    kk = np.array([3.0, 7.0, 11.0, 16.0])
    tb = np.c_[kk * h - 1e-9, [2.0, 4.0, 6.0, 8.0], [0.5] * 4]           # just below a cell boundary in x
    t = np.r_[corners, tb, t]
    near = md * (1.0 - 2.0 ** -40)
    c = [corners[0] - [near, 0, 0], corners[0] - [md, 0, 0], corners[0] - [md * (1 + 2.0 ** -40), 0, 0],
         corners[1] + [near, 0, 0], corners[1] + [0, md, 0], corners[1] + [0, 0, md * (1 + 2.0 ** -40)],
         corners[0] - [0.3, 0.3, 0.3], corners[1] + [0.2, 0.2, 0.2], corners[1] + [2.0, 0, 0], corners[0] - [0, 9.0, 0]]
    c += [r + [near, 0, 0] for r in tb]                                  # across the boundary, just inside max_dist
    c = np.r_[np.array(c), np.c_[rng.uniform(-0.6, 10.6, (600, 2)), rng.uniform(-0.6, 1.6, 600)]]
    return c, t, md


def test_grid_edges_on_few_and_many_truths(vcp_ctx):
    c, t, md = _edge_case()
    for T in (40, 3000):
        g, _ = _check(vcp_ctx, c, t[:T], I4, md)
        d0 = R.distances(c[:6], np.r_[t[:1].repeat(3, 0), t[1:2].repeat(3, 0)])
        assert (d0 < md).tolist() == [True, False, False, True, False, False]
        assert g["count"] > 0
    assert np.all(R.distances(c[10:14], t[2:6]) < md)
    assert np.all(np.floor(c[10:14, 0] / (md * (1 + 2.0 ** -20))) == np.floor(t[2:6, 0] / (md * (1 + 2.0 ** -20))) + 1)


def test_infinite_max_dist_pairs_every_truth_through_one_cell(vcp_ctx):
    rng = np.random.default_rng(32)
    c, t = rng.normal(0, 3, (700, 3)), rng.normal(0, 3, (500, 3))
    g, _ = _check(vcp_ctx, c, t, I4, np.inf)
    assert g["count"] == 500 and np.all(g["center_of"] >= 0)


def test_degenerate_thresholds_and_non_finite_points(vcp_ctx):
    rng = np.random.default_rng(33)
    t = rng.uniform(0, 5, (300, 3))
    c = t[rng.permutation(300)[:200]] + rng.normal(0, 0.02, (200, 3))
    for md in (np.nan, 0.0, -1.0):
        g, _ = _check(vcp_ctx, c, t, I4, md)
        assert g["count"] == 0 and g["rounds"] == 0 and np.all(g["truth_of"] == -1) and np.all(g["center_of"] == -1)
        assert np.all(np.isinf(g["pair_dist"]))
    c2, t2 = c.copy(), t.copy()
    c2[5, 0], c2[17, 2], t2[40, 1] = np.nan, np.inf, np.nan
    for md in (0.2, np.inf):
        g, _ = _check(vcp_ctx, c2, t2, I4, md)
        assert g["truth_of"][5] == -1 and g["truth_of"][17] == -1 and g["center_of"][40] == -1
        assert g["count"] > 150  # the other pairs are still there (which ones: the reference above)
    # every truth non-finite: nobody pairs
    g, _ = _check(vcp_ctx, c[:20], np.full((7, 3), np.nan), I4, 1.0)
    assert g["count"] == 0


def test_empty_lists_and_null_arguments(vcp_ctx):
    g = vcp_ctx.match_unique(np.zeros((0, 3)), [[1.0, 2, 3], [4.0, 5, 6]], I4, 1.0)
    assert g["count"] == 0 and g["center_of"].tolist() == [-1, -1] and len(g["truth_of"]) == 0
    with pytest.raises(_native.VcpError) as e:
        vcp_ctx.match_unique([[0.0, 0, 0]], np.zeros((0, 3)), I4, 1.0)
    assert e.value.code == -2  # VCP_ERR_EMPTY
    import ctypes as C
    lib, z, cnt = _native.lib(), np.zeros(3), C.c_int32(0)
    out = np.zeros(1, np.int32)
    p = lambda a: None if a is None else C.c_void_p(a.ctypes.data)
    for M, to, co in ((None, out, out), (I4.reshape(16), None, out), (I4.reshape(16), out, None)):
        rc = lib.vcp_match_unique(vcp_ctx._h, p(z), C.c_int32(1), p(z), C.c_int32(1), p(M), C.c_double(1.0), None, p(to),
                                  p(co), None, C.byref(cnt), None)
        assert rc == -1  # VCP_ERR_ARG


def test_rotation_and_translation_with_nearly_equal_distances(vcp_ctx):
    rng = np.random.default_rng(34)
    M = np.eye(4)
    M[:3, :3] = synth.rotation_about((1.0, 2.0, -0.5), 17.0)
    M[:3, 3] = (0.3, -1.2, 2.5)
    t = np.c_[rng.integers(0, 25, (1500, 2)), rng.integers(0, 3, 1500)] * 0.5 + rng.normal(0, 1e-9, (1500, 3))
    want = np.c_[rng.integers(0, 50, (1700, 2)), rng.integers(0, 6, 1700)] * 0.25 + rng.normal(0, 1e-9, (1700, 3))
    c = (want - M[:3, 3]) @ M[:3, :3]  # M * (c, 1) ~ want
    g, v = _check(vcp_ctx, c, t, M, 0.6)
    assert g["count"] > 500 and g["count"] < v["count"]


def test_p2_agreement_with_vcp_match_where_nearest_is_injective(vcp_ctx):
    rng = np.random.default_rng(35)
    t = np.c_[rng.permutation(4000)[:1500] * 1.0, rng.uniform(0, 0.2, 1500), rng.uniform(0, 0.2, 1500)]
    c = np.r_[t[rng.permutation(1500)[:1200]] + rng.normal(0, 0.02, (1200, 3)), rng.uniform(-50, -10, (100, 3))]
    g, v = _check(vcp_ctx, c, t, I4, 0.45)
    got = v["nearest"][v["is_matched"] == 1]
    assert len(got) == 1200 and len(set(got.tolist())) == len(got)
    assert np.array_equal(g["truth_of"], np.where(v["is_matched"] == 1, v["nearest"], -1)) and g["count"] == v["count"]


def test_dev_form_repeatability_and_timing_phases(vcp_ctx):
    import torch
    c, t = R.lattice(seed=11)
    M = np.eye(4)
    M[:3, 3] = (0.01, -0.02, 0.03)
    a = vcp_ctx.match_unique(c, t, M, 0.6)
    b = vcp_ctx.match_unique(c, t, M, 0.6)
    for k in ("matched_xyz", "truth_of", "center_of", "pair_dist"):
        assert np.array_equal(a[k], b[k]), k
    assert (a["count"], a["rounds"]) == (b["count"], b["rounds"])
    K, T = len(c), len(t)
    d_c, d_t = torch.from_numpy(c).cuda(), torch.from_numpy(t).cuda()
    o = dict(matched_xyz=torch.zeros((K, 3), dtype=torch.float64, device="cuda"),
             truth_of=torch.zeros(K, dtype=torch.int32, device="cuda"),
             center_of=torch.zeros(T, dtype=torch.int32, device="cuda"),
             pair_dist=torch.zeros(K, dtype=torch.float64, device="cuda"))
    torch.cuda.synchronize()
    r = vcp_ctx.match_unique_dev(d_c.data_ptr(), K, d_t.data_ptr(), T, M, 0.6, o["truth_of"].data_ptr(),
                                 o["center_of"].data_ptr(), o["pair_dist"].data_ptr(), o["matched_xyz"].data_ptr())
    for k, v in o.items():
        assert np.array_equal(v.cpu().numpy(), a[k]), k
    assert (r["count"], r["rounds"]) == (a["count"], a["rounds"])
    # the optional outputs left out
    o2 = dict(truth_of=torch.zeros(K, dtype=torch.int32, device="cuda"), center_of=torch.zeros(T, dtype=torch.int32, device="cuda"))
    torch.cuda.synchronize()
    r = vcp_ctx.match_unique_dev(d_c.data_ptr(), K, d_t.data_ptr(), T, M, 0.6, o2["truth_of"].data_ptr(),
                                 o2["center_of"].data_ptr())
    assert np.array_equal(o2["truth_of"].cpu().numpy(), a["truth_of"]) and r["count"] == a["count"]
    vcp_ctx.timing_enable(True)
    try:
        vcp_ctx.match_unique(c, t, M, 0.6)
        assert [p for p, _ in vcp_ctx.timing()] == ["matchu_grid", "matchu_rounds"]
        vcp_ctx.match_unique(c, t, M, np.nan)
        assert [p for p, _ in vcp_ctx.timing()] == ["matchu_grid", "matchu_rounds"]
    finally:
        vcp_ctx.timing_enable(False)


def test_matcher_one_to_one(vcp_ctx):
    from vtkcloudpoint_amd.datamodel import Point3D
    from vtkcloudpoint_amd.tools import Matcher
    t = np.array([[0.0, 0, 0], [0.0, 0.875, 0], [9.0, 9, 9]])
    cen = []
    for x, y in ((0.0, 0.375), (0.25, 0.0), (5.0, 5.0)):
        p = Point3D()
        p.tmp_X, p.tmp_Y, p.tmp_Z = x, y, 0.0
        cen.append(p)
    m = Matcher(cen, t, I4, vcp_ctx)
    assert m.RecorrectMatchingPtsByDistance(1.0) == 2 and m.matchedID == [0, 0]  # the reference's rule: t0 twice
    assert m.MatchOneToOne(1.0) == 2
    assert m.matchedID == [1, 0] and m.unmatchedTruths == [2]
    assert [p.isMatched for p in cen] == [True, True, False] and [cen[0].matchNum, cen[1].matchNum] == [1, 0]
    assert (cen[0].matched_X, cen[0].matched_Y) == (0.0, 0.375)


def test_field_of_thirty_thousand_truths_with_contested_ones(vcp_ctx):
    c, t = R.field(seed=41)
    assert len(t) == 30000 and len(c) == 30000 and not t[:, 2].any()
    g, v = _check(vcp_ctx, c, t, I4, 0.1)  # five jitter sigmas
    assert g["count"] < v["count"]
    assert g["count"] > 25000
