"""vcp_register_pairs on the device against the numpy restatement of its definition (tests/register_ref.py): score, pick,
n_hyp, inliers and best for equality, M_all and M_best bit for bit."""
import ctypes as C

import numpy as np
import pytest

import register_ref as R
from vtkcloudpoint_amd import _native as N

pytestmark = pytest.mark.gpu

# csrc/register.hip: a workgroup's LDS queue holds 512 hypotheses (RG_QCAP) and is scored as soon as it holds more than 256
QUEUE, QUEUE_SCORED_ABOVE = 512, 256


def _check(ctx, src, tgt, bases, len_tol, inlier_dist, mirror=False, max_landmarks=200, ref=None):
    src, tgt = np.asarray(src, np.float64).reshape(-1, 3), np.asarray(tgt, np.float64).reshape(-1, 3)
    g = ctx.register_pairs(src, tgt, bases, len_tol, inlier_dist, mirror, max_landmarks)
    ref = ref or R.register(src, tgt, bases, len_tol, inlier_dist, mirror, max_landmarks)
    R.same(g, ref)
    return g


def test_two_and_two(vcp_ctx):
    # the two ordered target pairs tie on score 2: the lower (f, i, j)
    g = _check(vcp_ctx, [[0.0, 0, 0], [2.0, 0, 0]], [[1.0, 1, 0], [1.0, 3, 0]], [[0, 1]], 0.0, 0.125)
    assert g["score"].tolist() == [2] and g["pick"].tolist() == [[0, 0, 1]] and g["n_hyp"].tolist() == [2]
    assert g["inliers"].tolist() == [2] and g["best"] == 0
    assert g["M"].tolist() == [[0.0, -1.0, 0.0, 1.0], [1.0, 0.0, 0.0, 1.0], [0.0, 0.0, 1.0, 0.0], [0.0, 0.0, 0.0, 1.0]]


def test_three_and_four_with_a_known_answer(vcp_ctx):
    # the source turned by a quarter and moved by (1, 1) is targets 0..2; target 3 is far away.  The base (0, 1) has
    # length 2 and so have (0, 1) and (1, 0) only: the first puts all three points on a target, the second two
    src = [[0.0, 0, 0], [2.0, 0, 0], [0.0, 1, 0]]
    tgt = [[1.0, 1, 0], [1.0, 3, 0], [0.0, 1, 0], [5.0, 5, 0]]
    g = _check(vcp_ctx, src, tgt, [[0, 1]], 0.0, 0.25)
    assert g["score"].tolist() == [3] and g["pick"].tolist() == [[0, 0, 1]] and g["n_hyp"].tolist() == [2]
    assert g["M"].tolist() == [[0.0, -1.0, 0.0, 1.0], [1.0, 0.0, 0.0, 1.0], [0.0, 0.0, 1.0, 0.0], [0.0, 0.0, 0.0, 1.0]]
    g = _check(vcp_ctx, src, tgt, [[1, 0], [0, 2], [2, 1]], 0.0, 0.25)
    assert g["score"].tolist() == [3, 3, 3] and g["pick"].tolist() == [[0, 1, 0], [0, 0, 2], [0, 2, 1]] and g["best"] == 0


@pytest.mark.parametrize("mirror", [False, True])
def test_integer_lattice_is_all_ties(vcp_ctx, mirror):
    xy = np.array([[x, y, 0.0] for y in range(4) for x in range(4)])
    bases = [[0, 1], [0, 5], [0, 3], [5, 10], [15, 0], [1, 7], [6, 6]]
    g = _check(vcp_ctx, xy, xy, bases, 0.0, 0.5, mirror)
    # a lattice maps onto itself in many ways: every base but the degenerate one has several hypotheses of full score
    assert g["score"][:6].tolist() == [16] * 6 and g["score"][6] == -1 and g["n_hyp"].tolist() == [k * (2 if mirror else 1) for k in (48, 36, 16, 36, 4, 48, 0)]
    assert g["pick"][:6].tolist() == [[0, 0, 1], [0, 0, 5], [0, 0, 3], [0, 5, 10], [0, 0, 15], [0, 1, 7]] and g["best"] == 0


def test_length_boundary(vcp_ctx):
    # u = (0.75, 1) has length 1.25 and v = (1.5, 0) length 1.5: the difference is 0.25 exactly
    src = [[0.0, 0, 0], [0.75, 1.0, 0], [4.0, 4.0, 0]]
    tgt = [[0.0, 0, 0], [1.5, 0, 0]]
    g = _check(vcp_ctx, src, tgt, [[0, 1]], 0.25, 0.25)       # midpoint on midpoint: both ends 0.125 from their targets
    assert g["n_hyp"].tolist() == [2] and g["score"].tolist() == [2] and g["pick"].tolist() == [[0, 0, 1]]
    g = _check(vcp_ctx, src, tgt, [[0, 1]], np.nextafter(0.25, 0.0), 0.25)
    assert g["n_hyp"].tolist() == [0] and g["score"].tolist() == [-1] and g["best"] == -1
    g = _check(vcp_ctx, src, tgt, [[0, 1], [1, 0]], np.inf, 0.25)
    assert g["n_hyp"].tolist() == [2, 2]


def test_inlier_boundary(vcp_ctx):
    # the base lies on targets (0, 1) by the identity; the third point is then exactly 0.5 from target 2
    src = [[0.0, 0, 0], [2.0, 0, 0], [1.0, 1.0, 0]]
    tgt = [[0.0, 0, 0], [2.0, 0, 0], [1.0, 1.5, 0]]
    g = _check(vcp_ctx, src, tgt, [[0, 1]], 0.0, 0.5)
    assert g["score"].tolist() == [2] and g["inliers"].tolist() == [2] and g["pick"].tolist() == [[0, 0, 1]]
    assert np.array_equal(g["M"], np.eye(4))
    g = _check(vcp_ctx, src, tgt, [[0, 1]], 0.0, np.nextafter(0.5, 1.0))
    assert g["score"].tolist() == [3] and g["inliers"].tolist() == [3]


def test_mirror_on_a_reflected_scene(vcp_ctx):
    rng = np.random.default_rng(9)
    tgt = np.c_[rng.uniform(0, 10, (30, 2)), np.zeros(30)]
    P = R.planted()
    src = np.ascontiguousarray((tgt - P[:3, 3]) @ P[:3, :3]) * np.array([1.0, -1.0, 1.0])
    g1 = _check(vcp_ctx, src, tgt, [[2, 11], [4, 20]], 1e-9, 1e-6, mirror=True)
    g0 = _check(vcp_ctx, src, tgt, [[2, 11], [4, 20]], 1e-9, 1e-6, mirror=False)
    assert g1["pick"].tolist() == [[1, 2, 11], [1, 4, 20]] and g1["score"].tolist() == [30, 30]
    assert np.all(g0["score"] < 30) and np.array_equal(g1["n_hyp"], 2 * g0["n_hyp"])


def test_degenerate_inputs(vcp_ctx):
    tgt = np.array([[0.0, 0, 0], [1.0, 0, 0], [1.0, 0, 0], [0.0, 2, 0]])       # targets 1 and 2 coincide: Lv = 0
    src = np.array([[0.0, 0, 0], [1.0, 0, 0], [np.nan, 0, 0]])
    g = _check(vcp_ctx, src, tgt, [[1, 1], [0, 2], [0, 1]], 0.0, 0.25)            # a = b'; a NaN coordinate; a good base
    assert g["score"].tolist() == [-1, -1, 2] and g["n_hyp"].tolist() == [0, 0, 4] and g["best"] == 2
    g = _check(vcp_ctx, src, tgt, [[1, 1], [0, 2], [0, 1]], np.inf, 0.25)
    assert g["n_hyp"].tolist() == [0, 0, 10]                                      # 12 ordered pairs less (1, 2) and (2, 1)
    g = _check(vcp_ctx, src, tgt, [[1, 1], [0, 2], [2, 2]], np.inf, 0.25, mirror=True)
    assert g["best"] == -1 and np.array_equal(g["M"], np.eye(4)) and not g["M_all"].any()
    assert g["score"].tolist() == [-1] * 3 and g["pick"].tolist() == [[0, -1, -1]] * 3 and not g["inliers"].any()
    # a target with a non-finite coordinate makes no hypothesis and is nobody's inlier
    tgt2 = np.r_[tgt, [[np.inf, 0, 0], [3.0, np.nan, 0]]]
    _check(vcp_ctx, src, tgt2, [[0, 1]], np.inf, 0.25)
    # inlier_dist = +inf: one cell, every finite landmark counts
    g = _check(vcp_ctx, src, tgt, [[0, 1]], 0.0, np.inf)
    assert g["score"].tolist() == [2] and g["inliers"].tolist() == [2]


@pytest.mark.parametrize("nt,n_bases", [(70, 4), (40, 16)])
def test_queue_overflow(vcp_ctx, nt, n_bases):
    """len_tol = +inf: every ordered pair fits every base, so row i queues (nt - 1) * n_bases hypotheses: 276 (scored in
    the middle of the row, once the queue holds more than 256) and 624 (more than the queue's 512 slots)."""
    rng = np.random.default_rng(12)
    tgt = np.c_[rng.uniform(0, 8, (nt, 2)), np.zeros(nt)]
    src = np.c_[rng.uniform(0, 8, (16, 2)), np.zeros(16)]
    src[:10] = (tgt[:10] - R.planted()[:3, 3]) @ R.planted()[:3, :3]
    bases = np.array([(a, b) for a in range(16) for b in range(16) if a != b])[rng.permutation(240)[:n_bases]]
    assert (nt - 1) * n_bases > (QUEUE if n_bases == 16 else QUEUE_SCORED_ABOVE)
    g = _check(vcp_ctx, src, tgt, bases, np.inf, 0.1)
    assert np.all(g["n_hyp"] == nt * (nt - 1))


def test_landmark_step(vcp_ctx):
    rng = np.random.default_rng(13)
    tgt = np.c_[rng.uniform(0, 12, (300, 2)), np.zeros(300)]
    src = np.r_[tgt[:250], np.c_[rng.uniform(0, 12, (200, 2)), np.zeros(200)]]
    src = np.ascontiguousarray((src[rng.permutation(450)] - R.planted()[:3, 3]) @ R.planted()[:3, :3])
    from vtkcloudpoint_amd.icp import choose_bases
    bases = choose_bases(src, 3, 3.0, 5.0, 2)
    assert len(R.landmark_indices(450, 200)) == 225
    a = _check(vcp_ctx, src, tgt, bases, 1e-3, 0.05, max_landmarks=200)          # step 2: 225 landmarks
    b = _check(vcp_ctx, src, tgt, bases, 1e-3, 0.05, max_landmarks=450)          # every point
    c = _check(vcp_ctx, src, tgt, bases, 1e-3, 0.05, max_landmarks=10 ** 6, ref=b)
    print("landmark step: score", a["score"], b["score"], "hypotheses", a["n_hyp"])
    assert np.all(a["score"] <= 225) and np.array_equal(b["score"], b["inliers"])
    assert a["score"].max() < b["score"].max() and np.array_equal(a["n_hyp"], b["n_hyp"])


def test_4096_bases(vcp_ctx):
    rng = np.random.default_rng(14)
    tgt = np.c_[rng.integers(0, 12, (30, 2)) * 0.5, np.zeros(30)]
    src = np.ascontiguousarray((tgt[rng.permutation(30)] - R.planted()[:3, 3]) @ R.planted()[:3, :3])
    src[:, 2] = 0.0
    bases = rng.integers(0, 30, (4096, 2))
    g = _check(vcp_ctx, src, tgt, bases, 1e-6, 0.01)
    assert (g["score"] == -1).sum() >= (bases[:, 0] == bases[:, 1]).sum() > 0 and (g["score"] >= 28).sum() > 3000
    assert g["n_hyp"].sum() > 4096


@pytest.mark.parametrize("name", sorted(R.SCENES))
def test_partial_overlap_scene(vcp_ctx, name):
    """The scene of tests/test_register.py::test_reference_behaviour_on_a_partial_overlap: equal to the reference, and
    through global_icp under the same conditions."""
    from vtkcloudpoint_amd.icp import gate_schedule, global_icp, register_pairs
    sc, bases, ref = R.scene_case(name)
    g = _check(vcp_ctx, sc["source"], sc["truths"], bases, R.LEN_TOL, R.INLIER, ref=ref)
    n = sc["planted"]
    assert g["inliers"][g["best"]] >= 0.95 * n
    R.same(register_pairs(sc["source"], sc["truths"], bases, R.LEN_TOL, R.INLIER, ctx=vcp_ctx), ref)
    g0, g1, gr, rounds = R.POLISH
    p = global_icp(sc["source"], sc["truths"], bases, R.LEN_TOL, R.INLIER, gate_schedule(g0, g1, gr), max_iter=rounds,
                   ctx=vcp_ctx)
    R.same(p["registration"], ref)
    assert p["bases_used"].tolist() == np.flatnonzero(ref["score"] >= 0).tolist()
    print(name, "planted", n, "registration", g["inliers"], "after global_icp", p["inliers"])
    assert p["inliers"][p["best"]] >= 0.95 * n
    assert R.inliers_of(sc, p["M"][:3, :3], p["M"][:3, 3]) == p["inliers"][p["best"]]


def test_grid_path(vcp_ctx):
    """4000 truths: the score goes through a grid of many cells.  With len_tol = 2e-5 the reference sees 146 hypotheses
    (printed; the assertion allows up to 400)."""
    rng = np.random.default_rng(15)
    tgt = np.c_[rng.uniform(0, 60, (4000, 2)), np.zeros(4000)]
    seen = tgt[(tgt[:, 0] < 24) & (tgt[:, 1] < 24)]
    seen = seen[rng.permutation(len(seen))[:560]] + np.c_[rng.normal(0, 0.003, (560, 2)), np.zeros(560)]
    src = np.r_[seen, np.c_[rng.uniform(0, 24, (40, 2)), np.zeros(40)]]
    src = np.ascontiguousarray((src[rng.permutation(600)] - R.planted()[:3, 3]) @ R.planted()[:3, :3])
    from vtkcloudpoint_amd.icp import choose_bases
    bases = choose_bases(src, 2, 6.0, 9.0, 3)
    ref = R.register(src, tgt, bases, 2e-5, 0.05)
    print("grid path: hypotheses", ref["n_hyp"], "score", ref["score"], "inliers", ref["inliers"])
    assert 2 <= ref["n_hyp"].sum() <= 400
    g = _check(vcp_ctx, src, tgt, bases, 2e-5, 0.05, ref=ref)
    assert g["n_hyp"].sum() == ref["n_hyp"].sum()


def _raw(ctx, src, ns, tgt, nt, bases, nb, len_tol, ml, inlier, outs, M=True, best=True, have_bases=True):
    Mb, bst = outs["M"], outs["best"]
    return N.lib().vcp_register_pairs(ctx._h, N._ptr(src), C.c_int64(ns), N._ptr(tgt), C.c_int64(nt),
                                      N._ptr(bases) if have_bases else None, C.c_int32(nb), C.c_double(len_tol), 0, int(ml),
                                      C.c_double(inlier), N._ptr(Mb) if M else None, N._ptr(bst) if best else None,
                                      N._ptr(outs["M_all"]), N._ptr(outs["score"]), N._ptr(outs["inliers"]),
                                      N._ptr(outs["pick"]), N._ptr(outs["n_hyp"]))


def test_every_error_code_and_nothing_written(vcp_ctx):
    rng = np.random.default_rng(16)
    src, tgt = np.c_[rng.uniform(0, 5, (20, 2)), np.zeros(20)], np.c_[rng.uniform(0, 5, (25, 2)), np.zeros(25)]
    bases = np.array([[0, 1], [2, 3]], np.int32)
    big = np.zeros((4097, 2), np.int32)
    big[:, 1] = 1
    far = np.zeros((65537, 3))

    def outs(nb=2):
        return dict(M=np.full(16, 7.0), best=np.full(1, 77, np.int32), M_all=np.full((nb, 16), 7.0),
                    score=np.full(nb, 77, np.int32), inliers=np.full(nb, 77, np.int32), pick=np.full((nb, 3), 77, np.int32),
                    n_hyp=np.full(nb, 77, np.int64))

    def untouched(o):
        return all(np.all(v == (7.0 if v.dtype == np.float64 else 77)) for v in o.values())

    cases = [(-1, dict(nb=0)), (-1, dict(ml=0)), (-1, dict(len_tol=-1e-300)), (-1, dict(len_tol=np.nan)),
             (-1, dict(inlier=0.0)), (-1, dict(inlier=-1.0)), (-1, dict(inlier=np.nan)), (-1, dict(M=False)),
             (-1, dict(best=False)), (-1, dict(have_bases=False)),
             (-2, dict(ns=1)), (-2, dict(nt=1)), (-2, dict(ns=0)),
             (-4, dict(bases=np.array([[0, 1], [2, 20]], np.int32))), (-4, dict(bases=np.array([[-1, 1], [2, 3]], np.int32))),
             (-8, dict(bases=big, nb=4097)), (-8, dict(tgt=far, nt=65537))]
    for code, kw in cases:
        a = dict(src=src, ns=20, tgt=tgt, nt=25, bases=bases, nb=2, len_tol=0.1, ml=200, inlier=0.1)
        a.update(kw)
        o = outs(max(a["nb"], 2))
        rc = _raw(vcp_ctx, outs=o, **a)
        assert rc == code, (kw.keys(), rc)
        assert untouched(o), kw.keys()
    o = outs()                                   # and the same call without a fault runs; len_tol 0 and +inf are valid
    assert _raw(vcp_ctx, src, 20, tgt, 25, bases, 2, 0.0, 200, 0.1, o) == 0 and o["best"][0] in (-1, 0, 1)
    assert _raw(vcp_ctx, src, 20, tgt, 25, bases, 2, np.inf, 200, np.inf, o) == 0 and o["n_hyp"].tolist() == [600, 600]
    # every per-base output may be left out
    Mb, bst = np.zeros(16), np.zeros(1, np.int32)
    rc = N.lib().vcp_register_pairs(vcp_ctx._h, N._ptr(src), C.c_int64(20), N._ptr(tgt), C.c_int64(25), N._ptr(bases),
                                    C.c_int32(2), C.c_double(np.inf), 0, 200, C.c_double(np.inf), N._ptr(Mb), N._ptr(bst),
                                    None, None, None, None, None)
    assert rc == 0 and np.array_equal(Mb, o["M"]) and bst[0] == o["best"][0]
    with pytest.raises(N.VcpError) as e:
        vcp_ctx.register_pairs(src, tgt, [[0, 20]], 0.1, 0.1)
    assert e.value.code == -4


def test_dev_form_two_calls_phases_and_vcp_match(vcp_ctx):
    import torch
    sc, bases, ref = R.scene_case("half")
    src, tgt = sc["source"], sc["truths"]
    a = vcp_ctx.register_pairs(src, tgt, bases, R.LEN_TOL, R.INLIER, True)
    b = vcp_ctx.register_pairs(src, tgt, bases, R.LEN_TOL, R.INLIER, True)
    R.same(a, b)                                                      # two calls: identical bits
    B, ns, nt = len(bases), len(src), len(tgt)
    d_s, d_t, d_b = torch.from_numpy(src).cuda(), torch.from_numpy(tgt).cuda(), torch.from_numpy(bases).cuda()
    o = dict(M_all=torch.zeros((B, 4, 4), dtype=torch.float64, device="cuda"),
             score=torch.zeros(B, dtype=torch.int32, device="cuda"), inliers=torch.zeros(B, dtype=torch.int32, device="cuda"),
             pick=torch.zeros((B, 3), dtype=torch.int32, device="cuda"), n_hyp=torch.zeros(B, dtype=torch.int64, device="cuda"))
    torch.cuda.synchronize()
    r = vcp_ctx.register_pairs_dev(d_s.data_ptr(), ns, d_t.data_ptr(), nt, d_b.data_ptr(), B, R.LEN_TOL, R.INLIER, True, 200,
                                   o["M_all"].data_ptr(), o["score"].data_ptr(), o["inliers"].data_ptr(),
                                   o["pick"].data_ptr(), o["n_hyp"].data_ptr())
    got = {k: v.cpu().numpy() for k, v in o.items()}
    got.update(best=r["best"], M=r["M"])
    R.same(got, a)                                                    # the device-pointer form equals the host form
    r2 = vcp_ctx.register_pairs_dev(d_s.data_ptr(), ns, d_t.data_ptr(), nt, d_b.data_ptr(), B, R.LEN_TOL, R.INLIER, True)
    assert r2["best"] == a["best"] and np.array_equal(r2["M"], a["M"])  # the per-base arrays left out
    # inliers[b] is vcp_match's count_matched under the base's matrix
    for k in np.flatnonzero(a["score"] >= 0):
        assert vcp_ctx.match(src, tgt, a["M_all"][k], R.INLIER)["count"] == a["inliers"][k], k
    vcp_ctx.timing_enable(True)
    try:
        vcp_ctx.register_pairs(src, tgt, bases, R.LEN_TOL, R.INLIER)
        assert [p for p, _ in vcp_ctx.timing()] == ["regp_grid", "regp_search", "regp_final"]
        vcp_ctx.register_pairs(src, tgt, [[0, 0]], R.LEN_TOL, R.INLIER)   # no hypothesis at all: the same phases
        assert [p for p, _ in vcp_ctx.timing()] == ["regp_grid", "regp_search", "regp_final"]
    finally:
        vcp_ctx.timing_enable(False)
    vcp_ctx.release_workspace()                                       # the workspace is the context's own
    R.same(vcp_ctx.register_pairs(src, tgt, bases, R.LEN_TOL, R.INLIER, True), a)
