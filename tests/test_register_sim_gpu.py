"""vcp_register_sim on the device against the numpy restatement of its definition (tests/register_sim_ref.py): score, pick,
n_hyp, inliers and best for equality, M_all, M_best and scale bit for bit; and global_sim_icp on the scaled scenes."""
import ctypes as C

import numpy as np
import pytest

import register_ref as R
import register_sim_ref as S
from vtkcloudpoint_amd import _native as N

pytestmark = pytest.mark.gpu

# csrc/register.hip: a workgroup's LDS queue holds 512 hypotheses (RG_QCAP) and is scored as soon as it holds more than 256
QUEUE, QUEUE_SCORED_ABOVE = 512, 256
LATTICE = np.array([[x, y, 0.0] for y in range(4) for x in range(4)])
LATTICE_BASES = [[0, 1], [0, 5], [0, 3], [5, 10], [15, 0], [1, 7], [6, 6]]


def _check(ctx, src, tgt, bases, lo, hi, inlier_dist, mirror=False, max_landmarks=200, ref=None):
    src, tgt = np.asarray(src, np.float64).reshape(-1, 3), np.asarray(tgt, np.float64).reshape(-1, 3)
    g = ctx.register_sim(src, tgt, bases, lo, hi, inlier_dist, mirror, max_landmarks)
    ref = ref or S.register(src, tgt, bases, lo, hi, inlier_dist, mirror, max_landmarks)
    S.same(g, ref)
    return g


def test_two_and_two(vcp_ctx):
    # a base of length 2 on two targets 4 apart: k = 2 exactly, the two orders tie on score 2: the lower (f, i, j)
    g = _check(vcp_ctx, [[0.0, 0, 0], [2.0, 0, 0]], [[1.0, 1, 0], [1.0, 5, 0]], [[0, 1]], 2.0, 2.0, 0.125)
    assert g["score"].tolist() == [2] and g["pick"].tolist() == [[0, 0, 1]] and g["n_hyp"].tolist() == [2]
    assert g["inliers"].tolist() == [2] and g["best"] == 0 and g["scale"].tolist() == [2.0]
    assert g["M"].tolist() == [[0.0, -2.0, 0.0, 1.0], [2.0, 0.0, 0.0, 1.0], [0.0, 0.0, 2.0, 0.0], [0.0, 0.0, 0.0, 1.0]]


def test_three_and_four_with_a_known_answer(vcp_ctx):
    # the source doubled, turned by a quarter and moved by (1, 1) is targets 0..2; target 3 is far away.  The base (0, 1)
    # has length 1 and only (0, 1) and (1, 0) are 2 long: the first puts all three points on a target, the second two
    src = [[0.0, 0, 0], [1.0, 0, 0], [0.0, 0.5, 0]]
    tgt = [[1.0, 1, 0], [1.0, 3, 0], [0.0, 1, 0], [5.0, 5, 0]]
    g = _check(vcp_ctx, src, tgt, [[0, 1]], 2.0, 2.0, 0.25)
    assert g["score"].tolist() == [3] and g["pick"].tolist() == [[0, 0, 1]] and g["n_hyp"].tolist() == [2]
    assert g["M"].tolist() == [[0.0, -2.0, 0.0, 1.0], [2.0, 0.0, 0.0, 1.0], [0.0, 0.0, 2.0, 0.0], [0.0, 0.0, 0.0, 1.0]]
    g = _check(vcp_ctx, src, tgt, [[1, 0], [0, 2], [2, 1]], 1.9, 2.1, 0.25)
    assert g["score"].tolist() == [3, 3, 3] and g["pick"].tolist() == [[0, 1, 0], [0, 0, 2], [0, 2, 1]] and g["best"] == 0


@pytest.mark.parametrize("mirror", [False, True])
def test_scale_one_on_the_lattice_is_the_rigid_call(vcp_ctx, mirror):
    """On the integer lattice equal lengths are bit-equal and unequal ones far apart: [1, 1] selects the pairs len_tol = 0
    selects, and with k = 1 every pose is the rigid one's bit for bit."""
    g = _check(vcp_ctx, LATTICE, LATTICE, LATTICE_BASES, 1.0, 1.0, 0.5, mirror)
    r = vcp_ctx.register_pairs(LATTICE, LATTICE, LATTICE_BASES, 0.0, 0.5, mirror)
    R.same(g, r)
    assert g["scale"].tolist() == [1.0] * 6 + [0.0]
    assert g["n_hyp"].tolist() == [k * (2 if mirror else 1) for k in (48, 36, 16, 36, 4, 48, 0)]


@pytest.mark.parametrize("lo,hi", [(2.0, 2.0), (0.5, 2.0)])
def test_lattice_at_other_scales_with_the_mirror(vcp_ctx, lo, hi):
    g = _check(vcp_ctx, LATTICE, LATTICE, LATTICE_BASES, lo, hi, 0.5, True)
    won = g["score"] >= 0
    assert g["score"][6] == -1 and won[:2].all() and g["best"] >= 0
    assert np.all((g["scale"][won] >= lo) & (g["scale"][won] <= hi)) and not g["scale"][~won].any()
    if lo == hi:
        # the unit base at twice its size: 16 ordered pairs two apart along x, 16 along y, both flips; the bases of
        # length 3 and sqrt(18) find no pair twice as long on a lattice whose points are at most 3 apart along an axis
        assert g["n_hyp"][0] == 64 and g["scale"][0] == 2.0 and g["n_hyp"][[2, 4]].tolist() == [0, 0]


def test_ratio_boundary(vcp_ctx):
    # the base is 5 long (3-4-5); A B are 10 apart, C D 15, and the other pairs give k = 4 (A C), 3.22 (B C), 4.66, 6.28
    src = [[0.0, 0, 0], [3.0, 4.0, 0], [1.0, 1.0, 0]]
    tgt = [[0.0, 0, 0], [6.0, 8.0, 0], [20.0, 0, 0], [29.0, 12.0, 0]]
    down, up = (lambda x: float(np.nextafter(x, 0.0))), (lambda x: float(np.nextafter(x, 9.0)))
    for lo, hi, n in ((1.0, 2.0, 2), (1.0, down(2.0), 0), (2.0, 3.0, 4), (up(2.0), 3.0, 2), (2.0, down(3.0), 2), (3.0, 3.0, 2),
                      (up(3.0), 3.1, 0), (3.0, 4.0, 6), (2.0, 2.0, 2)):
        g = _check(vcp_ctx, src, tgt, [[0, 1]], lo, hi, 0.25)
        assert g["n_hyp"].tolist() == [n], (lo, hi, g["n_hyp"])
        assert (g["best"] == 0 and lo <= g["scale"][0] <= hi) if n else (g["best"] == -1 and g["scale"][0] == 0.0)


def test_inlier_boundary(vcp_ctx):
    # the base doubled lies on targets (0, 1) with M = diag(2, 2, 2, 1); the third point is then exactly 0.5 from target 2
    src = [[0.0, 0, 0], [1.0, 0, 0], [0.5, 0.5, 0]]
    tgt = [[0.0, 0, 0], [2.0, 0, 0], [1.0, 1.5, 0]]
    g = _check(vcp_ctx, src, tgt, [[0, 1]], 2.0, 2.0, 0.5)
    assert g["score"].tolist() == [2] and g["inliers"].tolist() == [2] and g["pick"].tolist() == [[0, 0, 1]]
    assert np.array_equal(g["M"], np.diag([2.0, 2.0, 2.0, 1.0]))
    g = _check(vcp_ctx, src, tgt, [[0, 1]], 2.0, 2.0, np.nextafter(0.5, 1.0))
    assert g["score"].tolist() == [3] and g["inliers"].tolist() == [3]


def test_mirror_on_a_reflected_scene(vcp_ctx):
    rng = np.random.default_rng(9)
    tgt = np.c_[rng.uniform(0, 10, (30, 2)), np.zeros(30)]
    P = R.planted()
    src = np.ascontiguousarray((tgt - P[:3, 3]) @ P[:3, :3]) * np.array([1.0, -1.0, 1.0]) / 3.0
    g1 = _check(vcp_ctx, src, tgt, [[2, 11], [4, 20]], 2.9, 3.1, 1e-6, mirror=True)
    g0 = _check(vcp_ctx, src, tgt, [[2, 11], [4, 20]], 2.9, 3.1, 1e-6, mirror=False)
    assert g1["pick"].tolist() == [[1, 2, 11], [1, 4, 20]] and g1["score"].tolist() == [30, 30]
    assert np.all(g0["score"] < 30) and np.array_equal(g1["n_hyp"], 2 * g0["n_hyp"])
    assert np.abs(g1["scale"] - 3.0).max() < 1e-12


def test_degenerate_inputs(vcp_ctx):
    tgt = np.array([[0.0, 0, 0], [1.0, 0, 0], [1.0, 0, 0], [0.0, 2, 0]])       # targets 1 and 2 coincide: Lv = 0
    src = np.array([[0.0, 0, 0], [1.0, 0, 0], [np.nan, 0, 0]])
    g = _check(vcp_ctx, src, tgt, [[1, 1], [0, 2], [0, 1]], 1.0, 1.0, 0.25)       # a = b'; a NaN coordinate; a good base
    assert g["score"].tolist() == [-1, -1, 2] and g["n_hyp"].tolist() == [0, 0, 4] and g["best"] == 2
    assert g["scale"].tolist() == [0.0, 0.0, 1.0]
    g = _check(vcp_ctx, src, tgt, [[1, 1], [0, 2], [0, 1]], 1e-300, 1e300, 0.25)
    assert g["n_hyp"].tolist() == [0, 0, 10]                                      # 12 ordered pairs less (1, 2) and (2, 1)
    # no hypothesis at all
    g = _check(vcp_ctx, src, tgt, [[1, 1], [0, 2], [2, 2]], 1e-300, 1e300, 0.25, mirror=True)
    assert g["best"] == -1 and np.array_equal(g["M"], np.eye(4)) and not g["M_all"].any()
    assert g["score"].tolist() == [-1] * 3 and g["pick"].tolist() == [[0, -1, -1]] * 3 and not g["inliers"].any()
    assert g["scale"].tolist() == [0.0] * 3
    g = _check(vcp_ctx, src, tgt, [[0, 1]], 5.0, 6.0, 0.25)                       # a good base, no pair in the range
    assert g["best"] == -1 and g["n_hyp"].tolist() == [0] and g["scale"].tolist() == [0.0]
    # a target with a non-finite coordinate makes no hypothesis and is nobody's inlier
    tgt2 = np.r_[tgt, [[np.inf, 0, 0], [3.0, np.nan, 0]]]
    _check(vcp_ctx, src, tgt2, [[0, 1]], 1e-300, 1e300, 0.25)
    # inlier_dist = +inf: one cell, every finite landmark counts
    g = _check(vcp_ctx, src, tgt, [[0, 1]], 2.0, 2.0, np.inf)
    assert g["score"].tolist() == [2] and g["inliers"].tolist() == [2] and g["n_hyp"].tolist() == [2]


@pytest.mark.parametrize("nt,n_bases", [(70, 4), (40, 16)])
def test_queue_overflow(vcp_ctx, nt, n_bases):
    """A range every ordered pair passes for every base, so row i queues (nt - 1) * n_bases hypotheses: 276 (scored in the
    middle of the row, once the queue holds more than 256) and 624 (more than the queue's 512 slots)."""
    rng = np.random.default_rng(12)
    tgt = np.c_[rng.uniform(0, 8, (nt, 2)), np.zeros(nt)]
    src = np.c_[rng.uniform(0, 8, (16, 2)), np.zeros(16)]
    src[:10] = (tgt[:10] - R.planted()[:3, 3]) @ R.planted()[:3, :3]
    bases = np.array([(a, b) for a in range(16) for b in range(16) if a != b])[rng.permutation(240)[:n_bases]]
    ref = S.register(src, tgt, bases, 1e-3, 1e3, 0.1)
    assert np.all(ref["n_hyp"] == nt * (nt - 1))                                  # every row holds every (j, base)
    assert int(ref["n_hyp"].sum()) // nt > (QUEUE if n_bases == 16 else QUEUE_SCORED_ABOVE)
    _check(vcp_ctx, src, tgt, bases, 1e-3, 1e3, 0.1, ref=ref)


def test_landmark_step(vcp_ctx):
    rng = np.random.default_rng(13)
    tgt = np.c_[rng.uniform(0, 12, (300, 2)), np.zeros(300)]
    src = np.r_[tgt[:250], np.c_[rng.uniform(0, 12, (200, 2)), np.zeros(200)]]
    src = np.ascontiguousarray((src[rng.permutation(450)] - R.planted()[:3, 3]) @ R.planted()[:3, :3]) / 2.5
    from vtkcloudpoint_amd.icp import choose_bases
    bases = choose_bases(src, 3, 3.0 / 2.5, 5.0 / 2.5, 2)
    assert len(R.landmark_indices(450, 200)) == 225
    a = _check(vcp_ctx, src, tgt, bases, 2.499, 2.501, 0.05, max_landmarks=200)          # step 2: 225 landmarks
    b = _check(vcp_ctx, src, tgt, bases, 2.499, 2.501, 0.05, max_landmarks=450)          # every point
    _check(vcp_ctx, src, tgt, bases, 2.499, 2.501, 0.05, max_landmarks=10 ** 6, ref=b)
    print("landmark step: score", a["score"], b["score"], "hypotheses", a["n_hyp"])
    assert np.all(a["score"] <= 225) and np.array_equal(b["score"], b["inliers"])
    assert a["score"].max() < b["score"].max() and np.array_equal(a["n_hyp"], b["n_hyp"])


def test_4096_bases(vcp_ctx):
    rng = np.random.default_rng(14)
    tgt = np.c_[rng.integers(0, 12, (30, 2)) * 0.5, np.zeros(30)]
    src = np.ascontiguousarray((tgt[rng.permutation(30)] - R.planted()[:3, 3]) @ R.planted()[:3, :3]) / 2.0
    src[:, 2] = 0.0
    bases = rng.integers(0, 30, (4096, 2))
    g = _check(vcp_ctx, src, tgt, bases, 2.0 - 1e-6, 2.0 + 1e-6, 0.01)
    assert (g["score"] == -1).sum() >= (bases[:, 0] == bases[:, 1]).sum() > 0 and (g["score"] >= 28).sum() > 3000
    assert g["n_hyp"].sum() > 4096


def test_grid_path(vcp_ctx):
    """4000 truths: the score goes through a grid of many cells.  With the range 2.5 (1 -+ 1e-5) the reference sees 60
    hypotheses (printed; the assertion allows up to 400)."""
    rng = np.random.default_rng(15)
    tgt = np.c_[rng.uniform(0, 60, (4000, 2)), np.zeros(4000)]
    seen = tgt[(tgt[:, 0] < 24) & (tgt[:, 1] < 24)]
    seen = seen[rng.permutation(len(seen))[:560]] + np.c_[rng.normal(0, 0.003, (560, 2)), np.zeros(560)]
    src = np.r_[seen, np.c_[rng.uniform(0, 24, (40, 2)), np.zeros(40)]]
    src = np.ascontiguousarray((src[rng.permutation(600)] - R.planted()[:3, 3]) @ R.planted()[:3, :3]) / 2.5
    from vtkcloudpoint_amd.icp import choose_bases
    bases = choose_bases(src, 2, 6.0 / 2.5, 9.0 / 2.5, 3)
    lo, hi = 2.5 * (1 - 1e-5), 2.5 * (1 + 1e-5)
    ref = S.register(src, tgt, bases, lo, hi, 0.05)
    print("grid path: hypotheses", ref["n_hyp"], "score", ref["score"], "inliers", ref["inliers"])
    assert 2 <= ref["n_hyp"].sum() <= 400
    g = _check(vcp_ctx, src, tgt, bases, lo, hi, 0.05, ref=ref)
    assert g["n_hyp"].sum() == ref["n_hyp"].sum()


@pytest.mark.parametrize("name", sorted(R.SCENES))
def test_scaled_scene_equals_the_golden_file(vcp_ctx, name):
    """The scenes of tests/test_register_sim.py: equal to the restatement's recorded result, directly and through
    register_similarity."""
    from vtkcloudpoint_amd.icp import register_similarity
    sc, bases = S.scaled_scene(name)
    ref = S.golden(name)
    g = _check(vcp_ctx, sc["source"], sc["truths"], bases, S.RANGE[0], S.RANGE[1], R.INLIER, ref=ref)
    assert g["inliers"][g["best"]] >= 0.95 * sc["planted"]
    S.same(register_similarity(sc["source"], sc["truths"], bases, S.RANGE, R.INLIER, ctx=vcp_ctx), ref)


@pytest.mark.parametrize("name", sorted(R.SCENES))
def test_global_sim_icp(vcp_ctx, name):
    """register_similarity, the gated polish and the scale refit on the scaled scenes.  The polish composes proper
    rotations onto the start, so without the refit the scale stays the registered k up to the rounding of max_iter 3 x 3
    products (a few 1e-16 each; 1e-12 allows for them); with it the scale may not be farther from the planted 2.5 than the
    registered one.  Measured on an MI355X: half 2.5009338 against 2.5033071 registered, third 2.4994041 against
    2.4990430."""
    from vtkcloudpoint_amd.icp import gate_schedule, global_sim_icp
    sc, bases = S.scaled_scene(name)
    ref, n = S.golden(name), sc["planted"]
    g0, g1, gr, rounds = R.POLISH
    gates = gate_schedule(g0, g1, gr)
    p = global_sim_icp(sc["source"], sc["truths"], bases, S.RANGE, R.INLIER, gates, max_iter=rounds, refine=False,
                       ctx=vcp_ctx)
    S.same(p["registration"], ref)
    assert p["bases_used"].tolist() == np.flatnonzero(ref["score"] >= 0).tolist()
    assert p["scale_registration"] == ref["scale"][p["bases_used"][p["best"]]]
    print(name, "planted", n, "registration", ref["inliers"], "polished", p["inliers"], "scale", p["scale"])
    assert p["inliers"][p["best"]] >= 0.95 * n
    assert abs(p["scale"] - p["scale_registration"]) <= 1e-12 * p["scale_registration"]
    q = global_sim_icp(sc["source"], sc["truths"], bases, S.RANGE, R.INLIER, gates, max_iter=rounds, ctx=vcp_ctx)
    print(name, "refined: inliers", q["inliers"], "scale", q["scale"], "registered", q["scale_registration"])
    assert q["scale_registration"] == p["scale_registration"]
    assert q["inliers"][q["best"]] >= 0.95 * n
    assert R.inliers_of(sc, q["M"][:3, :3], q["M"][:3, 3]) == q["inliers"][q["best"]]
    assert abs(q["scale"] - S.SCALE) <= abs(q["scale_registration"] - S.SCALE)


def _raw(ctx, src, ns, tgt, nt, bases, nb, lo, hi, ml, inlier, outs, M=True, best=True, have_bases=True):
    Mb, bst = outs["M"], outs["best"]
    return N.lib().vcp_register_sim(ctx._h, N._ptr(src), C.c_int64(ns), N._ptr(tgt), C.c_int64(nt),
                                    N._ptr(bases) if have_bases else None, C.c_int32(nb), C.c_double(lo), C.c_double(hi), 0,
                                    int(ml), C.c_double(inlier), N._ptr(Mb) if M else None, N._ptr(bst) if best else None,
                                    N._ptr(outs["M_all"]), N._ptr(outs["score"]), N._ptr(outs["inliers"]),
                                    N._ptr(outs["pick"]), N._ptr(outs["n_hyp"]), N._ptr(outs["scale"]))


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
                    n_hyp=np.full(nb, 77, np.int64), scale=np.full(nb, 7.0))

    def untouched(o):
        return all(np.all(v == (7.0 if v.dtype == np.float64 else 77)) for v in o.values())

    cases = [(-1, dict(nb=0)), (-1, dict(ml=0)), (-1, dict(lo=0.0)), (-1, dict(lo=-1.0)), (-1, dict(lo=np.nan)),
             (-1, dict(hi=np.nan)), (-1, dict(hi=np.inf)), (-1, dict(lo=np.inf, hi=np.inf)),
             (-1, dict(lo=2.0, hi=float(np.nextafter(2.0, 0.0)))),
             (-1, dict(inlier=0.0)), (-1, dict(inlier=-1.0)), (-1, dict(inlier=np.nan)), (-1, dict(M=False)),
             (-1, dict(best=False)), (-1, dict(have_bases=False)),
             (-2, dict(ns=1)), (-2, dict(nt=1)), (-2, dict(ns=0)),
             (-4, dict(bases=np.array([[0, 1], [2, 20]], np.int32))), (-4, dict(bases=np.array([[-1, 1], [2, 3]], np.int32))),
             (-8, dict(bases=big, nb=4097)), (-8, dict(tgt=far, nt=65537))]
    for code, kw in cases:
        a = dict(src=src, ns=20, tgt=tgt, nt=25, bases=bases, nb=2, lo=0.5, hi=2.0, ml=200, inlier=0.1)
        a.update(kw)
        o = outs(max(a["nb"], 2))
        rc = _raw(vcp_ctx, outs=o, **a)
        assert rc == code, (kw.keys(), rc)
        assert untouched(o), kw.keys()
    o = outs()                                   # and the same call without a fault runs; scale_min == scale_max is valid
    assert _raw(vcp_ctx, src, 20, tgt, 25, bases, 2, 1.0, 1.0, 200, 0.1, o) == 0 and o["best"][0] in (-1, 0, 1)
    assert _raw(vcp_ctx, src, 20, tgt, 25, bases, 2, 1e-300, 1e300, 200, np.inf, o) == 0
    assert o["n_hyp"].tolist() == [600, 600]
    # every per-base output may be left out
    Mb, bst = np.zeros(16), np.zeros(1, np.int32)
    rc = N.lib().vcp_register_sim(vcp_ctx._h, N._ptr(src), C.c_int64(20), N._ptr(tgt), C.c_int64(25), N._ptr(bases),
                                  C.c_int32(2), C.c_double(1e-300), C.c_double(1e300), 0, 200, C.c_double(np.inf),
                                  N._ptr(Mb), N._ptr(bst), None, None, None, None, None, None)
    assert rc == 0 and np.array_equal(Mb, o["M"]) and bst[0] == o["best"][0]
    with pytest.raises(N.VcpError) as e:
        vcp_ctx.register_sim(src, tgt, [[0, 20]], 0.5, 2.0, 0.1)
    assert e.value.code == -4


def test_dev_form_two_calls_phases_and_vcp_match(vcp_ctx):
    import torch
    sc, bases = S.scaled_scene("half")
    src, tgt = sc["source"], sc["truths"]
    lo, hi = S.RANGE
    a = vcp_ctx.register_sim(src, tgt, bases, lo, hi, R.INLIER, True)
    b = vcp_ctx.register_sim(src, tgt, bases, lo, hi, R.INLIER, True)
    S.same(a, b)                                                      # two calls: identical bits
    B, ns, nt = len(bases), len(src), len(tgt)
    d_s, d_t, d_b = torch.from_numpy(src).cuda(), torch.from_numpy(tgt).cuda(), torch.from_numpy(bases).cuda()
    o = dict(M_all=torch.zeros((B, 4, 4), dtype=torch.float64, device="cuda"),
             score=torch.zeros(B, dtype=torch.int32, device="cuda"), inliers=torch.zeros(B, dtype=torch.int32, device="cuda"),
             pick=torch.zeros((B, 3), dtype=torch.int32, device="cuda"), n_hyp=torch.zeros(B, dtype=torch.int64, device="cuda"),
             scale=torch.zeros(B, dtype=torch.float64, device="cuda"))
    torch.cuda.synchronize()
    r = vcp_ctx.register_sim_dev(d_s.data_ptr(), ns, d_t.data_ptr(), nt, d_b.data_ptr(), B, lo, hi, R.INLIER, True, 200,
                                 o["M_all"].data_ptr(), o["score"].data_ptr(), o["inliers"].data_ptr(),
                                 o["pick"].data_ptr(), o["n_hyp"].data_ptr(), o["scale"].data_ptr())
    got = {k: v.cpu().numpy() for k, v in o.items()}
    got.update(best=r["best"], M=r["M"])
    S.same(got, a)                                                    # the device-pointer form equals the host form
    r2 = vcp_ctx.register_sim_dev(d_s.data_ptr(), ns, d_t.data_ptr(), nt, d_b.data_ptr(), B, lo, hi, R.INLIER, True)
    assert r2["best"] == a["best"] and np.array_equal(r2["M"], a["M"])  # the per-base arrays left out
    # inliers[b] is vcp_match's count_matched under the base's matrix
    for k in np.flatnonzero(a["score"] >= 0):
        assert vcp_ctx.match(src, tgt, a["M_all"][k], R.INLIER)["count"] == a["inliers"][k], k
    vcp_ctx.timing_enable(True)
    try:
        vcp_ctx.register_sim(src, tgt, bases, lo, hi, R.INLIER)
        assert [p for p, _ in vcp_ctx.timing()] == ["regs_grid", "regs_search", "regs_final"]
        vcp_ctx.register_sim(src, tgt, [[0, 0]], lo, hi, R.INLIER)     # no hypothesis at all: the same phases
        assert [p for p, _ in vcp_ctx.timing()] == ["regs_grid", "regs_search", "regs_final"]
    finally:
        vcp_ctx.timing_enable(False)
    # the rigid call between two similarity calls shares the workspace and leaves it usable
    sc0, bases0, ref0 = R.scene_case("half")
    R.same(vcp_ctx.register_pairs(sc0["source"], sc0["truths"], bases0, R.LEN_TOL, R.INLIER), ref0)
    vcp_ctx.release_workspace()                                       # the workspace is the context's own
    S.same(vcp_ctx.register_sim(src, tgt, bases, lo, hi, R.INLIER, True), a)
