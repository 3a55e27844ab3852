"""vcp_register_sim without a GPU: the entry points in the header, the Python binding, the library, the C# imports and the
C++ mirror with matching arity; the host run of the pose arithmetic against the numpy restatement of the definition
(tests/register_sim_ref.py); hand-checked cases of that restatement; fit_scale and bbox_scale_range; the golden file; and
the behaviour claim on the two scaled partial-overlap scenes, held by the restatement alone -- the device is held to
equality with it in tests/test_register_sim_gpu.py."""
import inspect
import os
import re

import numpy as np
import pytest

import register_ref as R
import register_sim_ref as S
from test_abi import _csharp_imports, _declared, _header_prototypes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("vcp_register_sim", "vcp_register_sim_dev")
SELFTEST = "vcp_selftest_register_sim_pose"


def test_the_symbols_everywhere_with_matching_arity():
    from vtkcloudpoint_amd import _native, icp
    lib = _native.lib()
    decl, protos = _declared(), _header_prototypes()
    cs = {name: classes for _, name, classes in _csharp_imports()}
    for nm in NAMES:
        assert nm in decl and hasattr(lib, nm) and nm in _native.SYMBOLS, nm
        assert cs.get(nm) == protos[nm], (nm, cs.get(nm), protos[nm])
        assert len(protos[nm]) == 20
    assert protos["vcp_register_sim"] == ["ptr", "ptr", "i64", "ptr", "i64", "ptr", "i32", "f64", "f64", "i32", "i32",
                                          "f64"] + ["ptr"] * 8
    assert protos["vcp_register_sim_dev"] == protos["vcp_register_sim"]
    # the rigid call with one more double and one more array
    assert len(protos["vcp_register_pairs"]) == 18
    assert SELFTEST in decl and hasattr(lib, SELFTEST) and SELFTEST in _native.SYMBOLS
    assert protos[SELFTEST] == ["ptr"] * 4 + ["i32", "ptr", "ptr"]
    assert list(inspect.signature(_native.Context.register_sim).parameters)[:7] == \
        ["self", "source", "target", "bases", "scale_min", "scale_max", "inlier_dist"]
    assert callable(_native.Context.register_sim_dev)
    assert list(inspect.signature(icp.register_similarity).parameters) == \
        ["centers", "truths", "bases", "scale_range", "inlier_dist", "mirror", "max_landmarks", "ctx"]
    assert list(inspect.signature(icp.global_sim_icp).parameters) == \
        ["centers", "truths", "bases", "scale_range", "inlier_dist", "gates", "mirror", "max_iter", "max_landmarks",
         "min_pairs", "refine", "ctx"]
    for fn in (icp.bbox_scale_range, icp.fit_scale):
        assert callable(fn)
    host = os.path.join(ROOT, "vtkcloudpoint_amd", "host")
    with open(os.path.join(host, "csharp", "ICP.cs")) as f:
        assert re.search(r"public\s+int\s+RegisterSimilarity\s*\(", f.read())
    with open(os.path.join(host, "csharp", "MainForm.Gpu.cs")) as f:
        assert "VcpNative.vcp_register_sim(" in f.read()
    with open(os.path.join(host, "cpp", "vcp_host.hpp")) as f:
        src = f.read()
    m = re.search(r"vcp_register_sim\(([^;]*)\)\);", src, re.S)
    assert m and "int RegisterSimilarity(" in src
    depth, args = 0, 1                       # arguments of the mirror's call: commas outside brackets
    for ch in m.group(1):
        depth += ch in "(["
        depth -= ch in ")]"
        args += ch == "," and depth == 0
    assert args == 20


def _pose_cases():
    rng = np.random.default_rng(23)
    cases = []
    for _ in range(360):
        scale = float(rng.choice([1.0, 1e-3, 1e6, 37.0]))
        pts = rng.uniform(-5, 5, (4, 3)) * scale
        if rng.random() < 0.3:
            pts = np.round(pts * 4) / 4              # exact quarter turns, zero sines: signed zeros in M
        if rng.random() < 0.3:
            pts[2:] *= float(rng.choice([1e-3, 0.4, 3.0, 1e4]))     # the targets in another unit
        cases.append(pts)
    z = np.zeros(3)
    for p in (-3, -1, 1, 2, 10):                    # k an exact power of two: every product with k is exact
        k = 2.0 ** p
        cases += [np.array([[0.25, 0.5, 1.0], [3.25, 4.5, -1.0], [k * 1.0, k * 2.0, 0.5], [k * 5.0, k * 5.0, 0.25]]),
                  np.array([[0.0, 0, 0], [2.0, 0, 0], [1.0, 1, 0], [1.0, 1 + 2 * k, 0]])]       # a quarter turn, c = 0
    cases += [np.array([[0.0, 0, 0], [2.0, 0, 0], [1.0, 1, 0], [1.0, 3, 0]]),         # k = 1, c = 0 exactly
              np.array([[0.0, 0, 0], [2.0, 0, 0], [5.0, 1, 0], [7.0, 1, 0]]),         # k = 1, s = +0
              np.array([[0.0, 0, 0], [2.0, 0, 0], [7.0, 1, 0], [5.0, 1, 0]]),         # k = 1, c = -1, s = -0 or +0
              np.array([[0.0, 0, 0], [2.0, 0, 0], [11.0, 1, 0], [5.0, 1, 0]]),        # k = 3, c = -1
              np.array([[0.0, 0, 7.0], [3.0, 4.0, 1.0], [0.0, 0, 0], [5.0, 0, 2.5]]),  # k = 1 with z offsets
              np.array([z, z, [1.0, 0, 0], [2.0, 0, 0]]),                            # Lu = 0: k = inf, skipped
              np.array([[0.0, 0, 0], [1.0, 0, 0], [3.0, 3, 0], [3.0, 3, 0]]),         # Lv = 0: k = 0, skipped
              np.array([z, z, [3.0, 3, 0], [3.0, 3, 0]]),                            # 0 / 0
              np.array([[0.0, 0, 0], [1e-200, 0, 0], [0.0, 0, 0], [1e-200, 0, 0]]),   # nrm underflows: skipped
              np.array([[0.0, 0, 0], [1e200, 0, 0], [0.0, 0, 0], [1e200, 0, 0]]),     # nrm overflows: skipped
              np.array([[0.0, 0, 0], [1e-160, 0, 0], [0.0, 0, 0], [1e160, 0, 0]]),    # k overflows, nrm = 1
              np.array([[np.nan, 0, 0], [1.0, 0, 0], [0.0, 0, 0], [1.0, 0, 0]]),
              np.array([[0.0, 0, 0], [1.0, 0, 0], [0.0, np.inf, 0], [1.0, 0, 0]]),
              np.array([[0.0, 0, np.inf], [1.0, 0, 0], [0.0, 0, 0], [1.0, 0, 2.5]])]   # z only moves T.z
    return cases


def test_the_librarys_pose_arithmetic_equals_the_restatement_bit_for_bit():
    """vcp_selftest_register_sim_pose runs, on the host, the source the kernels execute: Lu, Lv, k and every bit of M must
    be the restatement's on about 800 hypotheses (flips, signed zeros, non-finite input, skipped ones, k a power of two),
    and where k is exactly 1 M must also be vcp_selftest_register_pose's."""
    from vtkcloudpoint_amd._native import selftest_register_pose, selftest_register_sim_pose
    cases = _pose_cases()
    assert 2 * len(cases) >= 760
    skipped = ones = pow2 = 0
    for pts in cases:
        src, tgt = np.ascontiguousarray(pts[:2]), np.ascontiguousarray(pts[2:])
        for f in (0, 1):
            Lu, Lv, k, M = selftest_register_sim_pose(src[0], src[1], tgt[0], tgt[1], f)
            _, rLu = S.candidates(src, tgt, np.array([[0, 1]]), 1.0, 1.0)
            rM, ok, rk = S.poses(src, tgt, 0, 1, f, [0], [1])
            with np.errstate(all="ignore"):
                v = tgt[1] - tgt[0]
                rLv = np.sqrt(v[0] * v[0] + v[1] * v[1])
                assert np.array([rLv / rLu[0]]).tobytes() == np.array([rk[0]]).tobytes()
            assert np.array([Lu, Lv, k]).tobytes() == np.array([rLu[0], rLv, rk[0]]).tobytes(), (pts, f, Lu, Lv, k)
            assert (M is not None) == bool(ok[0])
            if M is None:
                skipped += 1
                continue
            assert np.ascontiguousarray(M).tobytes() == np.ascontiguousarray(rM[0]).tobytes(), (pts, f, M, rM[0])
            if k == 1.0:
                ones += 1
                _, _, M1 = selftest_register_pose(src[0], src[1], tgt[0], tgt[1], f)
                assert M1 is not None and np.ascontiguousarray(M).tobytes() == np.ascontiguousarray(M1).tobytes()
            elif np.isfinite(k) and k > 0 and np.frexp(k)[0] == 0.5:
                pow2 += 1
                _, _, M1 = selftest_register_pose(src[0], src[1], tgt[0], tgt[1], f)       # the rotation is the rigid one's
                assert np.array_equal(M[:2, :2], k * M1[:2, :2]) and M[2, 2] == k
    assert skipped >= 12 and ones >= 8 and pow2 >= 10, (skipped, ones, pow2)


def test_two_and_two_at_twice_the_size():
    # one base of length 2, two targets 4 apart: k = 2 exactly; both orders put both points on a target; (0, 0, 1) wins
    src, tgt = [[0.0, 0, 0], [2.0, 0, 0]], [[1.0, 1, 0], [1.0, 5, 0]]
    r = S.register(src, tgt, [[0, 1]], 2.0, 2.0, 0.125)
    assert r["score"].tolist() == [2] and r["pick"].tolist() == [[0, 0, 1]] and r["n_hyp"].tolist() == [2]
    assert r["inliers"].tolist() == [2] and r["best"] == 0 and r["scale"].tolist() == [2.0]
    # u = (2, 0) on v = (0, 4): a quarter turn times 2; the midpoint (1, 0) goes to (1, 3)
    assert r["M"].tolist() == [[0.0, -2.0, 0.0, 1.0], [2.0, 0.0, 0.0, 1.0], [0.0, 0.0, 2.0, 0.0], [0.0, 0.0, 0.0, 1.0]]
    for lo, hi, n in ((1.0, np.nextafter(2.0, 0.0), 0), (np.nextafter(2.0, 3.0), 3.0, 0), (0.5, 2.0, 2), (2.0, 1e300, 2)):
        r = S.register(src, tgt, [[0, 1]], lo, hi, 0.125)
        assert r["n_hyp"].tolist() == [n] and r["best"] == (0 if n else -1) and r["scale"].tolist() == [2.0 if n else 0.0]
    # the brute-force existence test and the windowed one agree
    S.same(S.register(src, tgt, [[0, 1]], 0.5, 2.0, 0.125, True), S.register(src, tgt, [[0, 1]], 0.5, 2.0, 0.125, True,
                                                                             brute=True))


def test_scale_one_is_the_rigid_restatement_on_the_lattice():
    xy = np.array([[x, y, 0.0] for y in range(4) for x in range(4)])
    bases = [[0, 1], [0, 5], [0, 3], [5, 10], [15, 0], [1, 7], [6, 6]]
    for mirror in (False, True):
        s, r = S.register(xy, xy, bases, 1.0, 1.0, 0.5, mirror), R.register(xy, xy, bases, 0.0, 0.5, mirror)
        R.same(s, r)
        assert s["scale"].tolist() == [1.0] * 6 + [0.0]
    # at twice the size the unit base fits the pairs two apart: 2 * (2 * 4 * 2) of them
    s = S.register(xy, xy, bases, 2.0, 2.0, 0.5)
    assert s["n_hyp"][0] == 32 and s["scale"][0] == 2.0 and s["score"][6] == -1
    # the windowed count against the brute-force one on many hypotheses
    S.same(S.register(xy, xy, bases, 0.5, 2.0, 0.5, True), S.register(xy, xy, bases, 0.5, 2.0, 0.5, True, brute=True))


def test_the_planted_similarity_is_found_and_a_flip_needs_the_mirror():
    rng = np.random.default_rng(8)
    tgt = np.c_[rng.uniform(0, 10, (40, 2)), np.zeros(40)]
    P = R.planted()
    src = np.ascontiguousarray((tgt[:25] - P[:3, 3]) @ P[:3, :3]) / 3.0
    src[:, 2] = 0.0
    r = S.register(src, tgt, [[3, 17], [5, 6]], 2.9, 3.1, 1e-6)
    assert r["score"].tolist() == [25, 25] and r["inliers"].tolist() == [25, 25] and r["best"] == 0
    assert r["pick"].tolist() == [[0, 3, 17], [0, 5, 6]] and np.abs(r["scale"] - 3.0).max() < 1e-12
    P3 = P.copy()
    P3[:3, :3] *= 3.0
    assert np.abs(r["M"] - P3).max() < 1e-11
    r = S.register(src, tgt, [[3, 17]], 2.9, 3.1, 1e-6, max_landmarks=10)           # step 2: 12 landmarks
    assert r["score"].tolist() == [12] and r["inliers"].tolist() == [25]
    flipped = src * np.array([1.0, -1.0, 1.0])
    r0 = S.register(flipped, tgt, [[3, 17]], 2.9, 3.1, 1e-6, mirror=False)
    r1 = S.register(flipped, tgt, [[3, 17]], 2.9, 3.1, 1e-6, mirror=True)
    assert r1["pick"].tolist() == [[1, 3, 17]] and r1["score"].tolist() == [25] and r0["score"][0] < 25
    assert r1["n_hyp"][0] == 2 * r0["n_hyp"][0]
    # the mirrored winner is the planted k = 3 with det -k^2; the unmirrored one is some proper similarity of the range
    assert abs(np.linalg.det(r1["M"][:2, :2]) + 9.0) < 1e-10 and 2.9 ** 2 <= np.linalg.det(r0["M"][:2, :2]) <= 3.1 ** 2


def test_degenerate_bases_and_argument_errors():
    tgt = np.array([[0.0, 0, 0], [1.0, 0, 0], [1.0, 0, 0], [0.0, 2, 0]])
    src = np.array([[0.0, 0, 0], [1.0, 0, 0], [np.nan, 0, 0]])
    r = S.register(src, tgt, [[1, 1], [0, 2], [0, 1]], 1.0, 1.0, 0.25)
    assert r["score"].tolist() == [-1, -1, 2] and r["n_hyp"].tolist() == [0, 0, 4] and r["best"] == 2
    assert r["pick"][:2].tolist() == [[0, -1, -1]] * 2 and not r["M_all"][:2].any() and r["scale"].tolist() == [0, 0, 1.0]
    r = S.register(src, tgt, [[1, 1], [0, 2], [0, 1]], 1e-300, 1e300, 0.25)
    assert r["n_hyp"].tolist() == [0, 0, 10]                                      # 12 ordered pairs less (1, 2) and (2, 1)
    r = S.register(src, tgt, [[1, 1], [0, 2]], 1e-300, 1e300, 0.25, True)
    assert r["best"] == -1 and np.array_equal(r["M"], np.eye(4)) and r["inliers"].tolist() == [0, 0]
    assert r["scale"].tolist() == [0.0, 0.0]
    for code, kw in ((S.ERR_ARG, dict(scale_min=0.0)), (S.ERR_ARG, dict(scale_min=-1.0)), (S.ERR_ARG, dict(scale_min=np.nan)),
                     (S.ERR_ARG, dict(scale_max=np.nan)), (S.ERR_ARG, dict(scale_max=np.inf)),
                     (S.ERR_ARG, dict(scale_min=2.0, scale_max=np.nextafter(2.0, 0.0))), (S.ERR_ARG, dict(inlier_dist=0.0)),
                     (S.ERR_ARG, dict(max_landmarks=0)), (S.ERR_ARG, dict(bases=np.zeros((0, 2)))),
                     (S.ERR_EMPTY, dict(source=src[:1])), (S.ERR_EMPTY, dict(target=tgt[:1])),
                     (S.ERR_INDEX, dict(bases=[[0, 3]])), (S.ERR_INDEX, dict(bases=[[-1, 0]])),
                     (S.ERR_UNSUPPORTED, dict(bases=np.zeros((4097, 2))))):
        a = dict(source=src, target=tgt, bases=[[0, 1]], scale_min=0.5, scale_max=2.0, inlier_dist=0.25, max_landmarks=200)
        a.update(kw)
        with pytest.raises(S.RefError) as e:
            S.register(**a)
        assert e.value.code == code, kw
    assert S.register(src, tgt, [[0, 1]], 2.0, 2.0, np.inf)["n_hyp"].tolist() == [2]       # scale_min == scale_max is valid


def test_fit_scale_and_bbox_scale_range():
    from vtkcloudpoint_amd.icp import bbox_scale_range, fit_scale
    rng = np.random.default_rng(31)
    p = rng.uniform(-4, 9, (50, 3))
    for k, ang in ((2.5, 0.7), (0.125, 3.0), (1.0, 0.0)):
        y = k * p @ R.rz(ang).T + np.array([3.0, -2.0, 0.5])
        assert abs(fit_scale(p, y) - k) <= 1e-13 * k                 # an exact similarity: k up to rounding
        assert abs(fit_scale(p * np.array([1.0, -1.0, 1.0]), y) - k) <= 1e-13 * k      # and it ignores a reflection
    with pytest.raises(ValueError):
        fit_scale(p[:1], p[:1])
    src = np.array([[0.0, 0, 0], [2.0, 1, 0], [1.0, 4, 0]])
    tgt = np.array([[1.0, 1, 0], [7.0, 9, 0], [3.0, 3, 0]])          # extents 6 and 8 over 2 and 4: sx = 3, sy = 2
    assert bbox_scale_range(src, tgt, 1.0) == (2.0, 3.0) and bbox_scale_range(src, tgt, 2.0) == (1.0, 6.0)
    with pytest.raises(ValueError):
        bbox_scale_range(src, tgt, 0.5)


@pytest.mark.parametrize("name", sorted(R.SCENES))
def test_the_restatement_reproduces_the_golden_file(name):
    S.same(S.scene_case(name)[2], S.golden(name))


@pytest.mark.parametrize("name", sorted(R.SCENES))
def test_reference_behaviour_on_a_scaled_partial_overlap(name):
    """A scan in another unit (2.5 truth units to one of its own) that sees a window of the truth field: the similarity
    search finds the planted pose, while the reference's way (the bounding-box factors sx, sy, then a rigid registration)
    and the rigid registration of the unscaled scan both stay below half of its inliers.  Measured: 98 of 98 and 49 of 49
    against 11 and 9 (sx 4.29, sy 4.11; 6.65, 6.99) and 13 and 13."""
    sc, bases, r = S.scene_case(name)
    src, tgt, n = sc["source"], sc["truths"], sc["planted"]
    print(name, "source", len(src), "planted", n, "hypotheses", int(r["n_hyp"].sum()), "inliers", r["inliers"], "scale",
          r["scale"])
    assert n >= 40 and r["best"] >= 0
    assert r["inliers"][r["best"]] >= 0.95 * n
    ext = lambda a, c: a[:, c].max() - a[:, c].min()                  # noqa: E731
    sx, sy = ext(tgt, 0) / ext(src, 0), ext(tgt, 1) / ext(src, 1)
    boxed = R.register(src * np.array([sx, sy, 1.0]), tgt, bases, R.LEN_TOL, R.INLIER)
    plain = R.register(src, tgt, bases, R.LEN_TOL, R.INLIER)
    got = [int(q["inliers"][q["best"]]) if q["best"] >= 0 else 0 for q in (boxed, plain)]
    print(name, "bounding-box scale", sx, sy, "inliers", got[0], "unscaled rigid", got[1])
    assert got[0] < 0.5 * n
    assert got[1] < 0.5 * n
