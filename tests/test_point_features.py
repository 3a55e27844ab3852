"""Per-point features without a GPU: hand-derived cases of the restatement (tests/point_features_ref.py) on the 2^-10
lattice, the restatement against exact rational arithmetic and numpy.linalg.eigh under bounds derived beforehand, the scene
of three seeds under the conditions fixed beforehand, and the header include/vcp_features.h against the library, the
Python binding, vcp.h and vcp_planes.h."""
import ast
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import centroid_ref as CR
import cluster_moments_ref as MR
import point_features_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "vcp_features.h")
S = 2.0 ** -10
NAN_BITS = 0x7FF8000000000000


def _all_nan(f, i):
    return all((R.bits(f[key][i]) == NAN_BITS).all() for key in ("normal", "eval", "variation", "mean_dist"))


# ---- hand-derived cases -----------------------------------------------------------------------------------------------------
def _plane_case():
    rng = np.random.default_rng(1)
    pts = np.column_stack([rng.integers(-2000, 2000, (40, 2)) * S, np.full(40, 0.5)])
    nbr = rng.integers(0, 40, (40, 8)).astype(np.int32)
    nbr[:, 0] = np.arange(40)
    return pts, nbr


def test_rows_on_a_plane_and_the_viewpoint_rule():
    """z = 0.5 exactly: the z sums are exact, d_z = 0, so cov_xz = cov_yz = cov_zz = +0 and the solve never touches the
    third axis: normal (0, 0, 1) by the sign rule, eval[2] = +0, variation +0."""
    pts, nbr = _plane_case()
    f = R.features(pts, nbr)
    assert np.array_equal(f["normal"], np.tile([0.0, 0.0, 1.0], (40, 1))) and not np.signbit(f["normal"]).any()
    assert (R.bits(f["eval"][:, 2]) == 0).all() and (R.bits(f["variation"]) == 0).all() and (f["eval"][:, 1] > 0).all()
    assert f["valid"].all() and (f["count"] == 8).all()
    up, down = R.features(pts, nbr, (0.25, -3.0, 5.0)), R.features(pts, nbr, (0.25, -3.0, -5.0))
    assert R.same(up["normal"], f["normal"])                                        # s = 4.5 > 0: as it is
    assert np.array_equal(down["normal"][:, 2], np.full(40, -1.0)) and np.signbit(down["normal"]).all()   # exact negation
    inplane = R.features(pts, nbr, (7.0, 9.0, 0.5))                                 # v_z = 0: s == 0, no flip
    assert R.same(inplane["normal"], f["normal"])
    for g in (up, down, inplane):                                                   # nothing else depends on the viewpoint
        assert R.differs(g, f, [k for k in R.KEYS if k != "normal"]) is None


def test_collinear_rows():
    x = np.array([-3, -1, 0, 2, 5, 9]) * S
    nbr = np.tile(np.arange(6, dtype=np.int32), (6, 1))
    f3 = R.features(np.column_stack([x, np.full(6, 0.25), np.full(6, -0.75)]), nbr)
    assert np.array_equal(f3["normal"], np.tile([0.0, 0.0, 1.0], (6, 1))) and f3["valid"].all()
    assert (f3["eval"][:, 0] > 0).all() and (R.bits(f3["eval"][:, 1:]) == 0).all() and (R.bits(f3["variation"]) == 0).all()
    f2 = R.features(np.column_stack([x, np.full(6, 0.25)]), nbr)
    assert np.array_equal(f2["normal"], np.tile([0.0, 1.0], (6, 1))) and (R.bits(f2["eval"][:, 1]) == 0).all() and f2["valid"].all()


@pytest.mark.parametrize("D", [2, 3])
def test_copies_of_one_point(D):
    """k rows with the same coordinates, each listing all of them: cov +0, evec the identity (normal = the last unit
    vector), mean_dist 0 over the k - 1 others; valid by m >= D."""
    for k in (1, 2, 3, 5):
        pts = np.tile(np.array([1.25, -0.5, 3.0])[:D], (k, 1))
        f = R.features(pts, np.tile(np.arange(k, dtype=np.int32), (k, 1)), np.zeros(D))
        want_n = np.eye(D)[D - 1]
        assert (R.bits(f["eval"]) == 0).all() and (R.bits(f["variation"]) == 0).all() and (R.bits(f["cov"]) == 0).all()
        assert np.array_equal(np.abs(f["normal"]), np.tile(want_n, (k, 1))) and (f["count"] == k).all()
        assert f["valid"].tolist() == [1 if k >= D else 0] * k
        if k > 1:
            assert (R.bits(f["mean_dist"]) == 0).all()
        else:
            assert R.bits(f["mean_dist"])[0] == NAN_BITS                            # the row is its whole list: q = 0


def test_membership_by_hand():
    """Rows 0 .. 7 of one cloud: absent from its own list; only its own list; m = 0; m = 1 (another row); m = dim - 1; a NaN
    neighbour; the same list as row 0 with -1 / out-of-range slots in front, in the middle and at the end; a NaN row."""
    pts = np.array([[0, 0, 0], [3, 0, 0], [0, 4, 0], [0, 0, 12], [1, 1, 1], [2, 2, 2], [0, 0, 0], [np.nan, 1, 1]], np.float64) * S
    n = len(pts)
    nbr = np.array([[1, 2, 3, 4, 5, 1, 2, 3],
                    [1, -1, -1, -1, -1, -1, -1, -1],
                    [-1, n, -5, 2 ** 31 - 1, -2 ** 31, n + 1, -1, -1],
                    [-1, 0, -1, -1, -1, -1, -1, -1],
                    [0, 1, -1, -1, -1, -1, -1, -1],
                    [0, 1, 2, 7, 3, 4, 5, 5],
                    [n, 1, 2, -1, 3, 4, 5, -1],
                    [0, 1, 2, 3, 4, 5, 6, 0]], np.int32)
    f = R.features(pts, nbr, (0.0, 0.0, 1.0))
    assert f["count"].tolist() == [8, 1, 0, 1, 2, 8, 5, 8] and f["valid"].tolist() == [1, 0, 0, 0, 0, 0, 1, 1]
    # row 0 is not in its list: every member counts in mean_dist.  distances 3, 4, 12, sqrt(3), sqrt(12), 3, 4, 12 (in S)
    d = [3.0, 4.0, 12.0, np.sqrt(3.0), np.sqrt(12.0), 3.0, 4.0, 12.0]
    acc = 0.0
    for v in d:
        acc = acc + v * S
    assert f["mean_dist"][0] == acc / 8.0
    # row 1, only its own list: cov +0, evec the identity, q = 0
    assert R.bits(f["mean_dist"])[1] == NAN_BITS and f["normal"][1].tolist() == [0.0, 0.0, 1.0] and (R.bits(f["eval"][1]) == 0).all()
    assert _all_nan(f, 2)                                                          # m = 0
    assert f["mean_dist"][3] == 12 * S and f["normal"][3].tolist() == [0.0, 0.0, 1.0] and f["valid"][3] == 0   # m = 1
    assert f["mean_dist"][4] == (np.sqrt(3.0) * S + np.sqrt(6.0) * S) / 2.0 and np.isfinite(f["normal"][4]).all()   # m = dim - 1
    assert _all_nan(f, 5)                                                          # a NaN neighbour
    # row 7 is NaN itself, its members are not: only what reads p_i is NaN (s is NaN: the normal stays as it is)
    assert R.bits(f["mean_dist"])[7] == NAN_BITS and np.isfinite(f["normal"][7]).all() and np.isfinite(f["eval"][7]).all()
    assert R.same(f["normal"][7], R.features(pts, nbr)["normal"][7])
    # row 6 has row 0's coordinates and row 0's members 1 2 3 4 5 with skipped slots around them
    g = R.features(pts, np.array([[1, 2, 3, 4, 5]] * n, np.int32), (0.0, 0.0, 1.0))
    assert R.differs({k: f[k][6:7] for k in R.KEYS}, {k: g[k][0:1] for k in R.KEYS}) is None


def test_mean_dist_on_a_3_4_5_triangle():
    pts = np.array([[0, 0], [3, 0], [0, 4]], np.float64) * S
    f = R.features(pts, np.array([[0, 1, 2], [1, 0, 2], [2, 1, 0]], np.int32))
    assert f["mean_dist"].tolist() == [3.5 * S, 4.0 * S, 4.5 * S] and f["valid"].all()
    assert R.same(f["mean"], np.tile([S, 4 * S / 3.0], (3, 1)))


def test_sor_keep_and_centre_votes_by_hand():
    v = np.array([4.0, 1.0, np.nan, 2.0, 100.0, 3.0, np.inf, 2.5])            # finite: 1 2 2.5 3 4 100: lower median 2.5
    keep, med, mad = R.sor_keep(v, 2.0)                                        # |v - med|: .5 .5 0 1.5 1.5 97.5 -> lower median 0.5
    assert (med, mad) == (2.5, 0.5) and keep.tolist() == [False, True, False, True, False, True, False, True]
    assert R.sor_keep(v, 2.0, floor=1.5)[0].tolist() == [True, True, False, True, False, True, False, True]
    k0, m0, d0 = R.sor_keep(np.array([np.nan, np.inf]))
    assert not k0.any() and np.isnan(m0) and np.isnan(d0)
    from vtkcloudpoint_amd import features as FT
    pts, nrm = np.array([[1.0, 2.0, 3.0], [0.5, 0.25, 0.125]]), np.array([[0.0, 0.6, 0.8], [1.0, 0.0, 0.0]])
    want = R.centre_votes(pts, nrm, 0.0725, [1, 0])
    assert want[0].tolist() == [1.0, 2.0 - 0.0725 * 0.6, 3.0 - 0.0725 * 0.8] and (R.bits(want[1]) == NAN_BITS).all()
    assert R.same(R.canon(FT.centre_votes(pts, nrm, 0.0725, np.array([1, 0], np.uint8))), want)


# ---- the restatement against independent arithmetic --------------------------------------------------------------------------
N_HOODS, K_HOOD = 2000, 16
_hoods = {}


def _neighbourhoods(D):
    """2000 neighbourhoods of 16 members: half of them from a cloud around the origin, half from one around 1e6 (where a
    raw-moment covariance would have lost nine digits).  Returns (G [2000 * 16, D] the gathered members, labels, the
    restatement's cov and normal, the exact covariance, the bound of cluster_moments_ref.cov_bound)."""
    if D not in _hoods:
        rng = np.random.default_rng([5, D])
        G, cov, nrm = [], [], []
        for offset in (0.0, 1e6):
            pts = R.generic_rows(4000, D, 6, offset=offset)
            nbr = rng.integers(0, 4000, (N_HOODS // 2, K_HOOD)).astype(np.int32)
            # the first 1000 rows carry the lists; the other rows have none
            f = R.features(pts, np.vstack([nbr, np.full((4000 - len(nbr), K_HOOD), -1, np.int32)]))
            G.append(pts[nbr].reshape(-1, D))
            cov.append(f["cov"][:len(nbr)])
            nrm.append(f["normal"][:len(nbr)])
        G = np.concatenate(G)
        labels = np.repeat(np.arange(1, N_HOODS + 1, dtype=np.int32), K_HOOD)
        ex = MR.exact_cov(G, labels, N_HOODS)
        _hoods[D] = (G, labels, np.concatenate(cov), np.concatenate(nrm), ex, MR.cov_bound(G, labels, N_HOODS, ex=ex))
    return _hoods[D]


@pytest.mark.parametrize("D", [2, 3])
def test_covariance_within_the_derived_bound_of_the_exact_one(D):
    """cluster_moments_ref.cov_bound is derived for sums through a tree of depth tree_depth(m); a sequential sum of m
    terms passes each term through at most m - 1 additions, and 15 <= tree_depth(16), so the bound covers these sums."""
    assert K_HOOD - 1 <= CR.tree_depth(K_HOOD)
    _, _, cov, _, ex, bnd = _neighbourhoods(D)
    pairs = [(a, b) for a in range(D) for b in range(a, D)]
    worst = Fraction(0)
    for h in range(N_HOODS):
        W, _, Cx = ex[h]
        assert W == K_HOOD
        for j, ab in enumerate(pairs):
            err = abs(Fraction(float(cov[h, j])) - Cx[ab])
            assert err <= bnd[h][ab], (D, h, ab, float(err), float(bnd[h][ab]))
            worst = max(worst, err / bnd[h][ab])
    print("\ndim %d: worst covariance error / bound %.3g" % (D, float(worst)))


def angle_cap(bnd_row, D, gap):
    """The perturbation bound of a symmetric eigenvector: a perturbation E of the matrix turns the eigenvector of an
    eigenvalue that is `gap` away from the others by at most an angle theta with sin(theta) <= |E|_2 / gap (Davis and
    Kahan), here with |E|_2 <= |E|_F <= the Frobenius norm of the entrywise covariance bound."""
    e2 = sum(float(b) ** 2 * (1 if a == c else 2) for (a, c), b in bnd_row.items())
    return float(np.arcsin(min(1.0, np.sqrt(e2) / gap)))


@pytest.mark.parametrize("D", [2, 3])
def test_normal_against_eigh_on_the_exact_covariance(D):
    """Wherever the two smallest eigenvalues differ by more than 1e-6 of the largest, the angle between the restatement's
    normal and numpy.linalg.eigh's on the exact covariance (rounded to binary64 entry by entry) stays below angle_cap:
    the covariance bound over the gap.  The worst ratio is printed; DESIGN.md section 37 records it."""
    _, _, _, nrm, ex, bnd = _neighbourhoods(D)
    worst, used = 0.0, 0
    for h in range(N_HOODS):
        C = np.zeros((D, D))
        for (a, b), v in ex[h][2].items():
            C[a, b] = C[b, a] = float(v)
        lw, lv = np.linalg.eigh(C)                                                   # ascending
        gap = lw[1] - lw[0]
        if not gap > 1e-6 * lw[-1]:
            continue
        used += 1
        ang = float(np.arcsin(min(1.0, np.linalg.norm(np.cross(np.r_[nrm[h], [0.0] * (3 - D)], np.r_[lv[:, 0], [0.0] * (3 - D)])))))
        cap = angle_cap(bnd[h], D, gap)
        assert ang <= cap, (D, h, ang, cap)
        worst = max(worst, ang / cap)
    print("\ndim %d: %d of %d neighbourhoods with a gap; worst angle / cap %.3g" % (D, used, N_HOODS, worst))
    assert used > N_HOODS // 2


# ---- the scene -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", R.SCENE_SEEDS)
def test_scene_conditions_on_the_restatement(seed):
    """The conditions fixed beforehand, on the restatement alone (tests/test_point_features_gpu.py holds the device to the
    restatement's bits on rows of the same scene)."""
    pts, kind, centres, knn, f = R.scene_features(seed)
    assert len(pts) == 23300 and (kind == 0).sum() == 300 and (kind == -1).sum() == 20000
    keep, med, mad = R.sor_keep(f["mean_dist"], 6.0)
    stray = kind == 0
    vs, vf = np.median(f["variation"][kind > 0]), np.median(f["variation"][kind == -1])
    votes = R.centre_votes(pts, f["normal"], R.R_SPHERE, f["valid"])
    within = []
    for j in range(R.N_SPHERES):
        sel = (kind == j + 1) & (f["valid"] != 0)
        within.append(float((np.linalg.norm(votes[sel] - centres[j], axis=1) <= R.R_SPHERE / 4).mean()))
    print("\nseed %d: strays dropped %d of 300, others dropped %d of 23000, variation sphere %.5f floor %.5f (x %.2f), "
          "votes within R / 4 %s" % (seed, (~keep[stray]).sum(), (~keep[~stray]).sum(), vs, vf, vs / vf,
                                     ["%.3f" % w for w in within]))
    assert (~keep[stray]).sum() >= 280 and (~keep[~stray]).sum() <= 230
    assert vs >= 3.0 * vf
    assert min(within) >= 0.9


# ---- the header against the library, the binding, vcp.h and vcp_planes.h ---------------------------------------------------------
def _strip(src):
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    src = re.sub(r"//[^\n]*", "", src)
    return re.sub(r"^\s*#[^\n]*", "", src, flags=re.M)


def _prototypes(path):
    """{name: parameter count} of the vcp_ functions a header declares (the parser of tests/test_abi.py)."""
    with open(path) as f:
        src = _strip(f.read())
    protos = {}
    for stmt in src.replace("{", ";").replace("}", ";").split(";"):
        m = re.search(r"\b(vcp_[a-z0-9_]+)\s*\(([^()]*)\)\s*$", stmt, re.S)
        if m:
            params = " ".join(m.group(2).split())
            assert m.group(1) not in protos, m.group(1)
            protos[m.group(1)] = 0 if params in ("", "void") else len(params.split(","))
    return protos


def test_every_declared_function_is_exported_listed_and_called_with_its_arity():
    from vtkcloudpoint_amd import _native, features
    protos = _prototypes(HEADER)
    assert protos == {"vcp_point_features_shape": 2, "vcp_point_features": 14, "vcp_point_features_dev": 14}
    lib = _native.lib()
    assert [s for s in protos if not hasattr(lib, s)] == []
    assert sorted(features.SYMBOLS) == sorted(protos)
    assert {k: len(v) for k, v in features._PROTOTYPES.items()} == protos         # the ctypes prototypes
    with open(os.path.join(ROOT, "vtkcloudpoint_amd", "features.py")) as f:
        tree = ast.parse(f.read())
    calls = {}
    for node in ast.walk(tree):
        if not (isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute)):
            continue
        base = node.func.value
        if not (isinstance(base, ast.Call) and isinstance(base.func, ast.Name) and base.func.id == "_L"):
            continue
        name = node.func.attr
        assert name in protos, "%s (line %d) is not in vcp_features.h" % (name, node.lineno)
        assert not node.keywords and not any(isinstance(a, ast.Starred) for a in node.args), name
        assert len(node.args) == protos[name], "%s (line %d): %d arguments, the header has %d" % (
            name, node.lineno, len(node.args), protos[name])
        calls[name] = calls.get(name, 0) + 1
    assert sorted(calls) == sorted(protos)                                        # every function has a call site


def test_no_name_is_shared_with_vcp_h_or_vcp_planes_h():
    from vtkcloudpoint_amd import _native, features, planes
    new = _prototypes(HEADER)
    for other, symbols in (("vcp.h", _native.SYMBOLS), ("vcp_planes.h", planes.SYMBOLS)):
        old = _prototypes(os.path.join(ROOT, "include", other))
        assert len(old) >= 7 and not set(old) & set(new), other
        assert not set(features.SYMBOLS) & set(symbols)
    with open(HEADER) as f:
        assert '#include "vcp.h"' in f.read()


def test_the_package_exports_the_features_functions():
    import vtkcloudpoint_amd as V
    from vtkcloudpoint_amd import features
    for name in ("point_features", "sor_keep", "centre_votes", "point_features_shape", "PointFeatures"):
        assert getattr(V, name) is getattr(features, name)
    assert features.PointFeatures._fields == ("normal", "eval", "variation", "mean_dist", "count", "valid", "knn")
