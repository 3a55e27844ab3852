"""Plane extraction without a GPU: the sampler's fixed vectors, hand-derived cases of the restatement
(tests/plane_ref.py), the header include/vcp_planes.h against the library, the Python binding and vcp.h, and the recovery of
three known planes from five synthetic scenes by the restatement, under caps fixed in advance."""
import ast
import os
import re

import numpy as np
import pytest

import plane_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "vcp_planes.h")


# ---- the sampler ----------------------------------------------------------------------------------------------------------
def test_hash_vectors():
    assert R.mix(0, 0) == 0xE220A8397B1DCDAF and R.mix(0, 1) == 0x6E789E6AA1B965F4
    assert R.mix(0, 2) == 0x06C45D188009454F and R.mix(1234567, 0) == 0x599ED017FB08FC85
    assert [R.sample_slot(0, c, 18000) for c in (0, 1)] == [15899, 7767]
    assert R.mix(R.M64, R.M64) <= R.M64                                       # the counter and the seed wrap modulo 2^64
    act = np.arange(18000) * 2
    tri = R.sample(0, 0, 4, act)
    assert tri.shape == (4, 3) and tri.dtype == np.int32 and tri[0, 0] == 2 * 15899 and tri[0, 1] == 2 * 7767
    assert np.array_equal(R.sample(0, 1, 4, act)[0], [act[R.sample_slot(0, 12 + j, 18000)] for j in range(3)])


def test_slots_cover_the_list_and_stay_inside_it():
    for m in (1, 3, 7, 18000, (1 << 31) - 17):
        s = [R.sample_slot(5, c, m) for c in range(2000)]
        assert min(s) >= 0 and max(s) < m
    assert len(set(R.sample_slot(9, c, 7) for c in range(200))) == 7


# ---- hand-derived cases -----------------------------------------------------------------------------------------------------
def test_lattice_rows_on_and_beside_a_plane_counts_by_hand():
    """The plane z = 0.5 as (0, 0, 1, -0.5).  40 rows on it, 30 rows one lattice step 2^-10 above, 20 two steps below, 10
    three steps above, on the 2^-10 lattice: every product and sum is exact, so the residuals are 0, +s, -2 s, +3 s."""
    s = 2.0 ** -10
    rng = np.random.default_rng(1)
    xy = rng.integers(-2000, 2000, (100, 2)) * s
    z = np.concatenate([np.full(40, 0.5), np.full(30, 0.5 + s), np.full(20, 0.5 - 2 * s), np.full(10, 0.5 + 3 * s)])
    pts = np.column_stack([xy, z])
    pl = [0.0, 0.0, 1.0, -0.5]
    assert sorted(set(R.residual(pts, pl).tolist())) == [-2 * s, 0.0, s, 3 * s]
    for thr, want in ((0.0, 40), (s / 2, 40), (s, 70), (np.nextafter(s, 0), 40), (2 * s, 90), (np.nextafter(2 * s, 0), 70),
                      (3 * s, 100), (np.inf, 100)):
        assert R.score(pts, [pl], thr)[0] == want, thr
    active = np.ones(100, np.uint8)
    active[:15] = 0                                                           # 15 of the rows on the plane
    active[95:] = 0                                                           # 5 of the rows three steps above
    assert R.score(pts, [pl], 3 * s, active)[0] == 80 and R.score(pts, [pl], 0.0, active)[0] == 25
    assert R.score(pts, [pl, [np.nan, 0, 1, 0], [0, 0, -1.0, 0.5]], s).tolist() == [70, 0, 70]   # a NaN plane; no sign rule
    pts[3, 0] = np.nan                                                        # 0 * NaN: the row is an inlier of nothing
    pts[50, 1] = np.inf
    assert R.score(pts, [pl], np.inf)[0] == 98
    lab, act, k = R.label(pts, pl, 0.0, 7, np.full(100, -1), active)
    assert k == 25 and (lab == 7).sum() == 25 and (lab[:15] == -1).all() and act[15:40].sum() == 0 and act[40:95].all()


def test_plane_of_a_triple_by_hand():
    pts = np.array([[0, 0, 0.5], [1, 0, 0.5], [0, 1, 0.5], [2, 0, 0.5], [3, 0, 0.5], [1, 1, 1.5]], np.float64)
    pl, ok = R.from_triples(pts, [[0, 1, 2], [0, 2, 1], [0, 1, 3], [1, 1, 2], [0, 1, 6], [0, -1, 2], [0, 1, 5]])
    assert ok.tolist() == [1, 1, 0, 0, 0, 0, 1]
    assert pl[0].tolist() == [0.0, 0.0, 1.0, -0.5] and pl[1].tolist() == [-0.0, -0.0, -1.0, 0.5]   # the triple's order is the sign
    assert (R.bits(pl[2:6]) == 0x7FF8000000000000).all()                      # collinear, repeated, out of range (both ends)
    assert np.allclose(pl[6], [0.0, -np.sqrt(0.5), np.sqrt(0.5), -np.sqrt(0.5) * 0.5])
    # an exactly zero normal that is not a repeated index: three distinct collinear lattice rows
    s = 2.0 ** -10
    line = np.array([[k * 3 * s, k * 5 * s, k * 7 * s] for k in (1, 2, 5)]) + 0.25
    assert R.from_triples(line, [[0, 1, 2]])[1].tolist() == [0]
    # overflow and underflow of the cross product; a NaN row
    big = np.array([[0, 0, 0], [1e200, 0, 0], [0, 1e200, 0]], np.float64)
    small = big / 1e200 * 1e-200                                              # products of 1e-400 are 0: nrm = 0
    assert R.from_triples(big, [[0, 1, 2]])[1].tolist() == [0] and R.from_triples(small, [[0, 1, 2]])[1].tolist() == [0]
    assert R.from_triples(big * 1e-150, [[0, 1, 2]])[1].tolist() == [1]       # 1e50: squares of 1e200 are finite
    pts[2, 1] = np.nan
    assert R.from_triples(pts, [[0, 1, 2]])[1].tolist() == [0]


def test_extraction_stops_and_ties():
    s = 2.0 ** -10
    rng = np.random.default_rng(2)
    flat = np.column_stack([rng.integers(-500, 500, (300, 2)) * s, np.full(300, 0.25)])
    fit = R.ransac(flat, 0.0, 32, 3, refit=False, seed=4)                     # one exact plane: every valid hypothesis ties
    pl, ok = R.from_triples(flat, R.sample(4, 0, 32, np.arange(300)))
    first = int(np.nonzero(ok)[0][0])
    assert fit["n_planes"] == 1 and fit["counts"][0] == 300 and fit["winners"] == [first] and R.same(fit["planes"][0], pl[first])
    assert (fit["labels"] == 1).all() and (R.bits(fit["planes"][1:]) == 0x7FF8000000000000).all()
    assert R.ransac(flat, 0.0, 32, 3, min_inliers=301)["n_planes"] == 0       # min_inliers above every count
    assert R.ransac(flat, 0.0, 32, 0)["n_planes"] == 0 and R.ransac(flat[:2], 1.0, 32, 3)["n_planes"] == 0
    act = np.zeros(300, np.uint8)
    act[[5, 9]] = 1
    assert R.ransac(flat, 1.0, 32, 3, active=act)["n_planes"] == 0            # m < 3


# ---- the header against the library, the binding and vcp.h -------------------------------------------------------------------
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
    from vtkcloudpoint_amd import _native, planes
    protos = _prototypes(HEADER)
    assert len(protos) == 7 and protos["vcp_plane_ransac_dev"] == 16 and protos["vcp_plane_score_shape"] == 2
    lib = _native.lib()
    assert [s for s in protos if not hasattr(lib, s)] == []
    assert sorted(planes.SYMBOLS) == sorted(protos)
    assert {k: len(v) for k, v in planes._PROTOTYPES.items()} == protos           # the ctypes prototypes
    with open(os.path.join(ROOT, "vtkcloudpoint_amd", "planes.py")) as f:
        tree = ast.parse(f.read())
    calls = {}
    for node in ast.walk(tree):
        if not (isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute)):
            continue
        base = node.func.value
        if not (isinstance(base, ast.Call) and isinstance(base.func, ast.Name) and base.func.id == "_L"):
            continue
        name = node.func.attr
        assert name in protos, "%s (line %d) is not in vcp_planes.h" % (name, node.lineno)
        assert not node.keywords and not any(isinstance(a, ast.Starred) for a in node.args), name
        assert len(node.args) == protos[name], "%s (line %d): %d arguments, the header has %d" % (
            name, node.lineno, len(node.args), protos[name])
        calls[name] = calls.get(name, 0) + 1
    assert sorted(calls) == sorted(protos)                                        # every function has a call site


def test_no_name_collides_with_vcp_h_and_vcp_h_declares_none_of_them():
    from vtkcloudpoint_amd import _native, planes
    old = _prototypes(os.path.join(ROOT, "include", "vcp.h"))
    new = _prototypes(HEADER)
    assert len(old) >= 97 and not set(old) & set(new)
    assert not set(planes.SYMBOLS) & set(_native.SYMBOLS)
    with open(HEADER) as f:
        assert '#include "vcp.h"' in f.read()


def test_the_package_exports_the_planes_functions():
    import vtkcloudpoint_amd as V
    from vtkcloudpoint_amd import planes
    for name in ("extract_planes", "plane_score", "planes_from_triples", "plane_residuals", "remove_planes", "Planes"):
        assert getattr(V, name) is getattr(planes, name)
    fit = planes.Planes(np.zeros((0, 4)), np.zeros(0, np.int64), np.zeros(0, np.int64), np.array([0, 2, 0, 1], np.int32), 0)
    keep, idx = planes.remove_planes(fit)
    assert keep.tolist() == [1, 0, 1, 0] and idx.tolist() == [0, 2] and idx.dtype == np.int32
    pts = np.array([[1.0, 2.0, 3.0], [0.5, 0.25, 0.125]])
    assert R.same(planes.plane_residuals(pts, [0.5, -1.0, 2.0, 0.25]), R.residual(pts, [0.5, -1.0, 2.0, 0.25]))


# ---- recovery on the restatement ----------------------------------------------------------------------------------------------
# Caps, fixed before any run (the plain numpy version with an eigh refit gives, over the five scenes: worst angle 0.009
# degrees, worst recall 0.9875, most foreign rows 54, lowest winner count 3876).
MAX_ANGLE_DEG, MIN_RECALL, MAX_FOREIGN = 0.05, 0.98, 100

@pytest.mark.parametrize("k", range(5))
def test_restatement_recovers_the_three_planes(k):
    pts, truth, normals, fit = R.scene_fit(k)          # tests/test_planes_gpu.py holds the device to the same result
    assert len(pts) == 18000 and (truth > 0).sum() == 12000
    rec = R.recovery(fit, truth, normals)
    print("\nscene %d: counts %s, winners' counts %s, (plane, angle, recall, foreign) %s"
          % (k, fit["counts"][:3].tolist(), fit["hyp_counts"][:3].tolist(), rec))
    assert fit["n_planes"] == 3
    assert sorted(r[0] for r in rec) == [0, 1, 2]                                 # each a different true plane
    for _, ang, recall, foreign in rec:
        assert ang <= MAX_ANGLE_DEG and recall >= MIN_RECALL and foreign <= MAX_FOREIGN
    assert fit["hyp_counts"][:3].min() >= 1000 and (fit["counts"][:3] >= fit["hyp_counts"][:3]).all()
