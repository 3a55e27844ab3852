"""The four _dev forms of include/vcp_planes.h on a caller's non-blocking stream, under the scheme of
tests/test_stream_gpu.py (its docstring has the argument and the measured margins): the input buffers hold cloud A; on the
caller's stream a filler kernel, then the copy of cloud B over the inputs and a poison over the outputs; the entry point
is called while the filler still runs, blocks until its work on that stream is done, and must give the restatement's
answer for B, which differs from its answer for A.  A launch, copy or memset sent to the context's own stream reads A or
is overwritten by the poison."""
import ctypes as C

import numpy as np
import pytest
import torch

import plane_ref as R
from test_stream_gpu import Rig, dev, host
from vtkcloudpoint_amd import planes as PL

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rig():
    r = Rig()
    yield r
    r.close()


def test_plane_score_dev(rig):
    n, H = 5000, 1030                                     # two passes over the cloud, several tiles
    A, B, pl = R.lattice_rows(n, 40), R.lattice_rows(n, 41), R.generic_planes(H, 42)
    act = (np.arange(n) % 7 != 0).astype(np.uint8)
    wA, wB = R.score(A, pl, 0.25, act), R.score(B, pl, 0.25, act)
    assert not np.array_equal(wA, wB)
    buf, dB, d_pl, d_act = dev(A), dev(B), dev(pl), dev(act)
    counts = torch.zeros(H, dtype=torch.int64, device="cuda")
    rig.run(lambda: rig.ctx._chk(PL._L().vcp_plane_score_dev(rig.ctx._h, buf.data_ptr(), 3, n, d_act.data_ptr(), d_pl.data_ptr(),
                                                             H, 0.25, counts.data_ptr())),
            [(buf, dB)], [(counts, -7)])
    assert np.array_equal(host(counts), wB)


def test_planes_from_triples_dev(rig):
    n, H = 3000, 300
    A, B = R.lattice_rows(n, 43), R.lattice_rows(n, 44)
    tri = np.random.default_rng(45).integers(0, n, (H, 3)).astype(np.int32)
    (pA, _), (pB, okB) = R.from_triples(A, tri), R.from_triples(B, tri)
    assert not R.same(pA, pB) and okB.sum() > H // 2
    buf, dB, d_tri = dev(A), dev(B), dev(tri)
    out, ok = torch.zeros((H, 4), dtype=torch.float64, device="cuda"), torch.zeros(H, dtype=torch.uint8, device="cuda")
    rig.run(lambda: rig.ctx._chk(PL._L().vcp_planes_from_triples_dev(rig.ctx._h, buf.data_ptr(), 3, n, d_tri.data_ptr(), H,
                                                                     out.data_ptr(), ok.data_ptr())),
            [(buf, dB)], [(out, -7.0), (ok, 9)])
    assert R.same(host(out), pB) and np.array_equal(host(ok), okB)


def test_plane_label_dev(rig):
    """labels and active are in/out: before the filler they hold -9 and 0 (nothing active), behind it -5 and the flags."""
    n = 6000
    A, B = R.lattice_rows(n, 46), R.lattice_rows(n, 47)
    plane = np.ascontiguousarray(R.generic_planes(1, 48)[0])
    act = (np.arange(n) % 3 != 0).astype(np.uint8)
    lA, _, kA = R.label(A, plane, 0.5, 11, np.full(n, -5, np.int32), act)
    lB, aB, kB = R.label(B, plane, 0.5, 11, np.full(n, -5, np.int32), act)
    assert not np.array_equal(lA, lB) and kB > 0
    buf, dB, d_actB = dev(A), dev(B), dev(act)
    d_lab = torch.full((n,), -9, dtype=torch.int32, device="cuda")
    d_act = torch.zeros(n, dtype=torch.uint8, device="cuda")
    got = C.c_int64(-1)
    rig.run(lambda: rig.ctx._chk(PL._L().vcp_plane_label_dev(rig.ctx._h, buf.data_ptr(), 3, n, d_act.data_ptr(), plane.ctypes.data,
                                                             0.5, 11, d_lab.data_ptr(), C.byref(got))),
            [(buf, dB), (d_act, d_actB)], [(d_lab, -5)])
    assert got.value == kB and np.array_equal(host(d_lab), lB) and np.array_equal(host(d_act), aB)


def test_plane_ransac_dev(rig):
    pts, _, _, want = R.scene_fit(0, masked=True)
    act, c = R.scene_mask(0), R.scene_call(0)
    n, mp = len(pts), c["max_planes"]
    A = np.zeros_like(pts)                                # every triple is degenerate: no plane
    assert R.ransac(A, active=act, **c)["n_planes"] == 0 and want["n_planes"] == 3
    buf, dB, d_act = dev(A), dev(np.array(pts)), dev(act)
    labels = torch.zeros(n, dtype=torch.int32, device="cuda")
    planes, counts, hyp, npl = np.full((mp, 4), -7.0), np.full(mp, -7, np.int64), np.full(mp, -7, np.int64), C.c_int32(-7)
    rig.run(lambda: rig.ctx._chk(PL._L().vcp_plane_ransac_dev(rig.ctx._h, buf.data_ptr(), 3, n, d_act.data_ptr(), c["thr"], c["H"],
                                                              mp, c["min_inliers"], c["seed"], 1, labels.data_ptr(),
                                                              planes.ctypes.data, counts.ctypes.data, hyp.ctypes.data,
                                                              C.byref(npl))),
            [(buf, dB)], [(labels, -7)])
    got = dict(labels=host(labels), planes=planes, counts=counts, hyp_counts=hyp, n_planes=npl.value)
    assert R.differs(got, want) is None, R.differs(got, want)
