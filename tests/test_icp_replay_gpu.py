"""Bit-exact host replay of the device ICP loop: icp.hip says of horn() "host and device: same code, same rounding", and
this is the test of it.  vcp_icp_sums(model, data, R, T) runs the pass of a round that starts from state (R, T) -- the same
icp_run, workgroup count and fixed-order reduction -- so its 16 sums are the bits that round's k_icp_step sees.  The replay
feeds them to vcp_selftest_horn (the HOST run of horn(), basis all zero before round 1 and fed back afterwards), applies
the stop rule and the composition of icp_step_body in plain Python floats, and must land on the device's R, T, sse and
iters bit for bit.  With that, what tests/test_horn_step.py finds on the host holds for the kernel.

A difference is a finding (first suspects: a contraction or another sqrt/division expansion in the device build of
horn(); a basis or pre_d that does not survive the 8-round batch boundary): the failing assertion names the round count.
All inputs are finite and small: at most 300 000 points and 17 rounds."""
import ctypes as C
import math

import numpy as np
import pytest

from vtkcloudpoint_amd import _native as N

pytestmark = pytest.mark.gpu

REFERENCE, VTK = "reference", "vtk"
ROUNDS = (1, 2, 8, 9, 17)  # around the 8-round batch boundary


def _horn(S, nd, V):
    R1, T1 = np.zeros(9), np.zeros(3)
    Vb = np.ascontiguousarray(V, np.float64).copy()
    rc = N.lib().vcp_selftest_horn(S.ctypes.data_as(C.c_void_p), C.c_int64(nd), Vb.ctypes.data_as(C.c_void_p), C.c_int(1),
                                   R1.ctypes.data_as(C.c_void_p), T1.ctypes.data_as(C.c_void_p))
    assert rc == 1
    return [float(x) for x in R1], [float(x) for x in T1], Vb


def _compose(R1, T1, R, T):
    """R <- R1 R, T <- R1 T + T1 in icp_step_body's order: row by row, k ascending, acc + T1[i] last."""
    tR, tT = [0.0] * 9, [0.0] * 3
    for i in range(3):
        for j in range(3):
            acc = 0.0
            for k in range(3):
                acc += R1[3 * i + k] * R[3 * k + j]
            tR[3 * i + j] = acc
    for i in range(3):
        acc = 0.0
        for k in range(3):
            acc += R1[3 * i + k] * T[k]
        tT[i] = acc + T1[i]
    return tR, tT


def trace(ctx, model, data, R, T, rounds, mode):
    """Rounds 1..rounds with every round asked to continue: [(d, R after, T after)] per round."""
    R, T = [float(x) for x in np.asarray(R).reshape(9)], [float(x) for x in np.asarray(T).reshape(3)]
    V = np.zeros(16)
    out = []
    for rnd in range(1, rounds + 1):
        S, _ = ctx.icp_sums(model, data, np.array(R).reshape(3, 3), np.array(T), want_nn=False)
        R1, T1, V = _horn(S, len(data), V)
        if mode == REFERENCE and rnd == 1:  # the first result overwrites R, T
            R, T = R1, T1
        else:
            R, T = _compose(R1, T1, R, T)
        out.append((float(S[15]), list(R), list(T)))
    return out


def predict(tr, nd, max_iter, stop_rule=N.STOP_SSE_DELTA, tol=0.0, R0=None, T0=None):
    """icp_step_body's stop rule (MODE_REFERENCE) walked over a trace: (R, T, sse, iters).  R0, T0 = what the caller's
    buffers hold when no round asks to continue (vcp_icp_dev leaves them untouched)."""
    R, T = R0, T0
    d = 0.0
    for rnd in range(1, max_iter + 1):
        pre_d, d = d, tr[rnd - 1][0]
        go = math.sqrt(d / nd) >= tol if stop_rule == N.STOP_RMSE else abs(d - pre_d) >= tol
        if go:
            R, T = tr[rnd - 1][1], tr[rnd - 1][2]
        if not go or rnd >= max_iter:
            return R, T, d, rnd


def scene(seed, nm, nd, angle, shift, noise, planar=False, offset=0.0, scale=1.0):
    """A model and data drawn from it, moved back by a rigid motion about the cloud's centre, plus noise."""
    rng = np.random.default_rng(seed)
    model = rng.uniform(-10.0, 10.0, (nm, 3))
    ax = np.array([0.3, -0.2, 1.0])
    if planar:
        model[:, 2] = 0.0
        ax = np.array([0.0, 0.0, 1.0])
    ax = ax / np.linalg.norm(ax)
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    Rm = np.eye(3) + math.sin(angle) * K + (1 - math.cos(angle)) * (K @ K)
    x = model[rng.integers(0, nm, nd)] + noise * rng.normal(size=(nd, 3))
    t = np.asarray(shift, np.float64)
    if planar:
        x[:, 2] = 0.0
        t = t * (1, 1, 0)
    data = (x - t) @ Rm
    return np.ascontiguousarray((model + offset) * scale), np.ascontiguousarray((data + offset) * scale)


def _check_icp(ctx, model, data, label):
    nd = len(data)
    tr = trace(ctx, model, data, np.eye(3), np.zeros(3), max(ROUNDS), REFERENCE)
    zero9, zero3 = [0.0] * 9, [0.0] * 3  # Context.icp hands zeroed R, T to the library
    runs = [(r, N.STOP_SSE_DELTA, 0.0) for r in ROUNDS]
    # a tolerance that stops the run mid-way, per stop rule, and one that stops round 1 (R, T stay untouched)
    deltas = [abs(tr[0][0])] + [abs(tr[k][0] - tr[k - 1][0]) for k in range(1, len(tr))]
    rmse = [math.sqrt(t[0] / nd) for t in tr]
    runs += [(17, N.STOP_SSE_DELTA, 1.5 * deltas[4]), (17, N.STOP_RMSE, rmse[3] * (1 + 1e-9)),
             (17, N.STOP_SSE_DELTA, 2.0 * deltas[0]), (17, N.STOP_RMSE, 2.0 * rmse[0]), (9, N.STOP_RMSE, 0.0)]
    mid = 0
    for max_iter, rule, tol in runs:
        R, T, d, iters = predict(tr, nd, max_iter, rule, tol, zero9, zero3)
        g = ctx.icp(model, data, tol, max_iter, rule)
        what = (label, max_iter, rule, tol, "replay stops after", iters, "device after", g["iters"])
        assert g["iters"] == iters, what
        assert g["sse"] == d, what
        assert g["rmse"] == math.sqrt(d / nd), what
        assert np.array_equal(g["R"].reshape(9), np.array(R)), what
        assert np.array_equal(g["T"], np.array(T)), what
        mid += 1 < iters < max_iter
    assert mid >= 1, (label, deltas, rmse)  # some run did stop between round 1 and max_iter
    R, T, _, iters = predict(tr, nd, 17, N.STOP_RMSE, 2.0 * rmse[0], zero9, zero3)
    assert iters == 1 and R == zero9 and T == zero3
    return tr


@pytest.mark.parametrize("label,nm,nd", [("one-wave workgroups", 300, 20000), ("256-lane workgroups", 300, 300000),
                                         ("grid", 3000, 20000)])
def test_icp_is_the_replay(vcp_ctx, label, nm, nd):
    model, data = scene(1000 + nm + nd % 7, nm, nd, 0.12 if nm < 1000 else 0.05, (0.8, -0.5, 0.3), 0.05)
    tr = _check_icp(vcp_ctx, model, data, label)
    assert tr[-1][0] < tr[0][0]  # the run does converge: later rounds are warm starts on a nearly diagonal problem


@pytest.mark.parametrize("label,kw", [("offset 1e5", dict(offset=1e5)), ("planar", dict(planar=True)),
                                      ("scaled by 2^40", dict(scale=2.0 ** 40))])
def test_icp_is_the_replay_on_hard_clouds(vcp_ctx, label, kw):
    model, data = scene(77, 200, 5000, 0.1, (0.6, -0.4, 0.2), 0.03, **kw)
    _check_icp(vcp_ctx, model, data, label)


def _seq_mean(a):
    """Sequential binary64 sums over all points, one division (vcp.h, vcp_icp_vtklike's centroid start)."""
    s = [0.0, 0.0, 0.0]
    for row in a.tolist():
        for c in range(3):
            s[c] += row[c]
    return [s[c] / float(len(a)) for c in range(3)]


def _landmarks(src, ml):
    ns = len(src)
    step = ns // ml if ns > ml else 1
    return np.ascontiguousarray(src[::step][: ns // step])


@pytest.mark.parametrize("ns,ml", [(1000, 200), (150, 200)])
@pytest.mark.parametrize("centroids", [True, False])
def test_vtklike_is_the_replay(vcp_ctx, ns, ml, centroids):
    tgt, src = scene(300 + ns, 300, ns, 0.1, (0.7, -0.4, 0.0), 0.05, planar=True)
    lm = _landmarks(src, ml)
    assert len(lm) == (200 if ns == 1000 else 150)
    T0 = [0.0, 0.0, 0.0]
    if centroids:
        ms, mt = _seq_mean(src), _seq_mean(tgt)
        T0 = [mt[c] - ms[c] for c in range(3)]
    tr = trace(vcp_ctx, tgt, lm, np.eye(3), T0, max(ROUNDS), VTK)
    for r in ROUNDS:
        g = vcp_ctx.icp_vtklike(src, tgt, r, ml, centroids)
        d, R, T = tr[r - 1]
        M = np.eye(4)
        M[:3, :3] = np.array(R).reshape(3, 3)
        M[:3, 3] = T
        assert g["iters"] == r
        assert np.array_equal(g["M"], M), ("rounds", r)
        assert g["mean_dist"] == math.sqrt(d / len(lm)), ("rounds", r)


@pytest.mark.parametrize("nt", [300, 3000])
def test_multistart_every_pose_is_its_own_replay(vcp_ctx, nt):
    """8 poses, one a reflection, generated T0_h = mt - R0_h ms: every pose's M and mean_dist equal its own replay from a
    cold basis, so no pose sees another's warm basis."""
    tgt, src = scene(500 + nt, nt, 1000, 0.1, (0.7, -0.4, 0.0), 0.05, planar=True)
    ml, rounds = 200, 17
    lm = _landmarks(src, ml)
    Rs = []
    for h in range(8):
        th = h * (2 * math.pi / 8)
        c, s = math.cos(th), math.sin(th)
        Rs.append([c, -s, 0.0, s, c, 0.0, 0.0, 0.0, 1.0])
    Rs[5] = [Rs[5][0], -Rs[5][1], 0.0, Rs[5][3], -Rs[5][4], 0.0, 0.0, 0.0, 1.0]  # Rz diag(1, -1, 1): det -1
    assert np.linalg.det(np.array(Rs[5]).reshape(3, 3)) < -0.99
    g = vcp_ctx.icp_multistart(src, tgt, np.array(Rs).reshape(8, 3, 3), None, rounds, ml, 1.0)
    ms, mt = _seq_mean(src), _seq_mean(tgt)
    for h in range(8):
        R0 = Rs[h]
        T0 = [mt[r] - (R0[3 * r] * ms[0] + R0[3 * r + 1] * ms[1] + R0[3 * r + 2] * ms[2]) for r in range(3)]
        d, R, T = trace(vcp_ctx, tgt, lm, R0, T0, rounds, VTK)[-1]
        M = np.eye(4)
        M[:3, :3] = np.array(R).reshape(3, 3)
        M[:3, 3] = T
        assert np.array_equal(g["M_all"][h], M), ("pose", h)
        assert g["mean_dist"][h] == math.sqrt(d / len(lm)), ("pose", h)
    assert np.linalg.det(g["M_all"][5][:3, :3]) < 0  # the reflection is kept: Horn's R1 is proper
