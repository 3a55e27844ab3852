"""vcp_cluster_quantiles / vcp_cluster_mad on the MI355X: every output equal to the numpy restatement of the definition
(tests/cluster_quant_ref.py), doubles by their bits, on the smallest shapes at which each size class and each hard value can
go wrong; the device-pointer forms, independence from the context's history, the timing phases, every error with its
outputs untouched, and robust.py down to robust_fixed_centroids."""
import ctypes as C

import numpy as np
import pytest
import torch

import cluster_quant_ref as R
from vtkcloudpoint_amd import _native as N

pytestmark = pytest.mark.gpu

Q4 = [0.0, 0.25, 0.5, 1.0]
N_WAVE, N_WG = R.WAVE_MAX, R.WG_MAX
POISON = -7.25


def _q_dev(ctx, flat, group, K, q, stride=1):
    dv, dg = torch.from_numpy(np.ascontiguousarray(flat, np.float64)).cuda(), torch.from_numpy(group).cuda()
    out = torch.full((K * len(q),), POISON, dtype=torch.float64, device="cuda")
    cnt = torch.full((K,), -7, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    ctx.cluster_quantiles_dev(dv.data_ptr(), stride, dg.data_ptr(), len(group), K, q, out.data_ptr(), cnt.data_ptr())
    return out.cpu().numpy().reshape(K, len(q)), cnt.cpu().numpy()


def _mad_dev(ctx, flat, group, K, c, floor, stride=1):
    dv, dg = torch.from_numpy(np.ascontiguousarray(flat, np.float64)).cuda(), torch.from_numpy(group).cuda()
    med, mad, thr = (torch.full((K,), POISON, dtype=torch.float64, device="cuda") for _ in range(3))
    rej = torch.full((len(group),), 9, dtype=torch.uint8, device="cuda")
    kept = torch.full((K,), -7, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    nr = ctx.cluster_mad_dev(dv.data_ptr(), stride, dg.data_ptr(), len(group), K, c, floor, med.data_ptr(), mad.data_ptr(),
                             thr.data_ptr(), rej.data_ptr(), kept.data_ptr())
    return dict(med=med.cpu().numpy(), mad=mad.cpu().numpy(), thr=thr.cpu().numpy(), reject=rej.cpu().numpy(),
                kept=kept.cpu().numpy(), n_rejected=nr)


def _check_q(ctx, flat, group, K, q, stride=1):
    """Host form and device-pointer form == restatement; returns the restatement."""
    group = np.ascontiguousarray(group, np.int32)
    want = R.quantiles(flat, group, K, q, stride)
    for name, got in (("host", ctx.cluster_quantiles(flat, group, K, q, stride)), ("dev", _q_dev(ctx, flat, group, K, q, stride))):
        assert R.same_bits(got[1], want[1]), "%s form: counts differ" % name
        bad = np.nonzero(R.bits(got[0]) != R.bits(want[0]))
        assert len(bad[0]) == 0, "%s form: out differs at (group - 1, rank) %s" % (name, list(zip(*bad))[:5])
    return want


def _check_mad(ctx, flat, group, K, c, floor, stride=1):
    group = np.ascontiguousarray(group, np.int32)
    want = R.mad(flat, group, K, c, floor, stride)
    for name, got in (("host", ctx.cluster_mad(flat, group, K, c, floor, stride)),
                      ("dev", _mad_dev(ctx, flat, group, K, c, floor, stride))):
        bad = R.same_mad(got, want)
        assert bad is None, "%s form: %s differs" % (name, bad)
    return want


# ---- size classes ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stride", [1, 3])
def test_size_classes(vcp_ctx, stride):
    flat, group, K, sizes = R.size_class_case(11 + stride, stride)
    assert {0, 1, 2, 3, 63, 64, 65, N_WAVE - 1, N_WAVE, N_WAVE + 1, N_WG - 1, N_WG, N_WG + 1} <= set(sizes)
    assert max(sizes) >= 5 * N_WG and (group == 0).sum() == 3000
    want = _check_q(vcp_ctx, flat, group, K, Q4, stride)
    assert want[1].tolist() == sizes
    _check_mad(vcp_ctx, flat, group, K, 3.0, 0.0, stride)      # the second select of the MAD chain, in every class


def test_class_independence(vcp_ctx):
    """The same values as one large group, as ten workgroup-sized ones and as two hundred wave-sized ones."""
    rng = np.random.default_rng(5)
    n = 3 * N_WG + 5
    v = np.round(rng.normal(0.0, 3.0, n), 3)
    one = _check_q(vcp_ctx, v, np.ones(n, np.int32), 1, Q4)
    assert one[1][0] > N_WG
    for K in (10, 200):
        group = (1 + np.arange(n) % K).astype(np.int32)
        w = _check_q(vcp_ctx, v, group, K, Q4)
        assert (N_WAVE < w[1].min() and w[1].max() <= N_WG) if K == 10 else w[1].max() <= N_WAVE
        assert w[0][:, 0].min() == one[0][0, 0] and w[0][:, 3].max() == one[0][0, 3]
    # every row a group of its own: each rank is the row
    small = v[:300]
    w = _check_q(vcp_ctx, small, np.arange(1, 301, dtype=np.int32), 300, Q4)
    assert R.same_bits(w[0], np.repeat(small[:, None], 4, axis=1))


# ---- hard values ----------------------------------------------------------------------------------------------------------
def _hard_groups():
    rng = np.random.default_rng(9)
    vals, grp, kinds = [], [], []
    base = np.array([1234.5]).view(np.uint64)[0] & ~np.uint64(255)
    for size in (40, 700, 5000):                # one size per class
        makers = [
            ("one value", lambda s: np.full(s, 17.125)),
            ("zeros", lambda s: np.where(rng.integers(0, 2, s) == 1, 0.0, -0.0)),
            ("lattice", lambda s: rng.integers(-40, 40, s) / 1024.0),
            ("last digit", lambda s: (base + rng.integers(0, 256, s).astype(np.uint64)).view(np.float64)),
            ("nan", lambda s: np.where(rng.random(s) < 0.3, R.hard_values()[-7:][rng.integers(0, 7, s)], rng.normal(0, 1, s))),
            ("inf", lambda s: rng.choice([np.inf, -np.inf, 1.0, -1.0, 0.0], s)),
            ("all nan", lambda s: R.hard_values()[-7:][rng.integers(0, 7, s)]),
            ("every hard value", lambda s: R.hard_values()[rng.integers(0, len(R.hard_values()), s)]),
        ]
        for name, mk in makers:
            v = mk(size)
            if name == "zeros":
                v[0], v[1] = 0.0, -0.0
            vals.append(v)
            grp.append(np.full(size, len(kinds) + 1, np.int32))
            kinds.append((name, size))
    v, g = np.concatenate(vals), np.concatenate(grp)
    order = rng.permutation(len(v))
    return v[order], g[order], kinds


def test_hard_values(vcp_ctx):
    v, g, kinds = _hard_groups()
    K = len(kinds)
    out, counts = _check_q(vcp_ctx, v, g, K, Q4)
    assert counts.tolist() == [s for _, s in kinds]
    for k, (name, _) in enumerate(kinds):
        b = R.bits(out[k])
        if name == "one value":
            assert np.all(out[k] == 17.125)
        elif name == "zeros":
            assert b[0] == R.SIGN and b[3] == 0                 # -0 is the minimum, +0 the maximum
        elif name == "last digit":
            assert len(set((b >> np.uint64(8)).tolist())) == 1 and b[0] < b[3]
        elif name in ("nan", "every hard value"):
            assert b[3] == R.NAN_BITS and not np.isnan(out[k, 0])
        elif name == "all nan":
            assert np.all(b == R.NAN_BITS)
        elif name == "inf":
            assert out[k, 0] == -np.inf and out[k, 3] == np.inf
    w = _check_mad(vcp_ctx, v, g, K, 3.0, 0.0)
    assert np.all(w["reject"][np.isnan(v)] == 1)                # a NaN row is rejected


# ---- MAD ------------------------------------------------------------------------------------------------------------------
def test_mad_scene(vcp_ctx):
    dist, group, planted, K = R.mad_scene()
    w = _check_mad(vcp_ctx, dist, group, K, 3.0, 0.0)
    got = vcp_ctx.cluster_mad(dist, group, K, 3.0, 0.0)
    assert np.all(got["reject"][planted] == 1)                                  # every planted outlier goes
    assert not np.any((got["reject"] != 0) & (w["reject"] == 0))                # no inlier of the restatement is lost
    inl = w["reject"] == 0
    assert ((dist[planted] >= dist[inl].min()) & (dist[planted] <= dist[inl].max())).sum() >= 1   # one band cannot


def test_mad_floor_and_zero_band(vcp_ctx):
    rng = np.random.default_rng(2)
    # mad == 0: more than half of a group is one value; a floor keeps the near ones
    v = np.r_[np.full(60, 5.0), 5.0 + rng.uniform(-0.01, 0.01, 30), 9.0, np.full(3000, 2.0), 2.004, 2.006, np.nan]
    g = np.r_[np.full(91, 1), np.full(3003, 2)].astype(np.int32)
    w = _check_mad(vcp_ctx, v, g, 2, 3.0, 0.005)
    assert w["mad"].tolist() == [0.0, 0.0] and w["thr"].tolist() == [0.005, 0.005]
    assert w["kept"][0] >= 60 and w["reject"][90] == 1 and w["reject"][:60].sum() == 0
    assert w["reject"][-3:].tolist() == [0, 1, 1]
    # floor = +inf rejects only NaN
    w = _check_mad(vcp_ctx, v, g, 2, 3.0, np.inf)
    assert w["n_rejected"] == 1 and w["reject"][-1] == 1
    # c_mad = 0, floor = 0: everything off the median goes
    w = _check_mad(vcp_ctx, v, g, 2, 0.0, 0.0)
    assert np.array_equal(w["reject"] != 0, ~(v == np.where(g == 1, 5.0, 2.0)))
    # an empty group, group 0 rows, K == 0 and n == 0
    g3 = np.where(g == 2, 3, g).astype(np.int32)
    g3[:5] = 0
    w = _check_mad(vcp_ctx, v, g3, 3, 3.0, 0.5)
    assert np.isnan(w["med"][1]) and np.isnan(w["mad"][1]) and w["thr"][1] == 0.5 and w["kept"][1] == 0
    assert w["reject"][:5].sum() == 0
    w = _check_mad(vcp_ctx, v[:7], np.zeros(7, np.int32), 0, 3.0, 0.0)
    assert w["n_rejected"] == 0 and w["reject"].tolist() == [0] * 7
    w = _check_mad(vcp_ctx, np.zeros(0), np.zeros(0, np.int32), 2, 3.0, 1.0)
    assert w["thr"].tolist() == [1.0, 1.0] and w["kept"].tolist() == [0, 0]
    q = _check_q(vcp_ctx, np.zeros(0), np.zeros(0, np.int32), 2, Q4)
    assert np.all(R.bits(q[0]) == R.NAN_BITS) and q[1].tolist() == [0, 0]
    _check_q(vcp_ctx, v[:7], np.zeros(7, np.int32), 0, Q4)


# ---- device forms, history, phases ----------------------------------------------------------------------------------------
def test_history_and_phases(vcp_ctx):
    flat, group, K, _ = R.size_class_case(21)
    a = _q_dev(vcp_ctx, flat, group, K, Q4)
    b = _q_dev(vcp_ctx, flat, group, K, Q4)
    m1 = _mad_dev(vcp_ctx, flat, group, K, 3.0, 0.0)
    pts = torch.from_numpy(np.random.default_rng(1).uniform(0, 10, (5000, 2))).cuda()
    lab = torch.zeros(5000, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    vcp_ctx.dbscan_dev(pts.data_ptr(), 5000, 2, 0.3, 5, d_labels=lab.data_ptr())
    c = _q_dev(vcp_ctx, flat, group, K, Q4)
    m2 = _mad_dev(vcp_ctx, flat, group, K, 3.0, 0.0)
    want = R.quantiles(flat, group, K, Q4)
    for got in (a, b, c):
        assert R.same_bits(got[0], want[0]) and R.same_bits(got[1], want[1])
    assert R.same_mad(m1, m2) is None
    vcp_ctx.timing_enable(True)
    try:
        _q_dev(vcp_ctx, flat, group, K, Q4)
        assert [nm for nm, _ in vcp_ctx.timing()] == ["cq_group", "cq_select"]
        _mad_dev(vcp_ctx, flat, group, K, 3.0, 0.0)
        t = vcp_ctx.timing()
        assert [nm for nm, _ in t] == ["cq_group", "cq_select", "cq_flag"] and all(ms >= 0 for _, ms in t)
    finally:
        vcp_ctx.timing_enable(False)


def test_on_a_callers_stream():
    """Both device forms under the vcp_set_stream contract (the rig of tests/test_stream_gpu.py): the copy of the values
    and the poison over the outputs are still queued behind a filler on the caller's stream when the call is made."""
    import test_stream_gpu as S
    rig = S.Rig()
    try:
        flat, group, K, _ = R.size_class_case(31)
        other = np.random.default_rng(32).normal(-3.0, 2.0, len(flat))
        wq, wm = R.quantiles(other, group, K, Q4), R.mad(other, group, K, 3.0, 0.0)
        assert not R.same_bits(R.quantiles(flat, group, K, Q4)[0], wq[0])
        buf, dB, dg = S.dev(flat), S.dev(other), S.dev(group)
        out = torch.zeros(K * 4, dtype=torch.float64, device="cuda")
        cnt = torch.zeros(K, dtype=torch.int64, device="cuda")
        rig.run(lambda: rig.ctx.cluster_quantiles_dev(buf.data_ptr(), 1, dg.data_ptr(), len(group), K, Q4, out.data_ptr(),
                                                      cnt.data_ptr()), [(buf, dB)], [(out, POISON), (cnt, -7)])
        assert R.same_bits(S.host(out).reshape(K, 4), wq[0]) and R.same_bits(S.host(cnt), wq[1])
        med, mad, thr = (torch.zeros(K, dtype=torch.float64, device="cuda") for _ in range(3))
        rej = torch.zeros(len(group), dtype=torch.uint8, device="cuda")
        kept = torch.zeros(K, dtype=torch.int64, device="cuda")
        buf.copy_(S.dev(flat))
        nr = rig.run(lambda: rig.ctx.cluster_mad_dev(buf.data_ptr(), 1, dg.data_ptr(), len(group), K, 3.0, 0.0,
                                                     med.data_ptr(), mad.data_ptr(), thr.data_ptr(), rej.data_ptr(),
                                                     kept.data_ptr()),
                     [(buf, dB)], [(med, POISON), (mad, POISON), (thr, POISON), (rej, 9), (kept, -7)])
        got = dict(med=S.host(med), mad=S.host(mad), thr=S.host(thr), reject=S.host(rej), kept=S.host(kept), n_rejected=nr)
        assert R.same_mad(got, wm) is None
    finally:
        rig.close()


def test_robust_module_on_tensors(vcp_ctx):
    from vtkcloudpoint_amd import robust
    rng = np.random.default_rng(4)
    n, K = 9000, 40
    xyz = rng.normal(0, 5, (n, 3))
    lab = rng.integers(0, K + 1, n).astype(np.int32)
    lab[lab == 7] = 0                                                    # an empty cluster
    want = np.concatenate([R.quantiles(xyz[:, a], lab, K, [0.5])[0] for a in range(3)], axis=1)
    assert R.same_bits(robust.cluster_medians(xyz, lab, K, vcp_ctx), want)
    txyz, tlab = torch.from_numpy(xyz).cuda(), torch.from_numpy(lab).cuda()
    got = robust.cluster_medians(txyz, tlab, K, vcp_ctx)
    assert got.is_cuda and R.same_bits(got.cpu().numpy(), want)
    o, c = robust.cluster_quantiles(txyz[:, 2], tlab, K, Q4, vcp_ctx)    # a column read in place
    w = R.quantiles(xyz[:, 2], lab, K, Q4)
    assert R.same_bits(o.cpu().numpy(), w[0]) and R.same_bits(c.cpu().numpy(), w[1])
    m = robust.cluster_mad(txyz[:, 0], tlab, K, 2.5, 0.01, vcp_ctx)
    assert R.same_mad({k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in m.items()},
                      R.mad(xyz[:, 0], lab, K, 2.5, 0.01)) is None
    assert R.same_mad(robust.cluster_mad(xyz[:, 0], lab, K, 2.5, 0.01, vcp_ctx), R.mad(xyz[:, 0], lab, K, 2.5, 0.01)) is None


# ---- errors ---------------------------------------------------------------------------------------------------------------
ARG, INDEX, TOO_LARGE, UNSUPPORTED = -1, -4, -5, -8


def test_errors_leave_the_outputs_untouched(vcp_ctx):
    lib, P, h = N.lib(), N._ptr, vcp_ctx._h
    n, K = 6, 2
    v = np.arange(6.0)
    g = np.array([1, 2, 1, 2, 0, 1], np.int32)
    q2 = np.array([0.0, 1.0])
    nan, big = float("nan"), 1 << 31

    def host_q(values=v, stride=1, group=g, n=n, K=K, q=q2, nq=2, out=True, cnt=True):
        o, c = np.full(8, POISON), np.full(4, -7, np.int64)
        rc = lib.vcp_cluster_quantiles(h, P(values), C.c_int64(stride), P(group), C.c_int64(n), C.c_int32(K), P(q),
                                       C.c_int32(nq), P(o) if out else None, P(c) if cnt else None)
        assert np.all(o == POISON) and np.all(c == -7), "outputs touched"
        return rc

    def host_mad(values=v, stride=1, group=g, n=n, K=K, c_mad=3.0, floor=0.0, null=None):
        bufs = dict(med=np.full(4, POISON), mad=np.full(4, POISON), thr=np.full(4, POISON), rej=np.full(8, 9, np.uint8),
                    kept=np.full(4, -7, np.int64))
        nr = C.c_int64(-7)
        a = {k: (None if k == null else P(b)) for k, b in bufs.items()}
        rc = lib.vcp_cluster_mad(h, P(values), C.c_int64(stride), P(group), C.c_int64(n), C.c_int32(K), C.c_double(c_mad),
                                 C.c_double(floor), a["med"], a["mad"], a["thr"], a["rej"], a["kept"],
                                 None if null == "nr" else C.byref(nr))
        assert all(np.all(b == (9 if k == "rej" else -7 if k == "kept" else POISON)) for k, b in bufs.items())
        assert nr.value == -7, "outputs touched"
        return rc

    for kw, code in ((dict(values=None), ARG), (dict(group=None), ARG), (dict(q=None), ARG), (dict(out=False), ARG),
                     (dict(n=-1), ARG), (dict(K=-1), ARG), (dict(stride=0), ARG), (dict(stride=-2), ARG), (dict(nq=0), ARG),
                     (dict(q=np.array([0.5, nan])), ARG), (dict(q=np.array([-0.1, 0.5])), ARG),
                     (dict(q=np.array([0.5, 1.0000001])), ARG), (dict(q=np.full(17, 0.5), nq=17), UNSUPPORTED),
                     (dict(n=big), TOO_LARGE), (dict(group=np.array([1, 2, 1, 2, 0, 3], np.int32)), INDEX),
                     (dict(group=np.array([1, 2, 1, 2, 0, -1], np.int32)), INDEX)):
        assert host_q(**kw) == code, kw
    for kw, code in ((dict(values=None), ARG), (dict(group=None), ARG), (dict(n=-1), ARG), (dict(K=-1), ARG),
                     (dict(stride=0), ARG), (dict(c_mad=nan), ARG), (dict(c_mad=-1.0), ARG), (dict(floor=nan), ARG),
                     (dict(floor=-1e-9), ARG), (dict(null="med"), ARG), (dict(null="mad"), ARG), (dict(null="thr"), ARG),
                     (dict(null="rej"), ARG), (dict(null="kept"), ARG), (dict(null="nr"), ARG), (dict(n=big), TOO_LARGE),
                     (dict(group=np.array([1, 2, 1, 2, 0, 3], np.int32)), INDEX),
                     (dict(group=np.array([1, 2, 1, 2, 0, -5], np.int32)), INDEX)):
        assert host_mad(**kw) == code, kw
    assert "outside 0..K" in (lib.vcp_last_error(h) or b"").decode()
    # the device forms: a bad label in the last row, found before any output is touched; and an argument error
    dv = torch.from_numpy(v).cuda()
    for gbad in ([1, 2, 1, 2, 0, 3], [1, 2, 1, 2, 0, -1]):
        dg = torch.tensor(gbad, dtype=torch.int32, device="cuda")
        out = torch.full((4,), POISON, dtype=torch.float64, device="cuda")
        cnt = torch.full((2,), -7, dtype=torch.int64, device="cuda")
        med, mad, thr = (torch.full((2,), POISON, dtype=torch.float64, device="cuda") for _ in range(3))
        rej = torch.full((6,), 9, dtype=torch.uint8, device="cuda")
        kept = torch.full((2,), -7, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        with pytest.raises(N.VcpError) as e:
            vcp_ctx.cluster_quantiles_dev(dv.data_ptr(), 1, dg.data_ptr(), n, K, q2, out.data_ptr(), cnt.data_ptr())
        assert e.value.code == INDEX
        with pytest.raises(N.VcpError) as e:
            vcp_ctx.cluster_mad_dev(dv.data_ptr(), 1, dg.data_ptr(), n, K, 3.0, 0.0, med.data_ptr(), mad.data_ptr(),
                                    thr.data_ptr(), rej.data_ptr(), kept.data_ptr())
        assert e.value.code == INDEX
        with pytest.raises(N.VcpError) as e:
            vcp_ctx.cluster_quantiles_dev(dv.data_ptr(), 1, dg.data_ptr(), n, K, [0.5, 2.0], out.data_ptr(), cnt.data_ptr())
        assert e.value.code == ARG
        with pytest.raises(N.VcpError) as e:
            vcp_ctx.cluster_mad_dev(dv.data_ptr(), 1, dg.data_ptr(), n, K, nan, 0.0, med.data_ptr(), mad.data_ptr(),
                                    thr.data_ptr(), rej.data_ptr(), kept.data_ptr())
        assert e.value.code == ARG
        torch.cuda.synchronize()
        assert torch.all(out == POISON) and torch.all(cnt == -7) and torch.all(rej == 9) and torch.all(kept == -7)
        assert all(torch.all(t == POISON) for t in (med, mad, thr))
    # the context still answers
    o, c = vcp_ctx.cluster_quantiles(v, g, K, q2)
    assert o.tolist() == [[0.0, 5.0], [1.0, 3.0]] and c.tolist() == [3, 2]


# ---- the fixed-point workflow ---------------------------------------------------------------------------------------------
def test_robust_fixed_centroids(vcp_ctx, tmp_path):
    """Three small files of one fixed target each, at different ranges, with far rows and repeated rows: the centroids are
    vcp_centroids_weighted's on the rows the restatement keeps."""
    from vtkcloudpoint_amd import io, robust
    rng = np.random.default_rng(8)
    files = []
    for k, rng_m in enumerate((8.0, 35.0, 120.0)):
        m = 120 + 17 * k
        rows = np.c_[rng.normal(10 + k, 0.01, m), rng.normal(-5 + k, 0.01, m), rng.normal(rng_m, 0.004, m)]
        rows[rng.choice(m, 6, replace=False), 2] += rng.choice([-1.0, 1.0], 6) * rng.uniform(2.0, 6.0, 6)
        rows = np.round(rows, 4)
        rows = np.r_[rows, rows[:9]]                                     # repeated rows: ptsCount 2
        p = tmp_path / ("fixed%d.txt" % k)
        p.write_text("".join("%.4f\t%.4f\t%.4f\n" % tuple(r) for r in rows))
        files.append(str(p))
    for ignore in (False, True):
        fixed = io.add_fixed_folder(files, 1.5, -0.5, typpe=3, ctx=vcp_ctx)
        clus = fixed[0]
        pts = [p for ob in clus for p in ob.li]
        dist = np.array([p.Distance for p in pts])
        group = np.array([p.pathId + 1 for p in pts], np.int32)
        want = R.mad(dist, group, 3, 3.0, 0.002)
        assert 18 <= want["n_rejected"] < len(pts) // 3 and max(p.ptsCount for p in pts) == 2
        c3, inside, mad = robust.robust_fixed_centroids(fixed, 3.0, 0.002, ignore, ctx=vcp_ctx)
        assert R.same_mad(mad, want) is None
        keep = want["reject"] == 0
        xyz = np.array([(p.X, p.Y, p.Z) for p in pts])
        w3, wi = vcp_ctx.centroids_weighted(xyz[keep], group[keep], np.array([p.clusterId for p in pts], np.int32)[keep],
                                            np.array([p.ptsCount for p in pts], np.int32)[keep], 3, ignore)
        # the kept rows are the same set in the same order, so the reduction tree is the same: equal bits
        assert R.same_bits(c3, w3) and np.array_equal(inside, wi)
        assert [p.isFilterByDistance for p in pts] == (want["reject"] != 0).tolist()
        naive, _ = vcp_ctx.centroids_weighted(xyz, group, None, np.array([p.ptsCount for p in pts], np.int32), 3, ignore)
        assert np.abs(naive - c3).max() > 1e-3                           # the far rows did pull the plain centroid
