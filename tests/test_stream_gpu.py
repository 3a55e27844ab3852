"""vcp_set_stream: every _dev entry point (and one host-buffer call) on a caller's non-blocking stream.

include/vcp.h promises that a call runs on the stream the context was given and returns when its work there is done.
A launch, copy, memset or event that went to the context's own stream instead would pass every other test, which
synchronise the device before each call.  Here it gives a wrong answer:

  1. the input buffers hold cloud A (copied and synchronised);
  2. on the caller's stream s: a filler kernel that spins for FILL_MS, then the copy of cloud B over the inputs and a
     poison value over the outputs;
  3. `not s.query()`: the filler is still running, the buffers still hold A;
  4. the entry point is called at once;
  5. on return `s.query()` is true: the call blocked until its work on s was done;
  6. the outputs are the reference's answer for B, where the references give different answers for A and for B.
A kernel on another stream reads A (or has its output overwritten by the poison that is queued behind the filler).

Measured on an MI355X (test_figures_for_the_docstring prints them): the filler runs 56.2 ms on s (60 asked for, 2.25 M
clock ticks per ms); the host needs 0.40 ms to queue it with the copy and the poison, so `not s.query()` holds with a
margin of two orders of magnitude; the largest call (dbscan_dev, 12 000 points) takes 0.31 ms on the context's own
stream.  With the search launch of csrc/kdist.hip sent to the own stream, test_kdist_dev fails: the output is the poison."""
import time

import numpy as np
import pytest
import torch

import centroid_ref
import cpp_mirror_cases as C
import eps_tree_ref
import gdbscan_ref
import kdist_ref
import match_unique_ref
import register_ref
import register_sim_ref
import shapes_ref
from vtkcloudpoint_amd import _native as N

pytestmark = pytest.mark.gpu

FILL_MS = 60.0


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.cpu().numpy()


class Rig:
    """A context of its own on a non-blocking stream of the caller's."""

    def __init__(self):
        self.ctx = N.Context(0)
        self.s = torch.cuda.Stream()
        self.ctx.set_stream(self.s.cuda_stream)
        # the spin kernel counts device clock ticks: find how many make a millisecond
        probe = 50_000_000   # some 20 ms: the launch overhead no longer counts
        self.ticks_per_ms = probe / self.fill_time(probe)
        self.ticks = int(FILL_MS * self.ticks_per_ms)

    def fill_time(self, ticks):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(self.s):
            e0.record()
            torch.cuda._sleep(ticks)
            e1.record()
        self.s.synchronize()
        return e0.elapsed_time(e1)

    def behind_filler(self, swaps=(), poison=()):
        """Queue on s: the filler, then B over the input buffers and the poison over the outputs."""
        torch.cuda.synchronize()
        with torch.cuda.stream(self.s):
            torch.cuda._sleep(self.ticks)
            for buf, b in swaps:
                buf.copy_(b, non_blocking=True)
            for out, v in poison:
                out.fill_(v)

    def run(self, call, swaps=(), poison=()):
        self.behind_filler(swaps, poison)
        assert not self.s.query()          # the filler still runs: nothing behind it has happened
        try:
            r = call()
        except N.VcpError as e:
            if e.code == -7:               # a HIP runtime error: nothing more is started on this device
                pytest.exit("HIP error on the caller's stream: %s" % e, 3)
            raise
        assert self.s.query()              # every call is blocking: its work on s is done
        return r

    def close(self):
        torch.cuda.synchronize()
        self.ctx.close()                   # the context goes before the stream it ran on
        self.s = None


@pytest.fixture(scope="module")
def rig():
    r = Rig()
    yield r
    r.close()


def _dbscan_on_s(rig, oracle, n, seeds, eps=0.25, min_pts=8):
    A, B = (C.lattice_cloud(n, s, blobs=max(2, n // 400), span=(n / 20.0) ** 0.5 + 4.0, sigma=0.3) for s in seeds)
    oA, oB = oracle.dbscan(A, eps, min_pts), oracle.dbscan(B, eps, min_pts)
    assert not np.array_equal(oA["labels"], oB["labels"]) and not np.array_equal(oA["is_key"], oB["is_key"])
    buf, dB = dev(A), dev(B)
    lab, core, cls = (torch.zeros(n, dtype=dt, device="cuda") for dt in (torch.int32, torch.uint8, torch.uint8))
    cf, ev = rig.run(lambda: rig.ctx.dbscan_dev(buf.data_ptr(), n, 2, eps, min_pts, d_labels=lab.data_ptr(),
                                                d_is_core=core.data_ptr(), d_is_classed=cls.data_ptr()),
                     [(buf, dB)], [(lab, -7), (core, 9), (cls, 9)])
    assert np.array_equal(host(lab), oB["labels"]) and (cf, ev) == (oB["cf"], oB["evals"])
    assert np.array_equal(host(core), oB["is_key"]) and np.array_equal(host(cls), oB["classed"])
    return buf, lab, oB


def test_dbscan_dev_and_a_growing_workspace(rig, oracle):
    rig.ctx.release_workspace()
    _dbscan_on_s(rig, oracle, 500, (1, 2))          # a small call first: the next one grows the workspace on s
    _dbscan_on_s(rig, oracle, 12000, (3, 4))


def test_figures_for_the_docstring(rig, oracle):
    """Prints the filler's duration on s, the host's time from queueing it to the call, and the largest call's duration
    on the context's own stream; asserts that the filler outlasts the host's part twentyfold."""
    fill = rig.fill_time(rig.ticks)
    n = 12000
    buf = dev(C.lattice_cloud(n, 3, blobs=30, span=28.5, sigma=0.3))
    lab = torch.zeros(n, dtype=torch.int32, device="cuda")
    t0 = time.perf_counter()
    rig.behind_filler([(buf, buf.clone())], [(lab, -7)])
    gap = (time.perf_counter() - t0) * 1e3
    rig.s.synchronize()
    rig.ctx.set_stream(0)
    try:
        torch.cuda.synchronize()
        rig.ctx.dbscan_dev(buf.data_ptr(), n, 2, 0.25, 8, d_labels=lab.data_ptr())
        t0 = time.perf_counter()
        rig.ctx.dbscan_dev(buf.data_ptr(), n, 2, 0.25, 8, d_labels=lab.data_ptr())
        call = (time.perf_counter() - t0) * 1e3
    finally:
        rig.ctx.set_stream(rig.s.cuda_stream)
    print("\nfiller %.1f ms on s (%.0f ticks per ms), host gap %.3f ms, dbscan_dev(12000) on the own stream %.2f ms"
          % (fill, rig.ticks_per_ms, gap, call))
    assert fill > 0.5 * FILL_MS and fill > 20.0 * gap


def test_gdbscan_dev(rig):
    n = 2000
    A, B = C.lattice_cloud(n, 5), C.lattice_cloud(n, 6)
    rng = np.random.default_rng(7)
    w = rng.integers(1, 6, n).astype(np.int32)
    aux = np.round(rng.uniform(5.0, 8.0, n) * 4) / 4
    rA, rB = (gdbscan_ref.gdbscan(c, 0.25, 16, N.L1_2D, w, aux, 0.5, 3) for c in (A, B))
    assert gdbscan_ref.same(rA, rB) is not None
    buf, dB, dw, da = dev(A), dev(B), dev(w), dev(aux)
    lab, core, ws = (torch.zeros(n, dtype=dt, device="cuda") for dt in (torch.int32, torch.uint8, torch.int64))
    cf = rig.run(lambda: rig.ctx.gdbscan_dev(buf.data_ptr(), n, 2, 0.25, 16, lab.data_ptr(), d_weights=dw.data_ptr(),
                                             d_aux=da.data_ptr(), gate=0.5, cf_in=3, d_is_core=core.data_ptr(),
                                             d_wsum=ws.data_ptr()),
                 [(buf, dB)], [(lab, -7), (core, 9), (ws, -7)])
    assert gdbscan_ref.same(dict(labels=host(lab), is_core=host(core), cf=cf, wsum=host(ws)), rB) is None


def test_kdist_dev(rig):
    n, k = 2500, 8
    A, B = C.lattice_cloud(n, 8), C.lattice_cloud(n, 9)
    (kA, _), (kB, nnB) = (kdist_ref.brute_rows(c, k, N.L1_2D, np.arange(n)) for c in (A, B))
    assert not np.array_equal(kA, kB)
    buf, dB = dev(A), dev(B)
    kd, knn = torch.zeros(n, dtype=torch.float64, device="cuda"), torch.zeros((n, k), dtype=torch.int32, device="cuda")
    rig.run(lambda: rig.ctx.kdist_dev(buf.data_ptr(), n, 2, k, kd.data_ptr(), knn.data_ptr()), [(buf, dB)],
            [(kd, -7.0), (knn, -7)])
    assert C.same(host(kd), kB) and np.array_equal(host(knn), nnB)


def test_eps_tree_dev(rig):
    n, k, eps_max = 1500, 5, 0.5
    A, B = C.lattice_cloud(n, 10), C.lattice_cloud(n, 11)
    rA, rB = (eps_tree_ref.eps_tree(c, k, eps_max, N.L1_2D) for c in (A, B))
    assert eps_tree_ref.same(dict(rA, n_merge=rA["n_merge"]), rB) is not None
    buf, dB = dev(A), dev(B)
    kd, re, w = (torch.zeros(n, dtype=torch.float64, device="cuda") for _ in range(3))
    a, b = (torch.zeros(n, dtype=torch.int32, device="cuda") for _ in range(2))
    m, _ = rig.run(lambda: rig.ctx.eps_tree_dev(buf.data_ptr(), n, 2, k, eps_max, w.data_ptr(), a.data_ptr(), b.data_ptr(),
                                                kd.data_ptr(), re.data_ptr()),
                   [(buf, dB)], [(kd, -7.0), (re, -7.0), (w, -7.0), (a, -7), (b, -7)])
    got = dict(kdist=host(kd), reach=host(re), merge_w=host(w)[:m], merge_a=host(a)[:m], merge_b=host(b)[:m], n_merge=m)
    assert eps_tree_ref.same(got, rB) is None, eps_tree_ref.same(got, rB)


def test_centroids_dev(rig):
    n, K = 3000, 7
    xA, mA, lab = C._labelled_cloud(n, K, 12)
    xB, mB, _ = C._labelled_cloud(n, K, 13)
    rA, rB = centroid_ref.tree_centroids(xA, mA, lab, K), centroid_ref.tree_centroids(xB, mB, lab, K)
    assert not C.same(rA[0], rB[0]) and not C.same(rA[1], rB[1]) and (rB[2] > 0).all()
    bx, bm, dxB, dmB, dl = dev(xA), dev(mA), dev(xB), dev(mB), dev(lab)
    c3, c2 = (torch.zeros((K, w), dtype=torch.float64, device="cuda") for w in (3, 2))
    cnt = torch.zeros(K, dtype=torch.int64, device="cuda")
    rig.run(lambda: rig.ctx.centroids_dev(bx.data_ptr(), bm.data_ptr(), dl.data_ptr(), n, K, c3.data_ptr(), c2.data_ptr(),
                                          cnt.data_ptr()),
            [(bx, dxB), (bm, dmB)], [(c3, -7.0), (c2, -7.0), (cnt, -7)])
    assert C.same(host(c3), rB[0]) and C.same(host(c2), rB[1]) and np.array_equal(host(cnt), rB[2])


def test_icp_dev(rig, oracle):
    from vtkcloudpoint_amd import synth
    a = synth.config_icp(nd=5000, nm=100, jitter=0.02)
    b = synth.config_icp(nd=5000, nm=100, jitter=0.02, deg=-4.0, shift=(-0.2, 0.1, 0.3))
    oA, oB = (oracle.icp(a["model"], d["data"], 1e-4, 100, 0) for d in (a, b))
    assert np.abs(oA["R"] - oB["R"]).max() > 1e-2 and np.abs(oA["T"] - oB["T"]).max() > 1e-2
    dm, buf, dB = dev(a["model"]), dev(a["data"]), dev(b["data"])
    g = rig.run(lambda: rig.ctx.icp_dev(dm.data_ptr(), 100, buf.data_ptr(), 5000, 1e-4, 100, 0), [(buf, dB)])
    assert g["iters"] == oB["iters"]
    assert np.abs(g["R"] - oB["R"]).max() < C.ICP_TOL and np.abs(g["T"] - oB["T"]).max() < C.ICP_TOL   # test_icp_gpu.py's


def test_match_unique_dev(rig):
    cases = C.match_cases(True)[0].inputs
    cB, truths, M = cases["centers.tmp"].reshape(-1, 3), cases["truths"].reshape(-1, 3), cases["M"]
    cA = cB[::-1].copy()
    K, T = len(cB), len(truths)
    rA, rB = (match_unique_ref.greedy_matching(c, truths, M, 0.25) for c in (cA, cB))
    assert not np.array_equal(rA["truth_of"], rB["truth_of"]) and rB["count"] > 100
    buf, dB, dt = dev(cA), dev(cB), dev(truths)
    to, co = torch.zeros(K, dtype=torch.int32, device="cuda"), torch.zeros(T, dtype=torch.int32, device="cuda")
    pd, mx = torch.zeros(K, dtype=torch.float64, device="cuda"), torch.zeros((K, 3), dtype=torch.float64, device="cuda")
    g = rig.run(lambda: rig.ctx.match_unique_dev(buf.data_ptr(), K, dt.data_ptr(), T, M, 0.25, to.data_ptr(), co.data_ptr(),
                                                 pd.data_ptr(), mx.data_ptr()),
                [(buf, dB)], [(to, -7), (co, -7), (pd, -7.0), (mx, -7.0)])
    assert g["count"] == rB["count"] and np.array_equal(host(to), rB["truth_of"]) and np.array_equal(host(co), rB["center_of"])
    assert C.same(host(pd), rB["pair_dist"]) and C.same(host(mx), rB["matched_xyz"])


def _shape_ref(oracle, xy, lab, K):
    circ = oracle.get_circles(xy, lab, K)
    rect = []
    for idx in shapes_ref.members(lab, K):
        f = oracle.min_circle_ex(xy[idx])
        rect.append(shapes_ref.rectangle(f["hull"], xy[idx] if f["inserted"] else None))
    return circ, rect


def test_cluster_shapes_dev(rig, oracle):
    n, K = 3000, 12
    rng = np.random.default_rng(14)
    lab = rng.integers(0, K + 1, n).astype(np.int32)
    A, B = (np.round(np.random.default_rng(s).normal(0, 2.0, (n, 2)) * 64) / 64 + 10.0 * lab[:, None] for s in (15, 16))
    (cA, _), (cB, rectB) = _shape_ref(oracle, A, lab, K), _shape_ref(oracle, B, lab, K)
    assert not C.same(cA["radius"], cB["radius"]) and cB["valid"].all()
    buf, dB, dl = dev(A), dev(B), dev(lab)
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device="cuda")
    o = dict(centers=z((K, 2), torch.float64), radius=z(K, torch.float64), valid=z(K, torch.uint8), hull_n=z(K, torch.int32),
             rect_xy=z((K, 4, 2), torch.float64), rect_len=z((K, 2), torch.float64), rect_edge=z(K, torch.int32),
             rect_valid=z(K, torch.uint8), hull_off=z(K + 1, torch.int32), hull_idx=z(n, torch.int32))
    p = {k: v.data_ptr() for k, v in o.items()}
    rig.run(lambda: rig.ctx.cluster_shapes_dev(buf.data_ptr(), dl.data_ptr(), None, n, n, K, p["centers"], p["radius"],
                                               p["valid"], p["hull_n"], p["rect_xy"], p["rect_len"], p["rect_edge"],
                                               p["rect_valid"], p["hull_off"], p["hull_idx"]),
            [(buf, dB)], [(v, 9 if v.dtype == torch.uint8 else -7) for v in o.values()])
    g = {k: host(v) for k, v in o.items()}
    for k in ("centers", "radius", "valid", "hull_n"):                      # test_shapes_gpu.py: the oracle's, bit for bit
        assert C.same(g[k], cB[k]), k
    for k, r in enumerate(rectB):
        assert g["rect_valid"][k] == r["valid"] == 1 and g["rect_edge"][k] == r["edge"]
        assert C.same(g["rect_len"][k], r["len"]) and C.same(g["rect_xy"][k], r["xy"])
    assert g["hull_off"][0] == 0 and np.array_equal(np.diff(g["hull_off"]), cB["hull_n"])


def test_cluster_filter_dev(rig):
    n, K = 20000, 40
    rng = np.random.default_rng(17)
    lA, lB = (rng.integers(0, K + 1, n).astype(np.int32) for _ in range(2))
    rad, val = np.round(rng.uniform(0, 4, K) * 4) / 4, (rng.random(K) < 0.8).astype(np.uint8)
    rl, rv = np.round(rng.uniform(0.25, 4, (K, 2)) * 4) / 4, (rng.random(K) < 0.8).astype(np.uint8)
    rA, rB = (shapes_ref.cluster_filter(l, K, rad, val, rl, rv, 2.0, 3.0) for l in (lA, lB))
    assert not np.array_equal(rA["keep"], rB["keep"]) and 0 < rB["n_filtered"] < K
    buf, dB, d_rad, d_val, d_rl, d_rv = dev(lA), dev(lB), dev(rad), dev(val), dev(rl), dev(rv)
    f, keep, idx = torch.zeros(K, dtype=torch.uint8, device="cuda"), torch.zeros(n, dtype=torch.uint8, device="cuda"), \
        torch.zeros(n, dtype=torch.int32, device="cuda")
    nf, nk = rig.run(lambda: rig.ctx.cluster_filter_dev(buf.data_ptr(), n, K, d_rad.data_ptr(), d_val.data_ptr(), d_rl.data_ptr(),
                                                        d_rv.data_ptr(), 2.0, 3.0, f.data_ptr(), keep.data_ptr(), idx.data_ptr()),
                     [(buf, dB)], [(f, 9), (keep, 9), (idx, -7)])
    assert (nf, nk) == (rB["n_filtered"], rB["n_kept"]) and np.array_equal(host(f), rB["filtered"])
    assert np.array_equal(host(keep), rB["keep"]) and np.array_equal(host(idx)[:nk], rB["kept_idx"])


def _register_on_s(rig, sim, sc, bases, refB, refA_fn):
    src, tgt = sc["source"], sc["truths"]
    srcA = np.zeros_like(src)                                   # every base has length zero: no hypothesis
    refA = refA_fn(srcA)
    assert refA["best"] == -1 and refB["best"] >= 0
    ns, nt, nb = len(src), len(tgt), len(bases)
    buf, dB, dt, db = dev(srcA), dev(src), dev(tgt), dev(np.asarray(bases, np.int32))
    z = lambda shape, dtp: torch.zeros(shape, dtype=dtp, device="cuda")
    o = dict(M_all=z((nb, 4, 4), torch.float64), score=z(nb, torch.int32), inliers=z(nb, torch.int32), pick=z((nb, 3), torch.int32),
             n_hyp=z(nb, torch.int64))
    if sim:
        o["scale"] = z(nb, torch.float64)
    p = {k: v.data_ptr() for k, v in o.items()}
    if sim:
        lo, hi = register_sim_ref.RANGE
        call = lambda: rig.ctx.register_sim_dev(buf.data_ptr(), ns, dt.data_ptr(), nt, db.data_ptr(), nb, lo, hi, register_ref.INLIER,
                                                d_M_all=p["M_all"], d_score=p["score"], d_inliers=p["inliers"], d_pick=p["pick"],
                                                d_n_hyp=p["n_hyp"], d_scale=p["scale"])
    else:
        call = lambda: rig.ctx.register_pairs_dev(buf.data_ptr(), ns, dt.data_ptr(), nt, db.data_ptr(), nb, register_ref.LEN_TOL,
                                                  register_ref.INLIER, d_M_all=p["M_all"], d_score=p["score"],
                                                  d_inliers=p["inliers"], d_pick=p["pick"], d_n_hyp=p["n_hyp"])
    g = rig.run(call, [(buf, dB)], [(v, -7) for v in o.values()])
    g.update({k: host(v) for k, v in o.items()})
    (register_sim_ref.same if sim else register_ref.same)(g, refB)


def test_register_pairs_dev(rig):
    sc, bases, ref = register_ref.scene_case("half")
    _register_on_s(rig, False, sc, bases, ref,
                   lambda a: register_ref.register(a, sc["truths"], bases, register_ref.LEN_TOL, register_ref.INLIER))


def test_register_sim_dev(rig):
    sc, bases = register_sim_ref.scaled_scene("half")
    lo, hi = register_sim_ref.RANGE
    _register_on_s(rig, True, sc, bases, register_sim_ref.golden("half"),
                   lambda a: register_sim_ref.register(a, sc["truths"], bases, lo, hi, register_ref.INLIER))


def test_selftest_scan_dev(rig):
    n = 20000
    rng = np.random.default_rng(18)
    A, B = (rng.integers(0, 1000, n).astype(np.int32) for _ in range(2))
    want = np.concatenate([[0], np.cumsum(B, dtype=np.int64)[:-1]])
    assert int(A.sum()) != int(B.sum())
    buf, dB, out = dev(A), dev(B), torch.zeros(n, dtype=torch.int32, device="cuda")
    tot = rig.run(lambda: rig.ctx.selftest_scan_dev(buf.data_ptr(), out.data_ptr(), n, 0), [(buf, dB)], [(out, -7)])
    assert tot == int(B.sum()) and np.array_equal(host(out).astype(np.int64), want)


def test_staged_blocks(rig, oracle):
    """blocks_begin on a device pointer, blocks_cluster_dev, blocks_finish_dev: each stage behind a filler of its own.  The
    cloud is swapped in front of begin only (the later stages read it in place); the poison over d_local and over the
    final arrays is queued in front of the stage that writes them."""
    n = 3000
    A = C.lattice_cloud(n, 19, blobs=8, span=10.0, sigma=0.2)
    B = C.lattice_cloud(n, 51, blobs=8, span=10.0, sigma=0.2)
    oA, oB = (oracle.block_pipeline(c, 0.125, 5, 200, 3) for c in (A, B))
    assert not np.array_equal(oA["labels"], oB["labels"]) and oB["cluster_amount"] > 1
    buf, dB = dev(A), dev(B)
    b = rig.run(lambda: rig.ctx.blocks_begin(None, 0.125, 5, 200, 3, device_ptr=buf.data_ptr(), n=n), [(buf, dB)])
    assert (b["rows"], b["cols"]) == (oB["rows"], oB["cols"]) and b["m"] == len(oB["order"])
    lo, hi, plo, phi = rig.ctx.blocks_share(0, 1)
    assert (plo, phi) == (0, b["m"])
    local = torch.zeros(max(b["m"], 1), dtype=torch.int32, device="cuda")
    ev = rig.run(lambda: rig.ctx.blocks_cluster_dev(lo, hi, local.data_ptr()), (), [(local, -5)])
    lab, blk = (torch.zeros(n, dtype=torch.int32, device="cuda") for _ in range(2))
    order = torch.zeros(n, dtype=torch.int64, device="cuda")
    f = rig.run(lambda: rig.ctx.blocks_finish_dev(local.data_ptr(), ev, lab.data_ptr(), blk.data_ptr(), order.data_ptr()), (),
                [(lab, -7), (blk, -7), (order, -7)])
    assert np.array_equal(host(lab), oB["labels"]) and np.array_equal(host(blk), oB["block_of"])
    assert f["m"] == len(oB["order"]) and np.array_equal(host(order)[:f["m"]], oB["order"])
    assert (f["kept"], f["del_sum"], f["cluster_amount"], f["evals"]) == (oB["kept"], oB["del_sum"], oB["cluster_amount"], oB["evals"])


def test_host_buffer_dbscan_blocks_on_the_callers_stream(rig, oracle):
    c = C.lattice_cloud(3000, 20)
    o = oracle.dbscan(c, 0.25, 8)
    g = rig.run(lambda: rig.ctx.dbscan(c, 0.25, 8))
    assert np.array_equal(g["labels"], o["labels"]) and (g["cf"], g["evals"]) == (o["cf"], o["evals"])
    assert np.array_equal(g["is_core"], o["is_key"]) and np.array_equal(g["is_classed"], o["classed"])


def test_timing_on_the_callers_stream(rig, oracle):
    rig.ctx.timing_enable(True)
    try:
        _dbscan_on_s(rig, oracle, 3000, (21, 22))
        phases = rig.ctx.timing()
    finally:
        rig.ctx.timing_enable(False)
    assert len(phases) > 0 and all(name and ms >= 0.0 for name, ms in phases), phases


def test_back_to_the_own_stream(rig, oracle):
    n = 3000
    c = C.lattice_cloud(n, 23)
    o = oracle.dbscan(c, 0.25, 8)
    buf, lab = dev(c), torch.zeros(n, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    rig.ctx.set_stream(0)                       # NULL: the context's own stream
    try:
        rig.behind_filler()                     # s is busy; the own stream is not, and the call does not wait for s
        cf, ev = rig.ctx.dbscan_dev(buf.data_ptr(), n, 2, 0.25, 8, d_labels=lab.data_ptr())
        still_busy = not rig.s.query()
        rig.s.synchronize()
    finally:
        rig.ctx.set_stream(rig.s.cuda_stream)
    assert np.array_equal(host(lab), o["labels"]) and (cf, ev) == (o["cf"], o["evals"])
    assert still_busy
