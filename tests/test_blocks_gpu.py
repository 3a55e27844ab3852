"""GPU parity for the block-partitioned pipeline (getClusterFromMotor + StartCode + CompleteWork3,
FrmMain.cs:1214-1291, :2782-2794, :1442-1520) through the C-ABI vs the CPU oracle: bit-exact labels,
block assignment, clusForMerge order and counters -- including the reference's demotion quirks."""
import numpy as np
import pytest

from vtkcloudpoint_amd import _native as N
from vtkcloudpoint_amd import synth

pytestmark = pytest.mark.gpu
KEYS = ("labels", "block_of", "order", "rows", "cols", "kept", "del_sum", "cluster_amount", "evals")


def _same(g, o, what):
    for k in KEYS:
        if isinstance(o[k], np.ndarray):
            assert np.array_equal(g[k], o[k]), "%s: %s" % (what, k)
        else:
            assert g[k] == o[k], "%s: %s %r != %r" % (what, k, g[k], o[k])


def test_random_small_incl_demotion_quirks(vcp_ctx, oracle):
    rng = np.random.default_rng(1)
    n_err = n_del = 0
    for trial in range(300):
        n = int(rng.integers(5, 400))
        motor = (rng.integers(0, 40, size=(n, 2)).astype(np.float64) * 0.25 if trial % 2
                 else rng.random((n, 2)) * 10)
        eps = float(rng.choice([0.25, 0.5, 0.75]))
        mp = int(rng.integers(1, 6))
        pic = int(rng.integers(3, 60))
        try:
            o = oracle.block_pipeline(motor, eps, mp, pic, 3)
        except oracle.OracleError as e:
            n_err += 1
            with pytest.raises(N.VcpError) as ge:
                vcp_ctx.dbscan_blocks(motor, eps, mp, pic, 3)
            assert ge.value.code == e.code, "trial %d error code" % trial
            continue
        g = vcp_ctx.dbscan_blocks(motor, eps, mp, pic, 3)
        _same(g, o, "trial %d" % trial)
        n_del += o["del_sum"] > 0
    assert n_err > 0 and n_del > 0  # the quirk paths were really exercised


def test_reference_defaults_200k_and_1m(vcp_ctx, oracle):
    for n, seed in ((200_000, 9), (1_000_000, 2)):
        d = synth.config_cloud(n, seed=seed)
        # the reference UI defaults: eps 0.07, minPts 7, 200 points per block (Clustering.Designer.cs:86,96,158)
        for eps, mp, pic in ((0.07, 7, 200), (d["eps_l1"], d["min_pts"], 500)):
            o = oracle.block_pipeline(d["motor"], eps, mp, pic, 3)
            g = vcp_ctx.dbscan_blocks(d["motor"], eps, mp, pic, 3)
            _same(g, o, "n=%d eps=%g" % (n, eps))


def test_staged_equals_one_shot(vcp_ctx, oracle):
    import torch
    d = synth.config_cloud(200_000, seed=9)
    eps, mp, pic = 0.1, 10, 200
    ref = vcp_ctx.dbscan_blocks(d["motor"], eps, mp, pic, 3)
    info = vcp_ctx.blocks_begin(d["motor"], eps, mp, pic, 3)
    assert info["rows"] == ref["rows"] and info["cols"] == ref["cols"] and info["m"] == len(ref["order"])
    m, n = info["m"], len(d["motor"])
    local = torch.zeros(m, dtype=torch.int32, device="cuda")
    evals = 0
    world = 3
    covered = 0
    for r in range(world):  # three "ranks" on one GPU: contiguous balanced block ranges
        lo, hi, plo, phi = vcp_ctx.blocks_share(r, world)
        assert plo == covered
        covered = phi
        evals += vcp_ctx.blocks_cluster_dev(lo, hi, local.data_ptr())
    assert covered == m
    labels = torch.zeros(n, dtype=torch.int32, device="cuda")
    block_of = torch.zeros(n, dtype=torch.int32, device="cuda")
    order = torch.zeros(m, dtype=torch.int64, device="cuda")
    out = vcp_ctx.blocks_finish_dev(local.data_ptr(), evals, labels.data_ptr(), block_of.data_ptr(), order.data_ptr())
    assert np.array_equal(labels.cpu().numpy(), ref["labels"])
    assert np.array_equal(block_of.cpu().numpy(), ref["block_of"])
    assert np.array_equal(order.cpu().numpy(), ref["order"])
    assert out["kept"] == ref["kept"] and out["cluster_amount"] == ref["cluster_amount"]
    assert out["evals"] == ref["evals"]


def test_errors(vcp_ctx):
    with pytest.raises(N.VcpError) as e:
        vcp_ctx.dbscan_blocks(np.zeros((0, 2)), 0.1, 3, 10)
    assert e.value.code == -2  # Min() of an empty list
    with pytest.raises(N.VcpError) as e:
        vcp_ctx.dbscan_blocks(np.random.rand(10, 2), 0.1, 3, 0)
    assert e.value.code == -2  # Take(0).Max()
    with pytest.raises(N.VcpError) as e:
        vcp_ctx.dbscan_blocks(np.ones((10, 2)), 0.1, 3, 5)
    assert e.value.code == -3  # zero-extent first block


def test_non_finite_partition_coordinates_then_a_good_call(vcp_ctx, oracle):
    """A NaN / +-inf key or motor coordinate fails with VCP_ERR_ARG after the selection pass (which then runs on the
    bounds of the finite coordinates); the same context then clusters a good cloud exactly."""
    mot = synth.config_cloud(20_000, seed=21)["motor"]
    key = mot[::-1].copy()
    for bad in (np.nan, np.inf, -np.inf):
        k2 = key.copy()
        k2[7, 1] = bad
        with pytest.raises(N.VcpError) as e:
            vcp_ctx.dbscan_blocks(mot, 0.1, 10, 300, 3, key_xy=k2)
        assert e.value.code == -1
        m2 = mot.copy()
        m2[11, 0] = bad
        with pytest.raises(N.VcpError) as e:
            vcp_ctx.dbscan_blocks(m2, 0.1, 10, 300, 3)
        assert e.value.code == -1
    _same(vcp_ctx.dbscan_blocks(mot, 0.1, 10, 300, 3, key_xy=key), oracle.block_pipeline(mot, 0.1, 10, 300, 3, key_xy=key),
          "after the failed calls")


def test_keyed_partition_getClusterFromList(vcp_ctx, oracle):
    """The 3-D twin (FrmMain.cs:1136-1213, Tools.getListByScale BC/Tools.cs:507-509): blocks are cut on (X, Y), every
    DBImproved still clusters on (motor_x, motor_y).  One-shot and staged forms vs the oracle."""
    import torch
    rng = np.random.default_rng(3)
    for trial in range(60):
        n = int(rng.integers(20, 500))
        motor = rng.integers(0, 40, size=(n, 2)).astype(np.float64) * 0.25
        key = rng.random((n, 2)) * 7 if trial % 2 else rng.integers(0, 30, size=(n, 2)).astype(np.float64) * 0.5
        eps, mp, pic = 0.5, int(rng.integers(1, 5)), int(rng.integers(3, 40))
        try:
            o = oracle.block_pipeline(motor, eps, mp, pic, 3, key_xy=key)
        except oracle.OracleError as e:
            with pytest.raises(N.VcpError) as ge:
                vcp_ctx.dbscan_blocks(motor, eps, mp, pic, 3, key_xy=key)
            assert ge.value.code == e.code
            continue
        _same(vcp_ctx.dbscan_blocks(motor, eps, mp, pic, 3, key_xy=key), o, "keyed trial %d" % trial)
    d = synth.config_cloud(300_000, seed=12)
    key = np.ascontiguousarray(d["xyz"][:, :2])
    o = oracle.block_pipeline(d["motor"], 0.07, 7, 200, 3, key_xy=key)
    g = vcp_ctx.dbscan_blocks(d["motor"], 0.07, 7, 200, 3, key_xy=key)
    _same(g, o, "keyed 300k")
    assert not np.array_equal(g["block_of"], vcp_ctx.dbscan_blocks(d["motor"], 0.07, 7, 200, 3)["block_of"])
    # staged, device-resident
    dm, dk = torch.from_numpy(d["motor"]).cuda(), torch.from_numpy(key).cuda()
    info = vcp_ctx.blocks_begin(None, 0.07, 7, 200, 3, device_ptr=dm.data_ptr(), n=len(key), key_device_ptr=dk.data_ptr())
    local = torch.zeros(max(info["m"], 1), dtype=torch.int32, device="cuda")
    lab = torch.zeros(len(key), dtype=torch.int32, device="cuda")
    ev = vcp_ctx.blocks_cluster_dev(0, info["nblocks"], local.data_ptr())
    fin = vcp_ctx.blocks_finish_dev(local.data_ptr(), ev, lab.data_ptr())
    assert np.array_equal(lab.cpu().numpy(), o["labels"]) and fin["cluster_amount"] == o["cluster_amount"]
    assert fin["evals"] == o["evals"]


def test_final_order_counting_sort_equals_library_sort(vcp_ctx, oracle):
    """CompleteWork3's order inside a block (stable by local id) comes from a per-block counting sort; the library
    radix-sort form stays for blocks with more ids than its table holds.  Both against the oracle and each other, on
    blocks of a few points (many empty ones) and of thousands (ptsInCell 5000: dozens of clusters per block)."""
    import os
    rng = np.random.default_rng(55)
    for n, eps, mp, pic in ((30_000, 0.1, 4, 20), (300_000, 0.07, 7, 5000), (200_000, 0.1, 10, 200)):
        d = synth.config_cloud(n, seed=int(rng.integers(1, 99)))
        o = oracle.block_pipeline(d["motor"], eps, mp, pic, 3)
        got = []
        for force in (False, True):
            if force:
                os.environ["VCP_BLOCKS_ORDER_SORT"] = "1"
            try:
                got.append(vcp_ctx.dbscan_blocks(d["motor"], eps, mp, pic, 3))
            finally:
                os.environ.pop("VCP_BLOCKS_ORDER_SORT", None)
        for g in got:
            assert np.array_equal(g["labels"], o["labels"])
            assert np.array_equal(g["order"], o["order"])
            assert g["kept"] == o["kept"] and g["cluster_amount"] == o["cluster_amount"] and g["evals"] == o["evals"]


@pytest.mark.parametrize("devices", [[0], [0, 0], [0, 0, 0]])
def test_blocks_multi_from_one_process_equals_the_single_device_call(vcp_ctx, oracle, devices):
    """vcp_dbscan_blocks_multi: one process drives one context (and one host thread) per listed device -- here the same
    GPU listed one to three times, which exercises the device threads, the range plan and the peer copies of the label
    slices; a box with several GPUs runs the same code with distinct ids (unmeasured on hardware).  Every output equals
    the one-device call and the oracle, also with the partition on separate keys (getClusterFromList)."""
    mc = N.MultiContext(devices)
    assert mc.count() == len(devices)
    d = synth.config_cloud(200_000, seed=21)
    motor = d["motor"]
    key = np.ascontiguousarray(d["xyz"][:, :2])
    for kx in (None, key):
        g1 = vcp_ctx.dbscan_blocks(motor, 0.07, 7, 200, 3, key_xy=kx)
        gm = mc.dbscan_blocks(motor, 0.07, 7, 200, 3, key_xy=kx)
        ob = oracle.block_pipeline(motor, 0.07, 7, 200, 3, key_xy=kx)
        for k in ("labels", "block_of", "order"):
            assert np.array_equal(gm[k], g1[k]), k
            assert np.array_equal(gm[k], ob[k]), k
        for k in ("rows", "cols", "kept", "del_sum", "cluster_amount", "evals"):
            assert gm[k] == g1[k] == ob[k], k
    # error behaviour like the single-device call: an empty list throws in the C# (FrmMain.cs:1224)
    with pytest.raises(N.VcpError) as e:
        mc.dbscan_blocks(np.zeros((0, 2)), 0.07, 7, 200, 3)
    assert e.value.code == -2
    # small lattice clouds: demotions, the clusLen quirk across the devices' shares, the inputs on which the C# throws
    rng = np.random.default_rng(5)
    n_err = n_del = 0
    for trial in range(80):
        n = int(rng.integers(5, 400))
        m2 = (rng.integers(0, 40, size=(n, 2)).astype(np.float64) * 0.25 if trial % 2 else rng.random((n, 2)) * 10)
        eps, mp, pic = float(rng.choice([0.25, 0.5, 0.75])), int(rng.integers(1, 6)), int(rng.integers(3, 60))
        try:
            ob = oracle.block_pipeline(m2, eps, mp, pic, 3)
        except oracle.OracleError as oe:
            n_err += 1
            with pytest.raises(N.VcpError) as ge:
                mc.dbscan_blocks(m2, eps, mp, pic, 3)
            assert ge.value.code == oe.code, "trial %d" % trial
            continue
        gm = mc.dbscan_blocks(m2, eps, mp, pic, 3)
        _same(gm, ob, "multi trial %d" % trial)
        n_del += ob["del_sum"] > 0
    assert (n_err > 0 and n_del > 0) or len(devices) == 1
    mc.close()


# ---- the sort-free partition (csrc/blockpart.hip): the paths the benchmark clouds do not reach -----------------------
def _check(vcp_ctx, oracle, motor, eps, mp, pic, what):
    motor = np.ascontiguousarray(motor, dtype=np.float64)
    o = oracle.block_pipeline(motor, eps, mp, pic, 3)
    g = vcp_ctx.dbscan_blocks(motor, eps, mp, pic, 3)
    _same(g, o, what)
    return o


def test_select_needs_many_passes(vcp_ctx, oracle):
    """Radix select of the first block when the first digit (exponent of d) does not isolate it: an outlier at the minimum
    corner puts every d into one octave; thousands of points share one d exactly (ties go by index through the index
    digits, more keys than the single-workgroup end of the selection takes)."""
    rng = np.random.default_rng(11)
    n = 300_000
    # everybody at x = 5 + tiny lattice noise, y below x: d = x - x_Min is one of a few values; the corner point fixes x_Min, y_Min
    motor = np.empty((n, 2))
    motor[:, 0] = 5.0 + rng.integers(0, 3, n) * 2.0 ** -10
    motor[:, 1] = rng.random(n) * 4.0
    motor[0] = (0.0, 0.0)
    for pic in (7, 2000, 150_000):
        _check(vcp_ctx, oracle, motor, 0.01, 5, pic, "one octave, pic %d" % pic)
    # far outlier: all d within a relative 1e-6 of each other
    motor2 = rng.random((100_000, 2)) * 10.0
    motor2[17] = (-1.0e7, -1.0e7)
    _check(vcp_ctx, oracle, motor2, 0.05, 4, 50, "far outlier at the minimum corner")


def test_large_blocks_ties_and_general_kernel(vcp_ctx, oracle):
    """Blocks of 10^4..10^5 points: cut into sub-ranges of d; a sub-range that comes out large (thousands of equal d) and a
    block whose points ALL share one d (ordered by index) take the general kernel."""
    rng = np.random.default_rng(12)
    bg = rng.random((20_000, 2)) * 100.0                       # sparse background: decides the block size (large blocks)
    blob = 50.0 + rng.normal(0.0, 0.4, size=(150_000, 2))      # one heart of 150 k points inside a block or two
    ties = np.column_stack([np.full(6_000, 70.0), 20.0 + rng.random(6_000) * 3.0])   # 6 k points with one d exactly
    line = np.column_stack([np.full(4_000, 90.0), 10.0 + np.arange(4_000) * 1e-4])   # a block that holds nothing else
    motor = np.concatenate([bg, blob, ties, line])
    motor = motor[rng.permutation(len(motor))]
    motor[0] = (0.0, 0.0)
    o = _check(vcp_ctx, oracle, motor, 0.02, 6, 300, "hearts, ties, one-d block")
    counts = np.bincount(o["block_of"][o["block_of"] >= 0])
    assert counts.max() > 30_000 and (counts > 1024).sum() >= 3


def test_millions_of_blocks(vcp_ctx, oracle):
    """A tiny first block makes millions of (mostly empty) blocks: super-buckets of more than 512 blocks (the split pass does
    not track the range of d per block there: large blocks go to the general kernel)."""
    rng = np.random.default_rng(13)
    n = 120_000
    motor = rng.random((n, 2)) * 10.0
    motor[:4] = np.array([[0.0, 0.0], [0.004, 0.001], [0.002, 0.004], [0.003, 0.003]])  # first block: 0.004 x 0.004
    dense = 5.0 + rng.random((3_000, 2)) * 0.003   # 3 000 points inside ONE tiny block
    motor = np.concatenate([motor, dense])
    o = _check(vcp_ctx, oracle, motor, 0.05, 4, 4, "tiny first block")
    assert o["rows"] * o["cols"] > 4_500_000


def test_small_blocks_all_pairs_kernel(vcp_ctx, oracle):
    """Blocks of up to 1024 points are clustered by the all-pairs kernel (blocks.hip: k_block_brute) with a candidate window
    from the in-block order of d: both size classes (<= 256, <= 1024 points), blocks with several clusters, border points
    between two clusters, pairs at distance exactly eps (lattice coordinates), duplicates (equal d), large coordinate offsets
    (the window's rounding slack), minPts 1 (every point core) and a minPts nobody reaches."""
    rng = np.random.default_rng(21)
    seen_mid = seen_clusters = 0
    for trial in range(40):
        nblob = int(rng.integers(5, 60))
        cen = rng.random((nblob, 2)) * 30.0
        pts = [cen[i] + rng.normal(0.0, 0.15, size=(int(rng.integers(5, 60)), 2)) for i in range(nblob)]
        pts.append(rng.random((int(rng.integers(200, 1500)), 2)) * 30.0)
        motor = np.concatenate(pts)
        if trial % 3 == 0:
            motor = np.round(motor * 4.0) / 4.0          # lattice: ties at exactly eps, duplicates
        if trial % 5 == 1:
            motor += np.array([3.0e8, -7.0e8])           # large offsets: coarse spacing of the doubles
        if trial % 7 == 2:
            motor = np.concatenate([motor, np.repeat(motor[:40], 6, axis=0)])   # heaps of identical points
        motor = motor[rng.permutation(len(motor))]
        eps = float(rng.choice([0.25, 0.3, 0.5]))
        mp = int(rng.choice([1, 3, 4, 6, 2000]))
        pic = int(rng.choice([100, 250, 300, 600, 1000]))
        try:
            o = _check(vcp_ctx, oracle, motor, eps, mp, pic, "all-pairs trial %d" % trial)
        except oracle.OracleError as e:   # the reference's index -1 while demoting the first cluster (FrmMain.cs:1487)
            with pytest.raises(N.VcpError) as ge:
                vcp_ctx.dbscan_blocks(np.ascontiguousarray(motor), eps, mp, pic, 3)
            assert ge.value.code == e.code
            continue
        counts = np.bincount(o["block_of"][o["block_of"] >= 0])
        seen_mid += int(((counts > 256) & (counts <= 1024)).any())
        seen_clusters += int(o["kept"] > 3)
    assert seen_mid > 5 and seen_clusters > 10


def test_tens_of_millions_of_blocks(vcp_ctx, oracle):
    """More than 2^25 blocks (a first block of 0.1 x 0.024 units on a 300 x 300 cloud): a launch of one workgroup per block
    would hold more than 2^32 threads -- the per-block kernels walk the blocks with a capped grid.  (Found by the fuzz sweep,
    seed 41: the wrapped launch left most blocks unclustered.)"""
    rng = np.random.default_rng(14)
    n = 60_000
    motor = np.round(rng.random((n, 2)) * 300.0 * 1024) / 1024
    motor[motor[:, 0] < 1.0, 0] += 1.0      # keep the band along both minimum edges clear ...
    motor[motor[:, 1] < 1.0, 1] += 1.0
    motor[0] = (0.0, 150.0)                 # ... so that x_Min, y_Min come from two different points
    motor[1] = (150.0, 0.0)
    motor[2] = (0.1, 0.0234375)             # the point of smallest d: the first block, 0.1 x 0.0234375
    o = _check(vcp_ctx, oracle, motor, 1.2, 7, 1, "37 M blocks")
    assert o["rows"] * o["cols"] > 35_000_000
