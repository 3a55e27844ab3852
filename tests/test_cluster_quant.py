"""vcp_cluster_quantiles / vcp_cluster_mad without a GPU: the symbols through every layer, the key and the rank from the
kernels' own source (vcp_selftest_rank_key) against the numpy restatement (tests/cluster_quant_ref.py), the restatement
against np.median and against the per-list max / min that Tools.GetGroupingManOrMin takes, and the calls that need no
device."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import cluster_quant_ref as R
import test_abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEVICE_CALLS = ["vcp_cluster_quantiles", "vcp_cluster_quantiles_dev", "vcp_cluster_mad", "vcp_cluster_mad_dev"]
NAMES = DEVICE_CALLS + ["vcp_selftest_rank_key"]


def test_symbols_in_every_layer():
    from vtkcloudpoint_amd import _native
    lib = _native.lib()
    protos = test_abi._header_prototypes()
    for nm in NAMES:
        assert nm in protos and hasattr(lib, nm) and nm in _native.SYMBOLS, nm
        assert not nm.startswith("vcp_group_")
    q = ["ptr", "ptr", "i64", "ptr", "i64", "i32", "ptr", "i32", "ptr", "ptr"]
    m = ["ptr", "ptr", "i64", "ptr", "i64", "i32", "f64", "f64", "ptr", "ptr", "ptr", "ptr", "ptr", "ptr"]
    assert protos["vcp_cluster_quantiles"] == q and protos["vcp_cluster_quantiles_dev"] == q
    assert protos["vcp_cluster_mad"] == m and protos["vcp_cluster_mad_dev"] == m
    assert protos["vcp_selftest_rank_key"] == ["f64", "f64", "i64", "ptr", "ptr"]
    cs = {name: classes for _, name, classes in test_abi._csharp_imports()}
    for nm in DEVICE_CALLS:
        assert cs.get(nm) == protos[nm], nm
    with open(os.path.join(ROOT, "vtkcloudpoint_amd", "host", "csharp", "MainForm.Gpu.cs")) as f:
        assert re.search(r"public\s+\w+\s+RejectPtsByDistanceRobust\s*\(\s*double\s+c\s*,\s*double\s+floor\s*\)", f.read())
    with open(os.path.join(ROOT, "include", "vcp.h")) as f:
        h = f.read()
    for nm, v in (("VCP_CQ_WAVE_MAX", R.WAVE_MAX), ("VCP_CQ_WG_MAX", R.WG_MAX), ("VCP_CQ_NQ_MAX", R.NQ_MAX)):
        assert re.search(r"^#define %s %d$" % (nm, v), h, flags=re.M), nm
    for meth in ("cluster_quantiles", "cluster_quantiles_dev", "cluster_mad", "cluster_mad_dev"):
        assert callable(getattr(_native.Context, meth))


def test_robust_signatures():
    from vtkcloudpoint_amd import robust

    def sig(f):
        return [(p.name, p.default) for p in inspect.signature(f).parameters.values()]

    E = inspect.Parameter.empty
    assert sig(robust.cluster_quantiles) == [("values", E), ("labels", E), ("K", E), ("q", E), ("ctx", None)]
    assert sig(robust.cluster_medians)[:3] == [("xyz", E), ("labels", E), ("K", E)]
    assert sig(robust.cluster_mad)[:5] == [("values", E), ("labels", E), ("K", E), ("c", 3.0), ("floor", 0.0)]
    assert sig(robust.robust_fixed_centroids)[:4] == [("fixed", E), ("c", 3.0), ("floor", 0.0),
                                                      ("ignore_duplication", False)]


def test_key_from_the_kernels_source():
    """key(v) over +-0, subnormals, +-inf, NaNs with payloads and one-ulp neighbours: the restatement's bits, and their
    unsigned order is the numeric order with -0 before +0 and every NaN last."""
    from vtkcloudpoint_amd import _native
    v = R.hard_values()
    want = R.key(v)
    got = np.array([_native.selftest_rank_key(float(x), 0.5, 3)[0] for x in v], np.uint64)
    assert np.array_equal(got, want)
    assert np.all(got[np.isnan(v)] == R.NAN_KEY) and not np.any(got[~np.isnan(v)] == R.NAN_KEY)
    num = v[~np.isnan(v)]
    order = np.argsort(R.key(num), kind="stable")
    s = num[order]
    assert np.all(s[:-1] <= s[1:])
    z = np.nonzero(s == 0)[0]
    assert len(z) == 2 and np.signbit(s[z[0]]) and not np.signbit(s[z[1]])
    assert np.array_equal(R.bits(R.unkey(R.key(num))), R.bits(num))          # the key gives the bits back
    assert np.all(R.bits(R.unkey(R.key(v[np.isnan(v)]))) == R.NAN_BITS)


def test_rank_from_the_kernels_source():
    from vtkcloudpoint_amd import _native
    qs = [0.0, 0.25, 0.5, 0.75, 1.0, float(np.nextafter(0.5, 0)), float(np.nextafter(1.0, 0))]
    for c in list(range(1, 10)) + [63, 64, 65, 4096, 4097, 2 ** 31 - 1]:
        for q in qs:
            r = _native.selftest_rank_key(1.0, q, c)[1]
            assert r == R.rank(q, c) and 0 <= r <= c - 1, (q, c)
        assert _native.selftest_rank_key(1.0, 0.0, c)[1] == 0 and _native.selftest_rank_key(1.0, 1.0, c)[1] == c - 1
        assert _native.selftest_rank_key(1.0, 0.5, c)[1] == (c - 1) // 2          # the lower median


def test_selftest_argument_errors():
    from vtkcloudpoint_amd import _native
    lib = _native.lib()
    key, rank = C.c_uint64(7), C.c_int64(7)

    def call(v, q, c, k=True, r=True):
        return lib.vcp_selftest_rank_key(C.c_double(v), C.c_double(q), C.c_int64(c), C.byref(key) if k else None,
                                         C.byref(rank) if r else None)

    assert call(1.0, 0.5, 1) == 1 and (key.value, rank.value) == (int(R.key([1.0])[0]), 0)
    key.value, rank.value = 7, 7
    for args in ((1.0, 0.5, 0), (1.0, 0.5, -3), (1.0, float("nan"), 5), (1.0, -1e-300, 5),
                 (1.0, float(np.nextafter(1.0, 2.0)), 5), (1.0, float("inf"), 5)):
        assert call(*args) == -1, args
    assert call(1.0, 0.5, 3, k=False) == -1 and call(1.0, 0.5, 3, r=False) == -1
    assert (key.value, rank.value) == (7, 7)                                   # nothing written on an error
    with pytest.raises(_native.VcpError):
        _native.selftest_rank_key(1.0, 2.0, 5)


def test_restatement_against_numpy_median_and_the_per_list_extremes():
    """Odd-sized groups without NaN: q = 0.5 is np.median.  q = 0 / 1 are the Min / Max of every list, from which
    Tools.GetGroupingManOrMin (Tools.cs:468-497) takes its overall result."""
    rng = np.random.default_rng(3)
    sizes = [1, 3, 5, 63, 65, 4097, 301]
    K = len(sizes)
    group = np.concatenate([np.full(s, k + 1, np.int32) for k, s in enumerate(sizes)] + [np.zeros(50, np.int32)])
    rng.shuffle(group)
    v = np.round(rng.normal(100.0, 30.0, len(group)), 2)
    v[rng.integers(0, len(v), 40)] = -0.0
    out, counts = R.quantiles(v, group, K, [0.0, 0.5, 1.0])
    assert counts.tolist() == sizes
    lists = [[float(x) for x in v[group == k]] for k in range(1, K + 1)]
    for k, li in enumerate(lists):
        assert out[k, 1] == np.median(li)
        assert out[k, 0] == min(li) and out[k, 2] == max(li)                   # li.Min / li.Max of the C#
    result = lists[0][0]                                                       # typpe 1 of the C#: the maximum
    for li in lists:
        result = max(li) if result < max(li) else result
    assert result == out[:, 2].max()
    result = lists[0][0]
    for li in lists:
        result = min(li) if result > min(li) else result
    assert result == out[:, 0].min()
    # strided values and an empty group
    flat = rng.normal(0, 1, 3 * len(v))
    flat[1::3] = v
    o3, c3 = R.quantiles(flat[1:], np.r_[group, np.zeros(0, np.int32)], K + 1, [0.0, 0.5, 1.0], stride=3)
    assert R.same_bits(o3[:K], out) and c3[K] == 0 and np.all(R.bits(o3[K]) == R.NAN_BITS)


def test_restatement_of_the_mad_chain_and_the_scene():
    """The scene of the GPU test: the restatement rejects every planted outlier, keeps what lies within its band, and no
    single band of Distance that keeps every inlier can reject all the planted rows."""
    dist, group, planted, K = R.mad_scene()
    assert len(dist) == 3000 and K == 6 and planted.sum() == 150
    w = R.mad(dist, group, K, 3.0, 0.0)
    assert np.all(w["reject"][planted] == 1)
    for k in range(1, K + 1):
        sel = group == k
        dev = np.abs(dist[sel] - w["med"][k - 1])
        assert w["med"][k - 1] == np.sort(dist[sel])[(sel.sum() - 1) // 2]
        assert w["mad"][k - 1] == np.sort(dev)[(sel.sum() - 1) // 2] and w["thr"][k - 1] == 3.0 * w["mad"][k - 1]
        assert np.array_equal(w["reject"][sel] != 0, ~(dev <= w["thr"][k - 1]))
        assert w["kept"][k - 1] == (dev <= w["thr"][k - 1]).sum() >= 0.85 * sel.sum()
    assert w["n_rejected"] == w["reject"].sum() == 3000 - w["kept"].sum()
    inl = w["reject"] == 0
    lo, hi = dist[inl].min(), dist[inl].max()                  # the tightest single band that keeps every inlier
    assert ((dist[planted] >= lo) & (dist[planted] <= hi)).sum() >= 1
    # the floor, a NaN row, group 0
    d2, g2 = np.r_[dist, np.nan, 1e9], np.r_[group, np.int32(2), np.int32(0)]
    w2 = R.mad(d2, g2, K, 3.0, np.inf)
    assert w2["n_rejected"] == 1 and w2["reject"][-2] == 1 and w2["reject"][-1] == 0 and np.all(np.isinf(w2["thr"]))


def test_null_context_and_no_device():
    import torch
    from vtkcloudpoint_amd import _native, robust
    lib = _native.lib()
    v, g, q = np.array([1.0, 2.0, 3.0]), np.array([1, 1, 1], np.int32), np.array([0.5])
    out, cnt, nr = np.full(1, -7.0), np.full(1, -7, np.int64), C.c_int64(-7)
    med, mad, thr, kept, rej = np.full(1, -7.0), np.full(1, -7.0), np.full(1, -7.0), np.full(1, -7, np.int64), \
        np.full(3, 7, np.uint8)
    P = _native._ptr
    for nm in ("vcp_cluster_quantiles", "vcp_cluster_quantiles_dev"):
        assert getattr(lib, nm)(None, P(v), C.c_int64(1), P(g), C.c_int64(3), 1, P(q), 1, P(out), P(cnt)) == -1, nm
    for nm in ("vcp_cluster_mad", "vcp_cluster_mad_dev"):
        assert getattr(lib, nm)(None, P(v), C.c_int64(1), P(g), C.c_int64(3), 1, C.c_double(3.0), C.c_double(0.0), P(med),
                                P(mad), P(thr), P(rej), P(kept), C.byref(nr)) == -1, nm
    assert out[0] == -7 and cnt[0] == -7 and nr.value == -7 and med[0] == -7 and kept[0] == -7 and rej.tolist() == [7, 7, 7]
    if torch.cuda.is_available():
        o, c = robust.cluster_quantiles(v, g, 1, [0.0, 0.5, 1.0])
        assert o.tolist() == [[1.0, 2.0, 3.0]] and c.tolist() == [3]
    else:
        for call in (lambda: robust.cluster_quantiles(v, g, 1, [0.5]), lambda: robust.cluster_mad(v, g, 1),
                     lambda: robust.cluster_medians(np.zeros((3, 3)), g, 1)):
            with pytest.raises(_native.VcpError) as e:
                call()
            assert e.value.code == -6                                   # VCP_ERR_NO_DEVICE
