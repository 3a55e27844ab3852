"""vcp_format_rows on the MI355X against the Python writers' formatting ('%.*f' % (bit, v), '%d') on the same arrays, as
bytes: the host form and the _dev form, under the staged k_fmt_write (VCP_FMT_DIRECT=0) and the direct one
(VCP_FMT_DIRECT=1; the switch is read at every call), on the smallest shapes at which each piece can go wrong -- a
workgroup is 256 lines, its LDS span 256 * VCP_FMT_LINE_MAX bytes, its stores 16 bytes wide.  The device compile of
csrc/scanfmt.hpp is held to the corpus of tests/scanfmt_corpus.py, the one the host compile is held to."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import scanfmt_corpus as K
from vtkcloudpoint_amd import _native as N
from vtkcloudpoint_amd import io as vio
from vtkcloudpoint_amd.datamodel import ClusObj, Point3D

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TT = 256
EOLS = (b"\n", b"\r\n")
BIG = -math.nextafter(1e15, 0.0)          # -999999999999999.875: 32 bytes at bit 15
INT32_MIN = -2147483648


@pytest.fixture(params=["staged", "direct"])
def mode(request, monkeypatch):
    monkeypatch.setenv("VCP_FMT_DIRECT", "1" if request.param == "direct" else "0")
    return request.param


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def ref_lines(a, b, c, ids=None, order=None, bit=6, eol=1):
    """The lines as the Python writers format them, one bytes object per line."""
    a, b, c = (np.asarray(x, np.float64).tolist() for x in (a, b, c))
    rows = range(len(a)) if order is None else [int(r) for r in order]
    num = "%%.%df\t%%.%df\t%%.%df" % (bit, bit, bit)
    if ids is None:
        return [(num % (a[r], b[r], c[r])).encode() + EOLS[eol] for r in rows]
    ids = [int(i) for i in ids]
    return [(("%d\t" + num) % (ids[r], a[r], b[r], c[r])).encode() + EOLS[eol] for r in rows]


def first_difference(got, lines):
    """A message that names the first line that differs (the texts are known to differ)."""
    o = 0
    for j, ln in enumerate(lines):
        if got[o:o + len(ln)] != ln:
            return "line %d: wanted %r, got %r" % (j, ln, got[o:o + len(ln) + 8])
        o += len(ln)
    return "%d bytes wanted, %d got; tail %r" % (o, len(got), got[o:o + 40])


def both_forms(ctx, a, b, c, ids=None, order=None, bit=6, eol=1):
    """The text from the host form and from the _dev form (the same views, on the device), each checked against ref_lines;
    a, b, c may be strided numpy views."""
    lines = ref_lines(a, b, c, ids, order, bit, eol)
    want = b"".join(lines)
    got = ctx.format_rows(a, b, c, ids, order, bit, eol).tobytes()
    assert got == want, "host form, " + first_difference(got, lines)
    assert ctx.format_rows(a, b, c, ids, order, bit, eol, count_only=True) == len(want)
    ta, tb, tc = device_views((a, b, c))
    t_ids = None if ids is None else dev(np.asarray(ids, np.int32))
    # an empty order still is an order: a pointer that is not NULL (an empty tensor's may be)
    t_ord = None if order is None else dev(np.asarray(order, np.int64) if len(order) else np.zeros(1, np.int64))
    n = len(a)
    m = n if order is None else len(order)
    args = (ta.data_ptr(), max(ta.stride(0), 1) if n else 1, tb.data_ptr(), max(tb.stride(0), 1) if n else 1,
            tc.data_ptr(), max(tc.stride(0), 1) if n else 1, n, None if t_ids is None else t_ids.data_ptr(),
            None if t_ord is None else t_ord.data_ptr(), m)
    torch.cuda.synchronize()
    assert ctx.format_rows_dev(*args, bit=bit, eol=eol) == len(want)
    out = np.full(len(want) + 32, 0xAA, np.uint8)
    assert ctx.format_rows_dev(*args, bit=bit, eol=eol, out=out) == len(want)
    got = out[:len(want)].tobytes()
    assert got == want, "_dev form, " + first_difference(got, lines)
    assert (out[len(want):] == 0xAA).all()                  # not a byte past the text
    return want


def device_views(cols):
    """The 1-D float64 numpy views on the device at their strides: the memory from a view's first to its last element is
    uploaded and viewed with the same stride; the same view twice is the same tensor, so the same pointer."""
    seen, out = {}, []
    for x in cols:
        assert x.dtype == np.float64 and x.ndim == 1
        if len(x) == 0:
            out.append(torch.zeros(1, dtype=torch.float64, device="cuda")[:0])
            continue
        s = x.strides[0] // 8
        key = (x.__array_interface__["data"][0], len(x), s)
        if key not in seen:
            seen[key] = dev(np.lib.stride_tricks.as_strided(x, ((len(x) - 1) * s + 1,), (8,)))[::s]
        out.append(seen[key])
    return out


def cloud(n, seed, lo=-400.0, hi=1000.0):
    rng = np.random.default_rng(seed)
    return np.round(rng.uniform(lo, hi, (n, 3)), 6)


def test_feature_symbols_exist():
    lib = N.lib()
    assert all(hasattr(lib, s) for s in ("vcp_format_rows", "vcp_format_rows_dev", "vcp_selftest_format_field"))


def test_the_switch_selects_the_kernel():
    """A child process per setting with the launch trace on (it is read once per process): VCP_FMT_DIRECT=1 launches
    k_fmt_write<false>, VCP_FMT_DIRECT=0 k_fmt_write<true>."""
    code = ("import numpy as np; from vtkcloudpoint_amd import _native as N; c = N.Context(0); "
            "a = np.arange(5.0); print(c.format_rows(a, a, a).tobytes())")
    for sw, kernel in (("1", "k_fmt_write<false>"), ("0", "k_fmt_write<true>")):
        env = dict(os.environ, VCP_FMT_DIRECT=sw, VCP_TRACE="1", PYTHONPATH=ROOT)
        r = subprocess.run([sys.executable, "-c", code], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env,
                           timeout=120)
        assert r.returncode == 0, r.stderr.decode()
        err = r.stderr.decode()
        assert "vcp-trace launch k_fmt_len" in err and "vcp-trace launch " + kernel in err, err
        assert b"0.000000\\t0.000000\\t0.000000\\r\\n1.000000" in r.stdout


# ---- workgroup boundaries ---------------------------------------------------------------------------------------------
def test_no_lines_and_one_line(vcp_ctx, mode):
    z = np.zeros(0)
    for eol in (0, 1):
        assert both_forms(vcp_ctx, z, z, z, eol=eol) == b""
        assert both_forms(vcp_ctx, z, z, z, ids=np.zeros(0, np.int32), order=np.zeros(0, np.int64), eol=eol) == b""
        one = both_forms(vcp_ctx, np.array([1.5]), np.array([-2.25]), np.array([300.125]), eol=eol)
        assert one == b"1.500000\t-2.250000\t300.125000" + EOLS[eol]
    # rows without lines: an empty order over a cloud
    r = cloud(10, 1)
    assert both_forms(vcp_ctx, r[:, 0], r[:, 1], r[:, 2], order=np.zeros(0, np.int64)) == b""


@pytest.mark.parametrize("n", [255, 256, 257])
def test_workgroup_edge(vcp_ctx, mode, n):
    r = cloud(n, n)
    both_forms(vcp_ctx, r[:, 0].copy(), r[:, 1].copy(), r[:, 2].copy(), ids=np.arange(n, dtype=np.int32) - 100)


def test_longest_and_shortest_lines(vcp_ctx, mode):
    n = 2 * TT + 1
    big = np.full(n, BIG)
    text = both_forms(vcp_ctx, big, big, big, ids=np.full(n, INT32_MIN, np.int32), bit=15, eol=1)
    assert len(text) == n * K.LINE_MAX                      # every workgroup's span is the LDS worst case
    z = np.zeros(n)
    assert both_forms(vcp_ctx, z, z, z, bit=0, eol=0) == b"0\t0\t0\n" * n


def test_store_alignment(vcp_ctx, mode):
    """Sixteen texts of the same 600 lines but the first, which has every length mod 16: over the sixteen, the spans of
    the second and the third workgroup start, and all three end, at every alignment of the 16-byte stores."""
    r = np.round(np.random.default_rng(16).uniform(-1000.0, 1000.0, (600, 3)), 2)
    residues, starts = set(), set()
    for d in range(1, 17):
        r[0] = (float(10 ** min(d, 15) - 1) * (-1.0 if d == 16 else 1.0), 0.0, 0.0)
        lines = ref_lines(r[:, 0], r[:, 1], r[:, 2], bit=2, eol=0)
        residues.add(len(lines[0]) % 16)
        starts.add(sum(len(x) for x in lines[:TT]) % 16)
        both_forms(vcp_ctx, r[:, 0], r[:, 1], r[:, 2], bit=2, eol=0)
    assert residues == set(range(16)) and starts == set(range(16))


# ---- column layouts and order -----------------------------------------------------------------------------------------
def test_column_layouts(vcp_ctx, mode):
    n = 300
    r = cloud(n, 7)
    ids = np.arange(n, dtype=np.int32) - 150
    ids[[0, 299]] = (INT32_MIN, 2147483647)
    sep = [r[:, k].copy() for k in range(3)]
    for use_ids in (None, ids):
        t1 = both_forms(vcp_ctx, sep[0], sep[1], sep[2], ids=use_ids)              # stride 1, three arrays
        t3 = both_forms(vcp_ctx, r[:, 0], r[:, 1], r[:, 2], ids=use_ids)           # stride 3, one [n, 3] array
        assert t1 == t3
        both_forms(vcp_ctx, sep[2], sep[2], sep[2], ids=use_ids)                   # one array three times
        both_forms(vcp_ctx, r[:, 1], r[:, 1], r[:, 1], ids=use_ids)
    # xyz of another width: the columns of an [n, 5] array
    w = np.round(np.random.default_rng(8).uniform(-50, 50, (n, 5)), 4)
    both_forms(vcp_ctx, w[:, 4], w[:, 0], w[:, 2], bit=3, eol=0)


def test_order(vcp_ctx, mode):
    n = 700
    r = cloud(n, 9)
    ids = (np.arange(n) % 5).astype(np.int32)
    rng = np.random.default_rng(10)
    cols = (r[:, 0], r[:, 1], r[:, 2])
    plain = both_forms(vcp_ctx, *cols, ids=ids)
    assert both_forms(vcp_ctx, *cols, ids=ids, order=np.arange(n)) == plain
    both_forms(vcp_ctx, *cols, ids=ids, order=rng.permutation(n))
    both_forms(vcp_ctx, *cols, order=np.sort(rng.choice(n, 300, replace=False)))       # a subset
    both_forms(vcp_ctx, *cols, ids=ids, order=rng.integers(0, n, 900))                   # repeats, more lines than rows
    both_forms(vcp_ctx, *cols, order=np.zeros(0, np.int64))


def test_order_out_of_range(vcp_ctx, mode):
    n = 700
    r = cloud(n, 11)
    a, b, c = (r[:, k].copy() for k in range(3))
    ta, tb, tc = dev(a), dev(b), dev(c)
    for first, second in ((n, -1), (-1, n)):
        order = np.arange(n, dtype=np.int64)
        order[300], order[600] = first, second           # the second and the third workgroup
        with pytest.raises(N.VcpError) as e:
            vcp_ctx.format_rows(a, b, c, order=order)
        assert e.value.code == -4 and e.value.err == (300, first)
        t_ord = dev(order)
        out = np.full(64, 0xAA, np.uint8)
        with pytest.raises(N.VcpError) as e:
            vcp_ctx.format_rows_dev(ta.data_ptr(), 1, tb.data_ptr(), 1, tc.data_ptr(), 1, n, None, t_ord.data_ptr(), n,
                                    out=out)
        assert e.value.code == -4 and e.value.err == (300, first) and (out == 0xAA).all()
    with pytest.raises(N.VcpError) as e:                  # rows without a single one in range
        vcp_ctx.format_rows(np.zeros(0), np.zeros(0), np.zeros(0), order=np.array([0]))
    assert e.value.code == -4 and e.value.err == (0, 0)


# ---- buffer sizing and limits -----------------------------------------------------------------------------------------
def test_capacity(vcp_ctx, mode):
    n = 600
    r = cloud(n, 12)
    a, b, c = (r[:, k].copy() for k in range(3))
    want = b"".join(ref_lines(a, b, c))
    ta, tb, tc = dev(a), dev(b), dev(c)
    args = (ta.data_ptr(), 1, tb.data_ptr(), 1, tc.data_ptr(), 1, n)
    assert vcp_ctx.format_rows_dev(*args) == len(want)                       # count-only
    assert vcp_ctx.format_rows(a, b, c, count_only=True) == len(want)
    for call in (lambda o: vcp_ctx.format_rows_dev(*args, out=o), lambda o: len(vcp_ctx.format_rows(a, b, c, out=o))):
        small = np.full(len(want) - 1, 0xAA, np.uint8)
        with pytest.raises(N.VcpError) as e:
            call(small)
        assert e.value.code == -4 and e.value.nbytes == len(want) and (small == 0xAA).all()
        exact = np.full(len(want), 0xAA, np.uint8)
        assert call(exact) == len(want) and exact.tobytes() == want


def test_argument_errors(vcp_ctx):
    a = np.arange(4.0)
    t = dev(a)
    p = t.data_ptr()
    ok = dict(d_a=p, stride_a=1, d_b=p, stride_b=1, d_c=p, stride_c=1, n=4)
    assert vcp_ctx.format_rows_dev(**ok) == len(b"".join(ref_lines(a, a, a)))
    for bad in (dict(bit=-1), dict(bit=16), dict(eol=2), dict(eol=-1), dict(stride_a=0), dict(stride_b=-3),
                dict(stride_c=0), dict(m=3), dict(d_a=None), dict(d_c=None), dict(n=-1)):
        with pytest.raises(N.VcpError) as e:
            vcp_ctx.format_rows_dev(**dict(ok, **bad))
        assert e.value.code == -1, bad


def test_exact_total(vcp_ctx):
    """The 2^32 limit is not run at size.  The byte count comes from k_fmt_sum, a 64-bit sum of the workgroup totals,
    which vcp_selftest_format_total_dev runs on words of the caller's: three words of 2^31 sum to 3 * 2^31, where a
    32-bit scan's total wraps to 2^31; 100 000 words of 256 * 112 = 28 672, the most a workgroup holds, give 2 867 200 000;
    150 000 of them 4 300 800 000 >= 2^32, the figure the driver compares."""
    for words in (np.full(3, 1 << 31, np.uint32), np.full(100_000, TT * K.LINE_MAX, np.uint32),
                  np.full(150_000, TT * K.LINE_MAX, np.uint32),
                  np.random.default_rng(3).integers(0, 1 << 32, 1001, dtype=np.uint64).astype(np.uint32),
                  np.zeros(0, np.uint32)):
        t = dev(words) if len(words) else torch.zeros(1, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        assert vcp_ctx.selftest_format_total_dev(t.data_ptr(), len(words)) == int(words.astype(np.uint64).sum())
    assert 150_000 * TT * K.LINE_MAX >= 1 << 32


# ---- unsupported values -----------------------------------------------------------------------------------------------
def test_unsupported_values(vcp_ctx, mode, tmp_path):
    n = 700
    r = cloud(n, 13)
    r[600, 0] = float("nan")
    r[300, 2] = 1e15
    r[300, 1] = float("inf")                             # column 1 comes before column 2
    a, b, c = r[:, 0], r[:, 1], r[:, 2]
    with pytest.raises(N.VcpError) as e:
        vcp_ctx.format_rows(a, b, c)
    assert e.value.code == -8 and e.value.err == (300, 1)
    t = dev(r)
    out = np.full(64, 0xAA, np.uint8)
    with pytest.raises(N.VcpError) as e:                  # in output order: row 600 is line 99 of the reversed cloud
        vcp_ctx.format_rows_dev(t.data_ptr(), 3, t.data_ptr() + 8, 3, t.data_ptr() + 16, 3, n,
                                d_order=dev(np.arange(n - 1, -1, -1)).data_ptr(), m=n, out=out)
    assert e.value.code == -8 and e.value.err == (99, 0) and (out == 0xAA).all()
    # the wrappers fall back to the host writer for the whole call
    want = b"".join(ref_lines(a, b, c))
    assert b"nan" in want and b"inf" in want
    assert vio.format_scan_text(a, b, c, ctx=vcp_ctx) == want
    assert vio.format_scan_text(t[:, 0], t[:, 1], t[:, 2], ctx=vcp_ctx) == want
    vio.write_scan_text_fast(str(tmp_path / "u.txt"), t, ctx=vcp_ctx)
    assert (tmp_path / "u.txt").read_bytes() == want
    # and the next call is none the worse for it
    good = cloud(n, 14)
    both_forms(vcp_ctx, good[:, 0], good[:, 1], good[:, 2])


# ---- the device compile against the corpus ----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def corpus():
    K.check_census(K.census())
    v = np.array(K.SUPPORTED, np.float64).reshape(-1, 3)
    return v, {bit: [[K.expected(x, bit) for x in row] for row in v.tolist()] for bit in K.BITS}


def test_device_compile_against_the_corpus(vcp_ctx, mode, corpus):
    v, want = corpus
    t = dev(v)
    n = len(v)
    args = (t.data_ptr(), 3, t.data_ptr() + 8, 3, t.data_ptr() + 16, 3, n)
    for bit in K.BITS:
        text = b"".join(b"\t".join(f) + b"\n" for f in want[bit])
        out = np.empty(len(text) + 4096, np.uint8)
        k = vcp_ctx.format_rows_dev(*args, bit=bit, eol=0, out=out)
        for form, got in (("_dev", out[:k].tobytes()), ("host", vcp_ctx.format_rows(v[:, 0], v[:, 1], v[:, 2], bit=bit,
                                                                                   eol=0).tobytes())):
            if got == text:
                continue
            rows = got.split(b"\n")
            for j, fields in enumerate(want[bit]):
                g = rows[j].split(b"\t") if j < len(rows) else []
                for col in range(3):
                    assert col < len(g) and g[col] == fields[col], "%s form, bit %d, v = %r: wanted %r, got %r" % (
                        form, bit, v[j, col], fields[col], g[col] if col < len(g) else None)
            assert False, "%s form, bit %d: %d bytes wanted, %d got" % (form, bit, len(text), len(got))


# ---- round trip, wrappers ---------------------------------------------------------------------------------------------
def test_round_trip_with_the_parser(vcp_ctx, mode):
    """parse_scan_text(format_scan_text(rows, bit=6)) == float('%.6f' % v) element by element, by their bits: 70 000 rows
    are 2.1 MB of text, far more than four of the parser's chunks, and 274 format workgroups."""
    n = 70_000
    rng = np.random.default_rng(21)
    rows = rng.uniform(-400.0, 1000.0, (n, 3))
    rows[::97, 0] = -1e-9                                  # prints as -0.000000 and reads back as -0.0
    want = np.array([float("%.6f" % x) for x in rows.reshape(-1).tolist()]).reshape(n, 3)
    t = dev(rows)
    text = vio.format_scan_text(t[:, 0], t[:, 1], t[:, 2], bit=6, ctx=vcp_ctx)
    got = vio.parse_scan_text(text, ctx=vcp_ctx)
    assert got["n"] == n and np.array_equal(got["rows"].view(np.uint64), want.view(np.uint64))
    assert np.signbit(got["rows"][0, 0]) and got["rows"][0, 0] == 0.0


def test_format_scan_text_in_pieces(vcp_ctx, mode):
    n = 2500
    r = cloud(n, 22)
    ids = (np.arange(n) % 7).astype(np.int32)
    order = np.random.default_rng(23).integers(0, n, 3100)
    t = dev(r)
    for cols in ((r[:, 0], r[:, 1], r[:, 2]), (t[:, 0], t[:, 1], t[:, 2])):
        for o in (None, order):
            want = b"".join(ref_lines(r[:, 0], r[:, 1], r[:, 2], ids, o, 4, 0))
            assert vio.format_scan_text(*cols, ids=ids, order=o, bit=4, eol="\n", ctx=vcp_ctx, max_lines=1000) == want
            assert vio.format_scan_text(*cols, ids=ids, order=o, bit=4, eol="\n", ctx=vcp_ctx) == want


def test_resident_wrappers_against_the_python_writers(vcp_ctx, mode, tmp_path):
    n = 3000
    rng = np.random.default_rng(24)
    rows = np.round(np.column_stack([rng.uniform(-40, 40, n), rng.uniform(-30, 30, n), rng.uniform(1, 900, n)]), 6)
    labels = rng.integers(0, 6, n).astype(np.int32)      # 0 = no cluster; clusters 1..5 interleaved in input order
    keep = rng.random(n) < 0.8
    pts = []
    for i in range(n):
        p = Point3D(0.0, 0.0, 0.0, int(labels[i]), True)
        p.motor_x, p.motor_y, p.Distance = rows[i].tolist()
        pts.append(p)

    def clus_list(points):
        cl = [ClusObj() for _ in range(5)]
        for p in points:                                  # Tools.GetClusList: every li in input order
            if p.clusterId >= 1:
                cl[p.clusterId - 1].li.append(p)
        return cl

    def ref(name, write, *args):
        write(str(tmp_path / name), *args)
        return (tmp_path / name).read_bytes()

    def got(name, write, *args, **kw):
        write(str(tmp_path / name), *args, ctx=vcp_ctx, **kw)
        return (tmp_path / name).read_bytes()

    t_rows, t_lab, t_keep = dev(rows), dev(labels), dev(keep)
    for bit in (6, 3):
        scan = ref("s.txt", vio.write_scan_text, pts, bit)
        assert got("a.txt", vio.write_scan_text_fast, rows, bit) == scan
        assert got("a.txt", vio.write_scan_text_fast, t_rows, bit) == scan
        assert got("a.txt", vio.write_scan_text_fast, (t_rows[:, 0], t_rows[:, 1], t_rows[:, 2]), bit) == scan
        clus = ref("c.txt", vio.write_clusters_text, clus_list(pts), bit)
        assert clus.count(b"\r\n") == int((labels >= 1).sum()) and clus.startswith(b"1\t")
        assert got("b.txt", vio.write_clusters_text_fast, labels, rows[:, 0], rows[:, 1], rows[:, 2], bit) == clus
        assert got("b.txt", vio.write_clusters_text_fast, t_lab, t_rows[:, 0], t_rows[:, 1], t_rows[:, 2], bit) == clus
        # export_resident on the tensors import_scan_resident returns
        imp = dict(motor=t_rows[:, :2].contiguous(), dist=t_rows[:, 2].contiguous())
        assert got("e.txt", vio.export_resident, imp, bit=bit) == scan
        assert got("e.txt", vio.export_resident, imp, labels=t_lab, bit=bit) == clus
        kept = [p for p, k in zip(pts, keep.tolist()) if k]     # cleanDataByDistance's RemoveAll
        assert got("e.txt", vio.export_resident, imp, keep=t_keep, bit=bit) == ref("s.txt", vio.write_scan_text, kept, bit)
        assert got("e.txt", vio.export_resident, imp, labels=t_lab, keep=t_keep, bit=bit) == ref(
            "c.txt", vio.write_clusters_text, clus_list(kept), bit)
    # the centroid export: X TAB Y TAB Z, one line per centre
    c3 = np.round(rng.uniform(-500, 500, (37, 3)), 5)
    want = b"".join(ref_lines(c3[:, 0], c3[:, 1], c3[:, 2], bit=4, eol=1))
    assert got("k.txt", vio.write_centroids_text_fast, c3, 4) == want
    assert got("k.txt", vio.write_centroids_text_fast, dev(c3), 4) == want


# ---- the context's history, the caller's stream, timing ----------------------------------------------------------------
def test_repeatability(vcp_ctx, mode):
    n = 1000
    r = cloud(n, 31)
    t = dev(r)
    args = (t.data_ptr(), 3, t.data_ptr() + 8, 3, t.data_ptr() + 16, 3, n)
    want = b"".join(ref_lines(r[:, 0], r[:, 1], r[:, 2]))

    def run():
        out = np.empty(len(want), np.uint8)
        assert vcp_ctx.format_rows_dev(*args, out=out) == len(want)
        return out.tobytes()

    assert run() == want and run() == want
    xy = dev(r[:, :2].copy())
    lab, core, cls = (torch.zeros(n, dtype=dt, device="cuda") for dt in (torch.int32, torch.uint8, torch.uint8))
    torch.cuda.synchronize()
    vcp_ctx.dbscan_dev(xy.data_ptr(), n, 2, 5.0, 4, d_labels=lab.data_ptr(), d_is_core=core.data_ptr(),
                       d_is_classed=cls.data_ptr())
    assert run() == want
    bad = dev(np.array([1.0, float("nan"), 2.0]))
    torch.cuda.synchronize()
    with pytest.raises(N.VcpError) as e:
        vcp_ctx.format_rows_dev(bad.data_ptr(), 1, bad.data_ptr(), 1, bad.data_ptr(), 1, 3)
    assert e.value.code == -8 and e.value.err == (1, 0)
    assert run() == want


def test_on_the_callers_stream(mode):
    """The method of tests/test_stream_gpu.py: on the caller's stream a filler kernel spins, and behind it cloud B is copied
    over the columns.  format_rows_dev runs on that stream, so it formats B; a launch on another stream would read A."""
    n = 1000
    A, B = cloud(n, 41), cloud(n, 42)
    ctx = N.Context(0)
    s = torch.cuda.Stream()
    ctx.set_stream(s.cuda_stream)
    try:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        probe = 50_000_000
        with torch.cuda.stream(s):
            e0.record()
            torch.cuda._sleep(probe)
            e1.record()
        s.synchronize()
        ticks = int(60.0 * probe / e0.elapsed_time(e1))   # a filler of some 60 ms
        buf, dB = dev(A), dev(B)
        wantA, wantB = (b"".join(ref_lines(x[:, 0], x[:, 1], x[:, 2])) for x in (A, B))
        assert wantA != wantB
        out = np.empty(max(len(wantA), len(wantB)) + 64, np.uint8)
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            torch.cuda._sleep(ticks)
            buf.copy_(dB, non_blocking=True)
        assert not s.query()                              # the filler still runs: buf still holds A
        k = ctx.format_rows_dev(buf.data_ptr(), 3, buf.data_ptr() + 8, 3, buf.data_ptr() + 16, 3, n, out=out)
        assert s.query()                                  # the call is blocking: its work on s is done
        assert out[:k].tobytes() == wantB
    finally:
        torch.cuda.synchronize()
        ctx.close()


def test_timing_phases(vcp_ctx, mode):
    r = cloud(500, 51)
    vcp_ctx.timing_enable(True)
    try:
        vcp_ctx.format_rows(r[:, 0], r[:, 1], r[:, 2], out=np.empty(1 << 16, np.uint8))
        names = [nm for nm, _ in vcp_ctx.timing()]
    finally:
        vcp_ctx.timing_enable(False)
    assert names == ["fmt_len", "fmt_write", "fmt_download"]
