"""The export formatter without a GPU: the host compile of csrc/scanfmt.hpp (vcp_selftest_format_field) against the
corpus of tests/scanfmt_corpus.py -- '%.*f' % (bit, v) byte for byte at every bit --, the unsupported list, the argument
errors, the longest line, the declarations, and the same source stand-alone under the host's address and
undefined-behaviour sanitizers (tools/scanfmt_check.cpp, a program of its own: nothing loaded into Python is sanitized)."""
import ctypes as C
import math
import os
import re
import subprocess

import pytest

import scanfmt_corpus as K
from vtkcloudpoint_amd import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def census():
    return K.census()


def test_corpus_census(census):
    K.check_census(census)


def test_host_compile_against_the_corpus(census):
    K.check_census(census)
    lib = N.lib()
    out = C.create_string_buffer(64)
    n = C.c_int64(0)
    done = 0
    for v in K.SUPPORTED:
        cv = C.c_double(v)
        for bit in K.BITS:
            want = K.expected(v, bit)
            rc = lib.vcp_selftest_format_field(cv, C.c_int(bit), out, C.c_int64(64), C.byref(n))
            got = out.raw[:n.value] if rc == 1 else None
            assert rc == 1 and n.value == len(want) and got == want, \
                "v = %r, bit = %d: wanted %r, got %r (rc %d, len %d)" % (v, bit, want, got, rc, n.value)
            done += 1
    assert done == census["supported"] * len(K.BITS)


def test_unsupported_values_write_nothing():
    lib = N.lib()
    for v in K.UNSUPPORTED:
        for bit in K.BITS:
            out = C.create_string_buffer(b"\xAA" * 64, 64)
            n = C.c_int64(-5)
            assert lib.vcp_selftest_format_field(C.c_double(v), C.c_int(bit), out, C.c_int64(64), C.byref(n)) == 0, (v, bit)
            assert out.raw == b"\xAA" * 64 and n.value == -5
            assert N.selftest_format_field(v, bit) is None
    # the last supported value on either side of the limit
    assert N.selftest_format_field(math.nextafter(1e15, 0.0), 3) == b"999999999999999.875"
    assert N.selftest_format_field(-math.nextafter(1e15, 0.0), 0) == b"-1000000000000000"


def test_argument_errors():
    lib = N.lib()
    out = C.create_string_buffer(b"\xAA" * 64, 64)
    n = C.c_int64(-5)
    v = C.c_double(-123.456)
    for bit in (-1, 16):
        assert lib.vcp_selftest_format_field(v, C.c_int(bit), out, C.c_int64(64), C.byref(n)) == -1
    assert lib.vcp_selftest_format_field(v, C.c_int(3), None, C.c_int64(64), C.byref(n)) == -1
    assert lib.vcp_selftest_format_field(v, C.c_int(3), out, C.c_int64(64), None) == -1
    assert out.raw == b"\xAA" * 64 and n.value == -5
    # -123.456 at bit 3 has 8 bytes: a cap of 7 is an error that reports the length and writes no byte
    assert lib.vcp_selftest_format_field(v, C.c_int(3), out, C.c_int64(7), C.byref(n)) == -1
    assert n.value == 8 and out.raw == b"\xAA" * 64
    assert lib.vcp_selftest_format_field(v, C.c_int(3), out, C.c_int64(8), C.byref(n)) == 1
    assert out.raw[:8] == b"-123.456" and out.raw[8:] == b"\xAA" * 56
    with pytest.raises(N.VcpError) as e:
        N.selftest_format_field(-123.456, 3, cap=7)
    assert e.value.code == -1 and e.value.len == 8


def _header():
    with open(os.path.join(ROOT, "include", "vcp.h")) as f:
        return f.read()


def test_longest_line(census):
    """The bound the kernels size their LDS by: an 11-byte id, three fields of 32 bytes, three tabs and "\\r\\n".  A line
    is constructed that reaches it; no field of the corpus or of the extremes exceeds 32 bytes, and the 16-digit integer
    part appears only without a decimal point."""
    line_max = int(re.search(r"^#define VCP_FMT_LINE_MAX (\d+)\b", _header(), flags=re.M).group(1))
    assert line_max == K.LINE_MAX
    big = -math.nextafter(1e15, 0.0)                       # -999999999999999.875
    field = N.selftest_format_field(big, 15)
    assert field == K.expected(big, 15) and len(field) == K.FIELD_MAX
    line = b"%d\t" % -2147483648 + field + b"\t" + field + b"\t" + field + b"\r\n"
    assert len(line) == line_max
    assert census["longest_field"] == K.FIELD_MAX
    # the largest magnitudes at every bit: 10^15 itself is reached at bit 0 alone
    x = math.nextafter(1e15, 0.0)
    for _ in range(64):
        for bit in K.BITS:
            got = N.selftest_format_field(-x, bit)
            assert got == K.expected(-x, bit) and len(got) <= K.FIELD_MAX
            if got.lstrip(b"-").split(b".")[0] == b"1000000000000000":
                assert bit == 0
        x = math.nextafter(x, 0.0)


def test_declared_and_bound():
    h = _header()
    for s in ("vcp_format_rows", "vcp_format_rows_dev", "vcp_selftest_format_field", "vcp_selftest_format_total_dev"):
        assert re.search(r"\b%s\s*\(" % s, h), s
        assert s in N.SYMBOLS and hasattr(N.lib(), s)
    assert hasattr(N.Context, "format_rows") and hasattr(N.Context, "format_rows_dev")


def test_host_fallback_equals_the_python_writers(tmp_path):
    """io._format_host is what the wrappers fall back to: the bytes write_scan_text / write_clusters_text put in a file."""
    from vtkcloudpoint_amd import io as vio
    from vtkcloudpoint_amd.datamodel import ClusObj, Point3D
    vals = K.SUPPORTED[:300] + [float("nan"), float("inf"), -1e300]
    while len(vals) % 3:
        vals.append(1.0)
    rows = [vals[i:i + 3] for i in range(0, len(vals), 3)]
    pts = []
    for k, r in enumerate(rows):
        p = Point3D(0.0, 0.0, 0.0, k % 4, True)
        p.motor_x, p.motor_y, p.Distance = r
        pts.append(p)
    a, b, c = ([r[k] for r in rows] for k in range(3))
    vio.write_scan_text(str(tmp_path / "s.txt"), pts, bit=4)
    assert (tmp_path / "s.txt").read_bytes() == vio._format_host(a, b, c, None, None, 4, "\r\n")
    labels = [p.clusterId for p in pts]
    order = vio.cluster_order(labels)
    clus = [ClusObj() for _ in range(3)]
    for p in pts:
        if p.clusterId >= 1:
            clus[p.clusterId - 1].li.append(p)
    vio.write_clusters_text(str(tmp_path / "c.txt"), clus, bit=6)
    assert (tmp_path / "c.txt").read_bytes() == vio._format_host(a, b, c, labels, order, 6, "\r\n")


def test_stand_alone_under_the_host_sanitizers(tmp_path):
    """tools/scanfmt_check.cpp: the same header, compiled on its own with -fsanitize=address,undefined, against the C
    library's "%.*f" on 300 000 seeded pairs (any bit pattern among them), every field written into a heap buffer of
    exactly its length."""
    exe = str(tmp_path / "scanfmt_check")
    # the runtimes are linked into the program, so it does not matter what else the process has loaded before it
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan", "-I" + os.path.join(ROOT, "vtkcloudpoint_amd", "csrc"),
                           os.path.join(ROOT, "tools", "scanfmt_check.cpp"), "-o", exe])
    r = subprocess.run([exe, "300000"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    text = r.stdout.decode(errors="replace")
    assert r.returncode == 0 and text.startswith("ok: 300000 pairs"), text
    assert "longest field 32 bytes" in text
