"""vcp_parse_scan_text on the MI355X against io.read_scan_text on a temporary file: rows by their bits (NaN signs and -0
count), group, seg_first, n, n_host, the three errors with read_scan_text's own ValueError text, the fallback, count-only,
independence from the context's history, read_folder_resident and the caller's stream -- on the smallest texts at which
each mechanism can go wrong (a chunk is VCP_TXT_CHUNK = 16384 bytes, a parse workgroup 256 lines, its LDS span 32 KiB).
The second half holds the device compile of csrc/scantext.hpp to the corpus of tests/scantext_corpus.py under both parse
kernels, and walks the staging decision, the indexing kernels' lane, wave and chunk boundaries, the host list and the
segment search at size; tests/fuzz_scantext.py supplies a bounded randomised sweep."""
import os
import random
import re

import numpy as np
import pytest
import torch

import scantext_corpus as K
import scantext_ref as R
from vtkcloudpoint_amd import _native as N
from vtkcloudpoint_amd import io as vio

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _constant(path, pattern):
    with open(os.path.join(ROOT, *path)) as f:
        return int(re.search(pattern, f.read(), flags=re.M).group(1))


# read out of the sources, so that a change of either moves the tests with it
CHUNK = _constant(("include", "vcp.h"), r"^#define VCP_TXT_CHUNK (\d+)\b")
STAGE_BYTES = _constant(("vtkcloudpoint_amd", "csrc", "scantext.hip"), r"^constexpr int STAGE_BYTES = (\d+);")
TT = 256                                                         # lines per parse workgroup


def u64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def ref_rows(tmp_path, data, name="ref.txt"):
    p = tmp_path / name
    p.write_bytes(data)
    return vio.read_scan_text(str(p))


def same(ctx, tmp_path, data, n_host=None):
    """parse_scan_text (host form and resident form) == read_scan_text on a file with these bytes."""
    want = ref_rows(tmp_path, data)
    got = vio.parse_scan_text(data, ctx=ctx)
    assert got["n"] == len(want) and got["rows"].shape == want.shape
    assert np.array_equal(u64(got["rows"]), u64(want))
    assert not got["group"].any() and got["seg_first"].tolist() == [0, len(want)]
    res = vio.parse_scan_text(data, resident=True, ctx=ctx)
    assert res["n"] == len(want) and np.array_equal(u64(res["rows"].cpu().numpy()), u64(want))
    assert res["n_host"] == got["n_host"]
    if n_host is not None:
        assert got["n_host"] == n_host
    return got


def test_feature_symbols_exist():
    lib = N.lib()
    assert all(hasattr(lib, s) for s in ("vcp_parse_scan_text", "vcp_parse_scan_text_dev", "vcp_selftest_parse_field"))


def test_empty_text(vcp_ctx, tmp_path):
    got = same(vcp_ctx, tmp_path, b"")
    assert got["n"] == 0 and got["n_host"] == 0
    assert vcp_ctx.parse_scan_text(b"", count_only=True)["n"] == 0


@pytest.mark.parametrize("term", [b"\n", b"\r\n", b"\r", b""])
def test_one_line(vcp_ctx, tmp_path, term):
    got = same(vcp_ctx, tmp_path, b"1.5\t-2.25\t300.125" + term, n_host=0)
    assert got["rows"].tolist() == [[1.5, -2.25, 300.125]]


def test_mixed_terminators(vcp_ctx, tmp_path):
    data = b"1\t2\t3\n4\t5\t6\r\n7\t8\t9\r10\t11\t12\r\r\n"       # the last two terminators enclose an empty line
    with pytest.raises(ValueError):
        ref_rows(tmp_path, data)
    data = b"1\t2\t3\n4\t5\t6\r\n7\t8\t9\r10\t11\t12\r13\t14\t15\n\r16\t17\t18"
    with pytest.raises(ValueError):                              # "\n\r" is two terminators: an empty line again
        ref_rows(tmp_path, data)
    data = b"1\t2\t3\n4\t5\t6\r\n7\t8\t9\r10\t11\t12\r13\t14\t15\r\n16\t17\t18\r"
    assert same(vcp_ctx, tmp_path, data)["n"] == 6


def _line(rng, k):
    a, b, d = rng.uniform(-360, 360), rng.uniform(-360, 360), rng.uniform(0, 1000)
    return ("%.6f\t%.6f\t%.6f" % (a, b, d)).encode() + (b"\n", b"\r\n", b"\r")[k % 3]


def _fill(buf, rng, upto):
    """F6 lines with the three terminators in turn until fewer than 64 bytes are left before `upto`."""
    while len(buf) < upto - 64:
        buf += _line(rng, len(buf))
    return buf


def _pad_line(buf, end, term):
    """One line (blanks after its last number) that makes the text exactly `end` bytes long."""
    body = b"1.25\t-0\t7"
    k = end - len(buf) - len(body) - len(term)
    assert k >= 0
    return buf + body + b" " * k + term


@pytest.fixture(scope="module")
def chunk_text():
    """Four chunks: a "\\r\\n" whose bytes are 16383 and 16384, a line across byte 32768, a lone '\\r' at 49151."""
    rng = random.Random(3)
    buf = _pad_line(_fill(bytearray(), rng, CHUNK), CHUNK + 1, b"\r\n")
    assert buf[CHUNK - 1:CHUNK + 1] == b"\r\n"
    buf = _pad_line(_fill(buf, rng, 2 * CHUNK - 64), 2 * CHUNK + 9, b"\n")
    assert b"\n" not in buf[2 * CHUNK - 8:2 * CHUNK + 8] and b"\r" not in buf[2 * CHUNK - 8:2 * CHUNK + 8]
    buf = _pad_line(_fill(buf, rng, 3 * CHUNK), 3 * CHUNK, b"\r")
    assert buf[3 * CHUNK - 1:3 * CHUNK] == b"\r"
    buf = _fill(buf, rng, 3 * CHUNK + 3000) + b"9\t8\t7"        # no terminator at the end: the wrapper's '\n'
    return bytes(buf)


def test_chunk_straddles(vcp_ctx, tmp_path, chunk_text):
    got = same(vcp_ctx, tmp_path, chunk_text, n_host=0)
    assert got["n"] > 4 * 256                                    # several parse workgroups


@pytest.mark.parametrize("n", [255, 256, 257])
def test_second_workgroup_and_masked_tail(vcp_ctx, tmp_path, n):
    rng = random.Random(n)
    data = b"".join(_line(rng, k) for k in range(n))
    assert same(vcp_ctx, tmp_path, data, n_host=0)["n"] == n


def test_resident_form_comes_back_for_room(vcp_ctx, tmp_path):
    """Lines shorter than the resident form's first guess of one line per 16 bytes: VCP_ERR_INDEX, then the exact room."""
    data = b"1\t2\t3\n" * 5000
    assert len(data) // 16 + 1024 < 5000
    assert same(vcp_ctx, tmp_path, data, n_host=0)["n"] == 5000


def test_extra_fields_and_blanks(vcp_ctx, tmp_path):
    data = (b"1\t2\t3\tgarbage\t\x41_not a number\n"             # '_' is unsupported wherever it stands: see below
            b" 1.5 \t  -2 \t+3e2  \t\t\t\n"
            b".5\t1.\t+.5e-3\textra\n"
            b"-0\t0e5\t-0.0\t1e\n")
    with pytest.raises(N.VcpError) as e:
        vio.parse_scan_text(data, ctx=vcp_ctx)
    assert e.value.code == -8 and e.value.err[0] == data.index(b"_")
    data = data.replace(b"_", b"-")
    got = same(vcp_ctx, tmp_path, data, n_host=0)
    assert u64(got["rows"][3]).tolist() == [1 << 63, 0, 1 << 63]


def test_classes_two_and_three(vcp_ctx, tmp_path):
    rng = random.Random(17)
    vals = [rng.uniform(-1e3, 1e3) for _ in range(300)]
    lines = [("%r\t%.18e\t%.17g" % (v, v * 1e3, v * 1e7)).encode() for v in vals]      # class 2 (some class 1)
    host = {5: b"1e400\t1\t1", 77: b"1\t-1e-400\t1", 130: b"nan\t-nan\tINF", 131: b"-Infinity\t+inf\tNaN",
            299: b"0.1000000000000000055511151231257827\t123456789012345678901234567890\t4.9e-324",
            256: b"1\t1e23\t9007199254740993e-23"}
    for k, v in host.items():
        lines[k] = v
    data = b"\n".join(lines) + b"\n"
    assert sum(R.field_class(f.decode())[0] == 2 for ln in lines for f in ln.split(b"\t")) > 500
    got = same(vcp_ctx, tmp_path, data, n_host=len(host))
    assert u64(got["rows"][130]).tolist() == [0x7FF8000000000000, 0xFFF8000000000000, 0x7FF0000000000000]


def test_field_longer_than_any_lds_budget(vcp_ctx, tmp_path):
    data = b"1\t2\t3\n" + b"0" * 40000 + b"1.5\t" + b"0" * 40000 + b"\t0." + b"0" * 40000 + b"\n4\t5\t6\n"
    got = same(vcp_ctx, tmp_path, data)
    assert got["rows"].tolist() == [[1, 2, 3], [1.5, 0, 0], [4, 5, 6]]


FILES = [b"1\t2\t3\n4\t5\t6\n", b"", b"7\t8\t9\r", b"10\t11\t12", b"", b"13\t14\t15\r\n16\t17\t18\r\n19\t20\t21\r\n", b""]


def test_segments_group_seg_first_and_cap(vcp_ctx, tmp_path):
    want = [ref_rows(tmp_path, f, "f%d.txt" % k) for k, f in enumerate(FILES)]
    got = vio.parse_scan_text(FILES, ctx=vcp_ctx)
    assert np.array_equal(u64(got["rows"]), u64(np.concatenate(want)))
    assert got["group"].tolist() == [0, 0, 2, 3, 5, 5, 5]
    assert got["seg_first"].tolist() == [0, 2, 2, 3, 4, 4, 7, 7] and got["n"] == 7
    text, seg_off = vio._join_segments(FILES)
    rows = torch.zeros((7, 3), dtype=torch.float64, device="cuda")
    group = torch.zeros(7, dtype=torch.int32, device="cuda")
    with pytest.raises(N.VcpError) as e:
        vcp_ctx.parse_scan_text_dev(text, 6, rows.data_ptr(), group.data_ptr(), seg_off)
    assert e.value.code == -4 and e.value.n == 7                 # VCP_ERR_INDEX, and *n is written
    r = vcp_ctx.parse_scan_text_dev(text, 7, rows.data_ptr(), group.data_ptr(), seg_off)
    assert r["n"] == 7 and np.array_equal(u64(rows.cpu().numpy()), u64(got["rows"]))
    assert group.cpu().tolist() == got["group"].tolist()
    # a segment without its final '\n'
    bad = np.array([0, 5, len(text)], np.uint64)
    with pytest.raises(N.VcpError) as e:
        vcp_ctx.parse_scan_text(text, bad)
    assert e.value.code == -1
    with pytest.raises(N.VcpError) as e:
        vcp_ctx.parse_scan_text(b"1\t2\t3")
    assert e.value.code == -1


def _both_raise(ctx, tmp_path, data):
    p = tmp_path / "bad.txt"
    p.write_bytes(data)
    with pytest.raises(ValueError) as want:
        vio.read_scan_text(str(p))
    with pytest.raises(ValueError) as got:
        vio.read_scan_text_fast(str(p), ctx=ctx)
    assert str(got.value) == str(want.value)
    return str(got.value)


def test_bad_lines_give_read_scan_texts_error(vcp_ctx, tmp_path):
    good = b"1\t2\t3\n"
    assert _both_raise(vcp_ctx, tmp_path, good * 3 + b"\n" + good).endswith(":4: expected motor_x<TAB>motor_y<TAB>Distance")
    assert _both_raise(vcp_ctx, tmp_path, good * 300 + b"1\t2\n" + good).endswith(":301: expected motor_x<TAB>motor_y<TAB>Distance")
    assert _both_raise(vcp_ctx, tmp_path, good + b"1\t2e\t3\n" + good).endswith(":2: not a number")
    assert _both_raise(vcp_ctx, tmp_path, good + b"1\tx\n").endswith(":2: expected motor_x<TAB>motor_y<TAB>Distance")
    # both kinds: the earlier line wins, whichever kind it is
    assert _both_raise(vcp_ctx, tmp_path, good * 5 + b"1\t\t3\n" + good * 400 + b"1\t2\n").endswith(":6: not a number")
    assert _both_raise(vcp_ctx, tmp_path, good * 5 + b"1\t2\n" + good * 400 + b"1\t \t3\n").endswith(":6: expected motor_x<TAB>motor_y<TAB>Distance")
    # a class-3 line before a bad one does not hide it, and the err triple names the segment
    with pytest.raises(N.VcpError) as e:
        vcp_ctx.parse_scan_text(*vio._join_segments([good, b"", b"1e400\t1\t1\n" + good + b"a\tb\tc\n", good]))
    assert e.value.code == -1 and e.value.err == (3, 2, 2)


@pytest.mark.parametrize("bad", [b"\x85", b"_", "测".encode("gb2312"), b"\x0b", b"\x00", b"\x7f"])
def test_unsupported_bytes_fall_back(vcp_ctx, tmp_path, bad):
    data = b"1\t2\t3\n" * 700 + b"4\t5\t6\t" + bad + b"\n7\t8\t9\n"           # in the extra field: only 0x0B.. split lines
    with pytest.raises(N.VcpError) as e:
        vcp_ctx.parse_scan_text(data)
    assert e.value.code == -8 and e.value.err[0] == data.index(bad)
    p = tmp_path / "u.txt"
    p.write_bytes(data)
    try:
        want = vio.read_scan_text(str(p))
    except ValueError as ex:
        with pytest.raises(ValueError) as got:
            vio.read_scan_text_fast(str(p), ctx=vcp_ctx)
        assert str(got.value) == str(ex)
    else:
        assert np.array_equal(u64(vio.read_scan_text_fast(str(p), ctx=vcp_ctx)), u64(want))
    # the first of two, found by different workgroups
    two = data + b"1\t2\t3\n" * 4000 + bad
    with pytest.raises(N.VcpError) as e:
        vcp_ctx.parse_scan_text(two + b"\n")
    assert e.value.err[0] == data.index(bad)


def test_count_only_and_history(vcp_ctx, tmp_path, chunk_text):
    full = vio.parse_scan_text(chunk_text, ctx=vcp_ctx)
    text, seg_off = vio._join_segments(chunk_text)
    cnt = vcp_ctx.parse_scan_text(text, seg_off, count_only=True)
    assert cnt["n"] == full["n"] and cnt["rows"] is None and cnt["seg_first"].tolist() == full["seg_first"].tolist()
    assert vcp_ctx.parse_scan_text_dev(text, 0, None)["n"] == full["n"]
    again = vio.parse_scan_text(chunk_text, ctx=vcp_ctx)
    vcp_ctx.import_convert(np.random.default_rng(1).uniform(1, 50, (5000, 3)))     # an unrelated call in between
    vio.parse_scan_text(b"1e400\t2\t3\n" * 300, ctx=vcp_ctx)                          # and one that fills the host list
    third = vio.parse_scan_text(chunk_text, ctx=vcp_ctx)
    for g in (again, third):
        assert np.array_equal(u64(g["rows"]), u64(full["rows"])) and np.array_equal(g["group"], full["group"])
        assert g["n_host"] == 0


def test_read_folder_resident(vcp_ctx, tmp_path):
    rng = random.Random(8)
    paths, rows = [], []
    for k, n in enumerate((40, 1, 300)):
        lines = [_line(rng, i) for i in range(n)]
        lines += lines[: n // 3]                                   # duplicates within the file
        if k == 2:
            lines += [b"1.000000\t2.000000\t0.000000\n", b"1e-400\t1\t5\n"] + rows_dup       # one line for the host (0.0)
        rows_dup = lines[:5]                                       # and across files
        p = tmp_path / ("scan%d.txt" % k)
        p.write_bytes(b"".join(lines))
        paths.append(str(p))
        rows.append(vio.read_scan_text(str(p)))
    group = np.concatenate([np.full(len(r), k, np.int32) for k, r in enumerate(rows)])
    for by_file in (False, True):
        want = vio.import_scan_resident(np.concatenate(rows), group if by_file else None, 1.5, -0.5, ctx=vcp_ctx)
        for max_bytes in ((1 << 32) - 4096, 2000):                 # one batch; many batches with the large file cut
            got = vio.read_folder_resident(paths, 1.5, -0.5, by_file=by_file, ctx=vcp_ctx, max_bytes=max_bytes)
            for key in ("motor", "xyz", "dist", "src", "count", "group", "row_to"):
                assert torch.equal(got[key], want[key]), (key, by_file, max_bytes)
            assert (got["m"], got["duplicates"]) == (want["m"], want["duplicates"]) and got["n_host"] == 1
            assert np.array_equal(u64(got["rows"].cpu().numpy()), u64(np.concatenate(rows)))
            assert np.array_equal(got["file"].cpu().numpy(), group)
    assert want["duplicates"] > 100


def test_stream_contract(tmp_path, chunk_text):
    """parse_scan_text_dev on a caller's stream (tests/test_stream_gpu.py: read-only use of its Rig): the outputs are
    poisoned behind a filler kernel on that stream; on return the stream is idle and the outputs hold the rows."""
    from test_stream_gpu import Rig
    rig = Rig()
    try:
        want = ref_rows(tmp_path, chunk_text)
        text, seg_off = vio._join_segments([chunk_text, b"1e400\t-0\tnan\n"])
        want = np.concatenate([want, [[np.inf, -0.0, np.nan]]])
        n = len(want)
        rows = torch.zeros((n, 3), dtype=torch.float64, device="cuda")
        group = torch.zeros(n, dtype=torch.int32, device="cuda")
        r = rig.run(lambda: rig.ctx.parse_scan_text_dev(text, n, rows.data_ptr(), group.data_ptr(), seg_off),
                    poison=[(rows, -7.0), (group, -7)])
        assert r["n"] == n and r["n_host"] == 1
        assert np.array_equal(u64(rows.cpu().numpy()), u64(want))
        assert group.cpu().tolist() == [0] * (n - 1) + [1]
    finally:
        rig.close()


# ---- the device compile of csrc/scantext.hpp on the corpus of tests/test_scantext.py, both parse kernels ---------------
KERNELS = pytest.mark.parametrize("direct", [False, True], ids=["staged", "direct"])


def _kernel(monkeypatch, direct):
    """The library reads VCP_TXT_DIRECT at every call: unset = k_txt_parse<true>, "1" = k_txt_parse<false>."""
    if direct:
        monkeypatch.setenv("VCP_TXT_DIRECT", "1")
    else:
        monkeypatch.delenv("VCP_TXT_DIRECT", raising=False)


def _split(text):
    """The lines of a text of supported bytes, as the contract cuts them."""
    parts = re.split(b"\r\n|\n|\r", text)
    return parts[:-1] if parts and parts[-1] == b"" else parts


def _host_lines(text):
    """Lines with a class-3 field among the first three, by the restatement."""
    return sum(any(R.field_class(f.decode("ascii"))[0] == 3 for f in ln.split(b"\t")[:3]) for ln in _split(text))


def _difference(text, got, want):
    """None, or the first field whose bits differ: its text, the bits wanted and the bits got."""
    g, w = u64(got), u64(want)
    if g.shape != w.shape:
        return "%d rows for %d" % (len(g), len(w))
    d = np.argwhere(g != w)
    if len(d) == 0:
        return None
    i, k = (int(x) for x in d[0])
    return "line %d field %d %r: want %016x, got %016x (%d fields differ)" % (
        i + 1, k, _split(text)[i].split(b"\t")[k][:60], int(w[i, k]), int(g[i, k]), len(d))


def held(ctx, text, want=None, n_host=None):
    """Host form and resident form against _rows_from_bytes, by bits; n_host against the restatement's classes."""
    want = vio._rows_from_bytes(text, "text") if want is None else want
    n_host = _host_lines(text) if n_host is None else n_host
    got = vio.parse_scan_text(text, ctx=ctx)
    bad = _difference(text, got["rows"], want)
    assert bad is None, "host form: " + bad
    assert got["n"] == len(want) and got["n_host"] == n_host
    res = vio.parse_scan_text(text, resident=True, ctx=ctx)
    bad = _difference(text, res["rows"].cpu().numpy(), want)
    assert bad is None, "resident form: " + bad
    assert res["n"] == len(want) and res["n_host"] == n_host
    return got


@pytest.fixture(scope="module")
def corpus():
    """(text, rows of the reference, lines with a class-3 field): computed once, left unchanged."""
    text = K.lines(K.value_fields())
    return text, vio._rows_from_bytes(text, "corpus"), _host_lines(text)


@KERNELS
def test_device_evaluates_the_host_corpus(vcp_ctx, corpus, monkeypatch, direct):
    """Every value string of tests/scantext_corpus.py (its census is asserted in tests/test_scantext.py), three to a
    line, in one call per kernel: both branches of eval_class2, ties, the sticky bit, the mantissa carry, the class
    boundaries and class 1 beyond F6 text, as the device compiler emits them."""
    _kernel(monkeypatch, direct)
    text, want, n_host = corpus
    assert len(want) == (len(K.value_fields()) + 2) // 3 and n_host >= 7
    held(vcp_ctx, text, want, n_host)


def test_chunk_straddles_direct(vcp_ctx, tmp_path, chunk_text, monkeypatch):
    _kernel(monkeypatch, True)
    assert same(vcp_ctx, tmp_path, chunk_text, n_host=0)["n"] > 4 * 256


@KERNELS
def test_class_zero_fields_in_every_position(vcp_ctx, tmp_path, monkeypatch, direct):
    _kernel(monkeypatch, direct)
    zero = [s for s in K.EDGE if K.EDGE_CLASSES[s] == 0]
    assert len(zero) == 9
    good = b"1\t2\t3\n"
    for s in zero:
        for k in range(3):
            f = [b"1.5", b"-2", b"3e2"]
            f[k] = s.encode()
            msg = _both_raise(vcp_ctx, tmp_path, good * 2 + b"\t".join(f) + b"\n" + good)
            assert msg.endswith(":3: not a number"), (s, k, msg)


# ---- the staging decision of k_txt_parse<true> ------------------------------------------------------------------------
def _starts(text):
    return [0] + [m.end() for m in re.finditer(b"\r\n|\n|\r", text)]


_TIES = []


def _class2_line(i):
    """A product tie, a halfway case of the division and a mantissa carry on one line."""
    if not _TIES:
        _TIES.extend((K.product_ties(), [s for s, c in K.halfway() if c == 2], K.below_power_of_two()))
    t, h, p = _TIES
    return ("%s\t%s\t%s\n" % (t[(3 * i + 1) % len(t)], h[(7 * i) % len(h)], p[i % 130])).encode()


def _staging_text(r, span):
    """Workgroup 0: 256 lines of r (mod 16) bytes in all; workgroup 1: 256 lines whose span from line_start[256] & ~15 is
    `span`, its first and last lines class-2 ties; workgroup 2: a short tail."""
    rng = random.Random(16 * span + r)
    wg0 = bytearray(b"".join(_line(rng, k) for k in range(TT - 1)))
    body = b"1.25\t-0\t7"
    wg0 += body + b" " * ((r - len(wg0) - len(body) - 1) % 16) + b"\n"
    assert len(wg0) % 16 == r
    room = span - r                                              # the bytes of workgroup 1
    ls = [_class2_line(r)] + [_line(rng, k) for k in range(TT - 2)] + [_class2_line(r + 16)]
    spare = room - sum(len(x) for x in ls)
    assert spare >= 2 * TT
    out = bytearray()
    for k, ln in enumerate(ls):
        p = spare // TT + (k < spare % TT)                       # blanks behind the third number, then an ignored field
        term = ln[len(ln.rstrip(b"\r\n")):]
        out += ln[:len(ln) - len(term)] + b" " * (p // 3) + b"\t" + b"z" * (p - p // 3 - 1) + term
    assert len(out) == room
    text = bytes(wg0 + out) + b"".join(_line(rng, k) for k in range(5))
    st = _starts(text)
    assert len(st) == 2 * TT + 5 + 1 and st[2 * TT] - (st[TT] & ~15) == span and st[TT] & 15 == r
    return text


@pytest.mark.parametrize("delta", [-1, 0, 1])
def test_staging_boundary(vcp_ctx, delta):
    """A workgroup whose span is STAGE_BYTES - 1, STAGE_BYTES (both staged) or STAGE_BYTES + 1 (read from global memory),
    at each of the sixteen residues of line_start[j0] & 15."""
    for r in range(16):
        text = _staging_text(r, STAGE_BYTES + delta)
        held(vcp_ctx, text, n_host=0)


def test_staged_and_unstaged_workgroups_alternate(vcp_ctx):
    """About 2 000 lines: the lines of every other workgroup carry 150 to 400 bytes (256 of them exceed STAGE_BYTES),
    the others are plain, so that one launch holds both kinds side by side."""
    rng = random.Random(41)
    ls = []
    for k in range(2000):
        ln = _class2_line(k) if k % 5 == 0 else _line(rng, k)
        if (k // TT) % 2:
            term = ln[len(ln.rstrip(b"\r\n")):]
            p = rng.randint(150, 400) - len(ln)
            ln = ln[:len(ln) - len(term)] + b" " * (p // 4) + b"\t" + b"y" * (p - p // 4 - 1) + term
        ls.append(ln)
    text = b"".join(ls)
    st = _starts(text)
    spans = [st[min(j + TT, 2000)] - (st[j] & ~15) for j in range(0, 2000, TT)]
    kinds = [s <= STAGE_BYTES for s in spans]
    assert kinds == [k % 2 == 0 for k in range(len(spans))]
    held(vcp_ctx, text, n_host=0)


# ---- the indexing kernels at lane (64 bytes), wave (4 096) and chunk boundaries ---------------------------------------
@pytest.mark.parametrize("term", [b"\n", b"\r\n", b"\r"])
def test_terminator_on_lane_wave_and_chunk_boundaries(vcp_ctx, term):
    for edge in (64, 4096, CHUNK):
        for at in range(edge - 2, edge + 3):                     # the terminator's first byte
            rng = random.Random(at)
            buf = _pad_line(_fill(bytearray(), rng, at), at + len(term), term)
            assert buf[at:at + len(term)] == term and buf[at - 1:at] not in (b"\r", b"\n")
            text = bytes(buf) + b"".join(_line(rng, k) for k in range(3)) + b"9\t8\t7\n"
            held(vcp_ctx, text, n_host=0)


def test_texts_of_exactly_a_lane_and_a_chunk(vcp_ctx):
    for nbytes in (63, 64, 65, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK):
        for term in (b"\n", b"\r\n"):
            rng = random.Random(nbytes)
            text = bytes(_pad_line(_fill(bytearray(), rng, nbytes), nbytes, term))
            assert len(text) == nbytes
            held(vcp_ctx, text, n_host=0)
            cnt = vcp_ctx.parse_scan_text(text, count_only=True)
            assert cnt["n"] == len(_split(text))


def test_unsupported_byte_at_lane_and_chunk_boundaries(vcp_ctx):
    rng = random.Random(12)
    wide = lambda k: b"1.25\t-0\t7\t" + b"z" * k + b"\n"         # an ignored fourth field of k bytes
    buf = bytearray(wide(100))
    buf = _fill(buf, rng, CHUNK - 64) + wide(200)
    buf = _fill(buf, rng, 2 * CHUNK + 3000)
    buf += wide(100 + (20 - (len(buf) + 111)) % 64)
    text = bytes(buf)
    nbytes = len(text)
    assert nbytes % 64 == 20 and nbytes > 2 * CHUNK
    held(vcp_ctx, text, n_host=0)
    last_lane = nbytes // 64 * 64 + 3
    for at in (0, 63, 64, CHUNK - 1, CHUNK, nbytes - 2, last_lane):
        assert at == 0 or text[at:at + 1] == b"z"
        for second in (None, nbytes - 2):
            if second is not None and second // CHUNK <= at // CHUNK:
                continue
            t = bytearray(text)
            t[at] = 0x85
            if second is not None:
                t[second] = 0x7F
            with pytest.raises(N.VcpError) as e:
                vcp_ctx.parse_scan_text(bytes(t))
            assert e.value.code == -8 and e.value.err[0] == at, (at, second, e.value.err)
            assert R.supported(t[:at]) and not R.supported(t[:at + 1])


# ---- the host list and the segments at size --------------------------------------------------------------------------
def _host_line(i):
    three = ("1e400", "-1e-400", "nan", "-inf", "%d" % (10 ** 24 + 7919 * i), "%de-320" % (i + 1), "-1e%d" % (400 + i),
             "0.%030d" % (i + 1))[i % 8]
    f = ["%d.5" % i, "-%d.25e-3" % i, "%d" % (7 * i)]
    f[i % 3] = three
    assert R.field_class(three)[0] == 3
    return "\t".join(f).encode() + (b"\n", b"\r\n", b"\r")[i % 3]


def test_a_thousand_host_lines(vcp_ctx):
    host = [_host_line(i) for i in range(1000)]
    text = b"".join(host)
    got = held(vcp_ctx, text, n_host=1000)
    assert len(np.unique(u64(got["rows"]), axis=0)) == 1000
    rng = random.Random(77)
    mixed = b"".join(b"".join(_line(rng, 3 * i + k) for k in range(3)) + host[i] for i in range(1000))
    held(vcp_ctx, mixed, n_host=1000)


def test_a_thousand_segments(vcp_ctx):
    rng = random.Random(1000)
    segs = []
    for k in range(1000):
        n = 0 if (k < 4 or k >= 990 or rng.random() < 0.32) else rng.randint(1, 5)
        if k == 700:
            n = 3
        s = b"".join(_host_line(rng.randrange(1000)) if rng.random() < 0.05 else _line(rng, rng.randrange(3)) for _ in range(n))
        if n and rng.random() < 0.3:
            s = s.rstrip(b"\r\n") + rng.choice((b"", b"\r"))         # the wrapper appends the '\n'
        segs.append(s)
    assert 250 < sum(not s for s in segs) < 450
    want = [vio._rows_from_bytes(s, "segment %d" % k) for k, s in enumerate(segs)]
    counts = [len(w) for w in want]
    text, seg_off = vio._join_segments(segs)
    for resident in (False, True):
        got = vio.parse_scan_text(segs, resident=resident, ctx=vcp_ctx)
        rows, group = (got[k].cpu().numpy() if resident else got[k] for k in ("rows", "group"))
        bad = _difference(text, rows, np.concatenate(want))
        assert bad is None, bad
        assert group.tolist() == [k for k, c in enumerate(counts) for _ in range(c)]
        assert got["seg_first"].tolist() == [0] + np.cumsum(counts).tolist() and got["n"] == sum(counts)
        assert got["n_host"] == _host_lines(text)
    cnt = vcp_ctx.parse_scan_text(text, seg_off, count_only=True)
    assert cnt["n"] == got["n"] and cnt["seg_first"].tolist() == got["seg_first"].tolist()
    lines700 = _split(segs[700])
    segs[700] = lines700[0] + b"\n" + b"1\tx\t3\n" + lines700[2] + b"\n"
    with pytest.raises(N.VcpError) as e:
        vcp_ctx.parse_scan_text(*vio._join_segments(segs))
    assert e.value.code == -1 and e.value.err == (2, 700, 2)
    with pytest.raises(vio.ScanTextError) as e:
        vio.parse_scan_text(segs, ctx=vcp_ctx)
    with pytest.raises(ValueError) as w:
        vio._rows_from_bytes(segs[700], "segment 700")
    assert str(e.value) == str(w.value)


def test_bounded_fuzz(vcp_ctx):
    """tests/fuzz_scantext.py: SUITE cases; what the list covers is asserted in tests/test_scantext.py as well."""
    import fuzz_scantext as F
    from test_scantext import fuzz_covers
    count, seed = F.SUITE
    lst = F.cases(count, seed)
    s = F.summary(lst, [F.check(vcp_ctx, c) for c in lst])
    print(s)
    assert fuzz_covers(s, count), s
