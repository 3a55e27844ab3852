"""vcp_parse_scan_text on the MI355X against io.read_scan_text on a temporary file: rows by their bits (NaN signs and -0
count), group, seg_first, n, n_host, the three errors with read_scan_text's own ValueError text, the fallback, count-only,
independence from the context's history, read_folder_resident and the caller's stream -- on the smallest texts at which
each mechanism can go wrong (a chunk is VCP_TXT_CHUNK = 16384 bytes, a parse workgroup 256 lines, its LDS span 32 KiB)."""
import random

import numpy as np
import pytest
import torch

import scantext_ref as R
from vtkcloudpoint_amd import _native as N
from vtkcloudpoint_amd import io as vio

pytestmark = pytest.mark.gpu

CHUNK = 16384


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
