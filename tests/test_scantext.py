"""vcp_selftest_parse_field (the __host__ __device__ source of csrc/scantext.hpp, run on the host: no GPU) against
tests/scantext_ref.py: the class AND the bits of the value of every field; and the host-only part of
io.read_folder_resident, the batching of files and the cuts at line ends."""
import random

import pytest

import scantext_ref as R
from vtkcloudpoint_amd import _native as N


def check(s):
    want_c, want_v = R.field_class(s)
    got_c, got_v = N.selftest_parse_field(s)
    assert got_c == want_c, (s, got_c, want_c)
    if want_c:
        assert R.value_bits(s, got_v) == R.value_bits(s, want_v), (s, got_v, want_v)
    return want_c


EDGE = ["1.", ".5", "+.5e-3", " 1 ", "-0", "1e", ".", "e5", "+ 1", "", "  ", "INF", "-Infinity", "-nan", "0x10", "1d5",
        "1,5"]


@pytest.mark.parametrize("s", EDGE)
def test_edge_list(s):
    check(s)


def test_edge_classes_as_stated():
    """The classes of the edge list by hand, so that a reference that called everything class 0 would not pass."""
    want = {"1.": 1, ".5": 1, "+.5e-3": 1, " 1 ": 1, "-0": 1, "1e": 0, ".": 0, "e5": 0, "+ 1": 0, "": 0, "  ": 0, "INF": 3,
            "-Infinity": 3, "-nan": 3, "0x10": 0, "1d5": 0, "1,5": 0}
    for s, c in want.items():
        assert R.field_class(s)[0] == c and N.selftest_parse_field(s)[0] == c, s
    assert R.bits(N.selftest_parse_field("-0")[1]) == 0x8000000000000000
    assert R.bits(N.selftest_parse_field("nan")[1]) == 0x7FF8000000000000
    assert R.bits(N.selftest_parse_field("+NaN")[1]) == 0x7FF8000000000000
    assert R.bits(N.selftest_parse_field("-nan")[1]) == 0xFFF8000000000000


def test_class_boundaries():
    p53 = 2 ** 53
    cases = {
        str(p53): 1, str(p53 + 1): 2, "%de22" % p53: 1, "%de23" % p53: 3, "%de-22" % p53: 1, "%de-23" % p53: 3,
        "1e22": 1, "1e23": 3, "1e-22": 1, "1e-23": 3, "3e19": 1, "3e-19": 1,
        "9" * 19: 2, "9" * 20: 3, "1" + "0" * 19: 3, "9" * 19 + "e19": 2, "9" * 19 + "e20": 3, "9" * 19 + "e-19": 2,
        "9" * 19 + "e-20": 3, "0." + "9" * 19: 2, "0.0" + "9" * 19: 3, str(p53 + 1) + "e19": 2, str(p53 + 1) + "e-19": 2,
        str(p53 + 1) + "e20": 3, "0e999999999999999999999": 1, "-0.000e-5": 1, "1.e5": 1, "1.E+05": 1, "00012.500": 1,
    }
    for s, c in cases.items():
        assert check(s) == c, s


def test_halfway_cases_of_binary64():
    """Decimal strings of at most 19 digits that lie exactly between two neighbouring doubles, and their neighbours one
    unit of the last digit away: ties to even, and the sticky bit of the division."""
    n = 0
    for m in (2 ** 53 + 1, 2 ** 53 + 3, 2 ** 54 + 2, 2 ** 54 + 6, 2 ** 60 + 2 ** 7, 2 ** 60 + 3 * 2 ** 7, 2 ** 63 + 2 ** 10,
              2 ** 63 + 3 * 2 ** 10):
        for d in (-1, 0, 1):
            assert check(str(m + d)) == (1 if m + d <= 2 ** 53 else 2)
            n += 1
    # m + 1/2 for odd and even m of 53 bits, written exactly: (2m + 1) * 5^k / 10^k with k fraction digits
    for m in (2 ** 52 + 1, 2 ** 52 + 2, 2 ** 52 + 12345, 2 ** 53 - 2):
        for sh in (1, 2, 3, 4, 5):                 # the tie at m + 1/2 scaled by 2^-sh: sh + 1 fraction digits
            num = (2 * m + 1) * 5 ** (sh + 1)      # value = num / 10^(sh + 1), exactly (2m + 1) / 2^(sh + 1)
            s = str(num)
            if len(s) > 19:
                continue
            for d in (-1, 0, 1):
                t = str(num + d)
                assert check(t[:-(sh + 1)] + "." + t[-(sh + 1):]) == 2
                assert check(t + "e-%d" % (sh + 1)) == 2
                n += 2
    assert n >= 60


def test_long_and_extreme_fields():
    assert check("0" * 400 + "1.5") == 1
    assert check("0." + "0" * 400 + "15") == 3
    assert check("0" * 400) == 1
    for s in ("1e400", "1e-400", "-1e400", "-1e-400", "4.9e-324", "2.4703282292062327e-324", "2.4703282292062328e-324",
              "2.2250738585072011e-308", "1.7976931348623157e308", "1.7976931348623159e308", "17976931348623157" + "0" * 292,
              "1" + "0" * 30, "123456789012345678901234567890", "0.1" + "0" * 30 + "1", "9007199254740993.00000000000000001"):
        assert check(s) == 3, s


def test_random_w_e_strings():
    """200 000 seeded "<w>e<e>" strings with 1 to 19 digits and |e| <= 19."""
    rng = random.Random(20240611)
    seen = {1: 0, 2: 0}
    for _ in range(200000):
        nd = rng.randint(1, 19)
        w = rng.randint(10 ** (nd - 1), 10 ** nd - 1)
        seen[check("%de%d" % (w, rng.randint(-19, 19)))] += 1
    assert seen[1] > 100000 and seen[2] > 20000       # 17 to 19 digits are class 2: 3 lengths of 19


def test_random_17_to_19_digit_strings():
    """The class-2 share of the family above is one in six; 50 000 more with 17 to 19 digits, as repr and %.18e write
    them (a point inside the digits)."""
    rng = random.Random(99)
    n2 = 0
    for _ in range(50000):
        nd = rng.randint(17, 19)
        w = str(rng.randint(10 ** (nd - 1), 10 ** nd - 1))
        e = rng.randint(-19, 19) + (nd - 1)
        n2 += check("%s.%se%+03d" % (w[0], w[1:], e)) == 2
    assert n2 > 45000


def test_f6_strings():
    """20 000 strings of the form the reference writes ("F6"): all class 1."""
    rng = random.Random(7)
    for _ in range(20000):
        v = rng.choice((rng.uniform(-360, 360), rng.uniform(0, 1000), rng.uniform(-1e6, 1e6)))
        assert check("%.6f" % v) == 1


def test_argument_errors():
    import ctypes as C
    lib = N.lib()
    v = C.c_double(0)
    assert lib.vcp_selftest_parse_field(b"1", C.c_int64(1), None) == -1
    assert lib.vcp_selftest_parse_field(None, C.c_int64(1), C.byref(v)) == -1
    assert lib.vcp_selftest_parse_field(b"1", C.c_int64(-1), C.byref(v)) == -1
    assert lib.vcp_selftest_parse_field(None, C.c_int64(0), C.byref(v)) == 0


def test_folder_batches_cut_at_line_ends(tmp_path):
    """io._batches / io._load_batch (host only): whatever the batch limit, the pieces of a file put together parse to the
    file's rows, no cut falls between a '\\r' and its '\\n', no batch exceeds the limit, and a piece knows how many lines
    of its file precede it."""
    import numpy as np
    from vtkcloudpoint_amd import io as vio
    rng = random.Random(5)
    paths, want = [], []
    for k, n in enumerate((0, 1, 60, 7)):
        lines = [b"%d\t%d.5\t%d" % (k, i, rng.randint(0, 10 ** rng.randint(1, 12))) + rng.choice((b"\n", b"\r\n", b"\r"))
                 for i in range(n)]
        data = b"".join(lines)
        if k == 3:
            data = data.rstrip(b"\r\n")                          # a file without a final terminator
        p = tmp_path / ("f%d.txt" % k)
        p.write_bytes(data)
        paths.append(str(p))
        want.append(vio.read_scan_text(str(p)))
    for max_bytes in (1 << 20, 400, 97, 64):
        got = [[] for _ in paths]
        for batch in vio._batches(paths, max_bytes):
            text, seg_off = vio._load_batch(batch, paths)
            assert len(text) <= max_bytes and seg_off[-1] == len(text) and len(seg_off) == len(batch) + 1
            for i, (k, _, line0, _) in enumerate(batch):
                piece = text[int(seg_off[i]):int(seg_off[i + 1])].tobytes()
                assert piece == b"" or piece.endswith(b"\n")
                assert line0 == sum(len(g) for g in got[k])
                got[k].append(vio._rows_from_bytes(piece, paths[k], line0))
        for k in range(len(paths)):
            rows = np.concatenate(got[k]) if got[k] else np.zeros((0, 3))
            assert np.array_equal(rows.view(np.uint64), want[k].view(np.uint64)), (k, max_bytes)
    with pytest.raises(ValueError, match="a line longer than"):
        list(vio._batches(paths, 8))
    text, seg_off = vio._join_segments([b"a\r", b"", b"b\n", b"c"])
    assert text == b"a\r\nb\nc\n" and seg_off.tolist() == [0, 3, 3, 5, 7]
