"""vcp_selftest_parse_field (the __host__ __device__ source of csrc/scantext.hpp, run on the host: no GPU) against
tests/scantext_ref.py: the class AND the bits of the value of every field; and the host-only part of
io.read_folder_resident, the batching of files and the cuts at line ends."""
import random

import pytest

import scantext_corpus as K
import scantext_ref as R
from vtkcloudpoint_amd import _native as N


def check(s):
    want_c, want_v = R.field_class(s)
    got_c, got_v = N.selftest_parse_field(s)
    assert got_c == want_c, (s, got_c, want_c)
    if want_c:
        assert R.value_bits(s, got_v) == R.value_bits(s, want_v), (s, got_v, want_v)
    return want_c


@pytest.mark.parametrize("s", K.EDGE)
def test_edge_list(s):
    check(s)


def test_edge_classes_as_stated():
    """The classes of the edge list by hand, so that a reference that called everything class 0 would not pass."""
    assert sorted(K.EDGE_CLASSES) == sorted(K.EDGE)
    for s, c in K.EDGE_CLASSES.items():
        assert R.field_class(s)[0] == c and N.selftest_parse_field(s)[0] == c, s
    assert R.bits(N.selftest_parse_field("-0")[1]) == 0x8000000000000000
    assert R.bits(N.selftest_parse_field("nan")[1]) == 0x7FF8000000000000
    assert R.bits(N.selftest_parse_field("+NaN")[1]) == 0x7FF8000000000000
    assert R.bits(N.selftest_parse_field("-nan")[1]) == 0xFFF8000000000000


def test_class_boundaries():
    cases = K.boundaries()
    assert len(cases) == 29
    for s, c in cases.items():
        assert check(s) == c, s


def test_halfway_cases_of_binary64():
    """Decimal strings of at most 19 digits that lie exactly between two neighbouring doubles, and their neighbours one
    unit of the last digit away: ties to even, and the sticky bit of the division."""
    n = 0
    for s, c in K.halfway():
        assert check(s) == c, s
        n += 1
    assert n >= 60


def test_long_and_extreme_fields():
    cases = K.long_and_extreme()
    assert len(cases) == 18 and cases[0] == ("0" * 400 + "1.5", 1) and sum(c == 3 for _, c in cases) == 16
    for s, c in cases:
        assert check(s) == c, s


def test_random_w_e_strings():
    """200 000 seeded "<w>e<e>" strings with 1 to 19 digits and |e| <= 19."""
    strings = K.random_w_e()
    assert len(strings) == 200000
    seen = {1: 0, 2: 0}
    for s in strings:
        seen[check(s)] += 1
    assert seen[1] > 100000 and seen[2] > 20000       # 17 to 19 digits are class 2: 3 lengths of 19


def test_random_17_to_19_digit_strings():
    """The class-2 share of the family above is one in six; 50 000 more with 17 to 19 digits, as repr and %.18e write
    them (a point inside the digits)."""
    strings = K.random_17_to_19_digits()
    assert len(strings) == 50000
    n2 = 0
    for s in strings:
        n2 += check(s) == 2
    assert n2 > 45000


def test_f6_strings():
    """20 000 strings of the form the reference writes ("F6"): all class 1."""
    strings = K.f6()
    assert len(strings) == 20000
    for s in strings:
        assert check(s) == 1


def test_just_below_a_power_of_two():
    """2^k * (1 - 2^-55), k = -3 .. 126, in 19 digits: class 2, and the rounding carries out of the mantissa to 2^k."""
    strings = K.below_power_of_two()
    assert len(strings) == 130
    for k, s in zip(range(-3, 127), strings):
        assert check(s) == 2, s
        assert R.bits(N.selftest_parse_field(s)[1]) == (k + 1023) << 52, s
        assert R.bits(N.selftest_parse_field("-" + s)[1]) == 1 << 63 | (k + 1023) << 52, s


def test_ties_on_the_product_path():
    """w * 10^z exactly between two doubles, and w - 1, w + 1: the exact 128-bit product and the tie rule."""
    strings = K.product_ties()
    assert len(strings) >= 1000 and len(strings) % 3 == 0
    for i in range(0, len(strings), 3):
        below, tie, above = (N.selftest_parse_field(s)[1] for s in strings[i:i + 3])
        assert all(check(s) == 2 for s in strings[i:i + 3])
        assert R.bits(above) - R.bits(below) == 1 and R.bits(tie) % 2 == 0, strings[i + 1]     # neighbours; the even one


def test_census_of_the_corpus():
    """What tests/test_scantext_gpu.py hands the device: it cannot pass by being empty-handed."""
    fields = K.value_fields()
    assert len(set(fields)) == len(fields) and all(R.field_class(s)[0] in (1, 2, 3) for s in fields)
    c = K.census(fields)
    print(len(fields), sorted(c.items()))
    for cell in ((1, 1), (1, -1), (2, 1), (2, -1)):
        assert c[cell] >= 40000, (cell, c[cell])
    ties = K.product_ties()
    assert len(ties) >= 1000 and K.census(ties) == {(2, 1): len(ties)}
    assert all(R.NUMBER.match(s).group(5) in "1234567" for s in ties)                 # e10 > 0
    assert len(K.below_power_of_two()) == 130 and set(K.census(K.below_power_of_two())) <= {(2, 1), (2, -1)}
    inside = set(fields)
    assert all(s in inside for s in ties) and all(s in inside for s in K.below_power_of_two())
    assert all((s in inside) == (c0 != 0) for s, c0 in K.EDGE_CLASSES.items())
    text = K.lines(fields)
    assert text.count(b"\n") == (len(fields) + 2) // 3 and text.endswith(b"\n") and R.supported(text)
    back = [f.decode() for ln in text.split(b"\n")[:-1] for f in ln.split(b"\t")]
    assert back[:len(fields)] == fields and all(f == "1" for f in back[len(fields):])


def fuzz_covers(s, count):
    """The conditions on fuzz_scantext.summary, for this file and for the bounded sweep of tests/test_scantext_gpu.py."""
    return (s["cases"] == count and all(s["defects"][d] >= 1 for d in ("few", "class0", "byte", "both"))
            and s["no_line"] >= 1 and s["over_stage"] >= 1 and s["many_segments"] >= 1 and s["class2_pos"] >= 1
            and s["class2_neg"] >= 1 and s["host_lines"] >= 1)


def test_the_fuzz_list_is_a_function_of_the_seed_and_not_empty_handed():
    import os
    import re
    import fuzz_scantext as F
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "vcp.h")) as f:
        assert re.search(r"^#define VCP_TXT_CHUNK %d\b" % F.CHUNK, f.read(), flags=re.M)
    with open(os.path.join(root, "vtkcloudpoint_amd", "csrc", "scantext.hip")) as f:
        assert re.search(r"^constexpr int STAGE_BYTES = %d;" % F.STAGE_BYTES, f.read(), flags=re.M)
    count, seed = F.SUITE
    lst = F.cases(count, seed)
    assert lst == F.cases(count, seed) and lst != F.cases(count, seed + 1)
    s = F.summary(lst, [F.expect(c) for c in lst])
    print(s)
    assert fuzz_covers(s, count), s
    assert 0 < s["resident"] < count


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
