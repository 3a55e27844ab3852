"""The field strings that hold the decimal-to-binary64 conversion of csrc/scantext.hpp to float(), as generator functions
with fixed seeds: tests/test_scantext.py runs them through the host compile of that source (vcp_selftest_parse_field),
tests/test_scantext_gpu.py packs the same strings into lines and runs them through the device compile (both forms of
k_txt_parse).  Not a test file.  Everything here is integers, fractions and float(): no GPU, no library."""
import random
from fractions import Fraction

import scantext_ref as R

P53 = 2 ** 53

EDGE = ["1.", ".5", "+.5e-3", " 1 ", "-0", "1e", ".", "e5", "+ 1", "", "  ", "INF", "-Infinity", "-nan", "0x10", "1d5",
        "1,5"]

# the classes of the edge list by hand, so that a reference that called everything class 0 would not pass
EDGE_CLASSES = {"1.": 1, ".5": 1, "+.5e-3": 1, " 1 ": 1, "-0": 1, "1e": 0, ".": 0, "e5": 0, "+ 1": 0, "": 0, "  ": 0,
                "INF": 3, "-Infinity": 3, "-nan": 3, "0x10": 0, "1d5": 0, "1,5": 0}

# Strings on which the device build once differed from the host build, by name.  None so far.
NAMED = []                                   # (name, string)


def boundaries():
    """{string: class}: 2^53 and 2^53 + 1, |e10| = 22 / 23 and 19 / 20, 19 and 20 digits."""
    return {
        str(P53): 1, str(P53 + 1): 2, "%de22" % P53: 1, "%de23" % P53: 3, "%de-22" % P53: 1, "%de-23" % P53: 3,
        "1e22": 1, "1e23": 3, "1e-22": 1, "1e-23": 3, "3e19": 1, "3e-19": 1,
        "9" * 19: 2, "9" * 20: 3, "1" + "0" * 19: 3, "9" * 19 + "e19": 2, "9" * 19 + "e20": 3, "9" * 19 + "e-19": 2,
        "9" * 19 + "e-20": 3, "0." + "9" * 19: 2, "0.0" + "9" * 19: 3, str(P53 + 1) + "e19": 2, str(P53 + 1) + "e-19": 2,
        str(P53 + 1) + "e20": 3, "0e999999999999999999999": 1, "-0.000e-5": 1, "1.e5": 1, "1.E+05": 1, "00012.500": 1,
    }


def halfway():
    """[(string, class)]: decimal strings of at most 19 digits that lie exactly between two neighbouring doubles, and
    their neighbours one unit of the last digit away: ties to even, and the sticky bit of the division."""
    out = []
    for m in (2 ** 53 + 1, 2 ** 53 + 3, 2 ** 54 + 2, 2 ** 54 + 6, 2 ** 60 + 2 ** 7, 2 ** 60 + 3 * 2 ** 7, 2 ** 63 + 2 ** 10,
              2 ** 63 + 3 * 2 ** 10):
        for d in (-1, 0, 1):
            out.append((str(m + d), 1 if m + d <= 2 ** 53 else 2))
    # m + 1/2 for odd and even m of 53 bits, written exactly: (2m + 1) * 5^k / 10^k with k fraction digits
    for m in (2 ** 52 + 1, 2 ** 52 + 2, 2 ** 52 + 12345, 2 ** 53 - 2):
        for sh in (1, 2, 3, 4, 5):                 # the tie at m + 1/2 scaled by 2^-sh: sh + 1 fraction digits
            num = (2 * m + 1) * 5 ** (sh + 1)      # value = num / 10^(sh + 1), exactly (2m + 1) / 2^(sh + 1)
            s = str(num)
            if len(s) > 19:
                continue
            for d in (-1, 0, 1):
                t = str(num + d)
                out.append((t[:-(sh + 1)] + "." + t[-(sh + 1):], 2))
                out.append((t + "e-%d" % (sh + 1), 2))
    return out


def long_and_extreme():
    """[(string, class)]: hundreds of leading zeros, and the numbers only the host reads."""
    out = [("0" * 400 + "1.5", 1), ("0." + "0" * 400 + "15", 3), ("0" * 400, 1)]
    for s in ("1e400", "1e-400", "-1e400", "-1e-400", "4.9e-324", "2.4703282292062327e-324", "2.4703282292062328e-324",
              "2.2250738585072011e-308", "1.7976931348623157e308", "1.7976931348623159e308", "17976931348623157" + "0" * 292,
              "1" + "0" * 30, "123456789012345678901234567890", "0.1" + "0" * 30 + "1", "9007199254740993.00000000000000001"):
        out.append((s, 3))
    return out


def random_w_e():
    """200 000 seeded "<w>e<e>" strings with 1 to 19 digits and |e| <= 19."""
    rng = random.Random(20240611)
    out = []
    for _ in range(200000):
        nd = rng.randint(1, 19)
        w = rng.randint(10 ** (nd - 1), 10 ** nd - 1)
        out.append("%de%d" % (w, rng.randint(-19, 19)))
    return out


def random_17_to_19_digits():
    """50 000 seeded strings with 17 to 19 digits, as repr and %.18e write them (a point inside the digits)."""
    rng = random.Random(99)
    out = []
    for _ in range(50000):
        nd = rng.randint(17, 19)
        w = str(rng.randint(10 ** (nd - 1), 10 ** nd - 1))
        e = rng.randint(-19, 19) + (nd - 1)
        out.append("%s.%se%+03d" % (w[0], w[1:], e))
    return out


def f6():
    """20 000 seeded strings of the form the reference writes ("F6"): all class 1."""
    rng = random.Random(7)
    out = []
    for _ in range(20000):
        v = rng.choice((rng.uniform(-360, 360), rng.uniform(0, 1000), rng.uniform(-1e6, 1e6)))
        out.append("%.6f" % v)
    return out


def below_power_of_two():
    """130 strings "<w>e<e10>": 2^k * (1 - 2^-55) for k = -3 .. 126, floored to 19 significant digits.  All are class 2
    (w >= 10^18 > 2^53, |e10| <= 19), and each lies above the midpoint 2^k * (1 - 2^-54) of 2^k and the double below it,
    so it rounds to 2^k exactly: the 53 bits kept are all ones and the rounding carries out of the mantissa."""
    out = []
    for k in range(-3, 127):
        x = Fraction(2) ** k * (1 - Fraction(1, 2 ** 55))
        e10 = -19
        while x / Fraction(10) ** e10 >= 10 ** 19:
            e10 += 1
        w = int(x / Fraction(10) ** e10)                       # floor: x > 0
        s = "%de%d" % (w, e10)
        assert 10 ** 18 <= w < 10 ** 19 and -19 <= e10 <= 19, s
        assert w > P53 and R.field_class(s)[0] == 2, s
        v = w * Fraction(10) ** e10
        assert Fraction(2) ** k * (1 - Fraction(1, 2 ** 54)) < v < Fraction(2) ** k, s
        assert float(s) == 2.0 ** k and R.bits(float(s)) == (k + 1023) << 52, s
        out.append(s)
    assert len(out) == 130
    return out


def product_ties():
    """Exact ties on the product path of class 2 (e10 > 0): for z = 1 .. 7, twenty seeded odd t such that 5^z * t has
    exactly 54 bits; for every a with w = t * 2^a > 2^53 and at most 19 digits, "<w + d>e<z>" for d = -1, 0, 1.
    w * 10^z = (5^z * t) * 2^(a + z) has 54 significant bits, the lowest of them set: it lies exactly between two
    neighbouring doubles, and its neighbours one unit of w away fall on either side."""
    out = []
    for z in range(1, 8):
        rng = random.Random(5400 + z)
        lo, hi = -(-2 ** 53 // 5 ** z), (2 ** 54 - 1) // 5 ** z          # 2^53 <= 5^z * t < 2^54
        ts = set()
        while len(ts) < 20:
            t = rng.randint(lo, hi) | 1
            if t <= hi and (5 ** z * t).bit_length() == 54:
                ts.add(t)
        for t in sorted(ts):
            a = 0
            while t << a < 10 ** 19:
                w = t << a
                a += 1
                if w <= P53:
                    continue
                n = w * 10 ** z
                assert n.bit_length() - ((n & -n).bit_length() - 1) == 54, (t, a, z)      # 54 significant bits: a tie
                for d in (-1, 0, 1):
                    s = "%de%d" % (w + d, z)
                    assert w + d > P53 and len(str(w + d)) <= 19 and R.field_class(s)[0] == 2, s
                    out.append(s)
    return out


def families():
    """[(name, [strings])], in the order of the list in tests/test_scantext.py; class-0 strings included."""
    return [("edge", list(EDGE)), ("named", [s for _, s in NAMED]), ("boundaries", list(boundaries())),
            ("halfway", [s for s, _ in halfway()]), ("long_and_extreme", [s for s, _ in long_and_extreme()]),
            ("random_w_e", random_w_e()), ("random_17_to_19_digits", random_17_to_19_digits()), ("f6", f6()),
            ("below_power_of_two", below_power_of_two()), ("product_ties", product_ties())]


_VALUE_FIELDS = None


def value_fields():
    """Every string above whose class is 1, 2 or 3, each once, in the order of families().  Computed once and shared:
    treat the list as read-only."""
    global _VALUE_FIELDS
    if _VALUE_FIELDS is None:
        seen, out = set(), []
        for _, strings in families():
            for s in strings:
                if s not in seen and R.field_class(s)[0] != 0:
                    seen.add(s)
                    out.append(s)
        _VALUE_FIELDS = out
    return _VALUE_FIELDS


def lines(fields):
    """The fields three to a line, round-robin over the three positions (field i is field i % 3 of line i // 3), every
    line '\\n'-terminated; a last line that is short of fields is filled with "1"."""
    fields = list(fields) + ["1"] * (-len(fields) % 3)
    return "".join("%s\t%s\t%s\n" % tuple(fields[i:i + 3]) for i in range(0, len(fields), 3)).encode("ascii")


def census(fields):
    """{(class, sign of e10): count} by the restatement; the sign is 1 for e10 >= 0 and -1 below, 0 for the names."""
    out = {}
    for s in fields:
        c = R.field_class(s)[0]
        m = R.NUMBER.match(s)
        if m:
            _, _, fp, fp2, ex = m.groups()
            e10 = int(ex or 0) - len(fp if fp is not None else (fp2 or ""))
            key = (c, 1 if e10 >= 0 else -1)
        else:
            key = (c, 0)
        out[key] = out.get(key, 0) + 1
    return out
