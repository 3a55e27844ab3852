"""The corpus of the export formatter (csrc/scanfmt.hpp), built from a fixed seed: one list of supported binary64 values,
each formatted at every bit in 0..15, and the unsupported list.  The host compile (tests/test_scanfmt.py, through
vcp_selftest_format_field) and the device compile (tests/test_scanfmt_gpu.py, three values to a line through
vcp_format_rows) are held to the same strings: expected(v, bit) = '%.*f' % (bit, v), CPython's correctly rounded
fixed-point formatting (the exact binary value, ties to even).  census() counts what the corpus holds, with exact rational
arithmetic, and check_census() asserts it, so that no consumer passes empty-handed."""
import math
import random
from fractions import Fraction

SEED = 20260331
BITS = tuple(range(16))
LIMIT = 1e15                      # supported: finite and |v| < LIMIT
LINE_MAX = 112                    # include/vcp.h: VCP_FMT_LINE_MAX
FIELD_MAX = 32


def expected(v, bit):
    return ("%.*f" % (bit, v)).encode("ascii")


def _build():
    rng = random.Random(SEED)
    vals = []
    # exact ties at every bit: k / 2^(bit + 1), k odd, both signs, with the neighbours on both sides
    ks = [1, 3, 5, 7, 9, 11, 199, 201, 1999, 2001, 19999, 99999, 100001, 999999]
    for bit in BITS:
        mine = ks + [2 * rng.randrange(1 << 24) + 1 for _ in range(6)]
        for k in mine:
            t = k / 2.0 ** (bit + 1)
            for s in (t, -t):
                vals += [s, math.nextafter(s, math.inf), math.nextafter(s, -math.inf)]
    # 10^p and the value below it: the rounding adds a digit
    for p in range(-6, 16):
        x = float("1e%d" % p)
        for s in (x, math.nextafter(x, 0.0)):
            if s < LIMIT:
                vals += [s, -s]
    vals += [0.5, 1.5, 2.5, -0.5, -1.5, -2.5]
    vals += [0.0, -0.0, 5e-324, -5e-324, 2.2250738585072014e-308, -2.2250738585072014e-308]
    vals += [math.nextafter(LIMIT, 0.0), -math.nextafter(LIMIT, 0.0)]
    # values that carry at many bits: 9.99..., 99.99..., 0.99...
    for s in ("9.9999999", "99.99999999999", "0.9999999999999999", "999999.9999995", "99999999999999.99", "0.95", "0.5"):
        vals += [float(s), -float(s)]
    # seeded: uniform, random mantissas with small exponents, F6 strings read back
    vals += [rng.uniform(-1000.0, 1000.0) for _ in range(1500)]
    for _ in range(1500):
        v = math.ldexp(rng.getrandbits(53), rng.randrange(-1100, -2))
        if v < LIMIT:
            vals.append(v if rng.random() < 0.5 else -v)
    vals += [float("%.6f" % rng.uniform(-400.0, 1000.0)) for _ in range(1500)]
    while len(vals) % 3:
        vals.append(0.25)
    return vals


SUPPORTED = _build()
UNSUPPORTED = [1e15, -1e15, 1e300, float("nan"), float("inf"), float("-inf")]


def census():
    c = dict(supported=len(SUPPORTED), unsupported=len(UNSUPPORTED), ties={b: 0 for b in BITS}, carries=0,
             negative_zero=0, longest_field=0)
    for v in SUPPORTED:
        assert math.isfinite(v) and abs(v) < LIMIT
        fr = abs(Fraction(v))
        for bit in BITS:
            scaled = fr * 10 ** bit
            if scaled.denominator == 2:
                c["ties"][bit] += 1
            e = expected(v, bit)
            digits = e.lstrip(b"-").split(b".")[0]
            if int(digits) > math.floor(fr):
                c["carries"] += 1
            if e.startswith(b"-") and not e.strip(b"-0."):
                c["negative_zero"] += 1
            c["longest_field"] = max(c["longest_field"], len(e))
    return c


def check_census(c):
    assert c["supported"] >= 6000 and c["supported"] % 3 == 0 and c["unsupported"] == 6
    assert all(c["ties"][b] >= 40 for b in BITS), c["ties"]
    assert c["carries"] >= 200 and c["negative_zero"] >= 1000
    assert c["longest_field"] == FIELD_MAX
