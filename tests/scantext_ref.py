"""The field grammar and the class rule of vcp_parse_scan_text (include/vcp.h), restated in Python: float() gives the
value, integers give w, nd and e10.  Not a test file: tests/test_scantext.py and tests/test_scantext_gpu.py import it."""
import re
import struct

NUMBER = re.compile(r" *([+-]?)(?:(\d+)(?:\.(\d*))?|\.(\d+))(?:[eE]([+-]?\d+))? *\Z")
NAME = re.compile(r" *[+-]?(?:inf|infinity|nan) *\Z", re.I)


def supported(data):
    """True when every byte is \\t \\n \\r or 0x20..0x7E without '_'."""
    return all(b in (9, 10, 13) or (0x20 <= b <= 0x7E and b != 0x5F) for b in data)


def field_class(s):
    """(class, value): class 0..3 by the contract's rule, value = float(s) (None for class 0)."""
    if NAME.match(s):
        return 3, float(s)
    m = NUMBER.match(s)
    if not m:
        try:
            float(s)
        except ValueError:
            return 0, None
        raise AssertionError("float() takes %r, the grammar does not" % s)
    _, ip, fp, fp2, ex = m.groups()
    ip, fp = (ip or ""), (fp if fp is not None else (fp2 or ""))
    digits = (ip + fp).lstrip("0")
    w, nd = (int(digits) if digits else 0), len(digits)
    e10 = int(ex or 0) - len(fp)
    v = float(s)
    if w == 0 or (w <= 2 ** 53 and -22 <= e10 <= 22):
        return 1, v
    if nd <= 19 and -19 <= e10 <= 19:
        return 2, v
    return 3, v


def bits(v):
    return struct.unpack("<Q", struct.pack("<d", v))[0]


def nan_bits(s):
    """CPython's float('nan') / float('-nan'): the quiet NaN with the sign of the text."""
    return 0xFFF8000000000000 if s.strip().startswith("-") else 0x7FF8000000000000


def value_bits(s, v):
    return nan_bits(s) if v != v else bits(v)
