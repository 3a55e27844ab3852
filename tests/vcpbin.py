"""The container host_check (vtkcloudpoint_amd/host/cpp/host_check.cpp) reads its cases from and writes its results to:
"VCPBIN1\\0", a uint32 record count, then per record a uint16 name length, the name (UTF-8), a uint8 dtype tag, a uint64
element count and the elements as raw little-endian bytes.  Doubles travel as their bits: NaN payloads and -0.0 survive."""
import struct

import numpy as np

MAGIC = b"VCPBIN1\0"
DTYPES = (np.dtype("<u1"), np.dtype("<i4"), np.dtype("<i8"), np.dtype("<f8"))   # the tag is the position


def as_record(value):
    """The 1-D little-endian array a value travels as: str / bytes as uint8 text, bool as uint8, an array of one of the
    four dtypes as it is.  Anything else is an error: nothing is converted behind the caller's back."""
    if isinstance(value, str):
        value = value.encode()
    if isinstance(value, bytes):
        return np.frombuffer(value, np.uint8).copy()
    a = np.asarray(value)
    if a.dtype == np.bool_:
        a = a.astype(np.uint8)
    for d in DTYPES:
        if a.dtype.kind == d.kind and a.dtype.itemsize == d.itemsize:
            return np.ascontiguousarray(a, d).reshape(-1)
    raise TypeError("vcpbin carries uint8, int32, int64 and float64, not %s" % a.dtype)


def dumps(records):
    """records: iterable of (name, value) in file order."""
    records = list(records)
    out = [MAGIC, struct.pack("<I", len(records))]
    for name, value in records:
        a = as_record(value)
        nb = name.encode()
        out.append(struct.pack("<H", len(nb)) + nb + struct.pack("<BQ", DTYPES.index(a.dtype), a.size))
        out.append(a.tobytes())
    return b"".join(out)


def loads(blob):
    """dict name -> 1-D array (file order kept); a repeated name is an error."""
    if blob[:8] != MAGIC:
        raise ValueError("not a vcpbin file")
    (n,), pos = struct.unpack_from("<I", blob, 8), 12
    out = {}
    for _ in range(n):
        (nl,) = struct.unpack_from("<H", blob, pos)
        name = blob[pos + 2:pos + 2 + nl].decode()
        tag, cnt = struct.unpack_from("<BQ", blob, pos + 2 + nl)
        pos += 2 + nl + 9
        d = DTYPES[tag]
        if name in out:
            raise ValueError("record %r twice" % name)
        out[name] = np.frombuffer(blob, d, cnt, pos).copy()
        pos += cnt * d.itemsize
    if pos != len(blob):
        raise ValueError("%d bytes after the last record" % (len(blob) - pos))
    return out


def write(path, records):
    with open(path, "wb") as f:
        f.write(dumps(records))


def read(path):
    with open(path, "rb") as f:
        return loads(f.read())


def text(a):
    return bytes(np.asarray(a, np.uint8)).decode()
