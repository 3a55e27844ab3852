"""Randomised sweep of vcp_parse_scan_text against io._rows_from_bytes and the restatement tests/scantext_ref.py, next to
tests/fuzz_import_compact.py: a case is a list of 1 to 50 segments whose lines are drawn from many field writers (%.6f,
integers, repr, %.17g, %.18e, "<w>e<e>", leading zeros, ".5" / "5.", blanks, signs, the names in mixed case), 0 to 3 ignored
extra fields, the three terminators and a last line without one, a line count log-uniform in 0 .. 20 000, now and then one
line of 33 to 80 KB; in about a quarter of the cases one defect is planted (too few fields, a class-0 field, an unsupported
byte, or a bad line together with an unsupported byte).  make_case(rng) builds the case (no GPU; a function of the seed
alone), expect(case) states what must come out from the reference alone, check(ctx, case) runs the device, host and
resident form in turn, and compares: rows by their bits, group, seg_first, n, n_host, the error text, the offset.
SUITE = (32, 9): building the cases takes about 1 s and the reference side of the bounded test about 1.1 s on the CPU.
usage: python tests/fuzz_scantext.py [cases] [seed]"""
import os
import random
import re
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import scantext_ref as R  # noqa: E402

SUITE = (32, 9)           # the bounded form of tests/test_scantext_gpu.py: (cases, seed)
N_MAX = 20_000
STAGE_BYTES = 32768       # csrc/scantext.hip; tests/test_scantext.py holds this copy to the source
CHUNK = 16384             # VCP_TXT_CHUNK of include/vcp.h, likewise
DEFECTS = ("few", "class0", "byte", "both")
NAMES = ("inf", "Infinity", "NaN", "nAn", "INF", "infinitY")
CLASS0 = ("1e", ".", "e5", "+ 1", "", "  ", "0x10", "1d5", "1,5", "--1", "1.2.3", "in", "1e+")
EXTRA = bytes(b for b in range(0x20, 0x7F) if b != 0x5F)      # supported bytes for the ignored fields (no tab)
BAD_BYTES = (0x85, 0x5F, 0x0B, 0x00, 0x7F, 0xB2)


def field(rng):
    k = rng.randrange(12)
    v = rng.choice((rng.uniform(-360, 360), rng.uniform(0, 1000), rng.uniform(-1e9, 1e9), rng.uniform(-1, 1) * 1e-3))
    if k == 0 or k == 1:
        s = "%.6f" % v
    elif k == 2:
        s = "%d" % rng.randint(-10 ** rng.randint(1, 18), 10 ** rng.randint(1, 18))
    elif k == 3:
        s = repr(v)
    elif k == 4:
        s = "%.17g" % v
    elif k == 5:
        s = "%.18e" % v
    elif k == 6:
        nd = rng.randint(1, 19)
        s = "%de%d" % (rng.randint(10 ** (nd - 1), 10 ** nd - 1), rng.randint(-19, 19))
    elif k == 7:
        s = "0" * rng.randint(1, 5) + "%.3f" % abs(v)
    elif k == 8:
        s = rng.choice((".5", "5.", "%d." % rng.randint(0, 999), ".%03d" % rng.randint(0, 999)))
    elif k == 9:
        s = rng.choice(NAMES) if rng.random() < 0.3 else "%de%d" % (rng.randint(1, 10 ** 19), rng.randint(15, 30))
    elif k == 10:
        s = "%.6fE%+03d" % (v, rng.randint(-12, 12))
    else:
        s = "%.9f" % v
    if rng.random() < 0.15 and not s.startswith("-"):
        s = "+" + s
    if rng.random() < 0.1:
        s = " " * rng.randint(0, 2) + s + " " * rng.randint(0, 3)
    return s


def line(rng, long_bytes=0):
    f = [field(rng), field(rng), field(rng)]
    for _ in range(rng.choice((0, 0, 0, 1, 2, 3))):
        f.append(bytes(rng.choice(EXTRA) for _ in range(rng.randint(0, 12))).decode("ascii"))
    if long_bytes:
        f.append("0" * long_bytes)
    return "\t".join(f).encode("ascii")


def make_case(rng):
    nseg = rng.choice((1, 1, 2, 5, rng.randint(1, 50)))
    total = int(10 ** rng.uniform(0, np.log10(N_MAX + 1))) - 1 if rng.random() < 0.9 else 0      # 0 .. 20 000, log-uniform
    cuts = sorted(rng.randint(0, total) for _ in range(nseg - 1))
    counts = [b - a for a, b in zip([0] + cuts, cuts + [total])]
    long_at = rng.randrange(total) if total and rng.random() < 0.2 else -1
    segs, j = [], 0
    for c in counts:
        buf = bytearray()
        for i in range(c):
            buf += line(rng, rng.randint(33_000, 80_000) if j == long_at else 0)
            buf += b"" if (i == c - 1 and rng.random() < 0.3) else rng.choice((b"\n", b"\r\n", b"\r"))
            j += 1
        segs.append(bytes(buf))
    defect = rng.choice(DEFECTS) if total and rng.random() < 0.25 else None
    if defect:
        k = rng.choice([k for k, c in enumerate(counts) if c])
        lines = re.split(b"(\r\n|\n|\r)", segs[k])                     # [line, terminator, line, ...]
        i = 2 * rng.randrange(counts[k])
        f = lines[i].split(b"\t")
        if defect in ("few", "both"):
            empty = rng.random() < 0.2 and i + 1 < len(lines) and lines[i + 1] != b""      # a line of its own only
            lines[i] = b"" if empty else b"\t".join(f[:rng.randint(1, 2)])
        elif defect == "class0":
            f[rng.randrange(3)] = rng.choice(CLASS0).encode()
            lines[i] = b"\t".join(f)
        if defect in ("byte", "both"):
            i = 2 * rng.randrange(counts[k])                           # in an ignored field: the line stays what it was
            lines[i] = lines[i] + b"\tq" + bytes([rng.choice(BAD_BYTES)]) + b"q"
        segs[k] = b"".join(lines)
    return dict(segs=segs, defect=defect, resident=bool(rng.random() < 0.5))


def cases(count, seed):
    rng = random.Random(seed)
    return [make_case(rng) for _ in range(count)]


def expect(case):
    """From the reference alone: dict(bad_byte = the first unsupported offset of the joined text or None, error = the
    text of the first segment's ValueError or None, rows, group, seg_first, n_host, classes)."""
    from vtkcloudpoint_amd import io as vio
    text, seg_off = vio._join_segments(case["segs"])
    out = dict(text=text, seg_off=seg_off, bad_byte=None, error=None, rows=None)
    if not R.supported(text):
        out["bad_byte"] = next(i for i, b in enumerate(text) if not R.supported(bytes([b])))
        return out                                                     # code -8 takes precedence over a bad line
    rows = []
    for k, s in enumerate(case["segs"]):
        try:
            rows.append(vio._rows_from_bytes(s, "segment %d" % k))
        except ValueError as e:
            out["error"] = str(e)                                      # the first segment that raises wins
            return out
    counts = [len(r) for r in rows]
    out["rows"] = np.concatenate(rows) if rows else np.zeros((0, 3))
    out["group"] = np.repeat(np.arange(len(rows), dtype=np.int32), counts)
    out["seg_first"] = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    n_host, classes = 0, {}
    for ln in re.split(b"\r\n|\n|\r", text):
        if ln == b"":
            continue                                                   # only the piece behind the last terminator is empty
        cs = [R.field_class(f.decode("ascii")) for f in ln.split(b"\t")[:3]]
        n_host += any(c == 3 for c, _ in cs)
        for (c, _), f in zip(cs, ln.split(b"\t")[:3]):
            if c == 2:
                m = R.NUMBER.match(f.decode("ascii"))
                e10 = int(m.group(5) or 0) - len(m.group(3) if m.group(3) is not None else (m.group(4) or ""))
                classes[(2, e10 >= 0)] = classes.get((2, e10 >= 0), 0) + 1
    out["n_host"], out["classes"] = n_host, classes
    return out


def check(ctx, case, want=None):
    from vtkcloudpoint_amd import _native as N
    from vtkcloudpoint_amd import io as vio
    want = want or expect(case)
    try:
        got = vio.parse_scan_text(case["segs"], resident=case["resident"], ctx=ctx)
    except vio.ScanTextError as e:
        assert want["bad_byte"] is None and str(e) == want["error"], (str(e), want["error"], want["bad_byte"])
        return want
    except N.VcpError as e:
        assert e.code == -8 and e.err[0] == want["bad_byte"], (e.code, e.err, want["bad_byte"], want["error"])
        return want
    assert want["bad_byte"] is None and want["error"] is None, (want["bad_byte"], want["error"])
    rows, group = (got[k].cpu().numpy() if case["resident"] else got[k] for k in ("rows", "group"))
    g, w = np.ascontiguousarray(rows).view(np.uint64), want["rows"].view(np.uint64)
    assert g.shape == w.shape, (g.shape, w.shape)
    d = np.argwhere(g != w)
    assert len(d) == 0, "row %d field %d: want %016x, got %016x (%d differ)" % (
        d[0][0], d[0][1], int(w[tuple(d[0])]), int(g[tuple(d[0])]), len(d))
    assert np.array_equal(group, want["group"]) and np.array_equal(got["seg_first"], want["seg_first"])
    assert got["n"] == len(w) and got["n_host"] == want["n_host"], (got["n"], got["n_host"], want["n_host"])
    return want


def summary(case_list, wants):
    """What the list covers, for the conditions that keep the sweep from passing by being empty."""
    def over_stage(w):
        st = [0] + [m.end() for m in re.finditer(b"\r\n|\n|\r", w["text"])]
        return any(st[min(j + 256, len(st) - 1)] - (st[j] & ~15) > STAGE_BYTES for j in range(0, len(st) - 1, 256))
    s = dict(cases=len(case_list), no_line=sum(len(w["text"]) == 0 for w in wants),
             defects={d: sum(c["defect"] == d for c in case_list) for d in DEFECTS},
             over_stage=sum(over_stage(w) for w in wants), resident=sum(c["resident"] for c in case_list),
             many_segments=sum(len(c["segs"]) > 256 or len(w["text"]) > CHUNK for c, w in zip(case_list, wants)),
             lines=sum(len(w["rows"]) for w in wants if w["rows"] is not None),
             host_lines=sum(w["n_host"] for w in wants if w["rows"] is not None),
             class2_pos=sum(w["classes"].get((2, True), 0) for w in wants if w["rows"] is not None),
             class2_neg=sum(w["classes"].get((2, False), 0) for w in wants if w["rows"] is not None))
    return s


if __name__ == "__main__":
    from vtkcloudpoint_amd import _native as N
    count = int(sys.argv[1]) if len(sys.argv) > 1 else 100
    seed = int(sys.argv[2]) if len(sys.argv) > 2 else 1
    ctx = N.Context(0)
    lst = cases(count, seed)
    print(summary(lst, [check(ctx, c) for c in lst]))
