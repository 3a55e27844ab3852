"""The reference's text formats on either side of the path (host side; the numeric work of an import runs on the
GPU through vcp_import_convert, or through vcp_import_compact where the result stays on the device or carries counts;
parse_scan_text / read_scan_text_fast / read_folder_resident read the scan files' text on the GPU as well, and
format_scan_text / write_*_fast / export_resident build the exports' text there).

* scan files          one point per line, `motor_x<TAB>motor_y<TAB>Distance` -- what MainForm.AddFolder reads
                      (FrmMain.cs:1005-1009 via FileMap.ReadFile, BaseClass/FileMap.cs:16-33) and what
                      Tools.ExportPoints-style code writes back (BaseClass/Tools.cs:233).
* clustering export   `clusterId<TAB>motor_x<TAB>motor_y<TAB>Distance`, clusters in list order
                      (BaseClass/Tools.cs:366-392).

Numbers are written with C#'s "F<bit>" format.  Python's fixed-point formatting rounds the exact binary value
half-to-even while .NET Framework 3.5 formats from a 15-digit decimal expansion; the two differ only for values
whose 16th significant digit decides a tie -- not reproduced here (no .NET in this image to pin it).
"""
import os

import numpy as np

from .datamodel import Point3D


def read_scan_text(path):
    """rows [n, 3] = (motor_x, motor_y, Distance) of a scan file.  Like `Convert.ToDouble(tmpxyz[k])`
    (FrmMain.cs:1006-1008) a line with fewer than three fields or a non-numeric field is an error; extra fields
    are ignored."""
    rows = []
    with open(path, "r", encoding="gb2312", errors="replace") as f:  # FileMap.cs:24 reads as GB2312
        for ln, line in enumerate(f.read().splitlines(), 1):
            parts = line.split("\t")
            if len(parts) < 3:
                raise ValueError("%s:%d: expected motor_x<TAB>motor_y<TAB>Distance" % (path, ln))
            try:
                rows.append((float(parts[0]), float(parts[1]), float(parts[2])))
            except ValueError:
                raise ValueError("%s:%d: not a number" % (path, ln))
    return np.array(rows, dtype=np.float64).reshape(-1, 3)


def write_scan_text(path, rawData, bit=6):
    """BaseClass/Tools.cs:233: one `motor_x<TAB>motor_y<TAB>Distance` line per point, "F<bit>"."""
    fmt = "%%.%df\t%%.%df\t%%.%df\n" % (bit, bit, bit)
    with open(path, "w", encoding="ascii", newline="\r\n") as f:  # StreamWriter.WriteLine on Windows
        for p in rawData:
            f.write(fmt % (p.motor_x, p.motor_y, p.Distance))


def write_clusters_text(path, clusList, bit=6):
    """BaseClass/Tools.cs:366-392: `clusterId<TAB>motor_x<TAB>motor_y<TAB>Distance`, cluster by cluster."""
    fmt = "%%d\t%%.%df\t%%.%df\t%%.%df\n" % (bit, bit, bit)
    with open(path, "w", encoding="ascii", newline="\r\n") as f:
        for clus in clusList:
            for p in clus.li:
                f.write(fmt % (p.clusterId, p.motor_x, p.motor_y, p.Distance))


def add_folder(files, x_angle=0.0, y_angle=0.0, xdir=2, ydir=1, typpe=1, ctx=None):
    """MainForm.AddFolder for scan points (FrmMain.cs:960-1100, typpe 1 = drop exact duplicates, 2 = keep them):
    reads the files in order, filters `Distance == 0 || Distance > 1000`, converts (motor_x, motor_y, Distance) to
    X, Y, Z and, for typpe 1, drops every point whose X, Y, Z equal those of a point already in the list -- over
    ALL files read so far, as `rawData` keeps growing.  Returns (rawData: list of Point3D, duplicatNum, pathList).
    The conversion and the duplicate search run on the GPU in one call."""
    if typpe not in (1, 2):
        raise NotImplementedError("typpe 3/4 (fixed points per file) are UI bookkeeping, not on the GPU path")
    from . import runtime
    ctx = ctx or runtime.default_context()
    rows, path_id = [], []
    for k, f in enumerate(files):
        r = read_scan_text(f)
        rows.append(r)
        path_id.append(np.full(len(r), k, np.int32))
    rows = np.concatenate(rows) if rows else np.zeros((0, 3))
    path_id = np.concatenate(path_id) if path_id else np.zeros(0, np.int32)
    res = ctx.import_convert(rows, x_angle, y_angle, xdir, ydir, dedupe=(typpe == 1))
    rawData = []
    for i in np.nonzero(res["state"] == 1)[0]:
        p = Point3D(res["xyz"][i, 0], res["xyz"][i, 1], res["xyz"][i, 2], 0, True)
        p.motor_x, p.motor_y, p.Distance = rows[i]
        p.pathId = int(path_id[i])
        rawData.append(p)
    return rawData, int(res["duplicates"]), list(files)


def import_scan_resident(rows, group=None, x_angle=0.0, y_angle=0.0, xdir=2, ydir=1, dedupe=True, ctx=None):
    """The import that stays in HBM (vcp_import_compact_dev): rows [n, 3] = (motor_x, motor_y, Distance) as a numpy array
    (uploaded once) or a float64 torch tensor on the context's device (read in place); group [n] int32 or None likewise.
    Returns a dict of torch device tensors, views of length m into buffers of n entries: motor [m, 2], xyz [m, 3],
    dist [m], src [m], count [m], group [m] (int32), and row_to [n] (int32, -1 = filtered), with m and duplicates as
    ints.  They are what dbscan_dev / gdbscan_dev(d_weights=count, d_aux=dist) / centroids_dev take as data_ptr()s; the
    labels of the raw rows are labels[row_to] where row_to >= 0.  The call orders itself after the current torch
    stream's work and returns when the result is in place."""
    import torch
    if torch.is_tensor(rows):
        if rows.dtype != torch.float64 or not rows.is_cuda:
            raise ValueError("rows must be a float64 tensor on the GPU (or a numpy array)")
        t_rows = rows.contiguous().reshape(-1, 3)
    else:
        t_rows = np.ascontiguousarray(rows, np.float64).reshape(-1, 3)
    n = len(t_rows)
    if group is not None:
        if torch.is_tensor(group):
            if group.dtype != torch.int32 or not group.is_cuda:
                raise ValueError("group must be an int32 tensor on the GPU (or a numpy array)")
            t_group = group.contiguous().reshape(-1)
        else:
            t_group = np.ascontiguousarray(group, np.int32).reshape(-1)
        if len(t_group) != n:
            raise ValueError("group has %d entries for %d rows" % (len(t_group), n))
    from . import runtime
    ctx = ctx or runtime.default_context()
    if not torch.is_tensor(t_rows):
        t_rows = torch.from_numpy(t_rows).cuda()
    dev = t_rows.device
    t_group = None if group is None else (t_group if torch.is_tensor(t_group) else torch.from_numpy(t_group).to(dev))
    room = max(n, 1)
    motor = torch.empty((room, 2), dtype=torch.float64, device=dev)
    xyz = torch.empty((room, 3), dtype=torch.float64, device=dev)
    dist = torch.empty(room, dtype=torch.float64, device=dev)
    src, count, gout, row_to = (torch.empty(room, dtype=torch.int32, device=dev) for _ in range(4))
    torch.cuda.current_stream(dev).synchronize()     # the library runs on the context's stream, not on torch's
    m, dup = ctx.import_compact_dev(t_rows.data_ptr(), n, None if t_group is None else t_group.data_ptr(), x_angle,
                                    y_angle, xdir, ydir, dedupe, motor.data_ptr(), xyz.data_ptr(), dist.data_ptr(),
                                    src.data_ptr(), count.data_ptr(), gout.data_ptr(), row_to.data_ptr())
    return dict(motor=motor[:m], xyz=xyz[:m], dist=dist[:m], src=src[:m], count=count[:m], group=gout[:m],
                row_to=row_to[:n], m=m, duplicates=dup)


# ---- the device reader of scan files (vcp_parse_scan_text) -------------------------------------------------------------
class ScanTextError(ValueError):
    """A bad line found by the device reader: .line (1-based within its file), .segment (the file's number), .kind
    (1 = fewer than three fields, 2 = not a number)."""

    def __init__(self, line, segment, kind, name=None):
        self.line, self.segment, self.kind = int(line), int(segment), int(kind)
        what = "expected motor_x<TAB>motor_y<TAB>Distance" if self.kind == 1 else "not a number"
        super().__init__("%s:%d: %s" % (name if name is not None else "segment %d" % self.segment, self.line, what))


def _join_segments(data):
    """One bytes object and seg_off for a bytes object or a list of them; a non-empty file without a final '\n' gets
    one ("...\r" becomes "...\r\n", still one terminator)."""
    parts = [data] if isinstance(data, (bytes, bytearray, memoryview)) else list(data)
    parts = [bytes(p) for p in parts]
    parts = [p if (not p or p.endswith(b"\n")) else p + b"\n" for p in parts]
    seg_off = np.zeros(len(parts) + 1, np.uint64)
    seg_off[1:] = np.cumsum([len(p) for p in parts], dtype=np.uint64)
    return b"".join(parts), seg_off


def parse_scan_text(data, resident=False, ctx=None):
    """The bytes of one scan file, or a list with the bytes of several, parsed on the GPU.  Returns dict(rows [n, 3]
    float64, group [n] int32 = the file of every row, seg_first [files + 1], n, n_host = the lines whose numbers the host
    had to read): numpy arrays, or with resident=True torch tensors on the context's device, the layout
    import_scan_resident takes.  rows equal read_scan_text's bit for bit.  A bad line raises ScanTextError; bytes outside
    the device reader's set raise _native.VcpError with code -8 (VCP_ERR_UNSUPPORTED) and .err[0] = the offset."""
    text, seg_off = _join_segments(data)
    return _parse_joined(text, seg_off, resident, ctx)


def _parse_joined(text, seg_off, resident, ctx):
    """parse_scan_text on the joined text (bytes or a uint8 numpy array) and its seg_off."""
    from . import _native, runtime
    ctx = ctx or runtime.default_context()
    try:
        if not resident:
            return ctx.parse_scan_text(text, seg_off) if len(seg_off) > 1 else dict(
                rows=np.zeros((0, 3)), group=np.zeros(0, np.int32), seg_first=np.zeros(1, np.int64), n=0, n_host=0)
        import torch
        # Room for one line per 16 bytes (an F6 line has 27 or more), so that the text is uploaded once; a text of shorter
        # lines comes back with VCP_ERR_INDEX and its n, and is parsed again with exactly that room.
        cap = len(text) // 16 + 1024
        res = dict(seg_first=np.zeros(len(seg_off), np.int64), n=0, n_host=0)
        while len(seg_off) > 1 and len(text) > 0:
            rows = torch.empty((cap, 3), dtype=torch.float64, device="cuda")
            group = torch.empty(cap, dtype=torch.int32, device="cuda")
            torch.cuda.current_stream().synchronize()    # the library runs on the context's stream, not on torch's
            try:
                res = ctx.parse_scan_text_dev(text, cap, rows.data_ptr(), group.data_ptr(), seg_off)
                break
            except _native.VcpError as e:
                if e.code != -4:
                    raise
                cap = e.n
        n = res["n"]
        if n == 0:
            rows = torch.empty((0, 3), dtype=torch.float64, device="cuda")
            group = torch.empty(0, dtype=torch.int32, device="cuda")
        elif cap > n + n // 4:                             # do not keep the unused room alive
            rows, group = rows[:n].clone(), group[:n].clone()
        return dict(rows=rows[:n], group=group[:n], seg_first=res["seg_first"], n=n, n_host=res["n_host"])
    except _native.VcpError as e:
        if e.code == -1 and getattr(e, "err", (0, 0, 0))[2] in (1, 2):
            raise ScanTextError(*e.err) from None
        raise


def read_scan_text_fast(path, ctx=None):
    """read_scan_text with the parse on the GPU: the same array, the same ValueError text; a file with bytes the device
    reader does not take goes through read_scan_text."""
    from . import _native
    with open(path, "rb") as f:
        data = f.read()
    try:
        return parse_scan_text(data, ctx=ctx)["rows"]
    except ScanTextError as e:
        raise ValueError(str(ScanTextError(e.line, e.segment, e.kind, name=path))) from None
    except _native.VcpError as e:
        if e.code != -8:
            raise
        return read_scan_text(path)


def _rows_from_bytes(data, name, line0=0):
    """read_scan_text on bytes already in memory (the same decoding, line splitting and errors); line0 = the lines of
    the file that precede them."""
    import io as _io
    rows = []
    text = _io.TextIOWrapper(_io.BytesIO(data), encoding="gb2312", errors="replace").read()
    for ln, line in enumerate(text.splitlines(), line0 + 1):
        parts = line.split("\t")
        if len(parts) < 3:
            raise ValueError("%s:%d: expected motor_x<TAB>motor_y<TAB>Distance" % (name, ln))
        try:
            rows.append((float(parts[0]), float(parts[1]), float(parts[2])))
        except ValueError:
            raise ValueError("%s:%d: not a number" % (name, ln))
    return np.array(rows, dtype=np.float64).reshape(-1, 3)


def _batches(files, max_bytes):
    """Pieces (file number, bytes or None = the whole file, lines of the file before the piece, length) in order,
    grouped so that no group exceeds max_bytes with the '\n' a piece may receive; a larger file is read here and cut
    after a line end."""
    batch, size = [], 0
    for k, f in enumerate(files):
        data, line0, length = None, 0, os.path.getsize(f)
        if length + 1 > max_bytes:
            with open(f, "rb") as fh:
                data = fh.read()
            while len(data) + 1 > max_bytes:
                cut = max(data.rfind(b"\n", 0, max_bytes - 1), data.rfind(b"\r", 0, max_bytes - 2)) + 1
                if cut <= 0:
                    raise ValueError("%s: a line longer than %d bytes" % (f, max_bytes))
                if data[cut - 1:cut] == b"\r" and data[cut:cut + 1] == b"\n":
                    cut += 1                                # never between the two bytes of one terminator
                if batch:
                    yield batch
                    batch, size = [], 0
                yield [(k, data[:cut], line0, cut)]
                line0 += data.count(b"\n", 0, cut) + data.count(b"\r", 0, cut) - data.count(b"\r\n", 0, cut)
                data = data[cut:]
            length = len(data)
        if size + length + 1 > max_bytes and batch:
            yield batch
            batch, size = [], 0
        batch.append((k, data, line0, length))
        size += length + 1
    if batch:
        yield batch


def _load_batch(batch, files):
    """The pieces of a batch one after the other in ONE uint8 array (a whole file is read straight into it), every
    non-empty piece ending with '\n'; returns (text, seg_off)."""
    buf = np.empty(sum(length + 1 for _, _, _, length in batch), np.uint8)
    view, o, seg_off = memoryview(buf), 0, np.zeros(len(batch) + 1, np.uint64)
    for i, (k, data, _, length) in enumerate(batch):
        if data is None:
            with open(files[k], "rb") as fh:
                got = fh.readinto(view[o:o + length])
        else:
            got = len(data)
            view[o:o + got] = data
        o += got
        if got and buf[o - 1] != 10:
            buf[o] = 10                                    # "...\r" becomes "...\r\n": still one terminator
            o += 1
        seg_off[i + 1] = o
    return buf[:o], seg_off


def read_folder_resident(files, x_angle=0.0, y_angle=0.0, xdir=2, ydir=1, dedupe=True, by_file=False, ctx=None,
                         max_bytes=(1 << 32) - 4096):
    """File -> resident import without a host parse: the files' bytes are uploaded in batches below 4 GiB (a larger file
    is cut at a line end), parsed on the GPU and handed to import_scan_resident as device tensors.  by_file: the file
    number is the group (duplicates are classes within a file, AddFolder's typpe 3 / 4); otherwise one class space over
    all files (typpe 1 / 2).  Returns import_scan_resident's dict plus rows [n, 3], file [n] (int32, the file of every
    raw row), n and n_host.  A batch with bytes the device reader does not take is parsed on the host, as read_scan_text
    does, and uploaded.  A bad line raises the ValueError read_scan_text raises."""
    import torch
    from . import _native, runtime
    ctx = ctx or runtime.default_context()
    files = list(files)
    rows, group, n_host = [], [], 0
    for batch in _batches(files, max_bytes):
        ks = np.array([piece[0] for piece in batch], np.int32)
        text, seg_off = _load_batch(batch, files)
        try:
            r = _parse_joined(text, seg_off, True, ctx)
        except ScanTextError as e:
            k = int(ks[e.segment])      # a piece of a cut file starts past the file's first line
            raise ValueError(str(ScanTextError(e.line + batch[e.segment][2], k, e.kind, name=files[k]))) from None
        except _native.VcpError as e:
            if e.code != -8:
                raise
            host = [_rows_from_bytes(text[int(seg_off[i]):int(seg_off[i + 1])].tobytes(), files[piece[0]], piece[2])
                    for i, piece in enumerate(batch)]
            fk = [np.full(len(h), k, np.int32) for h, k in zip(host, ks)]
            rows.append(torch.from_numpy(np.concatenate(host).reshape(-1, 3)).cuda())
            group.append(torch.from_numpy(np.concatenate(fk)).cuda())
            continue
        rows.append(r["rows"])
        group.append(torch.from_numpy(ks).cuda()[r["group"].long()])
        n_host += r["n_host"]
    if not rows:
        rows, group = [torch.zeros((0, 3), dtype=torch.float64, device="cuda")], [torch.zeros(0, dtype=torch.int32, device="cuda")]
    d_rows = torch.cat(rows) if len(rows) > 1 else rows[0]
    d_file = torch.cat(group) if len(group) > 1 else group[0]
    res = import_scan_resident(d_rows, d_file if by_file else None, x_angle, y_angle, xdir, ydir, dedupe, ctx=ctx)
    res.update(rows=d_rows, file=d_file, n=len(d_rows), n_host=n_host)
    return res


# ---- the device writer of the exports (vcp_format_rows) ---------------------------------------------------------------
# Lines per call: no call can reach 4 GiB of text, whatever the values (_native: VCP_FMT_LINE_MAX = 112 bytes a line).
_FMT_LINES = (1 << 32) // 112 - 1


def _format_host(a, b, c, ids, order, bit, eol):
    """The text as the Python writers build it (write_scan_text, write_clusters_text): one '%.*f' per number."""
    a, b, c = (np.asarray(x, np.float64).reshape(-1).tolist() for x in (a, b, c))
    rows = range(len(a)) if order is None else np.asarray(order, np.int64).reshape(-1).tolist()
    for r in rows:
        if not 0 <= r < len(a):
            raise IndexError("order holds %d for %d rows" % (r, len(a)))
    num = "%%.%df\t%%.%df\t%%.%df" % (bit, bit, bit) + eol
    if ids is None:
        return "".join([num % (a[r], b[r], c[r]) for r in rows]).encode("ascii")
    ids = np.asarray(ids).reshape(-1).tolist()
    return "".join([("%d\t" + num) % (ids[r], a[r], b[r], c[r]) for r in rows]).encode("ascii")


def _format_parts(a, b, c, ids, order, bit, eol, ctx, max_lines):
    """The pieces of the text, in order, as uint8 arrays (one per call of at most max_lines lines); a call that meets a
    value the device formatter does not take raises _native.VcpError with code -8."""
    import torch
    from . import runtime
    if eol not in ("\n", "\r\n"):
        raise ValueError("eol must be '\\n' or '\\r\\n'")
    e = 1 if eol == "\r\n" else 0
    ctx = ctx or runtime.default_context()
    resident = any(torch.is_tensor(x) for x in (a, b, c))
    if not resident:
        a, b, c = (np.asarray(x, np.float64) for x in (a, b, c))
        a, b, c = (x if x.ndim == 1 else x.reshape(-1) for x in (a, b, c))
        ids = None if ids is None else np.ascontiguousarray(ids.cpu().numpy() if torch.is_tensor(ids) else ids, np.int32)
        order = None if order is None else np.ascontiguousarray(
            order.cpu().numpy() if torch.is_tensor(order) else order, np.int64).reshape(-1)
        m = len(a) if order is None else len(order)
        for j0 in range(0, m, max_lines):
            j1 = min(j0 + max_lines, m)
            if order is None:
                yield ctx.format_rows(a[j0:j1], b[j0:j1], c[j0:j1], None if ids is None else ids[j0:j1], None, bit, e)
            else:
                yield ctx.format_rows(a, b, c, ids, order[j0:j1], bit, e)
        return
    cols = []
    for x in (a, b, c):
        if not torch.is_tensor(x):
            x = torch.from_numpy(np.ascontiguousarray(x, np.float64).reshape(-1)).cuda()
        if x.dtype != torch.float64 or not x.is_cuda or x.dim() != 1:
            raise ValueError("a column must be a 1-D float64 tensor on the GPU (or a numpy array)")
        if len(x) > 0 and x.stride(0) < 1:
            x = x.contiguous()
        cols.append(x)
    a, b, c = cols
    dev, n = a.device, len(a)
    if len(b) != n or len(c) != n:
        raise ValueError("columns of %d, %d and %d rows" % (n, len(b), len(c)))
    if ids is not None:
        ids = (ids if torch.is_tensor(ids) else torch.from_numpy(np.ascontiguousarray(ids, np.int32))).to(
            device=dev, dtype=torch.int32).contiguous().reshape(-1)
        if len(ids) != n:
            raise ValueError("ids has %d entries for %d rows" % (len(ids), n))
    if order is not None:
        order = (order if torch.is_tensor(order) else torch.from_numpy(np.ascontiguousarray(order, np.int64))).to(
            device=dev, dtype=torch.int64).contiguous().reshape(-1)
    m = n if order is None else len(order)
    torch.cuda.current_stream(dev).synchronize()     # the library runs on the context's stream, not on torch's
    for j0 in range(0, m, max_lines):
        j1 = min(j0 + max_lines, m)
        if order is None:
            pa, pb, pc = (x[j0:j1] for x in (a, b, c))
            args = (pa.data_ptr(), max(pa.stride(0), 1), pb.data_ptr(), max(pb.stride(0), 1), pc.data_ptr(),
                    max(pc.stride(0), 1), j1 - j0, None if ids is None else ids[j0:j1].data_ptr(), None, j1 - j0)
        else:
            args = (a.data_ptr(), max(a.stride(0), 1), b.data_ptr(), max(b.stride(0), 1), c.data_ptr(),
                    max(c.stride(0), 1), n, None if ids is None else ids.data_ptr(), order[j0:j1].data_ptr(), j1 - j0)
        nbytes = ctx.format_rows_dev(*args, bit=bit, eol=e)      # count-only: one pass over the lines, no text
        out = np.empty(max(nbytes, 1), np.uint8)
        ctx.format_rows_dev(*args, bit=bit, eol=e, out=out)
        yield out[:nbytes]


def _format_or_fall_back(a, b, c, ids, order, bit, eol, ctx, max_lines):
    """The list of pieces (uint8 arrays or bytes) of the whole text: the device's, or on VCP_ERR_UNSUPPORTED the host
    writer's for the whole call."""
    import torch
    from . import _native
    try:
        return list(_format_parts(a, b, c, ids, order, bit, eol, ctx, max_lines))
    except _native.VcpError as e:
        if e.code != -8:
            raise
    host = [None if x is None else (x.cpu().numpy() if torch.is_tensor(x) else np.asarray(x)) for x in (a, b, c, ids, order)]
    return [_format_host(host[0], host[1], host[2], host[3], host[4], bit, eol)]


def format_scan_text(a, b, c, ids=None, order=None, bit=6, eol="\r\n", ctx=None, max_lines=_FMT_LINES):
    """The export's text built on the GPU (vcp_format_rows): line j is `[ids[r] TAB] a[r] TAB b[r] TAB c[r] eol` with
    r = order[j] (None: every row in turn), numbers as '%.*f' % (bit, v) and ids as '%d' -- byte for byte what
    write_scan_text / write_clusters_text write.  a, b, c: 1-D float64 numpy arrays, or torch tensors on the context's
    device; strided views (rows[:, k]) are read in place, without a copy.  ids int32 [n] and order int64 [m] likewise.
    The text is built in calls of at most max_lines lines, each below 4 GiB.  A call with a value the device formatter
    does not take (NaN, an infinity, 1e15 or more in magnitude) is formatted by the host writer instead.  An entry of order
    outside the rows raises _native.VcpError with code -4 and .err = (line, entry)."""
    parts = _format_or_fall_back(a, b, c, ids, order, bit, eol, ctx, max_lines)
    if len(parts) == 1:
        return parts[0] if isinstance(parts[0], bytes) else parts[0].tobytes()
    return b"".join(p if isinstance(p, bytes) else p.tobytes() for p in parts)


def _write_parts(path, parts):
    with open(path, "wb") as f:
        for p in parts:
            f.write(p if isinstance(p, bytes) else memoryview(p))


def _three_columns(x):
    """(a, b, c) of rows [n, 3] (numpy or torch: its columns, as views) or of a sequence of three columns."""
    if hasattr(x, "ndim") and x.ndim == 2:
        if x.shape[1] != 3:
            raise ValueError("rows must be [n, 3]")
        return x[:, 0], x[:, 1], x[:, 2]
    a, b, c = x
    return a, b, c


def write_scan_text_fast(path, rows_or_columns, bit=6, ctx=None):
    """write_scan_text with the text built on the GPU: rows [n, 3] = (motor_x, motor_y, Distance) or three columns, numpy
    or torch device tensors.  The file is byte-identical to write_scan_text's on the same data."""
    a, b, c = _three_columns(rows_or_columns)
    _write_parts(path, _format_or_fall_back(a, b, c, None, None, bit, "\r\n", ctx, _FMT_LINES))


def cluster_order(labels):
    """The rows with label >= 1 in the order of the cluster export: stably sorted by label, which is clusList order with
    every li in input order (Tools.GetClusList).  A torch tensor gives a tensor on its device, built there."""
    import torch
    if torch.is_tensor(labels):
        idx = torch.nonzero(labels.reshape(-1) >= 1).reshape(-1)
        return idx[torch.sort(labels.reshape(-1)[idx], stable=True)[1]]
    labels = np.asarray(labels).reshape(-1)
    idx = np.nonzero(labels >= 1)[0]
    return idx[np.argsort(labels[idx], kind="stable")]


def write_clusters_text_fast(path, labels, motor_x, motor_y, dist, bit=6, ctx=None):
    """write_clusters_text with the text built on the GPU: labels [n] (0 = none) and the three columns of the same rows,
    numpy or torch device tensors.  The file is byte-identical to write_clusters_text's on GetClusList's clusList."""
    _write_parts(path, _format_or_fall_back(motor_x, motor_y, dist, labels, cluster_order(labels), bit, "\r\n", ctx,
                                            _FMT_LINES))


def write_centroids_text_fast(path, c3, bit, ctx=None):
    """Tools.exportClustersCenterFile (BaseClass/Tools.cs:322-354): one `X<TAB>Y<TAB>Z` line per centre, "F<bit>"; c3 is
    [K, 3], numpy or a torch device tensor (xyz of the centroid calls, read in place)."""
    a, b, c = _three_columns(c3)
    _write_parts(path, _format_or_fall_back(a, b, c, None, None, bit, "\r\n", ctx, _FMT_LINES))


def export_resident(path, imp, labels=None, keep=None, bit=6, ctx=None):
    """The exports from the tensors of import_scan_resident (imp["motor"] [m, 2], imp["dist"] [m]): the scan export
    (write_scan_text) when labels is None, the cluster export (write_clusters_text) of the device labels [m] otherwise.
    keep: an optional boolean device mask [m]; a row with keep false is left out, as cleanDataByDistance's RemoveAll and
    cluster_mad's rejection leave it out.  The order is built on the device; nothing but the text comes down."""
    import torch
    motor, dist = imp["motor"], imp["dist"]
    mx, my = motor[:, 0], motor[:, 1]
    if labels is None:
        order = None if keep is None else torch.nonzero(keep.reshape(-1)).reshape(-1)
        ids = None
    else:
        ids = labels.reshape(-1).to(torch.int32)
        order = cluster_order(ids if keep is None else torch.where(keep.reshape(-1), ids, torch.zeros_like(ids)))
    _write_parts(path, _format_or_fall_back(mx, my, dist, ids, order, bit, "\r\n", ctx, _FMT_LINES))


def add_fixed_folder(files, x_angle=0.0, y_angle=0.0, xdir=2, ydir=1, typpe=3, ctx=None):
    """MainForm.AddFolder for fixed points (FrmMain.cs:960-1100, typpe 3 / 4): one ClusObj per file; a row whose X, Y, Z
    equal those of a point already in ITS file's list is not added, the point found gets ptsCount += 1 (:1069-1085).  The
    duplicates are always searched; the two typpes differ in what they count: typpe 3 counts a duplicate in duplicatNum
    and a new point in pts, typpe 4 counts every unfiltered row in pts (:1076-1083).  Returns (clusList, duplicatNum, pts,
    pathList): clusList[k].li holds file k's points in file order with ptsCount, pathId = k and clusterId = k + 1.
    Filter, conversion, the per-file duplicate classes and their sizes are one vcp_import_compact call with the file
    number as the group."""
    from .datamodel import ClusObj
    if typpe not in (3, 4):
        raise ValueError("add_fixed_folder is AddFolder's typpe 3 / 4; typpe 1 / 2 is add_folder")
    from . import runtime
    ctx = ctx or runtime.default_context()
    rows, path_id = [], []
    for k, f in enumerate(files):
        r = read_scan_text(f)
        rows.append(r)
        path_id.append(np.full(len(r), k, np.int32))
    rows = np.concatenate(rows) if rows else np.zeros((0, 3))
    path_id = np.concatenate(path_id) if path_id else np.zeros(0, np.int32)
    res = ctx.import_compact(rows, path_id, x_angle, y_angle, xdir, ydir, dedupe=True)
    clusList = [ClusObj() for _ in files]
    for j in range(res["m"]):
        k = int(res["group"][j])
        p = Point3D(res["xyz"][j, 0], res["xyz"][j, 1], res["xyz"][j, 2], k + 1, True)
        p.motor_x, p.motor_y, p.Distance = float(res["motor"][j, 0]), float(res["motor"][j, 1]), float(res["dist"][j])
        p.pathId, p.ptsCount = k, int(res["count"][j])
        name = os.path.basename(str(files[k]))
        p.pointName = name[: name.index(".")] if "." in name else name      # FrmMain.cs:1021
        clusList[k].li.append(p)
    m, dup = res["m"], res["duplicates"]
    return clusList, (dup if typpe == 3 else 0), (m if typpe == 3 else m + dup), list(files)
