"""The reference's text formats on either side of the path (host side; the numeric work of an import runs on the
GPU through vcp_import_convert, or through vcp_import_compact where the result stays on the device or carries counts).

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
