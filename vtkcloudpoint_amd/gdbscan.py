"""DBSCAN with point weights and a range gate over the C-ABI (vcp_gdbscan / vcp_gdbscan_dev).

vcp_dbscan decides what the reference's DBImproved decides: every row counts once, and two rows are neighbours whenever
their (motor_x, motor_y) are within eps.  Two things in the data break that:

  multiplicity  the import drops exact duplicates and keeps their number in Point3D.ptsCount, so a target scanned three
                times has a third of its density afterwards.  weights = the counts clusters the distinct rows as if the
                duplicates were still there (sample_weight in scikit-learn's DBSCAN, MinWeight in GDBSCAN)
  range         a target and the wall behind it are neighbours in motor angles.  aux = Distance with a gate makes two
                rows neighbours only when their ranges are within the gate as well, which one global band of Distance
                cannot do for targets standing at several ranges

include/vcp.h states the definition; with neither weights nor aux the result is vcp_dbscan's.
"""
import numpy as np

from . import _native
from .kdist import _metric
from .runtime import default_context


def gdbscan(points, eps, min_weight, weights=None, aux=None, gate=None, metric="L1_2D", cf_in=0, ctx=None,
            want_wsum=False):
    """Returns (labels [n] int32, is_core [n] bool, n_clusters), and wsum [n] int64 as a fourth value with want_wsum.

    points: a numpy array [n, 2 or 3].  weights: non-negative int32 [n] or None (every row once).  aux [n] with gate:
    rows are neighbours only when |aux[i] - aux[j]| <= gate too.  A row is core when the weights of its neighbourhood
    (itself included) sum to min_weight or more; labels run from cf_in + 1, 0 = noise."""
    ctx = ctx or default_context()
    r = ctx.gdbscan(np.asarray(points, np.float64), float(eps), int(min_weight), _metric(metric), weights, aux, gate,
                    int(cf_in), want_wsum)
    out = (r["labels"], r["is_core"].astype(bool), r["cf"] - int(cf_in))
    return out + (r["wsum"],) if want_wsum else out


def multiplicity(rows):
    """(first_index, counts): the first occurrence of every distinct row of `rows` [n, d] in input order and how often the
    row occurs -- the import's duplicate removal with the count kept.  gdbscan(rows[first_index], ..., weights=counts) is
    then the clustering of the raw cloud, restricted to the first occurrences.  Rows are compared bit for bit (so -0.0
    and 0.0 differ, and a NaN row equals a NaN row of the same bits).
    The device form is vcp_import_compact (Context.import_compact, io.import_scan_resident): its src and count are this
    function's pair for the converted triples of a scan, computed without leaving HBM.  The one difference: the device
    compares with the C#'s `==`, so there -0.0 equals 0.0 and a row holding a NaN equals nothing, itself included."""
    rows = np.ascontiguousarray(rows, np.float64)
    if rows.ndim != 2:
        raise ValueError("rows must be [n, d]")
    if len(rows) == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int32)
    keys = rows.view(np.dtype((np.void, rows.dtype.itemsize * rows.shape[1]))).ravel()
    _, first, counts = np.unique(keys, return_index=True, return_counts=True)
    order = np.argsort(first, kind="stable")
    return first[order].astype(np.int64), counts[order].astype(np.int32)
