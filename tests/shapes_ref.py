"""The rectangle and the filter of include/vcp.h ("cluster shapes") restated in numpy, for the shapes tests.  Every
operation is a binary64 ufunc call of its own (numpy contracts nothing), so the figures are the definition's, bit for
bit.  No GPU, no oracle: the hull comes from the caller."""
import numpy as np

INF = np.inf


def edge_boxes(hull, members=None):
    """For every hull edge i: None when the edge is no candidate, else dict(area, U, V, L2, a, d, u0, u1, v0, v1).
    members: the extents are taken over these points instead of over the hull (a cluster on which the insertion rule
    of the circle fired: the hull is incomplete); members with both coordinates NaN are left out, as HullCull does."""
    hull = np.ascontiguousarray(hull, np.float64).reshape(-1, 2)
    h = len(hull)
    src = hull
    if members is not None:
        src = np.ascontiguousarray(members, np.float64).reshape(-1, 2)
        src = src[~(np.isnan(src[:, 0]) & np.isnan(src[:, 1]))]
    out = []
    with np.errstate(all="ignore"):
        for i in range(h):
            a, b = hull[i], hull[(i + 1) % h]
            dx, dy = b[0] - a[0], b[1] - a[1]
            L2 = dx * dx + dy * dy
            if not (0 < L2 < INF):
                out.append(None)
                continue
            rx, ry = src[:, 0] - a[0], src[:, 1] - a[1]
            u = rx * dx + ry * dy
            v = ry * dx - rx * dy
            # exact extremes (NaN propagates); a zero extreme counts as +0
            u0, u1, v0, v1 = (np.float64(x) + 0.0 for x in (u.min(), u.max(), v.min(), v.max()))
            U, V = u1 - u0, v1 - v0
            area = (U * V) / L2
            if not area < INF:
                out.append(None)
                continue
            out.append(dict(area=area, U=U, V=V, L2=L2, a=a.copy(), d=np.array([dx, dy]), u0=u0, u1=u1, v0=v0, v1=v1))
    return out


def rectangle(hull, members=None):
    """dict(valid, edge, len [2], xy [4, 2], areas) of the minimum-area bounding rectangle of a hull (the circle of
    the cluster being valid): the smallest area_i, the lowest i on ties.  members: see edge_boxes."""
    hull = np.ascontiguousarray(hull, np.float64).reshape(-1, 2)
    boxes = edge_boxes(hull, members)
    best = -1
    for i, e in enumerate(boxes):
        if e is not None and (best < 0 or e["area"] < boxes[best]["area"]):
            best = i
    areas = [None if e is None else float(e["area"]) for e in boxes]
    if best < 0:
        return dict(valid=0, edge=-1, len=np.zeros(2), xy=np.tile(hull[0], (4, 1)), areas=areas)
    e = boxes[best]
    with np.errstate(all="ignore"):
        L = np.sqrt(e["L2"])
        ln = np.array([e["U"] / L, e["V"] / L])
        (ax, ay), (dx, dy), L2 = e["a"], e["d"], e["L2"]
        xy = np.array([[ax + (u * dx - v * dy) / L2, ay + (u * dy + v * dx) / L2]
                       for u, v in ((e["u0"], e["v0"]), (e["u1"], e["v0"]), (e["u1"], e["v1"]), (e["u0"], e["v1"]))])
    return dict(valid=1, edge=best, len=ln, xy=xy, areas=areas)


def cluster_filter(labels, K, radius, valid, rect_len, rect_valid, max_radius, max_aspect):
    """dict(filtered [K], keep [n], kept_idx, n_filtered, n_kept): plain comparisons, no division."""
    labels = np.asarray(labels, np.int64)
    radius = np.asarray(radius, np.float64)
    valid = np.asarray(valid)
    with np.errstate(all="ignore"):
        f = radius > max_radius
        if rect_len is not None and rect_valid is not None:
            rl = np.asarray(rect_len, np.float64).reshape(-1, 2)
            f = f | ((np.asarray(rect_valid) == 1) & (rl.max(1) > max_aspect * rl.min(1)))
    filtered = ((valid == 1) & f).astype(np.uint8)
    inside = (labels >= 1) & (labels <= K)
    hit = np.zeros(len(labels), bool)
    hit[inside] = filtered[labels[inside] - 1] != 0
    keep = (~hit).astype(np.uint8)
    kept_idx = np.flatnonzero(keep).astype(np.int32)
    return dict(filtered=filtered, keep=keep, kept_idx=kept_idx, n_filtered=int(filtered.sum()), n_kept=len(kept_idx))


def members(labels, K, order=None):
    """List of K index arrays: the points of cluster k + 1 in list order (order = the list the C# iterates)."""
    labels = np.asarray(labels)
    order = np.arange(len(labels), dtype=np.int64) if order is None else np.asarray(order, np.int64)
    lab = labels[order]
    srt = np.argsort(lab, kind="stable")
    cuts = np.searchsorted(lab[srt], np.arange(1, K + 2))
    return [order[srt[cuts[k]:cuts[k + 1]]] for k in range(K)]


def inside_rectangle(pts, xy, tol):
    """Largest violation (<= 0 when inside) of the points against the rectangle with corners xy [4, 2]: the distance
    beyond the line of each of its four edges, measured along that edge's own normal.  (Measured along the neighbouring
    side instead, a rectangle whose width is a few ulps of its corners has no usable direction: the rounding of the
    corners turns that side anywhere.)  An edge of length zero bounds along the direction of the edge before it; without
    an area the distance from the line counts on both sides."""
    pts = np.asarray(pts, np.float64).reshape(-1, 2)
    q = np.asarray(xy, np.float64).reshape(4, 2)
    e = np.roll(q, -1, axis=0) - q
    l = np.hypot(e[:, 0], e[:, 1])
    a, b, c = q[1] - q[0], q[2] - q[0], q[3] - q[0]  # twice the area, from differences of neighbouring corners
    sgn = np.sign((a[0] * b[1] - a[1] * b[0]) + (b[0] * c[1] - b[1] * c[0]))
    worst = -INF
    for i in range(4):
        r = pts - q[i]
        if l[i] > 0:
            d = (e[i, 0] * r[:, 1] - e[i, 1] * r[:, 0]) / l[i]  # > 0: to the left of the edge
            d = -sgn * d if sgn else np.abs(d)
        elif l[i - 1] > 0:
            d = r @ e[i - 1] / l[i - 1]
        else:
            d = np.hypot(r[:, 0], r[:, 1])
        worst = max(worst, float(d.max()))
    return worst - tol
