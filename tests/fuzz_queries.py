"""Randomised parity sweep of the query entry points that came after tests/fuzz_parity.py: vcp_kdist, vcp_eps_tree,
vcp_gdbscan, vcp_match_unique, vcp_register_pairs, vcp_register_sim and vcp_assign_truths, each against the restatement
of its definition that tests/ already holds (or the oracle), for equality.  Each of them has a uniform grid of its own;
the fixed tests run those grids near the origin, on quantised coordinates and with round thresholds.  Here every case
draws one transform

    asis      fuzz_parity's cloud as it is
    shift     an unquantised cloud moved by 1e5, -7e5 or 2^40 (x - x0 rounds)
    scale     multiplied by 2^-83 or 2^116 (exact: the same pairs stay neighbours)
    nearthr   a family of tests/nearthr.py on one of its own frames (pairs AT / IN / OUT of eps by ulps)
    outliers  a handful of points at 1e3 .. 1e9 times the extent (the 2^22-cell cap doubles the cell edge)

and takes its threshold, in half the cases, from a distance that occurs in the case itself -- or the double just below or
above it -- the only inputs that tell `<` from `<=` and show a cell edge one rounding too small.

Every family is split in two: make_<family>(rng) builds the inputs and the reference result on the CPU (no GPU; the
case list is a function of the seed alone: fixed counts, no time budget), check_<family>(ctx, case) runs the device and
compares.  tests/test_fuzz_queries.py holds the case lists to conditions that keep the sweep from passing by being empty,
tests/test_fuzz_queries_gpu.py runs the bounded form on the GPU.
usage: python tests/fuzz_queries.py [cases per family] [seed]      (the register families run half as many)"""
import math
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import eps_tree_ref as ET  # noqa: E402
import fuzz_parity as FP  # noqa: E402  (its cloud())
import gdbscan_ref as GD  # noqa: E402
import kdist_ref as KR  # noqa: E402
import match_unique_ref as MU  # noqa: E402
import nearthr as NT  # noqa: E402
import register_ref as RR  # noqa: E402
import register_sim_ref as RS  # noqa: E402
from oracle import binding as O  # noqa: E402  (test tooling: vcp_assign_truths's reference)
from vtkcloudpoint_amd import _native as N  # noqa: E402
from vtkcloudpoint_amd import epstree as E  # noqa: E402

ctx = None
done = {}
spent = {}                # family -> [seconds building cases and references, seconds in check_<family>] of the last run()
QUIET = [False]

FAMILIES = ("kdist", "eps_tree", "gdbscan", "match_unique", "register_pairs", "register_sim", "assign_truths")
HALF = ("register_pairs", "register_sim")     # families that run half the cases (their restatement is the slowest)
TRANSFORMS = ("asis", "shift", "scale", "nearthr", "outliers")
SHIFTS = (1e5, -7e5, 2.0 ** 40)
SCALES = (2.0 ** -83, 2.0 ** 116)
VARIANTS = ("below", "at", "above")
N_MAX = 2000
PAIRS_MAX = 600_000       # pairs within eps a quadratic restatement walks in Python; a larger case is cut in half
# the bounded form of tests/test_fuzz_queries*.py: family -> (cases, seed); the seeds were picked so that the conditions
# of tests/test_fuzz_queries.py hold on the lists
SUITE = {"kdist": (48, 1), "eps_tree": (48, 1), "gdbscan": (48, 1), "match_unique": (48, 1),
         "register_pairs": (24, 1), "register_sim": (24, 1), "assign_truths": (48, 2)}


class Mismatch(AssertionError):
    pass


def say(*a, **k):
    if not QUIET[0]:
        print(*a, **k)


def fail(case, msg):
    """Inputs to an .npz under the temporary directory, the message names family, case number, seed and transform."""
    dump = os.path.join(tempfile.gettempdir(), "fuzz_queries_fail_%s.npz" % case["family"])
    arrays = {k: v for k, v in case.items() if isinstance(v, (np.ndarray, int, float, bool, str))}
    np.savez(dump, **arrays)
    text = "MISMATCH %s case %d seed %d transform %s: %s (inputs in %s)" % (
        case["family"], case["index"], case["seed"], case["tag"], msg, dump)
    print(text, flush=True)
    raise Mismatch(text)


# ---- clouds ----------------------------------------------------------------------------------------------------------
def log_int(rng, lo, hi):
    return int(min(hi, max(lo, round(10 ** rng.uniform(math.log10(lo), math.log10(hi))))))


def gd_of(metric):
    return 3 if metric == N.L2_3D else 2


def base_cloud(rng, n, dim, unquantised=False):
    """fuzz_parity.cloud on this stream; unquantised: not its lattice and not its 2^-10 grid."""
    FP.rng = rng
    for _ in range(50):
        c = FP.cloud(n, dim)
        if not (unquantised and FP.KIND[0] in (2, 6)):
            break
    return c


def extent_of(c):
    fin = c[np.isfinite(c).all(1)]
    ext = float((fin.max(0) - fin.min(0)).max()) if len(fin) else 0.0
    return ext if ext > 0.0 and math.isfinite(ext) else 1.0


def add_outliers(rng, c):
    """A handful of rows at 1e3 .. 1e9 times the extent from the middle of the cloud."""
    n, dim = c.shape
    fin = c[np.isfinite(c).all(1)]
    mid = (fin.max(0) + fin.min(0)) * 0.5 if len(fin) else np.zeros(dim)
    m = int(min(n, rng.integers(1, 6)))
    rows = rng.choice(n, m, replace=False)
    u = rng.normal(size=(m, dim))
    c = c.copy()
    c[rows] = mid + u * (extent_of(c) * 10.0 ** rng.uniform(3, 9, (m, 1)))
    return c


def frame_of(rng, allowed):
    """One transform of `allowed` with equal odds, and its parameter: dict(transform, tag, unit, shift, floor)."""
    t = str(rng.choice([x for x in TRANSFORMS if x in allowed]))
    fr = dict(transform=t, tag=t, unit=1.0, shift=0.0, floor=0.0)
    if t == "shift":
        fr["shift"] = float(rng.choice(SHIFTS))
        fr["tag"] = "shift %r" % fr["shift"]
        if abs(fr["shift"]) == 2.0 ** 40:      # a coordinate's ulp is 2^-12 there: a drawn threshold spans several
            fr["floor"] = float(rng.uniform(4.0, 64.0)) * 2.0 ** -12
    elif t == "scale":
        fr["unit"] = float(rng.choice(SCALES))
        fr["tag"] = "scale 2^%d" % round(math.log2(fr["unit"]))
    return fr


def apply_frame(rng, fr, c):
    if fr["transform"] == "shift":
        return c + fr["shift"]
    if fr["transform"] == "scale":
        return c * fr["unit"]
    if fr["transform"] == "outliers":
        return add_outliers(rng, c)
    return c


def nearthr_cloud(rng, metric, k):
    """(coords, eps, tag) of a near-threshold family on one of its frames, sized to N_MAX: isolated pairs, rings of
    3 k points round a probe that is core at min_pts = k by one point, dumbbells of clumps of k points."""
    frames = NT.frames(metric)
    frame = frames[int(rng.integers(len(frames)))]
    seed = int(rng.integers(1 << 31))
    fam = int(rng.integers(3))
    if fam == 1 and k >= 2:
        d, name = NT.rings_cloud(metric, frame, seed, n_rings=4, ring=max(3 * k, 60), inside=k - 1), "rings"
    elif fam == 2 and 3 <= k <= 80:
        d, name = NT.dumbbells_cloud(metric, frame, seed, n_bells=12, min_pts=k), "dumbbells"
    else:
        d, name = NT.pairs_cloud(metric, frame, seed, n_pairs=int(rng.integers(50, 700)), n_axis=100), "pairs"
    return np.ascontiguousarray(d["coords"]), float(d["eps"]), "nearthr %s %s" % (name, frame[0])


def draw_k(rng, values, n):
    """min_pts of a DBSCAN-like case on n points, from `values`.  One case in six: any of them (k > n included: nobody
    is core).  The others: one with 3 <= k <= n / 2 where there is one -- below 3 a cloud has no border point, and a k
    near n or beyond leaves nothing to decide -- else one that is <= n."""
    if rng.random() * 6.0 < 1.0:
        return int(rng.choice(values))
    fit = [v for v in values if 3 <= v <= n // 2] or [v for v in values if v <= n] or [min(values)]
    return int(rng.choice(fit))


def query_cloud(rng, metric, k, n, allowed=TRANSFORMS):
    """dict(c, metric, tag, transform, unit, floor, frame_eps): the cloud of a DBSCAN-like case (n rows, except on a
    near-threshold frame, whose families have sizes of their own)."""
    fr = frame_of(rng, allowed)
    if fr["transform"] == "nearthr":
        c, eps, tag = nearthr_cloud(rng, metric, k)
        fr.update(tag=tag, frame_eps=eps)
    else:
        dim = 3 if metric == N.L2_3D else int(rng.integers(2, 4))
        c = base_cloud(rng, n, dim, unquantised=fr["transform"] == "shift")
        c = apply_frame(rng, fr, c)
        fr["frame_eps"] = None
    fr["c"] = np.ascontiguousarray(c)
    return fr


# ---- thresholds ------------------------------------------------------------------------------------------------------
def vary(rng, d):
    """d, or the double just below or above it, with equal odds: (value, variant name)."""
    v = int(rng.integers(3))
    return float((np.nextafter(d, -np.inf), d, np.nextafter(d, np.inf))[v]), VARIANTS[v]


def threshold(rng, own, drawn):
    """Half the cases: a value of own() (a distance of the case) through vary(); the others: drawn().  Returns
    (value, "own" | "drawn", variant | "")."""
    if rng.random() < 0.5:
        d = own()
        if d is not None and math.isfinite(d):
            v, name = vary(rng, d)
            return v, "own", name
    return float(drawn()), "drawn", ""


def small_distance(rng, D, max_rank=64, rank=0):
    """One finite entry of the distance matrix D [a, b], of a random row: the `rank`-th smallest (rank 0: the nearest)
    in three draws of five, else the value of a log-uniform rank up to max_rank.  (A uniform draw over all pairs is
    about half the extent: everything one cluster.  The rank of a DBSCAN-like case is min_pts - 1, the row's own
    k-distance: at that eps, and not below it, the row is core.)"""
    if D.size == 0:
        return None
    row = D[int(rng.integers(len(D)))]
    row = np.sort(row[np.isfinite(row)])
    if len(row) == 0:
        return None
    r = rank if rng.random() < 0.6 else log_int(rng, 1, max_rank) - 1
    return float(row[min(len(row) - 1, r)])


def density_eps(rng, c, metric, fr):
    """fuzz_parity's eps: from none to a few dozen neighbours by the robust extent, or a round value (0 included), in
    the frame's unit."""
    gd = gd_of(metric)
    n = len(c)
    fin = c[np.isfinite(c).all(axis=1)]
    if len(fin) > 10:
        q = np.percentile(fin[:, :gd], [2, 98], axis=0)
        spans = np.maximum(q[1] - q[0], 0.0)
    else:
        spans = np.full(gd, fr["unit"])
    live = spans[spans > 0]
    vol = float(np.prod(live)) if len(live) else fr["unit"]
    eps = float((rng.uniform(0.2, 30) * vol / max(n, 1)) ** (1.0 / max(len(live), 1)))
    if rng.random() < 0.15:
        eps = float(rng.choice([0.0, 0.25, 1.0, 3.0])) * fr["unit"]
    return max(eps, fr["floor"]) if eps > 0.0 else eps


def dbscan_inputs(rng, metric, k, n, rank=None):
    """Cloud, distance matrix and eps of a DBSCAN-like case, cut in half while more than PAIRS_MAX pairs lie within eps.
    rank: which of a row's sorted distances an own eps is (default k - 1: the row's k-distance)."""
    fr = query_cloud(rng, metric, k, n)
    c = fr["c"]
    D = ET.dist_matrix(c, metric)
    if fr["frame_eps"] is not None and (D == fr["frame_eps"]).any():
        eps, variant = vary(rng, fr["frame_eps"])      # the frame's eps is the distance of its AT pairs
        mode = "own"
    else:
        eps, mode, variant = threshold(rng, lambda: small_distance(rng, D, rank=max(k, 1) - 1 if rank is None else rank),
                                       lambda: density_eps(rng, c, metric, fr))
    with np.errstate(invalid="ignore"):
        while int((D <= eps).sum()) > PAIRS_MAX:
            c = np.ascontiguousarray(c[:len(c) // 2])
            D = D[:len(c), :len(c)]
    fr.update(c=c, D=D, eps=eps, mode=mode, variant=variant, metric=metric,
              finite_rows=int(ET.finite_rows(c, metric).sum()))
    return fr


def case_of(family, fr, **more):
    out = dict(family=family, tag=fr["tag"], transform=fr["transform"], mode=fr["mode"], variant=fr["variant"],
               refusal=None)
    out.update(more)
    out["degenerate"] = bool(out["refusal"] is not None or out["finite_rows"] < 2)
    return out


def refused(case, call):
    """call() on the device under the rule for refusals: the same error code on both sides counts as compared (returns
    None), a refusal of one side alone is a mismatch."""
    try:
        got = call()
    except N.VcpError as e:
        if case["refusal"] != e.code:
            fail(case, "the device refuses with %d, the reference %s" % (e.code, case["refusal"]))
        return None
    if case["refusal"] is not None:
        fail(case, "the reference refuses with %d, the device does not" % case["refusal"])
    return got


def same_doubles(a, b):
    """Bits of the doubles; a NaN equals a NaN of any payload."""
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    if a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    return np.array_equal(a[~np.isnan(a)].view(np.uint64), b[~np.isnan(b)].view(np.uint64))


# ---- kdist -----------------------------------------------------------------------------------------------------------
def dbscan_stats(ref, Nb):
    """(clusters, whether a non-core point carries a label) of a gdbscan_ref result with its neighbourhood matrix."""
    core = ref["is_core"].astype(bool)
    border = bool(((Nb & core[None, :]).any(1) & ~core).any())
    return int(ref["cf"]), border


def make_kdist(rng):
    metric = int(rng.integers(0, 3))
    n = log_int(rng, 1, N_MAX)
    k = draw_k(rng, [1, 2, 3, 5, 16, 17, 64], n)
    fr = dbscan_inputs(rng, metric, k, n)
    c, eps = fr["c"], fr["eps"]
    kd, knn = KR.brute_rows(c, k, metric, np.arange(len(c)))
    live = np.flatnonzero(np.isfinite(kd))
    eps_list = [eps]                               # vcp.h states the identity for every finite eps >= 0
    if len(live):
        v = float(kd[live[int(rng.integers(len(live)))]])
        eps_list += [v, float(np.nextafter(v, -np.inf))]
    eps_list = [e for e in eps_list if math.isfinite(e) and e >= 0.0]
    ref = GD.gdbscan(c, eps, k, metric)
    clusters, border = dbscan_stats(ref, GD.neighbourhoods(c, eps, metric))
    with np.errstate(invalid="ignore"):
        decides = bool((kd == eps).any())        # a k-th neighbour at exactly eps: the flag changes just below
    return case_of("kdist", fr, c=c, metric=metric, k=k, eps=eps, kd=kd, knn=knn, eps_list=np.array(eps_list),
                   finite_rows=fr["finite_rows"], clusters=clusters, border=border, decides=decides, ref=ref)


def check_kdist(ctx, case):
    c, k, metric = case["c"], case["k"], case["metric"]
    got = refused(case, lambda: ctx.kdist(c, k, metric, want_knn=True))
    if got is None:
        return
    if not np.array_equal(got[0], case["kd"], equal_nan=True):
        fail(case, "kdist differs from the brute force (n %d k %d metric %d)" % (len(c), k, metric))
    if not np.array_equal(got[1], case["knn"]):
        fail(case, "knn differs from the brute force (n %d k %d metric %d)" % (len(c), k, metric))
    for eps in case["eps_list"].tolist():
        g = ctx.dbscan(c, eps, k, metric)
        with np.errstate(invalid="ignore"):
            want = (case["kd"] <= eps).astype(np.uint8)
        if not np.array_equal(g["is_core"], want):
            fail(case, "dbscan(eps %r, min_pts %d).is_core is not kdist <= eps at rows %s" % (
                eps, k, np.flatnonzero(g["is_core"] != want)[:5].tolist()))


# ---- eps_tree --------------------------------------------------------------------------------------------------------
def make_eps_tree(rng):
    metric = int(rng.integers(0, 3))
    n = log_int(rng, 1, N_MAX)
    k = draw_k(rng, [1, 2, 4, 10], n)
    fr = dbscan_inputs(rng, metric, k, n, rank=max(k, 2) - 1)      # (eps_max = 0 is refused)
    c, eps_max = fr["c"], fr["eps"]
    refusal = None if (eps_max > 0.0 and math.isfinite(eps_max)) else RR.ERR_ARG
    out = dict(c=c, metric=metric, k=k, eps=eps_max, finite_rows=fr["finite_rows"], refusal=refusal, clusters=0,
               border=False, decides=False, probes=np.zeros(0))
    if refusal is None:
        ref = ET.eps_tree(c, k, eps_max, metric)
        with np.errstate(invalid="ignore"):
            cores = int((ref["kdist"] <= eps_max).sum())
            labelled = int((ref["reach"] <= eps_max).sum())
            decides = bool((ref["kdist"] == eps_max).any())
            pool = np.concatenate([ref["merge_w"], ref["reach"][ref["reach"] <= eps_max]])
        probes = []
        if len(pool) and fr["finite_rows"] == len(c):     # vcp.h states the identities for all-finite input
            for v in pool[rng.integers(0, len(pool), 5)].tolist():
                probes += [v, float(np.nextafter(v, -np.inf))]
        out.update(ref=ref, clusters=cores - ref["n_merge"], border=labelled > cores, decides=decides,
                   probes=np.array([p for p in probes if p >= 0.0]))
    return case_of("eps_tree", fr, **out)


def check_eps_tree(ctx, case):
    c, k, metric, eps_max = case["c"], case["k"], case["metric"], case["eps"]
    r = refused(case, lambda: ctx.eps_tree(c, k, eps_max, metric))
    if r is None:
        return
    ref = case["ref"]
    bad = ET.same(r, ref)
    if bad is not None:
        fail(case, "%s differs from the walk (n %d k %d eps_max %r metric %d)" % (bad, len(c), k, eps_max, metric))
    if r["rounds"] > ET.round_bound(ref["n_p"]):
        fail(case, "%d rounds for |P| = %d" % (r["rounds"], ref["n_p"]))
    kd, _ = ctx.kdist(c, k, metric)
    if not same_doubles(r["kdist"], kd):
        fail(case, "the tree's kdist is not vcp_kdist's")
    tree = E.EpsTree(r["kdist"], r["reach"], r["merge_w"], r["merge_a"], r["merge_b"], eps_max, k, r["rounds"])
    for eps in case["probes"].tolist():
        g = ctx.dbscan(c, eps, k, metric)
        want = (int(g["is_core"].sum()), int(g["cf"]), int((g["labels"] != 0).sum()))
        if E.counts_at(tree, eps) != want:
            fail(case, "counts_at(%r) = %s, dbscan gives %s" % (eps, E.counts_at(tree, eps), want))


# ---- gdbscan ---------------------------------------------------------------------------------------------------------
def make_gdbscan(rng):
    metric = int(rng.integers(0, 3))
    n = log_int(rng, 1, N_MAX)
    mw = draw_k(rng, [0, 1, 2, 3, 5, 7, 17, 40], n)
    fr = dbscan_inputs(rng, metric, mw, n)
    c, D, eps = fr["c"], fr["D"], fr["eps"]
    n = len(c)
    cf_in = int(rng.integers(-4, 11))
    wkind = int(rng.integers(3))                  # none, 1 .. 3, 0 .. 3
    weights = None if wkind == 0 else rng.integers(2 - wkind, 4, n).astype(np.int32)
    aux, gate, gate_mode = None, None, ""
    if rng.random() < 0.5:
        aux = rng.uniform(0.0, 10.0, n) if rng.random() < 0.5 else rng.integers(0, 3, n).astype(np.float64)
        if rng.random() < 0.2 and n > 3:
            aux[rng.integers(0, n, max(1, n // 200))] = float(rng.choice([np.nan, np.inf]))

        def own():
            with np.errstate(invalid="ignore"):
                i, j = np.nonzero(np.triu(D <= eps, 1))
            if len(i) == 0:
                return None
            with np.errstate(invalid="ignore"):
                t = int(rng.integers(len(i)))
                return float(abs(aux[i[t]] - aux[j[t]]))
        gate, gate_mode, _ = threshold(rng, own, lambda: rng.choice([0.0, 0.5, 1.0, 3.0, np.inf]))
        if not gate >= 0.0:                       # (the double below a zero difference)
            gate = 0.0
    ref = GD.gdbscan(c, eps, mw, metric, weights, aux, gate, cf_in)
    Nb = GD.neighbourhoods(c, eps, metric, aux, gate)
    clusters, border = dbscan_stats(ref, Nb)
    w = np.ones(n, np.int64) if weights is None else weights.astype(np.int64)
    below = GD.neighbourhoods(c, float(np.nextafter(eps, -np.inf)), metric, aux, gate).astype(np.int64) @ w >= mw
    out = dict(c=c, metric=metric, eps=eps, mw=mw, cf_in=cf_in, finite_rows=fr["finite_rows"], ref=ref,
               clusters=clusters - cf_in, border=border, decides=bool((below != ref["is_core"].astype(bool)).any()),
               gate_mode=gate_mode, plain=None, expanded=None)
    if weights is not None:
        out["weights"] = weights
    if aux is not None:
        out.update(aux=aux, gate=float(gate))
    # vcp_dbscan has the same answer in two cases (include/vcp.h); a negative cf_in is compared from cf_in = 0 on
    cf0 = max(cf_in, 0)
    if aux is None and weights is None:
        out["plain"] = ref if cf0 == cf_in else GD.gdbscan(c, eps, mw, metric, cf_in=cf0)
    # (the copies of a row must be each other's neighbours: not so where N is empty, which min_weight <= 0 makes core)
    if aux is None and weights is not None and int(weights.min(initial=1)) >= 1 and int(weights.sum()) <= 6000 \
            and (mw >= 1 or bool(Nb.diagonal().all())):
        out["expanded"] = ref if cf0 == cf_in else GD.gdbscan(c, eps, mw, metric, weights, cf_in=cf0)
    return case_of("gdbscan", fr, **out)


def check_gdbscan(ctx, case):
    c, eps, mw, metric, cf_in = case["c"], case["eps"], case["mw"], case["metric"], case["cf_in"]
    w, aux, gate = case.get("weights"), case.get("aux"), case.get("gate")
    what = "(n %d eps %r min_weight %d metric %d weights %s aux %s gate %r cf_in %d)" % (
        len(c), eps, mw, metric, w is not None, aux is not None, gate, cf_in)
    g = refused(case, lambda: ctx.gdbscan(c, eps, mw, metric, w, aux, gate, cf_in, want_wsum=True))
    if g is None:
        return
    bad = GD.same(g, case["ref"])
    if bad is not None:
        fail(case, "%s differs from the restatement %s" % (bad, what))
    e = ctx.gdbscan(c, eps, mw, metric, w, aux, gate, cf_in)
    bad = GD.same(e, case["ref"])
    if bad is not None or e["wsum"] is not None:
        fail(case, "%s differs without wsum %s" % (bad, what))
    n, cf0 = len(c), max(cf_in, 0)
    if case["plain"] is not None:
        d = ctx.dbscan(c, eps, mw, metric, cf0)
        bad = GD.same(dict(labels=d["labels"], is_core=d["is_core"], cf=d["cf"]), case["plain"], wsum=False)
        if bad is not None:
            fail(case, "vcp_dbscan's %s differs from the restatement %s" % (bad, what))
    if case["expanded"] is not None:
        d = ctx.dbscan(GD.expand(c, w), eps, mw, metric, cf0)
        bad = GD.same(dict(labels=d["labels"][:n], is_core=d["is_core"][:n], cf=d["cf"]), case["expanded"], wsum=False)
        if bad is not None:
            fail(case, "vcp_dbscan's %s on the expanded cloud differs from the restatement %s" % (bad, what))


# ---- match_unique ----------------------------------------------------------------------------------------------------
def rigid(rng, at):
    """A rotation about z by a drawn angle and a translation of the size of `at`: row-major 4 x 4."""
    a = float(rng.uniform(0.0, 2.0 * math.pi))
    M = np.eye(4)
    M[:3, :3] = RR.rz(a)
    M[:3, 3] = rng.normal(0.0, 1.0, 3) * at
    return M


def pull_back(M, x):
    """The rows c with M (c, 1) ~ x (up to rounding: it only builds inputs)."""
    with np.errstate(all="ignore"):
        return np.ascontiguousarray((x - M[:3, 3]) @ M[:3, :3])


def nearest_of(D, max_dist):
    """vcp_match's rule on the matrix D [K, T] (a NaN distance never wins): (nearest [K], matched [K])."""
    Dn = np.where(np.isnan(D), np.inf, D)
    nearest = Dn.argmin(1)
    nd = Dn[np.arange(len(D)), nearest]
    return nearest, (nd < max_dist) & (nd < np.inf)


def make_match_unique(rng):
    fr = frame_of(rng, ("asis", "shift", "scale", "outliers"))
    T = log_int(rng, 1, N_MAX)
    truths = base_cloud(rng, T, 3, unquantised=fr["transform"] == "shift")
    if rng.random() < 0.5:
        truths[:, 2] = 0.0                        # the planar field the reference feeds
    ext = extent_of(truths) * fr["unit"]         # of the bulk: before any outlier
    truths = np.ascontiguousarray(apply_frame(rng, fr, truths))
    M = rigid(rng, ext)
    # noise from a thousandth to a tenth of the truths' mean spacing (extent / T^(1/3))
    sigma = ext * float(rng.choice([1e-4, 1e-3, 1e-2])) / max(1.0, T ** (1.0 / 3.0)) * 10.0
    room = N_MAX
    n_det = int(min(room, max(1, round(T * rng.uniform(0.3, 1.0)))))
    det = truths[rng.integers(0, T, n_det)] + rng.normal(0.0, sigma, (n_det, 3))
    n_near = int(rng.integers(0, max(1, min(room - n_det, n_det) + 1)))
    near = det[rng.integers(0, n_det, n_near)] + rng.normal(0.0, 2.0 * sigma, (n_near, 3))
    fin = truths[np.isfinite(truths).all(1)]
    lo, hi = (fin.min(0), fin.max(0)) if len(fin) else (np.zeros(3), np.ones(3))
    n_far = int(min(room - n_det - n_near, rng.integers(0, 40)))
    far = rng.uniform(lo - 0.1 * ext, hi + 0.1 * ext, (n_far, 3))
    n_out = int(min(room - n_det - n_near - n_far, rng.integers(0, 8)))
    outside = hi + ext * 10.0 ** rng.uniform(-2, 4, (n_out, 3)) * rng.choice([-1.0, 1.0], (n_out, 3))
    moved = np.concatenate([det, near, far, outside])
    moved = moved[rng.permutation(len(moved))]
    centers = pull_back(M, moved)
    if rng.random() < 0.1:
        which = centers if rng.random() < 0.5 else truths
        which[int(rng.integers(len(which))), int(rng.integers(3))] = float(rng.choice([np.nan, np.inf, -np.inf]))
    m = MU.transform(centers, M)
    D = MU.distances(m[:, None, :], truths[None, :, :])
    unit = sigma
    max_dist, mode, variant = threshold(rng, lambda: small_distance(rng, D, 3),
                                        lambda: unit * rng.choice([0.0, 1.0, 3.0, 10.0, 30.0]) if len(D) * T > 20000
                                        else rng.choice([0.0, unit, 3.0 * unit, 30.0 * unit, np.inf]))
    with np.errstate(invalid="ignore"):
        while int((D < max_dist).sum()) > PAIRS_MAX:
            centers, m, D = np.ascontiguousarray(centers[:len(centers) // 2]), m[:len(m) // 2], D[:len(D) // 2]
    ref = MU.greedy_matching(centers, truths, M, max_dist)
    nearest, matched = nearest_of(D, max_dist)      # match_unique_ref.nearest_match's rule, NaN rows allowed
    contested = len(np.unique(nearest[matched])) < int(matched.sum())
    dropped = False
    with np.errstate(invalid="ignore"):
        if (D == max_dist).any() and math.isfinite(max_dist):     # a pair at exactly max_dist: is it the only reason?
            above = MU.greedy_matching(centers, truths, M, float(np.nextafter(max_dist, np.inf)))
            dropped = not np.array_equal(above["truth_of"], ref["truth_of"])
    fr.update(mode=mode, variant=variant)
    finite = int(min(np.isfinite(centers).all(1).sum(), np.isfinite(truths).all(1).sum()))
    return case_of("match_unique", fr, centers=centers, truths=truths, M=M, max_dist=max_dist, ref=ref,
                   finite_rows=finite, contested=bool(contested), dropped=bool(dropped))


def check_match_unique(ctx, case):
    centers, truths, M, max_dist = case["centers"], case["truths"], case["M"], case["max_dist"]
    g = refused(case, lambda: ctx.match_unique(centers, truths, M, max_dist))
    if g is None:
        return
    ref = case["ref"]
    what = "(K %d T %d max_dist %r)" % (len(centers), len(truths), max_dist)
    for key in ("truth_of", "center_of"):
        if not np.array_equal(g[key], ref[key]):
            fail(case, "%s differs from the greedy walk at %s %s" % (
                key, np.flatnonzero(g[key] != ref[key])[:5].tolist(), what))
    for key in ("pair_dist", "matched_xyz"):
        if not same_doubles(g[key], ref[key]):
            fail(case, "%s differs from the greedy walk %s" % (key, what))
    if g["count"] != ref["count"]:
        fail(case, "count %d, the greedy walk has %d %s" % (g["count"], ref["count"], what))
    # three properties of a matching, from the device's output alone
    js = np.flatnonzero(g["truth_of"] >= 0)
    if len(np.unique(g["truth_of"][js])) != len(js):
        fail(case, "a truth appears twice %s" % what)
    if not (g["pair_dist"][js] < max_dist).all():
        fail(case, "a pair at max_dist or beyond %s" % what)
    free_c = np.flatnonzero(g["truth_of"] < 0)
    free_t = np.flatnonzero(g["center_of"] < 0)
    if len(free_c) and len(free_t):
        d = MU.distances(g["matched_xyz"][free_c][:, None, :], truths[free_t][None, :, :])
        with np.errstate(invalid="ignore"):
            if ((d < max_dist) & (d < np.inf)).any():
                fail(case, "a free centroid and a free truth closer than max_dist %s" % what)


# ---- register_pairs and register_sim ---------------------------------------------------------------------------------
HYP_MAX = 200      # hypotheses per flip a case may have: each is scored against every target by the restatement


def register_scene(rng):
    """A partial-overlap scene built like register_ref.overlap_scene with drawn sizes, window, pose and noise, through a
    frame: dict(truths, source, bases, M (the planted pose), unit) and the frame."""
    fr = frame_of(rng, ("asis", "shift", "scale", "outliers"))
    nt = log_int(rng, 2, 300)
    field = float(rng.choice([1.0, 20.0, 300.0]))
    truths = np.zeros((nt, 3))
    truths[:, :2] = rng.uniform(0.0, field, (nt, 2))
    if rng.random() < 0.3:
        truths[:, 2] = rng.normal(0.0, 0.01 * field, nt)
    if rng.random() < 0.2:                         # exact ties among the lengths
        truths[:, :2] = np.round(truths[:, :2] / field * 16) * (field / 16)
    window = field * float(rng.uniform(0.4, 1.0))
    noise = field * float(rng.choice([0.0, 5e-4, 5e-3]))
    seen = truths[(truths[:, 0] <= window) & (truths[:, 1] <= window)]
    seen = seen[rng.random(len(seen)) < 0.9].copy()
    seen[:, :2] += rng.normal(0.0, noise, (len(seen), 2))
    clutter = np.zeros((int(rng.integers(0, 11)), 3))
    clutter[:, :2] = rng.uniform(0.0, window, (len(clutter), 2))
    x = np.concatenate([seen, clutter])
    x = x[rng.permutation(len(x))]
    M = rigid(rng, field)
    M[2, 3] = 0.0
    unit = fr["unit"]
    if fr["transform"] == "shift":                 # both clouds far from the origin, the pose between them small
        truths, x = truths + fr["shift"], x + fr["shift"]
        M[:3, 3] = (np.eye(3) - M[:3, :3]) @ np.full(3, fr["shift"]) + M[:3, 3]
    elif fr["transform"] == "scale":
        truths, x = truths * unit, x * unit
        M[:3, 3] *= unit
    elif fr["transform"] == "outliers":
        truths = add_outliers(rng, truths)
    source = pull_back(M, x)
    ns = len(source)
    B = int(rng.integers(1, 17))
    bases = rng.integers(0, max(ns, 1), (B, 2)).astype(np.int32)
    if rng.random() < 0.1 and nt > 3:
        truths[int(rng.integers(nt)), int(rng.integers(3))] = float(rng.choice([np.nan, np.inf]))
    fr.update(truths=np.ascontiguousarray(truths), source=source, bases=bases, M=M, field=field * unit,
              noise=max(noise, 1e-3 * field) * unit, mirror=bool(rng.integers(2)),
              max_landmarks=int(rng.choice([200, 200, 50, 7])))
    return fr


def pair_lengths(sc):
    """(Lu [B], Lv [nt, nt]) as the header defines them."""
    src, tgt, bases = sc["source"], sc["truths"], sc["bases"]
    if len(src) == 0:                              # (refused: no base has a length)
        src = np.full((1, 3), np.nan)
    with np.errstate(all="ignore"):
        ux = src[bases[:, 1], 0] - src[bases[:, 0], 0]
        uy = src[bases[:, 1], 1] - src[bases[:, 0], 1]
        vx = tgt[None, :, 0] - tgt[:, None, 0]
        vy = tgt[None, :, 1] - tgt[:, None, 1]
        return np.sqrt(ux * ux + uy * uy), np.sqrt(vx * vx + vy * vy)


def inlier_threshold(rng, sc, run):
    """inlier_dist by the threshold rule: the own value is the distance from a landmark, moved by the pose that wins
    with a drawn inlier_dist, to its nearest target -- a distance the scoring of that very pose computes."""
    drawn = float(sc["noise"] * rng.choice([1.0, 3.0, 10.0, 100.0]))
    if rng.random() < 0.05:
        drawn = np.inf

    def own():
        try:
            r = run(drawn)
        except RR.RefError:
            return None
        if r["best"] < 0:
            return None
        src, tgt = sc["source"], sc["truths"]
        lm = src[RR.landmark_indices(len(src), sc["max_landmarks"])]
        m = RR.transform(r["M"][None], lm)[0]
        with np.errstate(all="ignore"):
            dx = tgt[None, :, 0] - m[:, None, 0]
            dy = tgt[None, :, 1] - m[:, None, 1]
            dz = tgt[None, :, 2] - m[:, None, 2]
            d = np.sqrt((dx * dx + dy * dy) + dz * dz)
        d = np.where(np.isnan(d), np.inf, d).min(1)
        d = d[np.isfinite(d) & (d > 0.0)]
        return float(d[int(rng.integers(len(d)))]) if len(d) else None
    return threshold(rng, own, lambda: drawn)


def register_case(family, sc, args, run, **more):
    refusal, ref = None, None
    try:
        ref = run(args["inlier_dist"])
    except RR.RefError as e:
        refusal = e.code
    finite = int(min(np.isfinite(sc["source"]).all(1).sum(), np.isfinite(sc["truths"]).all(1).sum()))
    return case_of(family, sc, source=sc["source"], truths=sc["truths"], bases=sc["bases"], mirror=sc["mirror"],
                   max_landmarks=sc["max_landmarks"], ref=ref, refusal=refusal, finite_rows=finite,
                   hypotheses=0 if ref is None else int(ref["n_hyp"].sum()), best=-1 if ref is None else ref["best"],
                   **args, **more)


def make_register_pairs(rng):
    sc = register_scene(rng)
    Lu, Lv = pair_lengths(sc)
    with np.errstate(all="ignore"):
        diff = np.abs(Lv[None, :, :] - Lu[:, None, None])
        ok = (Lv > 0.0) & (Lv < np.inf)
        diff = np.sort(diff[:, ok][(Lu > 0.0) & (Lu < np.inf)].ravel())
    diff = diff[np.isfinite(diff)]
    cap = float(np.nextafter(diff[HYP_MAX], -np.inf)) if len(diff) > HYP_MAX else np.inf
    len_tol, mode, variant = threshold(
        rng, lambda: float(diff[int(rng.integers(min(len(diff), HYP_MAX)))]) if len(diff) else None,
        lambda: min(cap, sc["noise"] * float(rng.choice([0.0, 1.0, 3.0, 10.0]))))
    if not len_tol >= 0.0:                        # (the double below a zero difference)
        len_tol = 0.0
    sc.update(mode=mode, variant=variant)

    def run(inlier):
        return RR.register(sc["source"], sc["truths"], sc["bases"], len_tol, inlier, sc["mirror"], sc["max_landmarks"])
    inlier, inl_mode, inl_variant = inlier_threshold(rng, sc, run)
    return register_case("register_pairs", sc, dict(len_tol=len_tol, inlier_dist=inlier), run, inlier_mode=inl_mode,
                         inlier_variant=inl_variant)


def check_register_pairs(ctx, case):
    g = refused(case, lambda: ctx.register_pairs(case["source"], case["truths"], case["bases"], case["len_tol"],
                                                 case["inlier_dist"], case["mirror"], case["max_landmarks"]))
    if g is None:
        return
    try:
        RR.same(g, case["ref"])
    except AssertionError as e:
        fail(case, "%s differs from the restatement (ns %d nt %d B %d len_tol %r inlier_dist %r mirror %d)" % (
            str(e.args[0])[:60] if e.args else "?", len(case["source"]), len(case["truths"]), len(case["bases"]),
            case["len_tol"], case["inlier_dist"], case["mirror"]))


def make_register_sim(rng):
    sc = register_scene(rng)
    k = float(rng.uniform(0.4, 4.0))
    sc["source"] = np.ascontiguousarray(sc["source"] / k)
    Lu, Lv = pair_lengths(sc)
    with np.errstate(all="ignore"):
        ratio = Lv[None, :, :] / Lu[:, None, None]
        ok = (Lv > 0.0) & (Lv < np.inf)
        ratio = np.sort(ratio[:, ok][(Lu > 0.0) & (Lu < np.inf)].ravel())
    ratio = ratio[np.isfinite(ratio) & (ratio > 0.0)]
    pos = int(np.searchsorted(ratio, k))
    lo = max(0, pos - int(rng.integers(1, HYP_MAX // 2)))
    hi = min(len(ratio) - 1, pos + int(rng.integers(0, HYP_MAX // 2)))
    u = float(rng.choice([0.003, 0.01, 0.03]))
    # the range holds at most HYP_MAX ratios: a drawn bound is pulled in to the ratio at that rank
    smin, mode, variant = threshold(rng, lambda: float(ratio[lo]) if len(ratio) else None,
                                    lambda: max(k * (1.0 - u), float(ratio[lo])) if len(ratio) else k * (1.0 - u))
    smax, mode2, variant2 = threshold(rng, lambda: float(ratio[hi]) if len(ratio) else None,
                                      lambda: min(k * (1.0 + u), float(ratio[hi])) if len(ratio) else k * (1.0 + u))
    if mode != "own":
        mode, variant = mode2, variant2
    sc.update(mode=mode, variant=variant)

    def run(inlier):
        return RS.register(sc["source"], sc["truths"], sc["bases"], smin, smax, inlier, sc["mirror"],
                           sc["max_landmarks"])
    inlier, inl_mode, inl_variant = inlier_threshold(rng, sc, run)
    return register_case("register_sim", sc, dict(scale_min=smin, scale_max=smax, inlier_dist=inlier), run,
                         inlier_mode=inl_mode, inlier_variant=inl_variant, scale=k)


def check_register_sim(ctx, case):
    g = refused(case, lambda: ctx.register_sim(case["source"], case["truths"], case["bases"], case["scale_min"],
                                               case["scale_max"], case["inlier_dist"], case["mirror"],
                                               case["max_landmarks"]))
    if g is None:
        return
    try:
        RS.same(g, case["ref"])
    except AssertionError as e:
        fail(case, "%s differs from the restatement (ns %d nt %d B %d scale [%r, %r] inlier_dist %r mirror %d)" % (
            str(e.args[0])[:60] if e.args else "?", len(case["source"]), len(case["truths"]), len(case["bases"]),
            case["scale_min"], case["scale_max"], case["inlier_dist"], case["mirror"]))


# ---- assign_truths ---------------------------------------------------------------------------------------------------
def make_assign_truths(rng):
    fr = frame_of(rng, ("asis", "shift", "scale", "outliers"))
    T = log_int(rng, 1, 600)
    truths = base_cloud(rng, T, 2, unquantised=fr["transform"] == "shift")
    dup = int(rng.integers(0, max(1, T // 4) + 1))
    if dup:
        truths[rng.integers(0, T, dup)] = truths[rng.integers(0, T, dup)]      # duplicates: the LAST one wins
    bulk = extent_of(truths)
    truths = np.ascontiguousarray(apply_frame(rng, fr, truths))
    ids = rng.integers(0, 50, T).astype(np.int32)                              # 0: a truth that counts as none
    n = log_int(rng, 1, N_MAX)
    sigma = bulk * fr["unit"] * float(rng.choice([1e-4, 1e-3, 1e-2]))
    fin = truths[np.isfinite(truths).all(1)]
    lo, hi = (fin.min(0), fin.max(0)) if len(fin) else (np.zeros(2), np.ones(2))
    kind = rng.random(n)
    motor = truths[rng.integers(0, T, n)] + rng.normal(0.0, sigma, (n, 2))
    box = kind > 0.6
    motor[box] = rng.uniform(lo, hi, (int(box.sum()), 2))
    out = kind > 0.95                                                          # outside the truths' box
    motor[out] = hi + (hi - lo + sigma) * 10.0 ** rng.uniform(-3, 2, (int(out.sum()), 2))
    if rng.random() < 0.1 and n > 3:
        motor[int(rng.integers(n)), int(rng.integers(2))] = float(rng.choice([np.nan, np.inf, -np.inf]))
    motor = np.ascontiguousarray(motor)
    with np.errstate(all="ignore"):
        ax = truths[None, :, 0] - motor[:, None, 0]
        ay = truths[None, :, 1] - motor[:, None, 1]
        D = np.sqrt(ax * ax + ay * ay)
    radius, mode, variant = threshold(rng, lambda: small_distance(rng, D, 4),
                                      lambda: sigma * rng.choice([0.0, 1.0, 3.0, 10.0, 100.0]))
    fr.update(mode=mode, variant=variant)
    want_ids, want_out = O.assign_truths(motor, truths, ids, radius)
    finite = int(min(np.isfinite(motor).all(1).sum(), max(2, np.isfinite(truths).all(1).sum())))
    return case_of("assign_truths", fr, motor=motor, truths=truths, ids=ids, radius=radius, want_ids=want_ids,
                   want_out=int(want_out), finite_rows=finite, assigned=int((want_ids != 0).sum()))


def check_assign_truths(ctx, case):
    g = refused(case, lambda: ctx.assign_truths(case["motor"], case["truths"], case["ids"], case["radius"]))
    if g is None:
        return
    what = "(n %d T %d radius %r)" % (len(case["motor"]), len(case["truths"]), case["radius"])
    if not np.array_equal(g[0], case["want_ids"]):
        fail(case, "ids differ from the oracle at %s %s" % (np.flatnonzero(g[0] != case["want_ids"])[:5].tolist(), what))
    if g[1] != case["want_out"]:
        fail(case, "%d outliers, the oracle has %d %s" % (g[1], case["want_out"], what))


# ---- the sweep -------------------------------------------------------------------------------------------------------
MAKE = {"kdist": make_kdist, "eps_tree": make_eps_tree, "gdbscan": make_gdbscan, "match_unique": make_match_unique,
        "register_pairs": make_register_pairs, "register_sim": make_register_sim, "assign_truths": make_assign_truths}
CHECK = {"kdist": check_kdist, "eps_tree": check_eps_tree, "gdbscan": check_gdbscan,
         "match_unique": check_match_unique, "register_pairs": check_register_pairs,
         "register_sim": check_register_sim, "assign_truths": check_assign_truths}


def case_list(family, count, seed):
    """The case list of a family: `count` cases from a stream of (seed, family) alone."""
    rng = np.random.default_rng([seed, FAMILIES.index(family)])
    for i in range(count):
        case = MAKE[family](rng)
        case.update(index=i, seed=seed)
        yield case


def run(cases=24, seed=1, families=None, quiet=False, device=0):
    """One sweep: `cases` cases of every family in `families` (all of them by default; the register families
    run half as many) from `seed`.  Returns the number of compared cases per family; raises Mismatch on the first
    disagreement."""
    global ctx
    own = ctx is None
    if own:
        ctx = N.Context(device)
    QUIET[0] = quiet
    done.clear()
    spent.clear()
    try:
        for fam in FAMILIES:
            if families is not None and fam not in families:
                continue
            done[fam] = 0
            spent[fam] = [0.0, 0.0]
            count = max(1, cases // 2) if fam in HALF else cases
            t0 = time.perf_counter()
            for case in case_list(fam, count, seed):
                t1 = time.perf_counter()
                CHECK[fam](ctx, case)
                done[fam] += 1
                spent[fam][0] += t1 - t0
                t0 = time.perf_counter()
                spent[fam][1] += t0 - t1
            say("%s: %d cases agree (seed %d; %.2f s references, %.2f s device and comparison)" % (
                fam, done[fam], seed, spent[fam][0], spent[fam][1]), flush=True)
    finally:
        if own:
            ctx.close()
            ctx = None
    print("OK: " + ", ".join("%d %s" % (v, k) for k, v in done.items()) + " cases equal to their restatement (seed %d)"
          % seed, flush=True)
    return dict(done)


if __name__ == "__main__":
    try:
        run(int(sys.argv[1]) if len(sys.argv) > 1 else 24, int(sys.argv[2]) if len(sys.argv) > 2 else 1)
    except Mismatch:
        sys.exit(1)
