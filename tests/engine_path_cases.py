"""The case table of tests/test_engine_paths.py (CPU) and tests/test_engine_paths_gpu.py: one deterministic cloud per
path of the DBSCAN engine (csrc/dbscan.hip), at the smallest shape that reaches the path.  Importable without a GPU.

The engine does not compute one way: its host driver (run_dbscan and the stage_* functions) picks the kernel sequence
from the metric's dimension, min_pts, the isClassed input, n against the number of grid cells, and a few early outs;
k_core_lds forks again inside.  A case is a cloud built so that ONE of those forks goes a known way for a structural
reason -- stated in the builder's docstring -- plus what the library's own trace (VCP_TRACE, csrc/vcp_ctx.hpp) must then
show: the launch sites that appear, those that must not, and the values on the `vcp-trace dbscan` line.

    case.build()   -> dict(coords, eps, min_pts, metric[, cf_in, in_classed, labels])     (kind "engine")
                      dict(motor, eps, min_pts, pts_in_cell)                               (kind "blocks")
                      dict(coords, eps, min_pts, metric, cuts)                             (kind "slabs")
    case.params    what the driver's choice rests on (gd, lists, regime, ...): sites(**params) is the launch set
    case.want      {key: value or predicate} on the `vcp-trace dbscan` line (default switches)
    case.needs     which of core / border / noise points the oracle's result must contain for the case to mean anything
    case.claim     optional check(inp, neighbour counts, oracle result) of what the docstring promises

Every coordinate lies on the 2^-10 lattice: differences, L1 sums and sums of squares are exact in binary64, so a pair at
the threshold is a tie in every evaluation order, and the oracle's answer is the only right one.  eps is 1 wherever the
case does not say otherwise, so a grid cell is the unit square (a hair more) and cell k of an axis is [k, k + 1).
"""
import numpy as np

L1_2D, L2_2D, L2_3D = 0, 1, 2
METRICS = (("l1", L1_2D), ("l2", L2_2D), ("l3", L2_3D))
Q = 1024.0

# every `VCP_LAUNCH(ctx, <site>, ...` of csrc/dbscan.hip, as the trace prints it (test_engine_paths.py holds this list to
# the source: a new launch site fails there until a case expects it)
CORE_LDS, CORE_GLOBAL = "(k_core_lds<GD, METRIC, GROUPED>)", "(k_core<GD, METRIC, GROUPED>)"
UNION_INIT = "(k_union_init<GD, METRIC, GROUPED>)"
UNION_DENSE, UNION_PRE = "(k_union<GD, METRIC, GROUPED, true, true>)", "(k_union<GD, METRIC, GROUPED, true>)"
UNION_PLAIN = "(k_union<GD, METRIC, GROUPED, false>)"
BORDER, BORDER_SLAB, BORDER_LIST = "(k_border<GD, METRIC, GROUPED>)", "(k_border<GD, METRIC, false>)", "k_border_list<GROUPED>"
OUTPUT = "(k_output<GROUPED>)"
SITES = frozenset([
    "k_unclassed_flag", "k_all_pairs", "k_degenerate", CORE_LDS, CORE_GLOBAL, "k_wl_fill", "k_union_init_list",
    "k_flatten0<2>", "k_flatten0<1>", "k_flatten0<0>", UNION_INIT, "k_chunkroot", UNION_DENSE, UNION_PRE, UNION_PLAIN,
    "k_flatten<true>", "k_flatten<false>", "k_slab_count", "k_slab_fill", "k_slab_out", "k_seedflag", "k_seed_popc",
    "k_rootk", "k_labk_rest", BORDER_LIST, BORDER, OUTPUT, "k_lonely_seeds<GD>", "k_group_stats", "k_slab_rootk",
    BORDER_SLAB, "k_slab_output"])
# which way a call goes on n against the cell count: n < ncells | ncells <= n <= 16 ncells | n > 16 ncells
REGIMES = ("lt", "ge", "dense")


def sites(gd, lists, regime, in_classed=False, lonely=False, grouped=False, slab=False, early=None, core_global=False,
          join_all=None):
    """The launch sites of dbscan.hip one engine call goes through: the host driver's choices, written down once more
    from its stage functions.  lists: neighbour lists are recorded (2 <= min_pts <= 16, no isClassed input, not staged,
    no VCP_NO_LISTS); regime: see REGIMES; early: "all_pairs" / "degenerate" / None; core_global, join_all: the switches
    VCP_CORE_GLOBAL and VCP_JOIN_ALL."""
    if early == "all_pairs":
        return frozenset(["k_all_pairs"] + (["k_unclassed_flag"] if in_classed else []))
    if early == "degenerate":
        return frozenset(["k_unclassed_flag", "k_degenerate"])
    s = {CORE_LDS if gd == 2 and not (grouped and core_global) else CORE_GLOBAL, "k_wl_fill"}
    if lists:
        every = (regime != "lt") if join_all is None else bool(join_all)
        s |= {"k_union_init_list", "k_flatten0<2>" if every else "k_flatten0<1>", "k_flatten0<0>"}
    elif gd == 2:
        s |= {UNION_INIT, "k_flatten0<0>"}
    pre = gd == 2 or lists
    if pre and regime == "dense":
        s |= {"k_chunkroot", UNION_DENSE}
    else:
        s.add(UNION_PRE if pre else UNION_PLAIN)
    s.add("k_flatten<false>" if regime == "lt" else "k_flatten<true>")
    if slab:
        return frozenset(s | {"k_slab_count", "k_slab_fill", "k_slab_out", "k_slab_rootk", "k_labk_rest", BORDER_SLAB,
                              "k_slab_output"})
    s |= {"k_seedflag", "k_seed_popc", "k_rootk", "k_labk_rest", BORDER_LIST if lists else BORDER}
    if grouped:
        s |= {OUTPUT, "k_group_stats"}
    if lonely:
        s.add("k_lonely_seeds<GD>")
    return frozenset(s)


# sites that depend on the regime of a call: left open (neither demanded nor forbidden) where one case makes several
# engine calls whose grids differ (the two ranks of a staged call, the shares of a grouped one)
BY_REGIME = frozenset(["k_flatten0<2>", "k_flatten0<1>", "k_chunkroot", UNION_DENSE, UNION_PRE, UNION_PLAIN,
                       "k_flatten<true>", "k_flatten<false>"])


def lists_on(min_pts, in_classed=False, slab=False):
    return 2 <= min_pts <= 16 and not in_classed and not slab


class Case:
    def __init__(self, name, build, params, want=None, needs=(), claim=None, kind="engine", open_sites=frozenset()):
        self.name, self.build, self.params, self.kind = name, build, dict(params), kind
        self.want, self.needs, self.claim, self.open_sites = dict(want or {}), tuple(needs), claim, frozenset(open_sites)
        self.__doc__ = build.__doc__

    def expect(self, **switches):
        """(must, must_not) among SITES, under the given switch overrides of `sites`."""
        p = dict(self.params)
        p.update(switches)
        must = sites(**p) - self.open_sites
        return must, SITES - must - self.open_sites


def dim_of(metric):
    return 3 if metric == L2_3D else 2


def q(a):
    return np.round(np.asarray(a, np.float64) * Q) / Q


def lattice_box(rng, n, lo, hi, step=1.0 / 64):
    """n DISTINCT lattice points (multiples of `step`) of the box [lo, hi] (per axis)."""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    k0, k1 = np.ceil(lo / step - 1e-9).astype(np.int64), np.floor(hi / step + 1e-9).astype(np.int64)
    span = k1 - k0 + 1
    total = int(np.prod(span))
    assert total >= n, (total, n)
    flat = rng.choice(total, n, replace=False)
    idx = np.stack(np.unravel_index(flat, span), axis=1)
    return (idx + k0) * step


def lift(c2, metric, z=0.0):
    """2-D coordinates in the metric's dimension (3-D: the plane z)."""
    c2 = np.asarray(c2, np.float64).reshape(-1, 2)
    if metric != L2_3D:
        return c2
    return np.concatenate([c2, np.full((len(c2), 1), z)], axis=1)


def neighbour_counts(coords, eps, metric):
    """Points within eps of each point, itself included (a non-finite point has none): the reference's predicate in
    binary64, all pairs."""
    c = np.asarray(coords, np.float64)[:, :dim_of(metric)]
    with np.errstate(invalid="ignore"):
        d = c[:, None, :] - c[None, :, :]
        v = np.abs(d).sum(axis=2) if metric == L1_2D else np.sqrt((d * d).sum(axis=2))
        return (v <= eps).sum(axis=1)


# ---- density regimes -----------------------------------------------------------------------------------------------------
REGIME_EXTENT = {2: {"lt": 39.5, "ge": 9.5, "dense": 4.5}, 3: {"lt": 11.5, "ge": 4.5, "dense": 3.5}}


def unit_cloud(dim, n=1200, seed=101):
    """The unit-cube shape all three extents stretch: four Gaussian clumps of 250 points (sigma 0.04) round four corners of
    [0.2, 0.8]^dim and 200 uniform points; the first two points are the cube's corners (the bounding box)."""
    rng = np.random.default_rng(seed)
    corners = np.array([[0.2, 0.2, 0.2], [0.8, 0.2, 0.8], [0.2, 0.8, 0.8], [0.8, 0.8, 0.2]])[:, :dim]
    parts = [corners[k] + rng.normal(0.0, 0.04, (250, dim)) for k in range(4)]
    parts.append(rng.random((n - 1000, dim)))
    u = np.clip(np.concatenate(parts), 0.0, 1.0)
    u = u[rng.permutation(n)]
    u[0], u[1] = 0.0, 1.0
    return u


def regime_cloud(metric, regime):
    dim = dim_of(metric)
    return q(unit_cloud(dim) * REGIME_EXTENT[dim][regime])


def build_regime(metric, regime, min_pts):
    def build():
        """1200 points -- four clumps and a uniform background, the same unit shape every time -- stretched over an extent
        of 39.5 / 9.5 / 4.5 eps in 2-D (40^2 = 1600, 10^2 = 100, 5^2 = 25 cells) and 11.5 / 4.5 / 3.5 in 3-D (1728, 125, 64
        cells): n < ncells, ncells <= n <= 16 ncells and n > 16 ncells.  The flatten filter, the all-points join round, the
        length of a core point's list and the chunk summary of the union all hang on those two comparisons.  min_pts 5
        records lists, 17 does not."""
        return dict(coords=regime_cloud(metric, regime), eps=1.0, min_pts=min_pts, metric=metric)
    return build


def regime_want(regime):
    return {"lt": lambda d: d["n"] < d["ncells"],
            "ge": lambda d: d["ncells"] <= d["n"] <= 16 * d["ncells"],
            "dense": lambda d: d["n"] > 16 * d["ncells"]}[regime]


# ---- the exact flips -----------------------------------------------------------------------------------------------------
def build_flip(metric, which, min_pts):
    def build():
        """n == ncells against n == ncells - 1, and n == 16 ncells against 16 ncells + 1: the first n points of ONE
        sequence in a box of D - 0.5 eps per axis, D = 8 (2-D) or 4 (3-D) for the first pair -- 64 cells either way -- and
        D = 3 (9 cells, n = 144 / 145) or 2 (8 cells, n = 128 / 129) for the second.  Points 0 and 1 are the box's corners,
        so both calls of a pair see the same grid; 40 % of the points fall into a patch of 2 eps per axis so that core,
        border and noise points all occur.  The trace's own n and ncells say on which side each call fell."""
        dim = dim_of(metric)
        D = ((8, 4) if which in ("eq", "below") else (3, 2))[dim - 2]
        ncells = D ** dim
        n = {"eq": ncells, "below": ncells - 1, "x16": 16 * ncells, "x16p1": 16 * ncells + 1}[which]
        rng = np.random.default_rng(7 + dim)
        m = 16 * ncells + 1
        c = rng.random((m, dim)) * (D - 0.5)
        patch = rng.random(m) < 0.4
        c[patch] = 0.25 + rng.random((int(patch.sum()), dim)) * min(2.0, D - 1.0)
        c[0], c[1] = 0.0, D - 0.5
        return dict(coords=q(c[:n]), eps=1.0, min_pts=min_pts, metric=metric)
    return build


# ---- min_pts edges on clumps of 15, 16 and 17 ----------------------------------------------------------------------------
CLUMP_FAR = {2: {"lt": 13.5, "ge": 5.5, "dense": None}, 3: {"lt": 5.5, "ge": 2.5, "dense": None}}
CLUMP_SIZES = (15, 16, 17, 100)
CLUMP_SPAN = {2: 2.65, 3: 1.65}  # low corner of the far boxes: three cells per axis in 2-D, two in 3-D


def clump_cloud(metric, regime):
    dim = dim_of(metric)
    rng = np.random.default_rng(31 + dim)
    # corners that differ from each other in two axes in 3-D: a straggler next to one box along x or y is far from the rest
    corners = np.array([[0, 0, 0], [1, 1, 0], [0, 1, 1], [1, 0, 1]], np.float64)[:, :dim] * CLUMP_SPAN[dim]
    parts = [corners[k] + lattice_box(rng, m, [0.0] * dim, [0.25] * dim) for k, m in enumerate(CLUMP_SIZES)]
    # stragglers 1.1 from a box's low face (towards the middle of the cloud): within eps of the box's far half only
    for k, axis in ((1, 0), (1, 1), (2, 0)):
        s = corners[k] + 0.125
        s[axis] = corners[k][axis] + (1.125 if corners[k][axis] == 0.0 else -0.875)
        parts.append(s[None, :])
    far = CLUMP_FAR[dim][regime]
    if far is not None:
        parts.append(np.full((1, dim), far))
    c = np.concatenate(parts)
    return q(c), rng.permutation(len(c))


def build_minpts(metric, regime, min_pts):
    def build():
        """Clumps of exactly 15, 16 and 17 points, each inside a box of 0.25 eps per axis (so mutually neighbouring) at
        corners of the cloud more than eps apart, a ballast clump of 100 at a fourth, and three stragglers 1.1 eps from the
        low face of the 16- and the 17-box, which neighbour the far part of their box and nothing else.  At min_pts 16 (NB =
        15: the count fills the four bits of the flag byte) the points of the 16-clump out of a straggler's reach are core on
        exactly 16 with a full list of 15, the 15-clump sits one short with 14 entries each and is noise, the stragglers are
        border points; 17 switches the lists off, 2 gives NB = 1, -1 / 0 / 1 make everybody core.  The regime comes from ONE
        far point: none (9 cells in 2-D, 8 in 3-D: n = 151 > 16 ncells), at 5.5 / 2.5 (36 / 27 cells), at 13.5 / 5.5 (196 /
        216 cells > n = 152).  3-D counts through k_core and its dynamic LDS."""
        c, perm = clump_cloud(metric, regime)
        return dict(coords=c[perm], eps=1.0, min_pts=min_pts, metric=metric)
    return build


def claim_minpts16(inp, cnt, o):
    core = o["is_key"].astype(bool)
    assert (core & (cnt == 16)).any(), "no core point with a full 15-entry list"
    assert (~core & (cnt == 15)).any(), "no point one short of min_pts"
    assert (cnt[core] > 16).any(), "no core point that leaves the count early"
    assert (cnt == 15).sum() >= 15 and (o["labels"][cnt == 15] == 0).all(), "the 15-clump is noise"


# ---- isClassed on entry --------------------------------------------------------------------------------------------------
def classed_state(n, seed):
    rng = np.random.default_rng(seed)
    cls = (rng.random(n) < 0.3).astype(np.uint8)
    lab = np.where(cls != 0, 1 + np.arange(n) % 3, 0).astype(np.int32)
    return cls, lab


def build_classed(metric, regime):
    def build():
        """The regime cloud with three points in ten classed on entry under ids 1..3 (cf_in = 3): no lists, so the border
        rule searches (k_border); the 2-D union builds its forest by search (k_union_init), the 3-D one has none
        (k_union<..., false>).  Classed points inside the clumps are core: they do not expand and take the largest adjacent
        cluster like a border point."""
        c = regime_cloud(metric, regime)
        cls, lab = classed_state(len(c), 77)
        return dict(coords=c, eps=1.0, min_pts=5, metric=metric, cf_in=3, in_classed=cls, labels=lab)
    return build


def claim_classed_core(inp, cnt, o):
    assert ((inp["in_classed"] != 0) & (cnt >= inp["min_pts"])).any(), "no classed core point"


def build_classed_block(metric):
    def build():
        """One grid row of three cells (y extent 0.9 eps): 200 classed points in cell 0, 120 unclassed in cell 1, 40 in
        cell 2; n = 360 > 16 * 3.  Cell 0 comes first in cell order, so positions 0..191 are three aligned chunks of 64
        without an expanding point (chunkroot == NONE), wholly inside the row range [0, own position) of every point of
        cell 1: the dense union skips them with one load each."""
        rng = np.random.default_rng(91)
        a = lattice_box(rng, 200, [0.0, 0.0], [0.875, 0.875])
        a[0] = 0.0
        b = lattice_box(rng, 120, [1.125, 0.0], [1.875, 0.875])
        c = lattice_box(rng, 40, [2.125, 0.0], [2.875, 0.875])
        c[0] = (2.875, 0.875)
        pts = q(np.concatenate([a, b, c]))
        cls = np.zeros(360, np.uint8)
        cls[:200] = 1
        lab = cls.astype(np.int32)
        perm = rng.permutation(360)
        return dict(coords=lift(pts, metric)[perm], eps=1.0, min_pts=5, metric=metric, cf_in=1, in_classed=cls[perm],
                    labels=lab[perm])
    return build


# ---- the dense union's three kinds of chunk ------------------------------------------------------------------------------
def build_dense_union(metric, min_pts):
    def build():
        """One grid row of five cells.  Cell 0: 130 points with a NaN x (a non-finite coordinate bins to cell 0 of its axis;
        such a point neighbours nobody) -- at least one aligned chunk of 64 positions with no expanding point.  Cell 1:
        clump A, 130 mutually neighbouring points -- a chunk that is one tree.  Cells 2 and 3: clumps L and R of 130, more
        than eps from A, whose ONLY pair within eps is (2.75, y0) - (3.75, y0), at exactly eps: their trees meet when the
        edge scan gets to that pair, so the chunk where L ends and R begins is mixed, and skipping it splits the cluster.
        n = 522 > 16 * 5.  min_pts 5 builds the forest from lists (also in 3-D), 20 by search (2-D; 3-D then has none)."""
        dim = dim_of(metric)
        rng = np.random.default_rng(55 + dim)
        hi = [0.25] * dim
        A = np.array([1.0625] + [0.0] * (dim - 1)) + lattice_box(rng, 130, [0.0] * dim, hi)
        L = np.array([2.5] + [0.0] * (dim - 1)) + lattice_box(rng, 130, [0.0] * dim, [0.25 - 1.0 / 64] + hi[1:])
        R = np.array([3.75] + [0.0] * (dim - 1)) + lattice_box(rng, 130, [1.0 / 64] + [0.0] * (dim - 1), hi)
        y0 = [0.125] * (dim - 1)
        L[0] = [2.75] + y0
        R[0] = [3.75] + y0
        nanx = lattice_box(rng, 130, [0.0] * dim, hi)
        nanx[:, 0] = np.nan
        ends = np.zeros((2, dim))
        ends[1, 0] = 4.0
        c = q(np.concatenate([ends, A, L, R])), nanx
        c = np.concatenate(c)
        return dict(coords=c[rng.permutation(len(c))], eps=1.0, min_pts=min_pts, metric=metric)
    return build


def claim_dense_union(inp, cnt, o):
    c = inp["coords"]
    lab = o["labels"]
    inL = (c[:, 0] >= 2.5) & (c[:, 0] <= 2.75)
    inR = (c[:, 0] >= 3.75) & (c[:, 0] <= 4.0) & (lab != 0)
    inA = (c[:, 0] >= 1.0) & (c[:, 0] <= 1.4)
    assert inL.sum() == 130 and inA.sum() == 130
    assert len(set(lab[inL])) == 1 and set(lab[inL]) == set(lab[inR]), "L and R are one cluster through their one edge"
    assert set(lab[inA]).isdisjoint(set(lab[inL])) and (lab[np.isnan(c[:, 0])] == 0).all()
    # the one edge: nobody else of L is within eps of anybody of R
    m = inp["metric"]
    both = np.concatenate([c[inL], c[inR]])[:, :dim_of(m)]
    d = both[:, None, :] - both[None, :, :]
    v = np.abs(d).sum(axis=2) if m == L1_2D else np.sqrt((d * d).sum(axis=2))
    nl = int(inL.sum())
    cross = v[:nl, nl:] <= inp["eps"]
    assert cross.sum() == 1 and v[:nl, nl:].min() == inp["eps"], "exactly one L-R pair, at exactly eps"


# ---- k_core_lds: the tile's capacity ---------------------------------------------------------------------------------------
TILE_MEDIAN = {L1_2D: 216, L2_2D: 257}


def build_tile(metric, extra, min_pts):
    def build():
        """Grid row 0 holds 200 points in cell 0, 56 in cell 1 and 256 (+ `extra`) in cell 2, nothing in cell 3; the only
        other point is far away at (9.5, 5.5).  Row 0 comes first in cell order, so the first workgroup is exactly cells 0
        and 1, and the candidate rows of its lanes unite to cells 0..2: 512 positions -- the tile's capacity, used to the
        last slot -- or 513 with extra = 1, where the workgroup takes the global-memory loop.  The second workgroup (cell
        2: 56 + 256 + extra candidates) uses the tile both times.  min_pts 5 makes everybody core through the hit masks;
        at the cloud's median count (216 in L1, 257 in L2) half of the points are core and the count has to be exact."""
        rng = np.random.default_rng(13)
        a = lattice_box(rng, 200, [0.0, 0.0], [0.875, 0.875])
        a[0] = 0.0
        b = lattice_box(rng, 56, [1.125, 0.0], [1.875, 0.875])
        c = lattice_box(rng, 256 + extra, [2.125, 0.0], [2.875, 0.875])
        pts = q(np.concatenate([a, b, c, [[9.5, 5.5]]]))
        return dict(coords=pts[rng.permutation(len(pts))], eps=1.0, min_pts=min_pts, metric=metric)
    return build


def claim_tile(inp, cnt, o):
    c = inp["coords"]
    row0 = c[:, 1] < 1.0
    per_cell = np.bincount(c[row0, 0].astype(np.int64), minlength=4)
    assert list(per_cell[:2]) == [200, 56] and per_cell[2] in (256, 257) and per_cell[3] == 0
    if inp["min_pts"] > 16:
        core = o["is_key"].mean()
        assert 0.2 < core < 0.8, "core share %.2f" % core


# ---- k_core_lds: hits beyond the masks of a lane below min_pts (rescan) ----------------------------------------------------
RESCAN_PROBE = (1.875, 0.5)


def build_rescan(metric, variant):
    def build():
        """The hit masks of k_core_lds cover a lane's first 32 candidates per row; a lane that stays below min_pts with a
        hit beyond them walks its rows again in binary64 (`rescan`).  The probe (1.875, 0.5) sits in cell 1 of grid row 0.
          own     cell 0 of its own row holds 41 points, all more than eps away (x <= 0.625): the probe itself is candidate 41
                  of the row and its two neighbours, (2.75, 0.5) and -- at exactly eps -- (2.875, 0.5) in cell 2, come later.
                  They belong to a chain of six that is core at min_pts 5; the probe counts 3 and is its border point.
          global  the same with 521 points in cell 0: the row is longer than the tile, so the workgroup counts in the
                  global-memory loop and the re-scan starts from there.
          above   cell 0 of the row ABOVE holds 40 far points and cell 2 of that row a clump of six, of which the probe
                  reaches one (L1) or four (L2): the probe is candidate 1 of its own row, the hits beyond the masks are in
                  another row.  min_pts 6.
        Without the re-scan the probe records no neighbour and comes out as noise."""
        rng = np.random.default_rng(3)
        chain = [(2.75, 0.5), (2.875, 0.5), (3.0, 0.5), (3.125, 0.5), (3.25, 0.5), (3.375, 0.5)]
        clump = [(2.125, 1.125), (2.125, 1.375), (2.375, 1.25), (2.5, 1.375), (2.375, 1.5), (2.5, 1.125)]
        if variant == "above":
            left = lattice_box(rng, 40, [0.0, 1.25], [0.625, 1.75])
            pts, mp = [[0.0, 0.0], RESCAN_PROBE] + clump, 6
        else:
            left = lattice_box(rng, 40 if variant == "own" else 520, [0.0, 0.25], [0.625, 0.75])
            pts, mp = [[0.0, 0.0], RESCAN_PROBE] + chain, 5
        c = q(np.concatenate([np.array(pts), left, [[9.5, 5.5]]]))
        return dict(coords=c[rng.permutation(len(c))], eps=1.0, min_pts=mp, metric=metric)
    return build


def claim_rescan(inp, cnt, o):
    c = inp["coords"]
    i = int(np.flatnonzero((c[:, 0] == RESCAN_PROBE[0]) & (c[:, 1] == RESCAN_PROBE[1]))[0])
    assert 1 < cnt[i] < inp["min_pts"], "the probe has a neighbour and stays below min_pts"
    assert o["labels"][i] != 0 and not o["is_key"][i], "the probe is a border point"
    far = c[:, 0] <= 0.625
    assert far.sum() >= 34  # the origin is one of them
    # everything in cell 0 of the row in question is out of the probe's reach, and its neighbours sit in cell 2
    d = c[:, :2] - np.array(RESCAN_PROBE)
    v = np.abs(d).sum(axis=1) if inp["metric"] == L1_2D else np.sqrt((d * d).sum(axis=1))
    near = v <= inp["eps"]
    assert not (near & far).any() and (c[near, 0] >= 1.875).all() and (c[near & (c[:, 0] > 1.875), 0] >= 2.125).all()
    assert o["labels"][i] == o["labels"][int(np.flatnonzero(near & (c[:, 0] > 2.0))[0])]


# ---- k_core_lds: the masked tail of a trip of four -------------------------------------------------------------------------
TAIL_MEDIAN = {L1_2D: 8, L2_2D: 10}


def build_tail(metric):
    def build():
        """A ladder two cells wide and twelve rows high: every lane's candidate row is a whole grid row, of 5, 6, 7, 9, 10
        or 11 points -- 1, 2 and 3 modulo 4 -- so the last trip of four reads one to three candidates past the row (the top
        row has 12, so that no trip reads past the last point of the cloud).
        In cell order those are the first points of the NEXT grid row: for the row below a lane's own, points of its own row,
        which really are within eps.  Counting them makes points core that are one to three short of min_pts (the cloud's
        median count: 8 in L1, 10 in L2)."""
        rng = np.random.default_rng(21)
        parts = []
        for row, m in enumerate([5, 6, 7, 9, 10, 11, 5, 6, 7, 9, 10, 12]):
            p = lattice_box(rng, m, [0.0, row + 0.125], [1.875, row + 0.875], step=1.0 / 16)
            parts.append(p)
        c = np.concatenate(parts)
        c[0], c[1] = (0.0, 0.0), (1.875, 0.5)
        c = q(c)
        return dict(coords=lift(c, metric)[rng.permutation(len(c))], eps=1.0, min_pts=TAIL_MEDIAN[metric], metric=metric)
    return build


def claim_tail(inp, cnt, o):
    c = inp["coords"]
    rows = np.bincount(c[:, 1].astype(np.int64))
    assert sorted(set(rows[:-1] % 4)) == [1, 2, 3] and rows[-1] % 4 == 0 and len(rows) == 12 and c[:, 0].max() < 2.0
    mp = inp["min_pts"]
    assert ((cnt >= mp - 3) & (cnt < mp)).sum() >= 10, "points one to three short of min_pts"


# ---- early outs ------------------------------------------------------------------------------------------------------------
TIE_BOX = {L1_2D: ((0.5, 0.5), 1.0), L2_2D: ((0.75, 1.0), 1.25), L2_3D: ((0.25, 0.5, 0.5), 0.75)}


def tie_cloud(metric, n=12):
    box, eps = TIE_BOX[metric]
    rng = np.random.default_rng(17)
    c = lattice_box(rng, n, [0.0625] * len(box), [b - 0.0625 for b in box], step=1.0 / 16)
    c[0], c[1] = 0.0, box
    return q(c), eps


def build_tie(metric, ulp_below, classed=False):
    def build():
        """Twelve points whose bounding box measures EXACTLY the threshold in the metric's distance form (L1: 0.5 + 0.5 = 1;
        L2: 0.75^2 + 1^2 = 1.25^2; 3-D: 0.25^2 + 0.5^2 + 0.5^2 = 0.75^2): box_measure == thr, every pair is within eps, the
        call ends in k_all_pairs and with min_pts 12 everybody is core.  With eps one ulp smaller the same cloud takes the
        grid path on a grid of ONE cell, and the two corner points, now eleven neighbours each, are border points."""
        c, eps = tie_cloud(metric)
        d = dict(coords=c, eps=float(np.nextafter(eps, 0.0)) if ulp_below else eps, min_pts=12, metric=metric)
        if classed:
            cls = np.zeros(12, np.uint8)
            cls[[2, 5]] = 1
            d.update(cf_in=4, in_classed=cls, labels=(cls * 2).astype(np.int32))
        return d
    return build


def claim_tie(inp, cnt, o):
    ulp = inp["eps"] not in (1.0, 1.25, 0.75)
    assert list(cnt[:2]) == ([11, 11] if ulp else [12, 12]) and (cnt[2:] == 12).all()


def small_cloud(metric, n, seed, nonfinite=False, dup=False):
    dim = dim_of(metric)
    rng = np.random.default_rng(seed)
    if dup:
        base = lattice_box(rng, n // 2, [0.0] * dim, [4.0] * dim, step=0.25)
        c = base[rng.integers(0, len(base), n)]
        c[0], c[1] = 0.0, 4.0
    else:
        c = rng.random((n, dim)) * 4.0
        c[: n // 2] = 1.0 + rng.random((n // 2, dim)) * 0.75
        c[0], c[1] = 0.0, 6.5  # seven cells per axis: n stays below the cell count
    c = q(c)
    if nonfinite:
        c[3, 0] = np.nan
        c[8, dim - 1] = np.inf
        c[11] = -np.inf
    return c


def build_eps(metric, eps, min_pts, nonfinite=False, classed=False):
    def build():
        """Forty points in a box of 6.5 per axis, half of them in a patch of 0.75.  eps = +inf ends in k_all_pairs (with a non-finite
        coordinate in the cloud: the grid path on a single cell of infinite edge); eps < 0 and eps = NaN end in
        k_degenerate, where nobody neighbours anybody, itself included, and min_pts <= 0 still makes everybody a cluster."""
        c = small_cloud(metric, 40, 5, nonfinite)
        d = dict(coords=c, eps=eps, min_pts=min_pts, metric=metric)
        if classed:
            cls, lab = classed_state(40, 6)
            d.update(cf_in=3, in_classed=cls, labels=lab)
        return d
    return build


def build_eps0(metric):
    def build():
        """eps = 0: only exact duplicates neighbour each other.  Sixty draws from twenty lattice points; the cell edge falls
        back to range / 2^20 and the grid is coarsened down to the cell budget."""
        return dict(coords=small_cloud(metric, 60, 8, dup=True), eps=0.0, min_pts=3, metric=metric)
    return build


def build_lonely(metric, min_pts):
    def build():
        """min_pts <= 0 with three points that have a NaN or infinite coordinate: each is a cluster of its own that is never
        marked classed -- the extra pass k_lonely_seeds."""
        return dict(coords=small_cloud(metric, 40, 9, nonfinite=True), eps=1.0, min_pts=min_pts, metric=metric)
    return build


# ---- work-list sizes -------------------------------------------------------------------------------------------------------
# building blocks at min_pts 3, eps 1 (offsets from the unit's corner; axis-parallel, so L1 and L2 agree):
TRI = [(0.0, 0.0), (0.5, 0.0), (0.0, 0.5)]                 # three core points
TRI_LEAF = TRI + [(-1.0, 0.0)]                             # ... and one border point (neighbours the first corner only)
STAR2 = [(0.0, 0.0), (1.0, 0.0), (-1.0, 0.0)]              # one core point, two border points
CHAIN4 = [(-1.0, 0.0), (0.0, 0.0), (1.0, 0.0), (2.0, 0.0)]  # two core points, two border points
PAIR = [(0.0, 0.0), (0.75, 0.0)]                           # two border candidates that end as noise
SOLO = [(0.0, 0.0)]
WORKLISTS = {  # name: (units, expanding points, border candidates)
    "e0": ([SOLO, SOLO, PAIR], 0, 2), "e1": ([STAR2], 1, 2), "e7": ([TRI, TRI, STAR2], 7, 2),
    "e8": ([TRI, TRI, CHAIN4], 8, 2), "e9": ([TRI, TRI, TRI], 9, 0),
    "b0": ([SOLO, SOLO], 0, 0), "b1": ([TRI_LEAF], 3, 1), "b7": ([TRI_LEAF, PAIR, PAIR, PAIR], 3, 7),
    "b8": ([PAIR] * 4, 0, 8), "b9": ([TRI_LEAF] + [PAIR] * 4, 3, 9)}


def build_worklist(metric, key):
    def build():
        """The union, flatten and border kernels cut their work list into eight bands (wl_fetch); with fewer entries than
        bands most bands are empty and the band bounds collide.  Units of known make (triangles of core points, stars and
        chains with border points, pairs below min_pts 3) five eps apart give exactly 0, 1, 7, 8 or 9 expanding points
        (e*) or border candidates (b*); the far point (2, 12) keeps n below the cell count."""
        units = WORKLISTS[key][0]
        pts = [(2.0 + 5.0 * k + x, 2.0 + y) for k, u in enumerate(units) for x, y in u] + [(0.0, 0.0), (2.0, 12.0)]
        return dict(coords=lift(q(pts), metric, z=0.0), eps=1.0, min_pts=3, metric=metric)
    return build


def claim_worklist(key):
    def claim(inp, cnt, o):
        _, nE, nB = WORKLISTS[key]
        assert int(o["is_key"].sum()) == nE == int((cnt >= 3).sum()), "expanding points"
        assert int(((cnt > 1) & (cnt < 3)).sum()) == nB, "border candidates"
    return claim


# ---- coarsened and trimmed grids; the cell budget --------------------------------------------------------------------------
def build_coarse(metric):
    def build():
        """1500 points (30 clumps of 40, 290 background) over 300 x 300 eps (3-D: 45^3): more eps-cells than the floor of the
        cell budget, 2^16, which is what n < 2048 points get -- the grid is coarsened.  Ten outliers at +-1e5 stretch the
        bounding box 600-fold: the robust range leaves them to the edge cells, so the cell edge stays within a few eps
        (untrimmed it would be hundreds)."""
        dim = dim_of(metric)
        ext = 300.0 if dim == 2 else 45.0
        rng = np.random.default_rng(41 + dim)
        cen = rng.random((30, dim)) * (ext - 4.0) + 2.0
        parts = [cen[k] + rng.normal(0.0, 0.5, (40, dim)) for k in range(30)]
        parts.append(rng.random((290, dim)) * ext)
        out = np.where(rng.random((10, dim)) < 0.5, -1.0, 1.0) * 1e5 + rng.random((10, dim))
        c = np.concatenate(parts + [out])
        return dict(coords=q(c)[rng.permutation(len(c))], eps=1.0, min_pts=5, metric=metric)
    return build


def build_budget():
    """2600 uniform points over 279.5 x 279.5 eps: 280^2 = 78400 cells, under the default budget of 32 cells per point
    (83200) and over the floor of 2^16 that VCP_CELL_BUDGET=1 leaves -- the switch coarsens this grid and no other of the
    table."""
    rng = np.random.default_rng(43)
    c = rng.random((2600, 2)) * 279.5
    c[:1300] = rng.random((1300, 2)) * 30.0 + 100.0
    c[0], c[1] = 0.0, 279.5
    return dict(coords=q(c), eps=1.0, min_pts=4, metric=L1_2D)


# ---- grouped and staged calls ----------------------------------------------------------------------------------------------
def build_grouped():
    """Context.dbscan_blocks on 3000 points, 1500 per block: blocks above 1024 points go to the grid engine as ONE grouped
    call (k_core_lds<..., GROUPED> with the candidates' group ids staged beside their coordinates, k_border_list<true>,
    k_output<true>, k_group_stats); VCP_BRUTE_MAX=0 sends the small blocks there too.  Against oracle.block_pipeline.
    (n = 3000: a block has to exceed the all-pairs kernel's 1024 points for the default path to reach the engine.)"""
    rng = np.random.default_rng(61)
    c = rng.random((3000, 2)) * 6.0
    c[:1800] = rng.random((1800, 2)) * 0.5 + rng.integers(0, 3, (1800, 2)) * 2.0
    return dict(motor=q(c), eps=0.125, min_pts=10, pts_in_cell=1500)


def build_slabs(metric):
    def build():
        """distributed.exact_slabs_local on two contexts, 1500 points sorted by x and cut in the middle: every rank makes a
        staged engine call (vcp_slab_begin: no lists, k_slab_count / _fill / _out after the flatten) on its slab plus halo,
        and finishes with vcp_slab_finish (k_slab_rootk, k_border<..., false>, k_slab_output)."""
        dim = dim_of(metric)
        rng = np.random.default_rng(71 + dim)
        ext = 12.0 if dim == 2 else 5.0
        c = rng.random((1500, dim)) * ext
        cen = rng.random((8, dim)) * (ext - 2.0) + 1.0
        c[:900] = cen[rng.integers(0, 8, 900)] + rng.normal(0.0, 0.3, (900, dim))
        c = q(c)
        c = c[np.argsort(c[:, 0], kind="stable")]
        return dict(coords=c, eps=0.25 if dim == 2 else 0.5, min_pts=5, metric=metric, cuts=[0, 750, 1500])
    return build


# ---- the table -------------------------------------------------------------------------------------------------------------
def _engine(name, build, metric, min_pts, regime, want=None, needs=(), claim=None, in_classed=False, lonely=False,
            early=None):
    w = {"gd": dim_of(metric), "metric": metric, "regime": regime_want(regime)} if early is None else {}
    w.update(want or {})
    params = dict(gd=dim_of(metric), lists=lists_on(min_pts, in_classed), regime=regime, in_classed=in_classed,
                  lonely=lonely, early=early)
    return Case(name, build, params, w, needs, claim)


def _table():
    t = []
    CBN = ("core", "border", "noise")
    for mn, m in METRICS:
        two_d = m != L2_3D
        for r in REGIMES:
            for mp in (5, 17):
                nb = mp - 1 if mp <= 16 else 0
                want = {"NB": nb, "core_cap": (min(nb, 4) if two_d and r == "lt" else nb), "dense": int(r == "dense" and (two_d or nb > 0)),
                        "join_all": int(nb > 0 and r != "lt"), "part_out": 1, "grouped": 0, "slab": 0}
                t.append(_engine("regime_%s_%s_mp%d" % (r, mn, mp), build_regime(m, r, mp), m, mp, r, want,
                                 CBN if r != "dense" else ("core",)))
        for which, mp, r in (("eq", 6, "ge"), ("below", 6, "lt"), ("x16", 16, "ge"), ("x16p1", 16, "dense")):
            nb = mp - 1
            want = {"eq": {"n": lambda d: d["n"] == d["ncells"]}, "below": {"n": lambda d: d["n"] == d["ncells"] - 1},
                    "x16": {"n": lambda d: d["n"] == 16 * d["ncells"]},
                    "x16p1": {"n": lambda d: d["n"] == 16 * d["ncells"] + 1}}[which]
            want.update(NB=nb, core_cap=min(nb, 4) if two_d and r == "lt" else nb, dense=int(r == "dense"))
            t.append(_engine("flip_%s_%s" % (which, mn), build_flip(m, which, mp), m, mp, r, want, ("core",)))
        for r in REGIMES:
            for mp in (-1, 0, 1, 2, 5, 16, 17):
                nb = mp - 1 if 2 <= mp <= 16 else 0
                t.append(_engine("minpts_%s_%s_mp%d" % (r, mn, mp), build_minpts(m, r, mp), m, mp, r, {"NB": nb},
                                 CBN if mp == 16 else ("core",), claim_minpts16 if mp == 16 else None))
            t.append(_engine("classed_%s_%s" % (r, mn), build_classed(m, r), m, 5, r, {"NB": 0, "in_classed": 1},
                             ("core", "border") if r != "dense" else ("core",), claim_classed_core, in_classed=True))
        for mp in (5, 20):
            t.append(_engine("dense_union_%s_mp%d" % (mn, mp), build_dense_union(m, mp), m, mp, "dense",
                             {"dense": int(two_d or mp == 5), "ncells": lambda d: d["ncells"] <= 6}, ("core", "noise"),
                             claim_dense_union))
        if two_d:
            t.append(_engine("classed_block_%s" % mn, build_classed_block(m), m, 5, "dense",
                             {"dense": 1, "ncells": 3, "in_classed": 1}, ("core",), in_classed=True))
            for extra in (0, 1):
                for mp in (5, TILE_MEDIAN[m]):
                    t.append(_engine("tile_%d_%s_mp%d" % (512 + extra, mn, mp), build_tile(m, extra, mp), m, mp, "ge",
                                     {"D": lambda d: d["D"][:2] == [10, 6]}, ("core",), claim_tile))
            for v in ("own", "global", "above"):
                t.append(_engine("rescan_%s_%s" % (v, mn), build_rescan(m, v), m, 6 if v == "above" else 5,
                                 "ge" if v == "global" else "lt", {"NB": 5 if v == "above" else 4},
                                 ("core", "border", "noise"), claim_rescan))
            t.append(_engine("tail_%s" % mn, build_tail(m), m, TAIL_MEDIAN[m], "ge",
                             {"D": lambda d: d["D"][:2] == [2, 12]}, ("core", "border"), claim_tail))
        # early outs
        t.append(_engine("tie_%s" % mn, build_tie(m, False), m, 12, "ge", None, ("core",), claim_tie, early="all_pairs"))
        t.append(_engine("tie_classed_%s" % mn, build_tie(m, False, True), m, 12, "ge", None, ("core",), claim_tie,
                         in_classed=True, early="all_pairs"))
        t.append(_engine("tie_ulp_one_cell_%s" % mn, build_tie(m, True), m, 12, "ge", {"ncells": 1, "NB": 11},
                         ("core", "border"), claim_tie))
        t.append(_engine("eps_inf_%s" % mn, build_eps(m, float("inf"), 5), m, 5, "ge", None, ("core",), early="all_pairs"))
        t.append(_engine("eps_inf_nonfinite_%s" % mn, build_eps(m, float("inf"), 5, nonfinite=True), m, 5, "dense",
                         {"ncells": 1}, ("core", "noise")))
        for en, e in (("neg", -1.0), ("nan", float("nan"))):
            t.append(_engine("eps_%s_%s_mp3" % (en, mn), build_eps(m, e, 3), m, 3, "ge", None, ("noise",), early="degenerate"))
            t.append(_engine("eps_%s_%s_mp0" % (en, mn), build_eps(m, e, 0, classed=True), m, 0, "ge", None, ("core",),
                             in_classed=True, early="degenerate"))
        t.append(_engine("eps0_dup_%s" % mn, build_eps0(m), m, 3, "lt", {"cellw": lambda d: d["cellw"] > 0.0},
                         ("core", "noise")))
        for mp in (0, -1):
            t.append(_engine("lonely_%s_mp%d" % (mn, mp), build_lonely(m, mp), m, mp, "lt", {"NB": 0}, ("core",),
                             lonely=True))
        for key in WORKLISTS:
            t.append(_engine("worklist_%s_%s" % (key, mn), build_worklist(m, key), m, 3, "lt", {"NB": 2},
                             claim=claim_worklist(key)))
        t.append(_engine("coarse_trimmed_%s" % mn, build_coarse(m), m, 5, "lt",
                         {"ncells": lambda d: d["ncells"] <= 65536, "cellw": lambda d: 1.2 < d["cellw"] < 20.0}, CBN))
        t.append(Case("slabs_%s" % mn, build_slabs(m),
                      dict(gd=dim_of(m), lists=False, regime="ge", in_classed=True, slab=True), {"slab": 1, "NB": 0},
                      ("core", "border", "noise"), kind="slabs", open_sites=BY_REGIME))
    t.append(_engine("budget_l1", build_budget, L1_2D, 4, "lt", {"cellw": lambda d: d["cellw"] < 1.01,
                                                                "ncells": lambda d: d["ncells"] > 65536}, CBN))
    t.append(Case("grouped_blocks", build_grouped, dict(gd=2, lists=True, regime="ge", grouped=True),
                  {"grouped": 1, "NB": 9, "part_out": 0}, kind="blocks", open_sites=BY_REGIME))
    names = [c.name for c in t]
    assert len(set(names)) == len(names)
    return t


CASES = _table()
BY_NAME = {c.name: c for c in CASES}


# ---- the trace -------------------------------------------------------------------------------------------------------------
def parse_trace_line(line):
    """`vcp-trace <what> ...` -> (what, payload): payload is the kernel for a launch, the bare word for the early outs
    (`dbscan all_pairs ...`), else a dict of the key=value fields (numbers parsed, D as a list of three)."""
    parts = line.split()
    assert parts[0] == "vcp-trace", line
    what = parts[1]
    if what == "launch":
        return what, " ".join(parts[2:])
    d = {}
    for f in parts[2:]:
        if "=" not in f:
            d.setdefault("_words", []).append(f)
            continue
        k, v = f.split("=", 1)
        if k == "D":
            d[k] = [int(x) for x in v.split(",")]
        else:
            try:
                d[k] = int(v)
            except ValueError:
                d[k] = float(v)
    return what, d
