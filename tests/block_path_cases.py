"""The case table of tests/test_block_paths.py (CPU) and tests/test_block_paths_gpu.py: one deterministic cloud per fork of
the block pipeline (csrc/blockpart.hip, csrc/blocks.hip), at the smallest shape that reaches the fork.  Importable without
a GPU.

Almost every fork of this pipeline is decided on the device, from the data: how many passes the radix select makes, whether
a block is its own bucket (fsh == 0, k_blk_starts) or shares one (k_blk_split, which tracks the range of d per block or does
not), which blocks are cut into sub-ranges of d and which runs end in the general kernel's list, which instance of the
all-pairs kernel a block takes, and whether the final order overflows its table of cluster ids and is repeated by library
sort.  The library prints what it chose (VCP_TRACE: `vcp-trace blocks plan / build / cluster / order`); this module says
what it must print:

    ref_partition(key_xy, pts_in_cell)   the partition restated in numpy: block_of, d, rows, cols, the block-major order by
                                         (block, d, index)
    model(inp, ...)                      the driver's choices, written down once more from the source as
                                         engine_path_cases.sites does for the grid engine: every field of the trace lines
    sites(M, ...)                        the launch sites of the two files one call goes through
    CASES                                the table; case.want holds the claim the case exists for, in terms of the model

Two kinds of case.  "position": min_pts = 1, small_max = 0, distinct points and eps below the smallest gap between two
points.  Every point is then a cluster of its own, nothing is demoted, and the pipeline returns labels[i] = 1 + (position of
i in the block-major list), 0 for the points in no block, and `order` = that list: labels, block_of and order of ONE public
call expose block ids, block starts and the order inside every block, and ref_partition reproduces them.  A wrong rank in one
sub-bucket of one block changes a label.  "clustered": a real eps and min_pts, for the forks of the cluster and finish stages.
"error": the call fails, in the device and in the oracle, with the same code.

Where a fork is a threshold, the two cases on its sides are built from ONE point sequence: every point draws its place in
the caller's list when it is generated, and the smaller case is the larger one without its last point(s).

Left open: `V * VTARGET * 8 < m`, the third reason for a large block to go to the general kernel whole.  V stops at
VMAX = 4096, so the condition needs a block of more than 4096 * 256 * 8 = 8.4 M points: no test of a few seconds reaches it.
(The launch sites of the two files that only the sharded stages reach -- SHARDED_ONLY -- belong to tests/test_shares_gpu.py.)
"""
import numpy as np

# the thresholds the model repeats; tests/test_block_paths.py holds every one to its definition in the source
CAND_CAP, MAXS, MAXF = 65536, 32768, 8192
VF, VMAX, SLICE, VTARGET = 512, 4096, 4096, 256
VCP_BIG_BLOCK, VCP_BRUTE_MAX, BRT, CS_CAP = 1024, 1024, 256, 512
PCH_MIN, PT = 8192, 1024
CONSTANTS = {"blockpart.hip": ("CAND_CAP", "MAXS", "MAXF", "VF", "VMAX", "SLICE", "VTARGET", "PCH_MIN", "PT"),
             "blocks.hip": ("BRT", "CS_CAP"), "blocks_state.hpp": ("VCP_BIG_BLOCK", "VCP_BRUTE_MAX")}

ERR_DEGENERATE = -3

# every `VCP_LAUNCH(ctx, <site>, ...` of blockpart.hip and blocks.hip, as the trace prints it
SORT_SMALL, SORT_LIST, SORT_BIG = "(k_blk_sort<false, false>)", "(k_blk_sort<false, true>)", "(k_blk_sort<true, true>)"
BRUTE_SMALL, BRUTE_MID = "k_block_brute<BRT>", "k_block_brute<BRUTE_CAP>"
STATS, STATS_BIG = "k_block_stats<1>", "k_block_stats<16>"
SELECT = frozenset(["k_sel_init", "k_sel_hist", "k_sel_pick", "k_sel_collect", "k_sel_final"])
# the sharded stages' own sites (vcp_blocks_plan_dev's cuts, the zeroing of an earlier share's last entry, the pair lists):
# several contexts, tests/test_shares_gpu.py
SHARDED_ONLY = frozenset(["k_sb_starts", "k_zero_one", "k_pairs", "k_scatter_pairs"])
SITES = frozenset(SELECT | SHARDED_ONLY | {
    "k_blk_hist", "k_transpose_u32", "k_blk_scatter", "k_blk_starts", "k_blk_split", SORT_SMALL, "k_big_count", "k_big_scan",
    "k_big_move", SORT_LIST, SORT_BIG, "k_zero_words", BRUTE_SMALL, BRUTE_MID, STATS, STATS_BIG, "k_block_order",
    "k_block_order_big", "k_cluster_sizes", "k_iota", "k_gather_u32", "k_keep", "k_newlab", "k_victims", "k_last_entry",
    "k_zero_flag", "k_compact", "k_final_labels"})


class PartitionError(Exception):
    def __init__(self, code):
        super().__init__("partition error %d" % code)
        self.code = code


# ---- the partition, restated -------------------------------------------------------------------------------------------
def _find_axis(v, vmin, vmax, cellw, cnt):
    """q with lo(q) < v <= hi(q), lo(q) = vmin + q * cellw, hi(q) = lo(q + 1), the last interval stretched to vmax; -1 where
    there is none.  The same expressions as find_axis (blockpart.hip) and the C# evaluate; the arithmetic guess only picks
    the window in which they are tried."""
    g = (v - vmin) / cellw
    q0 = np.where(np.isfinite(g), np.floor(g), 0.0).astype(np.int64)
    out = np.full(len(v), -1, np.int64)

    def attempt(q):
        ok = (q >= 0) & (q < cnt) & (out < 0)
        qq = np.clip(q, 0, cnt - 1).astype(np.float64)
        lo = vmin + qq * cellw
        hi = np.where(q == cnt - 1, vmax, vmin + (qq + 1.0) * cellw)
        hit = ok & (v > lo) & (v <= hi)
        out[hit] = q[hit]

    for off in (0, -1, 1, -2, 2):
        attempt(q0 + off)
    attempt(np.full(len(v), cnt - 1, np.int64))
    return out


def ref_partition(key_xy, pts_in_cell):
    """MainForm.getClusterFromMotor's partition on the coordinates key_xy [n, 2], in numpy: bounds, d = max(x - x_Min,
    y - y_Min), the `take` smallest (d, index) as block 0 and as the measure of the block size, rows and cols, and the
    (lo, hi] rectangle of every other point (rectangle 0 skipped).  -> dict(block_of, d, rows, cols, order, ...);
    order = the indices of the points that fell in a block, by (block, d, index)."""
    k = np.ascontiguousarray(key_xy, np.float64).reshape(-1, 2)
    n = len(k)
    x, y = k[:, 0], k[:, 1]
    x_Min, x_Max, y_Min, y_Max = x.min(), x.max(), y.min(), y.max()
    d = np.maximum(x - x_Min, y - y_Min) + 0.0
    take = min(int(pts_in_cell), n)
    by_d = np.lexsort((np.arange(n), d))
    first = by_d[:take]
    cell_x, cell_y = x[first].max() - x_Min, y[first].max() - y_Min
    with np.errstate(divide="ignore", invalid="ignore"):
        fr, fc = np.float64(y_Max - y_Min) / cell_y, np.float64(x_Max - x_Min) / cell_x
    if not (np.isfinite(fr) and np.isfinite(fc)):
        raise PartitionError(ERR_DEGENERATE)
    rows, cols = int(fr) + 1, int(fc) + 1
    q = _find_axis(x, x_Min, x_Max, cell_x, cols)
    p = _find_axis(y, y_Min, y_Max, cell_y, rows)
    index = p * cols + q
    block_of = np.where((p >= 0) & (q >= 0) & (index != 0), index, -1)
    block_of[first] = 0
    inside = np.flatnonzero(block_of >= 0)
    order = inside[np.lexsort((inside, d[inside], block_of[inside]))]
    return dict(block_of=block_of.astype(np.int32), d=d, rows=rows, cols=cols, order=order.astype(np.int64), take=take,
                d_T=d[first[-1]], idx_T=int(first[-1]), x_Min=x_Min, x_Max=x_Max, y_Min=y_Min, y_Max=y_Max, cell_x=cell_x,
                cell_y=cell_y, nblocks=rows * cols)


def position_labels(P, n):
    """what a "position" case returns as labels: 1 + the position in the block-major list, 0 for the points in no block"""
    lab = np.zeros(n, np.int32)
    lab[P["order"]] = 1 + np.arange(len(P["order"]), dtype=np.int32)
    return lab


# ---- the driver, modelled ----------------------------------------------------------------------------------------------
def select_passes(d, take):
    """Global passes of the radix select (vcp_blocks_plan's loop): twelve bits of the 96-bit string [bits of d | index]
    per pass, the bin that holds rank `take`, until that bin holds at most CAND_CAP keys."""
    k = np.ascontiguousarray(d, np.float64).view(np.uint64)
    idx = np.arange(len(k), dtype=np.uint64)
    alive = np.ones(len(k), bool)
    rank = take
    for p in range(8):
        sh = 84 - 12 * p  # position of the digit in the 96-bit string
        if sh >= 32:
            dig = (k >> np.uint64(sh - 32)) & np.uint64(0xFFF)
        elif sh == 24:
            dig = ((k & np.uint64(0xF)) << np.uint64(8)) | (idx >> np.uint64(24))
        else:
            dig = (idx >> np.uint64(sh)) & np.uint64(0xFFF)
        dig = dig.astype(np.int64)
        cum = np.cumsum(np.bincount(dig[alive], minlength=4096))
        b = int(np.searchsorted(cum, rank, side="left"))
        below = int(cum[b - 1]) if b else 0
        count = int(cum[b]) - below
        rank -= below
        alive &= dig == b
        if count <= CAND_CAP:
            return p + 1
    raise AssertionError("the selection does not end")


def _sub_ranges(m):
    V = 2
    while V < VMAX and V * VTARGET < m:
        V <<= 1
    return V


def _vmap(d, dmin, scale, V):
    """vmap of blockpart.hip: a subtraction, a product and a truncation in binary64"""
    v = (d - dmin) * scale
    return np.where(v >= float(V), V - 1, np.where(v > 0.0, np.floor(np.maximum(v, 0.0)), 0.0)).astype(np.int64)


def _clusters_of(pts, eps, min_pts):
    """clusters DBImproved finds in one block: components of its core points (L1 in the plane, `<= eps`)"""
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import connected_components
    near = (np.abs(pts[:, None, 0] - pts[None, :, 0]) + np.abs(pts[:, None, 1] - pts[None, :, 1])) <= eps
    core = near.sum(1) >= min_pts
    if not core.any():
        return 0
    return connected_components(csr_matrix(near[np.ix_(core, core)]), directed=False)[0]


def model(inp, brute_thr=VCP_BRUTE_MAX, order_sort=False):
    """What the trace of one call on `inp` must show: {"error": code} for a call that fails, else the fields of the
    `blocks plan`, `blocks build` and `blocks cluster` lines, `retry` (the final order is repeated by library sort), and
    what they rest on: the block sizes, the large blocks with their sub-ranges, the most cluster ids in a block."""
    motor = np.ascontiguousarray(inp["motor"], np.float64)
    key = np.ascontiguousarray(inp.get("key_xy", motor), np.float64)
    n = len(key)
    try:
        P = ref_partition(key, inp["pts_in_cell"])
    except PartitionError as e:
        return dict(error=e.code)
    nblocks = P["nblocks"]
    chunk = max((n + 255) // 256, PCH_MIN)
    chunk = (chunk + PT - 1) // PT * PT
    nb1, fsh = nblocks + 1, 0
    while ((nb1 + (1 << fsh) - 1) >> fsh) > MAXS:
        fsh += 1
    assert (1 << fsh) <= MAXF
    NS = (nb1 + (1 << fsh) - 1) >> fsh
    plan = dict(n=n, take=P["take"], passes=select_passes(P["d"], P["take"]), nblocks=nblocks, rows=P["rows"], cols=P["cols"],
                fsh=fsh, NS=NS, nchunk=(n + chunk - 1) // chunk, keyed=int("key_xy" in inp))
    # the large blocks
    bo, d = P["block_of"], P["d"]
    sizes = np.bincount(bo[bo >= 0], minlength=nblocks)
    tracked = (1 << fsh) <= VF
    nbinfo = nslice = nvirt = nfall = 0
    big = []
    for b in np.flatnonzero(sizes > VCP_BIG_BLOCK):
        m = int(sizes[b])
        db = d[bo == b]
        info = dict(b=int(b), m=m, V=None, direct=False, over=0)
        big.append(info)
        if fsh > 0 and not tracked:  # k_blk_split without the range of d: the general kernel takes the block whole
            info["direct"] = True
            nfall += 1
            continue
        if fsh > 0:  # the block's own range of d
            dmin, dmax = db.min(), db.max()
        elif b == 0:  # k_blk_starts: the range the block's rectangle allows; the first block: [0, d of its last point]
            dmin, dmax = 0.0, P["d_T"]
        else:
            p, q = divmod(int(b), P["cols"])
            lox = float(q) * P["cell_x"]
            hix = P["x_Max"] - P["x_Min"] if q == P["cols"] - 1 else float(q + 1) * P["cell_x"]
            loy = float(p) * P["cell_y"]
            hiy = P["y_Max"] - P["y_Min"] if p == P["rows"] - 1 else float(p + 1) * P["cell_y"]
            dmin, dmax = max(lox, loy), max(hix, hiy)
        V = _sub_ranges(m)
        with np.errstate(divide="ignore"):
            scale = np.float64(V) / np.float64(dmax - dmin)
        if not (dmax > dmin) or not (scale > 0.0) or not np.isfinite(scale) or V * VTARGET * 8 < m:
            info["direct"] = True
            nfall += 1
            continue
        fill = np.bincount(_vmap(db, dmin, scale, V), minlength=V)
        info.update(V=V, dmin=float(dmin), dmax=float(dmax), fill=fill, over=int((fill > VCP_BIG_BLOCK).sum()))
        nbinfo += 1
        nslice += (m + SLICE - 1) // SLICE
        nvirt += V
        nfall += info["over"]  # sub-ranges that came out too full: passed on by the LIST sort
    build = dict(S_lo=0, S_hi=NS, b_lo=0, b_hi=nblocks, m=len(P["order"]), nbig=len(big), nbinfo=nbinfo, nslice=nslice,
                 nvirt=nvirt, nfall=nfall)
    # the cluster stage's split of the blocks
    if brute_thr > 0:
        small = sizes <= brute_thr
        cluster = dict(pts_small=int(sizes[small].sum()), pts_big=int(sizes[~small].sum()),
                       any_mid=int((small & (sizes > BRT)).any()))
    else:
        cluster = dict(pts_small=0, pts_big=1, any_mid=0)
    # the most cluster ids in a block: the final order's table holds CS_CAP
    if inp["min_pts"] == 1 and inp["kind"] == "position":
        ids_max = int(sizes.max())
    else:
        ids_max = 0
        for b in np.flatnonzero(sizes > CS_CAP):  # (a block of up to CS_CAP points cannot overflow the table)
            ids_max = max(ids_max, _clusters_of(motor[bo == b], inp["eps"], inp["min_pts"]))
    return dict(error=0, P=P, plan=plan, build=build, cluster=cluster, sizes=sizes, big=big, tracked=tracked, ids_max=ids_max,
                retry=bool(ids_max > CS_CAP and not order_sort), by_sort=bool(order_sort))


def sites(M, staged=False):
    """The launch sites of blockpart.hip and blocks.hip one call goes through (vcp_blocks_plan, vcp_blocks_build,
    blocks_cluster, finish_local, finish_zero, finish_zcoords, blocks_finish), given the model M of the call; staged: the
    stages called one by one, with vcp_blocks_finish_local_dev before the finish.  The grid engine's own sites (dbscan.hip)
    belong to tests/engine_path_cases.py."""
    if M["error"]:
        return frozenset(SELECT)  # the zero extent shows when the selection has finished: nothing is partitioned
    s = set(SELECT) | {"k_blk_hist", "k_transpose_u32", "k_blk_scatter", "k_blk_starts" if M["plan"]["fsh"] == 0 else "k_blk_split",
                       SORT_SMALL, "k_big_count", "k_big_scan", "k_big_move", SORT_LIST, SORT_BIG}
    if M["cluster"]["pts_small"] > 0:
        s |= {"k_zero_words", BRUTE_SMALL}
        if M["cluster"]["any_mid"]:
            s.add(BRUTE_MID)
    s |= {STATS, "k_keep", "k_newlab", "k_victims", "k_zero_flag", "k_compact", "k_final_labels"}
    nbig = M["build"]["nbig"]
    if nbig:
        s.add(STATS_BIG)
    if not M["by_sort"]:
        s.add("k_block_order")
        if nbig:
            s.add("k_block_order_big")
    if M["by_sort"] or M["retry"]:
        s |= {"k_cluster_sizes", "k_iota", "k_gather_u32"}
    if staged:
        s.add("k_last_entry")
    return frozenset(s)


def order_lines(M, staged=False):
    """the `vcp-trace blocks order` lines of one call, in order: the first attempt, and the repeat when a block's ids
    overflow the table -- in the staged form once inside finish_local's loop and once more in the finish itself"""
    one = [{"by_sort": int(M["by_sort"])}] + ([{"by_sort": 1, "retry": 1}] if M["retry"] else [])
    return one + one if staged else one


# ---- clouds ------------------------------------------------------------------------------------------------------------
STEP = 2.0 ** -7          # the lattice of the position cases
EPS_POS = 2.0 ** -9       # ... and their eps: below the lattice step, so no two points are neighbours
FIRST3 = ((0.0, 0.0), (1.0, 0.5), (0.5, 1.0))  # a first block of three points and unit extent (pts_in_cell = 3)


class Cloud:
    """Points with the place each takes in the caller's list drawn when it is generated (a random key): dropping a point
    leaves everybody else's order alone, so the two sides of a threshold differ by the threshold only.

    The standard layout: the corner (0, 0) and two points at d = 1 make a first block of unit extent with pts_in_cell = 3,
    so block p * cols + q is the unit square (q, q + 1] x (p, p + 1] and every point outside (0, 1]^2 has d > 1; a point at
    (cols - 0.5, rows - 0.5) sets rows and cols."""

    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.pts, self.keys = [], []

    def add(self, pts, keep=None):
        pts = np.asarray(pts, np.float64).reshape(-1, 2)
        keys = self.rng.random(len(pts))  # (drawn for every point generated, kept or not)
        keep = len(pts) if keep is None else keep
        self.pts.append(pts[:keep])
        self.keys.append(keys[:keep])
        return self

    def cell(self, p, q, count, keep=None, k=None, step=STEP, at=(0, 0)):
        """`count` distinct lattice points of block (p, q): sites (q + i * step, p + j * step), at[0] < i <= at[0] + k, the
        same for j (k: sites per axis, the whole unit square by default); the first `keep` of them are used"""
        k = int(round(1.0 / step)) if k is None else k
        flat = self.rng.choice(k * k, count, replace=False)
        i, j = flat // k + 1 + at[0], flat % k + 1 + at[1]
        return self.add(np.stack([q + i * step, p + j * step], axis=1), keep)

    def one_d(self, p, q, count, step=2.0 ** -12):
        """`count` points of block (p, q), q > p, that share one d: x = q + 1 (the block's right edge), y distinct below it"""
        assert q > p and count <= int(round(1.0 / step))
        j = 1 + self.rng.choice(int(round(1.0 / step)), count, replace=False)
        return self.add(np.stack([np.full(count, q + 1.0), p + j * step], axis=1))

    def frame(self, cols, rows, first=FIRST3):
        return self.add(first).add([(cols - 0.5, rows - 0.5)])

    def points(self):
        pts, keys = np.concatenate(self.pts), np.concatenate(self.keys)
        return np.ascontiguousarray(pts[np.argsort(keys, kind="stable")])


def _position(motor, pts_in_cell=3, lattice=STEP, eps=EPS_POS, key_xy=None):
    inp = dict(kind="position", motor=motor, eps=eps, min_pts=1, pts_in_cell=pts_in_cell, small_max=0, lattice=lattice)
    if key_xy is not None:
        inp["key_xy"] = key_xy
    return inp


def _clustered(motor, eps, min_pts, pts_in_cell=3, small_max=3, lattice=2.0 ** -10):
    return dict(kind="clustered", motor=motor, eps=eps, min_pts=min_pts, pts_in_cell=pts_in_cell, small_max=small_max,
                lattice=lattice)


def _scatter(c, cols, rows, count, most=40, avoid=()):
    """`count` further blocks of a few points each: distinct blocks anywhere in the grid but block 0, the last row and
    column (the point that sets rows and cols stays the largest on both axes) and the blocks (p, q) of `avoid`, which the
    case fills itself"""
    taken = {0} | {p * (cols - 1) + q for p, q in avoid}
    for flat in c.rng.choice((rows - 1) * (cols - 1), count + len(taken), replace=False):
        if int(flat) in taken or count == 0:
            continue
        count -= 1
        c.cell(int(flat) // (cols - 1), int(flat) % (cols - 1), int(c.rng.integers(1, most)))
    return c


# -- select
def build_select_first_digit():
    """2000 points over 8 x 8 unit blocks.  The first digit of the select (sign and exponent of d) leaves the octave [1, 2)
    of the rank's key: far fewer than CAND_CAP keys, so one global pass and the single-workgroup end.  No block is large."""
    c = Cloud(1).frame(8, 8)
    _scatter(c, 8, 8, 47, most=70, avoid=[(6, 6)])
    rest = 2000 - sum(len(p) for p in c.pts)
    assert 0 < rest <= VCP_BIG_BLOCK
    c.cell(6, 6, rest)
    return _position(c.points())


def build_cand_cap(keys):
    def build():
        """The corner (0, 0) and `keys` distinct points whose d all lie in the octave [4, 8) (x in [4, 8), y in (0, 4.04]),
        pts_in_cell 50: the first digit's bin of rank 50 holds exactly `keys` keys.  65536 = CAND_CAP is still collected
        after one pass; 65537 needs a second digit.  Both are prefixes of one sequence of 66048 lattice points.  The blocks
        that result hold tens of thousands of points each: sub-ranges over several slices."""
        c = Cloud(2)
        i, j = np.meshgrid(np.arange(256), np.arange(258), indexing="ij")
        seq = np.stack([4.0 + i.ravel() / 64.0, (j.ravel() + 1) / 64.0], axis=1)
        c.add(seq[c.rng.permutation(len(seq))], keep=keys)
        c.add([(0.0, 0.0)])
        return _position(c.points(), pts_in_cell=50, lattice=2.0 ** -6)
    return build


def build_select_ties(pts_in_cell):
    def build():
        """The corner and 66000 distinct points with ONE d (x = 5, y distinct on the 2^-16 lattice, all below 5): every digit
        of d leaves all 66000 keys in the rank's bin, the digit that mixes the last bits of d with the top of the index
        too (the indices are below 2^24); the first index digit that differs (bits 12..23) cuts the bin to 4096 keys: seven
        global passes.  pts_in_cell 50: the index alone decides who is in the first block.  pts_in_cell 40000: the first
        block is a large block of one d beside the corner -- its range [0, d_T] is usable, every record but the corner
        lands in the last sub-range, which overflows into the general kernel's list."""
        c = Cloud(3)
        y = (1 + c.rng.permutation(66000)) * 2.0 ** -16
        c.add(np.stack([np.full(66000, 5.0), y], axis=1)).add([(0.0, 0.0)])
        return _position(c.points(), pts_in_cell=pts_in_cell, lattice=2.0 ** -16, eps=2.0 ** -18)
    return build


def build_take_tie():
    """pts_in_cell 4 on a cloud whose points 2, 3, 4 and 5 of the order by (d, index) all have d = 1: the index decides.
    The first block takes the corner and the three tied points of smallest index; the fourth, inside rectangle 0 but
    outside the take, falls in no block."""
    c = Cloud(4).frame(6, 6, first=FIRST3 + ((1.0, 0.25), (0.25, 1.0)))
    _scatter(c, 6, 6, 20)
    return _position(c.points(), pts_in_cell=4)


def claim_take_tie(inp, M):
    P, motor = M["P"], inp["motor"]
    tied = np.flatnonzero(P["d"] == 1.0)
    assert len(tied) == 4 and P["d_T"] == 1.0
    assert list(P["block_of"][tied]) == [0, 0, 0, -1], "the three tied points of smallest index are in, the fourth is out"
    assert (motor[tied[3]] <= 1.0).all()


def build_one_block(extra):
    def build():
        """pts_in_cell = n + `extra` on 300 points: take = n (clamped when pts_in_cell > n), the first block is the whole
        cloud and its extent the cloud's, so rows = cols = (int)1.0 + 1 = 2: four blocks, one of them populated."""
        c = Cloud(5).frame(8, 8)
        _scatter(c, 8, 8, 40)
        pts = c.points()[:300]
        assert len(pts) == 300
        return _position(pts, pts_in_cell=300 + extra)
    return build


def build_zero_extent():
    """pts_in_cell 1: the first block is the corner point alone, its extent zero, rows and cols undefined.  The device and
    the oracle both fail with VCP_ERR_DEGENERATE (-3), after the selection and before anything is partitioned."""
    c = Cloud(6).frame(6, 6)
    _scatter(c, 6, 6, 10)
    inp = _position(c.points(), pts_in_cell=1)
    inp["kind"] = "error"
    return inp


def build_pic1_two_minima():
    """pts_in_cell 1 where x_Min and y_Min come from two different points, (0, 5) and (5, 0): the first block is the one
    point of smallest d, (0.5, 0.25), and measures 0.5 x 0.25: cols = 13, rows = 25.  The two points that set the minima
    have x == x_Min or y == y_Min outside the first block: no rectangle (lo, hi] holds them."""
    c = Cloud(7)
    c.add([(0.0, 5.0), (5.0, 0.0), (0.5, 0.25), (6.0, 6.0)])
    for flat in c.rng.choice(25, 20, replace=False):  # distinct unit squares of [1, 6)^2, on the lattice, off the edges
        c.cell(1 + int(flat) // 5, 1 + int(flat) % 5, int(c.rng.integers(1, 30)), k=127)
    return _position(c.points(), pts_in_cell=1)


def claim_two_minima(inp, M):
    P = M["P"]
    edge = (inp["motor"][:, 0] == 0.0) | (inp["motor"][:, 1] == 0.0)
    assert edge.sum() == 2 and (P["block_of"][edge] == -1).all()


# -- bucket layout
def build_lds(cols, rows, big):
    def build():
        """`cols` x `rows` unit blocks, a few hundred points in scattered blocks and one block of 1500.  217 x 151 = 32767
        blocks and the points in no block are 32768 buckets: still one bucket per block (fsh = 0, k_blk_starts), with a
        histogram of 128 KB that needs the dynamic-LDS attribute.  128 x 256 = 32768 blocks are one bucket too many: the
        first split (fsh = 1, two blocks per super-bucket, k_blk_split, which tracks the range of d per block)."""
        c = Cloud(8).frame(cols, rows)
        _scatter(c, cols, rows, 60, avoid=[(rows // 2, cols // 3)])
        if big:
            c.cell(rows // 2, cols // 3, big)
        return _position(c.points())
    return build


def build_tracked_split():
    """256 x 128 blocks (fsh = 1, tracked) with a block of 1500 points of many d and a block of 1100 points of ONE d: the
    first gets a BigInfo with sub-ranges over its own min and max of d; the second has kmx == kmn and goes to the general
    kernel whole, without a BigInfo.  A small one-d block beside them is ordered by index in the LDS kernel."""
    c = Cloud(9).frame(256, 128)
    _scatter(c, 256, 128, 40, avoid=[(40, 70), (3, 90), (5, 17)])
    c.cell(40, 70, 1500).one_d(3, 90, 1100).one_d(5, 17, 300)
    return _position(c.points(), lattice=2.0 ** -12, eps=2.0 ** -14)


def build_untracked_split():
    """4097 x 4096 unit blocks: 16.8 M blocks in 16 k super-buckets of 2^10 blocks, more than the VF = 512 for which the
    split pass tracks the range of d.  About 3000 points, 1100 of them inside one unit block: a large block, listed, that
    goes to the general kernel whole (nbinfo = 0)."""
    c = Cloud(10).frame(4097, 4096)
    _scatter(c, 4097, 4096, 90, avoid=[(2000, 3000)])
    c.cell(2000, 3000, 1100)
    return _position(c.points())


def build_no_block():
    """Points on the minimum edges outside the first block, (0, 3.5) and (2.5, 0): x == x_Min or y == y_Min is in no
    (lo, hi] interval of its axis.  They fall in no block, ride along as block `nblocks`, end up behind the m others and
    keep label 0.  (take_tie has the other kind: a point inside rectangle 0 that the take does not reach.)"""
    c = Cloud(11).frame(6, 6)
    _scatter(c, 6, 6, 20)
    c.add([(0.0, 3.5), (2.5, 0.0)])
    return _position(c.points())


def claim_no_block(inp, M):
    assert M["build"]["m"] == len(inp["motor"]) - 2


# -- large blocks
def build_block_of(size, full):
    def build():
        """6 x 6 unit blocks, small blocks scattered, and one block of `size` points (the first `size` of a sequence of
        `full`).  1024 = VCP_BIG_BLOCK is still a small block for the LDS kernel (m / 2 = 512 sub-buckets, its most); 1025
        is cut into V = 8 sub-ranges of d in one slice.  4096 = SLICE fills one slice; 4097 starts a second, partial one."""
        c = Cloud(12).frame(6, 6)
        _scatter(c, 6, 6, 20, avoid=[(2, 3)])
        c.cell(2, 3, full, keep=size)
        return _position(c.points())
    return build


def build_first_block_large():
    """pts_in_cell 1499 with exactly 1499 points at d <= 1 (the corner, the two points at d = 1 and 1496 sites below 1 on
    both axes): the first block is a large block.  It is its own bucket (fsh = 0), so its V = 8 sub-ranges are laid over
    [0, d of its last point] = [0, 1]."""
    c = Cloud(13).frame(6, 6)
    _scatter(c, 6, 6, 20)
    c.cell(0, 0, 1496, k=127)
    return _position(c.points(), pts_in_cell=1499)


def claim_first_block_large(inp, M):
    assert M["sizes"][0] == 1499 and M["big"][0]["b"] == 0 and M["big"][0]["V"] == 8
    assert (M["big"][0]["dmin"], M["big"][0]["dmax"]) == (0.0, 1.0)


def build_one_d_big(keyed):
    def build():
        """6 x 6 unit blocks (fsh = 0) and a block of 1100 points of one d (its right edge): the rectangle's range of d is
        usable, so the block gets a BigInfo, but every record maps to the last sub-range, which comes out above 1024 and is
        passed on to the general kernel's list (nbinfo = 1, nfall = 1) -- which orders it by index.  The keyed form
        partitions on these coordinates and clusters on others (the same points, listed backwards)."""
        c = Cloud(14).frame(6, 6)
        _scatter(c, 6, 6, 20, avoid=[(1, 4), (0, 2)])
        c.one_d(1, 4, 1100).one_d(0, 2, 300)
        pts = c.points()
        if keyed:
            return _position(np.ascontiguousarray(pts[::-1]), lattice=2.0 ** -12, eps=2.0 ** -14, key_xy=pts)
        return _position(pts, lattice=2.0 ** -12, eps=2.0 ** -14)
    return build


def build_skewed():
    """A block of 2000 points in unit block (0, 1), where d = x - 0 runs over (1, 2]: 1100 of them with x in (1, 1.125], the
    first of its V = 8 sub-ranges, the other 900 anywhere.  That one sub-range comes out above 1024 and goes to the general
    kernel's list; the other seven stay with the LDS kernel."""
    c = Cloud(15).frame(6, 6)
    _scatter(c, 6, 6, 20, avoid=[(0, 1)])
    i, j = np.meshgrid(np.arange(1, 16), np.arange(1, 129), indexing="ij")  # x in (1, 1.125): 15 x 128 sites
    left = np.stack([1.0 + i.ravel() * STEP, j.ravel() * STEP], axis=1)
    c.add(left[c.rng.permutation(len(left))[:1100]])
    c.cell(0, 1, 900, k=64, at=(32, 0))  # x in (1.25, 1.75]
    return _position(c.points())


def claim_skewed(inp, M):
    (b,) = M["big"]
    assert b["m"] == 2000 and b["V"] == 8 and b["fill"][0] == 1100 and b["over"] == 1


def build_small_one_d():
    """Small blocks whose points all share one d (300 and 1024 points, the latter with the LDS kernel's most sub-buckets,
    nsb = 512): sb_map finds kmax == kmin and orders the run through by_idx, the index's own range."""
    c = Cloud(16).frame(6, 6)
    _scatter(c, 6, 6, 20, avoid=[(1, 3), (0, 4)])
    c.one_d(1, 3, 300).one_d(0, 4, 1024)
    return _position(c.points(), lattice=2.0 ** -12, eps=2.0 ** -14)


# -- the cluster stage
def build_all_pairs(size, full):
    def build():
        """Clustered: eps = 2^-6, min_pts 3, and a block of `size` points on a quarter of the sites of a 2^-6 lattice, so
        neighbours are the lattice neighbours at EXACTLY eps.  The all-pairs kernel has an instance for blocks of up to
        BRT = 256 points and one for up to 1024: 257 points need the second (any_mid), 1025 leave it for the grid engine
        (pts_big).  The other blocks hold up to 200 points."""
        c = Cloud(17).frame(6, 6)
        for p, q, cnt in ((1, 1, 200), (3, 2, 120), (4, 4, 60), (2, 4, 9), (4, 0, 1)):
            c.cell(p, q, cnt, k=2 * int(np.ceil(np.sqrt(cnt))), step=2.0 ** -6)
        c.cell(2, 3, full, keep=size, k=32 if full <= 257 else 64, step=2.0 ** -6)
        return _clustered(c.points(), 2.0 ** -6, 3)
    return build


# -- the final order
def build_ids_small(size):
    def build():
        """A small block of `size` points, every point a cluster: 512 ids fill the final order's table (CS_CAP), 513
        overflow it -- k_block_order raises the flag and the finish repeats the order by library sort.  No other block
        comes near."""
        c = Cloud(18).frame(6, 6)
        _scatter(c, 6, 6, 20, avoid=[(3, 3)])
        c.cell(3, 3, 513, keep=size)
        return _position(c.points())
    return build


def build_ids_big(singles):
    def build():
        """Clustered, min_pts 1 and eps = 2^-7: a block of 600 points that fill a 24 x 25 patch of the 2^-7 lattice (one
        cluster) and `singles` points 2^-5 apart and away from the patch (a cluster each): 1111 / 1112 points, a large
        block, with 512 / 513 cluster ids -- k_block_order_big's side of the CS_CAP edge."""
        c = Cloud(19).frame(6, 6)
        _scatter(c, 6, 6, 20, most=12, avoid=[(2, 3)])
        i, j = np.meshgrid(np.arange(1, 25), np.arange(1, 26), indexing="ij")
        c.add(np.stack([3.0 + i.ravel() * STEP, 2.0 + j.ravel() * STEP], axis=1))
        i, j = np.meshgrid(np.arange(1, 33), np.arange(1, 33), indexing="ij")
        far = (i.ravel() > 8) | (j.ravel() > 8)
        lone = np.stack([3.0 + i.ravel()[far] / 32.0, 2.0 + j.ravel()[far] / 32.0], axis=1)
        c.add(lone[c.rng.permutation(len(lone))[:512]], keep=singles)
        inp = _clustered(c.points(), STEP, 1, small_max=0, lattice=STEP)
        return inp
    return build


# ---- the table ---------------------------------------------------------------------------------------------------------
class Case:
    def __init__(self, name, build, want, claim=None, limit=10_000):
        self.name, self.build, self.want, self.claim, self.limit = name, build, dict(want), claim, limit
        self.__doc__ = build.__doc__


def _table():
    ge1 = lambda v: v >= 1  # noqa: E731
    t = [
        Case("select_first_digit", build_select_first_digit, {"plan.passes": 1, "plan.n": 2000, "plan.nblocks": 64, "build.nbig": 0}),
        Case("cand_cap_65536", build_cand_cap(65536), {"plan.passes": 1, "plan.n": 65537, "build.nslice": lambda v: v > 8},
             limit=70_000),
        Case("cand_cap_65537", build_cand_cap(65537), {"plan.passes": 2, "plan.n": 65538}, limit=70_000),
        Case("select_ties_pic50", build_select_ties(50), {"plan.passes": 7, "plan.take": 50}, limit=70_000),
        Case("select_ties_pic40000", build_select_ties(40000),
             {"plan.passes": 7, "plan.fsh": 0, "build.nbig": 1, "build.nbinfo": 1, "build.nfall": 1}, limit=70_000),
        Case("take_tie", build_take_tie, {"plan.take": 4}, claim_take_tie),
        Case("one_block_take_n", build_one_block(0), {"plan.take": 300, "plan.nblocks": 4, "build.m": 300}),
        Case("one_block_take_clamped", build_one_block(7), {"plan.take": 300, "plan.nblocks": 4, "build.m": 300}),
        Case("zero_extent", build_zero_extent, {"error": ERR_DEGENERATE}),
        Case("pic1_two_minima", build_pic1_two_minima, {"plan.take": 1, "plan.rows": 25, "plan.cols": 13}, claim_two_minima),
        Case("fsh0_lds_32767", build_lds(217, 151, 1500),
             {"plan.fsh": 0, "plan.NS": 32768, "plan.nblocks": 32767, "build.nbinfo": 1}),
        Case("fsh1_32768", build_lds(256, 128, 0), {"plan.fsh": 1, "plan.nblocks": 32768, "plan.NS": 16385, "build.nbig": 0}),
        Case("tracked_split", build_tracked_split,
             {"plan.fsh": 1, "build.nbig": 2, "build.nbinfo": 1, "build.nfall": ge1, "tracked": True}),
        Case("untracked_split", build_untracked_split,
             {"plan.fsh": 10, "build.nbig": 1, "build.nbinfo": 0, "build.nfall": 1, "tracked": False}),
        Case("no_block_points", build_no_block, {"plan.fsh": 0, "plan.NS": lambda v: v <= 16384}, claim_no_block),
        Case("big_edge_1024", build_block_of(1024, 1025), {"build.nbig": 0, "build.nvirt": 0, "build.nslice": 0}),
        Case("big_edge_1025", build_block_of(1025, 1025),
             {"build.nbig": 1, "build.nbinfo": 1, "build.nvirt": 8, "build.nslice": 1, "build.nfall": 0}),
        Case("first_block_large", build_first_block_large, {"plan.take": 1499, "build.nbig": ge1, "build.nbinfo": ge1},
             claim_first_block_large),
        Case("slices_4096", build_block_of(4096, 4097), {"build.nbig": 1, "build.nslice": 1, "build.nvirt": 16}),
        Case("slices_4097", build_block_of(4097, 4097), {"build.nbig": 1, "build.nslice": 2, "build.nvirt": 32}),
        Case("fsh0_one_d_big", build_one_d_big(False), {"plan.fsh": 0, "plan.keyed": 0, "build.nbinfo": 1, "build.nfall": 1}),
        Case("keyed_one_d_big", build_one_d_big(True), {"plan.fsh": 0, "plan.keyed": 1, "build.nbinfo": 1, "build.nfall": 1}),
        Case("skewed_d", build_skewed, {"build.nbig": 1, "build.nvirt": 8, "build.nfall": 1}, claim_skewed),
        Case("small_one_d", build_small_one_d, {"build.nbig": 0, "build.nfall": 0}),
        Case("all_pairs_256", build_all_pairs(256, 257), {"cluster.any_mid": 0, "cluster.pts_big": 0}),
        Case("all_pairs_257", build_all_pairs(257, 257), {"cluster.any_mid": 1, "cluster.pts_big": 0}),
        Case("all_pairs_1024", build_all_pairs(1024, 1025), {"cluster.any_mid": 1, "cluster.pts_big": 0}),
        Case("all_pairs_1025", build_all_pairs(1025, 1025), {"cluster.pts_big": 1025, "build.nbig": 1}),
        Case("ids_small_512", build_ids_small(512), {"ids_max": 512, "retry": False, "build.nbig": 0}),
        Case("ids_small_513", build_ids_small(513), {"ids_max": 513, "retry": True, "build.nbig": 0}),
        Case("ids_big_512", build_ids_big(511), {"ids_max": 512, "retry": False, "build.nbig": 1}),
        Case("ids_big_513", build_ids_big(512), {"ids_max": 513, "retry": True, "build.nbig": 1}),
    ]
    names = [c.name for c in t]
    assert len(set(names)) == len(names)
    return t


CASES = _table()
BY_NAME = {c.name: c for c in CASES}
# the two sides of every threshold: (smaller, larger, points the larger case has more)
PAIRS = (("cand_cap_65536", "cand_cap_65537", 1), ("big_edge_1024", "big_edge_1025", 1), ("slices_4096", "slices_4097", 1),
         ("all_pairs_256", "all_pairs_257", 1), ("all_pairs_1024", "all_pairs_1025", 1), ("ids_small_512", "ids_small_513", 1),
         ("ids_big_512", "ids_big_513", 1))


def lookup(M, key):
    """a field of the model by its dotted name ("plan.passes", "retry", ...)"""
    v = M
    for part in key.split("."):
        v = v[part]
    return v


def check_want(case, M):
    """-> complaints: the claims of the case that the model does not show"""
    bad = []
    for key, want in case.want.items():
        got = lookup(M, key)
        if not (want(got) if callable(want) else got == want):
            bad.append("%s: %s is %r%s" % (case.name, key, got, "" if callable(want) else ", wanted %r" % (want,)))
    return bad
