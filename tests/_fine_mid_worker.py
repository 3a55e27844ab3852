"""Worker of tests/test_fine_mid_gpu.py: one case of the grid build's fine pass (csrc/gridbuild.hip: k_part_fine_small,
k_part_fine_mid, k_part_fine) or of its output scatter (k_out_scatter) against the CPU oracle, in a process of its own
because VCP_FINE_MID is read once per process.  The parent sets VCP_TRACE and reads the trace from stderr.
usage: _fine_mid_worker.py CASE; exit status 0 = every comparison held.

The 2-D clouds are laid out by BUCKET.  eps = 1 and coordinates on the 2^-10 lattice (no pair is undecided); the cell
edge is eps * (1 + about 1e-4), so a point at (cx + f, cy + f) with 0.25 <= f < 0.75 lies in cell (cx, cy) for every
cx, cy < 1024, whose id is cy * D0 + cx.  With D0 cells per row a bucket of 2^csh cells is a band of 2^csh / D0 rows, and
what a bucket holds decides which kernel takes it:
    k_part_fine_small   at most SCAP = 2048 records and at most SPOP = 128 populous words (a word = 32 cells, populous =
                        some cell of three or more)
    k_part_fine_mid     the others of at most MCAP = 8192 records (2-D builds, VCP_FINE_MID not 0)
    k_part_fine         the rest
The parent checks the `small= mid= big=` counts printed here against the trace."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

Q = 1024.0
SCAP, SPOP, MCAP, STG = 2048, 128, 8192, 2048  # csrc/gridbuild.hip: scap(2), SPOP, mcap(2), mstg(2)
OT, OPT = 1024, 10                               # k_out_scatter: positions per workgroup = OT * OPT


def same(g, o, what):
    assert np.array_equal(g["labels"], o["labels"]), what + ": labels"
    assert np.array_equal(g["is_core"], o["is_key"]), what + ": is_core"
    assert np.array_equal(g["is_classed"], o["classed"]), what + ": is_classed"
    assert g["cf"] == o["cf"], what + ": cf %d != %d" % (g["cf"], o["cf"])
    assert g["evals"] == o["evals"], what + ": evals"


class Layout:
    """Buckets of a D0 x D1 grid, filled cell by cell."""

    def __init__(self, d0, d1, csh, seed):
        self.d0, self.d1, self.csh = d0, d1, csh
        self.rows = (1 << csh) // d0          # rows per bucket
        assert self.rows * d0 == 1 << csh and d1 % self.rows == 0
        self.rng = np.random.default_rng(seed)
        self.pts = []
        self.count = np.zeros(d1 // self.rows, np.int64)       # records per bucket
        self.cells = {}                                         # cell id -> records

    def put(self, b, cell, k):
        """k points in cell `cell` (0 .. 2^csh - 1) of bucket b"""
        cid = (b << self.csh) + cell
        cx, cy = cid % self.d0, cid // self.d0
        f = self.rng.integers(256, 768, (k, 2)) / Q
        self.pts.append(np.array([cx, cy], np.float64) + f)
        self.count[b] += k
        self.cells[cid] = self.cells.get(cid, 0) + k

    def spread(self, b, m, per_cell=2, first=0, step=1):
        """m records, per_cell to a cell, over the cells first, first + step, ..."""
        cell = first
        while m > 0:
            k = min(per_cell, m)
            self.put(b, cell, k)
            m -= k
            cell += step
        assert cell - step < 1 << self.csh

    def cloud(self, anchors=True):
        """-> coordinates in shuffled caller order; two anchor points span the grid (bucket 0, cell 0 and the last cell)"""
        if anchors:
            self.pts.append(np.array([[0.0, 0.0]]))
            self.count[0] += 1
            self.cells[0] = self.cells.get(0, 0) + 1
            self.pts.append(np.array([[self.d0 - 0.125, self.d1 - 0.125]]))
            self.count[-1] += 1
            last = self.d0 * self.d1 - 1
            self.cells[last] = self.cells.get(last, 0) + 1
        c = np.concatenate(self.pts)
        return c[self.rng.permutation(len(c))]

    def expect(self, mid_on):
        """which kernel takes each bucket -> (small, mid, big); the table's own last bucket (entry ncells) is small"""
        small = mid = big = 0
        for b, m in enumerate(self.count):
            words = {}
            for cid, k in self.cells.items():
                if cid >> self.csh == b and k >= 3:
                    words[cid >> 5] = 1
            if m <= SCAP and len(words) <= SPOP:
                small += 1
            elif m <= MCAP and mid_on:
                mid += 1
            else:
                big += 1
        nb = (self.d0 * self.d1 + 1 + (1 << self.csh) - 1) >> self.csh
        return small + (nb - len(self.count)), mid, big


def report(lay, mid_on):
    print("expect small=%d mid=%d big=%d csh=%d D=%d,%d" % (lay.expect(mid_on) + (lay.csh, lay.d0, lay.d1)))


def thresholds_layout():
    """512 x 512 cells, csh 14: 16 buckets of 32 rows (+ the table's last entry in a 17th).  n is about 58 k, below
    16 * 4096, so part_geom keeps 2^14 cells per bucket."""
    L = Layout(512, 512, 14, 101)
    L.spread(0, SCAP - 1)                   # with the anchor: exactly 2048 records, no populous word -> small
    L.spread(1, SCAP + 1)                   # 2049, no populous word -> handed on for its size
    L.spread(2, 3 * (SPOP + 1), 3, 0, 32)   # 387 records, 129 populous words -> handed on for its words
    L.spread(3, 2048, 8, 5, 32)             # exactly 2048 records in 256 populous words: one staged part, full
    L.spread(4, 4096)                       # the last bucket whose records are all in registers 0 .. 3
    L.spread(5, 4097)                       # one record in register 4 (its index waits in LDS)
    L.spread(6, MCAP, 3)                    # 8192: the last the mid kernel takes, four parts
    L.spread(7, MCAP + 1, 3)                # 8193: k_part_fine, three windows
    L.put(8, 4242, 4096)                    # one cell, even id: one half-word counts to 4096
    L.put(9, 4243, 4096)                    # one cell, odd id: the upper half-word
    L.put(10, 6000, 2048)                   # two cells of one 32-bit counter word ...
    L.put(10, 6001, 2048)                   # ... 2048 each
    # bucket 11 stays empty, between full ones
    L.put(12, 100, 2040)                    # final positions 0 .. 2039
    L.put(12, 131, 20)                      # 2040 .. 2059: one cell across the parts' border at 2047 | 2048
    L.put(12, 9000, 5)                      # a cell of five beside empty ones: one word's 32 starts in full
    L.spread(12, 500, 1, 9100, 3)
    L.put(13, 16383, 1)                     # exactly one record, in the bucket's last cell
    L.spread(14, 6000, 5, 3, 7)             # 6000 records in cells of five: populous words, two registers' worth parked
    L.spread(15, 2999, 2, 1, 5)             # the grid's last bucket with cells (with the anchor: 3000)
    return L


def case_thresholds(ctx, O, N, mid_on):
    L = thresholds_layout()
    c = L.cloud()
    report(L, mid_on)
    same(ctx.dbscan(c, 1.0, 4, N.L1_2D), O.dbscan(c, 1.0, 4, N.L1_2D), "thresholds")


def case_nonfinite(ctx, O, N, mid_on):
    """The same layout with 40 points made NaN / infinite: fewer than n records arrive (what a bucket then holds is read
    from the trace only)."""
    L = thresholds_layout()
    c = L.cloud()
    rng = np.random.default_rng(7)
    bad = rng.choice(len(c), 40, replace=False)
    c[bad[:10]] = np.nan
    c[bad[10:20], 0] = np.inf
    c[bad[20:30], 1] = -np.inf
    c[bad[30:], 1] = np.nan
    c[0], c[1] = [0.0, 0.0], [512 - 0.125, 512 - 0.125]  # the anchors stay
    same(ctx.dbscan(c, 1.0, 4, N.L1_2D), O.dbscan(c, 1.0, 4, N.L1_2D), "nonfinite")


def case_classed(ctx, O, N, mid_on):
    """An isClassed input: fine_flush writes the flags, k_out_write keeps the labels of unlabelled points."""
    L = thresholds_layout()
    c = L.cloud()
    rng = np.random.default_rng(8)
    cls = (rng.random(len(c)) < 0.3).astype(np.uint8)
    lab = np.where(cls != 0, 1 + rng.integers(0, 3, len(c)), 0).astype(np.int32)
    report(L, mid_on)
    g = ctx.dbscan(c, 1.0, 4, N.L1_2D, cf_in=3, in_classed=cls, labels=lab)
    same(g, O.dbscan(c, 1.0, 4, N.L1_2D, 3, cls, lab), "classed")


def coarse(csh, d0, d1, counts, seed):
    L = Layout(d0, d1, csh, seed)
    for b, m in enumerate(counts):
        L.spread(b, m, 10, b % 3, 1)
    return L


def case_coarse10(ctx, O, N, mid_on):
    """64 x 64 cells and 20 k points: part_geom goes down to 2^10 cells per bucket (64 scanning threads), 4 buckets."""
    L = coarse(10, 64, 64, [3000, 5000, 8700, 3300], 21)
    c = L.cloud()
    assert (L.d0 * L.d1 >> 11) * 4096 < len(c)
    report(L, mid_on)
    same(ctx.dbscan(c, 1.0, 4, N.L1_2D), O.dbscan(c, 1.0, 4, N.L1_2D), "coarse10")


def case_coarse12(ctx, O, N, mid_on):
    """256 x 128 cells and 30 k points: 2^12 cells per bucket (256 scanning threads), 8 buckets."""
    L = coarse(12, 256, 128, [2500, 4096, 4097, 8192, 8200, 1000, 1400, 500], 22)
    c = L.cloud()
    assert (L.d0 * L.d1 >> 13) * 4096 < len(c) <= (L.d0 * L.d1 >> 12) * 4096
    report(L, mid_on)
    same(ctx.dbscan(c, 1.0, 4, N.L1_2D), O.dbscan(c, 1.0, 4, N.L1_2D), "coarse12")


def case_3d(ctx, O, N, mid_on):
    """L2_3D: the 3-D build keeps the old path (the trace has to say mid_on=0); a clump of 9000 points in one bucket."""
    rng = np.random.default_rng(33)
    bg = rng.random((6000, 3)) * 48.0
    clump = 20.0 + rng.random((9000, 3)) * np.array([12.0, 3.0, 1.0])
    c = np.round(np.concatenate([bg, clump]) * Q) / Q
    c = c[rng.permutation(len(c))]
    same(ctx.dbscan(c, 1.0, 5, N.L2_3D), O.dbscan(c, 1.0, 5, N.L2_3D), "3d")


def case_grouped(ctx, O, N, mid_on):
    """Block pipeline (oracle.block_pipeline): the blocks above 1024 points go to the grid engine as one grouped call."""
    rng = np.random.default_rng(41)
    c = rng.random((24000, 2)) * 40.0
    c[:15000] = rng.random((15000, 2)) * 3.0 + rng.integers(0, 2, (15000, 2)) * 20.0
    motor = np.round(c * Q) / Q
    eps, mp, pic = 0.0625, 6, 6000
    g = ctx.dbscan_blocks(motor, eps, mp, pic, 3)
    o = O.block_pipeline(motor, eps, mp, pic, 3)
    for k in ("labels", "block_of", "order"):
        assert np.array_equal(g[k], o[k]), "grouped: %s" % k
    for k in ("rows", "cols", "kept", "del_sum", "cluster_amount", "evals"):
        assert g[k] == o[k], "grouped: %s %r != %r" % (k, g[k], o[k])


def case_slab(ctx, O, N, mid_on):
    """distributed.exact_slabs_local on two contexts: every rank's staged engine call builds its grid with d_ord."""
    import torch
    from vtkcloudpoint_amd import distributed as D
    rng = np.random.default_rng(51)
    c = rng.random((16000, 2)) * np.array([64.0, 24.0])
    c[:9000] = np.array([8.0, 4.0]) + rng.random((9000, 2)) * np.array([48.0, 2.0])
    c = np.round(c * Q) / Q
    c = c[np.argsort(c[:, 0], kind="stable")]
    ctx2 = N.Context(0)
    try:
        parts = [torch.from_numpy(np.ascontiguousarray(c[a:b])).cuda() for a, b in ((0, 8000), (8000, 16000))]
        res = D.exact_slabs_local([ctx, ctx2], parts, 0.25, 5, N.L1_2D, 0)
        o = O.dbscan(c, 0.25, 5, N.L1_2D)
        whole = {k: np.concatenate([r[k].cpu().numpy() for r in res]) for k in ("labels", "is_core", "is_classed")}
        for r in res:
            same(dict(whole, cf=r["cf"], evals=r["dist_evals"]), o, "slab")
    finally:
        ctx2.close()


def case_scatter(ctx, O, N, mid_on):
    """k_out_scatter<13> at its edges (the 14 and 15 instantiations start at 4 M and 8 M points: too large for a test of
    seconds).  n one below, at and one above a workgroup's span; n = 8192 and below: every list position in one window;
    5 * 8192 + 3 shuffled points: every workgroup touches all six windows; n not a multiple of 4 with output pointers
    off their natural alignment (device entry point)."""
    import torch
    rng = np.random.default_rng(61)
    span = OT * OPT
    for n in (span - 1, span, span + 1, 8192, 5 * 8192 + 3):
        c = np.round(rng.random((n, 2)) * 90.0 * Q) / Q
        same(ctx.dbscan(c, 1.0, 3, N.L1_2D), O.dbscan(c, 1.0, 3, N.L1_2D), "scatter n=%d" % n)
    n = 2 * span + 1023
    c = np.round(rng.random((n, 2)) * 120.0 * Q) / Q
    o = O.dbscan(c, 1.0, 3, N.L1_2D)
    d_c = torch.from_numpy(c).cuda()
    d_lab = torch.zeros(n + 8, dtype=torch.int32, device="cuda")
    d_core = torch.zeros(n + 8, dtype=torch.uint8, device="cuda")
    d_cls = torch.zeros(n + 8, dtype=torch.uint8, device="cuda")
    cf, ev = ctx.dbscan_dev(d_c.data_ptr(), n, 2, 1.0, 3, N.L1_2D, 0, None, d_lab[1:].data_ptr(), d_core[3:].data_ptr(),
                            d_cls[1:].data_ptr())
    torch.cuda.synchronize()
    g = dict(labels=d_lab[1:n + 1].cpu().numpy(), is_core=d_core[3:n + 3].cpu().numpy(),
             is_classed=d_cls[1:n + 1].cpu().numpy(), cf=cf, evals=ev)
    same(g, o, "scatter unaligned")
    assert int(d_lab[0]) == 0 and int(d_lab[n + 1]) == 0 and int(d_core[2]) == 0 and int(d_core[n + 3]) == 0


CASES = {"thresholds": case_thresholds, "nonfinite": case_nonfinite, "classed": case_classed, "coarse10": case_coarse10,
         "coarse12": case_coarse12, "3d": case_3d, "grouped": case_grouped, "slab": case_slab, "scatter": case_scatter}


def main():
    from oracle import binding as O
    from vtkcloudpoint_amd import _native as N
    O.build()
    mid_on = os.environ.get("VCP_FINE_MID", "1") != "0"
    ctx = N.Context(0)
    try:
        CASES[sys.argv[1]](ctx, O, N, mid_on)
    finally:
        ctx.close()
    print("ok", sys.argv[1], "VCP_FINE_MID=%s" % os.environ.get("VCP_FINE_MID", "(unset)"))


if __name__ == "__main__":
    main()
