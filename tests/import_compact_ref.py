"""vcp_import_compact's definition (include/vcp.h) restated as a sequential walk with a dict, and the inputs the tests of
it share.  The walk starts from a given per-row xyz [n, 3] and state [n] (0 = filtered), as vcp_import_convert or the
oracle's import_convert writes them with dedupe off, so the same code serves the CPU tests (the oracle's values) and the GPU
tests (the device's own values): duplicate decisions are exact on either.  With dedupe the directions are xdir 2 / ydir 1,
for which (X, Y, Z) IS the triple (tmpx, tmpy, tmpz) the classes are keyed on."""
import numpy as np

KEYS = ("motor", "xyz", "dist", "src", "count", "group", "row_to")


def compact(rows, xyz, state, group=None, dedupe=True):
    """dict(motor [m,2], xyz [m,3], dist [m], src [m], count [m], group [m], row_to [n], m, duplicates)."""
    rows = np.ascontiguousarray(rows, np.float64).reshape(-1, 3)
    xyz = np.ascontiguousarray(xyz, np.float64).reshape(-1, 3)
    n = len(rows)
    g = np.zeros(n, np.int32) if group is None else np.ascontiguousarray(group, np.int32)
    seen, src, count = {}, [], []
    row_to = np.full(n, -1, np.int32)
    unfiltered = 0
    for i, (st, gi, t) in enumerate(zip(np.asarray(state).tolist(), g.tolist(), xyz.tolist())):
        if st == 0:
            continue
        unfiltered += 1
        if dedupe and t[0] == t[0] and t[1] == t[1] and t[2] == t[2]:  # a triple holding a NaN is never entered
            key = (gi, t[0] + 0.0, t[1] + 0.0, t[2] + 0.0)             # -0.0 + 0.0 is +0.0
            j = seen.get(key)
            if j is not None:
                count[j] += 1
                row_to[i] = j
                continue
            seen[key] = len(src)
        row_to[i] = len(src)
        src.append(i)
        count.append(1)
    src = np.array(src, np.int32)
    return dict(motor=rows[src, :2].copy(), xyz=xyz[src].copy(), dist=rows[src, 2].copy(), src=src,
                count=np.array(count, np.int32), group=g[src].copy(), row_to=row_to, m=len(src),
                duplicates=unfiltered - len(src))


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def same(got, want, keys=KEYS):
    """None when the two results are equal -- doubles by their bits -- else the name of the first entry that differs."""
    for k in ("m", "duplicates"):
        if int(got[k]) != int(want[k]):
            return k
    for k in keys:
        a, b = np.asarray(got[k]), np.asarray(want[k])
        if a.dtype != b.dtype or a.shape != b.shape or not np.array_equal(_bits(a), _bits(b)):
            return k
    return None


def expanded(rng, k, n_unfiltered, max_rep=9):
    """n_unfiltered rows drawn from about k distinct (mx, my, D) on a 1/64 lattice, each 1..max_rep times (few classes are
    large), not yet shuffled."""
    base = np.c_[np.round(rng.uniform(0, 40, (k, 2)) * 64) / 64, np.round(rng.uniform(1, 900, k) * 8) / 8]
    reps = 1 + np.floor(max_rep * rng.uniform(0, 1, k) ** 1.6).astype(np.int64).clip(0, max_rep - 1)
    out = np.repeat(base, reps, axis=0)[:n_unfiltered]
    if len(out) < n_unfiltered:
        extra = n_unfiltered - len(out)
        out = np.r_[out, np.c_[rng.uniform(50, 60, (extra, 2)), rng.uniform(1, 900, extra)]]
    return out


def mixed_rows(seed=2024, n=5000, k=1200):
    """The mixed case of the tests: about k classes repeated 1 to 9 times, 10 % filtered rows (D = 0, -0, 1000.5, +inf and
    values above 1000 among them), a row with D = 1000 exactly and one with D < 0 (kept), a row with NaN mx twice (kept
    twice) and a row with NaN D (kept); shuffled.  Returns (rows, x_angle, y_angle)."""
    rng = np.random.default_rng(seed)
    nf = n // 10
    special = np.array([[3.0, 4.0, 1000.0], [3.0, 4.0, -3.5], [np.nan, 5.0, 7.0], [np.nan, 5.0, 7.0], [6.0, 7.0, np.nan]])
    filt = np.c_[rng.uniform(0, 40, (nf, 2)), rng.uniform(1000.01, 1100, nf)]
    filt[:4, 2] = [0.0, 1000.5, -0.0, np.inf]
    filt[4:nf // 2, 2] = 0.0
    rows = np.r_[expanded(rng, k, n - nf - len(special)), special, filt]
    assert len(rows) == n
    return np.ascontiguousarray(rows[rng.permutation(n)]), 1.51, -0.53    # off the lattice: no angle is exactly 0


def zero_pair(y=12.5, D=33.0):
    """(+0.0, y, D) and (-0.0, y, D) at x_angle = 0: (-2) * (mx - x_angle) is -0 for the first and +0 for the second, so
    tmpy is -0 and +0 while tmpx and tmpz agree: one class of two under `==`, two classes bit for bit."""
    return np.array([[0.0, y, D], [-0.0, y, D]])


def scan_rows(seed=40):
    """A 3 000-row scan of 12 blobs on a 1/256 lattice in two range bands, expanded to 9 000 raw rows, plus 300 filtered
    rows; shuffled.  The zero angles are off the lattice: no -0 and no NaN in the converted triples.  Returns (rows,
    x_angle, y_angle)."""
    rng = np.random.default_rng(seed)
    centres = rng.uniform(2, 38, (12, 2))
    motor = np.round((centres[rng.integers(0, 12, 3000)] + rng.normal(0, 0.25, (3000, 2))) * 256) / 256
    base = np.c_[motor, np.where(rng.uniform(size=3000) < 0.5, 30.0, 80.0) + np.round(rng.uniform(0, 2, 3000) * 64) / 64]
    raw = np.r_[base, base[rng.integers(0, 3000, 6000)]]
    filt = np.c_[rng.uniform(0, 40, (300, 2)), np.where(np.arange(300) % 2, 0.0, 1200.0)]
    raw = np.r_[raw, filt][rng.permutation(9300)]
    return np.ascontiguousarray(raw), 1.51, -0.53
