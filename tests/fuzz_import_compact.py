"""Randomised sweep of vcp_import_compact against the restatement of its definition (tests/import_compact_ref.py), next to
tests/fuzz_queries.py: a fixed number of cases from a seed, n up to 30 000, random duplication (from none to a few classes
that hold everything), filtering (none to all), groups (none, few, one per row, negative), zero angles far from the origin
(the conversion's arguments then round), rows that differ in the sign of a zero or hold a NaN, with and without the
duplicate search, host and device-pointer form.  make_case(rng) builds the inputs (no GPU; a function of the seed alone),
check(ctx, case) runs the device and compares for equality, doubles by their bits.
usage: python tests/fuzz_import_compact.py [cases] [seed]"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import import_compact_ref as R  # noqa: E402

SUITE = (24, 7)           # the bounded form of tests/test_import_compact_gpu.py: (cases, seed)
N_MAX = 30_000
ANGLES = (0.0, 1.5, -0.5, 1e5, -7e5, 2.0 ** 40)


def make_case(rng):
    u = rng.uniform()
    n = int(rng.integers(1000, N_MAX + 1)) if u < 0.5 else int(10 ** rng.uniform(0, 3)) if u < 0.9 else int(rng.integers(0, 4))
    x_angle, y_angle = (float(ANGLES[i]) for i in rng.integers(0, len(ANGLES), 2))
    k = max(1, int(n * rng.choice([1.0, 0.5, 0.1, 0.002])))                  # distinct rows to draw from
    base = np.c_[np.round(rng.uniform(0, 40, (k, 2)) * 64) / 64 + [x_angle, y_angle], np.round(rng.uniform(1, 900, k) * 8) / 8]
    rows = base[rng.integers(0, k, n)] if n else np.zeros((0, 3))
    for i in rng.integers(0, max(n, 1), min(n, 6)):                          # a few special rows, some of them twice
        rows[i] = [(x_angle, rows[i, 1], rows[i, 2]), (-x_angle if x_angle == 0 else x_angle, rows[i, 1], rows[i, 2]),
                   (np.nan, 5.0, 7.0), (3.0, 4.0, np.nan), (3.0, 4.0, 1000.0), (3.0, 4.0, -2.0)][int(rng.integers(0, 6))]
        rows[int(rng.integers(0, n))] = rows[i]
    if n and x_angle == 0:
        z = rng.integers(0, n, 4)
        rows[z[:2], 0], rows[z[2:], 0] = 0.0, -0.0                           # mx - x_angle = +0 and -0
    share = float(rng.choice([0.0, 0.05, 0.05, 0.5, 1.0]))                   # filtered
    f = rng.uniform(size=n) < share
    rows[f, 2] = rng.choice([0.0, -0.0, 1000.5, np.inf, 2000.0], int(f.sum()))
    kind = int(rng.integers(0, 4))
    group = (None, rng.integers(-2, 3, n), np.arange(n) - n // 2, np.full(n, -2 ** 31))[kind]
    group = None if group is None else np.ascontiguousarray(group, np.int32)
    return dict(rows=np.ascontiguousarray(rows), group=group, x_angle=x_angle, y_angle=y_angle,
                dedupe=bool(rng.uniform() < 0.8), dev=bool(rng.uniform() < 0.5))


def cases(count, seed):
    rng = np.random.default_rng(seed)
    return [make_case(rng) for _ in range(count)]


def run_dev(ctx, rows, group, x_angle, y_angle, dedupe, xdir=2, ydir=1):
    """The device-pointer form on torch tensors filled with a poison; the dict of Context.import_compact."""
    import torch
    n = len(rows)
    t = torch.from_numpy(np.ascontiguousarray(rows, np.float64)).cuda()
    g = None if group is None else torch.from_numpy(np.ascontiguousarray(group, np.int32)).cuda()
    room = max(n, 1)
    f = {k: torch.full((room * w,), -7.25, dtype=torch.float64, device="cuda") for k, w in (("motor", 2), ("xyz", 3), ("dist", 1))}
    i = {k: torch.full((room,), -9, dtype=torch.int32, device="cuda") for k in ("src", "count", "group", "row_to")}
    torch.cuda.synchronize()                      # the library runs on its own stream
    m, dup = ctx.import_compact_dev(t.data_ptr(), n, None if g is None else g.data_ptr(), x_angle, y_angle, xdir, ydir,
                                    dedupe, f["motor"].data_ptr(), f["xyz"].data_ptr(), f["dist"].data_ptr(),
                                    i["src"].data_ptr(), i["count"].data_ptr(), i["group"].data_ptr(), i["row_to"].data_ptr())
    out = dict(m=m, duplicates=dup)
    for k, w in (("motor", 2), ("xyz", 3), ("dist", 1)):
        a = f[k].cpu().numpy()
        assert (a[m * w:] == -7.25).all(), "%s written beyond m" % k
        out[k] = a[: m * w].reshape(m, w) if w > 1 else a[:m]
    for k in ("src", "count", "group"):
        a = i[k].cpu().numpy()
        assert (a[m:] == -9).all(), "%s written beyond m" % k
        out[k] = a[:m]
    out["row_to"] = i["row_to"].cpu().numpy()[:n]
    return out


def check(ctx, case):
    rows, group, xa, ya, dedupe = (case[k] for k in ("rows", "group", "x_angle", "y_angle", "dedupe"))
    c = ctx.import_convert(rows, xa, ya, 2, 1, dedupe=False)
    want = R.compact(rows, c["xyz"], c["state"], group, dedupe)
    got = run_dev(ctx, rows, group, xa, ya, dedupe) if case["dev"] else ctx.import_compact(rows, group, xa, ya, 2, 1, dedupe)
    bad = R.same(got, want)
    assert bad is None, "%s differs (n %d, dedupe %s, dev %s, angles %r %r)" % (bad, len(rows), dedupe, case["dev"], xa, ya)
    if group is None:                             # the identities with vcp_import_convert
        d = ctx.import_convert(rows, xa, ya, 2, 1, dedupe=dedupe)
        assert np.array_equal(got["src"], np.nonzero(d["state"] == 1)[0]) and got["duplicates"] == d["duplicates"]
        assert np.array_equal(got["xyz"].view(np.uint64), d["xyz"][got["src"]].view(np.uint64))
    return want


def summary(case_list, wants):
    """What the list covers, for the conditions that keep the sweep from passing by being empty."""
    return dict(cases=len(case_list), duplicates=sum(w["duplicates"] for w in wants),
                grouped=sum(c["group"] is not None for c in case_list), dev=sum(c["dev"] for c in case_list),
                plain=sum(not c["dedupe"] for c in case_list), largest=max(len(c["rows"]) for c in case_list),
                all_filtered=sum(len(c["rows"]) > 0 and w["m"] + w["duplicates"] == 0 for c, w in zip(case_list, wants)),
                big_class=max((int(w["count"].max()) for w in wants if w["m"]), default=0))


if __name__ == "__main__":
    from vtkcloudpoint_amd import _native as N
    count = int(sys.argv[1]) if len(sys.argv) > 1 else 200
    seed = int(sys.argv[2]) if len(sys.argv) > 2 else 1
    ctx = N.Context(0)
    lst = cases(count, seed)
    print(summary(lst, [check(ctx, c) for c in lst]))
