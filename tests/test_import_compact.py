"""vcp_import_compact without a GPU: the two entry points in the header, the library, the Python binding and the C#
imports with matching arity; the restatement of the definition (tests/import_compact_ref.py) held to the project's oracle
(AddFolder's sequential duplicate search) and to gdbscan.multiplicity, with the one stated difference between the two; a
grouped run against one run per group; what the entry points answer without a device.  The device is held to equality
with the restatement in tests/test_import_compact_gpu.py.  Every comparison is equality."""
import ctypes as C
import inspect

import numpy as np
import pytest

import import_compact_ref as R
import import_ref
from test_abi import _csharp_imports, _declared, _header_prototypes

NAMES = ("vcp_import_compact", "vcp_import_compact_dev")


def test_the_two_symbols_everywhere_with_matching_arity():
    from vtkcloudpoint_amd import _native, gdbscan, io
    lib = _native.lib()
    decl, protos = _declared(), _header_prototypes()
    cs = {name: classes for _, name, classes in _csharp_imports()}
    for nm in NAMES:
        assert nm in decl and hasattr(lib, nm) and nm in _native.SYMBOLS, nm
        assert cs.get(nm) == protos[nm], (nm, cs.get(nm), protos[nm])
        assert len(protos[nm]) == 18
    assert protos["vcp_import_compact"] == ["ptr", "ptr", "i64", "ptr", "f64", "f64", "i32", "i32", "i32"] + ["ptr"] * 9
    assert protos["vcp_import_compact_dev"] == protos["vcp_import_compact"]
    assert list(inspect.signature(_native.Context.import_compact).parameters) == \
        ["self", "rows", "group", "x_angle", "y_angle", "xdir", "ydir", "dedupe"]
    assert list(inspect.signature(_native.Context.import_compact_dev).parameters) == \
        ["self", "d_rows", "n", "d_group", "x_angle", "y_angle", "xdir", "ydir", "dedupe", "d_motor", "d_xyz", "d_dist",
         "d_src", "d_count", "d_group_out", "d_row_to"]
    assert list(inspect.signature(io.import_scan_resident).parameters) == \
        ["rows", "group", "x_angle", "y_angle", "xdir", "ydir", "dedupe", "ctx"]
    assert list(inspect.signature(io.add_fixed_folder).parameters) == \
        ["files", "x_angle", "y_angle", "xdir", "ydir", "typpe", "ctx"]
    assert "vcp_import_compact" in gdbscan.multiplicity.__doc__ and "==" in gdbscan.multiplicity.__doc__


@pytest.fixture(scope="module")
def cases(oracle):
    """(rows, x_angle, y_angle, the oracle's conversion without and with the duplicate search): the fixture rows, once
    as they are and once with every third row repeated further down, and the generated 5 000-row case."""
    f = import_ref.load()
    twice = np.r_[f["rows"], f["rows"][::3]]
    mixed, xa, ya = R.mixed_rows()
    out = []
    for rows, x_angle, y_angle in ((f["rows"], f["x_angle"], f["y_angle"]), (twice, f["x_angle"], f["y_angle"]),
                                   (mixed, xa, ya)):
        out.append((rows, x_angle, y_angle, oracle.import_convert(rows, x_angle, y_angle, 2, 1, dedupe=False),
                    oracle.import_convert(rows, x_angle, y_angle, 2, 1, dedupe=True)))
    return out


def test_restatement_keeps_what_the_oracle_keeps(cases):
    dups = 0
    for rows, _, _, plain, ded in cases:
        r = R.compact(rows, plain["xyz"], plain["state"])
        assert np.array_equal(r["src"], np.nonzero(ded["state"] == 1)[0])
        assert r["duplicates"] == ded["duplicates"] and r["m"] == ded["kept"]
        assert int(r["count"].sum()) == int((plain["state"] != 0).sum()) == r["m"] + r["duplicates"]
        assert np.array_equal(r["xyz"].view(np.uint64), ded["xyz"][r["src"]].view(np.uint64))
        assert np.array_equal(r["motor"], rows[r["src"], :2], equal_nan=True)
        assert np.array_equal(r["dist"], rows[r["src"], 2], equal_nan=True)
        assert np.array_equal(r["row_to"] >= 0, plain["state"] != 0)
        kept_of = r["src"][r["row_to"][r["row_to"] >= 0]]           # every unfiltered row's class keeps an earlier row
        assert (kept_of <= np.nonzero(r["row_to"] >= 0)[0]).all()
        assert np.array_equal(r["row_to"][r["src"]], np.arange(r["m"]))
        # without the duplicate search: every unfiltered row, count 1
        p = R.compact(rows, plain["xyz"], plain["state"], dedupe=False)
        assert np.array_equal(p["src"], np.nonzero(plain["state"] != 0)[0]) and p["duplicates"] == 0
        assert (p["count"] == 1).all()
        dups += r["duplicates"]
    assert dups > 3000                                              # the duplicate search had something to find


def test_count_is_multiplicity_where_bits_and_equality_agree(cases):
    from vtkcloudpoint_amd.gdbscan import multiplicity
    for rows, _, _, plain, _ in cases:
        unf = np.nonzero(plain["state"] != 0)[0]
        q = plain["xyz"][unf]
        ok = ~np.isnan(q).any(axis=1) & ~(np.signbit(q) & (q == 0)).any(axis=1)
        assert ok.sum() > 0.9 * len(q)
        unf, q = unf[ok], q[ok]
        state = np.zeros(len(rows), np.uint8)
        state[unf] = 1                                              # the rows with a NaN or a -0 in their triple left out
        r = R.compact(rows, plain["xyz"], state)
        first, cnt = multiplicity(q)
        assert np.array_equal(r["src"], unf[first]) and np.array_equal(r["count"], cnt)


def test_the_one_difference_to_multiplicity(oracle):
    from vtkcloudpoint_amd.gdbscan import multiplicity
    rows = R.zero_pair()
    o = oracle.import_convert(rows, 0.0, 0.0, 2, 1, dedupe=False)
    ty = o["xyz"][:, 1]
    assert ty[0] == ty[1] == 0 and np.signbit(ty[0]) and not np.signbit(ty[1])      # -0 and +0: the bits differ
    assert np.array_equal(o["xyz"][0, [0, 2]].view(np.uint64), o["xyz"][1, [0, 2]].view(np.uint64))
    r = R.compact(rows, o["xyz"], o["state"])
    assert r["m"] == 1 and r["count"].tolist() == [2] and r["row_to"].tolist() == [0, 0] and r["duplicates"] == 1
    assert np.signbit(r["xyz"][0, 1])                               # the first occurrence's bits
    first, cnt = multiplicity(o["xyz"])
    assert first.tolist() == [0, 1] and cnt.tolist() == [1, 1]      # bit for bit they are two rows
    assert oracle.import_convert(rows, 0.0, 0.0, 2, 1, dedupe=True)["state"].tolist() == [1, 2]
    # and the other way round: two rows with the same NaN bits are one row to multiplicity, two classes to `==`
    nan = np.array([[np.nan, 5.0, 7.0]] * 2)
    o = oracle.import_convert(nan, 0.0, 0.0, 2, 1, dedupe=False)
    assert np.isnan(o["xyz"]).any(axis=1).all()
    r = R.compact(nan, o["xyz"], o["state"])
    assert r["m"] == 2 and r["count"].tolist() == [1, 1] and r["row_to"].tolist() == [0, 1]
    assert oracle.import_convert(nan, 0.0, 0.0, 2, 1, dedupe=True)["state"].tolist() == [1, 1]


def test_a_grouped_run_is_one_run_per_group(cases):
    rows, _, _, plain, _ = cases[2]
    n = len(rows)
    group = (np.random.default_rng(9).integers(0, 3, n) * 5 - 5).astype(np.int32)   # -5, 0, 5, interleaved
    r = R.compact(rows, plain["xyz"], plain["state"], group)
    src, count, gout = [], [], []
    for g in (-5, 0, 5):
        idx = np.nonzero(group == g)[0]
        one = R.compact(rows[idx], plain["xyz"][idx], plain["state"][idx])
        src.append(idx[one["src"]])
        count.append(one["count"])
        gout.append(np.full(one["m"], g, np.int32))
        assert np.array_equal(r["row_to"][idx] >= 0, one["row_to"] >= 0)
        ok = one["row_to"] >= 0
        assert np.array_equal(r["src"][r["row_to"][idx][ok]], idx[one["src"][one["row_to"][ok]]])
    src, count, gout = np.concatenate(src), np.concatenate(count), np.concatenate(gout)
    order = np.argsort(src, kind="stable")
    assert np.array_equal(r["src"], src[order]) and np.array_equal(r["count"], count[order])
    assert np.array_equal(r["group"], gout[order])
    assert r["m"] > R.compact(rows, plain["xyz"], plain["state"])["m"]            # the groups split some classes


def test_the_fuzz_list_is_not_empty_handed(oracle):
    """The bounded sweep of tests/test_import_compact_gpu.py, on the oracle's conversion: what the seeded list covers."""
    import fuzz_import_compact as F
    count, seed = F.SUITE
    lst = F.cases(count, seed)
    wants = []
    for c in lst:
        o = oracle.import_convert(c["rows"], c["x_angle"], c["y_angle"], 2, 1, dedupe=False)
        wants.append(R.compact(c["rows"], o["xyz"], o["state"], c["group"], c["dedupe"]))
    s = F.summary(lst, wants)
    assert s["cases"] == count and s["duplicates"] > 10_000 and s["grouped"] >= 8 and s["dev"] >= 6 and s["plain"] >= 2
    assert s["largest"] > 10_000 and s["big_class"] >= 100 and s["all_filtered"] >= 1
    assert any(np.isnan(c["rows"]).any() for c in lst)
    far = [w["duplicates"] for c, w in zip(lst, wants) if abs(c["x_angle"]) >= 1e5 or abs(c["y_angle"]) >= 1e5]
    assert len(far) >= 5 and sum(far) > 1000


def test_without_a_device_and_the_errors_before_it(tmp_path):
    """A vcp_ctx exists only on a device, so without one VCP_ERR_NO_DEVICE comes from creating the context the two entry
    points need; the errors that precede it come first.  With a device the same calls answer."""
    import torch
    from vtkcloudpoint_amd import _native, io
    lib = _native.lib()
    m = C.c_int64(-3)
    rows = np.array([[1.0, 2.0, 3.0]])
    for nm in NAMES:                                                # a NULL context: VCP_ERR_ARG, *m untouched
        rc = getattr(lib, nm)(None, _native._ptr(rows), C.c_int64(1), None, C.c_double(0.0), C.c_double(0.0), 2, 1, 1,
                              None, None, None, None, None, None, None, C.byref(m), None)
        assert rc == -1 and m.value == -3, nm
    with pytest.raises(ValueError):                                 # before the context is asked for
        io.import_scan_resident(rows, group=np.zeros(2, np.int32))
    with pytest.raises(ValueError):
        io.add_fixed_folder([], typpe=1)
    path = tmp_path / "a.txt"
    path.write_text("1.0\t2.0\t3.0\n1.0\t2.0\t3.0\n")
    if torch.cuda.is_available():
        r = io.import_scan_resident(rows)
        assert r["m"] == 1 and r["duplicates"] == 0
        clus, dup, pts, paths = io.add_fixed_folder([str(path)], typpe=3)
        assert (dup, pts, len(clus[0].li), clus[0].li[0].ptsCount) == (1, 1, 1, 2)
    else:
        for call in (lambda: io.import_scan_resident(rows), lambda: io.add_fixed_folder([str(path)], typpe=3),
                     lambda: _native.Context(0).import_compact(rows)):
            with pytest.raises(_native.VcpError) as e:
                call()
            assert e.value.code == -6                               # VCP_ERR_NO_DEVICE
