"""The case table of the block pipeline's paths (tests/block_path_cases.py) held to the source and to the oracle, without a
GPU: every case is deterministic, small and says why it reaches its path; the numpy restatement of the partition equals the
oracle's block_of, rows, cols and order; the position cases return labels == 1 + position in the oracle; the model shows
what every case claims; every launch site of csrc/blockpart.hip and csrc/blocks.hip is expected by some case (or named as
the sharded stages' own), and every threshold the model repeats equals its definition in the source.
tests/test_block_paths_gpu.py runs the same table on the device."""
import os
import re

import numpy as np
import pytest

import block_path_cases as T
from test_engine_paths import launch_sites

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vtkcloudpoint_amd", "csrc")
_cache = {}


def built(case):
    """(inp, model, oracle result or None) of a case, computed once and left unchanged"""
    if case.name not in _cache:
        from oracle import binding as O
        inp = case.build()
        M = T.model(inp)
        o = None
        if not M["error"]:
            o = O.block_pipeline(inp["motor"], inp["eps"], inp["min_pts"], inp["pts_in_cell"], inp["small_max"],
                                 key_xy=inp.get("key_xy"))
        _cache[case.name] = (inp, M, o)
    return _cache[case.name]


@pytest.mark.parametrize("case", T.CASES, ids=lambda c: c.name)
def test_case_is_deterministic_small_and_says_why(case, oracle):
    assert case.__doc__ and len(case.__doc__) > 80, "every case says why its path is reached"
    inp, again = built(case)[0], case.build()
    for k in ("motor", "key_xy"):
        assert (k in inp) == (k in again) and (k not in inp or inp[k].tobytes() == again[k].tobytes()), "the same bits twice"
    assert {k: v for k, v in inp.items() if k not in ("motor", "key_xy")} == \
        {k: v for k, v in again.items() if k not in ("motor", "key_xy")}
    assert len(inp["motor"]) <= case.limit and case.limit in (10_000, 70_000)
    for k in ("motor", "key_xy"):
        if k in inp:
            c = inp[k]
            assert np.array_equal(c / inp["lattice"], np.round(c / inp["lattice"])), "coordinates on the case's lattice"
            assert len(np.unique(c, axis=0)) == len(c), "distinct points"
    if inp["kind"] in ("position", "error"):
        # distinct lattice points are at least one step apart: with eps below the step nobody has a neighbour
        assert inp["min_pts"] == 1 and inp["small_max"] == 0 and 0.0 < inp["eps"] < inp["lattice"]
    else:
        assert inp["eps"] >= inp["lattice"] and inp["eps"] / inp["lattice"] == round(inp["eps"] / inp["lattice"]), \
            "pairs at exactly eps exist on the lattice"


@pytest.mark.parametrize("case", T.CASES, ids=lambda c: c.name)
def test_the_restated_partition_equals_the_oracle(case, oracle):
    inp, M, o = built(case)
    if M["error"]:
        with pytest.raises(oracle.OracleError) as e:
            oracle.block_pipeline(inp["motor"], inp["eps"], inp["min_pts"], inp["pts_in_cell"], inp["small_max"])
        assert e.value.code == M["error"] == case.want["error"]
        return
    P = M["P"]
    assert (P["rows"], P["cols"]) == (o["rows"], o["cols"])
    assert np.array_equal(P["block_of"], o["block_of"])
    assert M["build"]["m"] == len(o["order"])
    if inp["kind"] == "position":
        assert np.array_equal(P["order"], o["order"]), "block-major order by (block, d, index)"
        assert np.array_equal(T.position_labels(P, len(inp["motor"])), o["labels"]), "labels == 1 + position"
        assert o["kept"] == o["cluster_amount"] == M["build"]["m"] and o["del_sum"] == 0
    else:
        assert np.array_equal(np.sort(P["order"]), np.sort(o["order"]))
        assert 0 < o["kept"] < M["build"]["m"] and (o["labels"] == 0).any() == (inp["min_pts"] > 1)


@pytest.mark.parametrize("case", T.CASES, ids=lambda c: c.name)
def test_the_model_shows_what_the_case_claims(case, oracle):
    inp, M, o = built(case)
    bad = T.check_want(case, M)
    assert not bad, "\n".join(bad)
    if case.claim:
        case.claim(inp, M)
    if M["error"]:
        return
    # the model's cluster ids per block against the oracle's own per-block DBImproved
    if "key_xy" not in inp and M["plan"]["nblocks"] < 1_000_000:
        sb = oracle.StagedBlocks()
        info = sb.blocks_begin(inp["motor"], inp["eps"], inp["min_pts"], inp["pts_in_cell"], inp["small_max"])
        local = np.zeros(max(info["m"], 1), np.int32)
        sb.blocks_cluster_dev(0, info["nblocks"], local.ctypes.data)
        start = sb.s["blockstart"]
        ids = np.maximum.reduceat(np.append(local, 0), np.minimum(start[:-1], len(local)))
        ids[start[1:] == start[:-1]] = 0
        if inp["kind"] == "position":
            assert np.array_equal(ids, M["sizes"]) and M["ids_max"] == ids.max()
        else:  # (the model looks at the blocks that can overflow the table only)
            big = M["sizes"] > T.CS_CAP
            assert (ids[big].max() if big.any() else 0) == M["ids_max"] and (ids[~big] <= T.CS_CAP).all()
    # sites() is a function of the model only: both forms expect known sites, and the staged form one more
    one, staged = T.sites(M), T.sites(M, staged=True)
    assert one <= T.SITES and staged - one == {"k_last_entry"}


def test_the_two_sides_of_a_threshold_differ_by_the_threshold_only():
    for small, large, more in T.PAIRS:
        a, b = built(T.BY_NAME[small])[0]["motor"], built(T.BY_NAME[large])[0]["motor"]
        assert len(b) == len(a) + more
        rows_a = {r.tobytes() for r in a}
        keep = np.array([r.tobytes() in rows_a for r in b])
        assert keep.sum() == len(a)
        assert np.array_equal(b[keep], a), "%s is %s without its last point, everybody else in place" % (small, large)


def test_every_launch_site_of_the_two_files_is_in_the_table():
    found = launch_sites(os.path.join(CSRC, "blockpart.hip")) + launch_sites(os.path.join(CSRC, "blocks.hip"))
    assert len(found) >= 38  # (k_transpose_u32 twice)
    assert set(found) == set(T.SITES), "block_path_cases.SITES against the source: %r" % (set(found) ^ set(T.SITES))
    expected = set()
    for c in T.CASES:
        M = built(c)[1]
        expected |= T.sites(M, staged=True)
    for c in T.CASES:  # VCP_BLOCKS_ORDER_SORT is a setting of the GPU test: the library-sort form on every case
        M = dict(built(c)[1])
        if not M["error"]:
            M.update(by_sort=True, retry=False)
            expected |= T.sites(M)
    missing = T.SITES - expected
    assert missing == T.SHARDED_ONLY, "launch sites no case expects: %r" % sorted(missing - T.SHARDED_ONLY)


def test_both_sides_of_every_fork_are_in_the_table():
    Ms = [built(c)[1] for c in T.CASES if not built(c)[1]["error"]]
    assert {M["plan"]["passes"] for M in Ms} >= {1, 2, 7}
    assert {M["plan"]["fsh"] for M in Ms} >= {0, 1, 10} and {M["tracked"] for M in Ms} == {True, False}
    assert any(M["plan"]["NS"] * 4 > 65536 for M in Ms) and any(M["plan"]["NS"] * 4 <= 65536 for M in Ms)
    assert {M["plan"]["keyed"] for M in Ms} == {0, 1}
    assert any(M["build"]["m"] < M["plan"]["n"] for M in Ms)
    bigs = [b for M in Ms for b in M["big"]]
    assert any(b["direct"] for b in bigs) and any(b["over"] for b in bigs) and any(b["V"] and not b["over"] for b in bigs)
    assert any(b["b"] == 0 for b in bigs) and min(b["V"] for b in bigs if b["V"]) == 8
    # the (d, index) tie term of k_blk_sort decides somewhere in each of its three forms: points that share a d inside a
    # small block, inside a sub-range that stays with the LDS kernel, and inside a run of the general kernel's list
    tied = {"small": False, "sub-range": False, "general": False}
    for M in Ms:
        bo, d = M["P"]["block_of"], M["P"]["d"]
        small = np.flatnonzero((M["sizes"] > 1) & (M["sizes"] <= T.VCP_BIG_BLOCK))[:50]
        tied["small"] |= any(len(np.unique(d[bo == b])) < M["sizes"][b] for b in small)
        for b in M["big"]:
            db = d[bo == b["b"]]
            if b["V"] is None:
                tied["general"] |= len(np.unique(db)) < len(db)
                continue
            sub = T._vmap(db, b["dmin"], np.float64(b["V"]) / np.float64(b["dmax"] - b["dmin"]), b["V"])
            for v in range(b["V"]):
                run = db[sub == v]
                tied["general" if len(run) > T.VCP_BIG_BLOCK else "sub-range"] |= len(np.unique(run)) < len(run)
    assert all(tied.values()), tied
    assert {M["cluster"]["any_mid"] for M in Ms} == {0, 1} and {M["cluster"]["pts_big"] > 0 for M in Ms} == {True, False}
    assert {M["retry"] for M in Ms} == {True, False}
    edge = {M["ids_max"] for M in Ms}
    assert {T.CS_CAP, T.CS_CAP + 1} <= edge
    sizes = set(np.concatenate([np.unique(M["sizes"]) for M in Ms]).tolist())
    for thr in (T.BRT, T.VCP_BIG_BLOCK, T.SLICE, T.CS_CAP):
        assert {thr, thr + 1} <= sizes, "no block of %d and %d points" % (thr, thr + 1)


def test_select_passes_on_known_strings():
    d = np.full(70_000, 5.0)
    assert T.select_passes(d[:65536], 9) == 1 and T.select_passes(d[:65537], 9) == 7
    d2 = d.copy()
    d2[::2] = np.nextafter(5.0, 6.0)  # the last bit of d is in digit 5: the halves part there
    assert T.select_passes(d2, 9) == 6
    assert T.select_passes(np.arange(70_000, dtype=np.float64), 70_000) == 1  # (the top octave holds 4464 of them)


def _constant(text, name):
    m = re.search(r"constexpr\s+\w+\s+%s\s*=\s*(\d+)\s*;" % re.escape(name), text)
    assert m, "no definition of %s" % name
    return int(m.group(1))


def test_the_thresholds_the_model_repeats_are_the_source_s():
    for fname, names in T.CONSTANTS.items():
        with open(os.path.join(CSRC, fname)) as f:
            text = f.read()
        for name in names:
            assert _constant(text, name) == getattr(T, name), "%s in %s" % (name, fname)
    with open(os.path.join(CSRC, "blockpart.hip")) as f:
        text = f.read()
    assert "s_out[2] <= CAND_CAP" in text and "F <= VF" in text and "(size_t)NS * 4 > 65536" in text
    assert text.count("V * VTARGET < m") == 2 and text.count("(unsigned long long)V * VTARGET * 8ull < m") == 2
