"""The entry points of include/vcp_planes.h under an overwritten workspace, as tests/test_workspace_poison_gpu.py holds
those of vcp.h: vcp_selftest_poison fills every workspace buffer the context lists (the b_pl_* of csrc/planes.hip are
listed like the others), the pinned scratch and the staging area with a known word before each call, and every output is
compared with the restatement tests/plane_ref.py.  Words 0x00000000, 0x00000001, then 0xFFFFFFFF (NaN as a double, -1 as
an index, UINT_MAX as a count).  The module has a context of its own; the session's is never armed.

Without a GPU: the case list names every function of the header whose first parameter is a vcp_ctx*."""
import os
import re

import numpy as np
import pytest

import plane_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORDS = (0x00000000, 0x00000001, 0xFFFFFFFF)


def _dev(a):
    import torch
    return torch.from_numpy(np.array(a, order="C")).cuda()


def _host(t):
    return t.cpu().numpy()


# ---- the cases: name, the functions they run, check(ctx) ----------------------------------------------------------------------
def _score(on_device):
    def check(ctx):
        from vtkcloudpoint_amd import planes as PL
        tile, chunk, _ = PL.plane_score_shape(ctx)
        pts, pl = R.lattice_rows(2 * tile + 3, 30), R.generic_planes(chunk + 1, 31)
        act = (np.arange(len(pts)) % 5 != 0).astype(np.uint8)
        want = R.score(pts, pl, 0.25, act)
        got = PL.plane_score(_dev(pts), _dev(pl), 0.25, _dev(act), ctx=ctx) if on_device else PL.plane_score(pts, pl, 0.25, act, ctx=ctx)
        assert np.array_equal(_host(got) if on_device else got, want) and want.sum() > 0
    return check


def _triples(ctx):
    from vtkcloudpoint_amd import planes as PL
    pts = R.lattice_rows(400, 32)
    tri = np.random.default_rng(33).integers(-2, 402, (130, 3)).astype(np.int32)
    want_pl, want_ok = R.from_triples(pts, tri)
    pl, ok = PL.planes_from_triples(_dev(pts), _dev(tri), ctx=ctx)
    assert np.array_equal(_host(ok), want_ok) and R.same(_host(pl), want_pl) and 0 < want_ok.sum() < 130


def _label(ctx):
    from vtkcloudpoint_amd import planes as PL
    pts, plane = R.lattice_rows(3000, 34), R.generic_planes(1, 35)[0]
    lab0, act0 = np.full(3000, -3, np.int32), (np.arange(3000) % 4 != 1).astype(np.uint8)
    want_lab, want_act, want_k = R.label(pts, plane, 0.5, 9, lab0, act0)
    d_lab, d_act = _dev(lab0), _dev(act0)
    assert PL.plane_label(_dev(pts), plane, 0.5, 9, d_lab, d_act, ctx=ctx) == want_k > 0
    assert np.array_equal(_host(d_lab), want_lab) and np.array_equal(_host(d_act), want_act)


def _ransac(on_device, refit):
    def check(ctx):
        import torch
        from vtkcloudpoint_amd import planes as PL
        pts, _, _, want = R.scene_fit(3, refit=refit, masked=True)
        act, c = R.scene_mask(3), R.scene_call(3)
        fit = PL.extract_planes(_dev(pts) if on_device else pts, c["thr"], c["H"], c["max_planes"], c["min_inliers"], c["seed"],
                                refit, _dev(act) if on_device else act, ctx=ctx)
        h = lambda a: _host(a) if torch.is_tensor(a) else a
        k = fit.n_planes
        assert k == want["n_planes"] == 3 and np.array_equal(h(fit.labels), want["labels"])
        assert R.same(h(fit.planes), want["planes"][:k]) and np.array_equal(h(fit.counts), want["counts"][:k])
        assert np.array_equal(h(fit.hyp_counts), want["hyp_counts"][:k])
    return check


def _shape(ctx):
    from vtkcloudpoint_amd import planes as PL
    a = PL.plane_score_shape(ctx)
    assert a == PL.plane_score_shape(ctx) and min(a) >= 1


CASES = [
    ("score/host", ("vcp_plane_score",), _score(False)),
    ("score/dev", ("vcp_plane_score_dev",), _score(True)),
    ("from_triples/dev", ("vcp_planes_from_triples_dev",), _triples),
    ("label/dev", ("vcp_plane_label_dev",), _label),
    ("ransac/host/refit", ("vcp_plane_ransac",), _ransac(False, True)),
    ("ransac/dev/refit", ("vcp_plane_ransac_dev",), _ransac(True, True)),
    ("ransac/dev/no_refit", ("vcp_plane_ransac_dev",), _ransac(True, False)),
    ("score_shape", ("vcp_plane_score_shape",), _shape),
]


def context_functions():
    """Every function of vcp_planes.h whose first parameter is a vcp_ctx* (the regex of tests/test_poison_cases.py)."""
    with open(os.path.join(ROOT, "include", "vcp_planes.h")) as f:
        src = f.read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    src = re.sub(r"//[^\n]*", "", src)
    return sorted(set(re.findall(r"\b(vcp_[a-z0-9_]+)\s*\(\s*(?:const\s+)?vcp_(?:ctx|multi)\s*\*", src)))


def test_the_case_list_names_every_context_entry_point():
    funcs = context_functions()
    named = {f for _, fs, _ in CASES for f in fs}
    assert len(funcs) == 7 and "vcp_plane_ransac_dev" in funcs and "vcp_plane_score_shape" in funcs
    assert sorted(named) == funcs
    assert len({name for name, _, _ in CASES}) == len(CASES)


_state = dict(fatal=None, most=0)


@pytest.fixture(scope="module")
def ctx():
    from vtkcloudpoint_amd import _native as N
    c = N.Context(0)
    yield c
    c.selftest_poison(0, armed=False)
    c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", [c[0] for c in CASES])
def test_case_under_every_word(ctx, name):
    if _state["fatal"]:                                  # the device reported an error: nothing more runs on it from here
        pytest.fail("not started: " + _state["fatal"])
    check = {c[0]: c[2] for c in CASES}[name]
    try:
        try:
            check(ctx)                                   # unpoisoned: the case is sound
            for word in WORDS:                           # 0xFFFFFFFF only after 0 and 1 have passed
                _, nbufs = ctx.selftest_poison(word)
                _state["most"] = max(_state["most"], nbufs)
                try:
                    check(ctx)
                except AssertionError as e:
                    raise AssertionError("under the word 0x%08X: %s" % (word, e)) from e
        finally:
            ctx.selftest_poison(0, armed=False)
    except AssertionError:
        raise
    except BaseException as e:                           # VcpError, a torch RuntimeError, ...: nothing more runs on the device
        _state["fatal"] = "%s ended with %s: %s" % (name, type(e).__name__, " ".join(str(e).split())[:300])
        raise


@pytest.mark.gpu
def test_the_fill_reaches_the_planes_buffers(ctx):
    """After the cases the context lists the five b_pl_* buffers of csrc/planes.hip beside those of the refit's
    vcp_cluster_moments_dev, and the hook fills them."""
    if _state["fatal"]:
        pytest.fail("not started: " + _state["fatal"])
    with open(os.path.join(ROOT, "vtkcloudpoint_amd", "csrc", "planes.hip")) as f:
        members = re.findall(r"^\s*DevBuf\s+([^;]+);", f.read(), flags=re.M)
    names = [m.strip() for d in members for m in d.split(",")]
    assert len(names) == 5 and all(re.fullmatch(r"b_pl_\w+", m) for m in names)
    for name in ("score/host", "ransac/host/refit"):         # between them they use all five (the shared result is cached)
        {c[0]: c[2] for c in CASES}[name](ctx)
    try:
        _, nbufs = ctx.selftest_poison(WORDS[0])
    finally:
        ctx.selftest_poison(0, armed=False)
    assert max(nbufs, _state["most"]) >= len(names) + 5     # + b_cm_misc, b_aux1 .. b_aux4 at the least
