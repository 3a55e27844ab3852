"""The case table of the workspace-poison test (tests/poison_cases.py), without a GPU: every entry point of include/vcp.h
that takes a context has a case or a stated exemption, the buffers vcp_selftest_poison leaves alone are the ones listed
here with their reasons, and the table is deterministic."""
import os
import re

import numpy as np

import poison_cases as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# entry points with a context that run no kernel on workspace a call could have left behind, and why
EXEMPT = {
    "vcp_destroy": "lifecycle",
    "vcp_last_error": "lifecycle: reads the context's message",
    "vcp_destroy_multi": "lifecycle",
    "vcp_multi_last_error": "lifecycle: reads the message",
    "vcp_set_stream": "selects the stream; tests/test_stream_gpu.py",
    "vcp_dev_alloc": "plain hipMalloc for the caller, no workspace",
    "vcp_dev_free": "plain hipFree",
    "vcp_h2d": "one copy, no workspace",
    "vcp_d2h": "one copy, no workspace",
    "vcp_release_workspace": "frees the workspace: nothing is read",
    "vcp_timing_enable": "timing: a host flag",
    "vcp_timing_count": "timing: reads the host's list",
    "vcp_timing_get": "timing: reads the host's list",
    "vcp_selftest_poison": "the instrument itself",
    "vcp_selftest_scan_generation": "sets a host counter; test_workspace_poison_gpu.py runs the wrap it reaches",
}

# what vcp_selftest_poison leaves alone (k_poison_left_alone in csrc/vcp_ctx.hip), name for name
LEFT_ALONE = {
    "b_scan_tmp": "the scan's ticket and generation-stamped descriptors: the look-back of k_scan spins on them, the ticket "
                  "orders the tiles; zero-filled by the driver on fresh memory only",
    "b_outcur": "the output partition's window cursors: zero between calls by design (k_out_write leaves them so), "
                "zero-filled by the driver on fresh memory only; k_out_scatter places records from them",
}


def _header():
    with open(os.path.join(ROOT, "include", "vcp.h")) as f:
        src = f.read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return re.sub(r"//[^\n]*", "", src)


def context_functions(src=None):
    """Every function of vcp.h whose first parameter is a vcp_ctx* or a vcp_multi*."""
    src = _header() if src is None else src
    return sorted(set(re.findall(r"\b(vcp_[a-z0-9_]+)\s*\(\s*(?:const\s+)?vcp_(?:ctx|multi)\s*\*", src)))


def missing(cases, exempt):
    named = set()
    for c in cases:
        named |= set(c.funcs)
    return [f for f in context_functions() if f not in named and f not in exempt]


def left_alone_in_source():
    """{member: comment} of the array k_poison_left_alone in csrc/vcp_ctx.hip."""
    with open(os.path.join(ROOT, "vtkcloudpoint_amd", "csrc", "vcp_ctx.hip")) as f:
        src = f.read()
    m = re.search(r"k_poison_left_alone\[\]\s*=\s*\{(.*?)\n\};", src, flags=re.S)
    assert m, "k_poison_left_alone not found"
    entries = re.findall(r"&vcp_ctx::(b_\w+)\s*,?[ \t]*(?://[ \t]*([^\n]*))?", m.group(1))
    assert len(entries) == m.group(1).count("&vcp_ctx::")
    return {name: why.strip() for name, why in entries}


def test_every_context_entry_point_has_a_case_or_an_exemption():
    funcs = context_functions()
    assert len(funcs) >= 97 and "vcp_dbscan_dev" in funcs and "vcp_dbscan_blocks_multi" in funcs and "vcp_last_error" in funcs
    assert "vcp_version" not in funcs and "vcp_selftest_horn" not in funcs          # no context: host only
    assert missing(P.CASES, EXEMPT) == []
    named = {f for c in P.CASES for f in c.funcs}
    assert not named & set(EXEMPT), "exempt and named: %s" % sorted(named & set(EXEMPT))
    assert all(EXEMPT.values())
    with open(os.path.join(ROOT, "include", "vcp.h")) as f:
        declared = set(re.findall(r"\b(vcp_[a-z0-9_]+)\s*\(", f.read()))
    assert named <= declared and set(EXEMPT) <= declared, sorted((named | set(EXEMPT)) - declared)


def test_the_coverage_check_notices_a_missing_case():
    """The mutation the issue asks for, kept: without any one family of cases the check names what is left uncovered."""
    for prefix, lost in (("text/parse", "vcp_parse_scan_text"), ("icp_run/vtklike", "vcp_icp_vtklike"),
                         ("selftest/wave", "vcp_selftest_wave_dev"), ("blocks/tracked_split/multi", "vcp_dbscan_blocks_multi")):
        rest = [c for c in P.CASES if not c.name.startswith(prefix)]
        assert len(rest) < len(P.CASES) and lost in missing(rest, EXEMPT), prefix
    assert "vcp_set_stream" in missing(P.CASES, {k: v for k, v in EXEMPT.items() if k != "vcp_set_stream"})


def test_left_alone_array_is_the_table():
    src = left_alone_in_source()
    assert sorted(src) == sorted(LEFT_ALONE), (sorted(src), sorted(LEFT_ALONE))
    assert all(len(why) > 20 for why in src.values()), "every entry of k_poison_left_alone carries its reason"
    assert all(LEFT_ALONE.values())
    with open(os.path.join(ROOT, "vtkcloudpoint_amd", "csrc", "vcp_ctx.hpp")) as f:
        hpp = f.read()
    for name in src:
        assert re.search(r"\b%s\b" % name, hpp), name


def _same(a, b, where):
    if isinstance(a, dict):
        assert isinstance(b, dict) and list(a) == list(b), where
        for k in a:
            _same(a[k], b[k], where + (k,))
    elif isinstance(a, (list, tuple)):
        assert type(a) is type(b) and len(a) == len(b), where
        for k, (x, y) in enumerate(zip(a, b)):
            _same(x, y, where + (k,))
    elif isinstance(a, np.ndarray):
        assert isinstance(b, np.ndarray) and a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), where
    elif isinstance(a, float):
        assert isinstance(b, float) and (a == b or (a != a and b != b)), where
    elif callable(a):
        assert callable(b), where
    else:
        assert a == b, where


def test_the_table_is_deterministic():
    """Two tables built independently name the same cases and give the same inputs, bit for bit (the query families' lists
    carry their references, which are compared with them)."""
    again = P.build_cases()
    assert [c.name for c in again] == [c.name for c in P.CASES] and len(again) > 400
    assert [c.funcs for c in again] == [c.funcs for c in P.CASES]
    for a, b in zip(P.CASES, again):
        _same(a.inputs(), b.inputs(), (a.name,))
