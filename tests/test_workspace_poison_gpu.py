"""Every entry point's results under an overwritten workspace.  A vcp_ctx keeps about a hundred growable device buffers, a
pinned scratch and a pinned staging area between calls, and every entry point promises that its result does not depend on
what an earlier call left there.  Here vcp_selftest_poison fills all of it (but the buffers that carry state by design)
with a known 32-bit word before each call of the case table (tests/poison_cases.py), and every output is compared with the
entry point's own reference.  A kernel that reads a counter, a flag, a cursor or a partial sum it did not write in this call
gives a wrong answer deterministically, whichever call ran before; while the context is armed, fresh allocations are filled
too, so memory the runtime happens to hand back zeroed hides nothing.

Per case: the check unpoisoned (the case itself is sound), then under 0x00000000, 0x00000001 and 0xFFFFFFFF in that order.
The first two stay inside every buffer when read as an index, a count or a flag; the third is NaN as a float or a double,
-1 as an int32 and UINT_MAX as a cursor, the one that shows a stale term in a floating-point sum, and it runs only after
the first two have passed: a stale read used as an address is a wrong answer before it can become a bad access.

The module has a context of its own; the session's is never armed."""
import os
import re

import numpy as np
import pytest

import poison_cases as P
from vtkcloudpoint_amd import _native as N

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORDS = (0x00000000, 0x00000001, 0xFFFFFFFF)

# The DevBuf members of vcp_ctx that the library's sources name: 104.  Two are left alone (tests/test_poison_cases.py);
# two more exist only for grids of more than 8192 buckets of 2^14 cells (k_part_split, csrc/gridbuild.hip: clouds of several
# million points, tests/test_full_size_gpu.py), which no small shape reaches.
NAMED_BUFFERS = 104
NOT_REACHED = {"b_rec2": "k_part_split: more than 8192 buckets", "b_bstart": "k_part_split: more than 8192 buckets"}
LEFT_ALONE = ("b_scan_tmp", "b_outcur")

_state = dict(ctx=None, first=None, most=0, ran=0, fatal=None)


@pytest.fixture(scope="module")
def ctx():
    c = N.Context(0)
    _state["ctx"] = c
    yield c
    c.selftest_poison(0, armed=False)
    P.close_extras()
    c.close()


def test_named_buffers_are_counted_from_the_sources():
    csrc = os.path.join(ROOT, "vtkcloudpoint_amd", "csrc")
    with open(os.path.join(csrc, "vcp_ctx.hpp")) as f:
        decl = re.findall(r"^\s*DevBuf\s+([^;]+);", f.read(), flags=re.M)
    members = [m.strip() for d in decl for m in d.split(",")]
    assert all(re.fullmatch(r"b_\w+", m) for m in members), members
    text = ""
    for fn in sorted(os.listdir(csrc)):
        if fn.endswith((".hip", ".hpp")) and fn != "vcp_ctx.hpp":
            with open(os.path.join(csrc, fn)) as f:
                text += f.read()
    named = [m for m in members if re.search(r"\b%s\b" % m, text)]
    assert len(named) == NAMED_BUFFERS == len(members)
    assert set(NOT_REACHED) | set(LEFT_ALONE) <= set(named)


@pytest.mark.parametrize("name", [c.name for c in P.CASES])
def test_case_under_every_word(ctx, name):
    if _state["fatal"]:                                  # the device reported an error: nothing more runs on it from here
        pytest.fail("not started: " + _state["fatal"])
    case = P.BY_NAME[name]
    try:
        case.check(ctx)                                  # unpoisoned: the case is sound
        for word in WORDS:                               # 0xFFFFFFFF only after 0 and 1 have passed
            nbytes, nbufs = ctx.selftest_poison(word)
            if _state["first"] is None:
                _state["first"] = (case, nbytes, nbufs)
            _state["most"] = max(_state["most"], nbufs)
            try:
                case.check(ctx, lambda c, w=word: c.selftest_poison(w))
            except AssertionError as e:
                raise AssertionError("under the word 0x%08X: %s" % (word, e)) from e
    except AssertionError as e:                          # a wrong answer; fuzz_queries reports a refusal it did not expect
        if "VCP_ERR_HIP" in str(e):                      # this way too, the device's own error (-7) included
            _state["fatal"] = "%s ended with %s" % (name, " ".join(str(e).split())[:300])
        raise
    except BaseException as e:                           # VcpError, a torch RuntimeError, ...: nothing more runs on the device
        _state["fatal"] = "%s ended with %s: %s" % (name, type(e).__name__, " ".join(str(e).split())[:300])
        raise
    _state["ran"] += 1


def _input_bytes(x):
    if isinstance(x, dict):
        return sum(_input_bytes(v) for v in x.values())
    if isinstance(x, (list, tuple)):
        return sum(_input_bytes(v) for v in x)
    return x.nbytes if isinstance(x, np.ndarray) else len(x) if isinstance(x, (bytes, bytearray)) else 0


def test_the_fill_is_not_vacuous(ctx):
    """After the first case the hook has filled device buffers, at least the input's size of device memory (the hook
    does not count the pinned areas); over the module the buffers it fills
    grow to every DevBuf member the sources name but the four excepted above.  (The list of a context only grows, so the
    largest count is the size of the union.)"""
    if _state["ran"] < len(P.CASES):
        pytest.fail("needs the whole case table: %d of %d cases ran" % (_state["ran"], len(P.CASES)))
    case, nbytes, nbufs = _state["first"]
    assert nbufs > 0 and nbytes >= _input_bytes(case.inputs()) > 0, (case.name, nbytes, nbufs)
    _, nbufs = ctx.selftest_poison(WORDS[0])
    print("buffers filled at the end: %d" % nbufs)
    assert max(nbufs, _state["most"]) >= NAMED_BUFFERS - len(LEFT_ALONE) - len(NOT_REACHED)


def test_scan_generation_wrap(ctx):
    """The 30-bit generation of the scan's descriptors wraps after 2^30 scans (memset, restart at 1): set it four short of
    the wrap and scan eight times, four tiles each, so that the look-back crosses it; each call is a sum and a maximum
    scan, exact against numpy.  The calls after the third run on the zero-filled descriptors and the restarted count."""
    import torch
    if _state["fatal"]:
        pytest.fail("not started: " + _state["fatal"])
    ctx.selftest_poison(0, armed=False)
    rng = np.random.default_rng(30)
    n = P.SCAN_N
    d_out = torch.zeros(n, dtype=torch.int32, device="cuda")
    first = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    P.check_scan(ctx, first, torch.from_numpy(first.view(np.int32)).cuda(), d_out, P.scan_reference(first))
    ctx.selftest_scan_generation(0x3FFFFFFC)
    for k in range(8):
        v = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
        if k % 2:
            v[:] = 0xFFFFFFFF                            # every partial sum wraps
        try:
            P.check_scan(ctx, v, torch.from_numpy(v.view(np.int32)).cuda(), d_out, P.scan_reference(v))
        except AssertionError as e:
            raise AssertionError("scan %d after the generation was set: %s" % (2 * k, e)) from e
    with pytest.raises(N.VcpError) as e:
        ctx.selftest_scan_generation(0x40000000)
    assert e.value.code == -1
