"""The C-ABI library on a CPU-only box: it loads, exports every symbol include/vcp.h declares, and fails
loudly (no CPU fallback) when there is no GPU.  No compute calls here."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    with open(os.path.join(ROOT, "include", "vcp.h")) as f:
        src = f.read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(vcp_[a-z0-9_]+)\s*\(", src)))


def test_library_exports_every_declared_symbol():
    from vtkcloudpoint_amd import _native
    lib = _native.lib()
    decl = _declared()
    assert len(decl) >= 25
    missing = [s for s in decl if not hasattr(lib, s)]
    assert not missing, missing
    assert sorted(_native.SYMBOLS) == decl  # the Python binding's list tracks the header
    assert lib.vcp_version() == 1


def test_no_silent_cpu_fallback():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from vtkcloudpoint_amd import _native
    with pytest.raises(_native.VcpError) as e:
        _native.Context(0)
    assert e.value.code == -6  # VCP_ERR_NO_DEVICE
    assert "no CPU fallback" in str(e.value)


def test_product_does_not_import_the_oracle():
    """oracle/ is test infrastructure: nothing under vtkcloudpoint_amd/ may reference it."""
    pkg = os.path.join(ROOT, "vtkcloudpoint_amd")
    for dp, _, files in os.walk(pkg):
        for fn in files:
            if fn.endswith((".py", ".hip", ".hpp", ".cpp", ".h")):
                with open(os.path.join(dp, fn), errors="ignore") as f:
                    text = f.read()
                assert not re.search(r"^\s*(from|import)\s+oracle\b", text, flags=re.M), fn
                assert "vcp_oracle" not in text and "libvcp_oracle" not in text, fn
    with open(os.path.join(ROOT, "vtkcloudpoint_amd", "csrc", "Makefile")) as f:
        assert "oracle" not in f.read()


def test_horn_step_cold_start_on_a_nan_or_garbage_basis():
    """The Horn step of vcp_icp (host run of the same __host__ __device__ source, no device needed): a warm-start basis
    full of NaN, or one that is not orthonormal, must take the cold-start path -- fmax() would have dropped the NaN."""
    import numpy as np
    from vtkcloudpoint_amd import _native
    lib = _native.lib()
    rng = np.random.default_rng(5)
    P = rng.uniform(-3, 3, (500, 3))
    a = 0.4
    Rz = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1.0]])
    Y = P @ Rz.T + np.array([0.5, -1.0, 2.0])
    sums = np.concatenate([P.sum(0), Y.sum(0), (P[:, :, None] * Y[:, None, :]).sum(0).reshape(9), [0.0]])

    def solve(V, use):
        R, T = np.zeros(9), np.zeros(3)
        Vb = None if V is None else np.ascontiguousarray(V, np.float64).reshape(16).copy()
        rc = lib.vcp_selftest_horn(sums.ctypes.data_as(C.c_void_p), C.c_int64(len(P)),
                                   None if Vb is None else Vb.ctypes.data_as(C.c_void_p), C.c_int(use),
                                   R.ctypes.data_as(C.c_void_p), T.ctypes.data_as(C.c_void_p))
        assert rc == 1
        return R.reshape(3, 3), T, Vb

    R0, T0, _ = solve(None, 0)
    assert np.allclose(R0, Rz, atol=1e-12) and np.allclose(T0, [0.5, -1.0, 2.0], atol=1e-12)
    Rc, Tc, Vc = solve(np.eye(4), 1)             # identity basis = the cold start, bit for bit
    assert np.array_equal(Rc, R0) and np.array_equal(Tc, T0)
    for bad in (np.full((4, 4), np.nan), rng.uniform(-1, 1, (4, 4)), np.eye(4) * 2.0):
        Rb, Tb, Vb = solve(bad, 1)
        assert np.array_equal(Rb, R0) and np.array_equal(Tb, T0)
        assert np.array_equal(Vb, Vc)             # the basis stored back is the cold start's
    Rw, Tw, _ = solve(Vc.reshape(4, 4), 1)        # a good basis: warm start, same answer to rounding
    assert np.allclose(Rw, R0, atol=1e-12) and np.allclose(Tw, T0, atol=1e-12)


def test_block_range_plan_for_2_3_8_ranks():
    """vcp_blocks_share_plan (host arithmetic behind vcp_blocks_share and vcp_dbscan_blocks_multi): contiguous ranges that
    cover every block once, cut at the first block whose first position reaches m * r / world, balanced on points."""
    import numpy as np
    from vtkcloudpoint_amd import _native
    rng = np.random.default_rng(11)
    for trial in range(200):
        nb = int(rng.integers(1, 400))
        sizes = rng.integers(0, 50, nb)
        if trial % 5 == 0:
            sizes[rng.integers(0, nb)] = 5000  # one block that dwarfs the rest
        if trial % 7 == 0:
            sizes[:] = 0
        heavy = trial % 3 == 1 and nb > 1
        if heavy:  # the last bucket (the points in no block) holds more than any rank's fair share
            sizes[-1] = 10 * int(sizes[:-1].sum()) + 100
        bs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint32)
        m = int(bs[-1])
        for world in (1, 2, 3, 8):
            cuts = _native.blocks_share_plan(bs, world)
            assert cuts[0] == 0 and cuts[-1] == nb and np.all(np.diff(cuts) >= 0)
            for r in range(1, world):
                target = (m * r) // world
                want = int(np.searchsorted(bs[:nb], target, side="left"))
                assert cuts[r] == max(want, cuts[r - 1])
            if m > 0 and sizes.max() > 0:
                share = np.diff(bs[cuts].astype(np.int64))
                assert share.sum() == m
                assert share.max() <= m / world + sizes.max()  # never worse than one block over the fair share
            if heavy and world > 1:  # the ranks behind the heavy bucket get the empty share [nb, nb)
                assert all(cuts[r] == nb for r in range(1, world)), (trial, world, cuts)
                assert cuts[world - 1] == nb


# ---- the C# and Python bindings against the header -------------------------------------------------------------------
# A parameter's width class is what the calling convention passes: a 32-bit integer, a 64-bit integer, a double or an
# address (pointers, arrays, C# out / ref / arrays / IntPtr).  A binding whose arity or classes differ from the header hands
# the library a register it never set, and the library may write through it.
_C_CLASS = {"int": "i32", "int32_t": "i32", "uint32_t": "i32", "unsigned": "i32", "int64_t": "i64", "uint64_t": "i64",
            "double": "f64"}
_CS_CLASS = {"int": "i32", "uint": "i32", "long": "i64", "ulong": "i64", "double": "f64", "IntPtr": "ptr"}


def _header_prototypes():
    with open(os.path.join(ROOT, "include", "vcp.h")) as f:
        src = f.read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    src = re.sub(r"//[^\n]*", "", src)
    src = re.sub(r"^\s*#[^\n]*", "", src, flags=re.M)
    protos = {}
    for stmt in src.replace("{", ";").replace("}", ";").split(";"):
        m = re.search(r"\b(vcp_[a-z0-9_]+)\s*\(([^()]*)\)\s*$", stmt, re.S)
        if not m:
            continue
        name, params = m.group(1), " ".join(m.group(2).split())
        classes = []
        if params not in ("", "void"):
            for p in params.split(","):
                p = p.strip()
                if "*" in p or "[" in p:
                    classes.append("ptr")
                    continue
                words = [w for w in p.split() if w != "const"]
                assert len(words) == 2 and words[0] in _C_CLASS, (name, p)
                classes.append(_C_CLASS[words[0]])
        assert name not in protos, name
        protos[name] = classes
    return protos


def _csharp_imports():
    imports = []
    d = os.path.join(ROOT, "vtkcloudpoint_amd", "host", "csharp")
    for fn in sorted(os.listdir(d)):
        if not fn.endswith(".cs"):
            continue
        with open(os.path.join(d, fn)) as f:
            src = f.read()
        n_dll = len(re.findall(r"\[DllImport\b", src))
        found = re.findall(r"\[DllImport\b[^\]]*\]\s*(?:(?:public|internal|private|static|unsafe)\s+)*extern\s+[\w\[\]]+\s+"
                           r"(\w+)\s*\(([^)]*)\)\s*;", src, re.S)
        assert len(found) == n_dll, "%s: %d DllImports, %d parsed" % (fn, n_dll, len(found))
        for name, params in found:
            classes = []
            for p in " ".join(params.split()).split(","):
                p = p.strip()
                if not p:
                    continue
                words = [w for w in p.split() if not w.startswith("[")]
                if words[0] in ("out", "ref") or words[0].endswith("[]") or words[0] == "string":
                    classes.append("ptr")
                else:
                    assert len(words) == 2 and words[0] in _CS_CLASS, (fn, name, p)
                    classes.append(_CS_CLASS[words[0]])
            imports.append((fn, name, classes))
    return imports


def test_csharp_dllimports_match_the_header():
    """Every DllImport in host/csharp/*.cs names a vcp.h function and passes the header's parameters: the same count,
    each of the same width class."""
    protos = _header_prototypes()
    assert len(protos) >= 25 and protos["vcp_blocks_finish_zero_dev"] == ["ptr", "i32", "ptr", "ptr"]
    imports = _csharp_imports()
    assert len(imports) >= 40
    bad = []
    for fn, name, classes in imports:
        if name not in protos:
            bad.append("%s: %s is not in vcp.h" % (fn, name))
        elif classes != protos[name]:
            bad.append("%s: %s(%s), vcp.h has (%s)" % (fn, name, ", ".join(classes), ", ".join(protos[name])))
    assert not bad, "\n".join(bad)


def test_python_binding_calls_pass_the_header_arity():
    """Every lib().vcp_*(...) call in _native.py passes as many arguments as the vcp.h prototype has parameters."""
    import ast
    protos = _header_prototypes()
    with open(os.path.join(ROOT, "vtkcloudpoint_amd", "_native.py")) as f:
        tree = ast.parse(f.read())
    calls = []
    for node in ast.walk(tree):
        if not (isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute)):
            continue
        base = node.func.value
        if not (isinstance(base, ast.Call) and isinstance(base.func, ast.Name) and base.func.id == "lib"):
            continue
        name = node.func.attr
        assert name in protos, "%s (line %d) is not in vcp.h" % (name, node.lineno)
        assert not node.keywords and not any(isinstance(a, ast.Starred) for a in node.args), name
        calls.append((name, node.lineno, len(node.args)))
    assert len(calls) >= 50
    bad = ["%s (line %d): %d arguments, vcp.h has %d" % (nm, ln, k, len(protos[nm]))
           for nm, ln, k in calls if k != len(protos[nm])]
    assert not bad, "\n".join(bad)


def test_kernels_launch_only_through_vcp_launch():
    """Every kernel launch in the library goes through VCP_LAUNCH (csrc/vcp_ctx.hpp), which refuses a dispatch the runtime
    would wrap and names the kernel of a launch that fails.  Its definition is the one place that calls the launch API."""
    csrc = os.path.join(ROOT, "vtkcloudpoint_amd", "csrc")
    raw = re.compile(r"hipLaunchKernel|<<<|hipModuleLaunchKernel|hipExtLaunchKernel")
    launcher = re.compile(r"^#define VCP_LAUNCH\(.*?[^\\]\n", flags=re.M | re.S)
    bad, uses = [], 0
    for fn in sorted(os.listdir(csrc)):
        if not fn.endswith((".hip", ".hpp")):
            continue
        with open(os.path.join(csrc, fn)) as f:
            text = f.read()
        if fn == "vcp_ctx.hpp":
            defs = launcher.findall(text)
            assert len(defs) == 1 and len(raw.findall(defs[0])) == 1, "the definition of VCP_LAUNCH"
            text = launcher.sub(lambda m: "\n" * m.group(0).count("\n"), text)
        uses += len(re.findall(r"\bVCP_LAUNCH\(ctx, ", text))
        bad += ["%s:%d" % (fn, text.count("\n", 0, m.start()) + 1) for m in raw.finditer(text)]
    assert not bad, "launches outside VCP_LAUNCH: " + ", ".join(bad)
    assert uses >= 100
