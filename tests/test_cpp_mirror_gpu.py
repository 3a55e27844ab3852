"""Every member of the C++ host mirror (vtkcloudpoint_amd/host/cpp/vcp_host.hpp) and the vcp_dev_* path, on the GPU:
host_check is run once per test on the group's cases (tests/cpp_mirror_cases.py) and every field it wrote back is
compared with what the oracle and the numpy restatements say -- never with the library's own output.  Labels, flags,
counters, matching, shapes, centroids, k-distances, the eps tree, the registrations and gdbscan bit for bit; go_hell_ICP
within the 1e-5 of tests/test_icp_gpu.py on all of R and T."""
import os
import subprocess

import pytest

import cpp_mirror_cases as C
import vcpbin

pytestmark = pytest.mark.gpu

EXE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "vtkcloudpoint_amd", "host", "cpp", "host_check")


@pytest.mark.parametrize("group", sorted(C.GROUPS))
def test_cpp_mirror(group, oracle, tmp_path):
    assert os.path.exists(EXE), "run __graft_entry__.build() first"
    cases = C.GROUPS[group]()
    fin, fout = str(tmp_path / "cases.bin"), str(tmp_path / "results.bin")
    vcpbin.write(fin, (r for c in cases for r in c.records()))
    out = subprocess.run([EXE, fin, fout], capture_output=True, text=True, timeout=120)
    if out.returncode < 0 or out.returncode in (124, 134, 137, 139):   # the program died on the device: run nothing more on it
        pytest.exit("host_check ended with status %d on group %s\n%s" % (out.returncode, group, out.stdout + out.stderr), 3)
    assert out.returncode == 0 and "host_check: %d cases" % len(cases) in out.stdout, out.stdout + out.stderr
    res = vcpbin.read(fout)
    for c in cases:
        mine = {k[len(c.name) + 1:]: v for k, v in res.items() if k.startswith(c.name + "/")}
        assert "threw" in mine, c.name
        try:
            c.check(mine, oracle)
        except AssertionError as e:
            raise AssertionError("case %s (%s): %s" % (c.name, c.op, e)) from e
