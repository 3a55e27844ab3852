"""No GPU: the container host_check speaks round-trips every dtype bit for bit, and every public member of
vtkcloudpoint_amd/host/cpp/vcp_host.hpp has a case in tests/cpp_mirror_cases.py (a member added later without one fails
here)."""
import os

import numpy as np
import pytest

import cpp_mirror_cases as C
import vcpbin

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "vtkcloudpoint_amd", "host", "cpp", "vcp_host.hpp")


def test_container_round_trips_every_dtype_bit_for_bit(tmp_path):
    f = np.array([0x7FF8000000000000, 0x7FF8000000000123, 0xFFF4000000000001, 0x7FF0000000000000, 0xFFF0000000000000,
                  0x8000000000000000, 0x0000000000000000, 0x0000000000000001, 0x800FFFFFFFFFFFFF, 0x3FF0000000000001,
                  0x7FEFFFFFFFFFFFFF], np.uint64).view(np.float64)
    rec = [("a/f64", f), ("a/i32", np.array([-2 ** 31, -1, 0, 2 ** 31 - 1], np.int32)),
           ("a/i64", np.array([-2 ** 63, -1, 0, 2 ** 63 - 1], np.int64)), ("a/u8", np.arange(256, dtype=np.uint8)),
           ("a/op", "Tools::GetClusList"), ("empty/f64", np.zeros(0)), ("empty/i32", np.zeros(0, np.int32)),
           ("empty/i64", np.zeros(0, np.int64)), ("empty/u8", np.zeros(0, np.uint8)), ("flag", np.array([True, False])),
           ("shape", np.arange(6.0).reshape(2, 3)), ("big-endian", np.arange(3, dtype=">i4"))]
    path = tmp_path / "rt.bin"
    vcpbin.write(str(path), rec)
    got = vcpbin.read(str(path))
    assert list(got) == [k for k, _ in rec]                                   # file order
    assert np.array_equal(got["a/f64"].view(np.uint64), f.view(np.uint64))    # NaN payloads, -0.0, subnormals
    assert np.signbit(got["a/f64"][5]) and not np.signbit(got["a/f64"][6])
    for k, d in (("a/f64", np.float64), ("a/i32", np.int32), ("a/i64", np.int64), ("a/u8", np.uint8)):
        assert got[k].dtype == d and got["empty/" + k[2:]].dtype == d and got["empty/" + k[2:]].size == 0
    assert np.array_equal(got["a/i32"], rec[1][1]) and np.array_equal(got["a/i64"], rec[2][1])
    assert np.array_equal(got["a/u8"], rec[3][1]) and vcpbin.text(got["a/op"]) == "Tools::GetClusList"
    assert got["flag"].tolist() == [1, 0] and got["shape"].tolist() == [0, 1, 2, 3, 4, 5] and got["big-endian"].tolist() == [0, 1, 2]
    # a second trip changes no byte
    assert vcpbin.dumps(got.items()) == path.read_bytes()
    for bad in (np.zeros(2, np.float32), np.zeros(2, np.uint32), np.zeros(2, np.complex128), np.array(["x"])):
        with pytest.raises(TypeError):
            vcpbin.dumps([("bad", bad)])
    with pytest.raises(ValueError):
        vcpbin.loads(path.read_bytes() + b"\0")
    with pytest.raises(ValueError):
        vcpbin.loads(vcpbin.dumps([("twice", np.zeros(1)), ("twice", np.zeros(1))]))


def test_every_public_member_of_the_mirror_has_a_case():
    with open(HEADER) as f:
        members = C.header_members(f.read())
    # the parser sees the header: the members the issue of this suite lists are all there
    for m in ("DBImproved::dbscan", "DBImproved::dbscanGeneral", "vcp::gdbscan", "ICP::go_hell_ICP", "ICP::RegisterPairs",
              "ICP::RegisterSimilarity", "Tools::GetClusList", "Tools::MergeIDByDistance", "Tools::getRectangles",
              "Tools::removeFilterPointFromClustering", "getClusterFromMotor", "RecorrectMatchingPtsByDistance",
              "MatchOneToOne", "k_distance", "EpsTree", "EpsTreeResult::clustersAt", "Context::release_workspace"):
        assert m in members, m
    cases = C.all_cases()
    covered = set()
    for c in cases:
        covered.add(c.op)
        covered.update(C.ALSO.get(c.op, ()))
    assert [m for m in members if m not in covered] == []
    names = [c.name for c in cases]
    assert len(set(names)) == len(names)
    # every case is in a group a GPU test runs, and travels through the container
    blob = vcpbin.dumps(r for c in cases for r in c.records())
    back = vcpbin.loads(blob)
    assert sum(k.endswith("/op") for k in back) == len(cases)


def test_the_parser_finds_a_member_added_later():
    with open(HEADER) as f:
        text = f.read()
    more = text.replace("class ICP {", "class ICP {\n public:\n  std::vector<int> NewMember(const std::vector<Point3D*>& a, int k = 3) { return {}; }\n", 1)
    more = more.replace("inline BlockResult getClusterFromMotor(", "inline int newFree(Context& c) { return 0; }\ninline BlockResult getClusterFromMotor(", 1)
    assert set(C.header_members(more)) - set(C.header_members(text)) == {"ICP::NewMember", "newFree"}
