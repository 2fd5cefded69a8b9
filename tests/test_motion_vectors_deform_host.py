"""Flow for deforming meshes, host side (no GPU): the two snapshot entry points are declared,
exported and bound, validate a null engine, and the C++ pass carries its switch."""
import os
import re
import subprocess

from pupiloptixlab_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("pupil_pt_snapshot_shape_vertices", "pupil_pt_clear_vertex_snapshots")


def test_new_entries_are_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "pupil_pt.h")).read()
    for name in NEW:
        assert re.search(r"\bint\s+" + name + r"\s*\(\s*pupil_pt\s*\*", header), name
        assert name in abi.SIGNATURES, name
    assert abi.SIGNATURES[NEW[0]][1][1:] == [abi.C.c_uint32] and len(abi.SIGNATURES[NEW[1]][1]) == 1
    # no flag bit, no ABI bump, no new counter: the entries are detected by symbol
    assert re.search(r"#define\s+PUPIL_VERTS_DEVICE\s+1u", header) and re.search(r"#define\s+PUPIL_VERTS_REBUILD\s+2u", header)
    assert abi.Counters._fields_[-1][0] == "hidden_instances"
    assert "does not see vertex" not in header and "only rigid instance motion is covered" not in header


def test_library_exports_the_new_entries():
    lib = abi.load_library()
    assert lib.pupil_abi_version() == 7
    for name in NEW:
        assert hasattr(lib, name), name
    out = subprocess.run(["nm", "-D", "--defined-only", abi.LIB_PATH], capture_output=True, text=True).stdout
    assert set(NEW) <= set(re.findall(r" T (pupil_\w+)", out))


def test_null_engine_is_invalid_and_sets_the_error():
    lib = abi.load_library()
    for call in (lambda: lib.pupil_pt_snapshot_shape_vertices(None, 0), lambda: lib.pupil_pt_clear_vertex_snapshots(None)):
        lib.pupil_pt_local_pixels(0, 0, 0, 0, 0, None, None)  # leaves another message behind
        before = lib.pupil_last_error()
        assert call() == abi.ERR_INVALID
        msg = lib.pupil_last_error()
        assert msg and msg != before and b"null" in msg


def test_framework_exports_the_switch():
    lib = os.path.join(os.path.dirname(abi.LIB_PATH), "libpupil_framework.so")
    out = subprocess.run(["nm", "-DC", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    assert "Pupil::pt::PTPass::SetKeepPreviousVertices(bool)" in out
