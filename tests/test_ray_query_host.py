"""Host side of the ray queries (pupil_pt_query_rays / _query_camera / _query_info): the symbols, the
ctypes mirror against the header, and PTPass.trace's validation, which refuses a bad ray tensor
before the library is called.  No GPU."""
import ctypes as C
import os
import re
import subprocess

import pytest

from pupiloptixlab_amd import abi, pt_pass

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "pupil_pt.h")
ENTRIES = ("pupil_pt_query_rays", "pupil_pt_query_camera", "pupil_pt_query_info")

C_TYPES = {"pupil_pt *": C.c_void_p, "uint32_t": C.c_uint32, "const void *": C.c_void_p, "void *": C.c_void_p,
           "const pupil_ray_hits *": C.POINTER(abi.RayHits), "float": C.c_float, "uint64_t *": C.POINTER(C.c_uint64),
           "double *": C.POINTER(C.c_double)}


def _declaration(name):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
    assert m, name
    params = []
    for p in m.group(1).split(","):
        p = " ".join(p.split())
        ctype = re.match(r"(.*?)(\w+)$", p).group(1).strip()  # drop the parameter's name
        params.append(ctype)
    return params


def test_symbols_exist_and_the_abi_version_stays():
    lib = abi.load_library()
    for name in ENTRIES:
        assert hasattr(lib, name), name
        assert name in abi.SIGNATURES
    assert lib.pupil_abi_version() == 7
    assert abi.QUERY_ANY_HIT == 1


@pytest.mark.parametrize("name", ENTRIES)
def test_signatures_match_the_header(name):
    res, args = abi.SIGNATURES[name]
    assert res is C.c_int
    declared = _declaration(name)
    assert len(declared) == len(args), (declared, args)
    for ctype, arg in zip(declared, args):
        assert C_TYPES[ctype] is arg or C_TYPES[ctype] == arg, (name, ctype, arg)


def test_ray_hits_layout_matches_c(tmp_path):
    fields = [f for f, _ in abi.RayHits._fields_]
    assert fields == ["hit", "instance", "primitive", "material", "position", "normal", "texcoord"]
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "pupil_pt.h"\nint main(void) {\n'
                   '  printf("%zu", sizeof(pupil_ray_hits));\n'
                   + "".join(f'  printf(" %zu", offsetof(pupil_ray_hits, {f}));\n' for f in fields)
                   + '  printf(" %d\\n", (int)PUPIL_QUERY_ANY_HIT);\n  return 0;\n}\n')
    exe = tmp_path / "probe"
    subprocess.run(["cc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got[0] == C.sizeof(abi.RayHits)
    assert got[1:-1] == [getattr(abi.RayHits, f).offset for f in fields]
    assert got[-1] == abi.QUERY_ANY_HIT
    assert tuple(pt_pass.QUERY_OUTPUTS) == tuple(fields)


class _NoLibrary:
    """Stands where the library would: any entry a test reaches is a failure."""

    def __getattr__(self, name):
        raise AssertionError(f"the library was called ({name})")


def _bare_pass():
    import torch

    pt = pt_pass.PTPass.__new__(pt_pass.PTPass)  # no device: only what trace() validates with
    pt._torch = torch
    pt._lib = _NoLibrary()
    pt._pt = C.c_void_p(1)
    pt.device_index = 0
    pt.device = "cuda:0"
    return pt


def test_trace_refuses_bad_rays_before_any_native_call():
    import torch

    pt = _bare_pass()
    try:
        # each case is wrong in one way only (but for living on the CPU, which is checked last),
        # and is refused by the check that names it
        cases = {
            "a CPU tensor": (torch.zeros((4, 8), dtype=torch.float32), r"needs rays on cuda:0, got a cpu tensor"),
            "float64": (torch.zeros((4, 8), dtype=torch.float64), r"needs float32 rays, got torch\.float64"),
            "shape (n, 7)": (torch.zeros((4, 7), dtype=torch.float32), r"needs an \(n, 8\) tensor of rays, got \(4, 7\)"),
            "one dimension": (torch.zeros(32, dtype=torch.float32), r"needs an \(n, 8\) tensor of rays, got \(32,\)"),
            "a non-contiguous view": (torch.zeros((4, 16), dtype=torch.float32)[:, ::2], r"needs contiguous rays"),
            "not a tensor": ([[0.0] * 8], r"needs a torch tensor"),
        }
        view = cases["a non-contiguous view"][0]
        assert not view.is_contiguous() and tuple(view.shape) == (4, 8)
        for what, (rays, message) in cases.items():
            with pytest.raises(ValueError, match=message):
                pt.trace(rays)
            with pytest.raises(ValueError, match=message):
                pt.trace(rays, any_hit=True, want=("hit",))
    finally:
        pt._pt = C.c_void_p()  # nothing for __del__ to destroy


def test_camera_ray_restates_the_pixel_centre():
    """pt_pass.camera_ray (what pick() traces): a unit direction through the film point, from the
    camera's origin, over the camera-ray interval."""
    import numpy as np

    s2c = np.array([[0.5, 0, 0, -0.25], [0, 0.5, 0, -0.25], [0, 0, 0, 1], [0, 0, 0, 1]], np.float32)
    c2w = np.array([[1, 0, 0, 2], [0, 1, 0, 3], [0, 0, 1, 4], [0, 0, 0, 1]], np.float32)
    r = pt_pass.camera_ray(s2c, c2w, 8, 8, 4, 4, jitter=(0.0, 0.0))
    assert r.dtype == np.float32 and r.shape == (8,)
    assert list(r[0:3]) == [2.0, 3.0, 4.0]
    assert list(r[3:6]) == [0.0, 0.0, 1.0]  # film (0.5, 0.5) is this camera's axis
    assert r[6] == np.float32(0.001) and r[7] == np.float32(1e16)
    off = pt_pass.camera_ray(s2c, c2w, 8, 8, 7, 4)
    assert off[3] > 0 and off[4] > 0 and abs(float(np.linalg.norm(off[3:6].astype(np.float64))) - 1) < 1e-6
