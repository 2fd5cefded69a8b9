"""Host side of the radiance along rays (pupil_pt_radiance_rays / _radiance_info): the symbols, the
ctypes mirror against the header, the argument check that needs no device, and PTPass.radiance's
validation, which refuses a bad call before the library is reached.  No GPU."""
import ctypes as C
import os
import re
import subprocess

import pytest

from pupiloptixlab_amd import abi, pt_pass

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "pupil_pt.h")
ENTRIES = ("pupil_pt_radiance_rays", "pupil_pt_radiance_info")

C_TYPES = {"pupil_pt *": C.c_void_p, "uint32_t": C.c_uint32, "const void *": C.c_void_p, "void *": C.c_void_p,
           "const uint32_t *": C.c_void_p, "const pupil_pt_launch *": C.POINTER(abi.Launch),
           "const pupil_ray_radiance *": C.POINTER(abi.RayRadiance), "uint64_t *": C.POINTER(C.c_uint64),
           "double *": C.POINTER(C.c_double)}


def _declaration(name):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
    assert m, name
    params = []
    for p in m.group(1).split(","):
        p = " ".join(p.split())
        params.append(re.match(r"(.*?)(\w+)$", p).group(1).strip())  # drop the parameter's name
    return params


def test_symbols_exist_and_the_abi_version_stays():
    lib = abi.load_library()
    for name in ENTRIES:
        assert hasattr(lib, name), name
        assert name in abi.SIGNATURES
    assert lib.pupil_abi_version() == 7


@pytest.mark.parametrize("name", ENTRIES)
def test_signatures_match_the_header(name):
    res, args = abi.SIGNATURES[name]
    assert res is C.c_int
    declared = _declaration(name)
    assert len(declared) == len(args), (declared, args)
    for ctype, arg in zip(declared, args):
        assert C_TYPES[ctype] is arg or C_TYPES[ctype] == arg, (name, ctype, arg)


def test_ray_radiance_layout_matches_c(tmp_path):
    assert C.sizeof(abi.RayRadiance) == 24
    fields = [f for f, _ in abi.RayRadiance._fields_]
    assert fields == ["radiance", "albedo", "normal"]
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "pupil_pt.h"\nint main(void) {\n'
                   '  printf("%zu", sizeof(pupil_ray_radiance));\n'
                   + "".join(f'  printf(" %zu", offsetof(pupil_ray_radiance, {f}));\n' for f in fields)
                   + '  printf("\\n");\n  return 0;\n}\n')
    exe = tmp_path / "probe"
    subprocess.run(["cc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got[0] == C.sizeof(abi.RayRadiance)
    assert got[1:] == [getattr(abi.RayRadiance, f).offset for f in fields]
    assert tuple(pt_pass.RADIANCE_OUTPUTS) == tuple(fields)


def test_a_null_engine_is_refused():
    lib = abi.load_library()
    la = abi.Launch()
    la.spp = 1
    out = abi.RayRadiance()
    assert lib.pupil_pt_radiance_rays(None, 0, None, None, C.byref(la), C.byref(out), None) == abi.ERR_INVALID
    assert lib.pupil_last_error()
    assert lib.pupil_pt_radiance_info(None, None, None, None, None, None, None) == abi.ERR_INVALID


class _NoLibrary:
    """Stands where the library would: any entry a test reaches is a failure."""

    def __getattr__(self, name):
        raise AssertionError(f"the library was called ({name})")


def _bare_pass():
    import torch

    pt = pt_pass.PTPass.__new__(pt_pass.PTPass)  # no device: only what radiance() validates with
    pt._torch = torch
    pt._lib = _NoLibrary()
    pt._pt = C.c_void_p(1)
    pt.device_index = 0
    pt.device = "cuda:0"
    return pt


def test_radiance_refuses_bad_rays_before_any_native_call():
    import torch

    pt = _bare_pass()
    try:
        cases = {
            "a CPU tensor": (torch.zeros((4, 8), dtype=torch.float32), r"needs rays on cuda:0, got a cpu tensor"),
            "float64": (torch.zeros((4, 8), dtype=torch.float64), r"needs float32 rays, got torch\.float64"),
            "shape (n, 6)": (torch.zeros((4, 6), dtype=torch.float32), r"needs an \(n, 8\) tensor of rays, got \(4, 6\)"),
            "a non-contiguous view": (torch.zeros((4, 16), dtype=torch.float32)[:, ::2], r"needs contiguous rays"),
            "not a tensor": ([[0.0] * 8], r"needs a torch tensor"),
        }
        for what, (rays, message) in cases.items():
            with pytest.raises(ValueError, match=message):
                pt.radiance(rays)
    finally:
        pt._pt = C.c_void_p()  # nothing for __del__ to destroy
