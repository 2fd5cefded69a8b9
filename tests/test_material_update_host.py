"""Material updates, host side: the new ABI entries exist with the right signatures,
pupil_world_set_material changes what pupil_world_get_desc reports (and nothing when it refuses),
and the oracle, which renders whatever the desc says, sees a world edited with set_material
exactly as a world built with that material from the start."""
import ctypes as C

import numpy as np

import oracle
from pupiloptixlab_amd import abi
from pupiloptixlab_amd import world as W

from material_cases import CUBE, FLOOR, SPHERE, SPP, base_materials, build_world, material_bytes, texels

EXPECTED = {
    "pupil_pt_update_materials": (C.c_int, [C.c_void_p, C.c_uint32, abi.u32p, C.POINTER(abi.Material)]),
    "pupil_pt_update_texture_device": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32,
                                                  C.c_void_p]),
    "pupil_pt_material_info": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_double)]),
    "pupil_debug_read_material": (C.c_int, [C.c_void_p, C.c_uint32, abi.u32p, abi.f32p]),
    "pupil_world_set_material": (C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(abi.Material)]),
}


def test_new_symbols_and_signatures():
    lib = abi.load_library()
    for name, (res, args) in EXPECTED.items():
        assert hasattr(lib, name), name
        assert abi.SIGNATURES[name] == (res, args), name
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args, name
    assert lib.pupil_abi_version() == 7  # no bump: the entries are detected by symbol
    # null engines are refused with a code, not a crash
    assert lib.pupil_pt_update_materials(None, 0, None, None) == abi.ERR_INVALID
    assert lib.pupil_pt_update_texture_device(None, 0, 0, None, 1, 1, None) == abi.ERR_INVALID
    assert lib.pupil_pt_material_info(None, None, None) == abi.ERR_INVALID
    assert lib.pupil_debug_read_material(None, 0, None, None) == abi.ERR_INVALID


def test_bitmap_texture_helper():
    t = texels(5, 3, 1)
    tex = W.bitmap(t, filter=0, uv_scale=(2.0, 3.0))
    assert (tex.type, tex.width, tex.height, tex.filter) == (abi.TEX_BITMAP, 5, 3, 0)
    assert tex.transform[0] == 2.0 and tex.transform[5] == 3.0
    m = W.diffuse(tex)
    del t, tex  # the material keeps the texel array alive
    got = np.ctypeslib.as_array(m.tex[0].rgba, shape=(3, 5, 4))
    assert np.array_equal(got, texels(5, 3, 1))


def test_set_material_shows_in_desc():
    w = build_world(base_materials())
    tx = texels(5, 3, 2)
    w.set_material(CUBE, W.rough_plastic(0.15, W.bitmap(tx, filter=0), (0.9, 0.8, 0.7), int_ior=1.6, nonlinear=True))
    d = w.desc()
    m = d.materials[CUBE]
    assert (m.type, m.nonlinear, m.twosided) == (abi.MAT_ROUGH_PLASTIC, 1, 0)
    assert m.int_ior == np.float32(1.6)
    assert list(m.tex[0].c0) == [np.float32(0.15)] * 3
    assert (m.tex[1].type, m.tex[1].width, m.tex[1].height, m.tex[1].filter) == (abi.TEX_BITMAP, 5, 3, 0)
    assert np.array_equal(np.ctypeslib.as_array(m.tex[1].rgba, shape=(3, 5, 4)), tx)
    assert list(m.tex[2].c0) == [np.float32(0.9), np.float32(0.8), np.float32(0.7)]
    # the other materials are the ones the world was built with
    ref = build_world(base_materials()).desc()
    for i in (SPHERE, FLOOR):
        assert d.materials[i].type == ref.materials[i].type
        assert list(d.materials[i].tex[0].c0) == list(ref.materials[i].tex[0].c0)


def test_oracle_sees_set_material_as_a_world_built_with_it():
    tx = texels(5, 3, 3)
    new = {SPHERE: lambda: W.twosided(W.diffuse(W.bitmap(tx, filter=1))),
           CUBE: lambda: W.rough_plastic(0.2, (0.2, 0.5, 0.3), 0.8)}
    w = build_world(base_materials())
    before = oracle.OracleScene(w.desc()).render(spp=SPP)
    for i, make in new.items():
        w.set_material(i, make())
    got = oracle.OracleScene(w.desc()).render(spp=SPP)
    mats = base_materials()
    for i, make in new.items():
        mats[i] = make()
    ref = oracle.OracleScene(build_world(mats).desc()).render(spp=SPP)
    for k in ("accum", "albedo", "normal", "test"):
        assert np.array_equal(got[k].view(np.uint32), ref[k].view(np.uint32)), k
    assert not np.array_equal(got["accum"], before["accum"])


def test_set_material_refusals_leave_the_desc():
    w = build_world(base_materials())
    lib = abi.load_library()
    before = material_bytes(w.desc())
    n = w.desc().num_materials
    good = W.diffuse((0.1, 0.2, 0.3))
    unknown = W.diffuse((0.1, 0.2, 0.3))
    unknown.tex[0].type = 3
    empty = W.diffuse((0.1, 0.2, 0.3))
    empty.tex[0].type = abi.TEX_BITMAP
    empty.tex[0].width = empty.tex[0].height = 2  # rgba stays NULL
    for material, m in ((n, good), (0xFFFFFFFF, good), (SPHERE, unknown), (SPHERE, empty)):
        assert lib.pupil_world_set_material(w._h, material, C.byref(m)) == abi.ERR_INVALID
        assert lib.pupil_last_error()
        assert material_bytes(w.desc()) == before
    assert lib.pupil_world_set_material(w._h, SPHERE, None) == abi.ERR_INVALID
    assert lib.pupil_world_set_material(None, SPHERE, C.byref(good)) == abi.ERR_INVALID
    assert lib.pupil_world_set_material(w._h, SPHERE, C.byref(good)) == abi.OK
    assert material_bytes(w.desc()) != before
