"""The staged resize of the engine's emitter tables (csrc/host/emitter_tables.h stage_resize /
adopt_resize) without a GPU: the stand-alone driver emitter_resize_driver.cpp puts a counting
allocator in place of the device and grows, shrinks, empties and refills the table, with and without
an env map.  Texel buffers of kept emitters are moved and not duplicated, those of emitters that
went are freed exactly once, a new bitmap is uploaded once per instance, and an allocation failing at
each staging step leaves cur() and book() untouched.  It is built with -fsanitize=address,undefined,
so a leak, a double free or a use after free fails the run.  Then the world: set_mesh keeps refusing
an emissive shape, set_mesh(allow_emissive=True) describes the re-meshed lamp as a world built on the
new mesh does; and the new entry points refuse NULL arguments."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from pupiloptixlab_amd import abi

import instance_set_cases as cases
import replace_mesh_cases as meshes

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "pupiloptixlab_amd", "csrc")


def test_staged_resize_owns_moves_and_frees(tmp_path):
    exe = tmp_path / "emitter_resize_driver"
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-O1", "-g",
                        "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", CSRC,
                        os.path.join(HERE, "emitter_resize_driver.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    env = {k: v for k, v in os.environ.items() if k != "PUPIL_EMITTER_SELECT"}  # the driver expects the guide
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env)
    assert r.returncode == 0 and r.stderr == "" and r.stdout.startswith("ok "), (r.returncode, r.stdout, r.stderr)


# ------------------------------------------------------------------ the world
LAMP = cases.LAMP
# a second lamp and a point light behind the first: their offsets and indices shift with the lamp's faces
SPECS = cases.BASE + (cases.SECOND_LAMP,)


def _world(lamp_mesh=None):
    w = cases.world(SPECS) if lamp_mesh is None else _built_on(lamp_mesh)
    return w


def _built_on(name):
    """the scene built from scratch with the LAMP shape = meshes.MESHES[name]: the same calls in the
    same order as instance_set_cases.empty_world, but for the lamp"""
    from pupiloptixlab_amd import World, scenes
    from pupiloptixlab_amd import world as W

    w = World()
    w.add_mesh([(-1, 0, -1), (1, 0, -1), (1, 0, 1), (-1, 0, 1)], [(0, 2, 1), (0, 3, 2)], [(0, 1, 0)] * 4,
               [(0, 0), (1, 0), (1, 1), (0, 1)])
    m = meshes.cube()
    w.add_mesh(m["positions"], m["faces"], m["normals"], m["texcoords"])
    w.add_builtin("sphere")
    v, nrm, uv, idx = scenes.uv_sphere(8, 6)
    w.add_mesh(v, idx, nrm, uv)
    m = meshes.MESHES[name]()
    assert w.add_mesh(m["positions"], m["faces"], m["normals"], m["texcoords"]) == LAMP
    t = meshes.tetrahedron()
    w.add_mesh(t["positions"], t["faces"], t["normals"], t["texcoords"])
    for x in cases._materials():
        w.add_material(x)
    w.set_film(cases.SIZE, cases.SIZE, 4)
    w.set_sensor(50.0, W.look_at_mitsuba((0.4, 1.4, -6.5), (0.0, -0.3, 0.0), (0, 1, 0)))
    for s in SPECS:
        cases.add(w, s)
    return w


def _struct_bytes(x, skip=()):
    """a ctypes struct field for field, pointers left out"""
    out = []
    for name, typ in x._fields_:
        if name in skip:
            continue
        v = getattr(x, name)
        if isinstance(v, C.Structure):
            out.append(_struct_bytes(v, skip))
        elif isinstance(v, C.Array):
            out.append(bytes(v))
        elif isinstance(v, (int, float)):
            out.append(np.array([v]).tobytes())
        # pointers (texel and mesh arrays) are compared through what they point at, below
    return b"".join(out)


def _same_desc(a, b):
    assert (a.num_shapes, a.num_instances, a.num_area_emitters, a.num_materials) == \
           (b.num_shapes, b.num_instances, b.num_area_emitters, b.num_materials)
    for i in range(a.num_instances):
        assert _struct_bytes(a.instances[i]) == _struct_bytes(b.instances[i]), ("instance", i)
    for e in range(a.num_area_emitters):
        assert _struct_bytes(a.area_emitters[e]) == _struct_bytes(b.area_emitters[e]), ("emitter", e)
    for s in range(a.num_shapes):
        x, y = a.shapes[s], b.shapes[s]
        assert (x.kind, x.num_vertices, x.num_faces) == (y.kind, y.num_vertices, y.num_faces), ("shape", s)
        for name, per in (("positions", 3 * x.num_vertices), ("normals", 3 * x.num_vertices),
                          ("texcoords", 2 * x.num_vertices), ("indices", 3 * x.num_faces)):
            p, q = getattr(x, name), getattr(y, name)
            assert bool(p) == bool(q), ("shape", s, name)
            if p:
                assert np.array_equal(np.ctypeslib.as_array(p, (per,)), np.ctypeslib.as_array(q, (per,))), ("shape", s, name)


def test_world_set_mesh_still_refuses_an_emissive_shape():
    w = _world()
    before = w.desc().num_area_emitters
    m = meshes.tetrahedron()
    with pytest.raises(abi.PupilError) as e:
        w.set_mesh(LAMP, m["positions"], m["faces"], m["normals"], m["texcoords"])
    assert e.value.code == abi.ERR_UNSUPPORTED
    assert w.desc().num_area_emitters == before
    assert w._lib.pupil_world_replace_mesh(w._h, LAMP, 4, 4, None, None, None, None, abi.WORLD_MESH_EMISSIVE_OK) == abi.ERR_INVALID
    p = np.ascontiguousarray(m["positions"], np.float32)
    f = np.ascontiguousarray(m["faces"], np.uint32)
    assert w._lib.pupil_world_replace_mesh(w._h, LAMP, 4, 4, p.ctypes.data_as(abi.f32p), None, None,
                                           f.ctypes.data_as(abi.u32p), 2) == abi.ERR_INVALID  # unknown flags
    assert w.desc().num_area_emitters == before


@pytest.mark.parametrize("name", ["tetrahedron", "cube", "icosphere"])
def test_world_set_mesh_allow_emissive_describes_the_new_ranges(name):
    w = _world()
    w.add_point_light((0.5, 2.0, -1.0), (3.0, 3.0, 3.0))
    d0 = w.desc()
    old = [d0.instances[i].emitter_offset for i in range(d0.num_instances)]
    assert old[cases.LAMP_INSTANCE] == 0 and old[-1] == 2 and d0.num_area_emitters == 5
    m = meshes.MESHES[name]()
    nf = len(m["faces"])
    w.set_mesh(LAMP, m["positions"], m["faces"], m["normals"], m["texcoords"], allow_emissive=True)
    d = w.desc()
    new = [d.instances[i].emitter_offset for i in range(d.num_instances)]
    assert new[cases.LAMP_INSTANCE] == 0 and new[-1] == nf and d.num_area_emitters == 2 * nf + 1
    assert [x for i, x in enumerate(new) if i not in (cases.LAMP_INSTANCE, len(new) - 1)] == [-1] * (len(new) - 2)
    assert d.area_emitters[2 * nf].type == abi.EMITTER_POINT
    total = sum(d.area_emitters[e].select_probability for e in range(d.num_area_emitters))
    assert abs(total - 1.0) < 1e-4
    ref = _built_on(name)
    ref.add_point_light((0.5, 2.0, -1.0), (3.0, 3.0, 3.0))
    _same_desc(d, ref.desc())


# ------------------------------------------------------------------ the ABI
def test_new_symbols_are_declared():
    for name in ("pupil_pt_set_instances_emitters", "pupil_pt_emitter_resize_info", "pupil_pt_emitter_table_info",
                 "pupil_world_replace_mesh"):
        assert name in abi.SIGNATURES, name


def test_null_arguments_are_invalid():
    lib = abi.load_library()
    desc = abi.SceneDesc()
    assert lib.pupil_pt_set_instances_emitters(None, C.byref(desc), None, None, 0, None) == abi.ERR_INVALID
    assert lib.pupil_pt_emitter_resize_info(None, None, None, None) == abi.ERR_INVALID
    assert lib.pupil_pt_emitter_table_info(None, None, None, None) == abi.ERR_INVALID
    assert lib.pupil_world_replace_mesh(None, 0, 1, 1, None, None, None, None, 0) == abi.ERR_INVALID
