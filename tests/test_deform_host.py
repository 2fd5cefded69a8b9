"""Deformable meshes, host side (no GPU): the new entry points exist and validate their
arguments, World.set_mesh_vertices changes what desc() describes -- vertices and, for an emissive
mesh, the area emitters -- exactly as a world built from scratch on the deformed mesh would."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import oracle
from pupiloptixlab_amd import World, abi
from pupiloptixlab_amd import world as W
from pupiloptixlab_amd import scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("pupil_pt_update_shape_vertices", "pupil_world_set_mesh_vertices")


def _mesh():
    v, nrm, uv, idx = scenes.uv_sphere(12, 8)
    return (np.asarray(v, np.float32).reshape(-1, 3), np.asarray(nrm, np.float32).reshape(-1, 3),
            np.asarray(uv, np.float32).reshape(-1, 2), np.asarray(idx, np.uint32).reshape(-1, 3))


def _bulge(p):
    q = p.copy()
    q[:, 2] *= (1.0 + 0.8 * np.sin(3.0 * p[:, 0])).astype(np.float32)
    return q


def _world(pos, nrm, emissive=True):
    """shape 0 / instance 0: the (emissive) mesh; a builtin sphere; a mesh without normals"""
    _, _, uv, idx = _mesh()
    w = World()
    m = w.add_material(W.twosided(W.diffuse((0.7, 0.4, 0.3))))
    w.add_instance(w.add_mesh(pos, idx, nrm, uv), m,
                   W.transform(scale=(1.1, 0.9, 1.0), rotate=((1, 2, 0), 25), translate=(0.2, 0.1, 0.3)),
                   emitter_radiance=(4.0, 3.0, 2.0) if emissive else None)
    w.add_instance(w.add_builtin("sphere"), m, W.transform(scale=(0.5, 0.5, 0.5), translate=(2.0, 0.0, 0.0)))
    tri = np.array([[-6, -2, -6], [6, -2, -6], [0, -2, 8]], np.float32)
    w.add_instance(w.add_mesh(tri, np.array([[0, 1, 2]], np.uint32)), m)
    w.add_const_env((0.2, 0.2, 0.3))
    w.set_film(32, 24, 3)
    w.set_sensor(45.0, W.look_at_mitsuba((0.5, 1.5, -7.0), (0.0, 0.2, 0.0), (0, 1, 0)))
    return w


def _emitter_bytes(desc):
    n = desc.num_area_emitters
    buf = C.string_at(desc.area_emitters, n * C.sizeof(abi.Emitter))
    a = np.frombuffer(buf, np.uint8).reshape(n, C.sizeof(abi.Emitter)).copy()
    # the radiance texture carries a pointer (null for an rgb texture) -- nothing else is an address
    return a


def test_new_entries_are_exported_declared_and_bound():
    lib = abi.load_library()
    header = open(os.path.join(ROOT, "include", "pupil_pt.h")).read()
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in abi.SIGNATURES, name
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
    assert re.search(r"#define\s+PUPIL_VERTS_DEVICE\s+1u", header) and re.search(r"#define\s+PUPIL_VERTS_REBUILD\s+2u", header)
    assert (abi.VERTS_DEVICE, abi.VERTS_REBUILD) == (1, 2)
    assert lib.pupil_abi_version() == 7
    assert abi.Counters._fields_[-1][0] == "hidden_instances"  # the counters did not grow


def test_invalid_arguments():
    lib = abi.load_library()
    p = np.zeros(9, np.float32)
    pp = p.ctypes.data_as(C.c_void_p)
    assert lib.pupil_pt_update_shape_vertices(None, 0, pp, None, 0, None) == abi.ERR_INVALID
    pos, nrm, _, _ = _mesh()
    w = _world(pos, nrm)
    f = lambda a: None if a is None else np.ascontiguousarray(a, np.float32).ctypes.data_as(abi.f32p)
    set_v = lib.pupil_world_set_mesh_vertices
    assert set_v(None, 0, f(pos), None) == abi.ERR_INVALID
    assert set_v(w._h, 0, None, None) == abi.ERR_INVALID
    assert set_v(w._h, 99, f(pos), None) == abi.ERR_INVALID
    assert set_v(w._h, 1, f(pos), None) == abi.ERR_INVALID          # the builtin sphere
    assert set_v(w._h, 2, f(pos[:3]), f(nrm[:3])) == abi.ERR_INVALID  # normals for a mesh without them
    assert set_v(w._h, 2, f(pos[:3]), None) == abi.OK
    with pytest.raises(ValueError):
        w.set_mesh_vertices(0, pos[:-1])
    with pytest.raises(abi.PupilError):
        w.set_mesh_vertices(7, pos)


def test_set_mesh_vertices_changes_the_desc():
    pos, nrm, _, _ = _mesh()
    w = _world(pos, nrm)
    d0 = w.desc()
    nv = d0.shapes[0].num_vertices
    assert np.array_equal(np.ctypeslib.as_array(d0.shapes[0].positions, (nv, 3)), pos)
    new = _bulge(pos)
    assert new[:, 2].max() > pos[:, 2].max() + 0.3  # the bulge leaves the old bounds
    w.set_mesh_vertices(0, new)  # normals kept
    d1 = w.desc()
    assert d1.shapes[0].num_vertices == nv and d1.shapes[0].num_faces == d0.shapes[0].num_faces
    assert np.array_equal(np.ctypeslib.as_array(d1.shapes[0].positions, (nv, 3)), new)
    assert np.array_equal(np.ctypeslib.as_array(d1.shapes[0].normals, (nv, 3)), nrm)
    w.set_mesh_vertices(0, new, -nrm)
    assert np.array_equal(np.ctypeslib.as_array(w.desc().shapes[0].normals, (nv, 3)), -nrm)


@pytest.mark.parametrize("deform", ["bulge", "shrink"])
def test_emitters_and_oracle_render_equal_a_world_built_from_scratch(deform):
    pos, nrm, _, _ = _mesh()
    new = _bulge(pos) if deform == "bulge" else (0.4 * pos).astype(np.float32)
    new_n = np.ascontiguousarray(nrm[:, [1, 2, 0]])  # any other normals
    w = _world(pos, nrm)
    before = _emitter_bytes(w.desc())
    w.set_mesh_vertices(0, new, new_n)
    d_upd = w.desc()
    scratch = _world(new, new_n)
    d_new = scratch.desc()
    assert d_upd.num_area_emitters == d_new.num_area_emitters == d_new.shapes[0].num_faces
    got, ref = _emitter_bytes(d_upd), _emitter_bytes(d_new)
    assert not np.array_equal(got, before)
    assert np.array_equal(got, ref)  # triangles, normals, area, select probability: byte for byte
    e = d_upd.area_emitters[5]
    assert e.area > 0.0 and e.select_probability > 0.0
    a = oracle.OracleScene(d_upd).render(spp=1)
    b = oracle.OracleScene(d_new).render(spp=1)
    for k in ("accum", "albedo", "normal"):
        assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), k
