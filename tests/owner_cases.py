"""The scene and the meshes of tests/test_engine_owner.py and of the repeated replacements in
tests/test_replace_mesh.py: the Cornell box of scenes.py at 32 x 32, depth 4, whose short box (a cube
of 12 triangles) carries a 5 x 3 bitmap."""
import os

import numpy as np

from pupiloptixlab_amd import World, abi, scenes
from pupiloptixlab_amd import world as W

from material_cases import texels

SIZE = 32


def cornell(tmp_path):
    """(world, box shape, its instance, its material)"""
    w = World().load_scene(scenes.cornell_xml(os.path.join(str(tmp_path), "cornell.xml"), SIZE, SIZE, 4))
    d = w.desc()
    box = next(s for s in range(d.num_shapes) if d.shapes[s].kind == abi.SHAPE_MESH and d.shapes[s].num_faces == 12)
    inst = next(i for i in range(d.num_instances) if d.instances[i].shape == box)
    assert d.instances[inst].emitter_offset < 0
    material = d.instances[inst].material
    w.set_material(material, W.twosided(W.diffuse(W.bitmap(texels(5, 3, 61), filter=1))))
    return w, box, inst, material


def box_meshes(world, box):
    """the box as the world holds it (12 triangles) and the same surface with every triangle split
    in four at its edge midpoints (48 triangles, 72 vertices, no normals or texcoords)"""
    sh = world.desc().shapes[box]
    p = np.ctypeslib.as_array(sh.positions, (sh.num_vertices, 3)).copy()
    f = np.ctypeslib.as_array(sh.indices, (sh.num_faces, 3)).copy()
    n = np.ctypeslib.as_array(sh.normals, (sh.num_vertices, 3)).copy() if sh.normals else None
    t = np.ctypeslib.as_array(sh.texcoords, (sh.num_vertices, 2)).copy() if sh.texcoords else None
    coarse = {"positions": p, "faces": f.astype(np.uint32), "normals": n, "texcoords": t}
    a, b, c = p[f[:, 0]], p[f[:, 1]], p[f[:, 2]]
    fine_p = np.stack([a, b, c, (a + b) / 2, (b + c) / 2, (c + a) / 2], 1).reshape(-1, 3).astype(np.float32)
    local = np.array([[0, 3, 5], [1, 4, 3], [2, 5, 4], [3, 4, 5]], np.uint32)
    fine_f = (6 * np.arange(len(f), dtype=np.uint32)[:, None, None] + local[None]).reshape(-1, 3)
    assert len(f) == 12 and len(fine_f) == 48
    fine = {"positions": fine_p, "faces": fine_f, "normals": None, "texcoords": None}
    return coarse, fine


def replace(pt, world, box, mesh):
    """the world and the engine, kept in step"""
    world.set_mesh(box, mesh["positions"], mesh["faces"], mesh["normals"], mesh["texcoords"])
    pt.replace_shape(box, mesh["positions"], mesh["faces"], mesh["normals"], mesh["texcoords"])
