"""The scene of tests/test_instance_set.py and test_instance_set_host.py, as a list of instance
specs a World is built from, so that "the edited world" and "a world built that way from the
start" are two lists.

Shapes: FLOOR, A (a cube), SPHERE, B (a uv sphere), LAMP (a rectangle), C (a tetrahedron no
instance of BASE shows).  BASE: 0 the floor, 1 and 2 shape A under two transforms (2 is hidden),
3 a sphere, 4 the lamp -- the only emitter, and not the last instance -- and 5 shape B.
109 primitives, film 48 x 48, depth 4."""
import numpy as np

from pupiloptixlab_amd import World, scenes
from pupiloptixlab_amd import world as W

import replace_mesh_cases as meshes

FLOOR, A, SPHERE, B, LAMP, C = range(6)
GREY, RED, BLUE, GLASS = range(4)
LAMP_INSTANCE = 4
SIZE = 48
RADIANCE = (14.0, 13.0, 11.0)


def inst(shape, material, visible=True, radiance=None, **xf):
    return {"shape": shape, "material": material, "visible": visible, "radiance": radiance, "xf": xf}


BASE = (
    inst(FLOOR, GREY, scale=(6, 1, 6), translate=(0.0, -1.6, 0.0)),
    inst(A, RED, scale=(0.8, 0.8, 0.8), rotate=((0, 1, 0), 30), translate=(-1.3, -0.4, 0.2)),
    inst(A, BLUE, visible=False, scale=(0.5, 0.7, 0.5), rotate=((1, 0, 1), -25), translate=(1.4, -0.6, -0.6)),
    inst(SPHERE, GLASS, scale=(0.6, 0.6, 0.6), translate=(0.1, -0.9, -1.4)),
    inst(LAMP, GREY, radiance=RADIANCE, scale=(1.2, 1.2, 1.0), rotate=((1, 0, 0), 90), translate=(0.0, 3.2, 0.0)),
    inst(B, GREY, scale=(0.7, 0.7, 0.7), translate=(0.3, 0.4, 1.2)),
)
# what the cases add
EXTRA_A = inst(A, BLUE, scale=(0.6, 0.6, 0.6), rotate=((0, 0, 1), 20), translate=(0.2, 0.6, -0.3))
EXTRA_C = inst(C, RED, scale=(0.7, 0.7, 0.7), translate=(-0.4, 0.2, -0.9))
HIDDEN_SPHERE = inst(SPHERE, RED, visible=False, scale=(0.5, 0.5, 0.5), translate=(0.9, 0.5, 0.4))
SECOND_LAMP = inst(LAMP, GREY, radiance=RADIANCE, scale=(0.5, 0.5, 1.0), rotate=((1, 0, 0), 90), translate=(1.5, 2.5, 0.0))


def _materials():
    return [W.twosided(W.diffuse((0.6, 0.6, 0.55))),
            W.twosided(W.diffuse(W.checkerboard((0.8, 0.3, 0.2), (0.2, 0.3, 0.8), (4.0, 4.0)))),
            W.twosided(W.rough_plastic(0.2, (0.2, 0.4, 0.8))), W.dielectric()]


def empty_world():
    """shapes, materials, film and sensor; no instance yet"""
    w = World()
    fl = w.add_mesh([(-1, 0, -1), (1, 0, -1), (1, 0, 1), (-1, 0, 1)], [(0, 2, 1), (0, 3, 2)],
                    [(0, 1, 0)] * 4, [(0, 0), (1, 0), (1, 1), (0, 1)])
    m = meshes.cube()
    a = w.add_mesh(m["positions"], m["faces"], m["normals"], m["texcoords"])
    sp = w.add_builtin("sphere")
    v, nrm, uv, idx = scenes.uv_sphere(8, 6)
    b = w.add_mesh(v, idx, nrm, uv)
    lamp = w.add_builtin("rectangle")
    t = meshes.tetrahedron()
    c = w.add_mesh(t["positions"], t["faces"], t["normals"], t["texcoords"])
    assert (fl, a, sp, b, lamp, c) == (FLOOR, A, SPHERE, B, LAMP, C)
    assert [w.add_material(x) for x in _materials()] == [GREY, RED, BLUE, GLASS]
    w.set_film(SIZE, SIZE, 4)
    w.set_sensor(50.0, W.look_at_mitsuba((0.4, 1.4, -6.5), (0.0, -0.3, 0.0), (0, 1, 0)))
    return w


def add(w, spec):
    i = w.add_instance(spec["shape"], spec["material"], W.transform(**spec["xf"]), emitter_radiance=spec["radiance"])
    if not spec["visible"]:
        w.set_instance_visibility(i, 0)
    return i


def world(specs=BASE):
    w = empty_world()
    for s in specs:
        add(w, s)
    return w


def to_world(w):
    """(n, 12) float32: the transforms of the world's instances"""
    d = w.desc()
    return np.array([list(d.instances[i].to_world) for i in range(d.num_instances)], np.float32).reshape(-1, 12)


fixed_rays = meshes.fixed_rays
