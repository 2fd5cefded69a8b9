"""The scene and the meshes of tests/test_replace_mesh.py.

Instance order (desc().instances): 0 a mesh floor, 1 and 2 shape S under two transforms (2 is
hidden), 3 a sphere, 4 a second mesh -- behind S in instance order, so its prim_offset moves when
S changes its face count -- and 5 a rectangle lamp, the only emitter.  Shapes: FLOOR, S, SPHERE,
OTHER, LAMP.  Film 48 x 48, depth 4."""
import functools

import numpy as np

from pupiloptixlab_amd import World, scenes
from pupiloptixlab_amd import world as W

FLOOR, S, SPHERE, OTHER, LAMP = range(5)
S_INSTANCES = (1, 2)
HIDDEN = 2
SIZE = 48


def _mesh(p, f, n=None, t=None):
    return {"positions": np.ascontiguousarray(p, np.float32).reshape(-1, 3),
            "faces": np.ascontiguousarray(f, np.uint32).reshape(-1, 3),
            "normals": None if n is None else np.ascontiguousarray(n, np.float32).reshape(-1, 3),
            "texcoords": None if t is None else np.ascontiguousarray(t, np.float32).reshape(-1, 2)}


@functools.lru_cache(maxsize=None)
def cube():
    """12 faces, 24 vertices, face normals and per-face texcoords"""
    p, n, t, f = [], [], [], []
    for axis in range(3):
        for sign in (-1.0, 1.0):
            u, v = (axis + 1) % 3, (axis + 2) % 3
            base = len(p)
            for a, b in ((-1, -1), (1, -1), (1, 1), (-1, 1)):
                q = [0.0, 0.0, 0.0]
                q[axis], q[u], q[v] = sign, a * sign, b
                p.append(q)
                nn = [0.0, 0.0, 0.0]
                nn[axis] = sign
                n.append(nn)
                t.append([(a + 1) / 2, (b + 1) / 2])
            f += [[base, base + 1, base + 2], [base, base + 2, base + 3]]
    return _mesh(p, f, n, t)


@functools.lru_cache(maxsize=None)
def icosphere():
    """320 faces, 162 vertices (an icosahedron subdivided twice), normals, no texcoords"""
    g = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, g, 0), (1, g, 0), (-1, -g, 0), (1, -g, 0), (0, -1, g), (0, 1, g), (0, -1, -g), (0, 1, -g),
         (g, 0, -1), (g, 0, 1), (-g, 0, -1), (-g, 0, 1)]
    v = [np.array(x, np.float64) / np.linalg.norm(x) for x in v]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6),
         (7, 1, 8), (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10),
         (8, 6, 7), (9, 8, 1)]
    for _ in range(2):
        mid, nf = {}, []

        def m(a, b):
            k = (min(a, b), max(a, b))
            if k not in mid:
                x = v[a] + v[b]
                v.append(x / np.linalg.norm(x))
                mid[k] = len(v) - 1
            return mid[k]

        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    p = np.array(v, np.float32)
    assert len(f) == 320 and len(p) == 162
    return _mesh(1.2 * p, f, p)


@functools.lru_cache(maxsize=None)
def tetrahedron():
    """4 faces, no normals, no texcoords"""
    p = [(1, 1, 1), (1, -1, -1), (-1, 1, -1), (-1, -1, 1)]
    return _mesh(p, [(0, 1, 2), (0, 3, 1), (0, 2, 3), (1, 3, 2)])


@functools.lru_cache(maxsize=None)
def grid():
    """96 x 48 quads = 9216 faces over a wavy sheet, texcoords, no normals: with it the scene holds
    more than 8192 primitives"""
    nx, ny = 96, 48
    x, y = np.meshgrid(np.linspace(-1.5, 1.5, nx + 1), np.linspace(-1.0, 1.0, ny + 1), indexing="xy")
    z = 0.25 * np.sin(3.0 * x) * np.cos(4.0 * y)
    p = np.stack([x, y, z], -1).reshape(-1, 3)
    t = np.stack([(x + 1.5) / 3.0, (y + 1.0) / 2.0], -1).reshape(-1, 2)
    i = (np.arange(ny)[:, None] * (nx + 1) + np.arange(nx)[None, :]).reshape(-1)
    f = np.concatenate([np.stack([i, i + 1, i + nx + 2], 1), np.stack([i, i + nx + 2, i + nx + 1], 1)])
    assert len(f) == 9216
    return _mesh(p, f, None, t)


MESHES = {"cube": cube, "icosphere": icosphere, "tetrahedron": tetrahedron, "grid": grid}


def world(s_mesh="cube", hidden=True):
    """the test scene with S = MESHES[s_mesh]; instance HIDDEN hidden unless hidden=False"""
    w = World()
    fl = w.add_mesh([(-1, 0, -1), (1, 0, -1), (1, 0, 1), (-1, 0, 1)], [(0, 2, 1), (0, 3, 2)],
                    [(0, 1, 0)] * 4, [(0, 0), (1, 0), (1, 1), (0, 1)])
    m = MESHES[s_mesh]()
    s = w.add_mesh(m["positions"], m["faces"], m["normals"], m["texcoords"])
    sp = w.add_builtin("sphere")
    v, nrm, uv, idx = scenes.uv_sphere(8, 6)
    other = w.add_mesh(v, idx, nrm, uv)
    lamp = w.add_builtin("rectangle")
    assert (fl, s, sp, other, lamp) == (FLOOR, S, SPHERE, OTHER, LAMP)
    grey = w.add_material(W.twosided(W.diffuse((0.6, 0.6, 0.55))))
    red = w.add_material(W.twosided(W.diffuse(W.checkerboard((0.8, 0.3, 0.2), (0.2, 0.3, 0.8), (4.0, 4.0)))))
    blue = w.add_material(W.twosided(W.rough_plastic(0.2, (0.2, 0.4, 0.8))))
    glass = w.add_material(W.dielectric())
    w.add_instance(fl, grey, W.transform(scale=(6, 1, 6), translate=(0.0, -1.6, 0.0)))
    w.add_instance(s, red, W.transform(scale=(0.8, 0.8, 0.8), rotate=((0, 1, 0), 30), translate=(-1.3, -0.4, 0.2)))
    w.add_instance(s, blue, W.transform(scale=(0.5, 0.7, 0.5), rotate=((1, 0, 1), -25), translate=(1.4, -0.6, -0.6)))
    w.add_instance(sp, glass, W.transform(scale=(0.6, 0.6, 0.6), translate=(0.1, -0.9, -1.4)))
    w.add_instance(other, grey, W.transform(scale=(0.7, 0.7, 0.7), translate=(0.3, 0.4, 1.2)))
    w.add_instance(lamp, grey, W.transform(scale=(1.2, 1.2, 1.0), rotate=((1, 0, 0), 90), translate=(0.0, 3.2, 0.0)),
                   emitter_radiance=(14.0, 13.0, 11.0))
    w.set_film(SIZE, SIZE, 4)
    w.set_sensor(50.0, W.look_at_mitsuba((0.4, 1.4, -6.5), (0.0, -0.3, 0.0), (0, 1, 0)))
    if hidden:
        w.set_instance_visibility(HIDDEN, 0)
    return w


def set_mesh(w, name):
    m = MESHES[name]()
    w.set_mesh(S, m["positions"], m["faces"], m["normals"], m["texcoords"])
    return m


def fixed_rays(n=256, seed=5):
    """n rays from a shell around the scene towards points near its middle: (n, 8) float32"""
    rng = np.random.default_rng(seed)
    o = rng.normal(size=(n, 3))
    o = 5.0 * o / np.linalg.norm(o, axis=1, keepdims=True)
    o[:, 1] = np.abs(o[:, 1])
    d = rng.uniform(-1.5, 1.5, (n, 3)) - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    r = np.concatenate([o, d, np.full((n, 1), 0.001), np.full((n, 1), 1e16)], 1)
    return np.ascontiguousarray(r, np.float32)
