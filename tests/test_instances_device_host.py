"""Instances from device memory, host side (no GPU): the four entry points exist, the three that
touch no GPU refuse bad arguments, and pupil_debug_invert3x4 -- compiled from the text the kernel
compiles (pt_invert.h) -- gives bit for bit the to_object the world computes.

Also the world tests/test_instances_device.py runs on."""
import ctypes as C
import functools

import numpy as np

from pupiloptixlab_amd import World, abi
from pupiloptixlab_amd import world as W

from test_device_emitters_host import grid_mesh

NEW = ("pupil_pt_update_instances_device", "pupil_pt_get_instance_transforms", "pupil_pt_instances_device_info",
       "pupil_debug_invert3x4")
f32 = np.float32


# ------------------------------------------------------------------ the world of the GPU tests
# 24 instances: 0..17 a 17 x 17 grid (512 triangles: a BLAS of four BVH4 levels at two per leaf),
# 18, 19 a 5 x 4 grid, 20, 21 spheres, 22 an emissive rectangle, 23 an emissive sphere.  No env: the
# light comes from 22 and 23, and their three emissive primitives give the scene a terminal-ray
# cull set.  Film 64 x 48, depth 4.
N_GRID, N_INST = 18, 24
GRIDS = tuple(range(N_GRID))
SMALL, SPHERES, EMISSIVE_MESH, EMISSIVE_SPHERE = (18, 19), (20, 21), 22, 23


def _matrix(rng, k, moved):
    """instance k's to_world: non-uniform scale, a rotation about a random axis, a place on a
    6 x 4 lattice in front of the camera (moved: another scale, axis, angle and offset)"""
    s = rng.uniform(0.25, 0.6, 3)
    axis = rng.normal(size=3)
    angle = rng.uniform(-170.0, 170.0)
    cell = np.array([(k % 6) - 2.5, (k // 6) - 1.5, 0.0]) * np.array([1.5, 1.3, 1.0])
    t = cell + rng.uniform(-0.3, 0.3, 3) + np.array([0.0, 0.0, rng.uniform(-1.0, 1.0)])
    if k in (EMISSIVE_MESH, EMISSIVE_SPHERE):  # the lights stay above the field
        t[1] = 3.0 + (0.4 if moved else 0.0)
        t[2] = -1.5
    return W.transform(scale=tuple(s), rotate=(tuple(axis), angle), translate=tuple(t))


@functools.lru_cache(maxsize=None)
def transforms(state):
    """(24, 4, 4) float32: 'base' or 'moved' (every instance elsewhere)"""
    rng = np.random.default_rng({"base": 101, "moved": 202}[state])
    return np.stack([_matrix(rng, k, state == "moved") for k in range(N_INST)]).astype(f32)


def rows12(m):
    """(n, 4, 4) -> (n, 12): the 3x4 the engine takes"""
    return np.ascontiguousarray(np.asarray(m, f32).reshape(-1, 16)[:, :12])


def mixed(moved_ids):
    """the transforms with the instances in moved_ids at their 'moved' place, the others at base"""
    m = transforms("base").copy()
    ids = list(moved_ids)
    m[ids] = transforms("moved")[ids]
    return m


def world(xf=None):
    """the 24-instance world with to_world xf[k] ((24, 4, 4); None: base), built from scratch"""
    xf = transforms("base") if xf is None else xf
    w = World()
    p, n, uv, idx = grid_mesh(17, 17)
    big = w.add_mesh(p, idx, n, uv)
    p2, n2, uv2, idx2 = grid_mesh(5, 4)
    small = w.add_mesh(p2, idx2, n2, uv2)
    sphere, rect = w.add_builtin("sphere"), w.add_builtin("rectangle")
    m = w.add_material(W.twosided(W.diffuse((0.7, 0.6, 0.4))))
    m2 = w.add_material(W.twosided(W.diffuse((0.3, 0.5, 0.7))))
    for k in range(N_INST):
        if k < N_GRID:
            w.add_instance(big, m if k % 2 else m2, xf[k])
        elif k in SMALL:
            w.add_instance(small, m, xf[k])
        elif k in SPHERES:
            w.add_instance(sphere, m2, xf[k])
        elif k == EMISSIVE_MESH:
            w.add_instance(rect, m, xf[k], emitter_radiance=(30.0, 28.0, 24.0))
        else:
            w.add_instance(sphere, m, xf[k], emitter_radiance=(20.0, 22.0, 26.0))
    w.set_film(64, 48, 4)
    w.set_sensor(50.0, W.look_at_mitsuba((0.3, 0.4, -9.0), (0.0, 0.2, 0.0), (0, 1, 0)))
    return w


def desc_matrices(desc):
    """(to_world, to_object) of a desc's instances, (n, 12) float32 each"""
    n = desc.num_instances
    return (np.array([list(desc.instances[i].to_world) for i in range(n)], f32),
            np.array([list(desc.instances[i].to_object) for i in range(n)], f32))


# ------------------------------------------------------------------ symbols and argument checks
def test_the_four_symbols_exist():
    lib = abi.load_library()
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in abi.SIGNATURES, name


def test_null_and_range_checks_without_a_gpu():
    lib = abi.load_library()
    buf = np.zeros(12, f32)
    p = buf.ctypes.data_as(abi.f32p)
    assert lib.pupil_pt_update_instances_device(None, 1, None, C.c_void_p(16), None, None) == abi.ERR_INVALID
    assert b"null" in lib.pupil_last_error()
    assert lib.pupil_pt_get_instance_transforms(None, 0, 1, p, p) == abi.ERR_INVALID
    assert lib.pupil_pt_instances_device_info(None, None, None, None, None, None, None) == abi.ERR_INVALID
    assert lib.pupil_debug_invert3x4(None, p) == abi.ERR_INVALID
    assert lib.pupil_debug_invert3x4(p, None) == abi.ERR_INVALID


# ------------------------------------------------------------------ the inverse, bit for bit
def _invert(m12):
    lib = abi.load_library()
    a = np.ascontiguousarray(m12, f32)
    out = np.zeros(12, f32)
    abi.check(lib.pupil_debug_invert3x4(a.ctypes.data_as(abi.f32p), out.ctypes.data_as(abi.f32p)))
    return out


def _seeded_matrices(n=2000, seed=7):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        out.append(W.transform(scale=tuple(rng.uniform(0.05, 8.0, 3) * rng.choice([-1.0, 1.0], 3)),
                               rotate=(tuple(rng.normal(size=3)), rng.uniform(-180.0, 180.0)),
                               translate=tuple(rng.uniform(-50.0, 50.0, 3))))
    shear = np.eye(4, dtype=f32)
    shear[0, 1], shear[0, 2], shear[1, 2], shear[2, 0] = 0.7, -1.3, 0.45, 0.2
    shear[:3, 3] = (3.0, -2.0, 0.5)
    out.append(shear)
    return np.stack(out).astype(f32)


def test_invert3x4_equals_the_worlds_to_object_bit_for_bit():
    mats = _seeded_matrices()
    w = World()
    rect = w.add_builtin("rectangle")
    m = w.add_material(W.diffuse((0.5, 0.5, 0.5)))
    for x in mats:
        w.add_instance(rect, m, x)
    w.set_film(8, 8, 1)
    w.set_sensor(45.0, W.look_at_mitsuba((0, 0, -5), (0, 0, 0), (0, 1, 0)))
    tw, to = desc_matrices(w.desc())
    assert len(tw) == 2001
    assert np.array_equal(tw.view(np.uint32), rows12(mats).view(np.uint32))
    got = np.stack([_invert(x) for x in tw])
    assert np.array_equal(got.view(np.uint32), to.view(np.uint32))
    assert np.abs(got).max() > 0.0


def test_singular_matrix_gives_all_zeros():
    m = rows12(W.transform(scale=(1.0, 0.0, 2.0), translate=(1.0, 2.0, 3.0))[None])[0]
    out = _invert(m)
    assert np.array_equal(out.view(np.uint32), np.zeros(12, np.uint32))
    m2 = np.array([1, 2, 3, 0, 2, 4, 6, 0, 0, 1, 0, 5], f32)  # two proportional rows
    assert np.array_equal(_invert(m2).view(np.uint32), np.zeros(12, np.uint32))
