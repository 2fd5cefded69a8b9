"""Scene, material states and restatements shared by test_material_update_host.py (CPU) and
test_material_update.py (GPU).

The scene mirrors tests/test_deform.py: scenes.uv_sphere(12, 8) (material 0), a floor rectangle
(1), a cube (2), one emissive rectangle (3), a constant environment; film 64 x 48, depth 4.  The
world flattens one material per instance, so desc material i is instance i's.
"""
import ctypes as C

import numpy as np

from pupiloptixlab_amd import World, abi, scenes
from pupiloptixlab_amd import world as W

SPP = 2
SPHERE, FLOOR, CUBE, LIGHT = 0, 1, 2, 3


def base_materials():
    """every instance diffuse: one material bin in the whole scene"""
    return [W.twosided(W.diffuse((0.7, 0.4, 0.3))), W.twosided(W.diffuse((0.6, 0.6, 0.55))),
            W.diffuse((0.3, 0.5, 0.8)), W.diffuse((0.5, 0.5, 0.5))]


def mixed_materials():
    """a rough conductor, a diffuse floor, a dielectric: several bins, one parameter set of each"""
    return [W.rough_conductor(0.2, (0.2, 0.9, 1.1), (3.9, 2.4, 2.2)), W.twosided(W.diffuse((0.6, 0.6, 0.55))),
            W.dielectric(1.5, 1.0), W.diffuse((0.5, 0.5, 0.5))]


def build_world(mats):
    """a world built FROM SCRATCH with the four materials"""
    v, nrm, uv, idx = scenes.uv_sphere(12, 8)
    w = World()
    w.add_instance(w.add_mesh(v, idx, nrm, uv), w.add_material(mats[SPHERE]),
                   W.transform(scale=(1.1, 0.9, 1.0), rotate=((1, 2, 0), 25), translate=(0.2, 0.1, 0.3)))
    w.add_instance(w.add_builtin("rectangle"), w.add_material(mats[FLOOR]),
                   W.transform(scale=(6, 6, 1), rotate=((1, 0, 0), -90), translate=(0.0, -2.2, 0.0)))
    w.add_instance(w.add_builtin("cube"), w.add_material(mats[CUBE]),
                   W.transform(scale=(0.6, 0.6, 0.6), rotate=((0, 1, 0), 20), translate=(-1.9, -1.0, -1.2)))
    w.add_instance(w.add_builtin("rectangle"), w.add_material(mats[LIGHT]),
                   W.transform(scale=(0.8, 0.8, 1), rotate=((1, 0, 0), 90), translate=(0.5, 3.2, 0.0)),
                   emitter_radiance=(9.0, 8.0, 7.0))
    w.add_const_env((0.8, 0.9, 1.0))
    w.set_film(64, 48, 4)
    w.set_sensor(45.0, W.look_at_mitsuba((0.5, 1.5, -7.0), (0.0, 0.2, 0.0), (0, 1, 0)))
    return w


def texels(w, h, seed, lo=0.05, hi=0.95):
    """(h, w, 4) float32 texels in [lo, hi), alpha 1"""
    t = np.random.default_rng(seed).uniform(lo, hi, (h, w, 4)).astype(np.float32)
    t[..., 3] = 1.0
    return t


def wide_texels(w, h, seed):
    """texels spanning 1e-3 .. 1e3 (log-uniform): their float sum depends on the order of the adds"""
    t = (10.0 ** np.random.default_rng(seed).uniform(-3.0, 3.0, (h, w, 4))).astype(np.float32)
    t[..., 3] = 1.0
    return t


def material_bytes(desc):
    return C.string_at(desc.materials, desc.num_materials * C.sizeof(abi.Material))


# ------------------------------------------------------------------ the host's precompute, restated
def sequential_sums(rgba):
    """GetPixelAverage's sums: float32 r, g, b added texel by texel in row-major order"""
    flat = np.asarray(rgba, np.float32).reshape(-1, 4)
    r = g = b = np.float32(0.0)
    for px in flat:
        r = np.float32(r + px[0])
        g = np.float32(g + px[1])
        b = np.float32(b + px[2])
    return r, g, b


def pixel_average(tex):
    """of an rgb triple, a ("checkerboard", c0, c1) tuple or an (h, w, 4) array; vec3 / float
    multiplies by the reciprocal (vec_math.h), every operation rounded to float32"""
    f = np.float32
    if isinstance(tex, tuple) and tex and tex[0] == "checkerboard":
        return tuple(f(f(f(a) + f(b)) * f(0.5)) for a, b in zip(tex[1], tex[2]))
    if isinstance(tex, np.ndarray) and tex.ndim == 3:
        h, w = tex.shape[:2]
        inv = f(f(1.0) / f(f(f(1.0) * f(h)) * f(w)))
        return tuple(f(s * inv) for s in sequential_sums(tex))
    return tuple(f(c) for c in tex)


def luminance(c):
    f = np.float32
    return f(f(f(f(0.2126) * c[0]) + f(f(0.7152) * c[1])) + f(f(0.0722) * c[2]))


def specular_weight(diffuse, specular):
    """specular_sampling_weight of a plastic (optix_material.cpp:106-116) as float32"""
    d, s = luminance(pixel_average(diffuse)), luminance(pixel_average(specular))
    return np.float32(s / np.float32(s + d))
