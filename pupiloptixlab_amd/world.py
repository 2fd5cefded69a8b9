"""Python handle on the C++ scene/world layer (Pupil::resource::Scene +
Pupil::world::World inside libpupil_pt.so).

Mirrors the reference's world API (framework/world/world.h:26-66):
``World.load_scene(path)`` = World::LoadScene (world.cpp:76-139); the
programmatic ``add_*`` calls build the same ShapeInstance list the XML loader
would (resource/shape.cpp:181-217) for the procedural benchmark scenes.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import abi
from .abi import check, load_library


def _f32(a, n=None):
    arr = np.ascontiguousarray(np.asarray(a, dtype=np.float32).reshape(-1))
    if n is not None and arr.size != n:
        raise ValueError(f"expected {n} floats, got {arr.size}")
    return arr


def _ptr(arr, ctype=C.c_float):
    return arr.ctypes.data_as(C.POINTER(ctype)) if arr is not None else None


def _rgb3(v):
    v = np.atleast_1d(np.asarray(v, dtype=np.float32))
    return np.repeat(v, 3) if v.size == 1 else v


def _radians(deg) -> float:
    """Degrees to radians in float32, as the XML loader converts cutoff_angle and beam_width."""
    return float(np.float32(deg) * (np.float32(np.pi) / np.float32(180.0)))


def identity4():
    return np.eye(4, dtype=np.float32)


def rgb(r, g=None, b=None) -> abi.Texture:
    """util::Texture of type RGB (resource/texture.cpp:19-35)."""
    if g is None:
        g = b = r
    t = abi.Texture()
    t.type = abi.TEX_RGB
    t.c0[:] = (r, g, b)
    t.transform[:] = identity4().reshape(-1)
    return t


def checkerboard(color0, color1, uv_scale=(1.0, 1.0)) -> abi.Texture:
    """Checkerboard texture with a to_uv scale (scene.cpp:167-178, util_loader.cpp:188-194)."""
    t = abi.Texture()
    t.type = abi.TEX_CHECKERBOARD
    t.c0[:] = tuple(color0)
    t.c1[:] = tuple(color1)
    m = identity4()
    m[0, 0], m[1, 1] = uv_scale
    t.transform[:] = m.reshape(-1)
    return t


def bitmap(rgba, filter=1, uv_scale=(1.0, 1.0)) -> abi.Texture:
    """Bitmap texture from an (h, w, 4) float32 array, row 0 first (util::BitmapTexture's order);
    filter: 0 point, 1 bilinear.  The texture keeps the array alive: ctypes carries the reference
    into every Material the texture is copied into, and the world copies the texels when it takes
    the material (add_material / set_material)."""
    a = np.ascontiguousarray(np.asarray(rgba, dtype=np.float32))
    if a.ndim != 3 or a.shape[2] != 4 or a.shape[0] == 0 or a.shape[1] == 0:
        raise ValueError(f"bitmap needs an (h, w, 4) array, got {a.shape}")
    t = abi.Texture()
    t.type = abi.TEX_BITMAP
    t.height, t.width = a.shape[0], a.shape[1]
    t.filter = int(filter)
    m = identity4()
    m[0, 0], m[1, 1] = uv_scale
    t.transform[:] = m.reshape(-1)
    t.rgba = _ptr(a)  # the pointer object holds `a`, and t holds the pointer object
    return t


def _mat(mtype, textures, twosided=False, int_ior=1.0, ext_ior=1.0, nonlinear=False) -> abi.Material:
    m = abi.Material()
    m.type = mtype
    m.twosided = int(twosided)
    m.int_ior = int_ior
    m.ext_ior = ext_ior
    m.nonlinear = int(nonlinear)
    m._keep = list(textures)  # a bitmap's texel array lives as long as the material
    for k, t in enumerate(textures):
        m.tex[k] = t
    for k in range(len(textures), 4):
        m.tex[k] = rgb(0.0)
    return m


# material constructors with the reference loader defaults (resource/material.cpp:26-147)
def diffuse(reflectance=(0.5, 0.5, 0.5), twosided=False):
    return _mat(abi.MAT_DIFFUSE, [_tex(reflectance)], twosided)


def dielectric(int_ior=1.5046, ext_ior=1.000277, specular_reflectance=1.0, specular_transmittance=1.0):
    return _mat(abi.MAT_DIELECTRIC, [_tex(specular_reflectance), _tex(specular_transmittance)], False,
                int_ior, ext_ior)


def rough_dielectric(alpha=0.1, int_ior=1.5046, ext_ior=1.000277, specular_reflectance=1.0,
                     specular_transmittance=1.0):
    return _mat(abi.MAT_ROUGH_DIELECTRIC,
                [_tex(alpha), _tex(specular_reflectance), _tex(specular_transmittance)], False, int_ior, ext_ior)


def conductor(eta=(0.0, 0.0, 0.0), k=(1.0, 1.0, 1.0), specular_reflectance=1.0):
    return _mat(abi.MAT_CONDUCTOR, [_tex(eta), _tex(k), _tex(specular_reflectance)])


def rough_conductor(alpha=0.1, eta=(0.0, 0.0, 0.0), k=(1.0, 1.0, 1.0), specular_reflectance=1.0):
    return _mat(abi.MAT_ROUGH_CONDUCTOR, [_tex(alpha), _tex(eta), _tex(k), _tex(specular_reflectance)])


def plastic(diffuse_reflectance=0.5, specular_reflectance=1.0, int_ior=1.49, ext_ior=1.000277, nonlinear=False):
    return _mat(abi.MAT_PLASTIC, [_tex(diffuse_reflectance), _tex(specular_reflectance)], False, int_ior,
                ext_ior, nonlinear)


def rough_plastic(alpha=0.1, diffuse_reflectance=0.5, specular_reflectance=1.0, int_ior=1.49, ext_ior=1.000277,
                  nonlinear=False):
    return _mat(abi.MAT_ROUGH_PLASTIC, [_tex(alpha), _tex(diffuse_reflectance), _tex(specular_reflectance)],
                False, int_ior, ext_ior, nonlinear)


def twosided(m: abi.Material) -> abi.Material:
    m.twosided = 1
    return m


def _tex(v):
    if isinstance(v, abi.Texture):
        return v
    v = np.atleast_1d(np.asarray(v, dtype=np.float32))
    return rgb(float(v[0])) if v.size == 1 else rgb(float(v[0]), float(v[1]), float(v[2]))


@dataclass
class MeshData:
    positions: np.ndarray
    normals: np.ndarray | None
    texcoords: np.ndarray | None
    indices: np.ndarray


class World:
    """world::World + resource::Scene, owned by the C++ host layer."""

    def __init__(self):
        self._lib = load_library()
        h = C.c_void_p()
        check(self._lib.pupil_world_create(C.byref(h)))
        self._h = h
        self._keep = []  # numpy arrays referenced by the C++ side until get_desc copies them
        self._desc = None

    def close(self):
        if getattr(self, "_h", None):
            self._lib.pupil_world_destroy(self._h)
            self._h = None

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    def load_scene(self, path: str):
        check(self._lib.pupil_world_load_xml(self._h, str(path).encode()))
        self._desc = None
        return self

    def set_film(self, width: int, height: int, max_depth: int):
        check(self._lib.pupil_world_set_film(self._h, width, height, max_depth))

    def set_sensor(self, fov: float, to_world, fov_axis="x", near_clip=0.01, far_clip=10000.0):
        """Perspective sensor; ``to_world`` is a mitsuba-convention 4x4 (row-major)."""
        m = _f32(to_world, 16)
        check(self._lib.pupil_world_set_sensor(self._h, fov, fov_axis.encode(), near_clip, far_clip, _ptr(m)))

    def add_mesh(self, positions, indices, normals=None, texcoords=None) -> int:
        p = _f32(positions)
        i = np.ascontiguousarray(np.asarray(indices, dtype=np.uint32).reshape(-1))
        n = _f32(normals) if normals is not None else None
        t = _f32(texcoords) if texcoords is not None else None
        nv, nf = p.size // 3, i.size // 3
        out = C.c_uint32()
        check(self._lib.pupil_world_add_mesh(self._h, nv, nf, _ptr(p), _ptr(n), _ptr(t), _ptr(i, C.c_uint32),
                                             C.byref(out)))
        return out.value

    def add_builtin(self, name: str) -> int:
        out = C.c_uint32()
        check(self._lib.pupil_world_add_builtin_shape(self._h, name.encode(), C.byref(out)))
        return out.value

    def add_material(self, m: abi.Material) -> int:
        out = C.c_uint32()
        check(self._lib.pupil_world_add_material(self._h, C.byref(m), C.byref(out)))
        return out.value

    def add_instance(self, shape: int, material: int, to_world=None, flip_normals=False, flip_tex_coords=False,
                     emitter_radiance=None) -> int:
        m = _f32(identity4() if to_world is None else to_world, 16)
        rad = _tex(emitter_radiance) if emitter_radiance is not None else None
        out = C.c_uint32()
        check(self._lib.pupil_world_add_instance(self._h, shape, material, _ptr(m), int(flip_normals),
                                                 int(flip_tex_coords), int(rad is not None),
                                                 C.byref(rad) if rad is not None else None, C.byref(out)))
        self._desc = None
        return out.value

    def remove_instance(self, instance: int):
        """Remove instance `instance` (index into desc().instances); later instances shift down by
        one, their visibility masks with them.  The next desc() is that of a world built without
        it; PTPass.set_instances hands the new table to the engine."""
        check(self._lib.pupil_world_remove_instance(self._h, int(instance)))
        self._desc = None

    def set_instance_transform(self, instance: int, to_world):
        """Move instance `instance` (index into desc().instances); the next desc()
        carries the new matrices and area emitters (world/world.cpp:45-54)."""
        m = _f32(to_world, 16)
        check(self._lib.pupil_world_set_instance_transform(self._h, int(instance), _ptr(m)))
        self._desc = None

    def set_material(self, material: int, m: abi.Material):
        """Replace material `material` (index into desc().materials: the world flattens one per
        instance, in instance order); the next desc() carries it, and PTPass.update_material hands
        it to the engine.  Bitmap texels are copied by the world."""
        check(self._lib.pupil_world_set_material(self._h, int(material), C.byref(m)))
        self._desc = None

    def set_instance_visibility(self, instance: int, mask: int):
        """RenderObject::visibility_mask of instance `instance` (world/render_object.h:16): visible
        iff mask & 0xFF.  desc() does not change -- a hidden emitter stays in the emitter table,
        as in the reference; PTPass.update_instances hands the mask to the engine."""
        check(self._lib.pupil_world_set_instance_visibility(self._h, int(instance), int(mask) & 0xFFFFFFFF))

    def instance_visibility(self, instance: int) -> int:
        out = C.c_uint32()
        check(self._lib.pupil_world_get_instance_visibility(self._h, int(instance), C.byref(out)))
        return out.value

    def set_mesh_vertices(self, shape: int, positions, normals=None):
        """Deform mesh shape `shape` (index into desc().shapes): new positions, and normals unless
        None (kept).  The vertex count stays.  The next desc() carries the new vertices and the
        area emitters of the shape's emissive instances; PTPass.update_shape hands them to the
        engine."""
        d = self._desc if self._desc is not None else self.desc()
        if not 0 <= int(shape) < d.num_shapes:
            raise abi.PupilError(abi.ERR_INVALID, "shape out of range")
        nv = d.shapes[int(shape)].num_vertices
        p = _f32(positions)
        n = _f32(normals) if normals is not None else None
        if p.size != 3 * nv or (n is not None and n.size != 3 * nv):
            raise ValueError(f"shape {shape} has {nv} vertices")
        check(self._lib.pupil_world_set_mesh_vertices(self._h, int(shape), _ptr(p), _ptr(n)))
        self._desc = None

    def set_mesh(self, shape: int, positions, indices, normals=None, texcoords=None, allow_emissive: bool = False):
        """Replace mesh shape `shape` (index into desc().shapes) by a mesh of new topology: new
        vertex and face counts, normals and texcoords present or not whatever the old mesh had.
        The shape's instances keep material, transform and flags; the next desc() describes the
        scene a fresh engine is created from, and PTPass.replace_shape hands the mesh to the
        engine.  Refuses spheres and, unless allow_emissive, shapes an emissive instance shows.
        allow_emissive (pupil_world_replace_mesh): the next desc() describes the re-meshed emitter
        -- one area emitter per new face, later instances' emitter offsets shifted, new select
        probabilities -- which an engine with device_emitters on follows in place."""
        p = _f32(positions)
        i = np.ascontiguousarray(np.asarray(indices, dtype=np.uint32).reshape(-1))
        n = _f32(normals) if normals is not None else None
        t = _f32(texcoords) if texcoords is not None else None
        nv, nf = p.size // 3, i.size // 3
        if p.size != 3 * nv or i.size != 3 * nf or (n is not None and n.size != 3 * nv) or \
                (t is not None and t.size != 2 * nv):
            raise ValueError(f"arrays do not describe a mesh of {nv} vertices and {nf} faces")
        if allow_emissive:
            check(self._lib.pupil_world_replace_mesh(self._h, int(shape), nv, nf, _ptr(p), _ptr(n), _ptr(t),
                                                     _ptr(i, C.c_uint32), abi.WORLD_MESH_EMISSIVE_OK))
        else:
            check(self._lib.pupil_world_set_mesh(self._h, int(shape), nv, nf, _ptr(p), _ptr(n), _ptr(t),
                                                 _ptr(i, C.c_uint32)))
        self._desc = None

    def add_const_env(self, radiance):
        r = _f32(radiance, 3)
        check(self._lib.pupil_world_add_const_env(self._h, _ptr(r)))

    # ---- delta lights (PUPIL_EMITTER_POINT / _SPOT / _DIRECTIONAL in include/pupil_pt.h)
    def _add_light(self, e: abi.Emitter) -> int:
        out = C.c_uint32()
        check(self._lib.pupil_world_add_delta_emitter(self._h, C.byref(e), C.byref(out)))
        self._desc = None
        return out.value

    def add_point_light(self, position, intensity) -> int:
        """A point light of `intensity` (rgb, per steradian) at `position`.  Returns the light's
        number for set_light(): lights count in order of addition, whatever their types."""
        e = abi.Emitter()
        e.type = abi.EMITTER_POINT
        e.center[:] = tuple(_f32(position, 3))
        e.color[:] = tuple(_f32(_rgb3(intensity), 3))
        return self._add_light(e)

    def add_spot_light(self, position, direction, intensity, cutoff_deg=20.0, beam_deg=None) -> int:
        """A spot light shining along `direction` (normalised by the world): the point light times
        mitsuba's falloff -- full inside beam_deg (default 3/4 of the cutoff) off the axis, zero
        beyond cutoff_deg, linear in the angle between."""
        e = abi.Emitter()
        e.type = abi.EMITTER_SPOT
        e.center[:] = tuple(_f32(position, 3))
        e.nrm[0][:] = tuple(_f32(direction, 3))
        e.color[:] = tuple(_f32(_rgb3(intensity), 3))
        e.pos[0][0] = _radians(cutoff_deg)
        e.pos[0][1] = _radians(0.75 * cutoff_deg if beam_deg is None else beam_deg)
        return self._add_light(e)

    def add_directional_light(self, direction, irradiance) -> int:
        """A directional light travelling along `direction`, `irradiance` (rgb) on a plane that
        faces it."""
        e = abi.Emitter()
        e.type = abi.EMITTER_DIRECTIONAL
        e.nrm[0][:] = tuple(_f32(direction, 3))
        e.color[:] = tuple(_f32(_rgb3(irradiance), 3))
        return self._add_light(e)

    def light(self, light: int) -> abi.Emitter:
        """Light `light` as the world holds it (pupil_world_get_delta_emitter)."""
        e = abi.Emitter()
        check(self._lib.pupil_world_get_delta_emitter(self._h, int(light), C.byref(e)))
        return e

    def set_light(self, light: int, **fields):
        """Change fields of light `light`: position, direction, intensity (or irradiance: the same
        field), cutoff_deg, beam_deg, and type (abi.EMITTER_POINT <-> EMITTER_SPOT only; a light
        cannot cross between point / spot and directional).  Unnamed fields stay.  The next desc()
        carries the light; PTPass.update_lights hands it to the engine."""
        e = self.light(light)
        unknown = set(fields) - {"position", "direction", "intensity", "irradiance", "cutoff_deg", "beam_deg", "type"}
        if unknown:
            raise ValueError(f"unknown light field(s): {', '.join(sorted(unknown))}")
        if "type" in fields:
            e.type = int(fields["type"])
        if "position" in fields:
            e.center[:] = tuple(_f32(fields["position"], 3))
        if "direction" in fields:
            e.nrm[0][:] = tuple(_f32(fields["direction"], 3))
        for name in ("intensity", "irradiance"):
            if name in fields:
                e.color[:] = tuple(_f32(_rgb3(fields[name]), 3))
        if "cutoff_deg" in fields:
            e.pos[0][0] = _radians(fields["cutoff_deg"])
            if "beam_deg" not in fields and e.pos[0][1] == 0.0:  # a point turned spot: mitsuba's default
                e.pos[0][1] = _radians(0.75 * fields["cutoff_deg"])
        if "beam_deg" in fields:
            e.pos[0][1] = _radians(fields["beam_deg"])
        if e.type == abi.EMITTER_POINT:  # a point names neither axis nor angles
            e.nrm[0][:] = (0.0, 0.0, 0.0)
            e.pos[0][:] = (0.0, 0.0, 0.0)
        check(self._lib.pupil_world_set_delta_emitter(self._h, int(light), C.byref(e)))
        self._desc = None

    def desc(self) -> abi.SceneDesc:
        """Flattened scene (pointers owned by the world; valid until it changes)."""
        d = abi.SceneDesc()
        check(self._lib.pupil_world_get_desc(self._h, C.byref(d)))
        d._owner = self  # the arrays live in this world: keep it alive with the desc
        self._desc = d
        return d


def transform(scale=(1.0, 1.0, 1.0), rotate=None, translate=(0.0, 0.0, 0.0)):
    """Transform::Scale -> Rotate -> Translate, each left-multiplied (util_loader.cpp:182-198)."""
    m = np.diag([scale[0], scale[1], scale[2], 1.0]).astype(np.float64)
    if rotate is not None:
        axis, angle = rotate
        u = np.asarray(axis, dtype=np.float64)
        u = u / np.linalg.norm(u)
        th = np.deg2rad(angle)
        a, (b, c, d) = np.cos(0.5 * th), np.sin(0.5 * th) * u
        r = np.array([[1 - 2 * c * c - 2 * d * d, 2 * b * c - 2 * a * d, 2 * a * c + 2 * b * d, 0],
                      [2 * b * c + 2 * a * d, 1 - 2 * b * b - 2 * d * d, 2 * c * d - 2 * a * b, 0],
                      [2 * b * d - 2 * a * c, 2 * a * b + 2 * c * d, 1 - 2 * b * b - 2 * c * c, 0],
                      [0, 0, 0, 1]])
        m = r @ m
    t = np.eye(4)
    t[:3, 3] = translate
    return (t @ m).astype(np.float32)


def look_at_mitsuba(origin, target, up):
    """Mitsuba look-at to_world (+X left, +Z view) as a 4x4, for set_sensor()."""
    o, t, u = (np.asarray(v, dtype=np.float64) for v in (origin, target, up))
    f = t - o
    f /= np.linalg.norm(f)
    left = np.cross(u, f)
    left /= np.linalg.norm(left)
    nu = np.cross(f, left)
    m = np.eye(4)
    m[:3, 0], m[:3, 1], m[:3, 2], m[:3, 3] = left, nu, f, o
    return m.astype(np.float32)
