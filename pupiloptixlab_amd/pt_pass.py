"""Host-side mirror of the reference's pass API for the path tracer.

Reference surface (the drop-in boundary):
  * ``Pupil::Pass`` (framework/system/pass.h:22-39): ``run()`` times ``on_run()``.
  * ``Pupil::pt::PTPass`` (example/path_tracer/pt_pass.h:21-40,
    pt_pass.cpp:29-237): ``set_scene(world)``, ``on_run()``, the inspector
    knobs ``max_depth`` (clamped 1..128) and ``accumulate``; camera / instance
    events mark it dirty, which resets ``random_seed`` and ``sample_cnt``.
  * ``BufferManager`` (framework/system/buffer.h:44-63): named device buffers
    ("final result", "pt accum buffer", "albedo", "normal", "test"; "motion vector"
    once ``motion_vectors()`` was called).
  * ``System`` (framework/system/system.h:22-41), headless: ``add_pass``,
    ``set_scene``, ``run(frames)``.

The work itself happens in libpupil_pt.so through the C ABI
(include/pupil_pt.h); this module only owns buffers and frame counters.
There is no CPU fallback: without a HIP device ``PTPass`` raises.
"""
from __future__ import annotations

import ctypes as C
import time
from collections import defaultdict

from . import abi
from .abi import check, load_library

FINAL_RESULT = "final result"  # BufferManager::DEFAULT_FINAL_RESULT_BUFFER_NAME

# outputs of a ray query (the fields of pupil_ray_hits): channels and f(loat32) / i(nt32)
QUERY_OUTPUTS = {"hit": (4, "f"), "instance": (1, "i"), "primitive": (1, "i"), "material": (1, "i"),
                 "position": (3, "f"), "normal": (3, "f"), "texcoord": (2, "f")}
QUERY_WANT_ALL = tuple(QUERY_OUTPUTS)
# outputs of radiance() (the fields of pupil_ray_radiance): float32 channels
RADIANCE_OUTPUTS = {"radiance": 4, "albedo": 3, "normal": 3}


def camera_ray(s2c, c2w, width, height, x, y, jitter=(0.5, 0.5)):
    """The camera ray through pixel (x, y) at film jitter `jitter` as 8 float32 (o, d, tmin, tmax
    of a camera ray), computed in float32 in the engine's order of operations (camera_path):
    s2c, c2w are the (4, 4) sample_to_camera and camera_to_world."""
    import numpy as np

    f = np.float32

    def dot(a, b):
        acc = f(a[0]) * f(b[0])
        for k in range(1, len(a)):
            acc = f(acc + f(a[k]) * f(b[k]))
        return acc

    def normalize(v):
        inv = f(1.0) / np.sqrt(dot(v, v))
        return [f(c * inv) for c in v]

    film = [f(f(f(x) + f(jitter[0])) / f(width)), f(f(f(y) + f(jitter[1])) / f(height)), f(0.0), f(1.0)]
    d = [dot(s2c[r], film) for r in range(4)]
    inv_w = f(1.0) / d[3]
    d = normalize([f(d[0] * inv_w), f(d[1] * inv_w), f(d[2] * inv_w), f(0.0)])
    d = normalize([dot(c2w[r], d) for r in range(3)])
    return np.array([c2w[0][3], c2w[1][3], c2w[2][3], d[0], d[1], d[2], 0.001, 1e16], np.float32)


class Events:
    """util::Event dispatcher subset: CameraChange / RenderInstanceUpdate / SceneLoad."""

    CAMERA_CHANGE = "CameraChange"
    RENDER_INSTANCE_UPDATE = "RenderInstanceUpdate"
    SCENE_LOAD = "SceneLoad"

    def __init__(self):
        self._subs = defaultdict(list)

    def bind(self, event, fn):
        self._subs[event].append(fn)

    def dispatch(self, event, payload=None):
        for fn in self._subs[event]:
            fn(payload)


class BufferManager:
    """Named device buffers (float tensors on the pass's device)."""

    def __init__(self, device: str):
        import torch

        self._torch = torch
        self.device = device
        self.buffers = {}

    def alloc(self, name: str, count: int, channels: int):
        t = self._torch.zeros((count, channels), dtype=self._torch.float32, device=self.device)
        self.buffers[name] = t
        return t

    def get(self, name: str):
        return self.buffers[name]


class Pass:
    """Pupil::Pass: run() = timed on_run() (pass.cpp:6-11)."""

    def __init__(self, name: str):
        self.name = name
        self.last_ms = 0.0

    def run(self):
        t0 = time.perf_counter()
        self.on_run()
        self.last_ms = (time.perf_counter() - t0) * 1e3

    def on_run(self):  # pragma: no cover - abstract
        raise NotImplementedError


def _material_key(m) -> bytes:
    """What a material holds, without addresses: the struct with its texel pointers cleared, then
    the texels of its bitmap textures.  Equal for equal materials of separately built worlds."""
    import hashlib

    c = abi.Material()
    C.memmove(C.byref(c), C.byref(m), C.sizeof(abi.Material))
    h = hashlib.sha1()
    for k in range(4):
        t = c.tex[k]
        if t.rgba and t.width and t.height:
            h.update(C.string_at(t.rgba, 16 * t.width * t.height))
        t.rgba = None
    return bytes(c) + h.digest()


class PTPass(Pass):
    def __init__(self, name: str = "Path Tracing", device: int = 0, events: Events | None = None):
        super().__init__(name)
        import torch

        if not torch.cuda.is_available():
            raise RuntimeError("PTPass needs a HIP device (no CPU fallback)")
        self._torch = torch
        self._lib = load_library()
        self.device_index = device
        self.device = f"cuda:{device}"
        self.buffers = BufferManager(self.device)
        self._pt = C.c_void_p()
        self.width = self.height = 0
        self.scene_max_depth = 1
        self._max_depth = 1
        self._accumulate = True
        self.random_seed = 0
        self.sample_cnt = 0
        self.dirty = True
        self.tile = (32, 0, 1)  # tile_size, rank, world
        self._world = None  # the World the scene came from: its sensor is re-read when dirty
        self._shape_verts = []  # vertices of each shape of the scene in the engine (update_shape_device)
        self._mat_slots = {}  # the engine's material slots by content (set_instances), and each slot's content
        self._mat_keys = []
        self._pending = {}  # RenderInstanceUpdate events since the last render: id(world) -> (world, instances)
        # what motion_vectors() compares against: the camera in the engine and those of the last
        # two renders as (sample_to_camera, camera_to_world), the instance transforms now in the
        # engine and, if any moved since the render before the last one, the transforms before
        # that ((n, 12) float32)
        self._cam = self._last_cam = self._prev_cam = None
        self._to_world = self._prev_to_world = None
        self._moved = False  # update_instances ran since the last render
        # flow of deforming meshes: the shapes updated with keep_previous since the last render
        # (their snapshot, the first "before", stays), and whether the engine holds snapshots
        self._kept = set()
        self._snapshots = False
        self.events = events or Events()
        self.events.bind(Events.CAMERA_CHANGE, lambda _: self.mark_dirty())
        self.events.bind(Events.RENDER_INSTANCE_UPDATE, self._on_instance_update)
        self.events.bind(Events.SCENE_LOAD, lambda w: self.set_scene(w))

    def _on_instance_update(self, arg):
        """RenderInstanceUpdate handler: only records the moved instance and marks the pass
        dirty, like the reference's (pt_pass.cpp:216-218); the next render refits once
        for every instance recorded since the last one (GetIASHandle(2, true), :46)."""
        if arg is not None:
            world, instance = arg
            self._pending.setdefault(id(world), (world, set()))[1].add(int(instance))
        self.mark_dirty()

    def update_instance(self, world, instance: int):
        """RenderInstanceUpdate applied now: push instance `instance`'s new transform from
        `world` (already moved with World.set_instance_transform) into the engine, and the
        emitter table when the instance is emissive; restarts accumulation."""
        self.update_instances(world, [instance])

    def update_instances(self, world, instances):
        """Several moved, hidden or shown instances with ONE refit of the acceleration
        structure: their transforms and visibility masks as the world holds them
        (pupil_pt_update_instances_masked, IASManager::UpdateInstance), then the emitter table
        if any of them emits (a hidden emitter stays in it, as in the reference).  With
        device_emitters on the engine has rebuilt the table itself and nothing is uploaded."""
        import numpy as np

        ids = sorted({int(i) for i in instances})
        if not ids:
            return
        desc = world.desc()
        tw = np.array([list(desc.instances[i].to_world) for i in ids], np.float32)
        to = np.array([list(desc.instances[i].to_object) for i in ids], np.float32)
        idv = np.array(ids, np.uint32)
        vis = np.array([world.instance_visibility(i) if hasattr(world, "instance_visibility") else 1 for i in ids],
                       np.uint32)
        check(self._lib.pupil_pt_update_instances_masked(self._pt, len(ids),
                                                         idv.ctypes.data_as(C.POINTER(C.c_uint32)),
                                                         tw.ctypes.data_as(C.POINTER(C.c_float)),
                                                         to.ctypes.data_as(C.POINTER(C.c_float)),
                                                         vis.ctypes.data_as(C.POINTER(C.c_uint32))))
        if self._to_world is not None:
            if not self._moved:  # several updates before one render: the first one's "before" stays
                self._prev_to_world = self._to_world.copy()
                self._moved = True
            self._to_world[ids] = tw
        if not self.device_emitters and any(desc.instances[i].emitter_offset >= 0 for i in ids):
            check(self._lib.pupil_pt_update_emitters(self._pt, C.byref(desc)))
        self.dirty = True

    def update_instances_device(self, to_world, ids=None, to_object=None, stream=None):
        """Instances moved from device tensors with ONE refit (pupil_pt_update_instances_device):
        entry k of `to_world` (float32, contiguous, 12 per entry: row-major 3x4) moves instance
        ids[k] (int32 / uint32, distinct; None: instance k).  to_object: the inverses the world
        would compute, or None = the engine inverts on the device, bit for bit the world's.  The
        tensors are read in place after the work enqueued so far on `stream` (default: the current
        stream); no matrix passes through the host on its way in.  Visibility stays; an emissive
        instance needs device_emitters on (PUPIL_ERR_UNSUPPORTED otherwise: use update_instances).
        motion_vectors() after the next render covers the move; restarts accumulation."""
        torch = self._torch
        if not self._pt:
            raise abi.PupilError(abi.ERR_INVALID, "no scene set")
        if to_world is None:
            raise abi.PupilError(abi.ERR_INVALID, "null argument")
        ints = (torch.int32, getattr(torch, "uint32", torch.int32))
        for t, kinds in ((to_world, (torch.float32,)), (ids, ints), (to_object, (torch.float32,))):
            if t is None:
                continue
            if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype in kinds and t.is_contiguous()):
                raise ValueError("update_instances_device needs contiguous float32 (matrices) and int32 or uint32 "
                                 "(ids) device tensors")
            if t.device.index != self.device_index:  # the kernels read them on the engine's GPU
                raise ValueError(f"update_instances_device needs tensors on {self.device}, got {t.device}")
        n = int(ids.numel()) if ids is not None else to_world.numel() // 12
        if to_world.numel() != 12 * n or (to_object is not None and to_object.numel() != 12 * n):
            raise ValueError(f"update_instances_device needs 12 floats per entry for {n} entries")
        s = stream if stream is not None else torch.cuda.current_stream(self.device_index)
        check(self._lib.pupil_pt_update_instances_device(
            self._pt, n, C.c_void_p(ids.data_ptr()) if ids is not None and n else None,
            C.c_void_p(to_world.data_ptr()), C.c_void_p(to_object.data_ptr()) if to_object is not None else None,
            C.c_void_p(s.cuda_stream)))
        if self._to_world is not None and n:
            if not self._moved:  # several updates before one render: the first one's "before" stays
                self._prev_to_world = self._to_world.copy()
                self._moved = True
            self._to_world = self.instance_transforms()[0]
        self.dirty = True

    def instance_transforms(self):
        """The engine's host mirror of every instance's (to_world, to_object), (n, 12) float32 each
        (pupil_pt_get_instance_transforms), whichever update path wrote it."""
        import numpy as np

        n = 0 if self._to_world is None else len(self._to_world)
        tw, to = np.zeros((n, 12), np.float32), np.zeros((n, 12), np.float32)
        check(self._lib.pupil_pt_get_instance_transforms(self._pt, 0, n, tw.ctypes.data_as(abi.f32p),
                                                         to.ctypes.data_as(abi.f32p)))
        return tw, to

    def instances_device_info(self) -> dict:
        """Device instance updates since the scene was set: calls, instances moved, ids skipped as
        out of range, and the kernel launches, synchronisations and host time of the last call."""
        u = [C.c_uint64(0) for _ in range(3)]
        la, sy, ms = C.c_uint32(0), C.c_uint32(0), C.c_double(0.0)
        check(self._lib.pupil_pt_instances_device_info(self._pt, *[C.byref(x) for x in u], C.byref(la), C.byref(sy),
                                                       C.byref(ms)))
        return {"updates": u[0].value, "instances": u[1].value, "skipped": u[2].value, "last_launches": la.value,
                "last_syncs": sy.value, "last_ms": ms.value}

    def _keep_previous(self, shape: int):
        """The vertices `shape` has now become its "previous" vertices for motion_vectors()
        (pupil_pt_snapshot_shape_vertices), unless an update since the last render already kept
        them: like _prev_to_world, the first "before" stays.  The first kept update after a render
        forgets the snapshots of the frame before, so only the shapes deformed since that render
        carry vertex flow."""
        if shape in self._kept:
            return
        if not self._kept and self._snapshots:
            check(self._lib.pupil_pt_clear_vertex_snapshots(self._pt))
            self._snapshots = False
        check(self._lib.pupil_pt_snapshot_shape_vertices(self._pt, shape))
        self._kept.add(shape)
        self._snapshots = True

    def update_shape(self, world, shape: int, rebuild: bool = False, keep_previous: bool = False):
        """Deformed mesh applied now: the vertices `world` holds for `shape` (World.set_mesh_vertices)
        go into the engine with ONE refit over every instance of the shape
        (pupil_pt_update_shape_vertices; rebuild: PUPIL_VERTS_REBUILD), then the emitter table if
        an instance of the shape emits (with device_emitters on the engine has rebuilt it itself
        and nothing is uploaded); restarts accumulation.  keep_previous: the engine keeps
        the vertices from before, and motion_vectors() after the next render covers the
        deformation."""
        desc = world.desc()
        sh = desc.shapes[int(shape)] if 0 <= int(shape) < desc.num_shapes else None
        if keep_previous:
            self._keep_previous(int(shape))
        check(self._lib.pupil_pt_update_shape_vertices(
            self._pt, int(shape), C.cast(sh.positions, C.c_void_p) if sh is not None else None,
            C.cast(sh.normals, C.c_void_p) if sh is not None and sh.normals else None,
            abi.VERTS_REBUILD if rebuild else 0, None))
        if not self.device_emitters and any(
                desc.instances[i].shape == int(shape) and desc.instances[i].emitter_offset >= 0
                for i in range(desc.num_instances)):
            check(self._lib.pupil_pt_update_emitters(self._pt, C.byref(desc)))
        self.dirty = True

    def update_shape_device(self, shape: int, positions, normals=None, rebuild: bool = False, stream=None,
                            keep_previous: bool = False):
        """The same from device tensors (float32, contiguous, 3 per vertex, on the pass's device):
        the copy into the engine's arrays is ordered after the work enqueued so far on `stream`
        (default: the current stream) and never passes through the host.  A shape with an
        emissive instance needs device_emitters on: the engine then rebuilds the emitter table from
        the new vertices on the device; with it off such a shape raises PUPIL_ERR_UNSUPPORTED (use
        update_shape).  keep_previous: as update_shape's."""
        torch = self._torch
        if not self._pt:
            raise abi.PupilError(abi.ERR_INVALID, "no scene set")
        if not 0 <= int(shape) < len(self._shape_verts):
            raise abi.PupilError(abi.ERR_INVALID, "shape index out of range")
        if positions is None:
            raise abi.PupilError(abi.ERR_INVALID, "null argument")
        for t in (positions, normals):
            if t is None:
                continue
            if t.numel() != 3 * self._shape_verts[int(shape)]:
                raise ValueError(f"shape {shape} has {self._shape_verts[int(shape)]} vertices")
            if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
                raise ValueError("update_shape_device needs contiguous float32 device tensors")
            if t.device.index != self.device_index:  # the copy runs device to device on the engine's GPU
                raise ValueError(f"update_shape_device needs tensors on {self.device}, got {t.device}")
        s = stream if stream is not None else torch.cuda.current_stream(self.device_index)
        flags = abi.VERTS_DEVICE | (abi.VERTS_REBUILD if rebuild else 0)
        if keep_previous:
            self._keep_previous(int(shape))
        check(self._lib.pupil_pt_update_shape_vertices(
            self._pt, int(shape), C.c_void_p(positions.data_ptr()),
            C.c_void_p(normals.data_ptr()) if normals is not None else None, flags, C.c_void_p(s.cuda_stream)))
        self.dirty = True

    # ---- a mesh of new topology in place (pupil_pt_replace_shape_mesh)
    def _replace(self, shape: int, nv: int, nf: int, ptrs, flags: int, stream):
        if not self._pt:
            raise abi.PupilError(abi.ERR_INVALID, "no scene set")
        mesh = abi.Shape()
        mesh.kind = abi.SHAPE_MESH
        mesh.num_vertices, mesh.num_faces = nv, nf
        mesh.positions = C.cast(ptrs[0], abi.f32p)
        mesh.normals = C.cast(ptrs[1], abi.f32p)
        mesh.texcoords = C.cast(ptrs[2], abi.f32p)
        mesh.indices = C.cast(ptrs[3], abi.u32p)
        check(self._lib.pupil_pt_replace_shape_mesh(self._pt, int(shape) & 0xFFFFFFFF, C.byref(mesh), flags, stream))
        if 0 <= int(shape) < len(self._shape_verts):
            self._shape_verts[int(shape)] = nv
        self._kept.discard(int(shape))  # the engine dropped the shape's vertex snapshot
        self.dirty = True

    def replace_shape(self, shape: int, positions, faces, normals=None, texcoords=None):
        """Mesh shape `shape` replaced by a mesh of new topology, from host arrays: positions
        (nv, 3) float32, faces (nf, 3) uint32, optional normals (nv, 3) and texcoords (nv, 2), each
        present or not whatever the old mesh had.  Every instance of the shape shows the new mesh
        and the engine equals one created on the updated scene (World.set_mesh keeps the world in
        step).  The whole acceleration structure is rebuilt; the shape's vertex snapshot is
        dropped; restarts accumulation.  A shape an emissive instance shows needs device_emitters
        on: the engine then rebuilds its emitter table at the new size (World.set_mesh with
        allow_emissive=True keeps the world in step).  Refused, with the engine untouched: spheres,
        shapes an emissive instance shows with device_emitters off (PUPIL_ERR_UNSUPPORTED), an
        index >= nv."""
        import numpy as np

        p = np.ascontiguousarray(np.asarray(positions, np.float32).reshape(-1))
        f = np.ascontiguousarray(np.asarray(faces, np.uint32).reshape(-1))
        n = np.ascontiguousarray(np.asarray(normals, np.float32).reshape(-1)) if normals is not None else None
        t = np.ascontiguousarray(np.asarray(texcoords, np.float32).reshape(-1)) if texcoords is not None else None
        nv, nf = p.size // 3, f.size // 3
        if p.size != 3 * nv or f.size != 3 * nf or (n is not None and n.size != 3 * nv) or \
                (t is not None and t.size != 2 * nv):
            raise ValueError(f"arrays do not describe a mesh of {nv} vertices and {nf} faces")
        ptrs = [C.c_void_p(a.ctypes.data) if a is not None else None for a in (p, n, t, f)]
        self._replace(shape, nv, nf, ptrs, 0, None)

    def replace_shape_device(self, shape: int, positions, faces, normals=None, texcoords=None, stream=None):
        """The same from device tensors on the pass's device, all contiguous: positions / normals
        float32 with 3 per vertex, texcoords float32 with 2 per vertex, faces int32 or uint32 with
        3 per face.  They are read in place after the work enqueued so far on `stream` (default:
        the current stream) and copied into arrays the engine owns; no vertex or index passes
        through the host (the index check is a reduction on the device)."""
        torch = self._torch
        if positions is None or faces is None:
            raise abi.PupilError(abi.ERR_INVALID, "null argument")
        ints = (torch.int32, getattr(torch, "uint32", torch.int32))
        for t, kinds in ((positions, (torch.float32,)), (faces, ints), (normals, (torch.float32,)),
                         (texcoords, (torch.float32,))):
            if t is None:
                continue
            if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype in kinds and t.is_contiguous()):
                raise ValueError("replace_shape_device needs contiguous float32 (vertices) and int32 or uint32 "
                                 "(faces) device tensors")
            if t.device.index != self.device_index:  # the copies run device to device on the engine's GPU
                raise ValueError(f"replace_shape_device needs tensors on {self.device}, got {t.device}")
        nv, nf = positions.numel() // 3, faces.numel() // 3
        if positions.numel() != 3 * nv or faces.numel() != 3 * nf or \
                (normals is not None and normals.numel() != 3 * nv) or \
                (texcoords is not None and texcoords.numel() != 2 * nv):
            raise ValueError(f"tensors do not describe a mesh of {nv} vertices and {nf} faces")
        s = stream if stream is not None else torch.cuda.current_stream(self.device_index)
        ptrs = [C.c_void_p(t.data_ptr()) if t is not None else None for t in (positions, normals, texcoords, faces)]
        self._replace(shape, nv, nf, ptrs, abi.VERTS_DEVICE, C.c_void_p(s.cuda_stream))

    def prim_tables(self) -> dict:
        """(tests) The device's primitive -> instance tables (pupil_debug_read_prim_tables)."""
        import numpy as np

        c = [C.c_uint32(0) for _ in range(3)]
        check(self._lib.pupil_debug_read_prim_tables(self._pt, *[C.byref(x) for x in c], None, None, None))
        prim_inst = np.zeros(max(1, c[0].value), np.uint32)
        inst_first = np.zeros(len(self._to_world) + 1, np.uint32)
        inst_guide = np.zeros(c[2].value, np.uint32)
        check(self._lib.pupil_debug_read_prim_tables(self._pt, None, None, None, prim_inst.ctypes.data_as(abi.u32p),
                                                     inst_first.ctypes.data_as(abi.u32p),
                                                     inst_guide.ctypes.data_as(abi.u32p)))
        return {"num_prims": c[0].value, "guide_shift": c[1].value, "prim_inst": prim_inst[:c[0].value],
                "inst_first": inst_first, "inst_guide": inst_guide}

    # ---- the instance table as a whole (pupil_pt_set_instances)
    def _index_materials(self):
        """content -> the first engine slot that holds it"""
        self._mat_slots = {}
        for i, key in enumerate(self._mat_keys):
            self._mat_slots.setdefault(key, i)

    def _bindings(self, world):
        """the world's instances as the engine binds them: a copy of desc().instances whose material
        ids name the ENGINE's material slots (a world's desc carries one material per instance; the
        engine keeps those it was created with), and the world's visibility masks"""
        import numpy as np

        desc = world.desc()
        n = desc.num_instances
        arr = (abi.Instance * max(1, n))()
        for i in range(n):
            C.memmove(C.byref(arr[i]), C.byref(desc.instances[i]), C.sizeof(abi.Instance))
            key = _material_key(desc.materials[desc.instances[i].material])
            if key not in self._mat_slots:
                raise ValueError(f"instance {i} uses a material the engine does not hold: materials are not added "
                                 "to a live engine")
            arr[i].material = self._mat_slots[key]
        vis = np.array([world.instance_visibility(i) for i in range(n)], np.uint32)
        return n, arr, vis

    def _after_set_instances(self, world):
        """what the pass itself keeps per instance"""
        self._world = world
        self._pending = {}
        import numpy as np

        self._to_world = np.zeros((world.desc().num_instances, 12), np.float32)  # sizes instance_transforms()
        self._to_world = self.instance_transforms()[0]
        self._prev_to_world = None
        self._moved = False
        self.dirty = True

    def set_instances(self, world):
        """The engine's instance table becomes the world's (pupil_pt_set_instances, host path):
        instances added with World.add_instance, removed with World.remove_instance, or bound to
        another shape or material of the scene the engine was created on, with the world's
        visibility masks.  Shapes and materials stay.  With device_emitters on
        (pupil_pt_set_instances_emitters) the emissive set is free -- lamps added, removed,
        reordered, rebound, moved -- and the engine rebuilds its emitter table at the new size;
        with it off the emitters stay: emissive instances must be the old ones, in order
        (PUPIL_ERR_UNSUPPORTED otherwise).  Restarts accumulation."""
        if not self._pt:
            raise abi.PupilError(abi.ERR_INVALID, "no scene set")
        n, arr, vis = self._bindings(world)
        self._set_instances(world, n, arr, vis, None, 0, None)
        self._after_set_instances(world)

    def _set_instances(self, world, n, arr, vis, to_world, flags, stream):
        """device_emitters on and the world describes the engine's emitter table (the same env
        presence: pupil_pt_emitter_table_info): pupil_pt_set_instances_emitters with the world's desc,
        whose instance array is the _bindings copy -- the emissive set is free.  Otherwise
        pupil_pt_set_instances, which keeps the table: the mode is off, or the engine's emitters were
        set from another description than this world's."""
        src = world.desc()  # its arrays live in the world
        env = bool(src.env) and src.env.contents.type != abi.EMITTER_NONE
        if not self.device_emitters or env != self.emitter_table_info()["has_env"]:
            check(self._lib.pupil_pt_set_instances(self._pt, n, arr, vis.ctypes.data_as(abi.u32p), to_world, flags, stream))
            return
        desc = abi.SceneDesc()
        C.memmove(C.byref(desc), C.byref(src), C.sizeof(abi.SceneDesc))
        desc.instances = C.cast(arr, C.POINTER(abi.Instance))
        check(self._lib.pupil_pt_set_instances_emitters(self._pt, C.byref(desc), vis.ctypes.data_as(abi.u32p), to_world,
                                                        flags, stream))

    def emitter_table_info(self) -> dict:
        """The engine's emitter table: its entries, the triangle and sphere emitters among them, an env or none."""
        n, a, e = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
        check(self._lib.pupil_pt_emitter_table_info(self._pt, C.byref(n), C.byref(a), C.byref(e)))
        return {"emitters": n.value, "true_areas": a.value, "has_env": bool(e.value)}

    def set_instances_device(self, world, to_world, stream=None):
        """As set_instances, with the transforms from `to_world`, an (n, 12) or (n, 3, 4) float32
        CUDA tensor read in place after the work enqueued so far on `stream` (default: the current
        stream) and inverted on the device; shapes, materials, flips and masks from the world."""
        torch = self._torch
        if not self._pt:
            raise abi.PupilError(abi.ERR_INVALID, "no scene set")
        n, arr, vis = self._bindings(world)
        if not (isinstance(to_world, torch.Tensor) and to_world.is_cuda and to_world.dtype == torch.float32 and
                to_world.is_contiguous()):
            raise ValueError("set_instances_device needs a contiguous float32 device tensor")
        if to_world.device.index != self.device_index:
            raise ValueError(f"set_instances_device needs a tensor on {self.device}, got {to_world.device}")
        if to_world.numel() != 12 * n:
            raise ValueError(f"set_instances_device needs 12 floats for each of the world's {n} instances")
        s = stream if stream is not None else torch.cuda.current_stream(self.device_index)
        self._set_instances(world, n, arr, vis, C.c_void_p(to_world.data_ptr()), abi.INSTANCES_DEVICE,
                            C.c_void_p(s.cuda_stream))
        self._after_set_instances(world)

    def set_instances_info(self) -> dict:
        """Instance tables set since the scene was set; of the last one the BLAS builds it ran,
        whether the whole structure was built, and its host time."""
        n, b, w, ms = C.c_uint64(0), C.c_uint32(0), C.c_uint32(0), C.c_double(0.0)
        check(self._lib.pupil_pt_set_instances_info(self._pt, C.byref(n), C.byref(b), C.byref(w), C.byref(ms)))
        return {"calls": n.value, "last_blas_builds": b.value, "last_whole_rebuild": w.value, "last_ms": ms.value}

    def emitter_resize_info(self) -> dict:
        """Emitter tables rebuilt at a new size since the scene was set (set_instances* and
        replace_shape* with device_emitters on), the triangle and sphere emitters of the last one
        and the host time of its call."""
        n, a, ms = C.c_uint64(0), C.c_uint32(0), C.c_double(0.0)
        check(self._lib.pupil_pt_emitter_resize_info(self._pt, C.byref(n), C.byref(a), C.byref(ms)))
        return {"resizes": n.value, "last_true_areas": a.value, "last_ms": ms.value}

    def replace_info(self) -> dict:
        """Meshes replaced since the scene was set and the host time of the last call."""
        n, ms = C.c_uint64(0), C.c_double(0.0)
        check(self._lib.pupil_pt_replace_info(self._pt, C.byref(n), C.byref(ms)))
        return {"replacements": n.value, "last_ms": ms.value}

    def shadow_info(self) -> dict:
        """Shadow rays of the last counter render that found an occluder, the node visits they took,
        and whether any-hit rays use the overlap child order (pupil_pt_shadow_info)."""
        n, v, on = C.c_uint64(0), C.c_uint64(0), C.c_uint32(0)
        check(self._lib.pupil_pt_shadow_info(self._pt, C.byref(n), C.byref(v), C.byref(on)))
        return {"occluded_rays": n.value, "occluded_visits": v.value, "overlap_order": bool(on.value)}

    # ---- materials and textures in place (pupil_pt_update_materials / _update_texture_device)
    def update_material(self, world, material: int):
        """Material `material` as `world` holds it now (World.set_material) goes into the engine;
        restarts accumulation."""
        self.update_materials(world, [material])

    def update_materials(self, world, ids):
        """Several materials in ONE call: desc().materials[i] of `world` for every i in ids.  Any
        field may have changed, the type and the textures' kinds and sizes included; the
        acceleration structure is not touched."""
        import numpy as np

        ids = sorted({int(i) for i in ids})
        if not ids:
            return
        desc = world.desc()
        for i in ids:
            if not 0 <= i < desc.num_materials:
                raise abi.PupilError(abi.ERR_INVALID, "material index out of range")
        mats = (abi.Material * len(ids))()
        for k, i in enumerate(ids):
            C.memmove(C.byref(mats[k]), C.byref(desc.materials[i]), C.sizeof(abi.Material))
        idv = np.array(ids, np.uint32)
        check(self._lib.pupil_pt_update_materials(self._pt, len(ids), idv.ctypes.data_as(C.POINTER(C.c_uint32)), mats))
        for k, i in enumerate(ids):  # set_instances binds materials by what the slots hold now
            if i < len(self._mat_keys):
                self._mat_keys[i] = _material_key(mats[k])
        self._index_materials()
        self.mark_dirty()

    def update_texture_device(self, material: int, slot: int, tensor, stream=None):
        """The texels of bitmap slot `slot` of `material` from a contiguous float32 tensor of shape
        (h, w, 4) on the pass's device; the slot must already be an h x w bitmap
        (update_material sets kinds and sizes).  The copy is ordered after the work enqueued so
        far on `stream` (default: the current stream) and never passes through the host; a
        plastic's sampling weight follows on the device.  Restarts accumulation."""
        torch = self._torch
        if not self._pt:
            raise abi.PupilError(abi.ERR_INVALID, "no scene set")
        if not isinstance(tensor, torch.Tensor):
            raise ValueError("update_texture_device needs a torch tensor")
        if tensor.dim() != 3 or tensor.shape[2] != 4 or tensor.shape[0] == 0 or tensor.shape[1] == 0:
            raise ValueError(f"update_texture_device needs an (h, w, 4) tensor, got {tuple(tensor.shape)}")
        if not (tensor.is_cuda and tensor.dtype == torch.float32 and tensor.is_contiguous()):
            raise ValueError("update_texture_device needs a contiguous float32 device tensor")
        if tensor.device.index != self.device_index:  # the copy runs device to device on the engine's GPU
            raise ValueError(f"update_texture_device needs a tensor on {self.device}, got {tensor.device}")
        s = stream if stream is not None else torch.cuda.current_stream(self.device_index)
        check(self._lib.pupil_pt_update_texture_device(self._pt, int(material), int(slot), C.c_void_p(tensor.data_ptr()),
                                                       int(tensor.shape[1]), int(tensor.shape[0]),
                                                       C.c_void_p(s.cuda_stream)))
        self.mark_dirty()

    def material_info(self) -> dict:
        n, ms = C.c_uint64(0), C.c_double(0.0)
        check(self._lib.pupil_pt_material_info(self._pt, C.byref(n), C.byref(ms)))
        return {"updates": n.value, "last_ms": ms.value}

    def read_material(self, material: int) -> dict:
        """The device's copy of a material (pupil_debug_read_material): type, eta, int_fdr and
        specular_sampling_weight (float32)."""
        import numpy as np

        t = C.c_uint32(0)
        out = np.zeros(3, np.float32)
        check(self._lib.pupil_debug_read_material(self._pt, int(material), C.byref(t), out.ctypes.data_as(abi.f32p)))
        return {"type": t.value, "eta": out[0], "int_fdr": out[1], "specular_sampling_weight": out[2]}

    # ---- the env map in place (pupil_pt_update_env_device / _update_env_params)
    def update_env_device(self, tensor, stream=None):
        """The texels of the env map from a contiguous float32 tensor of shape (h, w, 4) on the
        pass's device; the scene's env must already be an h x w env map (a scene load or
        pupil_pt_update_emitters sets the size).  The copy is ordered after the work enqueued so far
        on `stream` (default: the current stream) and never passes through the host; the map's CDF
        tables follow on the device, bit for bit the host's.  Restarts accumulation."""
        torch = self._torch
        if not self._pt:
            raise abi.PupilError(abi.ERR_INVALID, "no scene set")
        if not isinstance(tensor, torch.Tensor):
            raise ValueError("update_env_device needs a torch tensor")
        if tensor.dim() != 3 or tensor.shape[2] != 4 or tensor.shape[0] == 0 or tensor.shape[1] == 0:
            raise ValueError(f"update_env_device needs an (h, w, 4) tensor, got {tuple(tensor.shape)}")
        if not (tensor.is_cuda and tensor.dtype == torch.float32 and tensor.is_contiguous()):
            raise ValueError("update_env_device needs a contiguous float32 device tensor")
        if tensor.device.index != self.device_index:  # the copy runs device to device on the engine's GPU
            raise ValueError(f"update_env_device needs a tensor on {self.device}, got {tensor.device}")
        s = stream if stream is not None else torch.cuda.current_stream(self.device_index)
        check(self._lib.pupil_pt_update_env_device(self._pt, C.c_void_p(tensor.data_ptr()), int(tensor.shape[1]),
                                                   int(tensor.shape[0]), C.c_void_p(s.cuda_stream)))
        self.mark_dirty()

    def update_env_params(self, scale: float, to_world3x3):
        """scale and rotation of the env map (to_world3x3: 9 floats, row-major) without touching
        its texels or tables.  to_local is the inverse of to_world3x3 as float32, computed on the
        host in float64 by the routine the World uses (pupil_world_invert3x3): a fresh engine's
        to_local comes from the world's own inverse of the emitter's transform, and this is that
        inverse, so the updated engine equals a scene loaded with the same rotation and scale bit
        for bit.  Restarts accumulation."""
        import numpy as np

        if not self._pt:
            raise abi.PupilError(abi.ERR_INVALID, "no scene set")
        tw = np.ascontiguousarray(np.asarray(to_world3x3, np.float32).reshape(-1))
        if tw.size != 9:
            raise ValueError("update_env_params needs a 3 x 3 matrix")
        tl = np.zeros(9, np.float32)
        check(self._lib.pupil_world_invert3x3(tw.ctypes.data_as(abi.f32p), tl.ctypes.data_as(abi.f32p)))
        check(self._lib.pupil_pt_update_env_params(self._pt, float(scale), tw.ctypes.data_as(abi.f32p),
                                                   tl.ctypes.data_as(abi.f32p)))
        self.mark_dirty()

    def env_info(self) -> dict:
        n, ms = C.c_uint64(0), C.c_double(0.0)
        check(self._lib.pupil_pt_env_info(self._pt, C.byref(n), C.byref(ms)))
        return {"updates": n.value, "last_ms": ms.value}

    def env_tables(self) -> dict:
        """The device's env-map tables (pupil_debug_read_env_tables): col_cdf (h, w + 1), row_cdf
        (h + 1,), row_weight (h,) and normalization, float32."""
        import numpy as np

        w, h = C.c_uint32(0), C.c_uint32(0)
        check(self._lib.pupil_debug_read_env_tables(self._pt, C.byref(w), C.byref(h), None, None, None, None))
        col = np.zeros((h.value, w.value + 1), np.float32)
        row = np.zeros(h.value + 1, np.float32)
        weight = np.zeros(h.value, np.float32)
        norm = np.zeros(1, np.float32)
        check(self._lib.pupil_debug_read_env_tables(self._pt, C.byref(w), C.byref(h), col.ctypes.data_as(abi.f32p),
                                                    row.ctypes.data_as(abi.f32p), weight.ctypes.data_as(abi.f32p),
                                                    norm.ctypes.data_as(abi.f32p)))
        return {"width": w.value, "height": h.value, "col_cdf": col, "row_cdf": row, "row_weight": weight,
                "normalization": norm[0]}

    # ---- engine-owned emitter table (pupil_pt_enable_device_emitters)
    @property
    def device_emitters(self):
        """Whether the engine owns the area-emitter table (asked of the engine: an emitter upload
        whose counts no longer match switches the mode off)."""
        return bool(self._pt) and self.device_emitters_info()["enabled"]

    @device_emitters.setter
    def device_emitters(self, v):
        """True: the engine derives the area-emitter table from its own arrays after every
        update of an emissive shape or instance (needs the World the scene came from, whose
        current desc gives the radiance weights); False: the host uploads it, as without the
        mode.  set_scene switches it off."""
        if not self._pt:
            raise abi.PupilError(abi.ERR_INVALID, "no scene set")
        if v:
            if self._world is None:
                raise abi.PupilError(abi.ERR_INVALID, "device_emitters needs a scene set from a World")
            desc = self._world.desc()
            check(self._lib.pupil_pt_enable_device_emitters(self._pt, C.byref(desc)))
        else:
            check(self._lib.pupil_pt_enable_device_emitters(self._pt, None))
        self.dirty = True

    def refresh_emitters(self):
        """pupil_pt_refresh_emitters: the rebuild now (device_emitters on)."""
        check(self._lib.pupil_pt_refresh_emitters(self._pt))
        self.dirty = True

    def update_lights(self, world=None):
        """Point, spot and directional lights added or changed on `world` (default: the World the
        scene came from) since the engine last saw its emitter table: World.add_*_light,
        World.set_light.  Hands the whole table to the engine (pupil_pt_update_emitters), which
        rewrites it in place when no light was added and none changed its type; restarts
        accumulation."""
        world = world if world is not None else self._world
        if world is None:
            raise abi.PupilError(abi.ERR_INVALID, "update_lights needs a scene set from a World")
        if not self._pt:
            raise abi.PupilError(abi.ERR_INVALID, "no scene set")
        desc = world.desc()
        check(self._lib.pupil_pt_update_emitters(self._pt, C.byref(desc)))
        self.dirty = True

    def emitter_sample(self, emitter: int, xi, position, normal):
        """The device's Emitter::SampleDirect of table entry `emitter` (the table's count: the env)
        from one shading point (pupil_debug_emitter_sample): xi (n, 2) in [0, 1].  Returns wi
        (n, 3), pdf (n,), distance (n,), radiance (n, 3)."""
        import numpy as np

        xi = np.asarray(xi, np.float32).reshape(-1, 2)
        n = xi.shape[0]
        inp = np.zeros((max(1, n), 3), np.float32)
        inp[:n, :2] = xi
        pn = np.ascontiguousarray(np.concatenate([np.asarray(position, np.float32).reshape(3),
                                                  np.asarray(normal, np.float32).reshape(3)]))
        out = np.zeros((max(1, n), 8), np.float32)
        check(self._lib.pupil_debug_emitter_sample(self._pt, int(emitter), n, inp.ctypes.data_as(abi.f32p),
                                                   pn.ctypes.data_as(abi.f32p), out.ctypes.data_as(abi.f32p)))
        out = out[:n]
        return {"wi": out[:, 0:3].copy(), "pdf": out[:, 3].copy(), "distance": out[:, 4].copy(),
                "radiance": out[:, 5:8].copy()}

    def device_emitters_info(self) -> dict:
        en, n, ms = C.c_uint32(0), C.c_uint64(0), C.c_double(0.0)
        check(self._lib.pupil_pt_device_emitters_info(self._pt, C.byref(en), C.byref(n), C.byref(ms)))
        return {"enabled": bool(en.value), "refreshes": n.value, "last_ms": ms.value}

    def emitter_table(self):
        """The engine's area-emitter table as numpy arrays (pupil_debug_read_emitters /
        _read_emitter_guide): select_probability, area, cdf (n,), type (n,) uint32, pos and nrm
        (n, 3, 3), guide_bits, and guide ((2^bits + 1,) uint32, or None when the table has none).
        The delta lights follow the area emitters; for one of them pos is (center, color,
        (cutoff, beam, 0)), nrm[0] the axis or direction and area 0."""
        import numpy as np

        cnt = C.c_uint32(0)
        bits = C.c_uint32(0)
        check(self._lib.pupil_debug_read_emitter_guide(self._pt, C.byref(bits), None, C.byref(cnt)))
        guide = None
        if cnt.value:
            guide = np.zeros(cnt.value, np.uint32)
            check(self._lib.pupil_debug_read_emitter_guide(self._pt, C.byref(bits),
                                                           guide.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(cnt)))
        # the count: an empty range is in bounds exactly up to it
        in_bounds = lambda k: self._lib.pupil_debug_read_emitters(self._pt, k, 0, None) == abi.OK
        lo, hi = 0, 1
        while in_bounds(hi):
            lo, hi = hi, 2 * hi
        while hi - lo > 1:
            mid = (lo + hi) // 2
            lo, hi = (mid, hi) if in_bounds(mid) else (lo, mid)
        n = lo
        raw = np.zeros((max(1, n), 24), np.float32)
        if n:
            check(self._lib.pupil_debug_read_emitters(self._pt, 0, n, raw.ctypes.data_as(C.POINTER(C.c_float))))
        raw = raw[:n]
        return {"select_probability": raw[:, 0].copy(), "area": raw[:, 1].copy(), "cdf": raw[:, 2].copy(),
                "type": raw[:, 3].copy().view(np.uint32), "pos": raw[:, 4:13].reshape(n, 3, 3).copy(),
                "nrm": raw[:, 13:22].reshape(n, 3, 3).copy(), "guide_bits": bits.value, "guide": guide}

    # ---- inspector knobs (pt_pass.cpp:225-237)
    @property
    def max_depth(self):
        return self._max_depth

    @max_depth.setter
    def max_depth(self, v):
        v = max(1, min(128, int(v)))
        if v != self._max_depth:
            self._max_depth = v
            self.dirty = True

    @property
    def accumulate(self):
        return self._accumulate

    @accumulate.setter
    def accumulate(self, v):
        if bool(v) != self._accumulate:
            self._accumulate = bool(v)
            self.dirty = True

    def mark_dirty(self):
        self.dirty = True

    def set_tiling(self, tile_size: int, rank: int, world: int):
        """Render only the image tiles t with t % world == rank (multi-GPU sharding)."""
        self.tile = (tile_size, rank, world)
        self._alloc_buffers()

    def local_pixel_count(self):
        ts, rank, world = self.tile
        n = C.c_uint32(0)
        check(self._lib.pupil_pt_local_pixels(self.width, self.height, ts, rank, world, None, C.byref(n)))
        return n.value

    def local_pixels(self):
        import numpy as np

        ts, rank, world = self.tile
        n = C.c_uint32(self.local_pixel_count())
        out = np.zeros(max(1, n.value), dtype=np.uint32)
        check(self._lib.pupil_pt_local_pixels(self.width, self.height, ts, rank, world,
                                              out.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(n)))
        return out[: n.value]

    # ---- PTPass::SetScene (pt_pass.cpp:107-209)
    def set_scene(self, world):
        desc = world.desc() if hasattr(world, "desc") else world
        self._world = world if hasattr(world, "desc") else None
        self.close_engine()
        self._pending = {}
        self._torch.cuda.set_device(self.device_index)
        check(self._lib.pupil_pt_create(C.byref(desc), self.device_index, C.byref(self._pt)))
        self.width, self.height = desc.width, desc.height
        self._shape_verts = [desc.shapes[i].num_vertices for i in range(desc.num_shapes)]
        # the engine's material slots by content, for set_instances (the first slot of equal ones)
        self._mat_slots = {}
        self._mat_keys = [_material_key(desc.materials[i]) for i in range(desc.num_materials)]
        self._index_materials()
        self.scene_max_depth = desc.max_depth
        self._max_depth = desc.max_depth
        self._accumulate = True
        self.random_seed = 0
        self.sample_cnt = 0
        self.dirty = True
        import numpy as np

        self._cam = self._last_cam = self._prev_cam = (list(desc.sample_to_camera), list(desc.camera_to_world))
        self._to_world = np.array([list(desc.instances[i].to_world) for i in range(desc.num_instances)],
                                  np.float32).reshape(-1, 12)
        self._prev_to_world = None
        self._moved = False
        self._alloc_buffers()
        # the engine creates every instance visible: the masks the world remembers go on now
        if self._world is not None and hasattr(self._world, "instance_visibility"):
            hidden = [i for i in range(desc.num_instances) if (self._world.instance_visibility(i) & 0xFF) == 0]
            if hidden:
                idv = np.array(hidden, np.uint32)
                vis = np.zeros(len(hidden), np.uint32)
                check(self._lib.pupil_pt_update_instances_masked(self._pt, len(hidden),
                                                                 idv.ctypes.data_as(C.POINTER(C.c_uint32)), None, None,
                                                                 vis.ctypes.data_as(C.POINTER(C.c_uint32))))

    def _alloc_buffers(self):
        n = self.local_pixel_count() if self.tile[2] > 1 else self.width * self.height
        b = self.buffers
        b.alloc(FINAL_RESULT, n, 4)
        b.alloc("pt accum buffer", n, 4)
        b.alloc("albedo", n, 3)
        b.alloc("normal", n, 3)
        b.alloc("test", n, 1)

    def _frame(self):
        b = self.buffers
        f = abi.Frame()
        f.accum = b.get("pt accum buffer").data_ptr()
        f.frame = b.get(FINAL_RESULT).data_ptr()
        f.albedo = b.get("albedo").data_ptr()
        f.normal = b.get("normal").data_ptr()
        f.test = b.get("test").data_ptr()
        f.compact = 1 if self.tile[2] > 1 else 0
        return f

    def render(self, spp: int = 1, collect_stats: int = 0, stream=None, continues: bool = False):
        """spp consecutive OnRun frames in one wavefront batch (asynchronous).
        collect_stats: bit 0 counters (node visits, ...), bit 1 per-stage HIP events.
        continues: the next render() continues this one (progressive rendering), so the
        engine traces its camera rays ahead (PUPIL_HINT_CONTINUE; single-spp renders
        always do)."""
        if not self._moved:
            self._prev_to_world = None  # no instance moved between the last render and this one
        if not self._kept and self._snapshots:  # nor did a mesh deform: its snapshot is a frame old
            check(self._lib.pupil_pt_clear_vertex_snapshots(self._pt))
            self._snapshots = False
        if self.dirty:  # pt_pass.cpp:40-49: camera re-uploaded, instances refitted, accumulation restarted
            pending, self._pending = self._pending, {}
            for world, ids in pending.values():
                self.update_instances(world, ids)
            if self._world is not None:
                d = self._world.desc()
                check(self._lib.pupil_pt_set_camera(self._pt, d.sample_to_camera, d.camera_to_world))
                self._cam = (list(d.sample_to_camera), list(d.camera_to_world))
            self.random_seed = 0
            self.sample_cnt = 0
            self.dirty = False
        la = abi.Launch()
        la.random_seed = self.random_seed
        la.sample_cnt = self.sample_cnt
        la.spp = spp
        la.max_depth = self._max_depth
        la.accumulate = int(self._accumulate)
        la.tile_size, la.tile_rank, la.tile_world = self.tile
        la.collect_stats = int(collect_stats)
        la.hints = 1 if continues else 0  # PUPIL_HINT_CONTINUE
        s = stream if stream is not None else self._torch.cuda.current_stream(self.device_index)
        f = self._frame()
        check(self._lib.pupil_pt_render(self._pt, C.byref(f), C.byref(la), C.c_void_p(s.cuda_stream)))
        self.random_seed += spp  # pt_pass.cpp:55-56
        if self._accumulate:
            self.sample_cnt += spp
        self._moved = False
        self._kept = set()
        self._prev_cam, self._last_cam = self._last_cam, self._cam  # the views of the last two renders

    def motion_vectors(self, prev_camera=None, prev_to_world=None, stream=None):
        """Screen-space flow (pupil_pt_motion_vectors) into the lazily allocated "motion vector"
        buffer ((n, 2): current minus previous pixel position, NaN = no previous pixel), in the
        index space of the other buffers; returns the buffer.  prev_camera: (sample_to_camera,
        camera_to_world) of the previous frame, 16 floats each; prev_to_world: (num_instances, 12)
        previous instance transforms, or None = no instance moved.  With no arguments both mean
        "since my previous render": the camera of the render before the last one and, if
        instances were moved between the two, the transforms they had before; the vertices of the
        meshes deformed between the two with keep_previous are covered too.  That needs the
        engine to hold what the last render used: after update_instances or a keep_previous
        update, render first (or pass prev_camera and prev_to_world; the vertex motion is then
        that of whatever snapshots the engine holds)."""
        import numpy as np

        if prev_camera is None:
            if self._moved:
                raise RuntimeError("instances were updated since the last render: render before motion_vectors(), "
                                   "or pass prev_camera / prev_to_world")
            if self._kept:
                raise RuntimeError("a mesh was deformed with keep_previous since the last render: render before "
                                   "motion_vectors(), or pass prev_camera")
            prev_camera = self._prev_cam
            if prev_to_world is None:
                prev_to_world = self._prev_to_world
        n = self.local_pixel_count() if self.tile[2] > 1 else self.width * self.height
        mv = self.buffers.buffers.get("motion vector")
        if mv is None or mv.shape[0] != n:
            mv = self.buffers.alloc("motion vector", n, 2)
        s2c = (C.c_float * 16)(*np.asarray(prev_camera[0], np.float32).reshape(16).tolist())
        c2w = (C.c_float * 16)(*np.asarray(prev_camera[1], np.float32).reshape(16).tolist())
        ptw = None
        if prev_to_world is not None:
            ptw_np = np.ascontiguousarray(np.asarray(prev_to_world, np.float32).reshape(-1))
            if ptw_np.size != self._to_world.size:
                raise ValueError("prev_to_world needs 12 floats per instance")
            ptw = ptw_np.ctypes.data_as(C.POINTER(C.c_float))
        ts, rank, world = self.tile
        s = stream if stream is not None else self._torch.cuda.current_stream(self.device_index)
        check(self._lib.pupil_pt_motion_vectors(self._pt, s2c, c2w, ptw, C.c_void_p(mv.data_ptr()),
                                                1 if world > 1 else 0, ts, rank, world, C.c_void_p(s.cuda_stream)))
        return mv

    # ---- ray queries from device memory (pupil_pt_query_rays / _query_camera)
    def _query_outputs(self, n, want, out):
        """The tensors of a query's outputs, (n, channels) each, taken from `out` where it holds a
        fitting one and allocated otherwise, and the pupil_ray_hits that names them."""
        torch = self._torch
        tensors = {}
        hits = abi.RayHits()
        for name in want:
            if name not in QUERY_OUTPUTS:
                raise ValueError(f"unknown query output {name!r} (one of {', '.join(QUERY_OUTPUTS)})")
            channels, kind = QUERY_OUTPUTS[name]
            dtype = torch.float32 if kind == "f" else torch.int32
            shape = (n, channels) if channels > 1 else (n,)
            t = out.get(name) if out else None
            if t is not None:
                if not (isinstance(t, torch.Tensor) and t.is_cuda and t.device.index == self.device_index
                        and t.dtype == dtype and tuple(t.shape) == shape and t.is_contiguous()):
                    raise ValueError(f"out[{name!r}] must be a contiguous {dtype} tensor of shape {shape} on "
                                     f"{self.device}")
            else:
                t = torch.empty(shape, dtype=dtype, device=self.device)
            tensors[name] = t
            setattr(hits, name, t.data_ptr() if n else None)
        return tensors, hits

    def _query_stream(self, stream, tensors):
        """The stream a query runs on.  Tensors allocated on the current stream and written on
        another one are made known to torch's caching allocator (record_stream), so their memory
        is not handed out again before the query has passed it."""
        torch = self._torch
        current = torch.cuda.current_stream(self.device_index)
        s = stream if stream is not None else current
        if s.cuda_stream != current.cuda_stream:
            for t in tensors:
                if t is not None and t.numel():
                    t.record_stream(s)
        return s

    def trace(self, rays, any_hit: bool = False, want=QUERY_WANT_ALL, out=None, stream=None) -> dict:
        """What the rays hit (pupil_pt_query_rays).  rays: (n, 8) contiguous float32 tensor on the
        pass's device, (ox, oy, oz, dx, dy, dz, tmin, tmax) per ray, traced in place.  Returns
        the outputs named in `want` as device tensors: "hit" (n, 4) = t, b1, b2, primitive id
        bits (t = -1 on a miss); "instance", "primitive" (face within the shape), "material" (n,)
        int32, -1 on a miss; "position", "normal" (n, 3) and "texcoord" (n, 2), 0 on a miss.
        any_hit: occlusion only, want = ("hit",), t = 1 or -1.  out: tensors of an earlier call
        to write into.  Asynchronous on `stream` (default: the current stream), after every
        render enqueued so far; nothing of the pass's accumulation changes.  On a stream other
        than the current one the rays and outputs are recorded on it (Tensor.record_stream), and
        the caller orders its own reads behind that stream."""
        torch = self._torch
        if not isinstance(rays, torch.Tensor):
            raise ValueError("trace needs a torch tensor of rays")
        # what the kernels would read out of bounds first, then where the tensor lives
        if rays.dtype != torch.float32:
            raise ValueError(f"trace needs float32 rays, got {rays.dtype}")
        if rays.dim() != 2 or rays.shape[1] != 8:
            raise ValueError(f"trace needs an (n, 8) tensor of rays, got {tuple(rays.shape)}")
        if not rays.is_contiguous():
            raise ValueError("trace needs contiguous rays")
        if not rays.is_cuda or rays.device.index != self.device_index:
            raise ValueError(f"trace needs rays on {self.device}, got a {rays.device} tensor")
        if not self._pt:
            raise abi.PupilError(abi.ERR_INVALID, "no scene set")
        n = int(rays.shape[0])
        if any_hit and want is QUERY_WANT_ALL:
            want = ("hit",)
        tensors, hits = self._query_outputs(n, tuple(want), out)
        if n == 0 and tensors:
            return tensors
        s = self._query_stream(stream, [rays, *tensors.values()])
        check(self._lib.pupil_pt_query_rays(self._pt, n, C.c_void_p(rays.data_ptr()),
                                            abi.QUERY_ANY_HIT if any_hit else 0, C.byref(hits),
                                            C.c_void_p(s.cuda_stream)))
        return tensors

    def primary_hits(self, jitter=(0.5, 0.5), want=QUERY_WANT_ALL, return_rays: bool = False, stream=None) -> dict:
        """The G-buffer (pupil_pt_query_camera): trace()'s outputs for the camera ray through every
        pixel at film jitter `jitter` ((0.5, 0.5) = the pixel centre), in the index space of the
        other buffers (the current tiling, as motion_vectors()).  return_rays: the rays too, as
        "rays" (n, 8).  The camera is the one in the engine (that of the last render)."""
        torch = self._torch
        if not self._pt:
            raise abi.PupilError(abi.ERR_INVALID, "no scene set")
        ts, rank, world = self.tile
        n = self.local_pixel_count() if world > 1 else self.width * self.height
        tensors, hits = self._query_outputs(n, tuple(want), None)
        rays = torch.empty((n, 8), dtype=torch.float32, device=self.device) if return_rays else None
        s = self._query_stream(stream, [rays, *tensors.values()])
        if n:
            check(self._lib.pupil_pt_query_camera(self._pt, float(jitter[0]), float(jitter[1]), 1 if world > 1 else 0,
                                                  ts, rank, world,
                                                  C.c_void_p(rays.data_ptr()) if rays is not None else None,
                                                  C.byref(hits), C.c_void_p(s.cuda_stream)))
        if rays is not None:
            tensors["rays"] = rays
        return tensors

    def pick(self, x: int, y: int):
        """What lies under the centre of pixel (x, y) (row 0 = bottom, as image()): a dict of
        instance, primitive, material (ints) and t (float), or None where the ray leaves the
        scene.  One ray through trace(); waits for the result."""
        import numpy as np

        if not (0 <= int(x) < self.width and 0 <= int(y) < self.height):
            raise ValueError(f"pixel ({x}, {y}) is outside the {self.width} x {self.height} film")
        s2c, c2w = (np.asarray(m, np.float32).reshape(4, 4) for m in self._cam)
        ray = camera_ray(s2c, c2w, self.width, self.height, int(x), int(y))
        rays = self._torch.from_numpy(ray.reshape(1, 8)).to(self.device)
        r = self.trace(rays, want=("hit", "instance", "primitive", "material"))
        t = float(r["hit"][0, 0].item())  # the copy waits for the query
        if int(r["instance"][0].item()) < 0:
            return None
        return {"instance": int(r["instance"][0].item()), "primitive": int(r["primitive"][0].item()),
                "material": int(r["material"][0].item()), "t": t}

    def query_info(self) -> dict:
        q, r, g, ms = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0), C.c_double(0.0)
        check(self._lib.pupil_pt_query_info(self._pt, C.byref(q), C.byref(r), C.byref(g), C.byref(ms)))
        return {"queries": q.value, "rays": r.value, "scratch_grows": g.value, "last_ms": ms.value}

    # ---- path-traced radiance along rays from device memory (pupil_pt_radiance_rays)
    def radiance(self, rays, spp: int = 1, seed: int = 0, sample_cnt: int = 0, accumulate: bool = False,
                 max_depth=None, stream_ids=None, want=("radiance",), out=None, stream=None) -> dict:
        """What the rays see (pupil_pt_radiance_rays): the render's integrator along each ray of an
        (n, 8) contiguous float32 tensor on the pass's device, (ox, oy, oz, dx, dy, dz, tmin, tmax)
        per ray as trace() takes them.  The direction must be unit length; tmin and tmax are
        ignored (every segment uses the path tracer's window [0.001, 1e16]).  Returns the outputs
        named in `want`: "radiance" (n, 4), rgb + 1, always among them; "albedo" and "normal"
        (n, 3), the first hit's AOVs, 0 on a miss.

        Sample s of ray i is a path with the RNG of pixel stream_ids[i] (default: i) at seed
        `seed` + s, so the camera ray a render of that seed draws for that pixel gives that
        render's pixel bit for bit.  spp samples enter "radiance" by the render's running mean
        when `accumulate` is set (count sample_cnt + s; pass the earlier result in
        out["radiance"] to continue it), else the last one stays.  max_depth: None = the
        scene's.  stream_ids: (n,) int32 or uint32 tensor.  out: tensors of an earlier call to
        write into.  Asynchronous on `stream` (default: the current stream), after every render
        enqueued so far; nothing the pass renders changes, and its camera plays no part.  On a
        stream other than the current one the rays, ids and outputs are recorded on it
        (Tensor.record_stream) and the caller orders its own reads and writes of them, as for
        trace(); outputs allocated here are written by the call alone."""
        torch = self._torch
        if not isinstance(rays, torch.Tensor):
            raise ValueError("radiance needs a torch tensor of rays")
        if rays.dtype != torch.float32:
            raise ValueError(f"radiance needs float32 rays, got {rays.dtype}")
        if rays.dim() != 2 or rays.shape[1] != 8:
            raise ValueError(f"radiance needs an (n, 8) tensor of rays, got {tuple(rays.shape)}")
        if not rays.is_contiguous():
            raise ValueError("radiance needs contiguous rays")
        if not rays.is_cuda or rays.device.index != self.device_index:
            raise ValueError(f"radiance needs rays on {self.device}, got a {rays.device} tensor")
        n = int(rays.shape[0])
        if stream_ids is not None:
            if not (isinstance(stream_ids, torch.Tensor) and stream_ids.dtype in (torch.int32, getattr(torch, "uint32", torch.int32))
                    and tuple(stream_ids.shape) == (n,) and stream_ids.is_contiguous() and stream_ids.is_cuda
                    and stream_ids.device.index == self.device_index):
                raise ValueError(f"stream_ids must be a contiguous int32 or uint32 tensor of shape ({n},) on "
                                 f"{self.device}")
        want = tuple(want)
        for name in want:
            if name not in RADIANCE_OUTPUTS:
                raise ValueError(f"unknown radiance output {name!r} (one of {', '.join(RADIANCE_OUTPUTS)})")
        if "radiance" not in want:
            raise ValueError('radiance always returns "radiance": name it in want')
        if int(spp) < 1:
            raise ValueError("radiance needs spp >= 1")
        if not self._pt:
            raise abi.PupilError(abi.ERR_INVALID, "no scene set")
        tensors = {}
        filled = False
        arrays = abi.RayRadiance()
        for name in want:
            shape = (n, RADIANCE_OUTPUTS[name])
            t = out.get(name) if out else None
            if t is not None:
                if not (isinstance(t, torch.Tensor) and t.is_cuda and t.device.index == self.device_index
                        and t.dtype == torch.float32 and tuple(t.shape) == shape and t.is_contiguous()):
                    raise ValueError(f"out[{name!r}] must be a contiguous float32 tensor of shape {shape} on "
                                     f"{self.device}")
            elif name == "radiance" and accumulate and int(sample_cnt) > 0:
                # the one case in which the engine reads what the array holds: a mean continued
                # without the earlier result starts from 0.  The fill runs on the current stream
                t = torch.zeros(shape, dtype=torch.float32, device=self.device)
                filled = True
            else:  # written whole, as trace()'s outputs: nothing of torch's is enqueued for it
                t = torch.empty(shape, dtype=torch.float32, device=self.device)
            tensors[name] = t
            setattr(arrays, name, t.data_ptr() if n else None)
        if n == 0:
            return tensors
        la = abi.Launch()
        la.random_seed = int(seed) & 0xFFFFFFFF
        la.sample_cnt = int(sample_cnt)
        la.spp = int(spp)
        la.max_depth = 0 if max_depth is None else int(max_depth)
        la.accumulate = int(bool(accumulate))
        s = self._query_stream(stream, [rays, stream_ids, *tensors.values()])
        if filled and s.cuda_stream != torch.cuda.current_stream(self.device_index).cuda_stream:
            s.wait_stream(torch.cuda.current_stream(self.device_index))  # the fill above, before the call reads it
        check(self._lib.pupil_pt_radiance_rays(self._pt, n, C.c_void_p(rays.data_ptr()),
                                               C.c_void_p(stream_ids.data_ptr()) if stream_ids is not None else None,
                                               C.byref(la), C.byref(arrays), C.c_void_p(s.cuda_stream)))
        return tensors

    def radiance_info(self) -> dict:
        """Calls and rays of radiance() since the scene was set, the extension and shadow rays their
        paths cast, growths of the engine's scratch, and the device time of the last call (waits
        for it)."""
        u = [C.c_uint64(0) for _ in range(5)]
        ms = C.c_double(0.0)
        check(self._lib.pupil_pt_radiance_info(self._pt, *[C.byref(x) for x in u], C.byref(ms)))
        return {"calls": u[0].value, "rays": u[1].value, "extension_rays": u[2].value, "shadow_rays": u[3].value,
                "scratch_grows": u[4].value, "last_ms": ms.value}

    def on_run(self):
        self.render(1)
        self._torch.cuda.synchronize(self.device_index)  # m_optix_pass->Synchronize()

    def stats(self) -> dict:
        c = abi.Counters()
        check(self._lib.pupil_pt_stats(self._pt, C.byref(c)))
        return c.as_dict()

    def export_bvh4(self):
        """The flattened BVH4 the traversal kernels read: (uint8 (n, 64) nodes, float32 (m, 12)
        world records, root link), or None for the two-level structure / other node formats."""
        import numpy as np

        nn, nr, root = C.c_uint32(0), C.c_uint32(0), C.c_int32(0)
        if self._lib.pupil_pt_export_bvh4(self._pt, C.byref(nn), None, C.byref(nr), None, C.byref(root)) != 0:
            return None
        nodes = np.zeros((max(1, nn.value), 64), np.uint8)
        recs = np.zeros((max(1, nr.value), 12), np.float32)
        check(self._lib.pupil_pt_export_bvh4(self._pt, C.byref(nn), nodes.ctypes.data_as(C.c_void_p), C.byref(nr),
                                             recs.ctypes.data_as(C.POINTER(C.c_float)), C.byref(root)))
        return nodes[: nn.value], recs[: nr.value], root.value

    def export_world_bvh4(self):
        """(tests) The world-mode two-level structure (pupil_debug_export_world_bvh4): a dict of
        nodes (uint8 (n, 64): TLAS, reserve, world BLAS copies), recs (float32 (m, 12) world record
        slots, the spheres' leaves last), boxes (float32 (instances, 6)), root, tlas_nodes, tlas_cap
        and braid; None for the flattened BVH and for object mode."""
        import numpy as np

        nn, nr, ni = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
        root, tn, tc, br = C.c_int32(0), C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
        scalars = [C.byref(root), C.byref(tn), C.byref(tc), C.byref(br)]
        rc = self._lib.pupil_debug_export_world_bvh4(self._pt, C.byref(nn), None, C.byref(nr), None, C.byref(ni), None,
                                                     *scalars)
        if rc == abi.ERR_UNSUPPORTED:
            return None
        check(rc)
        nodes = np.zeros((max(1, nn.value), 64), np.uint8)
        recs = np.zeros((max(1, nr.value), 12), np.float32)
        boxes = np.zeros((max(1, ni.value), 6), np.float32)
        check(self._lib.pupil_debug_export_world_bvh4(self._pt, C.byref(nn), nodes.ctypes.data_as(C.c_void_p), C.byref(nr),
                                                      recs.ctypes.data_as(abi.f32p), C.byref(ni),
                                                      boxes.ctypes.data_as(abi.f32p), *scalars))
        return {"nodes": nodes[: nn.value], "recs": recs[: nr.value], "boxes": boxes[: ni.value], "root": root.value,
                "tlas_nodes": tn.value, "tlas_cap": tc.value, "braid": br.value}

    def image(self, name: str = FINAL_RESULT):
        """Full-frame (h, w, c) numpy image, row 0 = bottom (reference pixel order)."""
        t = self.buffers.get(name).cpu().numpy()
        if self.tile[2] > 1:
            import numpy as np

            full = np.zeros((self.width * self.height, t.shape[1]), dtype=np.float32)
            full[self.local_pixels()] = t
            t = full
        return t.reshape(self.height, self.width, -1)

    def close_engine(self):
        if self._pt:
            self._lib.pupil_pt_destroy(self._pt)
            self._pt = C.c_void_p()
        self._kept = set()  # the snapshots went with the engine
        self._snapshots = False

    def __del__(self):  # pragma: no cover
        try:
            self.close_engine()
        except Exception:
            pass


class System:
    """Headless Pupil::System: passes run in order once per frame (system.cpp:81-114)."""

    def __init__(self):
        self.passes = []
        self.events = Events()
        self.world = None

    def add_pass(self, p: Pass):
        self.passes.append(p)
        if isinstance(p, PTPass):
            p.events = self.events
            self.events.bind(Events.CAMERA_CHANGE, lambda _: p.mark_dirty())
            self.events.bind(Events.RENDER_INSTANCE_UPDATE, p._on_instance_update)
            self.events.bind(Events.SCENE_LOAD, lambda w: p.set_scene(w))

    def set_scene(self, world):
        self.world = world
        self.events.dispatch(Events.SCENE_LOAD, world)

    def run(self, frames: int = 1):
        for _ in range(frames):
            for p in self.passes:
                p.run()
