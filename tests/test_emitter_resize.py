"""The engine-owned emitter table rebuilt at a new size (device_emitters on): emissive instances
added, removed, reordered, rebound and hidden through pupil_pt_set_instances_emitters, and an
emissive mesh replaced through pupil_pt_replace_shape_mesh.

The reference, for every comparison: an engine freshly created on the world's own description of
the new scene, whose table world.cpp and emitter_tables() derive on the host -- code that shares
nothing with the kernels under test.  Equal means bit for bit: the render's buffers, the camera
G-buffer, radiance along fixed rays, the primitive tables, the structure's counters (the helpers of
test_instance_set.py) and the emitter table with its CDF and guide.

Scenes: instance_set_cases.BASE (109 primitives; 48 x 48, 2 spp, depth 4) and what the cases add."""
import functools

import numpy as np
import pytest

from pupiloptixlab_amd import abi
from pupiloptixlab_amd import world as W

import instance_set_cases as cases
import replace_mesh_cases as meshes
from instance_set_cases import A, BASE, LAMP, LAMP_INSTANCE, SECOND_LAMP, SPHERE
from test_instance_set import ACCELS, _accel, _bits, _no_blas_build, _outputs, _pass, _same

POINT = ((0.5, 2.0, -1.0), (3.0, 3.0, 3.0))
TEXELS = np.array([[[4, 3, 2, 1], [0.5, 6, 1, 1]], [[2, 2, 2, 1], [0.25, 1, 8, 1]]], np.float32)
BITMAP_LAMP = cases.inst(LAMP, cases.GREY, radiance=W.bitmap(TEXELS), scale=(0.6, 0.6, 1.0), rotate=((1, 0, 0), 90),
                         translate=(-1.4, 2.6, 0.3))
EMISSIVE_SPHERE = cases.inst(SPHERE, cases.GREY, radiance=(5.0, 6.0, 7.0), scale=(0.3, 0.3, 0.3), translate=(1.2, 1.4, -0.4))
CUBE_LAMP = dict(BASE[LAMP_INSTANCE], shape=A, xf=dict(scale=(0.4, 0.1, 0.4), translate=(0.0, 3.0, 0.0)))


@functools.lru_cache(maxsize=None)
def small_grid():
    """24 x 24 quads = 1152 faces, texcoords, no normals: the smallest table that crosses the
    chains' 1024-value chunk and needs 11 guide bits"""
    n = 24
    x, y = np.meshgrid(np.linspace(-1.0, 1.0, n + 1), np.linspace(-1.0, 1.0, n + 1), indexing="xy")
    z = 0.1 * np.sin(3.0 * x) * np.cos(2.0 * y)
    p = np.stack([x, y, z], -1).reshape(-1, 3)
    t = np.stack([(x + 1.0) / 2.0, (y + 1.0) / 2.0], -1).reshape(-1, 2)
    i = (np.arange(n)[:, None] * (n + 1) + np.arange(n)[None, :]).reshape(-1)
    f = np.concatenate([np.stack([i, i + 1, i + n + 2], 1), np.stack([i, i + n + 2, i + n + 1], 1)])
    assert len(f) == 1152
    return meshes._mesh(p, f, None, t)


LAMP_MESHES = {"tetrahedron": meshes.tetrahedron, "icosphere": meshes.icosphere, "grid": small_grid}


def build(specs, lamp=None, point=False, env=False, scale=1.0):
    """the world of `specs`; lamp: the LAMP shape re-meshed (its vertices scaled); a point light; a constant env"""
    w = cases.world(specs)
    if lamp is not None:
        m = LAMP_MESHES[lamp]()
        w.set_mesh(LAMP, m["positions"] * np.float32(scale), m["faces"], m["normals"], m["texcoords"], allow_emissive=True)
    if point:
        w.add_point_light(*POINT)
    if env:
        w.add_const_env((0.3, 0.4, 0.5))
    return w


def _table(pt):
    t = pt.emitter_table()
    return {"emitters." + k: _bits(np.asarray(0 if v is None else v)) for k, v in t.items()} | \
        {"emitters.has_guide": _bits(np.array([t["guide"] is not None]))}


def _state(pt, flow=False):
    return _outputs(pt, flow) | _table(pt)


def _fresh(world):
    pt = _pass(world)
    try:
        return _state(pt)
    finally:
        pt.close_engine()


def _engine(world):
    pt = _pass(world)
    pt.device_emitters = True
    return pt


def _set(pt, world, device=False):
    if not device:
        pt.set_instances(world)
        return
    import torch

    side = torch.cuda.Stream(pt.device)
    with torch.cuda.stream(side):
        t = torch.from_numpy(cases.to_world(world)).to(pt.device) + 0
        pt.set_instances_device(world, t.reshape(-1, 3, 4), stream=side)
    side.synchronize()


def _steps(accel, monkeypatch, first, steps, device=False, **kw):
    """an engine on build(first) taken through `steps` (spec lists): equal to fresh after each"""
    _accel(monkeypatch, accel)
    pt = _engine(build(first, **kw))
    try:
        for n, specs in enumerate(steps):
            w = build(specs, **kw)
            _set(pt, w, device)
            assert pt.device_emitters
            _same(_state(pt), _fresh(w), (accel, "step", n))
        assert pt.emitter_resize_info()["resizes"] == len(steps)
        return pt.emitter_resize_info()
    finally:
        pt.close_engine()


# ------------------------------------------------------------------ the emissive set through set_instances
@pytest.mark.gpu
@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("accel", ACCELS)
def test_add_a_lamp_then_remove_it(accel, device, monkeypatch):
    """fails without the feature: PUPIL_ERR_UNSUPPORTED, the emitter table would change"""
    info = _steps(accel, monkeypatch, BASE, [BASE + (SECOND_LAMP,), BASE], device)
    assert info["last_true_areas"] == 2


@pytest.mark.gpu
@pytest.mark.parametrize("accel", ACCELS)
def test_remove_the_only_lamp_leaves_the_point_light(accel, monkeypatch):
    """zero triangle and sphere emitters, a delta light alone: its select probability, CDF and no guide"""
    no_lamp = BASE[:LAMP_INSTANCE] + BASE[LAMP_INSTANCE + 1:]
    info = _steps(accel, monkeypatch, BASE, [no_lamp, BASE], point=True)
    assert info["last_true_areas"] == 2


@pytest.mark.gpu
@pytest.mark.parametrize("accel", ACCELS)
def test_remove_the_only_lamp_under_an_env(accel, monkeypatch):
    """an empty table; the env's select probability follows the count"""
    no_lamp = BASE[:LAMP_INSTANCE] + BASE[LAMP_INSTANCE + 1:]
    _steps(accel, monkeypatch, BASE, [no_lamp, BASE], env=True)


@pytest.mark.gpu
@pytest.mark.parametrize("accel", ACCELS)
def test_guide_disappears_and_reappears(accel, monkeypatch):
    """total 2 -> 1 -> 2: a sphere lamp beside a point light, the point light's scene without the sphere, and back"""
    _accel(monkeypatch, accel)
    one = BASE[:LAMP_INSTANCE] + (EMISSIVE_SPHERE,) + BASE[LAMP_INSTANCE + 1:]  # the rectangle replaced by a sphere: 1 + the point
    none = BASE[:LAMP_INSTANCE] + BASE[LAMP_INSTANCE + 1:]
    pt = _engine(build(one, point=True))
    try:
        assert pt.emitter_table()["guide"] is not None
        _set(pt, build(none, point=True))
        assert pt.emitter_table()["guide"] is None and len(pt.emitter_table()["cdf"]) == 1
        _same(_state(pt), _fresh(build(none, point=True)), (accel, "one emitter"))
        _set(pt, build(one, point=True))
        assert pt.emitter_table()["guide"] is not None
        _same(_state(pt), _fresh(build(one, point=True)), (accel, "two again"))
    finally:
        pt.close_engine()


@pytest.mark.gpu
@pytest.mark.parametrize("accel", ACCELS)
def test_rebind_the_lamp_to_the_cube(accel, monkeypatch):
    """2 -> 12 emitters in front of a second lamp: guide_bits changes, the later offsets shift"""
    first = BASE + (SECOND_LAMP,)
    rebound = BASE[:LAMP_INSTANCE] + (CUBE_LAMP,) + BASE[LAMP_INSTANCE + 1:] + (SECOND_LAMP,)
    info = _steps(accel, monkeypatch, first, [rebound, first])
    assert info["last_true_areas"] == 4


@pytest.mark.gpu
@pytest.mark.parametrize("accel", ACCELS)
def test_swap_two_lamps_add_a_sphere_hide_a_lamp(accel, monkeypatch):
    first = BASE + (SECOND_LAMP,)
    swapped = BASE[:LAMP_INSTANCE] + (SECOND_LAMP,) + BASE[LAMP_INSTANCE + 1:] + (BASE[LAMP_INSTANCE],)
    sphere = swapped[:2] + (EMISSIVE_SPHERE,) + swapped[2:]
    hidden = sphere[:-1] + (dict(sphere[-1], visible=False),)  # it stays in the table
    info = _steps(accel, monkeypatch, first, [swapped, sphere, hidden], point=True)
    assert info["last_true_areas"] == 5


@pytest.mark.gpu
@pytest.mark.parametrize("accel", ACCELS)
def test_bitmap_lamp_added_and_removed(accel, monkeypatch):
    """the weight is summed on the host, the texels go up once; the lamp that stays -- constant, and
    then the bitmap one -- still renders after the other's texels are freed"""
    both = BASE + (BITMAP_LAMP,)
    only_bitmap = BASE[:LAMP_INSTANCE] + BASE[LAMP_INSTANCE + 1:] + (BITMAP_LAMP,)
    _steps(accel, monkeypatch, BASE, [both, only_bitmap, both, BASE], point=True)


# ------------------------------------------------------------------ an emissive mesh replaced
@pytest.mark.gpu
@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("name", list(LAMP_MESHES))
@pytest.mark.parametrize("accel", ACCELS)
def test_replace_the_lamp_mesh(accel, name, device, monkeypatch):
    """fails without the feature: PUPIL_ERR_UNSUPPORTED, its emitter range would change.  A second lamp
    and a point light sit behind the replaced one: their offsets and indices shift.  Then the vertices
    and the lamp's transform change on the device: the table follows, so the new bookkeeping is live."""
    import torch

    _accel(monkeypatch, accel)
    # the second lamp shows the same shape: both ranges change.  Nothing hidden, so that bvh_nodes is
    # comparable after a replacement (test_replace_mesh.py test_counters: a world-mode TLAS built while
    # an instance is hidden leaves its entries out, a fresh engine's keeps them, with equal hits)
    specs = tuple(dict(s, visible=True) for s in BASE) + (SECOND_LAMP,)
    pt = _engine(build(specs, point=True))
    try:
        m = LAMP_MESHES[name]()
        if device:
            dev = lambda a, dt: None if a is None else torch.from_numpy(np.ascontiguousarray(a).astype(dt)).to(pt.device)
            pt.replace_shape_device(LAMP, dev(m["positions"], np.float32), dev(m["faces"], np.int32),
                                    dev(m["normals"], np.float32), dev(m["texcoords"], np.float32))
        else:
            pt.replace_shape(LAMP, m["positions"], m["faces"], m["normals"], m["texcoords"])
        w = build(specs, lamp=name, point=True)
        got, ref = _state(pt), _fresh(w)
        assert len(pt.emitter_table()["cdf"]) == 2 * len(m["faces"]) + 1
        _same(got, ref, (accel, name, "replaced"))
        info = pt.emitter_resize_info()
        assert info["resizes"] == 1 and info["last_true_areas"] == 2 * len(m["faces"])
        # new vertices for the new topology, from device memory
        pt.update_shape_device(LAMP, torch.from_numpy(m["positions"] * np.float32(0.75)).to(pt.device),
                               None if m["normals"] is None else torch.from_numpy(m["normals"]).to(pt.device), rebuild=True)
        _same(_state(pt), _fresh(build(specs, lamp=name, point=True, scale=0.75)), (accel, name, "deformed"))
        # and the lamp moved on the device
        xf = dict(scale=(1.0, 1.0, 1.0), rotate=((1, 0, 0), 90), translate=(0.3, 3.0, 0.1))
        moved = specs[:LAMP_INSTANCE] + (dict(specs[LAMP_INSTANCE], xf=xf),) + specs[LAMP_INSTANCE + 1:]
        wm = build(moved, lamp=name, point=True, scale=0.75)
        t = torch.from_numpy(cases.to_world(wm)[LAMP_INSTANCE:LAMP_INSTANCE + 1]).to(pt.device)
        pt.update_instances_device(t, torch.tensor([LAMP_INSTANCE], dtype=torch.int32, device=pt.device))
        _same(_state(pt), _fresh(wm), (accel, name, "moved"), structure=False)
        assert pt.emitter_resize_info()["resizes"] == 1
    finally:
        pt.close_engine()


@pytest.mark.gpu
@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("name", ["tetrahedron", "grid"])
@pytest.mark.parametrize("accel", ACCELS)
def test_replace_the_mesh_of_a_bitmap_lamp(accel, name, device, monkeypatch):
    """The radiance and tex[v] of the new records show only in the render: a lamp whose radiance is a
    2 x 2 bitmap of four unlike texels, re-meshed to the grid (1152 faces with texcoords: a wrong
    tex[] of any face changes what the lamp emits there) and to the tetrahedron (no texcoords: zero).
    The constant lamp in front shows the same shape, so the bitmap lamp's range moves; its texels are
    kept -- moved into the new table -- and must still be the ones sampled."""
    import torch

    _accel(monkeypatch, accel)
    specs = tuple(dict(s, visible=True) for s in BASE) + (BITMAP_LAMP,)
    pt = _engine(build(specs, point=True))
    try:
        before = _state(pt)
        m = LAMP_MESHES[name]()
        if device:
            dev = lambda a, dt: None if a is None else torch.from_numpy(np.ascontiguousarray(a).astype(dt)).to(pt.device)
            pt.replace_shape_device(LAMP, dev(m["positions"], np.float32), dev(m["faces"], np.int32),
                                    dev(m["normals"], np.float32), dev(m["texcoords"], np.float32))
        else:
            pt.replace_shape(LAMP, m["positions"], m["faces"], m["normals"], m["texcoords"])
        got = _state(pt)
        assert not np.array_equal(got["pt accum buffer"], before["pt accum buffer"])
        _same(got, _fresh(build(specs, lamp=name, point=True)), (accel, name, "bitmap lamp replaced"))
        # and once more, to the mesh with texcoords: the texels move a second time
        pt.replace_shape(LAMP, *[LAMP_MESHES["grid"]()[k] for k in ("positions", "faces", "normals", "texcoords")])
        _same(_state(pt), _fresh(build(specs, lamp="grid", point=True)), (accel, name, "replaced again"))
        assert pt.emitter_resize_info()["resizes"] == 2
    finally:
        pt.close_engine()


# ------------------------------------------------------------------ the old entry and the new one
@pytest.mark.gpu
@pytest.mark.parametrize("accel", ACCELS)
def test_unchanged_emissive_set_equals_the_old_entry(accel, monkeypatch):
    _accel(monkeypatch, accel)
    added = BASE + (cases.EXTRA_A,)
    states, infos = [], []
    for new_entry in (False, True):
        pt = _engine(cases.world(BASE))
        try:
            w = cases.world(added)
            if new_entry:
                pt.set_instances(w)
                assert pt.emitter_resize_info()["resizes"] == 1
            else:  # the old entry, as a caller of the C interface reaches it
                n, arr, vis = pt._bindings(w)
                abi.check(pt._lib.pupil_pt_set_instances(pt._pt, n, arr, vis.ctypes.data_as(abi.u32p), None, 0, None))
                pt._after_set_instances(w)
                assert pt.emitter_resize_info()["resizes"] == 0
            _no_blas_build(pt, accel)
            info = pt.set_instances_info()
            infos.append((info["calls"], info["last_blas_builds"], info["last_whole_rebuild"],
                          pt.device_emitters_info()["refreshes"]))  # a resize counts as the old entry's refresh does
            states.append(_state(pt))
        finally:
            pt.close_engine()
    _same(states[0], states[1], (accel, "old entry against new"))
    assert infos[0] == infos[1]


def _counters(pt):
    return (pt.set_instances_info()["calls"], pt.replace_info()["replacements"], pt.emitter_resize_info()["resizes"],
            pt.device_emitters_info()["refreshes"], pt.stats()["accel_refits"])


@pytest.mark.gpu
@pytest.mark.parametrize("accel", ACCELS)
def test_refusals_change_nothing(accel, monkeypatch):
    import ctypes as C

    _accel(monkeypatch, accel)
    pt = _pass(cases.world(BASE))
    try:
        before, counters = _state(pt), _counters(pt)
        m = meshes.tetrahedron()
        w2 = cases.world(BASE + (SECOND_LAMP,))
        n, arr, vis = pt._bindings(w2)
        desc = abi.SceneDesc()
        C.memmove(C.byref(desc), C.byref(w2.desc()), C.sizeof(abi.SceneDesc))
        desc.instances = C.cast(arr, C.POINTER(abi.Instance))
        vp = vis.ctypes.data_as(abi.u32p)
        call = lambda d, ptr=None, flags=0: pt._lib.pupil_pt_set_instances_emitters(pt._pt, C.byref(d), vp, ptr, flags, None)

        # the mode off, both calls: as before the feature
        with pytest.raises(abi.PupilError) as e:
            pt.replace_shape(LAMP, m["positions"], m["faces"])
        assert e.value.code == abi.ERR_UNSUPPORTED
        assert call(desc) == abi.ERR_UNSUPPORTED
        assert b"pupil_pt_enable_device_emitters" in pt._lib.pupil_last_error()
        with pytest.raises(abi.PupilError) as e:
            pt.set_instances(w2)  # the pass routes to the old entry
        assert e.value.code == abi.ERR_UNSUPPORTED
        _same(_state(pt), before, (accel, "mode off"))
        assert _counters(pt) == counters

        pt.device_emitters = True
        before, counters = _state(pt), _counters(pt)
        # ranges that are not the face count: the second lamp's range starts one early
        arr[len(BASE)].emitter_offset = 1
        assert call(desc) == abi.ERR_INVALID
        arr[len(BASE)].emitter_offset = 2
        # one emitter too many for the ranges
        more = (abi.Emitter * (desc.num_area_emitters + 1))()
        C.memmove(more, desc.area_emitters, C.sizeof(abi.Emitter) * desc.num_area_emitters)
        C.memmove(C.byref(more[desc.num_area_emitters]), desc.area_emitters, C.sizeof(abi.Emitter))
        d_more = abi.SceneDesc()
        C.memmove(C.byref(d_more), C.byref(desc), C.sizeof(abi.SceneDesc))
        d_more.area_emitters = C.cast(more, C.POINTER(abi.Emitter))
        d_more.num_area_emitters = desc.num_area_emitters + 1
        assert call(d_more) == abi.ERR_INVALID
        # the env's presence changed
        w_env = cases.world(BASE + (SECOND_LAMP,))
        w_env.add_const_env((0.3, 0.4, 0.5))
        d_env = abi.SceneDesc()
        C.memmove(C.byref(d_env), C.byref(w_env.desc()), C.sizeof(abi.SceneDesc))
        d_env.instances = C.cast(arr, C.POINTER(abi.Instance))
        assert call(d_env) == abi.ERR_INVALID
        # a table out of order: a directional light in front of a point light
        w_ord = cases.world(BASE + (SECOND_LAMP,))
        w_ord.add_point_light(*POINT)
        w_ord.add_point_light((1.0, 2.0, 0.0), (1.0, 1.0, 1.0))
        d_ord = w_ord.desc()
        ems = (abi.Emitter * d_ord.num_area_emitters)()
        C.memmove(ems, d_ord.area_emitters, C.sizeof(ems))
        ems[d_ord.num_area_emitters - 2].type = abi.EMITTER_DIRECTIONAL
        d2 = abi.SceneDesc()
        C.memmove(C.byref(d2), C.byref(d_ord), C.sizeof(abi.SceneDesc))
        d2.instances = C.cast(arr, C.POINTER(abi.Instance))
        d2.area_emitters = C.cast(ems, C.POINTER(abi.Emitter))
        assert call(d2) == abi.ERR_INVALID
        # the device flag without a pointer, a pointer without the flag, a NULL scene
        assert call(desc, None, abi.INSTANCES_DEVICE) == abi.ERR_INVALID
        assert call(desc, C.c_void_p(256), 0) == abi.ERR_INVALID
        assert pt._lib.pupil_pt_set_instances_emitters(pt._pt, None, vp, None, 0, None) == abi.ERR_INVALID
        # a mesh whose index is out of range, for the emissive shape
        bad = m["faces"].copy()
        bad[0, 0] = 99
        with pytest.raises(abi.PupilError) as e:
            pt.replace_shape(LAMP, m["positions"], bad)
        assert e.value.code == abi.ERR_INVALID
        _same(_state(pt), before, (accel, "mode on"))
        assert _counters(pt) == counters and pt.device_emitters
        # and the call the refusals were variations of goes through: successes only are counted
        assert call(desc) == abi.OK
        assert pt.emitter_resize_info()["resizes"] == 1 and pt.emitter_resize_info()["last_true_areas"] == 4
        pt._after_set_instances(w2)
        _same(_state(pt), _fresh(w2), (accel, "accepted"))
    finally:
        pt.close_engine()
