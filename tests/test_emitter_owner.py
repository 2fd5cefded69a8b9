"""The emitter tables' one owner (csrc/host/emitter_tables.h) on the GPU: an engine that has lived
through replacing and in-place emitter updates, the device-side mode, a new instance table and a
moved lamp holds what a freshly created engine holds, and a refused update is a no-op however often
it is made.  Every comparison is bit-exact.

Scene: a floor, a two-triangle lamp, a sphere emitter, a point light, and one non-emissive instance
that can go in front of the others.  Film 16 x 16, 2 spp, depth 4."""
import ctypes as C

import numpy as np
import pytest

from pupiloptixlab_amd import World, abi
from pupiloptixlab_amd import world as W

from test_visibility import _render

pytestmark = pytest.mark.gpu

SPP = 2
LAMP_AT, LAMP_MOVED = (0.0, 1.9, 0.0), (0.4, 1.7, -0.3)
LAMP_TEXELS = np.ascontiguousarray(np.float32([[[4, 3, 2, 1], [0.5, 6, 1, 1]], [[2, 2, 2, 1], [0.25, 1, 8, 1]]]))  # 2 x 2
ENV_TEXELS = np.ascontiguousarray(
    (0.25 + (np.arange(4 * 3 * 4, dtype=np.float32) * 7) % 11).reshape(3, 4, 4))  # 4 wide, 3 high


def world(extra_in_front=False, lamp_at=LAMP_AT):
    w = World()
    rect, sphere = w.add_builtin("rectangle"), w.add_builtin("sphere")
    grey = W.twosided(W.diffuse((0.6, 0.6, 0.55)))
    if extra_in_front:  # the floor's material: one the engine holds
        w.add_instance(rect, w.add_material(grey), W.transform(scale=(0.5, 0.5, 1), rotate=((0, 1, 0), 30), translate=(-0.8, 0.2, 0.5)))
    w.add_instance(rect, w.add_material(grey), W.transform(scale=(3, 3, 1), rotate=((1, 0, 0), -90), translate=(0, -1, 0)))
    w.add_instance(rect, w.add_material(W.twosided(W.diffuse((0.2, 0.2, 0.2)))),
                   W.transform(scale=(0.5, 0.5, 1), rotate=((1, 0, 0), 90), translate=lamp_at), emitter_radiance=(4.0, 3.0, 2.0))
    w.add_instance(sphere, w.add_material(W.diffuse((0.3, 0.3, 0.3))), W.transform(scale=(0.3, 0.3, 0.3), translate=(1.0, 0.0, 0.2)),
                   emitter_radiance=(3.0, 3.0, 2.5))
    w.add_point_light((-1.0, 0.5, -0.5), (2.0, 2.0, 3.0))
    w.set_film(16, 16, 4)
    w.set_sensor(50.0, W.look_at_mitsuba((0.0, 0.8, -4.0), (0.0, 0.2, 0.0), (0, 1, 0)))
    return w


def _texture(texels):
    t = W.rgb(0.0)
    t.type = abi.TEX_BITMAP
    t.height, t.width = texels.shape[0], texels.shape[1]
    t.filter = 1
    t.rgba = texels.ctypes.data_as(abi.f32p)  # the module keeps the texels alive
    return t


def env_map(radiance):
    e = abi.Emitter()
    e.type = abi.EMITTER_ENV_MAP
    e.weight = e.select_probability = e.scale = 1.0
    e.radiance = radiance
    e.to_world[:] = e.to_local[:] = (1, 0, 0, 0, 1, 0, 0, 0, 1)
    return e


def scene(w, lamp_bitmap=False, env=None):
    """the world's desc with the lamp's radiance a 2 x 2 bitmap, and with an env emitter"""
    desc = w.desc()
    n = desc.num_area_emitters
    arr = (abi.Emitter * n)()
    C.memmove(arr, desc.area_emitters, C.sizeof(arr))
    if lamp_bitmap:
        for k in range(n):
            if arr[k].type == abi.EMITTER_TRI_AREA:
                arr[k].radiance = _texture(LAMP_TEXELS)
    out = abi.SceneDesc()
    C.memmove(C.byref(out), C.byref(desc), C.sizeof(abi.SceneDesc))
    out.area_emitters = C.cast(arr, C.POINTER(abi.Emitter))
    out.env = C.pointer(env) if env is not None else None
    out._keep = (arr, env, desc, w)  # what the copy points into
    return out


def _pass(world_or_desc):
    from pupiloptixlab_amd.pt_pass import PTPass

    pt = PTPass(device=0)
    pt.set_scene(world_or_desc)
    return pt


def _update(pt, desc):
    return pt._lib.pupil_pt_update_emitters(pt._pt, C.byref(desc))


def _picks(pt):
    p = np.random.default_rng(5).random(64, dtype=np.float32)
    p[0], p[1] = 0.0, np.nextafter(np.float32(1.0), np.float32(0.0))
    out = np.zeros(64, np.int32)
    abi.check(pt._lib.pupil_debug_select_emitter(pt._pt, 64, p.ctypes.data_as(abi.f32p), out.ctypes.data_as(C.POINTER(C.c_int32))))
    return out


def _env(pt):
    d = np.random.default_rng(9).normal(size=(16, 3))
    d = np.ascontiguousarray(d / np.linalg.norm(d, axis=1, keepdims=True), np.float32)
    pn = np.float32([0.3, 0.0, 0.2, 0.0, 1.0, 0.0])
    out = np.zeros((16, 8), np.float32)
    rc = pt._lib.pupil_debug_env(pt._pt, 16, d.ctypes.data_as(abi.f32p), pn.ctypes.data_as(abi.f32p), 1, out.ctypes.data_as(abi.f32p))
    return rc, out


def _state(pt, env=False):
    """everything the emitter tables decide: the whole table, the guide, the picks, the render"""
    t = pt.emitter_table()
    s = {k: v for k, v in t.items() if k not in ("guide_bits", "guide")}
    s["guide"] = np.append(t["guide"], t["guide_bits"]).astype(np.uint32)
    s["picks"] = _picks(pt)
    if env:
        rc, s["env"] = _env(pt)
        assert rc == abi.PUPIL_OK
    s.update(_render(pt, SPP))
    return s


def _assert_same(got, ref, what):
    assert got.keys() == ref.keys()
    for k in ref:
        assert got[k].shape == ref[k].shape and np.array_equal(got[k].view(np.uint32), ref[k].view(np.uint32)), (what, k)


def test_a_long_lived_engine_equals_a_fresh_one():
    env = env_map(_texture(ENV_TEXELS))
    a, b = world(), world(extra_in_front=True)
    pt = _pass(a)  # constant radiance, no env
    try:
        textured, constant = scene(a, lamp_bitmap=True, env=env), scene(a, env=env)
        assert _update(pt, textured) == abi.PUPIL_OK  # replace
        assert _update(pt, textured) == abi.PUPIL_OK  # replace again: the first one's texels and env block go
        assert _update(pt, constant) == abi.PUPIL_OK  # back to constant radiance, the same env
        assert _update(pt, constant) == abi.PUPIL_OK  # in place
        pt.device_emitters = True
        pt.set_instances(b)  # the emissive indices shift from 1, 2 to 2, 3
        assert pt.device_emitters
        b.set_instance_transform(2, W.transform(scale=(0.5, 0.5, 1), rotate=((1, 0, 0), 90), translate=LAMP_MOVED))
        pt.update_instance(b, 2)
        got = _state(pt, env=True)
    finally:
        pt.close_engine()
    final = scene(world(extra_in_front=True, lamp_at=LAMP_MOVED), env=env)
    pt = _pass(final)
    try:
        abi.check(pt._lib.pupil_pt_enable_device_emitters(pt._pt, C.byref(final)))
        ref = _state(pt, env=True)
    finally:
        pt.close_engine()
    assert len(ref["area"]) == 4 and ref["guide"][-1] == 2 and ref["env"].any() and ref["pt accum buffer"].any()
    _assert_same(got, ref, "long-lived against fresh")


def test_a_refused_update_is_a_no_op_twice():
    """An env of type ENV_MAP whose radiance is no bitmap is refused; the tables' types are the
    engine's and no radiance is a bitmap, so a second identical call would be written in place if the
    first had left its env desc behind (before the owner it returned PUPIL_OK, read from the code and
    confirmed once on that commit)."""
    a = world()
    held = scene(a, env=env_map(_texture(ENV_TEXELS)))
    refused = scene(a, env=env_map(W.rgb(1.0, 1.0, 1.0)))
    pt = _pass(held)
    try:
        before = _state(pt, env=True)
        assert before["env"].any()
        for attempt in range(2):
            assert _update(pt, refused) == abi.ERR_INVALID, attempt
            assert pt._lib.pupil_last_error().decode() == "env map needs a bitmap"
            _assert_same(_state(pt, env=True), before, f"after refusal {attempt}")
        assert _update(pt, scene(a)) == abi.PUPIL_OK
        rc, _ = _env(pt)
        assert rc == abi.ERR_INVALID and pt._lib.pupil_last_error().decode() == "the scene has no env emitter"
    finally:
        pt.close_engine()
