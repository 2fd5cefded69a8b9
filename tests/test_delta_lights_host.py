"""Point, spot and directional lights on the host: the XML loader, the programmatic adders and
setter, the emitter table's order and the reference's selection probabilities
(EmitterHelper::ComputeProbability, world/emitter.cpp:321-337), and the ABI.  No GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import delta_light_cases as dc
from pupiloptixlab_amd import World, abi
from pupiloptixlab_amd import world as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32

HEAD = """<scene version="3.0.0">
  <integrator type="path"><integer name="max_depth" value="3"/></integrator>
  <sensor type="perspective"><float name="fov" value="45"/>
    <transform name="to_world"><lookat origin="0, 3, 4" target="0, 0, 0" up="0, 1, 0"/></transform>
    <film type="hdrfilm"><integer name="width" value="16"/><integer name="height" value="16"/></film>
  </sensor>
  <shape type="rectangle"><bsdf type="diffuse"><rgb name="reflectance" value="0.5, 0.6, 0.7"/></bsdf>
    <transform name="to_world"><scale value="2"/><rotate x="1" angle="-90"/></transform></shape>
  <shape type="rectangle"><bsdf type="diffuse"/>
    <transform name="to_world"><scale value="0.25"/><rotate x="1" angle="90"/><translate x="0" y="2" z="0"/></transform>
    <emitter type="area"><rgb name="radiance" value="4, 5, 6"/></emitter></shape>
"""
LIGHTS = """  <emitter type="directional"><vector name="direction" x="0.3" y="-1" z="0.2"/>
    <rgb name="irradiance" value="3, 2, 1"/></emitter>
  <emitter type="point"><point name="position" x="0.3" y="1.5" z="-0.2"/><rgb name="intensity" value="10, 8, 6"/></emitter>
  <emitter type="constant"><rgb name="radiance" value="0.1, 0.2, 0.3"/></emitter>
  <emitter type="spot"><rgb name="intensity" value="7"/><float name="cutoff_angle" value="35"/>
    <float name="beam_width" value="20"/>
    <transform name="to_world"><lookat origin="0.3, 1.5, -0.2" target="0.8, 0, -0.2" up="0, 0, 1"/></transform></emitter>
"""
TAIL = "</scene>\n"


def _load(tmp_path, name, body):
    p = tmp_path / name
    p.write_text(HEAD + body + TAIL)
    return World().load_scene(str(p))


def _table(d):
    return [dc.emitter_fields(d.area_emitters[i]) for i in range(d.num_area_emitters)]


# ------------------------------------------------------------------ 1. XML
def test_xml_lights_table_order_and_probabilities(tmp_path, capfd):
    w = _load(tmp_path, "lights.xml", LIGHTS)
    d = w.desc()
    assert "unknown emitter" not in capfd.readouterr().err
    t = _table(d)
    # two triangles of the rectangle, then point and spot in file order, then the directional
    assert [e["type"] for e in t] == [abi.EMITTER_TRI_AREA, abi.EMITTER_TRI_AREA, abi.EMITTER_POINT,
                                      abi.EMITTER_SPOT, abi.EMITTER_DIRECTIONAL]
    assert bool(d.env) and d.env.contents.type == abi.EMITTER_CONST_ENV
    point, spot, sun = t[2], t[3], t[4]
    assert np.array_equal(point["center"], f32([0.3, 1.5, -0.2])) and np.array_equal(point["color"], f32([10, 8, 6]))
    assert not point["axis"].any() and point["cutoff"] == 0 and point["beam"] == 0
    # a lookat is built as the inverse of a view matrix: the origin's image is the eye to rounding
    assert np.allclose(spot["center"], [0.3, 1.5, -0.2], rtol=0, atol=1e-6) and np.array_equal(spot["color"], f32([7, 7, 7]))
    axis = np.array([0.5, -1.5, 0.0]) / np.linalg.norm([0.5, -1.5, 0.0])  # the image of +Z: towards the target
    assert np.allclose(spot["axis"], axis, rtol=0, atol=1e-6)
    deg = f32(np.pi) / f32(180.0)
    assert spot["cutoff"] == f32(35.0) * deg and spot["beam"] == f32(20.0) * deg
    assert np.allclose(sun["axis"], dc.DIR_D, rtol=0, atol=1e-7) and np.array_equal(sun["color"], f32([3, 2, 1]))
    assert not sun["center"].any()
    for e in t[2:]:
        assert e["weight"] == 1.0 and e["area"] == 0.0
        assert abs(np.linalg.norm(e["axis"].astype(np.float64)) - (0.0 if e["type"] == abi.EMITTER_POINT else 1.0)) < 1e-6
    # ComputeProbability: emitter_num = 2 + 3 + 1
    sel, env_sel = dc.compute_probability([t[0]["weight"], t[1]["weight"]], 3, True)
    got = f32([e["select_probability"] for e in t])
    assert np.array_equal(dc.bits(got), dc.bits(sel)), (got, sel)
    assert dc.bits(d.env.contents.select_probability) == dc.bits(env_sel) and d.env.contents.weight == 1.0
    assert env_sel == f32(1.0) / f32(6.0) and sel[2] == sel[3] == sel[4] == env_sel
    # the rectangle's range is what it is without the lights
    plain = _load(tmp_path, "plain.xml", "").desc()
    offs = [d.instances[i].emitter_offset for i in range(d.num_instances)]
    assert offs == [plain.instances[i].emitter_offset for i in range(plain.num_instances)] == [-1, 0]
    assert plain.num_area_emitters == 2 and d.num_area_emitters == 5


def test_xml_spot_defaults_and_unknown_type(tmp_path, capfd):
    body = """  <emitter type="spot"><rgb name="intensity" value="1, 2, 3"/>
    <transform name="to_world"><translate x="1" y="2" z="3"/></transform></emitter>
  <emitter type="laser"><rgb name="intensity" value="1"/></emitter>
  <emitter type="point"><rgb name="intensity" value="2"/>
    <transform name="to_world"><translate x="-1" y="4" z="0.5"/></transform></emitter>
"""
    d = _load(tmp_path, "spot.xml", body).desc()
    err = capfd.readouterr().err
    assert "unknown emitter type [laser]" in err and err.count("unknown emitter") == 1
    t = _table(d)
    assert [e["type"] for e in t] == [abi.EMITTER_TRI_AREA, abi.EMITTER_TRI_AREA, abi.EMITTER_SPOT, abi.EMITTER_POINT]
    deg = f32(np.pi) / f32(180.0)
    spot, point = t[2], t[3]
    assert spot["cutoff"] == f32(20.0) * deg and spot["beam"] == f32(15.0) * deg  # 3/4 of the cutoff
    assert np.array_equal(spot["axis"], f32([0, 0, 1])) and np.array_equal(spot["center"], f32([1, 2, 3]))
    assert np.array_equal(point["center"], f32([-1, 4, 0.5]))  # the translation of its to_world
    assert d.env is None or not d.env


# ------------------------------------------------------------------ 2. adders and setter
def _emitter(kind, position=(0, 0, 0), axis=(0, 0, 0), color=(1, 1, 1), cutoff=0.0, beam=0.0):
    e = abi.Emitter()
    e.type = kind
    e.center[:] = position
    e.nrm[0][:] = axis
    e.color[:] = color
    e.pos[0][0], e.pos[0][1] = cutoff, beam
    return e


def _snapshot(w):
    d = w.desc()
    return [(e["type"], e["select_probability"].tobytes(), e["center"].tobytes(), e["color"].tobytes(),
             e["axis"].tobytes(), e["cutoff"].tobytes(), e["beam"].tobytes()) for e in _table(d)]


def test_adders_round_trip_and_invalid_cases():
    w = dc.floor_world()
    assert w.add_directional_light((0.0, -2.0, 0.0), (3, 2, 1)) == 0
    assert w.add_point_light((0.3, 1.5, -0.2), (10, 8, 6)) == 1
    assert w.add_spot_light((1, 2, 3), (0.0, -3.0, 4.0), 5.0, cutoff_deg=35, beam_deg=20) == 2
    d = w.desc()
    t = _table(d)
    # lights 1 and 2 (point, spot) come first, light 0 (directional) last; no env
    assert [e["type"] for e in t] == [abi.EMITTER_POINT, abi.EMITTER_SPOT, abi.EMITTER_DIRECTIONAL]
    assert d.num_area_emitters == 3 and not d.env
    assert all(d.instances[i].emitter_offset == -1 for i in range(d.num_instances))
    assert np.array_equal(t[1]["axis"], f32([0.0, -0.6, 0.8])) and np.array_equal(t[2]["axis"], f32([0, -1, 0]))
    assert np.array_equal(t[1]["color"], f32([5, 5, 5])) and np.array_equal(t[0]["color"], f32([10, 8, 6]))
    deg = f32(np.pi) / f32(180.0)
    assert t[1]["cutoff"] == f32(35) * deg and t[1]["beam"] == f32(20) * deg
    sel, _ = dc.compute_probability([], 3, False)
    assert np.array_equal(dc.bits([e["select_probability"] for e in t]), dc.bits(sel)) and sel[0] == f32(1) / f32(3)
    assert all(e["weight"] == 1.0 for e in t)

    lib, h = w._lib, w._h
    before = _snapshot(w)
    inv = abi.ERR_INVALID
    good = _emitter(abi.EMITTER_POINT)
    out = C.c_uint32(99)
    bad = [
        lambda: lib.pupil_world_add_delta_emitter(None, C.byref(good), C.byref(out)),
        lambda: lib.pupil_world_add_delta_emitter(h, None, C.byref(out)),
        lambda: lib.pupil_world_set_delta_emitter(None, 0, C.byref(good)),
        lambda: lib.pupil_world_set_delta_emitter(h, 1, None),
    ]
    for kind in (abi.EMITTER_NONE, abi.EMITTER_TRI_AREA, abi.EMITTER_CONST_ENV, abi.EMITTER_ENV_MAP, 8):  # not 5, 6, 7
        e = _emitter(kind, axis=(0, -1, 0), cutoff=0.5, beam=0.3)
        bad.append(lambda e=e: lib.pupil_world_add_delta_emitter(h, C.byref(e), None))
        bad.append(lambda e=e: lib.pupil_world_set_delta_emitter(h, 1, C.byref(e)))
    for axis in ((0, 0, 0), (np.nan, 1, 0), (np.inf, 0, 0)):  # zero or non-finite axis / direction
        for kind in (abi.EMITTER_SPOT, abi.EMITTER_DIRECTIONAL):
            e = _emitter(kind, axis=axis, cutoff=0.5, beam=0.3)
            bad.append(lambda e=e: lib.pupil_world_add_delta_emitter(h, C.byref(e), None))
        e = _emitter(abi.EMITTER_SPOT, axis=axis, cutoff=0.5, beam=0.3)
        bad.append(lambda e=e: lib.pupil_world_set_delta_emitter(h, 2, C.byref(e)))
    for cutoff, beam in ((0.5, 0.0), (0.5, -0.1), (0.3, 0.5), (3.2, 0.5), (np.nan, 0.1), (0.5, np.nan), (0.0, 0.0)):
        e = _emitter(abi.EMITTER_SPOT, axis=(0, -1, 0), cutoff=cutoff, beam=beam)
        bad.append(lambda e=e: lib.pupil_world_add_delta_emitter(h, C.byref(e), None))
        bad.append(lambda e=e: lib.pupil_world_set_delta_emitter(h, 2, C.byref(e)))
    bad.append(lambda: lib.pupil_world_set_delta_emitter(h, 3, C.byref(good)))  # light out of range
    sun = _emitter(abi.EMITTER_DIRECTIONAL, axis=(0, -1, 0))
    bad.append(lambda: lib.pupil_world_set_delta_emitter(h, 1, C.byref(sun)))   # point -> directional
    bad.append(lambda: lib.pupil_world_set_delta_emitter(h, 2, C.byref(sun)))   # spot -> directional
    bad.append(lambda: lib.pupil_world_set_delta_emitter(h, 0, C.byref(good)))  # directional -> point
    for k, call in enumerate(bad):
        assert call() == inv, k
        assert lib.pupil_last_error()
    assert out.value == 99
    assert _snapshot(w) == before  # the world is unchanged by every refused call

    # the setter: unnamed fields stay, a point may become a spot and back, beam == cutoff is allowed
    w.set_light(1, position=(0.0, 1.0, 0.0))
    w.set_light(2, cutoff_deg=40, beam_deg=40, direction=(0, -2, 0))
    w.set_light(0, irradiance=(1, 1, 2))
    t = _table(w.desc())
    assert np.array_equal(t[0]["center"], f32([0, 1, 0])) and np.array_equal(t[0]["color"], f32([10, 8, 6]))
    assert t[1]["cutoff"] == t[1]["beam"] == f32(40) * deg and np.array_equal(t[1]["axis"], f32([0, -1, 0]))
    assert np.array_equal(t[1]["center"], f32([1, 2, 3]))
    assert np.array_equal(t[2]["color"], f32([1, 1, 2])) and np.array_equal(t[2]["axis"], f32([0, -1, 0]))
    w.set_light(1, type=abi.EMITTER_SPOT, direction=(0, -1, 0), cutoff_deg=30)
    t = _table(w.desc())
    assert [e["type"] for e in t] == [abi.EMITTER_SPOT, abi.EMITTER_SPOT, abi.EMITTER_DIRECTIONAL]
    assert t[0]["cutoff"] == f32(30) * deg and t[0]["beam"] == f32(22.5) * deg
    w.set_light(1, type=abi.EMITTER_POINT)
    t = _table(w.desc())
    assert t[0]["type"] == abi.EMITTER_POINT and not t[0]["axis"].any() and t[0]["cutoff"] == 0
    with pytest.raises(ValueError):
        w.set_light(1, colour=(1, 1, 1))


def test_lights_beside_an_area_light_and_env():
    """Every emissive triangle counts as one emitter: a point light beside a two-triangle lamp is
    picked one time in three (one in four with an env)."""
    w = dc.floor_world()
    rect = w.add_builtin("rectangle")
    lamp = w.add_instance(rect, 0, W.transform(scale=(0.5, 0.5, 1), rotate=((1, 0, 0), 90), translate=(0, 3, 0)),
                          emitter_radiance=(4.0, 4.0, 4.0))
    w.add_point_light((0, 1, 0), 1.0)
    d = w.desc()
    t = _table(d)
    assert [e["type"] for e in t] == [abi.EMITTER_TRI_AREA, abi.EMITTER_TRI_AREA, abi.EMITTER_POINT]
    assert d.instances[lamp].emitter_offset == 0
    sel, _ = dc.compute_probability([t[0]["weight"], t[1]["weight"]], 1, False)
    assert np.array_equal(dc.bits([e["select_probability"] for e in t]), dc.bits(sel))
    assert t[2]["select_probability"] == f32(1) / f32(3)
    w.add_const_env((0.1, 0.1, 0.1))
    d = w.desc()
    sel, env_sel = dc.compute_probability([t[0]["weight"], t[1]["weight"]], 1, True)
    assert np.array_equal(dc.bits([e["select_probability"] for e in _table(d)]), dc.bits(sel))
    assert dc.bits(d.env.contents.select_probability) == dc.bits(env_sel) == dc.bits(f32(1) / f32(4))


# ------------------------------------------------------------------ 3. ABI
def test_abi_sizes_symbols_and_constants(tmp_path):
    # what the structs measured before the delta lights: no field was added
    assert C.sizeof(abi.Emitter) == 336 and C.sizeof(abi.SceneDesc) == 200
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include "pupil_pt.h"\nint main(void) { printf("%zu %zu %u %u %u\\n", '
                   "sizeof(pupil_emitter), sizeof(pupil_scene_desc), PUPIL_EMITTER_POINT, PUPIL_EMITTER_SPOT, "
                   "PUPIL_EMITTER_DIRECTIONAL); return 0; }\n")
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True).stdout.split()]
    assert got == [336, 200, 5, 6, 7]
    assert (abi.EMITTER_POINT, abi.EMITTER_SPOT, abi.EMITTER_DIRECTIONAL) == (5, 6, 7)
    lib = abi.load_library()
    for name in ("pupil_world_add_delta_emitter", "pupil_world_set_delta_emitter", "pupil_world_get_delta_emitter",
                 "pupil_debug_emitter_sample"):
        assert hasattr(lib, name) and name in abi.SIGNATURES, name
    assert lib.pupil_abi_version() == 7  # no bump: the entries are detected by symbol
    assert lib.pupil_debug_emitter_sample(None, 0, 0, None, None, None) == abi.ERR_INVALID
