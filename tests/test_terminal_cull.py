"""Terminal-ray cull: an extension ray that feeds a path's last shade is tested against the
scene's emissive primitives (the cull set) and, when it hits none, is counted but neither traced
nor shaded.  Every render here is compared bit for bit with the CPU oracle -- accum, albedo,
normal, test and the three ray counts -- and the positive cases also pin 0 < terminal_rays_culled
< the rays of the terminal generation (the oracle's extension rays at max_depth minus those at
max_depth - 1: the same paths, cut one bounce earlier)."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import oracle
from pupiloptixlab_amd import World, abi, scenes
from pupiloptixlab_amd import world as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TMP = os.path.join(tempfile.gettempdir(), "pupil_terminal_cull_scenes")  # the Cornell XML files written here
gpu = pytest.mark.gpu
BUFS = (("pt accum buffer", "accum"), ("albedo", "albedo"), ("normal", "normal"), ("test", "test"))
RAYS = ("primary_rays", "extension_rays", "shadow_rays")


# ------------------------------------------------------------------ CPU: the counters struct
def test_counters_struct_matches_header(tmp_path):
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "pupil_pt.h"\n'
                   'int main(void) { printf("%zu %zu\\n", sizeof(pupil_pt_counters), '
                   'offsetof(pupil_pt_counters, terminal_rays_culled)); return 0; }\n')
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    size, off = (int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True).stdout.split())
    assert size == C.sizeof(abi.Counters)
    # in the slot that was reserved before it: the struct keeps its size and its last field
    assert off == abi.Counters.terminal_rays_culled.offset == abi.Counters.coop_slots.offset - 8
    assert abi.Counters.hidden_instances.offset == size - 8
    assert "terminal_rays_culled" in abi.Counters().as_dict()


# ------------------------------------------------------------------ helpers
def _desc(w):
    return w.desc() if hasattr(w, "desc") else w


def _pass(w, tile=None):
    from pupiloptixlab_amd.pt_pass import PTPass

    pt = PTPass(device=0)
    pt.set_scene(w)
    if tile:
        pt.set_tiling(*tile)
    pt.dirty = False
    pt.random_seed, pt.sample_cnt = 0, 0
    return pt


def _grab(pt):
    import torch

    torch.cuda.synchronize()
    out = {k: pt.buffers.get(k).cpu().numpy().copy() for k, _ in BUFS}
    out["stats"] = pt.stats()
    return out


def _render(w, spp, tile=None, stats=True):
    pt = _pass(w, tile)
    pt.render(spp, collect_stats=stats)
    out = _grab(pt)
    pt.close_engine()
    return out


def _same_as_oracle(got, ref, name):
    for gk, rk in BUFS:
        g, r = np.asarray(got[gk]).reshape(-1), np.asarray(ref[rk]).reshape(-1)
        assert np.array_equal(g.view(np.uint32), r.view(np.uint32)), f"{name}: {gk} differs from the oracle"
    s, rs = got["stats"], ref["stats"]
    assert tuple(s[k] for k in RAYS) == tuple(rs[k] for k in RAYS), name


def _terminal_rays(w, spp, pixels=None):
    """Extension rays of the terminal generation: the oracle's count at the scene's max_depth minus
    its count one bounce shallower (depth 1 casts none)."""
    d = _desc(w)
    deep = oracle.OracleScene(d).render(spp=spp, pixels=pixels)
    depth = d.max_depth
    if depth < 2:
        return deep, 0
    if depth == 2:
        return deep, deep["stats"]["extension_rays"]
    d.max_depth = depth - 1
    try:
        shallow = oracle.OracleScene(d).render(spp=spp, pixels=pixels)["stats"]["extension_rays"]
    finally:
        d.max_depth = depth
    return deep, deep["stats"]["extension_rays"] - shallow


def _positive(w, spp, name, tile=None, pixels=None, stats=True):
    got = _render(w, spp, tile, stats)
    ref, terminal = _terminal_rays(w, spp, pixels)
    culled = got["stats"]["terminal_rays_culled"]
    print(f"{name}: terminal rays {terminal}, culled {culled}, extension rays {ref['stats']['extension_rays']}")
    _same_as_oracle(got, ref, name)
    assert 0 < culled < terminal, (name, culled, terminal)
    return got


def _off(w, spp, name):
    got = _render(w, spp)
    _same_as_oracle(got, oracle.OracleScene(_desc(w)).render(spp=spp), name)
    assert got["stats"]["terminal_rays_culled"] == 0, name
    return got


def _cornell(res, depth):
    return World().load_scene(scenes.cornell_xml(os.path.join(TMP, f"tc_cb{res}_d{depth}.xml"), res, res, depth))


def _room(res, depth, light="quad", occluder=False, env=False, radiance=(30.0, 28.0, 24.0)):
    """A closed 4 x 4 x 4 room seen from inside.  light: "quad" = a 1 x 1 light 0.1 under the
    ceiling; "inset" = the ceiling is a 3 x 3 grid of quads whose centre quad is the light, in the
    ceiling's plane and sharing its four edges and vertices with non-emissive triangles;
    "sphere" = a sphere emitter.  occluder: a 1.6 x 1.6 plate 0.5 under the light."""
    wd = W.World()
    wd.set_film(res, res, depth)
    rect = wd.add_builtin("rectangle")
    grey = wd.add_material(W.twosided(W.diffuse((0.7, 0.6, 0.5))))
    black = wd.add_material(W.twosided(W.diffuse((0.0, 0.0, 0.0))))
    walls = [((2, 2, 1), ((1, 0, 0), -90), (0, 0, 0)), ((2, 2, 1), None, (0, 2, -2)),
             ((2, 2, 1), ((0, 1, 0), 180), (0, 2, 2)), ((2, 2, 1), ((0, 1, 0), 90), (-2, 2, 0)),
             ((2, 2, 1), ((0, 1, 0), -90), (2, 2, 0))]
    for sc, rot, tr in walls:
        wd.add_instance(rect, grey, W.transform(scale=sc, rotate=rot, translate=tr))
    if light == "inset":
        g = np.array([-2.0, -0.5, 0.5, 2.0], np.float32)
        P = np.array([(x, 4.0, z) for z in g for x in g], np.float32)
        quads = [(j * 4 + i, j * 4 + i + 1, (j + 1) * 4 + i + 1, (j + 1) * 4 + i) for j in range(3) for i in range(3)]
        tris = lambda qs: np.array([t for a, b, c, d in qs for t in ((a, b, c), (a, c, d))], np.uint32)
        # each mesh keeps all 16 vertices: the light's corners are bit for bit the ceiling's
        wd.add_instance(wd.add_mesh(P, tris([q for k, q in enumerate(quads) if k != 4])), grey)
        wd.light = wd.add_instance(wd.add_mesh(P, tris([quads[4]])), black, emitter_radiance=radiance)
    else:
        wd.add_instance(rect, grey, W.transform(scale=(2, 2, 1), rotate=((1, 0, 0), 90), translate=(0, 4, 0)))
        if light == "sphere":
            wd.light = wd.add_instance(wd.add_builtin("sphere"), black,
                                       W.transform(scale=(0.3, 0.3, 0.3), translate=(0.4, 3.2, -0.3)),
                                       emitter_radiance=radiance)
        else:
            wd.light = wd.add_instance(rect, black, W.transform(scale=(0.5, 0.5, 1), rotate=((1, 0, 0), 90),
                                                                 translate=(0, 3.9, 0)),
                                       emitter_radiance=radiance)
    if occluder:
        wd.add_instance(rect, grey, W.transform(scale=(0.8, 0.8, 1), rotate=((1, 0, 0), 90), translate=(0.5, 3.4, 0)))
    if env:
        wd.add_const_env((0.4, 0.5, 0.6))
    wd.set_sensor(60.0, W.look_at_mitsuba((0.0, 2.0, 1.9), (0.0, 1.9, 0.0), (0, 1, 0)), fov_axis="y")
    return wd


# ------------------------------------------------------------------ Cornell box
@gpu
@pytest.mark.parametrize("depth", [2, 3, 5])
def test_cornell_stage_pipeline(depth, monkeypatch):
    monkeypatch.setenv("PUPIL_FRAME_PATHS", "0")  # render(4) through the stage launches
    _positive(_cornell(48, depth), 4, f"cornell48-d{depth}")


@gpu
def test_cornell_pipelined_sequence(monkeypatch):
    """12 x render(1), frames in flight between the renders: every frame's running mean equals the
    oracle's, and the per-render ray counts add up to the running total, culled rays included."""
    w = _cornell(48, 4)
    pt = _pass(w)
    t0 = pt.stats()["rays_traced_total"]
    per = 0
    for _ in range(12):
        pt.render(1)
        c = _grab(pt)["stats"]
        per += sum(c[k] for k in RAYS)
    got = _grab(pt)
    assert got["stats"]["rays_traced_total"] - t0 == per
    ref, terminal = _terminal_rays(w, 12)
    assert np.array_equal(got["pt accum buffer"].view(np.uint32), ref["accum"].view(np.uint32))
    for gk, rk in BUFS[1:]:
        assert np.array_equal(np.asarray(got[gk]).reshape(-1), np.asarray(ref[rk]).reshape(-1)), gk
    # the frames in flight have cast rays of their own: at least the 12 finished frames' share
    culled = got["stats"]["terminal_rays_culled"]
    in_flight = got["stats"]["frames_in_flight"]
    assert per >= sum(ref["stats"][k] for k in RAYS)
    pt.close_engine()
    monkeypatch.setenv("PUPIL_PIPE", "1")  # pipelining off: frame by frame the oracle's counts
    pt = _pass(w)
    per = 0
    for _ in range(12):
        pt.render(1)
        c = _grab(pt)["stats"]
        per += sum(c[k] for k in RAYS)
    s = pt.stats()
    pt.close_engine()
    assert per == sum(ref["stats"][k] for k in RAYS)
    assert 0 < s["terminal_rays_culled"] < terminal
    # pipelined: all the culls of the 12 finished frames, and at most those of the frames in flight
    # besides, which are the next seeds of the same progressive render
    _, terminal_ahead = _terminal_rays(w, 12 + in_flight)
    print(f"pipelined: culled {culled}, unpipelined {s['terminal_rays_culled']}, {in_flight} frames in flight")
    assert s["terminal_rays_culled"] <= culled < terminal_ahead


@gpu
def test_cornell_one_launch_frame():
    """The size and knobs of test_one_launch_frames_match_oracle's "cornell" case: 64 x 64, 1 spp,
    the default PUPIL_FRAME_PATHS, so the frame runs as one persistent launch."""
    got = _positive(_cornell(64, 4), 1, "cornell64-one-launch", stats=False)  # counter renders take the stages
    assert got["stats"]["frame_launches"] == 1


@gpu
def test_cornell_two_rank_tiling(monkeypatch):
    monkeypatch.setenv("PUPIL_FRAME_PATHS", "0")
    w = _cornell(48, 4)
    d = w.desc()
    lib = abi.load_library()
    for rank in (0, 1):
        n = C.c_uint32(0)
        lib.pupil_pt_local_pixels(d.width, d.height, 16, rank, 2, None, C.byref(n))
        pixels = np.zeros(n.value, np.uint32)
        lib.pupil_pt_local_pixels(d.width, d.height, 16, rank, 2, pixels.ctypes.data_as(abi.u32p), C.byref(n))
        got = _render(w, 4, tile=(16, rank, 2))
        ref, terminal = _terminal_rays(w, 4, pixels)
        for gk, rk in BUFS:  # the rank's pixels of every buffer (a rank's buffer may be compact)
            r = np.asarray(ref[rk]).reshape(len(pixels), -1)
            g = np.asarray(got[gk]).reshape(-1, r.shape[1])
            g = g if len(g) == len(pixels) else g[pixels]
            assert np.array_equal(g.view(np.uint32), r.view(np.uint32)), (rank, gk)
        s, rs = got["stats"], ref["stats"]
        assert tuple(s[k] for k in RAYS) == tuple(rs[k] for k in RAYS)
        assert 0 < s["terminal_rays_culled"] < terminal


@gpu
@pytest.mark.parametrize("frame_paths", ["0", None])
def test_knob_off_changes_only_the_counter(frame_paths, monkeypatch):
    """PUPIL_TERMINAL_CULL=0 against =1: every buffer and every counter but terminal_rays_culled."""
    if frame_paths is not None:
        monkeypatch.setenv("PUPIL_FRAME_PATHS", frame_paths)
    w = _cornell(48, 4)
    runs = {}
    for knob in ("0", "1"):
        monkeypatch.setenv("PUPIL_TERMINAL_CULL", knob)
        runs[knob] = _render(w, 2)
    for gk, _ in BUFS:
        assert np.array_equal(runs["0"][gk].view(np.uint32), runs["1"][gk].view(np.uint32)), gk
    timed = {"build_ms", "last_render_ms", "trace_ms", "extend_ms", "shade_ms", "frame_ms", "ring_budget_bytes"}
    a, b = runs["0"]["stats"], runs["1"]["stats"]
    assert a["terminal_rays_culled"] == 0 and b["terminal_rays_culled"] > 0
    # what the traversal did (node visits, primitive tests, refills) differs by design: the counters of what the integrator cast, and of the structure, do not
    traced = {"node_visits", "prim_tests", "extend_node_visits", "extend_prim_tests", "unique_node_fetches",
              "node_loop_iters", "node_loop_lanes",
              "leaf_loop_iters", "leaf_loop_lanes", "refills", "refill_lanes", "trace_bytes", "extend_bytes"}
    for k in a:
        if k in timed or k in traced or k == "terminal_rays_culled":
            continue
        assert a[k] == b[k], k
    for r in (a, b):  # the queue accounting covers every ray cast, culled or traced
        assert r["queue_handed"] == r["queue_activated"] == r["queue_retired"] == r["queue_listed"] == \
            sum(r[k] for k in RAYS)
    assert b["node_visits"] < a["node_visits"]


# ------------------------------------------------------------------ geometry cases
@gpu
@pytest.mark.parametrize("case", ["occluder", "inset", "sphere"])
@pytest.mark.parametrize("frame_paths", ["0", None])
def test_emitter_geometry(case, frame_paths, monkeypatch):
    """occluder: part of the light hides behind a plate, so some terminal rays pass the cull and
    are then stopped by the plate in the traversal.  inset: the light lies in the ceiling's plane
    and shares its edges with the ceiling's triangles (32 x 32).  sphere: a sphere emitter."""
    if frame_paths is not None:
        monkeypatch.setenv("PUPIL_FRAME_PATHS", frame_paths)
    w = _room(32 if case == "inset" else 40, 4, light={"occluder": "quad"}.get(case, case), occluder=case == "occluder")
    _positive(w, 4, f"room-{case}")


@gpu
def test_environment_map_is_off():
    _off(_room(32, 4, env=True), 2, "room-env")


@gpu
def test_emissive_mesh_is_off():
    _off(scenes.sphere_field(8, 64, 36, 4, seed=3, emissive_groups=1), 2, "emissive-mesh")


@gpu
@pytest.mark.parametrize("accel,culls", [("flat", True), ("two_level", True), ("two_level_object", False)])
def test_acceleration_structures(accel, culls, monkeypatch):
    monkeypatch.setenv("PUPIL_ACCEL", "two_level" if accel.startswith("two_level") else "flat")
    if accel == "two_level_object":
        monkeypatch.setenv("PUPIL_TL_MODE", "object")
    monkeypatch.setenv("PUPIL_FRAME_PATHS", "0")
    w = _room(32, 3, light="sphere" if accel != "flat" else "quad")
    if culls:
        got = _positive(w, 2, f"room-{accel}")
    else:
        got = _off(w, 2, f"room-{accel}")
    assert got["stats"]["two_level"] == (accel != "flat")


# ------------------------------------------------------------------ updates
def _fresh_equal(pt, w, spp, name, oracle_desc=None):
    """A render of the updated engine equals a fresh engine's on the updated scene, the oracle's,
    and culls as many rays as the fresh engine (no stale set).  oracle_desc: what the oracle renders
    when it is not w.desc() (the oracle knows no visibility masks: it gets the scene without the
    hidden instances)."""
    before = pt.stats()["terminal_rays_culled"]
    pt.random_seed, pt.sample_cnt = 0, 0
    pt.dirty = False
    pt.render(spp, collect_stats=True)
    got = _grab(pt)
    fresh = _render(w, spp)
    for gk, _ in BUFS:
        assert np.array_equal(got[gk].view(np.uint32), fresh[gk].view(np.uint32)), f"{name}: {gk} differs from a fresh engine"
    _same_as_oracle(got, oracle.OracleScene(oracle_desc if oracle_desc is not None else w.desc()).render(spp=spp), name)
    culled = got["stats"]["terminal_rays_culled"] - before
    assert culled == fresh["stats"]["terminal_rays_culled"], (name, culled, fresh["stats"]["terminal_rays_culled"])
    return culled


@gpu
@pytest.mark.parametrize("accel", ["flat", "two_level"])
def test_updates_keep_the_set_current(accel, monkeypatch):
    monkeypatch.setenv("PUPIL_ACCEL", accel)
    monkeypatch.setenv("PUPIL_FRAME_PATHS", "0")
    monkeypatch.setenv("PUPIL_PIPE", "1")  # every render complete in itself
    spp = 2
    w = _room(32, 3, light="inset")
    light = w.light
    pt = _pass(w)
    base = _fresh_equal(pt, w, spp, "before")
    assert base > 0
    # the light's instance sinks from the ceiling to mid height: both of its faces can now be
    # reached, from the floor and from the ceiling, so fewer terminal rays are culled
    w.set_instance_transform(light, W.transform(translate=(0, -2, 0)))
    pt.update_instance(w, light)
    moved = _fresh_equal(pt, w, spp, "moved")
    print(f"updates: base {base}, moved {moved}")
    assert moved < base
    w.set_instance_transform(light, W.identity4())
    pt.update_instance(w, light)
    assert _fresh_equal(pt, w, spp, "moved back") == base
    # its vertices: the light shrinks to a quarter of its area -> more rays culled
    d = w.desc()
    shape = d.instances[light].shape
    P0 = np.ctypeslib.as_array(d.shapes[shape].positions, (d.shapes[shape].num_vertices * 3,)).reshape(-1, 3).copy()
    small = P0.copy()
    small[:, 0] *= 0.5
    small[:, 2] *= 0.5
    for rebuild in (False, True):
        w.set_mesh_vertices(shape, small)
        pt.update_shape(w, shape, rebuild=rebuild)
        assert _fresh_equal(pt, w, spp, f"shrunk rebuild={rebuild}") > base
        w.set_mesh_vertices(shape, P0)
        pt.update_shape(w, shape, rebuild=rebuild)
        assert _fresh_equal(pt, w, spp, f"restored rebuild={rebuild}") == base
    pt.close_engine()


def _without(desc, hidden):
    """desc without the instances in `hidden`; everything else (the emitter table included) as it is."""
    keep = [i for i in range(desc.num_instances) if i not in set(hidden)]
    arr = (abi.Instance * max(1, len(keep)))()
    for k, i in enumerate(keep):
        C.memmove(C.byref(arr[k]), C.byref(desc.instances[i]), C.sizeof(abi.Instance))
    out = abi.SceneDesc()
    C.memmove(C.byref(out), C.byref(desc), C.sizeof(abi.SceneDesc))
    out.num_instances = len(keep)
    out.instances = C.cast(arr, C.POINTER(abi.Instance))
    out._keep = (arr, desc)  # the arrays the copy points into
    return out


@gpu
def test_visibility_mask(monkeypatch):
    """The light hidden and shown again by its visibility mask.  Hidden, it stays in the emitter
    table (as in the reference) and in the set; its NaN records fail the cull's test as they fail
    the traversal's, so the render equals the oracle's of the scene without the instance and a fresh
    engine's on the masked world, bit for bit, and the terminal generation is culled whole."""
    monkeypatch.setenv("PUPIL_FRAME_PATHS", "0")
    monkeypatch.setenv("PUPIL_PIPE", "1")
    spp = 2
    w = _room(32, 3, light="quad")
    pt = _pass(w)
    base = _fresh_equal(pt, w, spp, "before")
    _, terminal = _terminal_rays(w, spp)
    assert 0 < base < terminal
    w.set_instance_visibility(w.light, 0)
    pt.update_instances(w, [w.light])
    assert pt.stats()["hidden_instances"] == 1
    gone = _without(w.desc(), [w.light])
    culled = _fresh_equal(pt, w, spp, "hidden", oracle_desc=gone)
    _, terminal_gone = _terminal_rays(gone, spp)
    print(f"visibility: shown {base} of {terminal}, hidden {culled} of {terminal_gone}")
    assert culled == terminal_gone and culled > base  # no ray can reach the hidden light
    w.set_instance_visibility(w.light, 255)
    pt.update_instances(w, [w.light])
    assert _fresh_equal(pt, w, spp, "shown") == base
    pt.close_engine()


@gpu
def test_radiance_to_zero_and_back(monkeypatch):
    """The light's radiance set to zero and back through the emitter update: each render equals a
    fresh engine's on that scene and the oracle's.  A dark emitter stays in the set -- its hit still
    multiplies the path's throughput by that zero, which only the shade restates -- so the rays
    culled are those of a fresh engine on the dark scene, and the lit scene's count returns."""
    from pupiloptixlab_amd.abi import check

    monkeypatch.setenv("PUPIL_FRAME_PATHS", "0")
    monkeypatch.setenv("PUPIL_PIPE", "1")
    spp = 2
    lit, dark = _room(32, 3), _room(32, 3, radiance=(0.0, 0.0, 0.0))
    pt = _pass(lit)
    base = _fresh_equal(pt, lit, spp, "lit")
    assert base > 0
    for w, name in ((dark, "dark"), (lit, "lit again")):
        d = w.desc()
        check(pt._lib.pupil_pt_update_emitters(pt._pt, C.byref(d)))
        culled = _fresh_equal(pt, w, spp, name)
        print(f"radiance {name}: culled {culled}, lit {base}")
        assert culled > 0
    assert culled == base
    pt.close_engine()
