"""Any-hit rays sort a node's children by overlap, not by distance (pt_traverse.h visit4;
PUPIL_SHADOW_ORDER=0 keeps them near to far).  A shadow ray's answer does not depend on the order of
its walk, so every frame here is the CPU oracle's bit for bit under both orders, the any-hit ray
query answers what the oracle's closest hit answers at the edges of the segment, and the counters of
two equal renders are equal."""
import os
import tempfile

import numpy as np
import pytest

import oracle
from pupiloptixlab_amd import World, scenes
from pupiloptixlab_amd import world as W

gpu = pytest.mark.gpu
TMP = os.path.join(tempfile.gettempdir(), "pupil_shadow_anyhit_scenes")
BUFS = (("pt accum buffer", "accum"), ("albedo", "albedo"), ("normal", "normal"), ("test", "test"))
ORDERS = ("0", "1")  # near to far, overlap
TIMED = {"build_ms", "last_render_ms", "trace_ms", "extend_ms", "shade_ms", "frame_ms", "ring_budget_bytes"}
_cache = {}


def _scene(name):
    """cornell: the 64 x 64 Cornell box, D = 4.  field: 4 tessellated spheres (8k triangles) over a
    floor under one light, 64 x 64, D = 4.  Each with the oracle's 12-spp frame, computed once."""
    if name not in _cache:
        if name == "cornell":
            w = World().load_scene(scenes.cornell_xml(os.path.join(TMP, "sa_cb64.xml"), 64, 64, 4))
        else:
            w = scenes.sphere_field(4, 64, 64, 4, seed=1)
        d = w.desc()
        _cache[name] = (w, oracle.OracleScene(d).render(spp=12))
    return _cache[name]


def _pass(w):
    from pupiloptixlab_amd.pt_pass import PTPass

    pt = PTPass(device=0)
    pt.set_scene(w.desc() if hasattr(w, "desc") else w)
    pt.dirty = False
    pt.random_seed, pt.sample_cnt = 0, 0
    return pt


def _grab(pt):
    import torch

    torch.cuda.synchronize()
    return {k: pt.buffers.get(k).cpu().numpy().copy() for k, _ in BUFS}


# ------------------------------------------------------------------ parity across the settings
@gpu
@pytest.mark.parametrize("frame_paths", ["0", None])  # the stage launches (mixed, mixed-ahead); the one-launch frame
@pytest.mark.parametrize("name", ["cornell", "field"])
def test_frames_equal_oracle_under_both_orders(name, frame_paths, monkeypatch):
    """3 x render(4), each continuing the last (frames in flight: the mixed-ahead kernel runs): the
    accumulation buffer and the AOVs are the oracle's 12-spp frame on every pixel, and identical
    between the two orders."""
    if frame_paths is not None:
        monkeypatch.setenv("PUPIL_FRAME_PATHS", frame_paths)
    w, ref = _scene(name)
    got = {}
    for order in ORDERS:
        monkeypatch.setenv("PUPIL_SHADOW_ORDER", order)
        pt = _pass(w)
        assert pt.shadow_info()["overlap_order"] == (order == "1")
        for _ in range(3):
            pt.render(4, continues=True)
        got[order] = _grab(pt)
        pt.close_engine()
        g = got[order]["pt accum buffer"].reshape(-1)
        assert np.array_equal(g.view(np.uint32), np.asarray(ref["accum"]).reshape(-1).view(np.uint32)), (name, order)
    for k, _ in BUFS:
        assert np.array_equal(got["0"][k].view(np.uint32), got["1"][k].view(np.uint32)), (name, k)


@gpu
def test_default_is_the_overlap_order(monkeypatch):
    monkeypatch.delenv("PUPIL_SHADOW_ORDER", raising=False)
    pt = _pass(_scene("cornell")[0])
    assert pt.shadow_info()["overlap_order"] is True
    pt.close_engine()


# ------------------------------------------------------------------ the edges of the segment
def _edge_world():
    """A 16 x 16 floor grid (512 triangles, y = 0), a quad of two triangles sharing the edge
    x = z (y = 1), a sphere of radius 0.5 at (3, 1, 0), and a mesh at y = 2 whose second triangle
    has zero area (two equal vertices) in the leaf of the first."""
    wd = W.World()
    wd.set_film(16, 16, 2)
    grey = wd.add_material(W.twosided(W.diffuse((0.5, 0.5, 0.5))))
    g = np.linspace(-4.0, 4.0, 17).astype(np.float32)
    P = np.array([(x, 0.0, z) for z in g for x in g], np.float32)
    T = np.array([t for j in range(16) for i in range(16)
                  for t in ((j * 17 + i, j * 17 + i + 1, (j + 1) * 17 + i + 1), (j * 17 + i, (j + 1) * 17 + i + 1, (j + 1) * 17 + i))],
                 np.uint32)
    wd.add_instance(wd.add_mesh(P, T), grey)
    Q = np.array([(-1, 1, -1), (1, 1, -1), (1, 1, 1), (-1, 1, 1)], np.float32)
    wd.add_instance(wd.add_mesh(Q, np.array([(0, 1, 2), (0, 2, 3)], np.uint32)), grey)
    wd.add_instance(wd.add_builtin("sphere"), grey, W.transform(scale=(0.5, 0.5, 0.5), translate=(3.0, 1.0, 0.0)))
    D = np.array([(-3.5, 2, -0.5), (-2.5, 2, -0.5), (-3.0, 2, 0.5), (-3.0, 2, 0.5)], np.float32)
    wd.add_instance(wd.add_mesh(D, np.array([(0, 1, 2), (1, 2, 3)], np.uint32)), grey)
    wd.add_instance(wd.add_builtin("rectangle"), grey, W.transform(translate=(0, 6, 0)), emitter_radiance=(5.0, 5.0, 5.0))
    wd.set_sensor(60.0, W.look_at_mitsuba((0.0, 3.0, 6.0), (0.0, 1.0, 0.0), (0, 1, 0)), fov_axis="y")
    return wd


def _edge_rays(orc):
    """(n, 8) rays = o, d, tmin, tmax.  Downward rays onto each occluder; per occluder the window
    ends exactly at the hit distance, one float short of it and one float past it, and starts
    exactly at it and one float past it."""
    f = np.float32
    down = (0.0, -1.0, 0.0)
    starts = {"quad interior": (0.5, 3.0, -0.25), "shared edge": (0.25, 3.0, 0.25), "shared edge b": (-0.5, 3.0, -0.5),
              "sphere": (3.0, 3.0, 0.0), "sphere off axis": (3.2, 3.0, 0.1), "degenerate leaf": (-3.0, 3.0, -0.2),
              "degenerate edge": (-3.0, 3.0, 0.5), "floor": (2.3, 0.75, 2.1), "past everything": (9.0, 3.0, 9.0)}
    rays = []
    for o in starts.values():
        base = np.array([*o, *down, 0.0, 1e16], f)
        t = orc.closest(base[None])[0, 0]
        rays.append(base)
        if t > 0:
            for tmax in (t, np.nextafter(f(t), f(0)), np.nextafter(f(t), f(np.inf))):
                rays.append(np.array([*o, *down, 0.0, tmax], f))
            t0 = f(t)
            for tmin in (t0, np.nextafter(t0, f(np.inf))):  # the floor may still lie behind
                rays.append(np.array([*o, *down, tmin, 1e16], f))
                rays.append(np.array([*o, *down, tmin, np.nextafter(t0, f(np.inf))], f))
    return np.stack(rays).astype(f)


@gpu
@pytest.mark.parametrize("order", ORDERS)
def test_any_hit_query_at_the_segment_edges(order, monkeypatch):
    """Occluders exactly at tmax, just short of and just beyond it, exactly at tmin; a ray through
    the shared edge of two triangles; a sphere record; a zero-area triangle in the leaf.  Expected:
    whether the oracle's closest hit on the same window finds anything."""
    import torch

    monkeypatch.setenv("PUPIL_SHADOW_ORDER", order)
    wd = _edge_world()
    orc = oracle.OracleScene(wd.desc())
    rays = _edge_rays(orc)
    want = orc.closest(rays)[:, 0] > 0
    assert want.any() and not want.all()  # both outcomes occur
    pt = _pass(wd)
    got = pt.trace(torch.from_numpy(rays).to(pt.device), any_hit=True)["hit"].cpu().numpy()
    pt.close_engine()
    assert set(np.unique(got[:, 0])) <= {1.0, -1.0}
    bad = np.flatnonzero((got[:, 0] > 0) != want)
    assert len(bad) == 0, [(int(i), rays[i].tolist(), bool(want[i])) for i in bad[:8]]


# ------------------------------------------------------------------ counters
@gpu
def test_counters_of_equal_renders_are_equal(monkeypatch):
    """Two engines, the same counter render: every counter of stats() but the clocks, and the
    shadow rays by outcome, are equal; occluded rays are some but not all of the shadow rays."""
    monkeypatch.setenv("PUPIL_FRAME_PATHS", "0")
    w, _ = _scene("field")
    runs = []
    for _ in range(2):
        pt = _pass(w)
        pt.render(4, collect_stats=True)
        _grab(pt)
        runs.append((pt.stats(), pt.shadow_info()))
        pt.close_engine()
    (a, sa), (b, sb) = runs
    for k in a:
        if k not in TIMED:
            assert a[k] == b[k], k
    assert sa == sb
    assert 0 < sa["occluded_rays"] < a["shadow_rays"]
    shadow_visits = a["node_visits"] - a["extend_node_visits"]
    assert 0 < sa["occluded_visits"] < shadow_visits
