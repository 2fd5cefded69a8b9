"""Instance visibility masks (RenderObject::visibility_mask -> OptixInstance::visibilityMask,
ias_manager.cpp:174,192): pupil_pt_update_instances_masked hides and shows instances by a refit.

Expected results come from the unchanged CPU oracle on a FILTERED desc: a copy of World.desc()
whose instance array omits the hidden instances while shapes, materials, area emitters and env
stay.  The oracle loads its emitters from area_emitters independently of the instances, so this is
exactly the reference's behaviour: a hidden emitter still lights the scene through next-event
estimation and is seen by no ray.  Dropping an instance shifts the later global primitive ids down
by its primitive count (order kept, so equal-t tie-breaks are unchanged); filtered_to_full_ids maps
the oracle's ids back for the pupil_pt_trace_rays comparisons."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import oracle
from pupiloptixlab_amd import World, abi, scenes
from pupiloptixlab_amd import world as W

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "build", "pupil_path_tracer")
MISS = 0xFFFFFFFF
KEYS = ("pt accum buffer", "final result", "albedo", "normal", "test")


# ------------------------------------------------------------------ the filtered desc
def filtered_desc(desc, hidden):
    """desc without the instances in `hidden`; everything else (emitters included) as it is."""
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


def env_only_desc(desc, behind=(0.0, 0.0, -1000.0)):
    """Every instance hidden.  The oracle builds from an empty instance list but its traversal then
    reads the root of a BVH that has no nodes, so "nothing" is given to it as one copy of instance 0
    translated to `behind`, a place no ray of the scene can reach (behind the camera, which looks
    away from it, with nothing else to bounce off): the oracle's image is that of the empty scene."""
    out = filtered_desc(desc, range(desc.num_instances))
    arr = out._keep[0]
    C.memmove(C.byref(arr[0]), C.byref(desc.instances[0]), C.sizeof(abi.Instance))
    for k in range(12):
        arr[0].to_world[k] = arr[0].to_object[k] = 1.0 if k in (0, 5, 10) else 0.0
    for a in range(3):
        arr[0].to_world[4 * a + 3] = behind[a]
        arr[0].to_object[4 * a + 3] = -behind[a]
    arr[0].emitter_offset = -1
    out.num_instances = 1
    return out


def prim_counts(desc):
    out = []
    for i in range(desc.num_instances):
        sh = desc.shapes[desc.instances[i].shape]
        out.append(1 if sh.kind == abi.SHAPE_SPHERE else sh.num_faces)
    return np.array(out, np.int64)


def filtered_to_full_ids(desc, hidden):
    """global primitive id in the filtered desc -> id in the full desc."""
    cnt = prim_counts(desc)
    first = np.concatenate([[0], np.cumsum(cnt)])
    keep = [i for i in range(desc.num_instances) if i not in set(hidden)]
    if not keep:
        return np.zeros(0, np.uint32)
    return np.concatenate([np.arange(first[i], first[i] + cnt[i]) for i in keep]).astype(np.uint32)


def oracle_hits(desc, hidden, rays):
    """closest hits of the filtered oracle with the id word mapped to the full scene's ids."""
    if len(set(hidden)) == desc.num_instances:  # nothing left: every ray misses
        ref = np.zeros((len(rays), 4), np.float32)
        ref[:, 0] = -1.0
        ref[:, 3] = np.array([MISS], np.uint32).view(np.float32)[0]
        return ref
    ref = oracle.OracleScene(filtered_desc(desc, hidden)).closest(rays)
    ids = ref[:, 3].copy().view(np.uint32)
    hit = ids != MISS
    ids[hit] = filtered_to_full_ids(desc, hidden)[ids[hit]]
    ref[:, 3] = ids.view(np.float32)
    return ref


# ------------------------------------------------------------------ engine helpers
def _accel(monkeypatch, accel):
    """flat | two_level (world mode) | two_level_object"""
    monkeypatch.setenv("PUPIL_ACCEL", "flat" if accel == "flat" else "two_level")
    if accel == "two_level_object":
        monkeypatch.setenv("PUPIL_TL_MODE", "object")


def _pass(world):
    from pupiloptixlab_amd.pt_pass import PTPass

    pt = PTPass(device=0)
    pt.set_scene(world)
    return pt


def _set_visibility(pt, world, masks):
    """masks: {instance: mask}; one masked update for all of them."""
    for i, m in masks.items():
        world.set_instance_visibility(i, m)
    pt.update_instances(world, list(masks))


def _trace(pt, rays, any_hit=0, tmin=0.001, tmax=1e16):
    r8 = np.ascontiguousarray(np.concatenate([rays, np.full((len(rays), 1), tmin, np.float32),
                                              np.full((len(rays), 1), tmax, np.float32)], 1), np.float32)
    out = np.zeros((len(rays), 4), np.float32)
    abi.check(pt._lib.pupil_pt_trace_rays(pt._pt, len(rays), r8.ctypes.data_as(abi.f32p),
                                          out.ctypes.data_as(abi.f32p), any_hit))
    return out


def _render(pt, spp):
    import torch

    pt.mark_dirty()  # accumulation from seed 0, like the oracle's render(spp)
    pt.render(spp)
    torch.cuda.synchronize()
    return {k: pt.buffers.get(k).cpu().numpy() for k in KEYS}


def _assert_render_equals(got, ref, what):
    for k, rk in zip(KEYS, ("accum", "accum", "albedo", "normal", "test")):
        assert np.array_equal(got[k].reshape(ref[rk].shape).view(np.uint32), ref[rk].view(np.uint32)), (what, k)


def _random_rays(n, lo, hi, seed):
    rng = np.random.default_rng(seed)
    org = rng.uniform(lo, hi, (n, 3))
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return np.concatenate([org, d], 1).astype(np.float32)


# ------------------------------------------------------------------ scenes
def mixed_field():
    """12 instances of one BLAS (0..11), the room (12..17), the light (18), a builtin sphere (19)
    and, last (20), a small mesh placed at instance 4's centre, which interpenetrates it: flattened
    leaves there mix the records of both."""
    w = scenes.instanced_field(num_instances=12, width=32, height=18, max_depth=4, seed=3, spheres_per_blas=10,
                               scale_range=(0.4, 2.5))
    m = w.add_material(W.diffuse((0.7, 0.4, 0.3)))
    w.add_instance(w.add_builtin("sphere"), m, W.transform(scale=(3.5, 3.5, 3.5), translate=(0.0, 6.0, 2.0)))
    t4 = w.desc().instances[4].to_world
    v, nrm, uv, idx = scenes.uv_sphere(8, 6)
    w.add_instance(w.add_mesh(v, idx, nrm, uv), m,
                   W.transform(scale=(1.5, 1.2, 1.5), translate=(float(t4[3]), float(t4[7]), float(t4[11]))))
    return w


MIXED_HIDDEN = (5, 19, 20)  # a middle mesh instance, the sphere, the last instance


def tiny_world(ntri, instances=1):
    """ntri stacked triangles per instance under a constant environment (test_tiny_scenes' shapes)."""
    w = World()
    tri = np.array([[-1, -1, 0], [1, -1, 0], [0, 1, 0]], np.float32)
    pos = np.concatenate([tri + [0, 0, 0.1 * k] for k in range(ntri)]).astype(np.float32)
    s = w.add_mesh(pos, np.arange(3 * ntri, dtype=np.uint32).reshape(-1, 3))
    m = w.add_material(W.twosided(W.diffuse((0.5, 0.5, 0.5))))
    for k in range(instances):
        w.add_instance(s, m, W.transform(translate=(0.6 * k, 0.0, 1.0 * k)))
    w.add_const_env((0.8, 0.9, 1.0))
    w.set_film(16, 16, 3)
    w.set_sensor(40.0, W.look_at_mitsuba((0, 0, -3), (0, 0, 0), (0, 1, 0)))
    return w


def tiny_rays():
    rng = np.random.default_rng(2)
    org = np.concatenate([rng.uniform(-1, 1.5, (500, 2)), np.full((500, 1), -2.0)], 1)
    d = np.concatenate([rng.uniform(-0.2, 0.2, (500, 2)), np.ones((500, 1))], 1)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return np.concatenate([org, d], 1).astype(np.float32)


# ------------------------------------------------------------------ 1. random rays
@pytest.mark.parametrize("accel", ["flat", "two_level", "two_level_object"])
def test_hidden_instances_random_rays(accel, monkeypatch):
    """A mesh instance, the builtin sphere and the last instance hidden in one call: 20k random
    rays, closest and any hit, equal the filtered oracle bit for bit."""
    _accel(monkeypatch, accel)
    w = mixed_field()
    desc = w.desc()
    rays = _random_rays(20000, [-5, 1, -4], [5, 11, 8], 17)
    full = oracle.OracleScene(desc).closest(rays)
    ref = oracle_hits(desc, MIXED_HIDDEN, rays)
    changed = (full.view(np.uint32) != ref.view(np.uint32)).any(axis=1).mean()
    hits = (ref[:, 3].view(np.uint32) != MISS).mean()
    print(f"rays changed by hiding {changed:.3f}, still hitting {hits:.3f}")
    assert changed >= 0.05 and hits >= 0.30  # the oracle alone: the comparison below is not vacuous
    pt = _pass(w)
    try:
        before = _trace(pt, rays)
        assert np.array_equal(before.view(np.uint32), full.view(np.uint32))
        _set_visibility(pt, w, {i: 0 for i in MIXED_HIDDEN})
        assert pt.stats()["hidden_instances"] == 3
        out = _trace(pt, rays)
        bad = (out.view(np.uint32) != ref.view(np.uint32)).any(axis=1)
        assert not bad.any(), f"{accel}: {bad.sum()} rays differ"
        occ = _trace(pt, rays, any_hit=1)
        assert np.array_equal(occ[:, 0] > 0, ref[:, 0] > 0)
    finally:
        pt.close_engine()


# ------------------------------------------------------------------ 2. render parity, hidden light
@pytest.mark.parametrize("accel", ["flat", "two_level"])
def test_render_with_hidden_light_equals_filtered_oracle(accel, monkeypatch):
    """Instance 3 and the emissive instance n-1 hidden: the emitter table stays (world.cpp:45-54), so
    next-event estimation still reaches the light and the image is not black."""
    _accel(monkeypatch, accel)
    w = scenes.sphere_field(8, 96, 64, 4, seed=5, merge=False)
    desc = w.desc()
    n = desc.num_instances
    assert desc.instances[n - 1].emitter_offset >= 0
    ref = oracle.OracleScene(filtered_desc(desc, (3, n - 1))).render(spp=2)
    assert ref["accum"][:, :3].max() > 0.0
    pt = _pass(w)
    try:
        _set_visibility(pt, w, {3: 0, n - 1: 0})
        got = _render(pt, 2)
        _assert_render_equals(got, ref, accel)
        assert got["pt accum buffer"][:, :3].max() > 0.0
        # no camera ray sees the hidden light: its pixels differ from the full scene's
        assert not np.array_equal(got["pt accum buffer"], oracle.OracleScene(desc).render(spp=2)["accum"])
    finally:
        pt.close_engine()


# ------------------------------------------------------------------ 3. round trip
@pytest.mark.parametrize("accel", ["flat", "two_level", "two_level_object"])
def test_hide_then_show_restores_everything(accel, monkeypatch):
    _accel(monkeypatch, accel)
    w = mixed_field()
    pt = _pass(w)
    try:
        rays = _random_rays(5000, [-5, 1, -4], [5, 11, 8], 23)
        img0, hit0 = _render(pt, 2), _trace(pt, rays)
        bvh0 = pt.export_bvh4()
        bound0 = pt.stats()["node_bound"]
        _set_visibility(pt, w, {i: 0 for i in MIXED_HIDDEN})
        assert not np.array_equal(_trace(pt, rays).view(np.uint32), hit0.view(np.uint32))
        _set_visibility(pt, w, {i: 1 for i in MIXED_HIDDEN})
        st = pt.stats()
        assert st["hidden_instances"] == 0 and st["node_bound"] == bound0
        img1, hit1 = _render(pt, 2), _trace(pt, rays)
        for k in KEYS:
            assert np.array_equal(img0[k].view(np.uint32), img1[k].view(np.uint32)), k
        assert np.array_equal(hit0.view(np.uint32), hit1.view(np.uint32))
        if accel == "flat":
            bvh1 = pt.export_bvh4()
            assert bvh0[2] == bvh1[2]
            assert bvh0[0].tobytes() == bvh1[0].tobytes()  # nodes
            assert bvh0[1].tobytes() == bvh1[1].tobytes()  # records
    finally:
        pt.close_engine()


# ------------------------------------------------------------------ 4. one refit
@pytest.mark.parametrize("accel,update", [("flat", "refit"), ("flat", "rebuild"), ("two_level", "refit"),
                                          ("two_level", "rebuild"), ("two_level_object", "refit")])
def test_hide_and_move_cost_one_refit(accel, update, monkeypatch):
    """Hide instance a and move instance b through the World, then one PTPass.update_instances."""
    _accel(monkeypatch, accel)
    if update == "rebuild":
        monkeypatch.setenv("PUPIL_FLAT_UPDATE", "rebuild")
        monkeypatch.setenv("PUPIL_TL_UPDATE", "rebuild")
    w = scenes.sphere_field(8, 48, 32, 4, seed=5, merge=False)
    pt = _pass(w)
    try:
        r0 = pt.stats()["accel_refits"]
        w.set_instance_visibility(2, 0)
        w.set_instance_transform(5, W.transform(scale=(1.4, 0.8, 1.1), rotate=((0, 1, 0), 40), translate=(0.5, 3.0, 1.5)))
        pt.update_instances(w, [2, 5])
        st = pt.stats()
        assert st["accel_refits"] == r0 + 1 and st["hidden_instances"] == 1
        ref = oracle.OracleScene(filtered_desc(w.desc(), (2,))).render(spp=2)
        _assert_render_equals(_render(pt, 2), ref, (accel, update))
    finally:
        pt.close_engine()


def test_pending_hide_and_move_coalesce_into_one_refit():
    """RENDER_INSTANCE_UPDATE events only record: a hide and a move before one render cost one refit."""
    from pupiloptixlab_amd.pt_pass import Events

    w = scenes.sphere_field(8, 48, 32, 4, seed=5, merge=False)
    pt = _pass(w)
    try:
        r0 = pt.stats()["accel_refits"]
        w.set_instance_visibility(1, 0)
        pt.events.dispatch(Events.RENDER_INSTANCE_UPDATE, (w, 1))
        w.set_instance_transform(6, W.transform(scale=(0.9, 0.9, 0.9), translate=(-2.0, 5.0, 1.0)))
        pt.events.dispatch(Events.RENDER_INSTANCE_UPDATE, (w, 6))
        assert pt.stats()["accel_refits"] == r0
        pt.render(1)
        st = pt.stats()
        assert st["accel_refits"] == r0 + 1 and st["hidden_instances"] == 1
        # a pass set up on a world that already hides an instance applies the mask
        pt2 = _pass(w)
        assert pt2.stats()["hidden_instances"] == 1
        ref = oracle.OracleScene(filtered_desc(w.desc(), (1,))).render(spp=1)
        _assert_render_equals(_render(pt2, 1), ref, "set_scene")
        pt2.close_engine()
    finally:
        pt.close_engine()


# ------------------------------------------------------------------ 5. smallest shapes
@pytest.mark.parametrize("accel", ["flat", "two_level", "two_level_object"])
@pytest.mark.parametrize("ntri", [1, 2, 5])
def test_hiding_the_only_instance_leaves_the_environment(ntri, accel, monkeypatch):
    """The root becomes empty: every pixel is the env-only oracle's, every ray misses; then back."""
    _accel(monkeypatch, accel)
    w = tiny_world(ntri)
    desc = w.desc()
    rays = tiny_rays()
    full_hits = oracle.OracleScene(desc).closest(rays)
    assert (full_hits[:, 0] > 0).any()
    pt = _pass(w)
    try:
        _set_visibility(pt, w, {0: 0})
        out = _trace(pt, rays)
        assert (out[:, 3].view(np.uint32) == MISS).all() and (out[:, 0] == -1.0).all()
        assert not (_trace(pt, rays, any_hit=1)[:, 0] > 0).any()
        got = _render(pt, 2)
        _assert_render_equals(got, oracle.OracleScene(env_only_desc(desc)).render(spp=2), "empty")
        assert (got["pt accum buffer"][:, :3] == np.array([0.8, 0.9, 1.0], np.float32)).all()  # the env alone
        _set_visibility(pt, w, {0: 255})
        assert np.array_equal(_trace(pt, rays).view(np.uint32), full_hits.view(np.uint32))
        _assert_render_equals(_render(pt, 2), oracle.OracleScene(desc).render(spp=2), "shown")
    finally:
        pt.close_engine()


@pytest.mark.parametrize("accel", ["flat", "two_level", "two_level_object"])
@pytest.mark.parametrize("ntri", [1, 5])
def test_two_instances_hidden_in_turn(ntri, accel, monkeypatch):
    _accel(monkeypatch, accel)
    w = tiny_world(ntri, instances=2)
    desc = w.desc()
    rays = tiny_rays()
    pt = _pass(w)
    try:
        for masks in ({0: 0, 1: 1}, {0: 1, 1: 0}, {0: 0, 1: 0}, {0: 1, 1: 1}):
            hidden = tuple(i for i, m in masks.items() if (m & 0xFF) == 0)
            _set_visibility(pt, w, masks)
            ref = oracle_hits(desc, hidden, rays)
            assert np.array_equal(_trace(pt, rays).view(np.uint32), ref.view(np.uint32)), (masks,)
            fd = env_only_desc(desc) if len(hidden) == 2 else filtered_desc(desc, hidden)
            _assert_render_equals(_render(pt, 1), oracle.OracleScene(fd).render(spp=1), masks)
    finally:
        pt.close_engine()


# ------------------------------------------------------------------ 6. pipelined sequence
def test_hide_between_pipelined_onruns(monkeypatch):
    """test_pipelined_onrun_sequence's "group" case: an instance is hidden between two continued OnRuns
    while split iterations of frames ahead are in flight; they are dropped, and the accumulation
    restarts on the filtered scene."""
    import torch

    monkeypatch.setenv("PUPIL_PIPE_GROUP_MAX", "4")
    w = scenes.sphere_field(8, 48, 32, 4, seed=5, merge=False)
    desc = w.desc()
    monkeypatch.setenv("PUPIL_PIPE_GROUP_PATHS", str(4 * desc.width * desc.height - 1))
    pt = _pass(w)
    try:
        def step(k, o):
            pt.render(1)
            torch.cuda.synchronize()
            got = {k2: pt.buffers.get(k2).cpu().numpy() for k2 in KEYS}
            _assert_render_equals(got, o.render(spp=k), k)

        o = oracle.OracleScene(desc)
        for k in range(1, 2 * desc.max_depth + 2):
            step(k, o)
        assert pt.stats()["frames_in_flight"] >= 1
        w.set_instance_visibility(4, 0)
        pt.update_instances(w, [4])
        o = oracle.OracleScene(filtered_desc(desc, (4,)))
        for k in range(1, desc.max_depth + 2):
            step(k, o)
    finally:
        pt.close_engine()


# ------------------------------------------------------------------ 7. flow
@pytest.mark.parametrize("accel", ["flat", "two_level"])
def test_flow_reports_what_lies_behind_a_hidden_instance(accel, monkeypatch):
    """motion_vectors() with a hidden foreground instance equals the flow of an engine created from
    the filtered desc (the previous camera is a shifted one, so the flow depends on the depth seen)."""
    import torch

    _accel(monkeypatch, accel)
    w = scenes.sphere_field(8, 48, 32, 4, seed=5, merge=False)
    desc = w.desc()
    # the foreground instance: the one most centre rays hit first
    o = oracle.OracleScene(desc)
    rays = np.array([o.camera_ray(p, 0) for p in range(0, desc.width * desc.height, 7)], np.float32)
    ids = o.closest(rays)[:, 3].view(np.uint32)
    first = np.concatenate([[0], np.cumsum(prim_counts(desc))])
    inst = np.searchsorted(first, ids[ids != MISS], side="right") - 1
    fg = int(np.bincount(inst[inst < 8]).argmax())
    prev_c2w = np.array(list(desc.camera_to_world), np.float32)
    prev_c2w[3] += 0.25
    prev_cam = (list(desc.sample_to_camera), prev_c2w.tolist())
    pt = _pass(w)
    other = _pass(filtered_desc(desc, (fg,)))
    try:
        shown = pt.motion_vectors(prev_cam).cpu().numpy().copy()
        _set_visibility(pt, w, {fg: 0})
        pt.render(1)
        got = pt.motion_vectors(prev_cam).cpu().numpy().copy()
        want = other.motion_vectors(prev_cam).cpu().numpy().copy()
        torch.cuda.synchronize()
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
        assert not np.array_equal(got.view(np.uint32), shown.view(np.uint32))
        # a static camera and no argument: still the filtered engine's flow
        pt.render(1)
        other.render(1)
        other.render(1)
        a, b = pt.motion_vectors().cpu().numpy(), other.motion_vectors().cpu().numpy()
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    finally:
        pt.close_engine()
        other.close_engine()


# ------------------------------------------------------------------ 8. exported tree after a hide
def _decode_children(node_bytes):
    f = node_bytes.view(np.float32)
    u = node_bytes.view(np.uint32)
    i = node_bytes.view(np.int32)
    org = np.array([f[0], f[1], f[2]], np.float32)
    scale = np.array([f[3], f[14], f[15]], np.float32)
    out = []
    for k in range(4):
        qlo = np.array([(u[8 + a] >> (8 * k)) & 0xFF for a in range(3)], np.float32)
        qhi = np.array([(u[11 + a] >> (8 * k)) & 0xFF for a in range(3)], np.float32)
        out.append((int(i[4 + k]), org + qlo * scale, org + qhi * scale))  # float32: the traversal's decode
    return out


def test_exported_tree_after_a_hide_bounds_every_visible_record(monkeypatch):
    """Flattened BVH4 after a hide: every record of a visible primitive lies inside the decoded child
    box of every ancestor; the records of hidden instances keep their id words and bound nothing."""
    _accel(monkeypatch, "flat")
    w = mixed_field()
    desc = w.desc()
    pt = _pass(w)
    try:
        _set_visibility(pt, w, {i: 0 for i in MIXED_HIDDEN})
        nodes, recs, root = pt.export_bvh4()
        st = pt.stats()
    finally:
        pt.close_engine()
    assert root == 0 and len(nodes) > 1
    assert np.isfinite(st["node_bound"]).all()
    EMPTY, SPHERE = 0x7FFFFFFF, 0x80000000
    words = recs.view(np.uint32)
    seen_visible = seen_hidden = 0
    stack = [(0, [])]  # node, ancestor boxes
    while stack:
        j, boxes = stack.pop()
        for link, lo, hi in _decode_children(nodes[j]):
            if link == EMPTY:
                continue
            if link >= 0:
                stack.append((link, boxes + [(lo, hi)]))
                continue
            first, count = ((~link) & 0xFFFFFFFF) >> 3, (((~link) & 0xFFFFFFFF) & 7) + 1
            for r in range(first, first + count):
                inst = int(words[r, 7])
                assert inst < desc.num_instances
                if inst in MIXED_HIDDEN:
                    seen_hidden += 1
                    assert np.isnan(recs[r, 0:3]).all()
                    continue
                seen_visible += 1
                if words[r, 3] & SPHERE:
                    rlo, rhi = recs[r, 0:3] - recs[r, 4:7], recs[r, 0:3] + recs[r, 4:7]
                else:
                    v = recs[r, [0, 1, 2, 4, 5, 6, 8, 9, 10]].reshape(3, 3)
                    rlo, rhi = v.min(0), v.max(0)
                for blo, bhi in boxes + [(lo, hi)]:
                    assert (blo <= rlo).all() and (rhi <= bhi).all(), (j, r)
    cnt = prim_counts(desc)
    assert seen_hidden == sum(cnt[i] for i in MIXED_HIDDEN)
    assert seen_visible == cnt.sum() - seen_hidden


# ------------------------------------------------------------------ 9. C++ drop-in
def _read_pfm(path):
    with open(path, "rb") as f:
        assert f.readline().strip() == b"PF"
        w, h = map(int, f.readline().split())
        scale = float(f.readline())
        data = np.frombuffer(f.read(), dtype="<f4" if scale < 0 else ">f4")
    return data.reshape(h, w, 3)


def test_example_pupil_hide_matches_python_pass():
    """PUPIL_HIDE=3 build/pupil_path_tracer on the sphere field == the Python pass == the filtered oracle."""
    assert os.path.exists(EXE), "C++ host layer not built (run __graft_entry__.build())"
    with tempfile.TemporaryDirectory(prefix="pupil_vis_") as tmp:
        xw = scenes.XmlWorld()
        scenes.sphere_field(8, 48, 32, 4, seed=5, merge=False, world=xw)
        xml = xw.save(os.path.join(tmp, "field.xml"))
        out = os.path.join(tmp, "field.pfm")
        r = subprocess.run([EXE, xml, "3", out], capture_output=True, text=True, timeout=300,
                           env=dict(os.environ, PUPIL_HIDE="3"))
        assert r.returncode == 0, r.stderr
        img = _read_pfm(out).reshape(-1, 3)
        w = World().load_scene(xml)
        w.set_instance_visibility(3, 0)
        pt = _pass(w)
        for _ in range(3):
            pt.on_run()
        py = pt.buffers.get("final result").cpu().numpy()[:, :3]
        pt.close_engine()
        assert np.array_equal(img, py)
        ref = oracle.OracleScene(filtered_desc(w.desc(), (3,))).render(spp=3)["accum"][:, :3]
        assert np.array_equal(img, ref)
        r = subprocess.run([EXE, xml, "1", out], capture_output=True, text=True, timeout=300,
                           env=dict(os.environ, PUPIL_HIDE="99"))
        assert r.returncode == 2 and "PUPIL_HIDE" in r.stderr
