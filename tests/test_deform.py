"""Deformable meshes: pupil_pt_update_shape_vertices replaces a shape's vertices and refits in
place (flattened BVH: world records, nodes, shading records; two-level: BLAS records, BLAS,
shading records, vmax and margins, world records / BLAS copies, TLAS).

Hit results do not depend on the BVH topology, so a render after an update must equal, bit for
bit, a freshly created engine on the deformed mesh and the CPU oracle's render of a world built
from scratch on it.  Mesh: scenes.uv_sphere(12, 8) (168 triangles, several BVH4 levels, odd leaf
sizes); film 64 x 48, 2 spp, depth 4."""
import functools

import numpy as np
import pytest

import oracle
from pupiloptixlab_amd import World, abi, scenes
from pupiloptixlab_amd import world as W

from test_bvh_invariants import _leaf_size, _records_by_id, check_bvh4
from test_visibility import KEYS, _assert_render_equals, _random_rays, _render, _trace, filtered_desc

pytestmark = pytest.mark.gpu

ACCELS = ["flat", "two_level", "two_level_object"]
SPP = 2


def _accel(monkeypatch, accel):
    """flat | two_level (PUPIL_TL_MODE=world) | two_level_object"""
    monkeypatch.setenv("PUPIL_ACCEL", "flat" if accel == "flat" else "two_level")
    if accel != "flat":
        monkeypatch.setenv("PUPIL_TL_MODE", "object" if accel == "two_level_object" else "world")


# ------------------------------------------------------------------ meshes and deformations
@functools.lru_cache(maxsize=None)
def base_mesh():
    v, nrm, uv, idx = scenes.uv_sphere(12, 8)
    return (np.asarray(v, np.float32).reshape(-1, 3), np.asarray(nrm, np.float32).reshape(-1, 3),
            np.asarray(uv, np.float32).reshape(-1, 2), np.asarray(idx, np.uint32).reshape(-1, 3))


def vertex_normals(p, idx):
    """area-weighted vertex normals of the deformed mesh"""
    n = np.zeros_like(p, dtype=np.float64)
    f = np.cross(p[idx[:, 1]] - p[idx[:, 0]], p[idx[:, 2]] - p[idx[:, 0]]).astype(np.float64)
    for k in range(3):
        np.add.at(n, idx[:, k], f)
    ln = np.linalg.norm(n, axis=1, keepdims=True)
    n = np.where(ln > 0, n / np.maximum(ln, 1e-30), [[0.0, 1.0, 0.0]])
    return n.astype(np.float32)


def bulge(p):
    """(a): z scaled by 1 + 0.8 sin(3x): vertices leave the original bounds (|z| up to 1.8)"""
    q = p.copy()
    q[:, 2] *= (1.0 + 0.8 * np.sin(3.0 * p[:, 0])).astype(np.float32)
    return q


def shrink(p):
    """(b): 0.4 x: every box must tighten"""
    return (0.4 * p).astype(np.float32)


def triple(p):
    """the largest |coordinate| triples (vmax, instance margins)"""
    return (3.0 * p).astype(np.float32)


# ------------------------------------------------------------------ worlds
def _finish(w):
    w.add_const_env((0.8, 0.9, 1.0))
    w.set_film(64, 48, 4)
    w.set_sensor(45.0, W.look_at_mitsuba((0.5, 1.5, -7.0), (0.0, 0.2, 0.0), (0, 1, 0)))
    return w


def _floor(w):
    m = w.add_material(W.twosided(W.diffuse((0.6, 0.6, 0.55))))
    w.add_instance(w.add_builtin("rectangle"), m,
                   W.transform(scale=(6, 6, 1), rotate=((1, 0, 0), -90), translate=(0.0, -2.2, 0.0)))


def single_world(pos, nrm, emissive=False):
    """instance 0: the deformable mesh (shape 0), instance 1: the floor"""
    _, _, uv, idx = base_mesh()
    w = World()
    s = w.add_mesh(pos, idx, nrm, uv)
    m = w.add_material(W.twosided(W.diffuse((0.7, 0.4, 0.3))))
    w.add_instance(s, m, W.transform(scale=(1.1, 0.9, 1.0), rotate=((1, 2, 0), 25), translate=(0.2, 0.1, 0.3)),
                   emitter_radiance=(4.0, 3.0, 2.0) if emissive else None)
    _floor(w)
    return _finish(w)


def shared_world(pos, nrm):
    """instances 0 and 1: the deformable shape under two transforms; 2: a cube; 3: the floor"""
    _, _, uv, idx = base_mesh()
    w = World()
    s = w.add_mesh(pos, idx, nrm, uv)
    m = w.add_material(W.twosided(W.diffuse((0.7, 0.4, 0.3))))
    w.add_instance(s, m, W.transform(scale=(0.9, 0.9, 0.9), rotate=((0, 1, 0), 40), translate=(-1.6, 0.0, 0.0)))
    w.add_instance(s, m, W.transform(scale=(0.6, 1.1, 0.8), rotate=((1, 0, 1), -30), translate=(1.5, 0.3, 0.8)))
    w.add_instance(w.add_builtin("cube"), w.add_material(W.diffuse((0.3, 0.5, 0.8))),
                   W.transform(scale=(0.4, 0.4, 0.4), rotate=((0, 1, 0), 20), translate=(0.0, -1.2, -1.5)))
    _floor(w)
    return _finish(w)


def two_triangle_world(pos):
    w = World()
    s = w.add_mesh(pos, np.array([[0, 1, 2], [3, 4, 5]], np.uint32))
    w.add_instance(s, w.add_material(W.twosided(W.diffuse((0.5, 0.5, 0.5)))), W.transform(translate=(0.1, 0.0, 0.5)))
    w.add_const_env((0.8, 0.9, 1.0))
    w.set_film(64, 48, 4)
    w.set_sensor(40.0, W.look_at_mitsuba((0, 0, -4), (0, 0, 0), (0, 1, 0)))
    return w


TWO_TRI = np.array([[-1, -1, 0], [1, -1, 0], [0, 1, 0], [-1, -1, 0.4], [1, -1, 0.4], [0, 1, 0.4]], np.float32)

BUILDERS = {"single": single_world, "shared": shared_world, "emissive": functools.partial(single_world, emissive=True)}


@functools.lru_cache(maxsize=None)
def state(kind, deform, normals):
    """(positions, normals) of a deformation of the base mesh; normals: 'new' | 'kept'"""
    p0, n0, _, idx = base_mesh()
    p = {"none": lambda x: x, "bulge": bulge, "shrink": shrink, "triple": triple}[deform](p0)
    return p, (vertex_normals(p, idx) if normals == "new" and deform != "none" else n0)


@functools.lru_cache(maxsize=None)
def oracle_ref(kind, deform, normals, hidden=()):
    """the oracle's render of a world built FROM SCRATCH on the deformed mesh (computed once)"""
    p, n = state(kind, deform, normals)
    desc = BUILDERS[kind](p, n).desc()
    return oracle.OracleScene(filtered_desc(desc, hidden) if hidden else desc).render(spp=SPP)


def _pass(world_or_desc):
    from pupiloptixlab_amd.pt_pass import PTPass

    pt = PTPass(device=0)
    pt.set_scene(world_or_desc)
    return pt


def _fresh(kind, deform, normals, rays=None):
    """render (and hits) of a freshly created engine on the deformed mesh"""
    p, n = state(kind, deform, normals)
    pt = _pass(BUILDERS[kind](p, n))
    try:
        img = _render(pt, SPP)
        hits = None if rays is None else (_trace(pt, rays), _trace(pt, rays, any_hit=1))
        return img, hits
    finally:
        pt.close_engine()


def _deform(pt, w, kind, deform, normals, **kw):
    p, n = state(kind, deform, normals)
    w.set_mesh_vertices(0, p, n if normals == "new" else None)
    pt.update_shape(w, 0, **kw)


def _same(a, b, what):
    for k in KEYS:
        assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), (what, k)


def _same_any(out, ref, what):
    """any hit: t (1 occluded, -1 not) and the id word (always the miss id) bit for bit.  b1 / b2
    are those of whichever occluder the traversal met first, which depends on the tree's topology
    and so legitimately differs between a refitted and a freshly built tree."""
    assert np.array_equal(out[:, [0, 3]].view(np.uint32), ref[:, [0, 3]].view(np.uint32)), what


def _rays():
    return _random_rays(4096, [-4, -2, -5], [4, 3, 4], 11)


# ------------------------------------------------------------------ 1. images
@pytest.mark.parametrize("accel", ACCELS)
def test_update_equals_fresh_engine_and_oracle(accel, monkeypatch):
    """(a) with the normals kept, then (b) with recomputed normals, on the same engine: every
    buffer equals a fresh engine's and the oracle's, and differs from the render before."""
    _accel(monkeypatch, accel)
    w = single_world(*state("single", "none", "kept"))
    pt = _pass(w)
    try:
        prev = _render(pt, SPP)
        _assert_render_equals(prev, oracle_ref("single", "none", "kept"), "undeformed")
        for deform, normals in (("bulge", "kept"), ("shrink", "new")):  # "kept" = the normals of create
            before = pt.stats()["accel_refits"]
            _deform(pt, w, "single", deform, normals)
            st = pt.stats()
            assert st["accel_refits"] == before + 1 and st["build_ms"] > 0.0
            got = _render(pt, SPP)
            for k in ("pt accum buffer", "albedo", "normal"):
                assert not np.array_equal(got[k], prev[k]), (deform, k)
            _same(got, _fresh("single", deform, normals)[0], (accel, deform, "fresh engine"))
            _assert_render_equals(got, oracle_ref("single", deform, normals), (accel, deform, "oracle"))
            prev = got
    finally:
        pt.close_engine()


# ------------------------------------------------------------------ 2. rays
@pytest.mark.parametrize("accel", ACCELS)
def test_random_rays_equal_fresh_engine(accel, monkeypatch):
    _accel(monkeypatch, accel)
    rays = _rays()
    w = single_world(*state("single", "none", "kept"))
    pt = _pass(w)
    try:
        hit0 = _trace(pt, rays)
        for deform in ("bulge", "shrink"):
            _deform(pt, w, "single", deform, "new")
            ref, ref_any = _fresh("single", deform, "new", rays)[1]
            out = _trace(pt, rays)
            assert (ref[:, 0] > 0).mean() > 0.1
            assert not np.array_equal(out.view(np.uint32), hit0.view(np.uint32))
            bad = (out.view(np.uint32) != ref.view(np.uint32)).any(axis=1)
            assert not bad.any(), f"{accel} {deform}: {bad.sum()} closest hits differ"
            _same_any(_trace(pt, rays, any_hit=1), ref_any, (accel, deform))
    finally:
        pt.close_engine()


# ------------------------------------------------------------------ 3. a shared shape
@pytest.mark.parametrize("accel", ACCELS)
def test_shared_shape_updates_every_instance_with_one_refit(accel, monkeypatch):
    _accel(monkeypatch, accel)
    w = shared_world(*state("shared", "none", "kept"))
    pt = _pass(w)
    try:
        prev = _render(pt, SPP)
        before = pt.stats()["accel_refits"]
        _deform(pt, w, "shared", "bulge", "new")
        assert pt.stats()["accel_refits"] == before + 1
        got = _render(pt, SPP)
        assert not np.array_equal(got["normal"], prev["normal"])
        _same(got, _fresh("shared", "bulge", "new")[0], (accel, "fresh engine"))
        _assert_render_equals(got, oracle_ref("shared", "bulge", "new"), (accel, "oracle"))
    finally:
        pt.close_engine()


# ------------------------------------------------------------------ 4. an emissive mesh
@pytest.mark.parametrize("accel", ACCELS)
def test_emissive_mesh_host_path_and_device_refusal(accel, monkeypatch):
    import torch

    _accel(monkeypatch, accel)
    w = single_world(*state("emissive", "none", "kept"), emissive=True)
    assert w.desc().instances[0].emitter_offset >= 0
    pt = _pass(w)
    try:
        prev = _render(pt, SPP)
        p, _ = state("emissive", "bulge", "new")
        with pytest.raises(abi.PupilError) as e:
            pt.update_shape_device(0, torch.from_numpy(p).to(pt.device))
        assert e.value.code == abi.ERR_UNSUPPORTED
        _same(_render(pt, SPP), prev, "a refused update changes nothing")
        _deform(pt, w, "emissive", "bulge", "new")
        got = _render(pt, SPP)
        assert not np.array_equal(got["pt accum buffer"], prev["pt accum buffer"])
        _same(got, _fresh("emissive", "bulge", "new")[0], (accel, "fresh engine"))
        _assert_render_equals(got, oracle_ref("emissive", "bulge", "new"), (accel, "oracle"))
    finally:
        pt.close_engine()


# ------------------------------------------------------------------ 5. device tensors
@pytest.mark.parametrize("accel", ACCELS)
def test_device_tensor_path_equals_host_path(accel, monkeypatch):
    """The vertices are produced on a side stream (a torch op scaling the tensor by 0.4) and handed
    over on that stream with no synchronisation in between: the update waits for the producer."""
    import torch

    _accel(monkeypatch, accel)
    p0, n0 = state("single", "none", "kept")
    w = single_world(p0, n0)
    pt = _pass(w)
    try:
        _render(pt, SPP)
        side = torch.cuda.Stream(device=pt.device)
        src = torch.from_numpy(p0).to(pt.device)
        filler = torch.ones((2048, 2048), device=pt.device)
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            for _ in range(8):  # work ahead of the producer on the same stream
                filler = filler @ filler * 1e-4
            dev = src * 0.4  # float32: exactly shrink()'s product
        before = pt.stats()["accel_refits"]
        pt.update_shape_device(0, dev, stream=side)
        assert pt.stats()["accel_refits"] == before + 1
        got = _render(pt, SPP)
        assert np.array_equal(dev.cpu().numpy(), shrink(p0))
        _same(got, _fresh("single", "shrink", "kept")[0], (accel, "fresh engine"))
        # the host path on a second engine
        w2 = single_world(p0, n0)
        pt2 = _pass(w2)
        try:
            _deform(pt2, w2, "single", "shrink", "kept")
            _same(got, _render(pt2, SPP), (accel, "host path"))
        finally:
            pt2.close_engine()
        # normals on the device too, and a rebuild from device vertices
        p1, n1 = state("single", "bulge", "new")
        pt.update_shape_device(0, torch.from_numpy(p1).to(pt.device), torch.from_numpy(n1).to(pt.device), rebuild=True)
        _same(_render(pt, SPP), _fresh("single", "bulge", "new")[0], (accel, "device rebuild"))
    finally:
        pt.close_engine()


# ------------------------------------------------------------------ 6. a hidden instance
@pytest.mark.parametrize("accel", ACCELS)
def test_hidden_instance_stays_hidden_and_shows_the_new_vertices(accel, monkeypatch):
    _accel(monkeypatch, accel)
    w = shared_world(*state("shared", "none", "kept"))
    pt = _pass(w)
    try:
        w.set_instance_visibility(1, 0)
        pt.update_instances(w, [1])
        _deform(pt, w, "shared", "bulge", "new")
        assert pt.stats()["hidden_instances"] == 1
        _assert_render_equals(_render(pt, SPP), oracle_ref("shared", "bulge", "new", hidden=(1,)), (accel, "hidden"))
        p, n = state("shared", "bulge", "new")
        hidden = _pass(filtered_desc(shared_world(p, n).desc(), (1,)))
        try:
            ref = _render(hidden, SPP)
        finally:
            hidden.close_engine()
        _same(_render(pt, SPP), ref, (accel, "fresh engine without the instance"))
        w.set_instance_visibility(1, 1)
        pt.update_instances(w, [1])
        _same(_render(pt, SPP), _fresh("shared", "bulge", "new")[0], (accel, "shown again"))
    finally:
        pt.close_engine()


# ------------------------------------------------------------------ 7. frames in flight
@pytest.mark.parametrize("accel", ACCELS)
def test_update_between_pipelined_renders(accel, monkeypatch):
    import torch

    _accel(monkeypatch, accel)
    w = single_world(*state("single", "none", "kept"))
    pt = _pass(w)
    try:
        for _ in range(6):
            pt.render(1, continues=True)
        assert pt.stats()["frames_in_flight"] > 0
        _deform(pt, w, "single", "bulge", "new")  # no synchronisation: ordered after the renders
        got = _render(pt, SPP)
        torch.cuda.synchronize()
        _same(got, _fresh("single", "bulge", "new")[0], accel)
    finally:
        pt.close_engine()


# ------------------------------------------------------------------ 8. a root-leaf scene
@pytest.mark.parametrize("accel", ACCELS)
def test_root_leaf_scene_stays_exact(accel, monkeypatch):
    _accel(monkeypatch, accel)
    moved = (TWO_TRI * np.array([1.6, 0.7, 1.0], np.float32) + np.array([0.3, 0.2, -0.5], np.float32)).astype(np.float32)
    w = two_triangle_world(TWO_TRI)
    pt = _pass(w)
    try:
        prev = _render(pt, SPP)
        before = pt.stats()["accel_refits"]
        w.set_mesh_vertices(0, moved)
        pt.update_shape(w, 0)
        assert pt.stats()["accel_refits"] == before + 1
        got = _render(pt, SPP)
        assert not np.array_equal(got["pt accum buffer"], prev["pt accum buffer"])
        desc1 = two_triangle_world(moved).desc()
        _assert_render_equals(got, oracle.OracleScene(desc1).render(spp=SPP), accel)
        fresh = _pass(desc1)
        try:
            _same(got, _render(fresh, SPP), (accel, "fresh engine"))
        finally:
            fresh.close_engine()
    finally:
        pt.close_engine()


# ------------------------------------------------------------------ 9. PUPIL_VERTS_REBUILD
@pytest.mark.parametrize("accel", ACCELS)
def test_rebuild_gives_the_same_images(accel, monkeypatch):
    _accel(monkeypatch, accel)
    w = shared_world(*state("shared", "none", "kept"))
    pt = _pass(w)
    try:
        w.set_instance_visibility(2, 0)  # the masks go back on after the rebuild
        pt.update_instances(w, [2])
        _deform(pt, w, "shared", "bulge", "new")
        refit = _render(pt, SPP)
        before = pt.stats()["accel_refits"]
        _deform(pt, w, "shared", "shrink", "new", rebuild=True)
        _deform(pt, w, "shared", "bulge", "new", rebuild=True)
        st = pt.stats()
        assert st["accel_refits"] == before + 2 and st["hidden_instances"] == 1
        _same(_render(pt, SPP), refit, accel)
        _assert_render_equals(refit, oracle_ref("shared", "bulge", "new", hidden=(2,)), accel)
    finally:
        pt.close_engine()


# ------------------------------------------------------------------ 10. the exported tree
def test_flat_tree_passes_the_exact_bounds_check(monkeypatch):
    """After each update the exported BVH4 satisfies what test_bvh_invariants asks of a refit
    (every child box contains the exact bounds under it, the topology is kept), and its records
    equal a fresh engine's."""
    _accel(monkeypatch, "flat")
    w = shared_world(*state("shared", "none", "kept"))
    pt = _pass(w)
    try:
        desc = w.desc()
        n_prims = sum(desc.shapes[desc.instances[i].shape].num_faces for i in range(desc.num_instances))
        n0 = pt.stats()
        check_bvh4(*pt.export_bvh4(), n_prims, _leaf_size(), stats=n0)
        for deform in ("bulge", "shrink"):
            _deform(pt, w, "shared", deform, "new")
            stats = pt.stats()
            nodes, recs, root = pt.export_bvh4()
            info = check_bvh4(nodes, recs, root, n_prims, _leaf_size(), refit=True, stats=stats)
            assert info["nodes"] == n0["bvh_nodes"]
            p, n = state("shared", deform, "new")
            fresh = _pass(shared_world(p, n))
            try:
                f_recs = fresh.export_bvh4()[1]
            finally:
                fresh.close_engine()
            assert np.array_equal(_records_by_id(recs), _records_by_id(f_recs)), deform
    finally:
        pt.close_engine()


# ------------------------------------------------------------------ 11. vmax and margins
@pytest.mark.parametrize("accel", ["two_level", "two_level_object"])
def test_two_level_tripled_coordinates(accel, monkeypatch):
    """The largest |coordinate| triples: a stale vmax leaves the object-space margins too small."""
    _accel(monkeypatch, accel)
    rays = _random_rays(4096, [-6, -2, -6], [6, 5, 6], 13)
    w = shared_world(*state("shared", "none", "kept"))
    pt = _pass(w)
    try:
        assert pt.stats()["two_level"] == 1
        _deform(pt, w, "shared", "triple", "kept")
        ref_img, (ref, ref_any) = _fresh("shared", "triple", "kept", rays)
        assert (ref[:, 0] > 0).mean() > 0.2
        out = _trace(pt, rays)
        bad = (out.view(np.uint32) != ref.view(np.uint32)).any(axis=1)
        assert not bad.any(), f"{accel}: {bad.sum()} closest hits differ"
        _same_any(_trace(pt, rays, any_hit=1), ref_any, accel)
        _same(_render(pt, SPP), ref_img, accel)
    finally:
        pt.close_engine()


# ------------------------------------------------------------------ 12. argument checks on a live engine
@pytest.mark.parametrize("accel", ["flat", "two_level"])
def test_invalid_arguments_on_a_live_engine(accel, monkeypatch):
    """The C entry called directly: a sphere shape, a shape out of range, null positions, normals
    for a mesh created without them and unknown flags return PUPIL_ERR_INVALID, tick no counter
    and change no pixel; a failed call is followed by a valid one that works."""
    import ctypes as C

    from test_deform_host import _mesh, _world

    _accel(monkeypatch, accel)
    pos, nrm, _, _ = _mesh()
    w = _world(pos, nrm, emissive=False)  # shape 0: the mesh, 1: a builtin sphere, 2: a mesh without normals
    desc = w.desc()
    assert desc.shapes[1].kind == abi.SHAPE_SPHERE and not desc.shapes[2].normals
    pt = _pass(w)
    try:
        prev = _render(pt, SPP)
        before = pt.stats()["accel_refits"]
        call = pt._lib.pupil_pt_update_shape_vertices
        vp = lambda a: np.ascontiguousarray(a, np.float32).ctypes.data_as(C.c_void_p)
        tri = np.ctypeslib.as_array(desc.shapes[2].positions, (3, 3)).copy()
        assert call(pt._pt, 1, vp(pos), None, 0, None) == abi.ERR_INVALID            # a sphere
        assert call(pt._pt, desc.num_shapes, vp(pos), None, 0, None) == abi.ERR_INVALID  # out of range
        assert call(pt._pt, 0xFFFFFFFF, vp(pos), None, 0, None) == abi.ERR_INVALID
        assert call(pt._pt, 0, None, None, 0, None) == abi.ERR_INVALID               # null positions
        assert call(pt._pt, 0, None, vp(nrm), 0, None) == abi.ERR_INVALID
        assert call(pt._pt, 2, vp(tri), vp(tri), 0, None) == abi.ERR_INVALID         # normals it never had
        assert call(pt._pt, 0, vp(pos), None, 4, None) == abi.ERR_INVALID            # unknown flags
        assert call(pt._pt, 0, vp(pos), None, 0x80000001, None) == abi.ERR_INVALID
        assert pt._lib.pupil_last_error()
        assert pt.stats()["accel_refits"] == before
        _same(_render(pt, SPP), prev, "refused updates change nothing")
        assert call(pt._pt, 2, vp(tri), None, 0, None) == abi.OK                      # the same mesh, no normals
        assert call(pt._pt, 0, vp(bulge(pos)), vp(nrm), 0, None) == abi.OK
        assert pt.stats()["accel_refits"] == before + 2
        assert not np.array_equal(_render(pt, SPP)["pt accum buffer"], prev["pt accum buffer"])
        with pytest.raises(ValueError):
            pt.update_shape_device(0, __import__("torch").zeros(3, device=pt.device))
        with pytest.raises(abi.PupilError):
            pt.update_shape_device(99, __import__("torch").zeros(3, device=pt.device))
    finally:
        pt.close_engine()
