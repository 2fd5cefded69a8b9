"""A mesh replaced by one of new topology, in place (pupil_pt_replace_shape_mesh): the engine must
equal, bit for bit, an engine freshly created on the updated world -- render AOVs, the camera
G-buffer, radiance along fixed rays, flow -- on the flattened BVH and both two-level modes.

Scene: replace_mesh_cases.world (109 primitives with the cube; 48 x 48, 2 spp, depth 4).  Hit
results do not depend on the tree's topology and every builder is deterministic, so equality is
exact: outputs are compared as bit patterns, no tolerance."""
import ctypes as C

import numpy as np
import pytest

from pupiloptixlab_amd import abi

import replace_mesh_cases as cases
from replace_mesh_cases import HIDDEN, LAMP, S, SPHERE

ACCELS = ["flat", "two_level", "two_level_object"]
SPP = 2
AOVS = ("pt accum buffer", "albedo", "normal")


def _accel(monkeypatch, accel):
    """flat | two_level (PUPIL_TL_MODE=world) | two_level_object"""
    monkeypatch.setenv("PUPIL_ACCEL", "flat" if accel == "flat" else "two_level")
    if accel != "flat":
        monkeypatch.setenv("PUPIL_TL_MODE", "object" if accel == "two_level_object" else "world")


def _pass(world):
    """an engine on `world`, with the visibility masks the world holds (create shows everything)"""
    from pupiloptixlab_amd.pt_pass import PTPass

    pt = PTPass(device=0)
    pt.set_scene(world)
    hidden = [i for i in range(world.desc().num_instances) if world.instance_visibility(i) & 0xFF == 0]
    if hidden:
        pt.update_instances(world, hidden)
    return pt


def _bits(t):
    a = t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)
    return np.ascontiguousarray(a).view(np.uint8).copy()


def _outputs(pt, flow=False):
    """everything the issue compares, as bytes: the render's AOVs, primary_hits, radiance on the
    fixed rays and, on request, the flow of a static camera"""
    import torch

    pt.mark_dirty()
    pt.render(SPP)
    torch.cuda.synchronize()
    out = {k: _bits(pt.buffers.get(k)) for k in AOVS}
    for k, v in pt.primary_hits().items():
        out["hits." + k] = _bits(v)
    rays = torch.from_numpy(cases.fixed_rays()).to(pt.device)
    for k, v in pt.radiance(rays, spp=SPP, seed=3, want=("radiance", "albedo", "normal")).items():
        out["radiance." + k] = _bits(v)
    if flow:
        out["flow"] = _bits(pt.motion_vectors(prev_camera=pt._cam))
    torch.cuda.synchronize()
    return out


def _same(got, ref, what):
    assert got.keys() == ref.keys()
    for k in got:
        assert np.array_equal(got[k], ref[k]), (what, k, int((got[k] != ref[k]).sum()))


def _fresh(world, flow=False, prepare=None):
    pt = _pass(world)
    try:
        if prepare:
            prepare(pt)
        return _outputs(pt, flow), pt.stats(), pt.prim_tables()
    finally:
        pt.close_engine()


def _same_tables(got, ref, what):
    assert got["num_prims"] == ref["num_prims"] and got["guide_shift"] == ref["guide_shift"], what
    for k in ("prim_inst", "inst_first", "inst_guide"):
        assert np.array_equal(got[k], ref[k]), (what, k)


def _replace(pt, w, name, device=False):
    m = cases.set_mesh(w, name)
    if not device:
        pt.replace_shape(S, m["positions"], m["faces"], m["normals"], m["texcoords"])
        return
    import torch

    side = torch.cuda.Stream(pt.device)
    with torch.cuda.stream(side):  # produced on a side stream; the call is made behind it
        t = {k: None if v is None else torch.from_numpy(v.astype(np.int32) if k == "faces" else v).to(pt.device) + 0
             for k, v in m.items()}
        pt.replace_shape_device(S, t["positions"], t["faces"], t["normals"], t["texcoords"], stream=side)
    side.synchronize()


# ------------------------------------------------------------------ 1. grow and shrink
@pytest.mark.gpu
@pytest.mark.parametrize("accel", ACCELS)
def test_grow_and_shrink(accel, monkeypatch):
    _accel(monkeypatch, accel)
    w = cases.world("cube")
    pt = _pass(w)
    try:
        before = _outputs(pt)
        for name in ("icosphere", "tetrahedron"):
            _replace(pt, w, name)
            got = _outputs(pt)
            ref, _, tables = _fresh(w)
            assert not np.array_equal(got["pt accum buffer"], before["pt accum buffer"]), name
            _same(got, ref, (accel, name))
            _same_tables(pt.prim_tables(), tables, (accel, name))
        w.set_instance_visibility(HIDDEN, 1)  # the hidden instance shows the new mesh when shown
        pt.update_instances(w, [HIDDEN])
        _same(_outputs(pt), _fresh(w)[0], (accel, "shown"))
    finally:
        pt.close_engine()


# ------------------------------------------------------------------ 2. the guide's shift
@pytest.mark.gpu
@pytest.mark.parametrize("accel", ACCELS)
def test_guide_shift_crossing(accel, monkeypatch):
    _accel(monkeypatch, accel)
    w = cases.world("cube")
    pt = _pass(w)
    try:
        first = pt.prim_tables()
        assert first["guide_shift"] == 0 and first["num_prims"] == 109
        _replace(pt, w, "grid")
        ref, _, tables = _fresh(w)
        got_tables = pt.prim_tables()
        assert got_tables["num_prims"] == 109 - 24 + 2 * 9216 > 8192 and got_tables["guide_shift"] == 2
        _same_tables(got_tables, tables, (accel, "grid"))
        _same(_outputs(pt), ref, (accel, "grid"))
        _replace(pt, w, "cube")
        _same_tables(pt.prim_tables(), first, (accel, "cube again"))
        _same(_outputs(pt), _fresh(w)[0], (accel, "cube again"))
    finally:
        pt.close_engine()


# ------------------------------------------------------------------ 3. host path = device path
@pytest.mark.gpu
@pytest.mark.parametrize("accel", ACCELS)
def test_host_path_equals_device_path(accel, monkeypatch):
    _accel(monkeypatch, accel)
    outs = []
    for device in (False, True):
        w = cases.world("cube")
        pt = _pass(w)
        try:
            _replace(pt, w, "icosphere", device=device)
            outs.append((_outputs(pt), pt.prim_tables()))
            if device:  # and the optional arrays absent, from device memory
                _replace(pt, w, "tetrahedron", device=True)
                _same(_outputs(pt), _fresh(w)[0], (accel, "device tetrahedron"))
        finally:
            pt.close_engine()
    _same(outs[0][0], outs[1][0], accel)
    _same_tables(outs[0][1], outs[1][1], accel)


# ------------------------------------------------------------------ 4. still a shape
@pytest.mark.gpu
@pytest.mark.parametrize("accel", ACCELS)
def test_continues_to_work_as_a_shape(accel, monkeypatch):
    import torch

    from pupiloptixlab_amd import world as W

    _accel(monkeypatch, accel)
    w = cases.world("cube")
    pt = _pass(w)
    try:
        pt.render(1)
        # snapshots of S and of the other mesh, taken before the replacement: S's must go, the
        # other's stays (the flow pass then reads a table of snapshot arrays without S)
        for shape in (S, cases.OTHER):
            abi.check(pt._lib.pupil_pt_snapshot_shape_vertices(pt._pt, shape))
        _replace(pt, w, "icosphere")

        def other_snapshot(f):
            f.render(1)
            abi.check(f._lib.pupil_pt_snapshot_shape_vertices(f._pt, cases.OTHER))

        _same(_outputs(pt, flow=True), _fresh(w, flow=True, prepare=other_snapshot)[0], (accel, "flow"))
        abi.check(pt._lib.pupil_pt_clear_vertex_snapshots(pt._pt))

        m = cases.icosphere()
        p1 = (m["positions"] * np.float32([1.0, 1.3, 0.8])).astype(np.float32)
        old = cases.cube()["positions"]
        with pytest.raises(ValueError):  # the old vertex count
            w.set_mesh_vertices(S, old)
        with pytest.raises(ValueError):
            pt.update_shape_device(S, torch.from_numpy(old).to(pt.device))
        w.set_mesh_vertices(S, p1)
        pt.update_shape(w, S)
        _same(_outputs(pt), _fresh(w)[0], (accel, "update_shape"))
        p2 = (m["positions"] * np.float32([0.7, 1.0, 1.2])).astype(np.float32)
        w.set_mesh_vertices(S, p2)
        pt.update_shape_device(S, torch.from_numpy(p2).to(pt.device))
        _same(_outputs(pt), _fresh(w)[0], (accel, "update_shape_device"))

        ids = list(cases.S_INSTANCES)
        for k, i in enumerate(ids):
            w.set_instance_transform(i, W.transform(scale=(0.6, 0.9, 0.7), rotate=((0, 1, 1), 20 + 30 * k),
                                                    translate=(-1.0 + 2.2 * k, -0.2, 0.4 * k)))
        d = w.desc()
        tw = np.array([list(d.instances[i].to_world) for i in ids], np.float32)
        pt.update_instances_device(torch.from_numpy(tw).to(pt.device),
                                   ids=torch.tensor(ids, dtype=torch.int32, device=pt.device))
        _same(_outputs(pt), _fresh(w)[0], (accel, "update_instances_device"))
    finally:
        pt.close_engine()


# ------------------------------------------------------------------ 5. pipelined frames
@pytest.mark.gpu
@pytest.mark.parametrize("accel", ACCELS)
def test_pipelined_frames(accel, monkeypatch):
    import torch

    _accel(monkeypatch, accel)

    def three(p):
        for _ in range(3):
            p.render(1, continues=True)
        torch.cuda.synchronize()
        return {k: _bits(p.buffers.get(k)) for k in AOVS}

    w = cases.world("cube")
    pt = _pass(w)
    try:
        pt.mark_dirty()
        three(pt)  # leaves frames in flight
        _replace(pt, w, "icosphere")  # drops them; accumulation restarts at seed 0
        got = three(pt)
    finally:
        pt.close_engine()
    f = _pass(w)
    try:
        f.mark_dirty()
        _same(got, three(f), accel)
    finally:
        f.close_engine()


# ------------------------------------------------------------------ 6. refusals
@pytest.mark.gpu
@pytest.mark.parametrize("accel", ACCELS)
def test_refusals_leave_the_engine_untouched(accel, monkeypatch):
    import torch

    _accel(monkeypatch, accel)
    w = cases.world("cube")
    pt = _pass(w)
    try:
        before = _outputs(pt)
        state = (pt.stats()["accel_refits"], pt.stats()["bvh_prims"], pt.replace_info()["replacements"])
        tables = pt.prim_tables()
        m = cases.icosphere()
        bad = m["faces"].copy()
        bad[-1, 2] = len(m["positions"])  # == num_vertices, in the last face
        dev = lambda a, dt=None: torch.from_numpy(a if dt is None else a.astype(dt)).to(pt.device)  # noqa: E731
        mesh = abi.Shape()
        mesh.kind, mesh.num_vertices, mesh.num_faces = abi.SHAPE_MESH, len(m["positions"]), len(m["faces"])
        mesh.positions = m["positions"].ctypes.data_as(abi.f32p)
        mesh.indices = m["faces"].ctypes.data_as(abi.u32p)
        calls = [
            ("index, host", abi.ERR_INVALID, lambda: pt.replace_shape(S, m["positions"], bad, m["normals"])),
            ("index, device", abi.ERR_INVALID,
             lambda: pt.replace_shape_device(S, dev(m["positions"]), dev(bad, np.int32), dev(m["normals"]))),
            ("sphere", abi.ERR_INVALID, lambda: pt.replace_shape(SPHERE, m["positions"], m["faces"])),
            ("out of range", abi.ERR_INVALID, lambda: pt.replace_shape(99, m["positions"], m["faces"])),
            ("no faces", abi.ERR_INVALID,
             lambda: pt.replace_shape(S, m["positions"], np.zeros((0, 3), np.uint32))),
            ("flags", abi.ERR_INVALID,
             lambda: abi.check(pt._lib.pupil_pt_replace_shape_mesh(pt._pt, S, C.byref(mesh), 4, None))),
            ("null mesh", abi.ERR_INVALID,
             lambda: abi.check(pt._lib.pupil_pt_replace_shape_mesh(pt._pt, S, None, 0, None))),
            ("emissive", abi.ERR_UNSUPPORTED, lambda: pt.replace_shape(LAMP, m["positions"], m["faces"])),
        ]
        for what, code, call in calls:
            with pytest.raises(abi.PupilError) as e:
                call()
            assert e.value.code == code, what
            torch.cuda.synchronize()
            assert (pt.stats()["accel_refits"], pt.stats()["bvh_prims"], pt.replace_info()["replacements"]) == state, what
            _same_tables(pt.prim_tables(), tables, what)
            _same(_outputs(pt), before, (accel, what))
    finally:
        pt.close_engine()


# ------------------------------------------------------------------ 7. counters
@pytest.mark.gpu
@pytest.mark.parametrize("accel", ACCELS)
def test_counters(accel, monkeypatch):
    """Nothing hidden here, so that bvh_nodes is comparable: a world-mode TLAS built while an
    instance is hidden leaves its entries out, one built before it was hidden (the fresh engine's:
    create shows everything) keeps them, and the node counts then differ with equal hits."""
    _accel(monkeypatch, accel)
    w = cases.world("cube", hidden=False)
    pt = _pass(w)
    try:
        st0, info0 = pt.stats(), pt.replace_info()
        _replace(pt, w, "icosphere")
        st, info = pt.stats(), pt.replace_info()
        _, fresh, _ = _fresh(w)
        assert st["bvh_prims"] == fresh["bvh_prims"] == st0["bvh_prims"] - 2 * 12 + 2 * 320
        assert st["bvh_nodes"] == fresh["bvh_nodes"] and st["bvh_depth"] == fresh["bvh_depth"]
        assert st["accel_refits"] == st0["accel_refits"] + 1
        assert info["replacements"] == info0["replacements"] + 1 == 1
        assert st["build_ms"] == info["last_ms"] > 0.0
    finally:
        pt.close_engine()


# ------------------------------------------------------------------ CPU: the world and the ABI
def test_world_set_mesh_describes_the_new_mesh():
    w = cases.world("cube", hidden=False)
    d0 = w.desc()
    kept = [(d0.instances[i].material, list(d0.instances[i].to_world), d0.instances[i].shape,
             d0.instances[i].emitter_offset) for i in range(d0.num_instances)]
    assert (d0.shapes[S].num_vertices, d0.shapes[S].num_faces) == (24, 12)
    for name in ("icosphere", "tetrahedron", "grid"):
        m = cases.set_mesh(w, name)
        d = w.desc()
        sh = d.shapes[S]
        nv, nf = len(m["positions"]), len(m["faces"])
        assert (sh.kind, sh.num_vertices, sh.num_faces) == (abi.SHAPE_MESH, nv, nf)
        assert np.array_equal(np.ctypeslib.as_array(sh.positions, (nv, 3)), m["positions"])
        assert np.array_equal(np.ctypeslib.as_array(sh.indices, (nf, 3)), m["faces"])
        for key, width, ptr in (("normals", 3, sh.normals), ("texcoords", 2, sh.texcoords)):
            assert bool(ptr) == (m[key] is not None), (name, key)
            if m[key] is not None:
                assert np.array_equal(np.ctypeslib.as_array(ptr, (nv, width)), m[key])
        assert d.num_shapes == d0.num_shapes and d.num_instances == d0.num_instances
        assert kept == [(d.instances[i].material, list(d.instances[i].to_world), d.instances[i].shape,
                         d.instances[i].emitter_offset) for i in range(d.num_instances)]
        assert d.shapes[cases.OTHER].num_faces == d0.shapes[cases.OTHER].num_faces


def test_world_set_mesh_refusals():
    w = cases.world("cube")
    m = cases.tetrahedron()
    d0 = w.desc()
    shape0 = (d0.shapes[S].num_vertices, d0.shapes[LAMP].num_faces)
    for shape, code in ((SPHERE, abi.ERR_INVALID), (LAMP, abi.ERR_UNSUPPORTED), (99, abi.ERR_INVALID)):
        with pytest.raises(abi.PupilError) as e:
            w.set_mesh(shape, m["positions"], m["faces"])
        assert e.value.code == code, shape
    bad = m["faces"].copy()
    bad[-1, 2] = 4
    with pytest.raises(abi.PupilError) as e:
        w.set_mesh(S, m["positions"], bad)
    assert e.value.code == abi.ERR_INVALID
    d = w.desc()
    assert (d.shapes[S].num_vertices, d.shapes[LAMP].num_faces) == shape0


def test_abi_exposes_the_entry_points():
    lib = abi.load_library()
    for name in ("pupil_pt_replace_shape_mesh", "pupil_pt_replace_info", "pupil_world_set_mesh"):
        assert name in abi.SIGNATURES and hasattr(lib, name), name
    n, ms = C.c_uint64(7), C.c_double(1.0)
    assert lib.pupil_pt_replace_info(None, C.byref(n), C.byref(ms)) == abi.ERR_INVALID
    assert lib.pupil_pt_replace_shape_mesh(None, 0, None, 0, None) == abi.ERR_INVALID


# ------------------------------------------------------------------ 8. repeated replacements
@pytest.mark.gpu
def test_repeated_replacement_holds_no_memory(tmp_path):
    """20 alternating 12- and 48-triangle replacements of the Cornell box's short box, a vertex
    snapshot taken before every second one: the free device memory stays within one granule (upper
    bound: what the engine's creation cost) of its value after the second replacement, and the
    image after the last equals a fresh engine's bit for bit"""
    import torch

    import owner_cases

    from pupiloptixlab_amd.pt_pass import PTPass

    w, box, _, _ = owner_cases.cornell(tmp_path)
    coarse, fine = owner_cases.box_meshes(w, box)
    free = lambda: torch.cuda.mem_get_info(0)[0]  # noqa: E731

    def image(p):
        p.mark_dirty()
        p.render(SPP)
        torch.cuda.synchronize()
        return {k: _bits(p.buffers.get(k)) for k in AOVS}

    pt = PTPass(device=0)
    f_before = free()
    pt.set_scene(w)
    granule = abs(f_before - free())
    try:
        image(pt)  # the ring and every lazily allocated buffer exist from here on
        f2 = None
        for k in range(20):
            if k % 2 == 1:
                abi.check(pt._lib.pupil_pt_snapshot_shape_vertices(pt._pt, box))
            owner_cases.replace(pt, w, box, fine if k % 2 == 0 else coarse)
            if k == 1:
                f2 = free()
        f20 = free()
        print(f"creation cost {granule} B; free after the second replacement {f2}, after the 20th {f20}")
        assert granule > 0 and abs(f20 - f2) <= granule
        assert pt.replace_info()["replacements"] == 20 and w.desc().shapes[box].num_faces == 12
        got = image(pt)
    finally:
        pt.close_engine()
    fresh = PTPass(device=0)
    fresh.set_scene(w)
    try:
        _same(got, image(fresh), "after 20 replacements")
    finally:
        fresh.close_engine()
