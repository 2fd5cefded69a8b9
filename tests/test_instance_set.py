"""The instance table replaced in place (pupil_pt_set_instances): instances added, removed and
rebound.  The engine must equal, bit for bit, an engine freshly created on the edited world with
the same masks -- render AOVs, the camera G-buffer, radiance along fixed rays, flow, the primitive
tables, the structure's counters and (flattened) the exported BVH4 -- on the flattened BVH and both
two-level modes.

Scene: instance_set_cases.BASE (109 primitives; 48 x 48, 2 spp, depth 4).  Hit results do not
depend on the tree's topology and every builder is deterministic, so equality is exact: outputs
are compared as bit patterns, no tolerance."""
import numpy as np
import pytest

from pupiloptixlab_amd import abi

import instance_set_cases as cases
from instance_set_cases import A, B, BASE, BLUE, C, LAMP_INSTANCE

ACCELS = ["flat", "two_level", "two_level_object"]
SPP = 2
AOVS = ("pt accum buffer", "albedo", "normal")


def _accel(monkeypatch, accel):
    """flat | two_level (PUPIL_TL_MODE=world) | two_level_object"""
    monkeypatch.setenv("PUPIL_ACCEL", "flat" if accel == "flat" else "two_level")
    if accel != "flat":
        monkeypatch.setenv("PUPIL_TL_MODE", "object" if accel == "two_level_object" else "world")


def _pass(world):
    from pupiloptixlab_amd.pt_pass import PTPass

    pt = PTPass(device=0)
    pt.set_scene(world)  # applies the world's masks after create
    return pt


def _bits(t):
    a = t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)
    return np.ascontiguousarray(a).view(np.uint8).copy()


def _by_content(pt, ids):
    """Material ids name the slots of the engine's table.  A World describes one material per
    instance, so a fresh engine on the edited world numbers the same materials differently from the
    engine that kept its table: the ids are compared by the content of the slot they name."""
    import hashlib

    ids = ids.cpu().numpy().astype(np.int64) & 0xFFFFFFFF
    digest = np.array([int.from_bytes(hashlib.sha1(k).digest()[:4], "little") for k in pt._mat_keys], np.int64)
    known = ids < len(digest)
    return np.where(known, digest[np.minimum(ids, len(digest) - 1)], ids)


def _outputs(pt, flow=True):
    """everything the issue compares, as bytes"""
    import torch

    pt.mark_dirty()
    pt.render(SPP)
    torch.cuda.synchronize()
    out = {k: _bits(pt.buffers.get(k)) for k in AOVS}
    for k, v in pt.primary_hits().items():
        out["hits." + k] = _bits(_by_content(pt, v) if k == "material" else v)
    rays = torch.from_numpy(cases.fixed_rays()).to(pt.device)
    for k, v in pt.radiance(rays, spp=SPP, seed=3, want=("radiance", "albedo", "normal")).items():
        out["radiance." + k] = _bits(v)
    if flow:
        out["flow"] = _bits(pt.motion_vectors(prev_camera=pt._cam))
    torch.cuda.synchronize()
    tab = pt.prim_tables()
    out["tables.counts"] = _bits(np.array([tab["num_prims"], tab["guide_shift"]], np.uint32))
    for k in ("prim_inst", "inst_first", "inst_guide"):
        out["tables." + k] = _bits(tab[k])
    st = pt.stats()
    out["stats"] = _bits(np.array([st["bvh_prims"], st["bvh_nodes"], st["hidden_instances"]], np.uint64))
    bvh = pt.export_bvh4()  # None in the two-level modes
    if bvh is not None:
        out["bvh.nodes"], out["bvh.records"] = _bits(bvh[0]), _bits(bvh[1])
        out["bvh.root"] = _bits(np.array([bvh[2]], np.int64))
    return out


def _same(got, ref, what, structure=True):
    """structure=False: after a refit, which keeps a topology a fresh build does not choose, the
    node count and the exported tree are left out; what the rays return is compared all the same"""
    assert got.keys() == ref.keys(), what
    for k in got:
        if not structure and (k == "stats" or k.startswith("bvh.")):
            continue
        assert got[k].shape == ref[k].shape and np.array_equal(got[k], ref[k]), (what, k)


def _fresh(specs, prepare=None, flow=True):
    pt = _pass(cases.world(specs))
    try:
        if prepare:
            prepare(pt)
        return _outputs(pt, flow)
    finally:
        pt.close_engine()


def _set(pt, specs, device=False):
    """the table of `specs` into the engine; device: transforms produced on a side stream"""
    w = cases.world(specs)
    if not device:
        pt.set_instances(w)
        return w
    import torch

    side = torch.cuda.Stream(pt.device)
    with torch.cuda.stream(side):
        t = torch.from_numpy(cases.to_world(w)).to(pt.device) + 0
        pt.set_instances_device(w, t.reshape(-1, 3, 4), stream=side)
    side.synchronize()
    return w


def _no_blas_build(pt, accel):
    info = pt.set_instances_info()
    if accel == "two_level":
        assert info["last_blas_builds"] == 0 and info["last_whole_rebuild"] == 0, info


# ------------------------------------------------------------------ 1. add, then remove again
@pytest.mark.gpu
@pytest.mark.parametrize("accel", ACCELS)
def test_add_and_remove(accel, monkeypatch):
    _accel(monkeypatch, accel)
    pt = _pass(cases.world(BASE))
    try:
        before = _outputs(pt)
        added = BASE + (cases.EXTRA_A,)
        _set(pt, added)
        _no_blas_build(pt, accel)
        got = _outputs(pt)
        assert not np.array_equal(got["pt accum buffer"], before["pt accum buffer"])
        _same(got, _fresh(added), (accel, "added"))
        _set(pt, BASE)
        _no_blas_build(pt, accel)
        _same(_outputs(pt), before, (accel, "removed again"))
        assert pt.set_instances_info()["calls"] == 2
    finally:
        pt.close_engine()


# ------------------------------------------------------------------ 2. the lamp's index shifts
@pytest.mark.gpu
@pytest.mark.parametrize("device_emitters", [False, True])
@pytest.mark.parametrize("accel", ACCELS)
def test_remove_before_the_lamp(accel, device_emitters, monkeypatch):
    _accel(monkeypatch, accel)
    pt = _pass(cases.world(BASE))
    try:
        if device_emitters:
            pt.device_emitters = True
        fewer = BASE[:1] + BASE[2:]  # instance 1 goes: the hidden instance, the sphere and the lamp shift down
        assert fewer[LAMP_INSTANCE - 1]["radiance"] is not None
        _set(pt, fewer)
        _no_blas_build(pt, accel)
        assert pt.device_emitters == device_emitters
        tables = []

        def table(f):
            tables.append(f.emitter_table())

        _same(_outputs(pt), _fresh(fewer, prepare=table), (accel, "fewer"))
        if device_emitters:
            got = pt.emitter_table()
            for k, v in tables[0].items():
                assert np.array_equal(_bits(np.asarray(got[k])), _bits(np.asarray(v))), (accel, k)
            # the lamp under its new index, moved on the device: the table follows
            import torch

            from pupiloptixlab_amd import world as W

            w = cases.world(fewer)
            m = W.transform(scale=(1.0, 1.0, 1.0), rotate=((1, 0, 0), 90), translate=(0.3, 3.0, 0.1))
            w.set_instance_transform(LAMP_INSTANCE - 1, m)
            t = torch.from_numpy(cases.to_world(w)[LAMP_INSTANCE - 1:LAMP_INSTANCE]).to(pt.device)
            pt.update_instances_device(t, torch.tensor([LAMP_INSTANCE - 1], dtype=torch.int32, device=pt.device))
            moved = list(fewer)
            moved[LAMP_INSTANCE - 1] = dict(fewer[LAMP_INSTANCE - 1], xf=dict(scale=(1.0, 1.0, 1.0), rotate=((1, 0, 0), 90),
                                                                            translate=(0.3, 3.0, 0.1)))
            _same(_outputs(pt, flow=False), _fresh(moved, flow=False), (accel, "lamp moved"), structure=False)
    finally:
        pt.close_engine()


# ------------------------------------------------------------------ 3. another shape, another material
@pytest.mark.gpu
@pytest.mark.parametrize("accel", ACCELS)
def test_rebind(accel, monkeypatch):
    _accel(monkeypatch, accel)
    pt = _pass(cases.world(BASE))
    try:
        before = _outputs(pt)
        rebound = list(BASE)
        rebound[1] = dict(BASE[1], shape=B, material=BLUE)  # a diffuse cube becomes a rough-plastic uv sphere
        _set(pt, rebound)
        _no_blas_build(pt, accel)
        got = _outputs(pt)
        assert not np.array_equal(got["pt accum buffer"], before["pt accum buffer"])
        _same(got, _fresh(rebound), (accel, "rebound"))
        # every instance on one material: the shading schedule's bins change with the table
        grey = [dict(s, material=cases.GREY) for s in BASE]
        _set(pt, grey)
        _same(_outputs(pt), _fresh(grey), (accel, "one bin"))
    finally:
        pt.close_engine()


@pytest.mark.gpu
def test_materials_are_bound_by_what_the_engine_holds_now(monkeypatch):
    """after update_materials the pass binds by the slots' new contents"""
    from pupiloptixlab_amd import world as W

    _accel(monkeypatch, "flat")
    w = cases.world(BASE)
    pt = _pass(w)
    try:
        assert len(set(pt._mat_keys)) == 4 and len(pt._mat_keys) == len(BASE)
        green = W.twosided(W.diffuse((0.1, 0.7, 0.2)))
        w.set_material(1, green)  # instance 1's material: red becomes green
        pt.update_material(w, 1)
        assert len(set(pt._mat_keys)) == 4 and pt._mat_slots[pt._mat_keys[1]] == 1
        pt.set_instances(w)  # the world's instance 1 names the green material: slot 1 holds it now
        n, arr, _ = pt._bindings(w)
        assert arr[1].material == 1
        with pytest.raises(ValueError):  # red is gone from the engine
            pt.set_instances(cases.world(BASE))
    finally:
        pt.close_engine()


# ------------------------------------------------------------------ 4. a shape's first and last instance
@pytest.mark.gpu
@pytest.mark.parametrize("accel", ACCELS)
def test_first_and_last_instance_of_a_shape(accel, monkeypatch):
    _accel(monkeypatch, accel)
    pt = _pass(cases.world(BASE))
    try:
        first = BASE + (cases.EXTRA_C,)  # shape C had no instance
        _set(pt, first)
        info = pt.set_instances_info()
        if accel != "flat":
            assert info["last_whole_rebuild"] == 1 and info["last_blas_builds"] >= 1, info
        _same(_outputs(pt), _fresh(first), (accel, "first instance"))
        last = tuple(s for s in first if s["shape"] != B)  # B loses its only instance
        _set(pt, last)
        info = pt.set_instances_info()
        if accel != "flat":
            assert info["last_whole_rebuild"] == 1 and info["last_blas_builds"] >= 1, info
        _same(_outputs(pt), _fresh(last), (accel, "last instance"))
        # B changes while no instance shows it -- new topology, then new vertices with a larger
        # extent -- and gets an instance back each time: its BLAS is built from the arrays and the
        # extent the shape has then, not from what its earlier use left behind
        import torch

        m = cases.meshes.icosphere()
        big = torch.from_numpy((m["positions"] * np.float32([3.0, 0.5, 2.0])).astype(np.float32)).to(pt.device)

        def replace(f):
            f.replace_shape(B, m["positions"], m["faces"], m["normals"], m["texcoords"])

        def replace_and_deform(f):
            replace(f)
            f.update_shape_device(B, big)

        again = last + (BASE[5],)
        replace(pt)
        _set(pt, again)
        info = pt.set_instances_info()
        if accel != "flat":
            assert info["last_whole_rebuild"] == 1, info
        _same(_outputs(pt), _fresh(again, prepare=replace), (accel, "replaced while unused"))
        _set(pt, last)
        pt.update_shape_device(B, big)
        _set(pt, again)
        _same(_outputs(pt), _fresh(again, prepare=replace_and_deform), (accel, "deformed while unused"), structure=False)
    finally:
        pt.close_engine()


# ------------------------------------------------------------------ 5. transforms from device memory
@pytest.mark.gpu
@pytest.mark.parametrize("accel", ACCELS)
def test_device_path(accel, monkeypatch):
    _accel(monkeypatch, accel)
    specs = BASE + (cases.HIDDEN_SPHERE, cases.EXTRA_A)
    outs = []
    for device in (False, True):
        pt = _pass(cases.world(BASE))
        try:
            _set(pt, specs, device=device)
            _no_blas_build(pt, accel)
            outs.append(_outputs(pt))
            tw, to = pt.instance_transforms()
            d = cases.world(specs).desc()
            for i in range(d.num_instances):  # the mirror: the world's own inverse, the hidden sphere's included
                assert np.array_equal(_bits(tw[i]), _bits(np.array(list(d.instances[i].to_world), np.float32))), i
                assert np.array_equal(_bits(to[i]), _bits(np.array(list(d.instances[i].to_object), np.float32))), i
        finally:
            pt.close_engine()
    _same(outs[0], outs[1], (accel, "host = device"))
    _same(outs[1], _fresh(specs), (accel, "device = fresh"))
    assert outs[1]["stats"].view(np.uint64)[2] == 2  # the hidden cube and the hidden sphere


# ------------------------------------------------------------------ 6. refusals change nothing
@pytest.mark.gpu
@pytest.mark.parametrize("accel", ACCELS)
def test_refusals(accel, monkeypatch):
    import ctypes as Ct

    _accel(monkeypatch, accel)
    w = cases.world(BASE)
    pt = _pass(w)
    try:
        before = _outputs(pt)
        n, arr, vis = pt._bindings(w)
        lib, vp = pt._lib, vis.ctypes.data_as(abi.u32p)
        arr[2].shape = 99
        assert lib.pupil_pt_set_instances(pt._pt, n, arr, vp, None, 0, None) == abi.ERR_INVALID
        arr[2].shape = A
        assert lib.pupil_pt_set_instances(pt._pt, n, arr, vp, None, abi.INSTANCES_DEVICE, None) == abi.ERR_INVALID
        assert lib.pupil_pt_set_instances(pt._pt, n, arr, vp, None, 2, None) == abi.ERR_INVALID
        assert lib.pupil_pt_set_instances(pt._pt, 0, arr, vp, None, 0, None) == abi.ERR_INVALID
        assert lib.pupil_pt_set_instances(pt._pt, n, None, vp, None, 0, None) == abi.ERR_INVALID
        with pytest.raises(abi.PupilError) as e:  # a new emissive instance
            pt.set_instances(cases.world(BASE + (cases.SECOND_LAMP,)))
        assert e.value.code == abi.ERR_UNSUPPORTED
        with pytest.raises(abi.PupilError) as e:  # the lamp removed
            pt.set_instances(cases.world(BASE[:LAMP_INSTANCE] + BASE[LAMP_INSTANCE + 1:]))
        assert e.value.code == abi.ERR_UNSUPPORTED
        moved = list(BASE)
        moved[LAMP_INSTANCE] = dict(BASE[LAMP_INSTANCE], xf=dict(scale=(1.2, 1.2, 1.0), rotate=((1, 0, 0), 90),
                                                               translate=(0.5, 3.2, 0.0)))
        for device in (False, True):  # a moved emissive instance, device emitters off
            with pytest.raises(abi.PupilError) as e:
                _set(pt, moved, device=device)
            assert e.value.code == abi.ERR_UNSUPPORTED
        assert pt.set_instances_info()["calls"] == 0
        _same(_outputs(pt), before, (accel, "after the refusals"))
    finally:
        pt.close_engine()


# ------------------------------------------------------------------ 7. the engine goes on working
@pytest.mark.gpu
@pytest.mark.parametrize("accel", ACCELS)
def test_interplay(accel, monkeypatch):
    import torch

    from pupiloptixlab_amd import world as W

    _accel(monkeypatch, accel)
    specs = list(BASE + (cases.EXTRA_A,))
    pt = _pass(cases.world(BASE))
    try:
        pt.render(1)
        w = _set(pt, specs)
        # the new last id moves, from device memory
        last = len(specs) - 1
        xf = dict(scale=(0.6, 0.6, 0.6), rotate=((0, 0, 1), 50), translate=(-0.2, 0.8, -0.5))
        w.set_instance_transform(last, W.transform(**xf))
        specs[last] = dict(specs[last], xf=xf)
        t = torch.from_numpy(cases.to_world(w)[last:]).to(pt.device)
        pt.update_instances_device(t, torch.tensor([last], dtype=torch.int32, device=pt.device))
        _same(_outputs(pt, flow=False), _fresh(specs, flow=False), (accel, "moved on the device"), structure=False)
        # a shape deforms
        p = (cases.meshes.cube()["positions"] * np.float32([1.0, 1.3, 0.8])).astype(np.float32)
        w.set_mesh_vertices(A, p)
        pt.update_shape(w, A)

        def deform(f):
            f._world.set_mesh_vertices(A, p)
            f.update_shape(f._world, A)

        _same(_outputs(pt, flow=False), _fresh(specs, prepare=deform, flow=False), (accel, "deformed"), structure=False)
        # a mesh is replaced
        m = cases.meshes.icosphere()
        pt.replace_shape(A, m["positions"], m["faces"], m["normals"], m["texcoords"])

        def replace(f):
            f.replace_shape(A, m["positions"], m["faces"], m["normals"], m["texcoords"])

        _same(_outputs(pt, flow=False), _fresh(specs, prepare=replace, flow=False), (accel, "replaced"))
        # and another table after all that, then pipelined frames
        specs2 = specs[:2] + specs[3:]
        _set(pt, specs2)

        def frames(f):
            f.mark_dirty()
            for k in range(3):
                f.render(1, continues=k > 0)
            torch.cuda.synchronize()
            return _bits(f.buffers.get("pt accum buffer"))

        got = frames(pt)
        f = _pass(cases.world(specs2))
        try:
            replace(f)
            assert np.array_equal(got, frames(f)), (accel, "pipelined")
        finally:
            f.close_engine()
    finally:
        pt.close_engine()
