"""Engine-owned area-emitter table (pupil_pt_enable_device_emitters): after vertex and transform
updates of emissive shapes and instances the engine rebuilds the table on the device
(pt_emitters.hip), and the result must equal, bit for bit, the table of a freshly created engine on
a world built from scratch -- which the host computed.  Every comparison is bit-exact.

World A (test_device_emitters_host.world_a): 195 emitters, emitter ranges starting at 0, 96, 97,
193.  Film 64 x 48, 4 spp, depth 4."""
import ctypes as C
import functools

import numpy as np
import pytest

import oracle
from pupiloptixlab_amd import abi

from test_device_emitters_host import (XF_MOVED, big_world, bulge, grid_mesh, no_normals_world, one_emitter_world,
                                       squeeze, vertex_normals, world_a, ONE_TRI)
from test_visibility import KEYS, _assert_render_equals, _render

pytestmark = pytest.mark.gpu

ACCELS = ["flat", "two_level", "two_level_object"]
SPP = 4
TABLE_KEYS = ("select_probability", "area", "cdf", "type", "pos", "nrm")


def _accel(monkeypatch, accel):
    monkeypatch.setenv("PUPIL_ACCEL", "flat" if accel == "flat" else "two_level")
    if accel != "flat":
        monkeypatch.setenv("PUPIL_TL_MODE", "object" if accel == "two_level_object" else "world")


def _pass(world_or_desc):
    from pupiloptixlab_amd.pt_pass import PTPass

    pt = PTPass(device=0)
    pt.set_scene(world_or_desc)
    return pt


def _dev(pt, a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(pt.device)


def _same_table(got, ref, what):
    for k in TABLE_KEYS:
        assert np.array_equal(got[k].view(np.uint32), ref[k].view(np.uint32)), (what, k)
    assert got["guide_bits"] == ref["guide_bits"], what
    assert (got["guide"] is None) == (ref["guide"] is None), what
    if ref["guide"] is not None:
        assert np.array_equal(got["guide"], ref["guide"]), (what, "guide")


def _same(a, b, what):
    for k in KEYS:
        assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), (what, k)


def _picks(pt):
    p = np.random.default_rng(17).random(4096, dtype=np.float32)
    out = np.zeros(4096, np.int32)
    abi.check(pt._lib.pupil_debug_select_emitter(pt._pt, 4096, p.ctypes.data_as(abi.f32p),
                                                 out.ctypes.data_as(C.POINTER(C.c_int32))))
    return out


# ------------------------------------------------------------------ states of World A's grid
@functools.lru_cache(maxsize=None)
def state(name):
    """(positions, normals) of the grid: 'base'; 'bulge' with recomputed normals; 'squeeze' of the
    bulged grid with the bulge's normals kept"""
    p0, n0, _, idx = grid_mesh()
    if name == "base":
        return p0, n0
    pb = bulge(p0)
    nb = vertex_normals(pb, idx)
    return (pb, nb) if name == "bulge" else (squeeze(pb), nb)


@functools.lru_cache(maxsize=None)
def fresh(name, moved=False):
    """table, render and emitter picks of a freshly created engine (mode off: the host's table) on
    World A built from scratch in that state; computed once"""
    pt = _pass(world_a(*state(name), xf=XF_MOVED if moved else None))
    try:
        return pt.emitter_table(), _render(pt, SPP), _picks(pt)
    finally:
        pt.close_engine()


@functools.lru_cache(maxsize=None)
def oracle_ref(name, moved=False):
    return oracle.OracleScene(world_a(*state(name), xf=XF_MOVED if moved else None).desc()).render(spp=SPP)


def _refreshes(pt):
    return pt.device_emitters_info()["refreshes"]


# ------------------------------------------------------------------ 1. enable equals host
def test_enable_reproduces_the_host_table():
    pt = _pass(world_a())
    try:
        before = pt.emitter_table()
        assert len(before["area"]) == 195 and before["guide"] is not None and len(before["guide"]) == 257
        assert pt.device_emitters_info() == {"enabled": False, "refreshes": 0, "last_ms": 0.0}
        pt.device_emitters = True
        info = pt.device_emitters_info()
        assert info["enabled"] and info["refreshes"] == 1 and info["last_ms"] > 0.0
        _same_table(pt.emitter_table(), before, "enable")
        _assert_render_equals(_render(pt, SPP), oracle_ref("base"), "enabled, nothing moved")
    finally:
        pt.close_engine()


# ------------------------------------------------------------------ 2. deform from device tensors
@pytest.mark.parametrize("accel", ACCELS)
def test_deform_from_device_tensors(accel, monkeypatch):
    _accel(monkeypatch, accel)
    pt = _pass(world_a())
    try:
        prev = _render(pt, SPP)
        pt.device_emitters = True
        n = _refreshes(pt)
        pb, nb = state("bulge")
        pt.update_shape_device(0, _dev(pt, pb), _dev(pt, nb))
        assert _refreshes(pt) == n + 1
        table, ref_img, _ = fresh("bulge")
        _same_table(pt.emitter_table(), table, (accel, "bulge"))
        got = _render(pt, SPP)
        for k in ("pt accum buffer", "normal"):
            assert not np.array_equal(got[k], prev[k]), k
        _same(got, ref_img, (accel, "fresh engine"))
        _assert_render_equals(got, oracle_ref("bulge"), (accel, "oracle"))
        # the normals kept
        ps, _ = state("squeeze")
        pt.update_shape_device(0, _dev(pt, ps))
        table_s, ref_s, _ = fresh("squeeze")
        _same_table(pt.emitter_table(), table_s, (accel, "normals kept"))
        _same(_render(pt, SPP), ref_s, (accel, "normals kept"))
        # a rebuild of the structure from device vertices
        pt.update_shape_device(0, _dev(pt, pb), _dev(pt, nb), rebuild=True)
        _same_table(pt.emitter_table(), table, (accel, "rebuild"))
        _same(_render(pt, SPP), ref_img, (accel, "rebuild"))
        # keep_previous: flow does not involve emitters, it must simply still run
        pt.update_shape_device(0, _dev(pt, ps), keep_previous=True)
        assert _refreshes(pt) == n + 4
        _same(_render(pt, SPP), ref_s, (accel, "keep_previous"))
        mv = pt.motion_vectors().cpu().numpy()
        assert mv.shape == (64 * 48, 2) and np.isfinite(mv).any()
        _same_table(pt.emitter_table(), table_s, (accel, "keep_previous"))
    finally:
        pt.close_engine()


# ------------------------------------------------------------------ 3. host vertices, mode on
def test_host_vertices_with_the_mode_on_upload_no_table():
    w = world_a()
    pt = _pass(w)
    try:
        pt.device_emitters = True
        calls = []
        real = pt._lib.pupil_pt_update_emitters
        n = _refreshes(pt)
        w.set_mesh_vertices(0, *state("bulge"))
        try:
            pt._lib.pupil_pt_update_emitters = lambda *a: calls.append(a) or real(*a)
            pt.update_shape(w, 0)
        finally:
            pt._lib.pupil_pt_update_emitters = real
        assert not calls and _refreshes(pt) == n + 1
        table, ref_img, _ = fresh("bulge")
        _same_table(pt.emitter_table(), table, "host vertices")
        _same(_render(pt, SPP), ref_img, "host vertices")
    finally:
        pt.close_engine()


# ------------------------------------------------------------------ 4. a rigid move; hiding
def test_rigid_move_rebuilds_and_hiding_does_not():
    from pupiloptixlab_amd import world as W

    w = world_a()
    pt = _pass(w)
    try:
        pt.device_emitters = True
        n = _refreshes(pt)
        for i, t in XF_MOVED.items():
            w.set_instance_transform(i, W.transform(**t))
        pt.update_instances(w, list(XF_MOVED))
        assert _refreshes(pt) == n + 1
        table, ref_img, _ = fresh("base", moved=True)
        _same_table(pt.emitter_table(), table, "moved")
        assert not np.array_equal(table["pos"], fresh("base")[0]["pos"])
        got = _render(pt, SPP)
        _same(got, ref_img, "moved, fresh engine")
        _assert_render_equals(got, oracle_ref("base", moved=True), "moved, oracle")
        # a mask-only call hides emissive instance 2: the table stays, nothing is rebuilt
        ids, vis = np.array([2], np.uint32), np.array([0], np.uint32)
        abi.check(pt._lib.pupil_pt_update_instances_masked(pt._pt, 1, ids.ctypes.data_as(abi.u32p), None, None,
                                                           vis.ctypes.data_as(abi.u32p)))
        assert pt.stats()["hidden_instances"] == 1 and _refreshes(pt) == n + 1
        _same_table(pt.emitter_table(), table, "hidden")
        # moving a non-emissive instance (the floor) rebuilds nothing either
        w.set_instance_transform(4, W.transform(scale=(6, 6, 1), rotate=((1, 0, 0), -90), translate=(0.0, -2.5, 0.0)))
        pt.update_instances(w, [4])
        assert _refreshes(pt) == n + 1
    finally:
        pt.close_engine()


# ------------------------------------------------------------------ 5. the emitter pick
def test_emitter_pick_after_a_deform_equals_a_fresh_engine():
    pt = _pass(world_a())
    try:
        before = _picks(pt)
        pt.device_emitters = True
        pt.update_shape_device(0, *(_dev(pt, a) for a in state("bulge")))
        ref = fresh("bulge")[2]
        got = _picks(pt)
        assert np.array_equal(got, ref)
        assert len(np.unique(ref)) > 50 and (ref == -1).any() and not np.array_equal(ref, before)
    finally:
        pt.close_engine()


# ------------------------------------------------------------------ 6. edges
def _edge(build, deform, normals=True, guide=True):
    """enable, then the deformed vertices from device tensors: table and render against a fresh
    engine on the deformed mesh"""
    pos, idx = deform
    nrm = vertex_normals(pos, idx) if normals else None
    ref_pt = _pass(build(pos, nrm) if normals else build(pos))
    try:
        ref, ref_img = ref_pt.emitter_table(), _render(ref_pt, SPP)
    finally:
        ref_pt.close_engine()
    assert (ref["guide"] is not None) == guide
    pt = _pass(build())
    try:
        before = pt.emitter_table()
        pt.device_emitters = True
        _same_table(pt.emitter_table(), before, "enable")
        pt.update_shape_device(0, _dev(pt, pos), _dev(pt, nrm) if normals else None)
        got = pt.emitter_table()
        assert not np.array_equal(got["pos"], before["pos"])
        _same_table(got, ref, "deformed")
        _same(_render(pt, SPP), ref_img, "deformed")
        return got
    finally:
        pt.close_engine()


def test_edge_exactly_one_emitter_has_no_guide():
    moved = (ONE_TRI * np.array([1.5, 0.6, 1.0], np.float32) + np.array([0.2, 0.1, -0.3], np.float32)).astype(np.float32)
    got = _edge(lambda pos=None, nrm=None: one_emitter_world(pos), (moved, np.array([[0, 1, 2]], np.uint32)),
                normals=False, guide=False)
    assert len(got["area"]) == 1 and got["select_probability"][0] == 1.0 and got["cdf"][0] == 1.0


def test_edge_4098_emitters_span_many_chain_chunks():
    p0, _, _, idx = grid_mesh(65, 33)
    got = _edge(big_world, (bulge(p0), idx))
    assert len(got["area"]) == 4098 and got["guide_bits"] == 13 and len(got["guide"]) == 8193


def test_edge_mesh_without_normals():
    p0, _, _, idx = grid_mesh()
    got = _edge(no_normals_world, (bulge(p0), idx), normals=False)
    assert len(got["area"]) == 97


def test_edge_binary_select_has_no_guide(monkeypatch):
    monkeypatch.setenv("PUPIL_EMITTER_SELECT", "binary")
    p0, _, _, idx = grid_mesh()
    got = _edge(world_a, (bulge(p0), idx), guide=False)
    assert len(got["area"]) == 195 and got["guide"] is None
    _same_table({**got, "guide": None}, {**fresh("bulge")[0], "guide": None}, "binary == guided, but for the guide")


# ------------------------------------------------------------------ 7. mode off is today's behaviour
def test_mode_off_behaves_as_before():
    w = world_a()
    pt = _pass(w)
    try:
        pb = _dev(pt, state("bulge")[0])

        def refused():
            with pytest.raises(abi.PupilError) as e:
                pt.update_shape_device(0, pb)
            assert e.value.code == abi.ERR_UNSUPPORTED
            assert pt._lib.pupil_pt_refresh_emitters(pt._pt) == abi.ERR_INVALID

        table = pt.emitter_table()
        refused()
        pt.device_emitters = True
        assert pt.device_emitters and pt._lib.pupil_pt_refresh_emitters(pt._pt) == abi.OK
        pt.device_emitters = False
        assert not pt.device_emitters
        refused()
        _same_table(pt.emitter_table(), table, "nothing moved")
        # an emitter upload with another emitter count switches the mode off, and says so
        pt.device_emitters = True
        same = w.desc()
        abi.check(pt._lib.pupil_pt_update_emitters(pt._pt, C.byref(same)))
        assert pt.device_emitters  # the counts still match: the mode stays
        other = world_a(rect_emissive=False).desc()
        assert other.num_area_emitters == 193
        abi.check(pt._lib.pupil_pt_update_emitters(pt._pt, C.byref(other)))
        assert b"switched off" in pt._lib.pupil_last_error()
        assert not pt.device_emitters and len(pt.emitter_table()["area"]) == 193
        refused()
        # set_scene is a new engine: the mode is off
        pt.device_emitters = False
        pt.set_scene(w)
        assert not pt.device_emitters
    finally:
        pt.close_engine()


# ------------------------------------------------------------------ 8. argument checks
def test_enable_refuses_a_scene_that_is_not_the_engines():
    w = world_a()
    pt = _pass(w)
    try:
        desc = w.desc()
        enable = pt._lib.pupil_pt_enable_device_emitters

        def variant(**kw):
            d = abi.SceneDesc()
            C.memmove(C.byref(d), C.byref(desc), C.sizeof(d))
            inst = (abi.Instance * desc.num_instances)()
            C.memmove(inst, desc.instances, C.sizeof(inst))
            for i, off in kw.pop("offsets", {}).items():
                inst[i].emitter_offset = off
            d.instances = C.cast(inst, C.POINTER(abi.Instance))
            for k, v in kw.items():
                setattr(d, k, v)
            d._keep = inst
            return d

        bad = [variant(offsets={2: 98}), variant(offsets={4: 195}), variant(offsets={3: -1}),
               variant(num_area_emitters=194), variant(num_instances=4)]
        for on in (False, True):
            if on:
                pt.device_emitters = True
            info, table = pt.device_emitters_info(), pt.emitter_table()
            for d in bad:
                assert enable(pt._pt, C.byref(d)) == abi.ERR_INVALID
                assert pt._lib.pupil_last_error()
            assert pt.device_emitters_info() == info and info["enabled"] == on
            _same_table(pt.emitter_table(), table, on)
        assert pt._lib.pupil_debug_read_emitters(pt._pt, 195, 1, np.zeros(24, np.float32).ctypes.data_as(abi.f32p)) \
            == abi.ERR_INVALID
        assert pt._lib.pupil_debug_read_emitters(pt._pt, 100, 96, np.zeros(24 * 96, np.float32).ctypes.data_as(abi.f32p)) \
            == abi.ERR_INVALID
        assert enable(pt._pt, C.byref(variant())) == abi.OK  # an unchanged copy is accepted
    finally:
        pt.close_engine()
