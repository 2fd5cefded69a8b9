"""Instances from device memory (pupil_pt_update_instances_device): after a move whose ids and
matrices come from device tensors, the engine must equal, bit for bit, a freshly created engine on
a world built from scratch with the same transforms -- render (all AOVs), trace() hits over a
fixed ray set, the emitter table and the host mirror's matrices.  Every comparison is bit-exact.

The world (test_instances_device_host.world): 24 instances -- 18 of a 512-triangle grid, 2 of a
small grid, 2 spheres, an emissive rectangle, an emissive sphere; film 64 x 48, 4 spp, depth 4."""
import functools

import numpy as np
import pytest

from pupiloptixlab_amd import abi

from test_instances_device_host import (EMISSIVE_MESH, EMISSIVE_SPHERE, GRIDS, N_INST, desc_matrices, mixed, rows12,
                                        transforms, world)
from test_visibility import KEYS, _random_rays, _render

pytestmark = pytest.mark.gpu

ACCELS = ["flat", "two_level", "two_level_object"]
SPP = 4
ALL = tuple(range(N_INST))
SUBSET = (13, 2, 19, 20, 7)  # unsorted: grids, a small grid, a sphere
HIDDEN = (5, 20)             # a grid instance and a sphere
TABLE_KEYS = ("select_probability", "area", "cdf", "type", "pos", "nrm")


def _accel(monkeypatch, accel):
    monkeypatch.setenv("PUPIL_ACCEL", "flat" if accel == "flat" else "two_level")
    monkeypatch.setenv("PUPIL_TL_MODE", "object" if accel == "two_level_object" else "world")
    monkeypatch.delenv("PUPIL_TL_UPDATE", raising=False)
    monkeypatch.delenv("PUPIL_FLAT_UPDATE", raising=False)


def _pass(w):
    from pupiloptixlab_amd.pt_pass import PTPass

    pt = PTPass(device=0)
    pt.set_scene(w)
    return pt


def _dev(pt, a, dtype=np.float32):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a, dtype)).to(pt.device)


@functools.lru_cache(maxsize=None)
def _rays():
    return np.concatenate([_random_rays(2048, (-6.0, -4.0, -9.0), (6.0, 4.0, 3.0), 31),
                           np.tile(np.array([[0.001, 1e16]], np.float32), (2048, 1))], 1).astype(np.float32)


def _state(pt):
    """everything a comparison looks at"""
    r = pt.trace(_dev(pt, _rays()), want=("hit", "instance", "primitive"))
    tw, to = pt.instance_transforms()
    return {"render": _render(pt, SPP), "hit": r["hit"].cpu().numpy(), "instance": r["instance"].cpu().numpy(),
            "primitive": r["primitive"].cpu().numpy(), "table": pt.emitter_table(), "to_world": tw, "to_object": to}


@functools.lru_cache(maxsize=None)
def fresh(moved=(), hidden=()):
    """the state of a freshly created engine on the world built from scratch with the instances in
    `moved` at their moved place (and those in `hidden` hidden); computed once per argument"""
    w = world(mixed(moved))
    for i in hidden:
        w.set_instance_visibility(i, 0)
    pt = _pass(w)
    try:
        s = _state(pt)
        s["desc"] = desc_matrices(w.desc())
        return s
    finally:
        pt.close_engine()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype.itemsize == 4 else a


def _same(got, ref, what, mirror=True):
    for k in KEYS:
        assert np.array_equal(_bits(got["render"][k]), _bits(ref["render"][k])), (what, "render", k)
    for k in ("hit", "instance", "primitive"):
        assert np.array_equal(_bits(got[k]), _bits(ref[k])), (what, k)
    for k in TABLE_KEYS:
        assert np.array_equal(_bits(got["table"][k]), _bits(ref["table"][k])), (what, "table", k)
    if mirror:
        for k in ("to_world", "to_object"):
            assert np.array_equal(_bits(got[k]), _bits(ref[k])), (what, k)


def _move(pt, ids, to_object=False, explicit_ids=True, **kw):
    """the device move of `ids` to their moved place"""
    ids = list(ids)
    tw = rows12(transforms("moved")[ids])
    to = _dev(pt, fresh(ALL)["desc"][1][ids]) if to_object else None
    pt.update_instances_device(_dev(pt, tw), _dev(pt, ids, np.int32) if explicit_ids else None, to, **kw)


# ------------------------------------------------------------------ 1. everything moves
@pytest.mark.parametrize("accel", ACCELS)
def test_all_instances_moved_with_and_without_to_object(accel, monkeypatch):
    _accel(monkeypatch, accel)
    ref = fresh(ALL)
    assert not np.array_equal(ref["render"]["pt accum buffer"], fresh()["render"]["pt accum buffer"])
    for given in (False, True):
        pt = _pass(world())
        try:
            pt.device_emitters = True  # 22 and 23 emit
            _move(pt, ALL, to_object=given, explicit_ids=False)
            tw, to = pt.instance_transforms()
            assert np.array_equal(_bits(tw), _bits(ref["desc"][0])), (accel, given)
            assert np.array_equal(_bits(to), _bits(ref["desc"][1])), (accel, given)
            _same(_state(pt), ref, (accel, "to_object given" if given else "engine inverts"))
            info = pt.instances_device_info()
            assert info["updates"] == 1 and info["instances"] == N_INST and info["skipped"] == 0
            assert info["last_launches"] > 0 and info["last_syncs"] > 0 and info["last_ms"] > 0.0
        finally:
            pt.close_engine()


# ------------------------------------------------------------------ 2. an unsorted subset
@pytest.mark.parametrize("accel", ACCELS)
def test_unsorted_subset_costs_one_refit(accel, monkeypatch):
    _accel(monkeypatch, accel)
    pt = _pass(world())
    try:
        before = pt.instance_transforms()
        refits = pt.stats()["accel_refits"]
        _move(pt, SUBSET)
        assert pt.stats()["accel_refits"] == refits + 1
        after = pt.instance_transforms()
        rest = [i for i in ALL if i not in SUBSET]
        for b, a in zip(before, after):
            assert np.array_equal(_bits(a[rest]), _bits(b[rest]))
            assert not np.array_equal(_bits(a[list(SUBSET)]), _bits(b[list(SUBSET)]))
        _same(_state(pt), fresh(tuple(sorted(SUBSET))), (accel, "subset"))
    finally:
        pt.close_engine()


# ------------------------------------------------------------------ 3. an id out of range
@pytest.mark.parametrize("accel", ACCELS)
def test_id_out_of_range_is_skipped_and_counted(accel, monkeypatch):
    _accel(monkeypatch, accel)
    pt = _pass(world())
    try:
        ids = [4, N_INST, 18, 21]
        tw = np.zeros((4, 12), np.float32)
        tw[[0, 2, 3]] = rows12(transforms("moved")[[4, 18, 21]])
        tw[1] = np.nan  # never read
        pt.update_instances_device(_dev(pt, tw), _dev(pt, ids, np.int32))
        assert b"out of range" in pt._lib.pupil_last_error()
        info = pt.instances_device_info()
        assert info["skipped"] == 1 and info["instances"] == 3 and info["updates"] == 1
        _same(_state(pt), fresh((4, 18, 21)), (accel, "skipped id"))
    finally:
        pt.close_engine()


# ------------------------------------------------------------------ 4. moved while hidden
@pytest.mark.parametrize("accel", ACCELS)
def test_hidden_instances_move_and_stay_hidden(accel, monkeypatch):
    _accel(monkeypatch, accel)
    w = world()
    pt = _pass(w)
    try:
        for i in HIDDEN:
            w.set_instance_visibility(i, 0)
        pt.update_instances(w, HIDDEN)
        _move(pt, HIDDEN)
        got = _state(pt)
        assert not np.isin(got["instance"], HIDDEN).any()
        _same(got, fresh(HIDDEN, HIDDEN), (accel, "hidden"))
        for i in HIDDEN:  # shown by the host path, at the new transform
            w.set_instance_transform(i, transforms("moved")[i])
            w.set_instance_visibility(i, 255)
        pt.update_instances(w, HIDDEN)
        got = _state(pt)
        assert np.isin(got["instance"], HIDDEN).any()
        _same(got, fresh(HIDDEN), (accel, "shown"))
    finally:
        pt.close_engine()


# ------------------------------------------------------------------ 5. emissive instances
@pytest.mark.parametrize("accel", ACCELS)
def test_emissive_instances_need_the_device_emitter_table(accel, monkeypatch):
    _accel(monkeypatch, accel)
    lights = (EMISSIVE_MESH, EMISSIVE_SPHERE)
    pt = _pass(world())
    try:
        before = _state(pt)
        with pytest.raises(abi.PupilError) as e:
            _move(pt, lights)
        assert e.value.code == abi.ERR_UNSUPPORTED
        assert pt.instances_device_info()["updates"] == 0
        _same(_state(pt), before, (accel, "refused"))
        pt.device_emitters = True
        _move(pt, lights)
        ref = fresh(lights)
        assert not np.array_equal(ref["table"]["pos"], before["table"]["pos"])
        _same(_state(pt), ref, (accel, "lights moved"))
    finally:
        pt.close_engine()


# ------------------------------------------------------------------ 6. ordered on the caller's stream
@pytest.mark.parametrize("accel", ACCELS)
def test_matrices_produced_on_a_side_stream(accel, monkeypatch):
    import torch

    _accel(monkeypatch, accel)
    pt = _pass(world())
    try:
        ids = list(GRIDS)
        src = _dev(pt, rows12(transforms("moved")[ids]))
        tw = torch.zeros_like(src)
        busy = torch.ones((2048, 2048), device=pt.device)
        torch.cuda.synchronize()
        side = torch.cuda.Stream(device=pt.device_index)
        with torch.cuda.stream(side):
            for _ in range(8):  # keeps the side stream busy while the call below is issued
                busy = busy @ busy * 0.0 + 1.0
            x = src * busy[0, :12]  # times one: the bits stay
            for _ in range(4):
                x = x * 1.0
            tw.copy_(x)
        pt.update_instances_device(tw, _dev(pt, ids, np.int32), stream=side)
        _same(_state(pt), fresh(tuple(ids)), (accel, "side stream"))
    finally:
        pt.close_engine()


# ------------------------------------------------------------------ 7. a device update, then a TLAS build
def test_stale_braid_entries_are_recomputed_by_a_build(monkeypatch):
    _accel(monkeypatch, "two_level")
    w = world()
    pt = _pass(w)
    try:
        pt.device_emitters = True
        _move(pt, ALL, explicit_ids=False)
        monkeypatch.setenv("PUPIL_TL_UPDATE", "rebuild")
        for i in ALL:
            w.set_instance_transform(i, transforms("moved")[i])
        pt.update_instances(w, [9])
        _same(_state(pt), fresh(ALL), "device update, then a host build")
    finally:
        pt.close_engine()


# ------------------------------------------------------------------ 8. both paths on the same instances
@pytest.mark.parametrize("accel", ACCELS)
def test_device_then_host_and_host_then_device(accel, monkeypatch):
    _accel(monkeypatch, accel)
    ids = sorted(SUBSET)
    w = world()
    pt = _pass(w)
    try:
        _move(pt, ids)  # device, then the host path back to base (where the world still is)
        pt.update_instances(w, ids)
        _same(_state(pt), fresh(), (accel, "device then host"))
        for i in ids:  # host, then the device path on top
            w.set_instance_transform(i, transforms("moved")[i])
        pt.update_instances(w, ids)
        _same(_state(pt), fresh(tuple(ids)), (accel, "host"))
        pt.update_instances_device(_dev(pt, rows12(transforms("base")[ids])), _dev(pt, ids, np.int32))
        _same(_state(pt), fresh(), (accel, "host then device"))
    finally:
        pt.close_engine()


# ------------------------------------------------------------------ 9. flow covers the move
@pytest.mark.parametrize("accel", ACCELS)
def test_motion_vectors_equal_the_host_paths(accel, monkeypatch):
    import torch

    _accel(monkeypatch, accel)
    ids = sorted(SUBSET)
    flows = []
    for device in (True, False):
        w = world()
        pt = _pass(w)
        try:
            pt.render(1)
            if device:
                _move(pt, ids)
            else:
                for i in ids:
                    w.set_instance_transform(i, transforms("moved")[i])
                pt.update_instances(w, ids)
            pt.render(1)
            mv = pt.motion_vectors()
            torch.cuda.synchronize()
            flows.append(mv.cpu().numpy())
        finally:
            pt.close_engine()
    assert np.array_equal(_bits(flows[0]), _bits(flows[1])), accel
    moved = np.isfinite(flows[0]).all(1) & (np.abs(flows[0]).max(1) > 0.5)
    assert moved.any(), "no pixel saw the move"


# ------------------------------------------------------------------ 10. frames in flight
@pytest.mark.parametrize("accel", ACCELS)
def test_frames_in_flight_are_dropped(accel, monkeypatch):
    _accel(monkeypatch, accel)
    pt = _pass(world())
    try:
        pt.render(1, continues=True)
        _move(pt, GRIDS)
        _same(_state(pt), fresh(GRIDS), (accel, "after a continued render"))
    finally:
        pt.close_engine()


# ------------------------------------------------------------------ 11. the scaling claim, without a timer
@pytest.mark.parametrize("accel", ["flat", "two_level"])
def test_launches_and_syncs_do_not_depend_on_the_count(accel, monkeypatch):
    _accel(monkeypatch, accel)
    counts = []
    for ids in ((3, 11), GRIDS):
        pt = _pass(world())
        try:
            _move(pt, ids)
            info = pt.instances_device_info()
            assert info["instances"] == len(ids)
            counts.append((info["last_launches"], info["last_syncs"]))
        finally:
            pt.close_engine()
    assert counts[0] == counts[1], counts
    assert counts[0][0] >= 3 and counts[0][1] >= 2, counts
