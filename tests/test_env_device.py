"""The env map updated in place: texels from device memory with the CDF tables rebuilt on the GPU
(pupil_pt_update_env_device, pt_envmap.hip), and scale / rotation alone (pupil_pt_update_env_params).

The yardstick throughout: an updated engine equals a fresh one -- a second engine created from a
World that loaded the new texels (or rotation and scale) from its own PFM and XML -- bit for bit,
on uint32 views: the tables, the SampleDirect and Eval probes, every output buffer.  Scenes and
inputs: env_device_cases.py; film 8 x 8, 2 spp, depth 2."""
import ctypes as C

import numpy as np
import pytest

from pupiloptixlab_amd import abi, scenes

import env_device_cases as ec
import sampling_cases as sc
from test_gpu_sampling_probes import N, P, gpu_env
from test_visibility import KEYS, _assert_render_equals, _pass, _render

pytestmark = pytest.mark.gpu

SPP = 2
ACCELS = ["flat", "two_level"]
TABLES = ("col_cdf", "row_cdf", "row_weight", "normalization")


def _accel(monkeypatch, accel):
    """flat | two_level (PUPIL_TL_MODE=world), as test_material_update._accel"""
    monkeypatch.setenv("PUPIL_ACCEL", "flat" if accel == "flat" else "two_level")
    if accel != "flat":
        monkeypatch.setenv("PUPIL_TL_MODE", "world")


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same_tables(got, ref, what):
    assert (got["width"], got["height"]) == (ref["width"], ref["height"]), what
    for k in TABLES:
        a, b = _bits(got[k]).reshape(-1), _bits(ref[k]).reshape(-1)
        bad = np.flatnonzero(a != b)
        assert bad.size == 0, f"{what}: {k} differs in {bad.size} of {a.size} entries, first at {bad[0]}"


def _same_render(got, fresh, what):
    """every buffer of KEYS against the fresh engine's, through test_visibility's comparison"""
    ref = {"accum": fresh["pt accum buffer"], "albedo": fresh["albedo"], "normal": fresh["normal"], "test": fresh["test"]}
    _assert_render_equals(got, ref, what)
    assert np.array_equal(_bits(got["final result"]), _bits(fresh["final result"])), (what, "final result")


def _probes(pt):
    xi = ec.probe_xi(pt.env_tables()["row_cdf"])
    return gpu_env(pt, xi, 0), gpu_env(pt, ec.probe_dirs(), 1, pos=np.zeros(3, np.float32))


def _same_probes(pt, fresh, what):
    # the same inputs on both: xi from the fresh engine's table (the updated one's equals it or the test fails anyway)
    xi = ec.probe_xi(fresh.env_tables()["row_cdf"])
    dirs = ec.probe_dirs()
    assert len(xi) == 256 and len(dirs) == 256
    for mode, x, kw in ((0, xi, {}), (1, dirs, {"pos": np.zeros(3, np.float32)})):
        a, b = gpu_env(pt, x, mode, **kw), gpu_env(fresh, x, mode, **kw)
        bad = np.flatnonzero((_bits(a) != _bits(b)).any(axis=1))
        assert bad.size == 0, f"{what}: mode {mode} differs on {bad.size} inputs, first {x[bad[0]]}: {a[bad[0]]} != {b[bad[0]]}"
        if mode == 0:  # row index h (xi.x above row_cdf[h - 1]) reads the trailing zero: pdf 0
            assert (a[3:11, 3] == 0).all()


def _device(pt, rgba):
    import torch

    return torch.from_numpy(np.ascontiguousarray(rgba, np.float32)).to(pt.device)


def _pair(size, tag):
    """two worlds of one size with texels from two seeds: the engine's and the fresh one's"""
    w, h = size
    return (ec.env_world(ec.texels(w, h, 1), f"{tag}_{w}x{h}_a"), ec.env_world(ec.texels(w, h, 2), f"{tag}_{w}x{h}_b"))


# ------------------------------------------------------------------ 1. + 2. tables and probes
@pytest.mark.parametrize("size", ec.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_tables_and_probes_equal_a_fresh_engine(size):
    wa, wb = _pair(size, "tables")
    new = ec.desc_texels(wb.desc())
    assert new.shape == (size[1], size[0], 4)
    pt, fresh = _pass(wa), _pass(wb)
    try:
        before, ref = pt.env_tables(), fresh.env_tables()
        assert ref["col_cdf"].shape == (size[1], size[0] + 1) and ref["row_cdf"].shape == (size[1] + 1,)
        assert not np.array_equal(_bits(before["col_cdf"]), _bits(ref["col_cdf"]))  # the update has something to do
        assert np.isfinite(ref["col_cdf"]).all() and np.isfinite(ref["row_cdf"]).all()
        pt.update_env_device(_device(pt, new))
        assert pt.dirty
        got = pt.env_tables()
        _same_tables(got, ref, f"tables {size}")
        assert np.array_equal(_bits(got["row_weight"]), _bits(before["row_weight"]))  # it depends on h only
        assert pt.env_info()["updates"] == 1 and pt.env_info()["last_ms"] > 0.0
        _same_probes(pt, fresh, f"probes {size}")
    finally:
        pt.close_engine()
        fresh.close_engine()


# ------------------------------------------------------------------ 3. render
@pytest.mark.parametrize("accel", ACCELS)
def test_render_equals_a_fresh_engine(accel, monkeypatch):
    _accel(monkeypatch, accel)
    wa, wb = _pair(ec.RENDER_SIZE, "render")
    pt, fresh = _pass(wa), _pass(wb)
    try:
        before = _render(pt, SPP)
        pt.update_env_device(_device(pt, ec.desc_texels(wb.desc())))
        got, ref = _render(pt, SPP), _render(fresh, SPP)
        assert not np.array_equal(got["pt accum buffer"], before["pt accum buffer"])
        _same_render(got, ref, f"render {accel}")
    finally:
        pt.close_engine()
        fresh.close_engine()


# ------------------------------------------------------------------ 4. side stream
@pytest.mark.parametrize("accel", ACCELS)
def test_texels_from_a_side_stream(accel, monkeypatch):
    """the tensor is filled by a kernel on a non-default stream and handed over right after it,
    with no synchronise in between: the engine's copy must wait for the kernel"""
    import torch

    _accel(monkeypatch, accel)
    wa, wb = _pair(ec.RENDER_SIZE, "side")
    w, h = ec.RENDER_SIZE
    new = ec.desc_texels(wb.desc())
    pt, fresh = _pass(wa), _pass(wb)
    try:
        _render(pt, SPP)
        # 2 x the texels, tiled to 1024 x 1024 texels: a kernel that takes a while, and * 0.5 is exact
        big = torch.from_numpy(np.tile(new * np.float32(2.0), (128, 64, 1))).to(pt.device)
        torch.cuda.synchronize()
        side = torch.cuda.Stream(device=pt.device)
        with torch.cuda.stream(side):
            dev = (big * 0.5)[:h, :w].contiguous()
            pt.update_env_device(dev, stream=side)
        _same_tables(pt.env_tables(), fresh.env_tables(), f"side stream {accel}")
        _same_render(_render(pt, SPP), _render(fresh, SPP), f"side stream {accel}")
    finally:
        pt.close_engine()
        fresh.close_engine()


# ------------------------------------------------------------------ 5. back to the host
def test_host_update_after_a_device_update_restores_the_env():
    """pupil_pt_update_emitters with the ORIGINAL desc after a device update: the desc equals the
    engine's stale env_src byte for byte, and must all the same replace the device-fed texels"""
    wa, wb = _pair(ec.RENDER_SIZE, "back")
    desc = wa.desc()
    pt = _pass(wa)
    try:
        before, tables = _render(pt, SPP), pt.env_tables()
        pt.update_env_device(_device(pt, ec.desc_texels(wb.desc())))
        assert not np.array_equal(_render(pt, SPP)["pt accum buffer"], before["pt accum buffer"])
        abi.check(pt._lib.pupil_pt_update_emitters(pt._pt, C.byref(desc)))
        _same_tables(pt.env_tables(), tables, "back to the host: tables")
        _same_render(_render(pt, SPP), before, "back to the host")
        # and the same after a parameter update alone
        e = desc.env.contents
        pt.update_env_params(0.25, np.eye(3, dtype=np.float32))
        assert not np.array_equal(_render(pt, SPP)["pt accum buffer"], before["pt accum buffer"])
        abi.check(pt._lib.pupil_pt_update_emitters(pt._pt, C.byref(desc)))
        _same_render(_render(pt, SPP), before, "back to the host after update_env_params")
        assert e.scale == np.float32(ec.SCALE)
    finally:
        pt.close_engine()


# ------------------------------------------------------------------ 6. scale and rotation
def test_params_equal_a_fresh_engine():
    w, h = ec.RENDER_SIZE
    rotation, scale = '<rotate value="0.3, 1, -0.4" angle="75"/>', 2.25
    wa = ec.env_world(ec.texels(w, h, 1), "params_a")
    wr = ec.env_world(ec.texels(w, h, 1), "params_a_rot", rotation, scale)    # the same texels, rotated
    wbr = ec.env_world(ec.texels(w, h, 2), "params_b_rot", rotation, scale)   # other texels, rotated
    e = wr.desc().env.contents
    to_world = np.array(list(e.to_world), np.float32)
    assert e.scale == np.float32(scale) and not np.array_equal(to_world, np.array(list(wa.desc().env.contents.to_world)))
    pt, fresh = _pass(wa), _pass(wr)
    try:
        before, tables = _render(pt, SPP), pt.env_tables()
        pt.update_env_params(scale, to_world.reshape(3, 3))
        assert pt.dirty and pt.env_info()["updates"] == 1
        _same_tables(pt.env_tables(), tables, "params: the tables stay")
        _same_tables(pt.env_tables(), fresh.env_tables(), "params: fresh tables")
        _same_probes(pt, fresh, "params")
        got = _render(pt, SPP)
        assert not np.array_equal(got["pt accum buffer"], before["pt accum buffer"])
        _same_render(got, _render(fresh, SPP), "params")
        # the device-fed state takes parameters too
        fresh.close_engine()
        fresh = _pass(wbr)
        pt.update_env_device(_device(pt, ec.desc_texels(wbr.desc())))
        pt.update_env_params(1.0, np.eye(3, dtype=np.float32))
        pt.update_env_params(scale, to_world)
        assert pt.env_info()["updates"] == 4
        _same_tables(pt.env_tables(), fresh.env_tables(), "params after device texels")
        _same_probes(pt, fresh, "params after device texels")
        _same_render(_render(pt, SPP), _render(fresh, SPP), "params after device texels")
    finally:
        pt.close_engine()
        fresh.close_engine()


# ------------------------------------------------------------------ 7. pipelining
def test_update_drops_frames_in_flight():
    """modelled on test_material_update.test_update_drops_frames_in_flight"""
    import torch

    wa, wb = _pair(ec.RENDER_SIZE, "flight")
    w, h = ec.RENDER_SIZE
    pt = _pass(wa)
    try:
        pt.mark_dirty()
        for _ in range(4):
            pt.render(1, continues=True)
        torch.cuda.synchronize()
        assert pt.stats()["frames_in_flight"] > 0
        seed, cnt = pt.random_seed, pt.sample_cnt
        # straight through the ABI: the pass's counters go on, so the next render WOULD continue
        # the sequence and take the frame shaded ahead under the old env map
        dev = _device(pt, ec.desc_texels(wb.desc()))
        abi.check(pt._lib.pupil_pt_update_env_device(pt._pt, C.c_void_p(dev.data_ptr()), w, h, None))
        for k in KEYS:
            pt.buffers.get(k).zero_()
        pt.dirty = False
        pt.render(1, continues=True)
        torch.cuda.synchronize()
        got = {k: pt.buffers.get(k).cpu().numpy() for k in KEYS}
        fresh = _pass(wb)
        try:
            fresh.random_seed, fresh.sample_cnt, fresh.dirty = seed, cnt, False
            fresh.render(1)
            torch.cuda.synchronize()
            _same_render(got, {k: fresh.buffers.get(k).cpu().numpy() for k in KEYS}, "first render after the update")
            # the same for the parameters: frames are in flight again
            for _ in range(3):
                pt.render(1, continues=True)
            torch.cuda.synchronize()
            assert pt.stats()["frames_in_flight"] > 0
            ident = np.eye(3, dtype=np.float32).reshape(-1)
            abi.check(pt._lib.pupil_pt_update_env_params(pt._pt, 0.5, ident.ctypes.data_as(abi.f32p),
                                                         ident.ctypes.data_as(abi.f32p)))
            fresh.close_engine()
            fresh = _pass(ec.env_world(ec.texels(w, h, 2), "flight_ident", '<rotate y="1" angle="0"/>', 0.5))
            seed, cnt = pt.random_seed, pt.sample_cnt
            for k in KEYS:
                pt.buffers.get(k).zero_()
            pt.render(1, continues=True)
            fresh.random_seed, fresh.sample_cnt, fresh.dirty = seed, cnt, False
            fresh.render(1)
            torch.cuda.synchronize()
            _same_render({k: pt.buffers.get(k).cpu().numpy() for k in KEYS},
                         {k: fresh.buffers.get(k).cpu().numpy() for k in KEYS}, "first render after update_env_params")
        finally:
            fresh.close_engine()
    finally:
        pt.close_engine()


# ------------------------------------------------------------------ 8. refusals
def _refused(pt, calls, what):
    before = _render(pt, SPP)
    for k, call in enumerate(calls):
        assert call() == abi.ERR_INVALID, (what, k)
        assert pt._lib.pupil_last_error(), (what, k)
    assert pt.env_info()["updates"] == 0, what
    after = _render(pt, SPP)
    for k in KEYS:
        assert np.array_equal(_bits(after[k]), _bits(before[k])), (what, k)


def test_refusals():
    import os
    import torch

    from pupiloptixlab_amd import World

    w, h = ec.RENDER_SIZE
    ident = np.eye(3, dtype=np.float32).reshape(-1)
    i9 = ident.ctypes.data_as(abi.f32p)
    sizing = lambda p: p._lib.pupil_debug_read_env_tables(p._pt, C.byref(C.c_uint32()), C.byref(C.c_uint32()), None, None,
                                                          None, None)
    no_env = World().load_scene(scenes.cornell_xml(os.path.join(sc.TMP, "env_device_cornell.xml"), 8, 8, 2))
    for what, world in (("no env", no_env), ("constant env", sc.const_env_scene())):
        pt = _pass(world)
        try:
            dev = _device(pt, np.ones((h, w, 4), np.float32))
            ptr = C.c_void_p(dev.data_ptr())
            _refused(pt, [lambda: pt._lib.pupil_pt_update_env_device(pt._pt, ptr, w, h, None),
                          lambda: pt._lib.pupil_pt_update_env_params(pt._pt, 1.0, i9, i9),
                          lambda: sizing(pt)], what)
            with pytest.raises(abi.PupilError):
                pt.update_env_device(dev)
        finally:
            pt.close_engine()
    wa, wb = _pair(ec.RENDER_SIZE, "refuse")
    pt = _pass(wa)
    lib = pt._lib
    try:
        good = _device(pt, ec.desc_texels(wb.desc()))
        other = _device(pt, np.ones((h + 1, w, 4), np.float32))
        pg, po = C.c_void_p(good.data_ptr()), C.c_void_p(other.data_ptr())
        tables = pt.env_tables()
        _refused(pt, [lambda: lib.pupil_pt_update_env_device(pt._pt, po, w, h + 1, None),   # another size
                      lambda: lib.pupil_pt_update_env_device(pt._pt, pg, h, w, None),       # the same texel count, transposed
                      lambda: lib.pupil_pt_update_env_device(pt._pt, None, w, h, None),
                      lambda: lib.pupil_pt_update_env_device(None, pg, w, h, None),
                      lambda: lib.pupil_pt_update_env_params(pt._pt, 1.0, None, i9),
                      lambda: lib.pupil_pt_update_env_params(pt._pt, 1.0, i9, None),
                      lambda: lib.pupil_pt_update_env_params(None, 1.0, i9, i9),
                      lambda: lib.pupil_pt_env_info(None, None, None),
                      lambda: lib.pupil_debug_read_env_tables(None, None, None, None, None, None, None)], "env map")
        assert b"pupil_pt_update_emitters first" in (lib.pupil_pt_update_env_device(pt._pt, po, w, h + 1, None),
                                                     lib.pupil_last_error())[1]
        _same_tables(pt.env_tables(), tables, "after the refused calls")
        # the pass rejects what is no (h, w, 4) float32 tensor on its device before the engine sees it
        bad = [ec.desc_texels(wb.desc()), good.double(), good[:, :, :3], good.reshape(-1), good.cpu(),
               good.transpose(0, 1), good[:, ::2]]
        if torch.cuda.device_count() > 1:
            bad.append(good.to("cuda:1"))
        for t in bad:
            with pytest.raises(ValueError):
                pt.update_env_device(t)
        with pytest.raises(ValueError):
            pt.update_env_params(1.0, np.eye(4))
        with pytest.raises(abi.PupilError):
            pt.update_env_params(1.0, np.zeros((3, 3)))  # singular: no inverse
        assert pt.env_info()["updates"] == 0
        # and the accepted one counts
        pt.update_env_device(good)
        assert pt.env_info()["updates"] == 1
        fresh = _pass(wb)
        try:
            _same_render(_render(pt, SPP), _render(fresh, SPP), "accepted after the refusals")
        finally:
            fresh.close_engine()
    finally:
        pt.close_engine()


# ------------------------------------------------------------------ 9. memory
def test_repeated_updates_allocate_nothing():
    import torch

    size = (ec.ENV_STAGE + 6, 3)
    wa, wb = _pair(size, "memory")
    pt = _pass(wa)
    free = lambda: torch.cuda.mem_get_info(pt.device_index)[0]
    try:
        _render(pt, SPP)  # the ring and every lazily allocated buffer exist from here on
        devs = [_device(pt, ec.desc_texels(wa.desc())), _device(pt, ec.desc_texels(wb.desc()))]
        torch.cuda.synchronize()
        f0 = free()
        pt.update_env_device(devs[1])
        pt.update_env_device(devs[0])
        f2 = free()
        for k in range(10):
            pt.update_env_device(devs[(k + 1) % 2])
        f12 = free()
        print(f"free before the first update {f0}, after the 2nd {f2}, after the 12th {f12}")
        assert f12 == f2
        assert pt.env_info()["updates"] == 12
        fresh = _pass(wa)  # the 12th update put the first texels back
        try:
            _same_tables(pt.env_tables(), fresh.env_tables(), "after 12 updates")
        finally:
            fresh.close_engine()
    finally:
        pt.close_engine()
