"""Materials and textures updated in place (pupil_pt_update_materials,
pupil_pt_update_texture_device).

The yardstick throughout: an updated engine equals a freshly created one, and both equal the CPU
oracle's render of a world built from scratch with the final materials, bit for bit on every
buffer in KEYS.  Scene and restatements: material_cases.py; film 64 x 48, 2 spp, depth 4."""
import ctypes as C

import numpy as np
import pytest

import oracle
from pupiloptixlab_amd import abi
from pupiloptixlab_amd import world as W

from material_cases import (CUBE, FLOOR, LIGHT, SPHERE, SPP, base_materials, build_world, mixed_materials,
                            sequential_sums, specular_weight, texels, wide_texels)
from test_visibility import KEYS, _assert_render_equals, _pass, _render

pytestmark = pytest.mark.gpu

ACCELS = ["flat", "two_level"]
UV = np.random.default_rng(5).uniform(-0.5, 1.5, (64, 2)).astype(np.float32)  # the fixed uv set (wraps included)


def _accel(monkeypatch, accel):
    """flat | two_level (PUPIL_TL_MODE=world), as test_deform._accel"""
    monkeypatch.setenv("PUPIL_ACCEL", "flat" if accel == "flat" else "two_level")
    if accel != "flat":
        monkeypatch.setenv("PUPIL_TL_MODE", "world")


def _same(a, b, what):
    for k in KEYS:
        assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), (what, k)


def _tex_sample(pt, material, slot):
    out = np.zeros((len(UV), 3), np.float32)
    abi.check(pt._lib.pupil_debug_tex_sample(pt._pt, material, slot, len(UV), UV.ctypes.data_as(abi.f32p),
                                             out.ctypes.data_as(abi.f32p)))
    return out


def _check(pt, mats, what, sample=None):
    """pt (updated in place) against a fresh engine and the oracle, both on a world built from
    scratch with `mats`; sample = (material, slot): the texture probe too.  Returns pt's render."""
    got = _render(pt, SPP)
    w = build_world(mats)
    _assert_render_equals(got, oracle.OracleScene(w.desc()).render(spp=SPP), what + ": oracle")
    fresh = _pass(w)
    try:
        _same(got, _render(fresh, SPP), what + ": fresh engine")
        if sample:
            a, b = _tex_sample(pt, *sample), _tex_sample(fresh, *sample)
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (what, "tex_sample")
    finally:
        fresh.close_engine()
    return got


def _apply(pt, w, mats, changes):
    """changes: {material: abi.Material}; one engine call for all of them"""
    for i, m in changes.items():
        w.set_material(i, m)
        mats[i] = m
    pt.update_materials(w, list(changes))


# ------------------------------------------------------------------ 1. parameter edits within a type
@pytest.mark.parametrize("accel", ACCELS)
def test_parameter_edits(accel, monkeypatch):
    _accel(monkeypatch, accel)
    mats = mixed_materials()
    w = build_world(mats)
    pt = _pass(w)
    try:
        prev = _check(pt, mats, "as created")
        refits = pt.stats()["accel_refits"]
        edits = [("diffuse reflectance", {FLOOR: W.twosided(W.diffuse((0.2, 0.7, 0.3)))}),
                 ("rough conductor alpha and eta", {SPHERE: W.rough_conductor(0.45, (0.14, 0.4, 1.5), (3.9, 2.4, 2.2))}),
                 ("dielectric IORs", {CUBE: W.dielectric(1.9, 1.1)}),
                 ("twosided off", {FLOOR: W.diffuse((0.2, 0.7, 0.3))})]
        for k, (what, changes) in enumerate(edits):
            _apply(pt, w, mats, changes)
            got = _check(pt, mats, what)
            if "twosided" not in what:  # the floor is seen from its front: the toggle need not show
                assert not np.array_equal(got["pt accum buffer"], prev["pt accum buffer"]), what
            prev = got
            assert pt.material_info()["updates"] == k + 1
        assert pt.stats()["accel_refits"] == refits  # the structure is not touched
    finally:
        pt.close_engine()


# ------------------------------------------------------------------ 2. type changes
def _type_cycle():
    return [("dielectric", W.dielectric(1.5, 1.0)), ("rough_plastic", W.rough_plastic(0.2, (0.2, 0.5, 0.3), 0.8)),
            ("diffuse", W.twosided(W.diffuse((0.7, 0.4, 0.3))))]


@pytest.mark.parametrize("shade_list", ["auto", "bins"])
@pytest.mark.parametrize("accel", ACCELS)
def test_type_changes(accel, shade_list, monkeypatch):
    """diffuse -> dielectric -> rough_plastic -> diffuse on one material of a scene whose instances
    all share the diffuse bin: one bin -> two -> two others -> one, so shade_list / single_bin
    flip in both directions (auto), or stay on the partition (PUPIL_SHADE_LIST=bins forced)."""
    _accel(monkeypatch, accel)
    if shade_list != "auto":
        monkeypatch.setenv("PUPIL_SHADE_LIST", shade_list)
    mats = base_materials()
    w = build_world(mats)
    pt = _pass(w)
    try:
        _check(pt, mats, "as created")
        for what, m in _type_cycle():
            _apply(pt, w, mats, {SPHERE: m})
            _check(pt, mats, what)
        assert pt.stats()["accel_refits"] == 0
    finally:
        pt.close_engine()


@pytest.mark.parametrize("accel", ACCELS)
def test_one_bin_to_two_and_back(accel, monkeypatch):
    """the cube (a builtin mesh) and then the floor leave the scene's only bin and come back"""
    _accel(monkeypatch, accel)
    mats = base_materials()
    w = build_world(mats)
    pt = _pass(w)
    try:
        for what, changes in (("cube conductor", {CUBE: W.conductor((0.2, 0.9, 1.1), (3.9, 2.4, 2.2))}),
                              ("cube diffuse again", {CUBE: W.diffuse((0.3, 0.5, 0.8))}),
                              ("floor plastic, cube rough dielectric",
                               {FLOOR: W.plastic((0.4, 0.3, 0.2), 0.9), CUBE: W.rough_dielectric(0.1, 1.5, 1.0)}),
                              ("all diffuse", {FLOOR: W.twosided(W.diffuse((0.6, 0.6, 0.55))), CUBE: W.diffuse((0.3, 0.5, 0.8))})):
            _apply(pt, w, mats, changes)
            _check(pt, mats, what)
    finally:
        pt.close_engine()


# ------------------------------------------------------------------ 3. texture kinds and sizes on one slot
@pytest.mark.parametrize("accel", ACCELS)
def test_texture_kind_and_size_changes(accel, monkeypatch):
    _accel(monkeypatch, accel)
    mats = base_materials()
    w = build_world(mats)
    pt = _pass(w)
    t53, t88 = texels(5, 3, 7), texels(8, 8, 8)
    steps = [("checkerboard", W.checkerboard((0.9, 0.1, 0.1), (0.1, 0.1, 0.9), (4.0, 3.0))),
             ("bitmap 5x3 point", W.bitmap(t53, filter=0)),
             ("bitmap 5x3 bilinear", W.bitmap(t53, filter=1, uv_scale=(2.0, 1.0))),
             ("bitmap 8x8", W.bitmap(t88, filter=1)),
             ("bitmap 5x3 again", W.bitmap(t53, filter=0)),
             ("rgb", W.rgb(0.7, 0.4, 0.3))]
    try:
        for what, tex in steps:
            _apply(pt, w, mats, {SPHERE: W.twosided(W.diffuse(tex))})
            _check(pt, mats, what, sample=(SPHERE, 0))
    finally:
        pt.close_engine()


# ------------------------------------------------------------------ 4. device texels
@pytest.mark.parametrize("accel", ACCELS)
def test_device_texels_on_a_side_stream(accel, monkeypatch):
    """the tensor is filled by a kernel on a non-default stream and handed over right after it,
    with no synchronise in between: the engine's copy must wait for the kernel"""
    import torch

    _accel(monkeypatch, accel)
    mats = base_materials()
    mats[SPHERE] = W.twosided(W.diffuse(W.bitmap(texels(5, 3, 11), filter=1)))
    w = build_world(mats)
    pt = _pass(w)
    try:
        _check(pt, mats, "as created")
        src_host = texels(5, 3, 12)
        big = torch.from_numpy(np.tile(src_host, (256, 256, 1))).to(pt.device)  # 768 x 1280 texels: a kernel that takes a while
        torch.cuda.synchronize()
        side = torch.cuda.Stream(device=pt.device)
        with torch.cuda.stream(side):
            dev = (big * 0.5)[:3, :5].contiguous()  # * 0.5 is exact: the host knows the texels bit for bit
            pt.update_texture_device(SPHERE, 0, dev, stream=side)
        mats[SPHERE] = W.twosided(W.diffuse(W.bitmap((src_host * np.float32(0.5)).astype(np.float32), filter=1)))
        _check(pt, mats, "device texels", sample=(SPHERE, 0))
    finally:
        pt.close_engine()


SIZES = [(1, 1), (64, 2), (67, 3), (130, 1)]  # w x h: one texel, whole steps of the wave, a partial last step, 2 steps + 2


def _plastic(kind, diffuse, specular):
    return W.plastic(diffuse, specular) if kind == "plastic" else W.rough_plastic(0.2, diffuse, specular)


def _as_texture(t):
    return W.bitmap(t, filter=0) if isinstance(t, np.ndarray) else W.rgb(*t)


@pytest.mark.parametrize("accel", ACCELS)
def test_device_texels_recompute_the_plastic_weight(accel, monkeypatch):
    """specular_sampling_weight after a device update, read back from the device, against the
    float32 restatement of GetPixelAverage and the weight formula, as bit patterns: plastic and
    rough_plastic; the diffuse slot, the specular slot, or both a bitmap with one of them updated."""
    import torch

    _accel(monkeypatch, accel)
    mats = base_materials()
    w = build_world(mats)
    pt = _pass(w)
    const = (0.3, 0.6, 0.2)
    try:
        seed = 100
        for kind in ("plastic", "rough_plastic"):
            first = 0 if kind == "plastic" else 1  # the diffuse slot; the specular one follows
            for wd, ht in SIZES:
                for mode in ("diffuse", "specular", "both"):
                    seed += 1
                    old, other, new = wide_texels(wd, ht, seed), wide_texels(wd, ht, 1000 + seed), wide_texels(wd, ht, 2000 + seed)
                    if wd * ht >= 128:  # the order of the adds shows in the bits: no pass by luck
                        pair = [np.sum(new[..., c].reshape(-1), dtype=np.float32) for c in range(3)]
                        assert any(p.view(np.uint32) != s.view(np.uint32) for p, s in zip(pair, sequential_sums(new)))
                    before = {"diffuse": (old, const), "specular": (const, old), "both": (old, other)}[mode]
                    after = {"diffuse": (new, const), "specular": (const, new), "both": (new, other)}[mode]
                    _apply(pt, w, mats, {CUBE: _plastic(kind, _as_texture(before[0]), _as_texture(before[1]))})
                    got = pt.read_material(CUBE)["specular_sampling_weight"]
                    assert got.view(np.uint32) == specular_weight(*before).view(np.uint32), (kind, wd, ht, mode, "host")
                    slot = first + (1 if mode == "specular" else 0)
                    pt.update_texture_device(CUBE, slot, torch.from_numpy(new).to(pt.device))
                    got = pt.read_material(CUBE)
                    want = specular_weight(*after)
                    assert got["type"] == (abi.MAT_PLASTIC if kind == "plastic" else abi.MAT_ROUGH_PLASTIC)
                    assert got["specular_sampling_weight"].view(np.uint32) == want.view(np.uint32), (kind, wd, ht, mode)
        # and the render uses it: the last state against a fresh engine and the oracle
        mats[CUBE] = _plastic(kind, _as_texture(after[0]), _as_texture(after[1]))
        _check(pt, mats, "after the device updates", sample=(CUBE, slot))
        # a slot outside the pair, and a material that is no plastic, launch nothing and change no weight
        _apply(pt, w, mats, {CUBE: W.rough_plastic(W.bitmap(texels(5, 3, 1), filter=0), (0.2, 0.5, 0.3), 0.8)})
        before = pt.read_material(CUBE)["specular_sampling_weight"]
        pt.update_texture_device(CUBE, 0, torch.from_numpy(texels(5, 3, 2)).to(pt.device))
        assert pt.read_material(CUBE)["specular_sampling_weight"].view(np.uint32) == before.view(np.uint32)
    finally:
        pt.close_engine()


# ------------------------------------------------------------------ 5. partial writes
@pytest.mark.parametrize("accel", ACCELS)
def test_other_materials_keep_a_device_weight(accel, monkeypatch):
    import torch

    _accel(monkeypatch, accel)
    mats = base_materials()
    mats[CUBE] = W.plastic(W.bitmap(wide_texels(67, 3, 31), filter=0), (0.3, 0.6, 0.2))
    w = build_world(mats)
    pt = _pass(w)
    try:
        new = wide_texels(67, 3, 32)
        pt.update_texture_device(CUBE, 0, torch.from_numpy(new).to(pt.device))
        weight = pt.read_material(CUBE)["specular_sampling_weight"]
        assert weight.view(np.uint32) == specular_weight(new, (0.3, 0.6, 0.2)).view(np.uint32)
        assert weight.view(np.uint32) != specular_weight(wide_texels(67, 3, 31), (0.3, 0.6, 0.2)).view(np.uint32)
        # one call, two OTHER materials: the engine's host mirror of the cube's weight is stale
        # and must not come back
        _apply(pt, w, mats, {SPHERE: W.twosided(W.diffuse((0.1, 0.8, 0.4))), FLOOR: W.rough_conductor(0.3)})
        assert pt.read_material(CUBE)["specular_sampling_weight"].view(np.uint32) == weight.view(np.uint32)
        mats[CUBE] = W.plastic(W.bitmap(new, filter=0), (0.3, 0.6, 0.2))  # the final state, from scratch
        _check(pt, mats, "two materials updated, a third holds device texels")
    finally:
        pt.close_engine()


# ------------------------------------------------------------------ 6. pipelining
def test_update_drops_frames_in_flight():
    import torch

    mats = base_materials()
    w = build_world(mats)
    pt = _pass(w)
    try:
        pt.mark_dirty()
        for _ in range(4):
            pt.render(1, continues=True)
        torch.cuda.synchronize()
        assert pt.stats()["frames_in_flight"] > 0
        seed, cnt = pt.random_seed, pt.sample_cnt
        # straight through the ABI: the pass's counters go on, so the next render WOULD continue
        # the sequence and take the frame shaded ahead with the old material
        new = W.twosided(W.diffuse((0.1, 0.9, 0.2)))
        w.set_material(SPHERE, new)
        mats[SPHERE] = new
        ids = (C.c_uint32 * 1)(SPHERE)
        abi.check(pt._lib.pupil_pt_update_materials(pt._pt, 1, ids, C.byref(w.desc().materials[SPHERE])))
        for k in KEYS:
            pt.buffers.get(k).zero_()
        pt.dirty = False
        pt.render(1, continues=True)
        torch.cuda.synchronize()
        got = {k: pt.buffers.get(k).cpu().numpy() for k in KEYS}
        fresh = _pass(build_world(mats))
        try:
            fresh.random_seed, fresh.sample_cnt, fresh.dirty = seed, cnt, False
            fresh.render(1)
            torch.cuda.synchronize()
            _same(got, {k: fresh.buffers.get(k).cpu().numpy() for k in KEYS}, "first render after the update")
        finally:
            fresh.close_engine()
        # through the pass: accumulation restarts and a render that continues nothing keeps no frame
        pt.update_material(w, SPHERE)
        assert pt.dirty
        _check(pt, mats, "after the ring was dropped")
        assert pt.stats()["frames_in_flight"] == 0
    finally:
        pt.close_engine()


# ------------------------------------------------------------------ 7. no-op and refusals
@pytest.mark.parametrize("accel", ACCELS)
def test_noop_and_refusals(accel, monkeypatch):
    import torch

    _accel(monkeypatch, accel)
    mats = mixed_materials()
    mats[FLOOR] = W.twosided(W.diffuse(W.bitmap(texels(5, 3, 41), filter=1)))
    w = build_world(mats)
    pt = _pass(w)
    lib = pt._lib
    try:
        before = _render(pt, SPP)
        refits = pt.stats()["accel_refits"]
        pt.update_materials(w, [SPHERE, FLOOR, CUBE, LIGHT])  # every material to itself
        _same(_render(pt, SPP), before, "no-op update")
        assert pt.stats()["accel_refits"] == refits
        assert pt.material_info()["updates"] == 1 and pt.material_info()["last_ms"] > 0.0

        desc = w.desc()
        n = desc.num_materials
        good = W.diffuse((0.1, 0.2, 0.3))
        empty = W.diffuse((0.1, 0.2, 0.3))
        empty.tex[0].type = abi.TEX_BITMAP
        empty.tex[0].width = empty.tex[0].height = 2  # rgba stays NULL
        unknown = W.diffuse((0.1, 0.2, 0.3))
        unknown.tex[3].type = 7
        two = (abi.Material * 2)(good, empty)  # the first entry is fine: nothing of it may be applied
        dev53 = torch.from_numpy(texels(5, 3, 42)).to(pt.device)
        dev88 = torch.from_numpy(texels(8, 8, 43)).to(pt.device)
        p53, p88 = C.c_void_p(dev53.data_ptr()), C.c_void_p(dev88.data_ptr())
        ids = lambda *v: (C.c_uint32 * len(v))(*v)
        refused = [
            lambda: lib.pupil_pt_update_materials(pt._pt, 1, ids(n), C.byref(good)),                # bad material id
            lambda: lib.pupil_pt_update_materials(pt._pt, 2, ids(SPHERE, n), (abi.Material * 2)(good, good)),
            lambda: lib.pupil_pt_update_materials(pt._pt, 2, ids(SPHERE, CUBE), two),               # bitmap without texels
            lambda: lib.pupil_pt_update_materials(pt._pt, 1, ids(SPHERE), C.byref(unknown)),        # unknown texture type
            lambda: lib.pupil_pt_update_materials(pt._pt, 1, None, None),
            lambda: lib.pupil_pt_update_texture_device(pt._pt, n, 0, p53, 5, 3, None),              # bad material id
            lambda: lib.pupil_pt_update_texture_device(pt._pt, FLOOR, 4, p53, 5, 3, None),          # slot 4
            lambda: lib.pupil_pt_update_texture_device(pt._pt, FLOOR, 1, p53, 5, 3, None),          # an rgb slot
            lambda: lib.pupil_pt_update_texture_device(pt._pt, FLOOR, 0, p88, 8, 8, None),          # another size
            lambda: lib.pupil_pt_update_texture_device(pt._pt, FLOOR, 0, p53, 3, 5, None),          # the same texel count, transposed
            lambda: lib.pupil_pt_update_texture_device(pt._pt, FLOOR, 0, None, 5, 3, None),
        ]
        for k, call in enumerate(refused):
            assert call() == abi.ERR_INVALID, k
            assert lib.pupil_last_error(), k
        assert b"pupil_pt_update_materials first" in (lib.pupil_pt_update_texture_device(pt._pt, FLOOR, 0, p88, 8, 8, None),
                                                      lib.pupil_last_error())[1]
        assert pt.material_info()["updates"] == 1
        _same(_render(pt, SPP), before, "after the refused calls")
        # the pass rejects what is no (h, w, 4) float32 tensor on its device before the engine sees it
        for bad in (texels(5, 3, 42), dev53.double(), dev53[:, :, :3], dev53.reshape(-1), dev53.cpu(),
                    dev88.transpose(0, 1)):
            with pytest.raises(ValueError):
                pt.update_texture_device(FLOOR, 0, bad)
        assert pt.material_info()["updates"] == 1
        # and the accepted one counts
        pt.update_texture_device(FLOOR, 0, dev53)
        assert pt.material_info()["updates"] == 2
        mats[FLOOR] = W.twosided(W.diffuse(W.bitmap(texels(5, 3, 42), filter=1)))
        _check(pt, mats, "accepted device update", sample=(FLOOR, 0))
    finally:
        pt.close_engine()


# ------------------------------------------------------------------ 8. memory
def test_repeated_reallocation_holds_no_memory():
    """20 alternating 5 x 3 <-> 8 x 8 updates: the free device memory stays within one allocation
    granule (read from what the first reallocation cost) of its value after the second update"""
    import torch

    mats = base_materials()
    mats[SPHERE] = W.twosided(W.diffuse(W.bitmap(texels(5, 3, 51), filter=1)))
    w = build_world(mats)
    pt = _pass(w)
    small = W.twosided(W.diffuse(W.bitmap(texels(5, 3, 51), filter=1)))
    large = W.twosided(W.diffuse(W.bitmap(texels(8, 8, 52), filter=1)))
    free = lambda: torch.cuda.mem_get_info(pt.device_index)[0]
    try:
        _render(pt, SPP)  # the ring and every lazily allocated buffer exist from here on
        f0 = free()
        _apply(pt, w, mats, {SPHERE: large})
        f1 = free()
        _apply(pt, w, mats, {SPHERE: small})
        f2 = free()
        granule = abs(f0 - f1)
        for k in range(20):
            _apply(pt, w, mats, {SPHERE: large if k % 2 == 0 else small})
        print(f"free after create {f0}, first reallocation {f1}, second {f2}, after 20 more {free()}; granule {granule}")
        assert abs(free() - f2) <= granule
        assert pt.material_info()["updates"] == 22
        _check(pt, mats, "after 22 reallocations", sample=(SPHERE, 0))
    finally:
        pt.close_engine()
