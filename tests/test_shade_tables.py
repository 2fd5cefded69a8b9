"""Block-resident scene tables of the shade kernels: each shade block copies the instance, material,
area-emitter (CDF, guide, env) and cull-set tables into its LDS when they are within their caps,
and reads a table over its cap from global memory, decided per table.  Only where the operands come
from differs, so every render here equals the CPU oracle bit for bit -- accum, albedo, normal, test
and the three ray counts -- with every table resident, with each table one entry over its cap and
exactly at it, after in-place updates, and when the shade grid's last stride is partial.  The caps
come from the library (pupil_debug_shade_tables), so the scenes follow a later change of them.

All scenes are 64 x 64 (one 72 x 72) at 2-4 spp and run through the stage kernels
(PUPIL_FRAME_PATHS=0): the one-launch frame kernel keeps the global tables."""
import ctypes as C

import numpy as np
import pytest

import oracle
from pupiloptixlab_amd import abi
from pupiloptixlab_amd import world as W

gpu = pytest.mark.gpu
BUFS = (("pt accum buffer", "accum"), ("albedo", "albedo"), ("normal", "normal"), ("test", "test"))
RAYS = ("primary_rays", "extension_rays", "shadow_rays")
INST, MAT, AREA, CULL = 1, 2, 4, 8  # bits of the fit mask
ALL = INST | MAT | AREA | CULL
ROOM = 6  # instances of the empty room: five walls and the ceiling


def caps():
    c = (C.c_uint32 * 4)()
    abi.check(abi.load_library().pupil_debug_shade_tables(None, c, None))
    return tuple(c)


def test_caps_are_exported_and_fit_five_blocks():
    inst, mat, area, cull = caps()
    assert min(inst, mat, area, cull) >= 1
    # the layout of pt_shade.h: 224-B instances, 352-B materials, 328-B emitters (+ the env), CDF, guide,
    # 2 x 48 B per cull entry, each part 16-B aligned, in 512-B granules, five blocks in a CU's 160 KB
    up = lambda x, a: (x + a - 1) // a * a  # noqa: E731
    size = inst * 224 + mat * 352 + up((area + 1) * 328, 16) + area * 4 + up((area + 1) * 4, 16) + cull * 96
    assert 5 * up(size, 512) <= 160 * 1024
    assert abi.load_library().pupil_debug_shade_tables(None, None, C.byref(C.c_uint32())) == abi.ERR_INVALID


# ------------------------------------------------------------------ scenes
def room(res=64, depth=4, instances=ROOM + 1, quads=1, mixed=False, radiance=(30.0, 28.0, 24.0)):
    """A closed 4 x 4 x 4 room seen from inside: `quads` square lights (two emissive triangles each)
    under the ceiling and small plates above the floor up to `instances` instances in all (the world
    keeps one material per instance).  mixed: the plates take the seven BSDF types in turn, one has
    a checkerboard reflectance, and the first light's radiance is a checkerboard."""
    wd = W.World()
    wd.set_film(res, res, depth)
    rect = wd.add_builtin("rectangle")
    grey = lambda: wd.add_material(W.twosided(W.diffuse((0.7, 0.6, 0.5))))  # noqa: E731
    for sc, rot, tr in [((2, 2, 1), ((1, 0, 0), -90), (0, 0, 0)), ((2, 2, 1), None, (0, 2, -2)),
                        ((2, 2, 1), ((0, 1, 0), 180), (0, 2, 2)), ((2, 2, 1), ((0, 1, 0), 90), (-2, 2, 0)),
                        ((2, 2, 1), ((0, 1, 0), -90), (2, 2, 0)), ((2, 2, 1), ((1, 0, 0), 90), (0, 4, 0))]:
        wd.add_instance(rect, grey(), W.transform(scale=sc, rotate=rot, translate=tr))
    wd.lights = []
    for k in range(quads):
        x, z = -1.5 + 0.75 * (k % 5), -1.0 + 0.9 * (k // 5)
        rad = (radiance[0] - k, radiance[1], radiance[2] + k)
        if mixed and k == 0:
            rad = W.checkerboard((40.0, 10.0, 5.0), (5.0, 10.0, 40.0), (4.0, 4.0))
        wd.lights.append(wd.add_instance(rect, wd.add_material(W.twosided(W.diffuse((0.0, 0.0, 0.0)))),
                                         W.transform(scale=(0.25, 0.25, 1), rotate=((1, 0, 0), 90),
                                                     translate=(x, 3.9 - 0.01 * k, z)), emitter_radiance=rad))
    kinds = [lambda: W.twosided(W.diffuse(W.checkerboard((0.8, 0.2, 0.2), (0.2, 0.2, 0.8), (3.0, 3.0)))),
             W.dielectric, W.rough_dielectric, lambda: W.twosided(W.conductor()),
             lambda: W.twosided(W.rough_conductor()), lambda: W.twosided(W.plastic()),
             lambda: W.twosided(W.rough_plastic())]
    wd.plates = []
    for k in range(instances - ROOM - quads):
        x, z = -1.6 + 0.46 * (k % 8), -1.5 + 0.5 * (k // 8)
        m = wd.add_material(kinds[k % 7]()) if mixed else grey()
        wd.plates.append(wd.add_instance(rect, m, W.transform(scale=(0.2, 0.2, 1), rotate=((1, 0, 0), -90 + 7 * (k % 5)),
                                                              translate=(x, 0.3 + 0.05 * (k % 7), z))))
    wd.set_sensor(60.0, W.look_at_mitsuba((0.0, 2.0, 1.9), (0.0, 1.9, 0.0), (0, 1, 0)), fov_axis="y")
    assert wd.desc().num_instances == instances
    return wd


def new_pass(w):
    from pupiloptixlab_amd.pt_pass import PTPass

    pt = PTPass(device=0)
    pt.set_scene(w)
    pt.dirty = False
    pt.random_seed, pt.sample_cnt = 0, 0
    return pt


def fit_of(pt):
    f = C.c_uint32()
    abi.check(pt._lib.pupil_debug_shade_tables(pt._pt, None, C.byref(f)))
    return f.value


def grab(pt):
    import torch

    torch.cuda.synchronize()
    out = {k: pt.buffers.get(k).cpu().numpy().copy() for k, _ in BUFS}
    out["stats"] = pt.stats()
    return out


def check(w, spp, name, fit):
    """One render(spp) of `w` against the oracle, bit for bit; `fit`: the tables expected in LDS."""
    pt = new_pass(w)
    try:
        assert fit_of(pt) == fit, (name, fit_of(pt))
        pt.render(spp, collect_stats=True)
        got = grab(pt)
    finally:
        pt.close_engine()
    ref = oracle.OracleScene(w.desc()).render(spp=spp)
    for gk, rk in BUFS:
        g, r = np.asarray(got[gk]).reshape(-1), np.asarray(ref[rk]).reshape(-1)
        assert np.array_equal(g.view(np.uint32), r.view(np.uint32)), f"{name}: {gk} differs from the oracle"
    assert tuple(got["stats"][k] for k in RAYS) == tuple(ref["stats"][k] for k in RAYS), name
    return got


@pytest.fixture(autouse=True)
def stage_kernels(monkeypatch):
    monkeypatch.setenv("PUPIL_FRAME_PATHS", "0")


# ------------------------------------------------------------------ every table resident
@gpu
@pytest.mark.parametrize("accel", ["flat", "two_level"])
def test_single_material_all_resident(accel, monkeypatch):
    monkeypatch.setenv("PUPIL_ACCEL", accel)
    got = check(room(instances=12), 3, f"single-{accel}", ALL)
    if accel == "flat":
        assert got["stats"]["terminal_rays_culled"] > 0  # the cull set's LDS records were read


@gpu
def test_seven_bsdfs_textured_emitter_bins():
    check(room(instances=ROOM + 2 + 14, quads=2, mixed=True), 3, "mixed", ALL)


# ------------------------------------------------------------------ one over each cap, and exactly at it
@gpu
def test_materials_one_over_cap():
    inst, mat, _, _ = caps()
    assert mat < inst, "the world keeps a material per instance: only then can the materials alone be over"
    check(room(instances=mat + 1), 2, "materials+1", ALL & ~MAT)


@gpu
def test_instances_one_over_cap():
    inst, mat, _, _ = caps()
    check(room(instances=inst + 1), 2, "instances+1", ALL & ~INST & (ALL if mat > inst else ~MAT))


@gpu
def test_instances_and_materials_at_cap():
    inst, mat, _, _ = caps()
    check(room(instances=mat), 2, "materials=cap", ALL)
    check(room(instances=inst), 2, "instances=cap", ALL if mat >= inst else ALL & ~MAT)


@gpu
def test_mixed_materials_over_cap_bins():
    _, mat, _, _ = caps()
    check(room(instances=mat + 1, quads=2, mixed=True), 2, "mixed materials+1", ALL & ~MAT)


@gpu
def test_area_emitters_over_and_at_cap():
    """An emissive mesh's worth of emitters: two per quad.  More emissive primitives than the cull
    set's default size means no set, which counts as fitting."""
    _, _, area, _ = caps()
    over = area // 2 + 1
    check(room(instances=ROOM + over + 2, quads=over), 2, "areas+", ALL & ~AREA)
    check(room(instances=ROOM + area // 2 + 2, quads=area // 2), 2, "areas=cap", ALL)


@gpu
def test_cull_set_over_and_at_cap(monkeypatch):
    _, _, area, cull = caps()
    monkeypatch.setenv("PUPIL_TERMINAL_CULL_K", "32")  # read when the engine is created
    over = cull // 2 + 1
    assert 2 * over <= area, "the cull set alone is over its cap"
    got = check(room(instances=ROOM + over + 2, quads=over), 2, "cull+", ALL & ~CULL)
    assert got["stats"]["terminal_rays_culled"] > 0
    got = check(room(instances=ROOM + cull // 2 + 2, quads=cull // 2), 2, "cull=cap", ALL)
    assert got["stats"]["terminal_rays_culled"] > 0


# ------------------------------------------------------------------ updates are seen by the next launch
def _edit(w):
    """A plate's colour and the light's transform, on the world."""
    w.set_material(w.desc().instances[w.plates[0]].material, W.twosided(W.diffuse((0.1, 0.8, 0.3))))
    w.set_instance_transform(w.lights[0], W.transform(scale=(0.4, 0.3, 1), rotate=((1, 0, 0), 90),
                                                      translate=(0.6, 3.7, -0.4)))


@gpu
def test_in_place_updates_between_progressive_renders():
    """A material colour, the transform of the emissive instance and its radiance change between
    two renders of one engine: the second render equals a fresh engine's of the edited scene (and
    the oracle's).  The world has no setter for an instance's radiance, so the new emitter table
    comes from a second world that differs in nothing else."""
    w = room(instances=12)
    edited = room(instances=12, radiance=(5.0, 40.0, 9.0))
    _edit(edited)
    pt = new_pass(w)
    try:
        pt.render(2, continues=True)
        grab(pt)
        _edit(w)
        pt.update_material(w, w.desc().instances[w.plates[0]].material)
        pt.update_instance(w, w.lights[0])
        d = edited.desc()
        abi.check(pt._lib.pupil_pt_update_emitters(pt._pt, C.byref(d)))
        pt.dirty = False
        pt.random_seed, pt.sample_cnt = 0, 0
        pt.render(3, collect_stats=True)
        got = grab(pt)
    finally:
        pt.close_engine()
    fresh = check(edited, 3, "fresh engine of the edited scene", ALL)
    plain = check(room(instances=12), 3, "the scene before the edits", ALL)
    assert not np.array_equal(plain["pt accum buffer"], got["pt accum buffer"]), "the edits changed nothing"
    for gk, _ in BUFS:
        assert np.array_equal(np.asarray(got[gk]).view(np.uint32), np.asarray(fresh[gk]).view(np.uint32)), gk
    assert tuple(got["stats"][k] for k in RAYS) == tuple(fresh["stats"][k] for k in RAYS)


# ------------------------------------------------------------------ the grid-stride loop
@gpu
@pytest.mark.parametrize("res,spp", [(64, 3), (72, 4)])
def test_partial_last_stride(res, spp, monkeypatch):
    """64 blocks of 256 threads (the smallest grid): 64 x 64 x 3 paths leave whole blocks without a
    path; 72 x 72 x 4 = 20736 paths take a second, partial stride, and the lists of the later bounces
    end inside a block."""
    monkeypatch.setenv("PUPIL_SHADE_MAX_BLOCKS", "64")  # read when the engine is created
    assert (res * res * spp < 64 * 256) == (res == 64)
    check(room(res=res, instances=12), spp, f"stride-{res}", ALL)
    check(room(res=res, instances=ROOM + 2 + 7, quads=2, mixed=True), spp, f"stride-mixed-{res}", ALL)
