"""Point, spot and directional lights on the GPU: closed forms of the direct term along rays
(PTPass.radiance, so nothing depends on film jitter), shadows, the reference's emitter selection,
the sampling probe, updates against a fresh engine, the engine-owned emitter table, the
terminal-ray cull and a render.  Scenes, the float64 restatements and the tolerance (RTOL, with
its derivation) are in delta_light_cases.py."""
import ctypes as C

import numpy as np
import pytest

import delta_light_cases as dc
from pupiloptixlab_amd import abi
from pupiloptixlab_amd import world as W

pytestmark = pytest.mark.gpu
f32 = np.float32
RAYS = dc.rays_down()
# with the occluder in the scene a ray from y = 2 would stop on it: those rays start under it, at
# y = 0.5, and reach the same 64 floor points
RAYS_UNDER = dc.rays_down(height=0.5)
POINT = dc.point_expect()  # (64, 3) float64: test 1's closed form, shared


def _pass(w):
    from pupiloptixlab_amd.pt_pass import PTPass

    pt = PTPass(device=0)
    pt.set_scene(w)
    return pt


def _radiance(pt, spp=1, seed=0, accumulate=False, rays=RAYS):
    import torch

    out = pt.radiance(torch.from_numpy(rays).to(pt.device), spp=spp, seed=seed, accumulate=accumulate)["radiance"]
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _err(got, exp):
    """Largest |got - exp| / |exp| (exp > 0)."""
    return float(np.max(np.abs(got.astype(np.float64) - exp) / np.abs(exp)))


def _point_world(**kw):
    w = dc.floor_world(**kw)
    w.add_point_light(tuple(dc.POINT_POS), tuple(dc.POINT_I))
    return w


# ------------------------------------------------------------------ 1. point light, closed form
def test_point_light_closed_form():
    pt = _pass(_point_world())
    try:
        one = _radiance(pt)
        four = _radiance(pt, spp=4, accumulate=True)
    finally:
        pt.close_engine()
    print("point: max rel err", _err(one[:, :3], POINT), "spp 4:", _err(four[:, :3], POINT))
    assert np.all(one[:, 3] == 1.0) and np.all(four[:, 3] == 1.0)
    assert _err(one[:, :3], POINT) <= dc.RTOL
    assert _err(four[:, :3], POINT) <= dc.RTOL  # a delta light adds no variance here


# ------------------------------------------------------------------ 2. shadow
def test_point_light_shadow():
    centre = (dc.POINT_POS[0], dc.POINT_POS[2])
    # the light is at y = 1.5 and the occluder at y = 0.75: every segment crosses its plane half way
    t = dc.OCC_Y / dc.POINT_POS[1]
    cross = (dc.POINTS + t * (dc.POINT_POS - dc.POINTS))[:, [0, 2]]
    dark, lit, left_out = dc.shadow_classes(cross, centre)
    assert dark.sum() > 0 and lit.sum() > 0 and left_out.sum() <= len(dc.POINTS) // 4
    pt = _pass(_point_world(occluder=centre))
    try:
        got = _radiance(pt, rays=RAYS_UNDER)[:, :3]
    finally:
        pt.close_engine()
    print("shadow: dark", dark.sum(), "lit", lit.sum(), "left out", left_out.sum(), "err", _err(got[lit], POINT[lit]))
    assert np.all(got[dark] == 0.0)
    assert _err(got[lit], POINT[lit]) <= dc.RTOL


# ------------------------------------------------------------------ 3. spot
def _spot_world(cutoff, beam):
    w = dc.floor_world()
    w.add_spot_light(tuple(dc.POINT_POS), tuple(dc.SPOT_AXIS), tuple(dc.POINT_I), cutoff_deg=cutoff, beam_deg=beam)
    return w


def test_spot_light_falloff():
    a = dc.spot_angle(dc.POINT_POS, dc.SPOT_AXIS, dc.POINTS)
    cutoff, beam = np.deg2rad(dc.SPOT_CUTOFF), np.deg2rad(dc.SPOT_BEAM)
    fall = dc.spot_falloff(a, cutoff, beam)
    plateau, outside = a < np.deg2rad(19.0), a > np.deg2rad(36.0)
    trans = (fall >= 0.1) & (fall <= 0.9)
    assert plateau.sum() > 0 and outside.sum() > 0 and trans.sum() >= 8, (plateau.sum(), outside.sum(), trans.sum())
    pt = _pass(_spot_world(dc.SPOT_CUTOFF, dc.SPOT_BEAM))
    try:
        got = _radiance(pt)[:, :3].astype(np.float64)
    finally:
        pt.close_engine()
    assert _err(got[plateau], POINT[plateau]) <= dc.RTOL
    assert np.all(got[outside] == 0.0)
    # In the transition the falloff is (cutoff - a) / (cutoff - beam) with a = dm_acos(..), which
    # tests/test_detmath.py pins to 4 ulp of its float32 result: an absolute error of the angle of
    # 4 * spacing(a), so of the falloff 4 * spacing(a) / (cutoff - beam), on top of RTOL of the value.
    acos_err = 4.0 * np.spacing(a.astype(f32)).astype(np.float64)
    exp = POINT * fall[:, None]
    tol = dc.RTOL * exp + (acos_err / (cutoff - beam))[:, None] * POINT
    excess = np.abs(got - exp)[trans] / tol[trans]
    print("spot: plateau err", _err(got[plateau], POINT[plateau]), "transition points", trans.sum(),
          "worst |err| / tol", excess.max())
    assert np.all(np.abs(got - exp)[trans] <= tol[trans])


def test_spot_light_hard_edge():
    a = dc.spot_angle(dc.POINT_POS, dc.SPOT_AXIS, dc.POINTS)
    edge = np.deg2rad(25.0)
    pt = _pass(_spot_world(25.0, 25.0))  # beam == cutoff
    try:
        got = _radiance(pt)[:, :3]
    finally:
        pt.close_engine()
    assert np.all(np.isfinite(got))
    inside, outside = a < edge - 1e-5, a > edge + 1e-5  # 1e-5 rad: far above the angle's float32 error
    assert inside.sum() > 0 and outside.sum() > 0 and (inside | outside).all()
    assert _err(got[inside], POINT[inside]) <= dc.RTOL and np.all(got[outside] == 0.0)


# ------------------------------------------------------------------ 4. directional
def test_directional_light():
    exp = dc.dir_expect()
    # the shadow is displaced along the direction of travel: back along it from the floor to y = 0.75
    cross = (dc.POINTS - dc.DIR_D * (dc.OCC_Y / -dc.DIR_D[1]))[:, [0, 2]]
    centre = (dc.POINT_POS[0], dc.POINT_POS[2])
    dark, lit, left_out = dc.shadow_classes(cross, centre)
    assert dark.sum() > 0 and lit.sum() > 0 and left_out.sum() <= len(dc.POINTS) // 4
    got = {}
    for name, occ, d in (("open", None, dc.DIR_D), ("occluded", centre, dc.DIR_D), ("up", None, -dc.DIR_D)):
        w = dc.floor_world(occluder=occ)
        w.add_directional_light(tuple(d), tuple(dc.DIR_E))
        pt = _pass(w)
        try:
            got[name] = _radiance(pt, rays=RAYS_UNDER if occ else RAYS)[:, :3]
        finally:
            pt.close_engine()
    print("directional: err", _err(got["open"], exp), "dark", dark.sum(), "left out", left_out.sum())
    assert _err(got["open"], exp) <= dc.RTOL
    assert np.all(got["occluded"][dark] == 0.0) and _err(got["occluded"][lit], exp[lit]) <= dc.RTOL
    assert np.all(got["up"] == 0.0)


# ------------------------------------------------------------------ 5. selection
def _picks(pt, p):
    p = np.ascontiguousarray(p, f32)
    out = np.zeros(len(p), np.int32)
    abi.check(pt._lib.pupil_debug_select_emitter(pt._pt, len(p), p.ctypes.data_as(abi.f32p),
                                                 out.ctypes.data_as(C.POINTER(C.c_int32))))
    return out


def test_two_point_lights_selection():
    pos2, int2 = np.array([-0.8, 1.0, 0.6]), np.array([4.0, 9.0, 5.0])
    w = dc.floor_world()
    w.add_point_light(tuple(dc.POINT_POS), tuple(dc.POINT_I))
    w.add_point_light(tuple(pos2), tuple(int2))
    l1, l2 = 2.0 * POINT, 2.0 * dc.point_expect(pos=pos2, intensity=int2)  # select_probability = 1/2 divides
    pt = _pass(w)
    try:
        first = second = 0
        for seed in range(64):
            got = _radiance(pt, seed=seed)[:, :3].astype(np.float64)
            is1 = np.all(np.abs(got - l1) <= dc.RTOL * l1, axis=1)
            is2 = np.all(np.abs(got - l2) <= dc.RTOL * l2, axis=1)
            assert np.all(is1 | is2), seed
            first, second = first + is1.sum(), second + is2.sum()
        assert first > 0 and second > 0
        table = pt.emitter_table()
        assert np.array_equal(table["select_probability"], f32([0.5, 0.5]))
        p = np.random.default_rng(5).random(4096, dtype=f32)
        assert np.array_equal(_picks(pt, p), dc.select_scan(table["select_probability"], p, False))
    finally:
        pt.close_engine()
    print("two lights: picks", first, second)


def test_selection_with_area_point_directional_and_env():
    w = dc.floor_world()
    w.add_instance(0, 0, W.transform(scale=(0.5, 0.5, 1), rotate=((1, 0, 0), 90), translate=(0, 3, 0)),
                   emitter_radiance=(4.0, 4.0, 4.0))
    w.add_directional_light(tuple(dc.DIR_D), tuple(dc.DIR_E))
    w.add_point_light(tuple(dc.POINT_POS), tuple(dc.POINT_I))
    w.add_const_env((0.2, 0.3, 0.4))
    pt = _pass(w)
    try:
        table = pt.emitter_table()
        assert list(table["type"]) == [abi.EMITTER_TRI_AREA, abi.EMITTER_TRI_AREA, abi.EMITTER_POINT,
                                       abi.EMITTER_DIRECTIONAL]  # five emitters with the env
        sp = table["select_probability"]
        cdf = np.zeros(4, f32)
        s = f32(0.0)
        for i in range(4):
            s = f32(s + sp[i])
            cdf[i] = s
        assert np.array_equal(dc.bits(table["cdf"]), dc.bits(cdf))  # accumulated over the whole table, in order
        p = np.concatenate([np.random.default_rng(6).random(4096, dtype=f32), f32([0.0, 1.0 - 2.0 ** -24]), cdf,
                            np.nextafter(cdf, f32(0.0)), np.nextafter(cdf, f32(2.0))])
        p = p[p < 1.0]
        ref = dc.select_scan(sp, p, True)
        assert np.array_equal(_picks(pt, p), ref)
        assert set(ref.tolist()) == {0, 1, 2, 3, -1}
        # a delta entry as pupil_debug_read_emitters shows it
        assert np.array_equal(table["pos"][2], f32([dc.POINT_POS, dc.POINT_I, (0, 0, 0)])) and table["area"][2] == 0
        assert np.allclose(table["nrm"][3][0], dc.DIR_D, rtol=0, atol=1e-7) and table["area"][3] == 0
    finally:
        pt.close_engine()


# ------------------------------------------------------------------ 6. the sampling probe
def test_emitter_sample_probe():
    w = dc.floor_world()
    w.add_point_light(tuple(dc.POINT_POS), tuple(dc.POINT_I))
    w.add_spot_light(tuple(dc.POINT_POS), tuple(dc.SPOT_AXIS), tuple(dc.POINT_I), dc.SPOT_CUTOFF, dc.SPOT_BEAM)
    w.add_directional_light(tuple(dc.DIR_D), tuple(dc.DIR_E))
    rng = np.random.default_rng(11)
    pts = np.column_stack([rng.uniform(-1.4, 1.4, 32), rng.uniform(-0.5, 0.5, 32), rng.uniform(-1.4, 1.4, 32)])
    nrm = rng.normal(size=(32, 3))
    nrm /= np.linalg.norm(nrm, axis=1)[:, None]
    pts, nrm = pts.astype(f32).astype(np.float64), nrm.astype(f32).astype(np.float64)
    wi, dist, rad = dc.point_sample(dc.POINT_POS, dc.POINT_I, pts)
    assert ((wi * nrm).sum(1) <= 0).sum() > 0  # NoL <= 0 is among them: the sample is still returned
    a = dc.spot_angle(dc.POINT_POS, dc.SPOT_AXIS, pts)
    cutoff, beam = np.deg2rad(dc.SPOT_CUTOFF), np.deg2rad(dc.SPOT_BEAM)
    fall = dc.spot_falloff(a, cutoff, beam)
    spot_tol = dc.RTOL * rad * fall[:, None] + (4.0 * np.spacing(a.astype(f32)) / (cutoff - beam))[:, None] * rad
    pt = _pass(w)
    try:
        assert pt._lib.pupil_debug_emitter_sample(pt._pt, 3, 0, None, None, None) == abi.ERR_INVALID  # no env
        xi = rng.random((1, 2), dtype=f32)
        for k in range(32):
            p = pt.emitter_sample(0, xi, pts[k], nrm[k])
            s = pt.emitter_sample(1, xi, pts[k], nrm[k])
            d = pt.emitter_sample(2, xi, pts[k], nrm[k])
            for r in (p, s, d):
                assert r["pdf"][0] == 1.0
            for r in (p, s):
                assert np.all(np.abs(r["wi"][0] - wi[k]) <= dc.RTOL)
                assert abs(r["distance"][0] - dist[k]) <= dc.RTOL * dist[k]
            assert np.all(np.abs(p["radiance"][0] - rad[k]) <= dc.RTOL * rad[k])
            assert np.all(np.abs(s["radiance"][0] - rad[k] * fall[k]) <= spot_tol[k]), (k, a[k])
            assert np.all(np.abs(d["wi"][0] + dc.DIR_D) <= dc.RTOL) and d["distance"][0] == f32(1e16)
            assert np.all(np.abs(d["radiance"][0] - dc.DIR_E) <= dc.RTOL * dc.DIR_E)
    finally:
        pt.close_engine()


# ------------------------------------------------------------------ 7. updates equal a fresh engine
def test_light_updates_equal_a_fresh_engine():
    w = dc.floor_world()
    w.add_point_light(tuple(dc.POINT_POS), tuple(dc.POINT_I))
    w.add_spot_light((-0.5, 1.2, 0.4), tuple(dc.SPOT_AXIS), (5.0, 6.0, 7.0), dc.SPOT_CUTOFF, dc.SPOT_BEAM)
    pt = _pass(w)
    try:
        before = _radiance(pt, seed=3)
        steps = (("move the point", lambda: w.set_light(0, position=(-0.2, 1.1, 0.5))),
                 ("spot angles", lambda: w.set_light(1, cutoff_deg=50, beam_deg=30)),
                 ("add a directional", lambda: w.add_directional_light(tuple(dc.DIR_D), tuple(dc.DIR_E))))
        for name, change in steps:
            change()
            pt.update_lights()
            got = _radiance(pt, seed=3)
            fresh = _pass(w)  # a new engine on the same world
            try:
                ref = _radiance(fresh, seed=3)
                ref_table = fresh.emitter_table()
            finally:
                fresh.close_engine()
            assert np.array_equal(dc.bits(got), dc.bits(ref)), name
            assert not np.array_equal(dc.bits(got), dc.bits(before)), name  # the change is visible
            table = pt.emitter_table()
            for key in ("select_probability", "cdf", "type", "pos", "nrm"):
                assert np.array_equal(np.asarray(table[key]).view(np.uint32), np.asarray(ref_table[key]).view(np.uint32)), (name, key)
            before = got
    finally:
        pt.close_engine()


# ------------------------------------------------------------------ 8. engine-owned emitter table
def test_device_emitter_table_with_delta_lights():
    import torch

    w = dc.floor_world()
    lamp = w.add_instance(0, 0, W.transform(scale=(0.5, 0.5, 1), rotate=((1, 0, 0), 90), translate=(0, 3, 0)),
                          emitter_radiance=(4.0, 5.0, 6.0))
    w.add_point_light(tuple(dc.POINT_POS), tuple(dc.POINT_I))
    w.add_directional_light(tuple(dc.DIR_D), tuple(dc.DIR_E))
    pt = _pass(w)
    try:
        pt.device_emitters = True
        assert pt.device_emitters
        start = pt.emitter_table()
        w.set_instance_transform(lamp, W.transform(scale=(0.7, 0.3, 1), rotate=((1, 0.2, 0), 75), translate=(0.4, 2.5, -0.3)))
        d = w.desc()
        tw = torch.tensor([list(d.instances[lamp].to_world)], dtype=torch.float32, device=pt.device)
        to = torch.tensor([list(d.instances[lamp].to_object)], dtype=torch.float32, device=pt.device)
        ids = torch.tensor([lamp], dtype=torch.int32, device=pt.device)
        pt.update_instances_device(tw, ids, to)
        assert pt.device_emitters
        got = pt.emitter_table()
        fresh = _pass(w)
        try:
            ref = fresh.emitter_table()
        finally:
            fresh.close_engine()
    finally:
        pt.close_engine()
    assert list(got["type"]) == [abi.EMITTER_TRI_AREA, abi.EMITTER_TRI_AREA, abi.EMITTER_POINT, abi.EMITTER_DIRECTIONAL]
    assert not np.array_equal(got["pos"][:2], start["pos"][:2])
    for key in ("select_probability", "area", "cdf", "type", "pos", "nrm"):
        assert np.array_equal(np.asarray(got[key]).view(np.uint32), np.asarray(ref[key]).view(np.uint32)), key
    assert got["guide_bits"] == ref["guide_bits"] and np.array_equal(got["guide"], ref["guide"])


# ------------------------------------------------------------------ 9. terminal-ray cull
@pytest.mark.parametrize("lamp", [False, True])
def test_terminal_cull_with_delta_lights(lamp, monkeypatch):
    import torch

    out = {}
    for knob in ("1", "0"):
        monkeypatch.setenv("PUPIL_TERMINAL_CULL", knob)  # read when the engine is created
        pt = _pass(dc.box_world(lamp=lamp))
        try:
            pt.render(4)
            torch.cuda.synchronize()
            out[knob] = (pt.image("pt accum buffer").copy(), pt.stats()["terminal_rays_culled"])
        finally:
            pt.close_engine()
    assert np.array_equal(dc.bits(out["1"][0]), dc.bits(out["0"][0]))
    assert out["1"][0][..., :3].max() > 0
    assert out["0"][1] == 0  # the knob is off: an engine that never had a set
    # a scene lit by delta lights alone has no emissive primitive, so no cull set: nothing is culled;
    # with the lamp the set is the lamp's two triangles, and terminal rays that miss them are culled
    assert (out["1"][1] > 0) == lamp, out["1"][1]


# ------------------------------------------------------------------ 10. a render sees the lights
def test_render_sees_the_point_light():
    import torch

    pt = _pass(_point_world(film=(32, 32), cam_height=3.0))  # the floor fills the image
    try:
        pt.render(16)
        torch.cuda.synchronize()
        img = pt.image("pt accum buffer").reshape(-1, 4)[:, :3].astype(np.float64)
        hits = pt.primary_hits(want=("instance", "position"))
        torch.cuda.synchronize()
        centres = hits["position"].cpu().numpy().astype(np.float64)
        assert np.all(hits["instance"].cpu().numpy() == 0)
    finally:
        pt.close_engine()
    exp = dc.point_expect(p=centres)
    # Film jitter moves a hit by at most half a pixel, 0.054 along each axis here (the image spans
    # 2 * 3 tan 30 = 3.46 over 32 pixels).  f = h / (h^2 + r^2)^(3/2) with h = 1.5 has |grad f| / f =
    # 3 r / (h^2 + r^2) <= 3 / (2 h) = 1: one sample is within 1 * 0.054 * sqrt 2 = 7.7 % of its
    # pixel centre's value, with zero mean to first order, so the mean of 32 * 32 * 16 samples is within
    # 7.7 % / sqrt(16384) = 0.06 % (one sigma); the second-order term is below 0.5 * 6 / h^2 *
    # 2 * 0.054^2 / 3 = 0.3 %.  Together far inside the 2 % asked for, which stays.
    rel = abs(img.mean() - exp.mean()) / exp.mean()
    print("render: mean", img.mean(), "closed form", exp.mean(), "rel", rel)
    assert rel <= 0.02
    assert np.all(img.sum(axis=1) > 0)
