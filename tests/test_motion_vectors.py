"""Flow AOV of the engine (csrc/pt_flow.hip, pupil_pt_motion_vectors) against a float64 restatement:
pixel-centre rays built from the scene matrices in numpy, traced with pupil_pt_trace_rays (or
intersected analytically), then hit point, previous transform, previous projection and flow all in
float64.  TOL is 8 x the largest |flow_gpu - flow_float64| measured on an MI355X over the cases
below ("Flow AOV"); each test prints its own maximum before asserting."""
import os
import re
import tempfile

import numpy as np
import pytest

from pupiloptixlab_amd import World, abi, scenes
from pupiloptixlab_amd import world as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_TMPDIR = tempfile.TemporaryDirectory(prefix="pupil_test_scenes_")  # scene files written by these tests
TMP = _TMPDIR.name
pytestmark = pytest.mark.gpu

TOL = 8 * 3.13e-5  # pixels; 3.13e-5 = the measured maximum (the moved sphere; the Cornell cases reach 1.15e-5)
MAX_OUTLIERS = 2  # pixels per image whose ray grazes an edge differently in float32
WIDTH, HEIGHT = 64, 48


def _mat(v):
    return np.array(list(v), np.float64).reshape(4, 4)


def centre_rays(s2c, c2w, width, height):
    """(o, d) of the camera rays through the pixel centres, float64, pixel i = y * width + x."""
    yy, xx = np.mgrid[0:height, 0:width]
    film = np.stack([(xx + 0.5) / width, (yy + 0.5) / height, np.zeros_like(xx, float), np.ones_like(xx, float)], -1)
    d4 = film.reshape(-1, 4) @ s2c.T
    d = d4[:, :3] / d4[:, 3:4]
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d = d @ c2w[:3, :3].T
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    o = np.broadcast_to(c2w[:3, 3], d.shape)
    return o, d


def trace(pt, o, d):
    """closest hits of float32 rays through the production traversal: (t, prim) per ray (prim -1 = miss)."""
    n = len(o)
    r8 = np.zeros((n, 8), np.float32)
    r8[:, 0:3], r8[:, 3:6], r8[:, 6], r8[:, 7] = o, d, 0.001, 1e16
    out = np.zeros((n, 4), np.float32)
    abi.check(pt._lib.pupil_pt_trace_rays(pt._pt, n, r8.ctypes.data_as(abi.f32p), out.ctypes.data_as(abi.f32p), 0))
    prim = out[:, 3].copy().view(np.uint32).astype(np.int64)
    prim[prim == 0xFFFFFFFF] = -1
    return r8[:, 0:3].astype(np.float64), r8[:, 3:6].astype(np.float64), out[:, 0].astype(np.float64), prim


def flow_reference(o, d, t, hit, prev_s2c, prev_c2w, width, height, moved_by=None):
    """float64 flow and the previous homogeneous w; o, d (n, 3), t (n,), hit (n,) bool; moved_by
    (n, 3): how far each hit point has moved with its instance since the previous frame."""
    n = len(o)
    p = o + np.where(hit, t, 0.0)[:, None] * d
    if moved_by is not None:
        p = p - moved_by
    q = np.where(hit[:, None], np.concatenate([p, np.ones((n, 1))], 1), np.concatenate([d, np.zeros((n, 1))], 1))
    m = np.linalg.inv(prev_s2c) @ np.linalg.inv(prev_c2w)
    h = q @ m.T
    with np.errstate(divide="ignore", invalid="ignore"):
        u, v = h[:, 0] / h[:, 3] * width, h[:, 1] / h[:, 3] * height
    yy, xx = np.divmod(np.arange(n), width)
    return np.stack([xx + 0.5 - u, yy + 0.5 - v], 1), h[:, 3]


def gpu_flow(pt, prev_camera=None, prev_to_world=None):
    import torch

    mv = pt.motion_vectors(prev_camera, prev_to_world)
    torch.cuda.synchronize()
    return mv.cpu().numpy().astype(np.float64)


def compare(name, got, ref, mask, tol=None):
    """max |got - ref| over the masked pixels, printed; at most MAX_OUTLIERS above the tolerance."""
    tol = TOL if tol is None else tol
    err = np.abs(got[mask] - ref[mask]).max(-1)
    assert np.isfinite(got[mask]).all(), name
    order = np.sort(err)[::-1]
    worst_in = order[MAX_OUTLIERS] if len(order) > MAX_OUTLIERS else 0.0
    print(f"flow {name}: {mask.sum()} px, max err {order[0]:.3g} px, max without {MAX_OUTLIERS} outliers "
          f"{worst_in:.3g} px, max |flow| {np.abs(ref[mask]).max():.3g}")
    assert (err > tol).sum() <= MAX_OUTLIERS, (name, order[:5])
    return worst_in


def _pass(world):
    from pupiloptixlab_amd.pt_pass import PTPass

    pt = PTPass(device=0)
    pt.set_scene(world)
    return pt


def _cornell(open_back=False):
    path = scenes.cornell_xml(os.path.join(TMP, "cb_flow.xml"), WIDTH, HEIGHT, 4)
    if open_back:  # the same box without its back wall: the rays through it leave the scene
        text = open(path).read()
        text, k = re.subn(r'  <shape type="rectangle" id="BackWall">.*?</shape>\n', "", text, flags=re.S)
        assert k == 1
        path = os.path.join(TMP, "cb_flow_open.xml")
        open(path, "w").write(text)
    return World().load_scene(path)


def _rot_y(deg):
    return W.transform(rotate=((0, 1, 0), deg)).astype(np.float64)


def _camera_cases(c2w):
    t = c2w.copy()
    t[:3, 3] += [0.03, -0.02, 0.04]  # a few centimetres
    r = c2w.copy()
    r[:3, :3] = _rot_y(2.0)[:3, :3] @ c2w[:3, :3]
    return {"translate": t, "rotate": r}


@pytest.mark.parametrize("case", ["translate", "rotate"])
def test_cornell_camera_motion(case):
    w = _cornell()
    d = w.desc()
    s2c, c2w = _mat(d.sample_to_camera), _mat(d.camera_to_world)
    prev = _camera_cases(c2w)[case]
    pt = _pass(w)
    got = gpu_flow(pt, (s2c.astype(np.float32), prev.astype(np.float32)))
    o, dd = centre_rays(s2c, c2w, WIDTH, HEIGHT)
    o, dd, t, prim = trace(pt, o, dd)
    hit = prim >= 0
    assert hit.all()  # the closed box
    prev32 = prev.astype(np.float32).astype(np.float64)
    ref, hw = flow_reference(o, dd, t, hit, s2c, prev32, WIDTH, HEIGHT)
    assert (hw > 0).all() and np.abs(ref).max() > 0.5
    compare(case, got, ref, hit)
    pt.close_engine()


def test_cornell_behind_previous_camera():
    """The previous camera stood inside the box, past the front of the blocks: what lies behind its
    plane has no previous pixel (NaN), what lies in front has one."""
    w = _cornell()
    d = w.desc()
    s2c, c2w = _mat(d.sample_to_camera), _mat(d.camera_to_world)
    prev = c2w.copy()
    prev[:3, 3] = [0.0, 1.0, 0.3]
    pt = _pass(w)
    got = gpu_flow(pt, (s2c.astype(np.float32), prev.astype(np.float32)))
    o, dd = centre_rays(s2c, c2w, WIDTH, HEIGHT)
    o, dd, t, prim = trace(pt, o, dd)
    _, hw = flow_reference(o, dd, t, prim >= 0, s2c, prev, WIDTH, HEIGHT)
    behind, front = hw < -1e-3, hw > 1e-3
    assert behind.sum() > 50 and front.sum() > 50
    assert np.isnan(got[behind]).all()
    assert np.isfinite(got[front]).all()
    pt.close_engine()


@pytest.mark.parametrize("case", ["translate", "rotate"])
def test_open_box_environment(case):
    """Rays leaving through the missing back wall: the point at infinity (w = 0), so a camera
    translation gives no flow on the background and a rotation does."""
    w = _cornell(open_back=True)
    d = w.desc()
    s2c, c2w = _mat(d.sample_to_camera), _mat(d.camera_to_world)
    prev = _camera_cases(c2w)[case]
    pt = _pass(w)
    got = gpu_flow(pt, (s2c.astype(np.float32), prev.astype(np.float32)))
    o, dd = centre_rays(s2c, c2w, WIDTH, HEIGHT)
    o, dd, t, prim = trace(pt, o, dd)
    miss = prim < 0
    assert miss.sum() > 100
    ref, _ = flow_reference(o, dd, t, ~miss, s2c, prev.astype(np.float32).astype(np.float64), WIDTH, HEIGHT)
    compare("env " + case, got, ref, miss)
    compare("open " + case, got, ref, ~miss)
    if case == "translate":
        # the direction at infinity projects back onto its own pixel, up to the float32 rounding of the
        # traced direction: 2^-23 of a unit vector, times the film's pixels per radian at the image centre
        px_per_rad = WIDTH / (2 * np.tan(np.deg2rad(19.5) / 2))
        assert np.abs(ref[miss]).max() < px_per_rad * 2.0 ** -23
    else:
        assert np.abs(got[miss]).max(-1).min() > 1.0
    pt.close_engine()


@pytest.mark.parametrize("accel", ["flat", "two_level_object", "two_level_world"])
def test_identity_is_zero_flow(accel, monkeypatch):
    if accel != "flat":
        monkeypatch.setenv("PUPIL_ACCEL", "two_level")
        monkeypatch.setenv("PUPIL_TL_MODE", "object" if accel == "two_level_object" else "world")
    else:
        monkeypatch.setenv("PUPIL_ACCEL", "flat")
    w = _cornell()
    d = w.desc()
    s2c, c2w = _mat(d.sample_to_camera), _mat(d.camera_to_world)
    pt = _pass(w)
    assert pt.stats()["two_level"] == (0 if accel == "flat" else 1)
    got = gpu_flow(pt)  # no arguments: since the previous render = nothing moved
    compare("identity " + accel, got, np.zeros_like(got), np.ones(len(got), bool))
    # and the same flow as the flat build for a moved camera
    prev = _camera_cases(c2w)["rotate"]
    got = gpu_flow(pt, (s2c.astype(np.float32), prev.astype(np.float32)))
    o, dd = centre_rays(s2c, c2w, WIDTH, HEIGHT)
    o, dd, t, prim = trace(pt, o, dd)
    ref, _ = flow_reference(o, dd, t, prim >= 0, s2c, prev.astype(np.float32).astype(np.float64), WIDTH, HEIGHT)
    compare("rotate " + accel, got, ref, prim >= 0)
    pt.close_engine()


# ------------------------------------------------------------------ instance motion
CAM_Z, FOV = 5.0, 40.0


def _two_instances(right):
    """Camera at (0, 0, 5) looking down -z; left: a rectangle x in [-4, 0] in the plane z = 0;
    right: a rectangle x in [0, 4] in the same plane, or a sphere of radius 10 behind it."""
    w = World()
    w.set_film(WIDTH, HEIGHT, 2)
    w.set_sensor(FOV, W.look_at_mitsuba((0, 0, CAM_Z), (0, 0, 0), (0, 1, 0)), fov_axis="x")
    mat = w.add_material(W.diffuse((0.5, 0.5, 0.5), twosided=True))
    rect = w.add_builtin("rectangle")
    w.add_instance(rect, mat, W.transform(scale=(2, 2, 1), translate=(-2, 0, 0)))
    if right == "rectangle":
        m = W.transform(scale=(2, 2, 1), translate=(2, 0, 0))
        w.add_instance(rect, mat, m)
    else:
        m = W.transform(scale=(10, 10, 10), translate=(9.5, 0, -4))
        w.add_instance(w.add_builtin("sphere"), mat, m)
    w.add_instance(rect, mat, W.transform(scale=(0.1, 0.1, 1), translate=(0, 50, 0)),
                   emitter_radiance=W.rgb(1.0))  # a light out of view
    return w, m.astype(np.float64)


def _analytic_hits(o, d, right):
    """float64 nearest hits of the two instances: t and instance (0 left, 1 right, -1 none)."""
    t_plane = -o[:, 2] / d[:, 2]
    x = o[:, 0] + t_plane * d[:, 0]
    t = np.full(len(o), np.inf)
    inst = np.full(len(o), -1)
    left = (t_plane > 0) & (x < 0) & (x > -4)
    t[left], inst[left] = t_plane[left], 0
    if right == "rectangle":
        r = (t_plane > 0) & (x > 0) & (x < 4)
        t[r], inst[r] = t_plane[r], 1
    else:
        c, rad = np.array([9.5, 0.0, -4.0]), 10.0
        oc = o - c
        b = (oc * d).sum(1)
        disc = b * b - ((oc * oc).sum(1) - rad * rad)
        ts = -b - np.sqrt(np.maximum(disc, 0.0))
        r = (disc > 0) & (ts > 0) & (ts < t)
        t[r], inst[r] = ts[r], 1
    return t, inst


@pytest.mark.parametrize("right", ["rectangle", "sphere"])
def test_instance_motion(right):
    w, m_now = _two_instances(right)
    d = w.desc()
    s2c, c2w = _mat(d.sample_to_camera), _mat(d.camera_to_world)
    offset = np.array([0.11, -0.07, 0.0])  # in the rectangle's plane / sideways
    m_prev = m_now.copy()
    m_prev[:3, 3] -= offset
    prev_tw = np.array([list(d.instances[i].to_world) for i in range(d.num_instances)], np.float64).reshape(-1, 3, 4)
    prev_tw[1] = m_prev[:3]
    pt = _pass(w)
    got = gpu_flow(pt, (s2c.astype(np.float32), c2w.astype(np.float32)), prev_tw.astype(np.float32).reshape(-1, 12))
    o, dd = centre_rays(s2c, c2w, WIDTH, HEIGHT)
    t, inst = _analytic_hits(o, dd, right)  # float64 rays: nothing here comes from the GPU
    assert (inst >= 0).all()
    ref, _ = flow_reference(o, dd, t, inst >= 0, s2c, c2w, WIDTH, HEIGHT, moved_by=np.where((inst == 1)[:, None], offset, 0.0))
    cls = inst.reshape(HEIGHT, WIDTH)
    edge = np.zeros((HEIGHT, WIDTH), bool)  # within one column of the boundary between the instances
    edge[:, 1:] |= cls[:, 1:] != cls[:, :-1]
    edge[:, :-1] |= cls[:, 1:] != cls[:, :-1]
    assert edge.mean() <= 0.10 and edge.sum(1).max() <= 3
    keep = ~edge.reshape(-1)
    lm, rm = keep & (inst == 0), keep & (inst == 1)
    assert lm.sum() > 1000 and rm.sum() > 1000
    assert np.abs(ref[lm]).max() < 1e-9  # static camera, static instance
    # the moved instance: its points were `offset` further back along the move
    px_per_unit = WIDTH / (2 * CAM_Z * np.tan(np.deg2rad(FOV) / 2))
    if right == "rectangle":  # a plane parallel to the film: one flow for the whole instance
        assert np.allclose(np.abs(ref[rm]), np.abs(offset[:2]) * px_per_unit, rtol=1e-6)
    compare(f"instance {right} left", got, ref, lm)
    compare(f"instance {right} right", got, ref, rm)
    pt.close_engine()


@pytest.mark.parametrize("how", ["update_now", "event"])
def test_instance_motion_since_previous_render(how):
    """motion_vectors() with no arguments after an instance moved between two renders: the pass
    remembered the transforms of the render before.  A render without a move in between forgets
    them again, and an update that no render has used yet is refused."""
    import torch
    from pupiloptixlab_amd.pt_pass import Events

    w, m_now = _two_instances("rectangle")
    d = w.desc()
    s2c, c2w = _mat(d.sample_to_camera), _mat(d.camera_to_world)
    offset = np.array([0.11, -0.07, 0.0])
    pt = _pass(w)
    pt.render(1)
    m_new = m_now.copy()
    m_new[:3, 3] += offset
    w.set_instance_transform(1, m_new.astype(np.float32))
    if how == "update_now":
        pt.update_instance(w, 1)
        with pytest.raises(RuntimeError):
            pt.motion_vectors()  # the engine holds transforms no render has used
    else:
        pt.events.dispatch(Events.RENDER_INSTANCE_UPDATE, (w, 1))  # applied by the next render
    pt.render(1)
    got = gpu_flow(pt)
    o, dd = centre_rays(s2c, c2w, WIDTH, HEIGHT)
    t_plane = -o[:, 2] / dd[:, 2]
    x = o[:, 0] + t_plane * dd[:, 0]
    right = x > offset[0]  # the moved rectangle now spans x in [0.11, 4.11]
    left = x < 0
    ref, _ = flow_reference(o, dd, t_plane, np.ones(len(o), bool), s2c, c2w, WIDTH, HEIGHT,
                            moved_by=np.where(right[:, None], offset, 0.0))
    cls = np.where(left, 0, np.where(right, 1, -1)).reshape(HEIGHT, WIDTH)  # -1: the gap the move opened (1.9 px)
    edge = cls < 0
    edge[:, 1:] |= cls[:, 1:] != cls[:, :-1]
    edge[:, :-1] |= cls[:, 1:] != cls[:, :-1]
    keep = ~edge.reshape(-1)
    assert (~keep).mean() <= 0.10 and (keep & left).sum() > 1000 and (keep & right).sum() > 1000
    compare(f"since previous render ({how}) left", got, ref, keep & left)
    compare(f"since previous render ({how}) right", got, ref, keep & right)
    assert np.abs(ref[keep & right]).max() > 1.0
    pt.render(1)  # nothing moved between the last two renders
    torch.cuda.synchronize()
    got = gpu_flow(pt)
    compare(f"since previous render ({how}) static", got, np.zeros_like(got), keep)
    pt.close_engine()


# ------------------------------------------------------------------ tiling, side effects
def test_tiled_ranks_equal_full_image():
    import torch

    w = _cornell()
    d = w.desc()
    s2c, c2w = _mat(d.sample_to_camera), _mat(d.camera_to_world)
    cam = (s2c.astype(np.float32), _camera_cases(c2w)["rotate"].astype(np.float32))
    pt = _pass(w)
    full = pt.motion_vectors(cam).cpu().numpy().copy()
    stitched = np.full_like(full, np.inf)
    for rank in range(2):
        pt.set_tiling(32, rank, 2)
        part = pt.motion_vectors(cam)
        torch.cuda.synchronize()
        px = pt.local_pixels()
        assert part.shape[0] == len(px)
        stitched[px] = part.cpu().numpy()
    assert np.array_equal(stitched.view(np.uint32), full.view(np.uint32))
    pt.close_engine()


def test_flow_pass_has_no_side_effects():
    import torch

    w = _cornell()
    d = w.desc()
    s2c, c2w = _mat(d.sample_to_camera), _mat(d.camera_to_world)
    cam = (s2c.astype(np.float32), _camera_cases(c2w)["translate"].astype(np.float32))
    keys = ("pt accum buffer", "final result", "albedo", "normal", "test")

    def render(pt):
        pt.mark_dirty()
        pt.render(2)
        torch.cuda.synchronize()
        return {k: pt.buffers.get(k).cpu().numpy().copy() for k in keys}

    pt = _pass(w)
    before = render(pt)
    rays0 = pt.stats()["rays_traced_total"]
    pt.motion_vectors(cam)
    pt.motion_vectors()
    torch.cuda.synchronize()
    assert pt.stats()["rays_traced_total"] == rays0
    after = render(pt)
    for k in keys:
        assert np.array_equal(before[k].view(np.uint32), after[k].view(np.uint32)), k
    pt.close_engine()
