"""Flow for deforming meshes (pupil_pt_snapshot_shape_vertices, PTPass.update_shape(keep_previous=True))
against a float64 restatement with nothing taken from the GPU: pixel-centre rays from the scene
matrices, Moeller-Trumbore against every current triangle in numpy, the float64 barycentrics
applied to the PREVIOUS vertices, the previous instance transform, the previous camera.

TOL is 8 x MEASURED, the largest |flow_gpu - flow_float64| measured on an MI355X over the
reference cases below (1-4, 6 and 7): 1.09e-5 px, on the partly static mesh (the deformation alone
reaches 9.71e-6, with the instance and the camera moved 1.06e-5, the shared shape 1.03e-5; see
DESIGN.md, "Flow AOV").  No pixel of any case was above the tolerance.  Each test prints its own
maximum before asserting.  The bit-identity cases take no tolerance."""
import ctypes as C
import functools

import numpy as np
import pytest

from pupiloptixlab_amd import World, abi
from pupiloptixlab_amd import world as W
from test_motion_vectors import _camera_cases, _mat, centre_rays, compare, flow_reference, gpu_flow, trace

pytestmark = pytest.mark.gpu

MEASURED = 1.09e-5  # pixels
TOL = 8 * MEASURED
WIDTH, HEIGHT = 60, 44  # 2640 pixels: no multiple of the 256-lane block
CAM_Z, FOV = 5.0, 40.0
N = 9  # vertices per side of the grid
OFFSET = (0.11, -0.07, 0.0)  # the instance move of the cases that have one
KEYS = ("pt accum buffer", "final result", "albedo", "normal", "test")


# ------------------------------------------------------------------ scene
def grid():
    """9 x 9 vertices over [-3, 3]^2 at z = 0, 128 triangles, normals +z."""
    c = np.linspace(-3.0, 3.0, N)
    yy, xx = np.meshgrid(c, c, indexing="ij")
    pos = np.stack([xx, yy, np.zeros_like(xx)], -1).reshape(-1, 3).astype(np.float32)
    idx = []
    for j in range(N - 1):
        for i in range(N - 1):
            a = j * N + i
            idx += [(a, a + 1, a + N + 1), (a, a + N + 1, a + N)]
    nrm = np.tile(np.array([0, 0, 1], np.float32), (N * N, 1))
    return pos, np.array(idx, np.uint32), nrm


def deform(base, amount=1.0, only=None):
    """base + amount * (0.08 sin(1.3 y), 0.06 cos(0.9 x), 0.15 exp(-(x^2 + y^2) / 2)) as float32;
    only: the vertices that move (bool per vertex)."""
    x, y = base[:, 0].astype(np.float64), base[:, 1].astype(np.float64)
    d = amount * np.stack([0.08 * np.sin(1.3 * y), 0.06 * np.cos(0.9 * x), 0.15 * np.exp(-(x * x + y * y) / 2)], -1)
    if only is not None:
        d[~only] = 0.0
    return (base.astype(np.float64) + d).astype(np.float32)


def _world(extra=None):
    """instance 0: the flat grid (shape 0); extra = "shared": two instances of it, each filling its
    half, plus a sphere and a small second mesh in front of them; last: a light out of view."""
    pos, idx, nrm = grid()
    w = World()
    w.set_film(WIDTH, HEIGHT, 2)
    w.set_sensor(FOV, W.look_at_mitsuba((0, 0, CAM_Z), (0, 0, 0), (0, 1, 0)), fov_axis="x")
    mat = w.add_material(W.diffuse((0.5, 0.5, 0.5), twosided=True))
    g = w.add_mesh(pos, idx, nrm)
    if extra == "shared":
        w.add_instance(g, mat, W.transform(scale=(2 / 3, 2 / 3, 1), translate=(-2, 0, 0)))
        w.add_instance(g, mat, W.transform(scale=(2 / 3, 2 / 3, 1), translate=(2, 0, 0)))
        w.add_instance(w.add_builtin("sphere"), mat, W.transform(scale=(0.25, 0.25, 0.25), translate=(-0.8, 0.5, 1.0)))
        quad = np.array([[-1, -1, 0], [1, -1, 0], [1, 1, 0], [-1, 1, 0]], np.float32)
        w.add_instance(w.add_mesh(quad, np.array([[0, 1, 2], [0, 2, 3]], np.uint32)), mat,
                       W.transform(scale=(0.25, 0.25, 1), translate=(0.7, -0.4, 1.0)))
    else:
        w.add_instance(g, mat)
    w.add_instance(w.add_builtin("rectangle"), mat, W.transform(scale=(0.1, 0.1, 1), translate=(0, 50, 0)),
                   emitter_radiance=W.rgb(1.0))
    return w


def _pass(world):
    from pupiloptixlab_amd.pt_pass import PTPass

    pt = PTPass(device=0)
    pt.set_scene(world)
    return pt


def _to_world(desc):
    """(n, 4, 4) float64 of the float32 instance transforms the engine gets."""
    m = np.tile(np.eye(4), (desc.num_instances, 1, 1))
    for i in range(desc.num_instances):
        m[i, :3] = np.array(list(desc.instances[i].to_world), np.float64).reshape(3, 4)
    return m


def _camera(desc):
    return _mat(desc.sample_to_camera), _mat(desc.camera_to_world)


# ------------------------------------------------------------------ float64 reference
def _xf(m, p):
    return p @ m[:3, :3].T + m[:3, 3]


def intersect(o, d, objects):
    """Nearest float64 hit of every ray.  objects: ("mesh", to_world, vertices, indices) or
    ("sphere", to_world) (the unit sphere).  Returns t, object (-1 = none), triangle, the
    barycentrics (b1 on the triangle's second vertex, b2 on its third) and how many triangles of
    the nearest object the ray passes through."""
    n = len(o)
    best_t, best_obj = np.full(n, np.inf), np.full(n, -1)
    best_tri, best_b = np.full(n, -1), np.zeros((n, 2))
    crossings = np.zeros(n, int)
    for k, ob in enumerate(objects):
        if ob[0] == "sphere":
            inv = np.linalg.inv(ob[1])
            oo, dd = _xf(inv, o), d @ inv[:3, :3].T
            a, b, c = (dd * dd).sum(1), (oo * dd).sum(1), (oo * oo).sum(1) - 1.0
            disc = b * b - a * c
            t = (-b - np.sqrt(np.maximum(disc, 0.0))) / a
            ok = (disc > 0) & (t > 1e-3) & (t < best_t)
            best_t[ok], best_obj[ok], best_tri[ok] = t[ok], k, -1
            continue
        _, m, verts, idx = ob
        wv = _xf(m, verts.astype(np.float64))
        v0, v1, v2 = wv[idx[:, 0]], wv[idx[:, 1]], wv[idx[:, 2]]
        e1, e2 = v1 - v0, v2 - v0  # (m, 3)
        pv = np.cross(d[:, None, :], e2[None])  # (n, m, 3)
        det = (pv * e1[None]).sum(-1)
        tv = o[:, None, :] - v0[None]
        with np.errstate(divide="ignore", invalid="ignore"):
            u = (tv * pv).sum(-1) / det
            qv = np.cross(tv, e1[None])
            v = (qv * d[:, None, :]).sum(-1) / det
            t = (qv * e2[None]).sum(-1) / det
        hit = (np.abs(det) > 0) & (u >= 0) & (v >= 0) & (u + v <= 1) & (t > 1e-3)
        t = np.where(hit, t, np.inf)
        tri = t.argmin(1)
        tt = t[np.arange(n), tri]
        ok = tt < best_t
        best_t[ok], best_obj[ok], best_tri[ok] = tt[ok], k, tri[ok]
        best_b[ok] = np.stack([u[np.arange(n), tri], v[np.arange(n), tri]], -1)[ok]
        crossings[ok] = hit.sum(1)[ok]
    return best_t, best_obj, best_tri, best_b, crossings


def reference(cam, prev_cam, objects, prev):
    """float64 flow of the pixel-centre rays.  prev[k]: None = object k did not change, else
    (previous to_world, previous vertices or None = the current ones)."""
    o, d = centre_rays(cam[0], cam[1], WIDTH, HEIGHT)
    t, obj, tri, b, crossings = intersect(o, d, objects)
    assert (obj >= 0).all()  # the geometry overfills the frustum
    p = o + t[:, None] * d
    before = p.copy()
    for k, ob in enumerate(objects):
        sel = obj == k
        if prev[k] is None or not sel.any():
            continue
        ptw, pverts = prev[k]
        if ob[0] == "mesh":
            vv = (ob[2] if pverts is None else pverts).astype(np.float64)
            i = ob[3][tri[sel]]
            w0 = 1.0 - b[sel, 0] - b[sel, 1]
            local = w0[:, None] * vv[i[:, 0]] + b[sel, 0:1] * vv[i[:, 1]] + b[sel, 1:2] * vv[i[:, 2]]
        else:
            local = _xf(np.linalg.inv(ob[1]), p[sel])
        before[sel] = _xf(ptw, local)
    flow, hw = flow_reference(o, d, t, np.ones(len(o), bool), prev_cam[0], prev_cam[1], WIDTH, HEIGHT, moved_by=p - before)
    assert (hw > 0).all()
    return flow, obj, tri, crossings


def _neighbourhood(mask):
    """mask (bool per pixel) grown by one pixel in every direction."""
    m = mask.reshape(HEIGHT, WIDTH)
    g = m.copy()
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            s = np.zeros_like(m)
            s[max(0, dy):HEIGHT + min(0, dy), max(0, dx):WIDTH + min(0, dx)] = \
                m[max(0, -dy):HEIGHT + min(0, -dy), max(0, -dx):WIDTH + min(0, -dx)]
            g |= s
    return g.reshape(-1)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def _single(amount=1.0, moved_instance=False, moved_camera=False, partial=False):
    """The one-grid scene: flat before, deformed now.  Returns the current vertices, the cameras
    and the float64 reference, computed once and shared (callers do not modify them)."""
    pos, idx, _ = grid()
    only = pos[:, 0] > 0.5 if partial else None
    cur = deform(pos, amount, only)
    w = _world()
    d = w.desc()
    cam = _camera(d)
    tw_prev = _to_world(d)
    tw_now = tw_prev.copy()
    if moved_instance:
        tw_now[0] = W.transform(translate=OFFSET).astype(np.float32).astype(np.float64)
    prev_cam = cam
    if moved_camera:
        c32 = _camera_cases(cam[1])["translate"].astype(np.float32)
        prev_cam = (cam[0], c32.astype(np.float64))
    flow, obj, tri, crossings = reference(cam, prev_cam, [("mesh", tw_now[0], cur, idx)], [(tw_prev[0], pos)])
    assert (obj == 0).all()
    return dict(pos=pos, idx=idx, cur=cur, only=only, cam=cam, prev_cam=prev_cam, tw_prev=tw_prev, tw_now=tw_now,
                flow=flow, tri=tri, crossings=crossings)


def _deformed_pass(ref, keep=True, rebuild=False, device=False, move=True):
    """A pass on the flat grid, then the reference's deformation (and instance move) applied."""
    import torch

    w = _world()
    pt = _pass(w)
    if device:
        pt.update_shape_device(0, torch.from_numpy(ref["cur"]).to(pt.device), rebuild=rebuild, keep_previous=keep)
    else:
        w.set_mesh_vertices(0, ref["cur"])
        pt.update_shape(w, 0, rebuild=rebuild, keep_previous=keep)
    if move and not np.array_equal(ref["tw_now"], ref["tw_prev"]):
        w.set_instance_transform(0, ref["tw_now"][0].astype(np.float32))
        pt.update_instance(w, 0)
    return w, pt


def _explicit(ref):
    """prev_camera / prev_to_world arguments of the reference's previous frame."""
    cam = (ref["prev_cam"][0].astype(np.float32), ref["prev_cam"][1].astype(np.float32))
    moved = not np.array_equal(ref["tw_now"], ref["tw_prev"])
    return cam, (ref["tw_prev"][:, :3].astype(np.float32).reshape(-1, 12) if moved else None)


def _accel(monkeypatch, accel):
    if accel != "flat":
        monkeypatch.setenv("PUPIL_ACCEL", "two_level")
        monkeypatch.setenv("PUPIL_TL_MODE", "object" if accel == "two_level_object" else "world")
    else:
        monkeypatch.setenv("PUPIL_ACCEL", "flat")


# ------------------------------------------------------------------ 1. deformation only
def test_reference_scene_is_what_the_tolerance_assumes():
    """float64 only: every centre ray passes through exactly one triangle, most pixels move by
    more than half a pixel, and the flow is continuous across triangle edges -- a ray that picks
    the other triangle at a shared edge in float32 gets the same answer."""
    ref = _single()
    assert (ref["crossings"] == 1).all()
    mag = np.abs(ref["flow"]).max(-1)
    f = ref["flow"].reshape(HEIGHT, WIDTH, 2)
    jump = max(np.abs(np.diff(f, axis=0)).max(), np.abs(np.diff(f, axis=1)).max())
    print(f"deform reference: max |flow| {mag.max():.3g} px, {(mag > 0.5).mean():.0%} above 0.5 px, neighbour jump {jump:.3g} px")
    assert 1.3 < mag.max() < 1.4 and (mag > 0.5).mean() >= 0.85 and jump < 0.11


@pytest.mark.parametrize("accel", ["flat", "two_level_world", "two_level_object"])
def test_deformation_only(accel, monkeypatch):
    _accel(monkeypatch, accel)
    ref = _single()
    w, pt = _deformed_pass(ref)
    assert pt.stats()["two_level"] == (0 if accel == "flat" else 1)
    pt.render(1)
    got = gpu_flow(pt)
    assert np.abs(ref["flow"]).max() > 1.0
    compare("deform " + accel, got, ref["flow"], np.ones(len(got), bool), TOL)
    pt.close_engine()


# ------------------------------------------------------------------ 2. everything at once
def test_deformation_instance_and_camera_motion():
    """prev_to_world (to_object p - d): the deformation is undone in object space, before the
    previous instance transform and the previous camera."""
    ref = _single(moved_instance=True, moved_camera=True)
    w, pt = _deformed_pass(ref)
    pt.render(1)
    got = gpu_flow(pt, *_explicit(ref))
    compare("deform + instance + camera", got, ref["flow"], np.ones(len(got), bool), TOL)
    only_deform = _single()["flow"]
    assert np.abs(ref["flow"] - only_deform).max(-1).min() > 0.5  # the rigid motions are not a detail here
    pt.close_engine()


# ------------------------------------------------------------------ 3. partly static mesh
@pytest.mark.parametrize("moved_instance", [False, True])
def test_partly_static_mesh(moved_instance):
    ref = _single(moved_instance=moved_instance, moved_camera=True, partial=True)
    cam, ptw = _explicit(ref)
    assert (ptw is not None) == moved_instance
    w, pt = _deformed_pass(ref)
    kept = gpu_flow(pt, cam, ptw)
    pt.close_engine()
    w, pt = _deformed_pass(ref, keep=False)
    rigid = gpu_flow(pt, cam, ptw)
    pt.close_engine()
    moves = ref["only"][ref["idx"][ref["tri"]]]  # per pixel: which of the hit triangle's vertices move
    unmoved, moved = ~moves.any(1), moves.all(1)
    if not moved_instance:
        assert unmoved.sum() == 1320 and moved.sum() == 769
    assert unmoved.sum() > 1200 and moved.sum() > 600
    still = unmoved & ~_neighbourhood(~unmoved)
    assert still.sum() > 1000
    assert np.array_equal(_bits(kept[still]), _bits(rigid[still]))
    compare(f"partly static, moved triangles (instance moved: {moved_instance})", kept, ref["flow"], moved, TOL)
    compare(f"partly static, every pixel (instance moved: {moved_instance})", kept, ref["flow"], np.ones(len(kept), bool), TOL)
    assert np.abs(kept[moved] - rigid[moved]).max(-1).max() > 0.5


# ------------------------------------------------------------------ 4. shared shape and bystanders
def test_shared_shape_and_bystanders():
    pos, idx, _ = grid()
    cur = deform(pos)
    w = _world("shared")
    d = w.desc()
    cam = _camera(d)
    tw = _to_world(d)
    quad = np.array([[-1, -1, 0], [1, -1, 0], [1, 1, 0], [-1, 1, 0]], np.float32)
    objects = [("mesh", tw[0], cur, idx), ("mesh", tw[1], cur, idx), ("sphere", tw[2]),
               ("mesh", tw[3], quad, np.array([[0, 1, 2], [0, 2, 3]]))]
    c32 = _camera_cases(cam[1])["translate"].astype(np.float32)
    prev_cam = (cam[0], c32.astype(np.float64))
    ref, obj, _, _ = reference(cam, prev_cam, objects, [(tw[0], pos), (tw[1], pos), None, None])
    cam_arg = (cam[0].astype(np.float32), c32)
    flows = {}
    for keep in (True, False):
        w = _world("shared")
        pt = _pass(w)
        w.set_mesh_vertices(0, cur)
        pt.update_shape(w, 0, keep_previous=keep)
        flows[keep] = gpu_flow(pt, cam_arg)
        pt.close_engine()
    cls = obj.reshape(HEIGHT, WIDTH)
    edge = np.zeros((HEIGHT, WIDTH), bool)  # next to a pixel of another object
    edge[:, 1:] |= cls[:, 1:] != cls[:, :-1]
    edge[:, :-1] |= cls[:, 1:] != cls[:, :-1]
    edge[1:, :] |= cls[1:, :] != cls[:-1, :]
    edge[:-1, :] |= cls[1:, :] != cls[:-1, :]
    assert edge.mean() <= 0.10
    keep_px = ~edge.reshape(-1)
    for k, name in ((0, "left instance"), (1, "right instance")):
        assert (keep_px & (obj == k)).sum() > 800
        compare("shared shape, " + name, flows[True], ref, keep_px & (obj == k), TOL)
    for k, name in ((2, "sphere"), (3, "second mesh")):
        m = keep_px & (obj == k)
        assert m.sum() > 40, name
        assert np.array_equal(_bits(flows[True][m]), _bits(flows[False][m])), name
        compare("bystander " + name, flows[True], ref, m, TOL)
    grids = keep_px & (obj <= 1)
    assert np.abs(flows[True][grids] - flows[False][grids]).max() > 1.0  # the snapshot is what moves them


# ------------------------------------------------------------------ 5. device tensors
def test_device_tensors_equal_the_host_path():
    ref = _single()
    flows = []
    for device in (False, True):
        w, pt = _deformed_pass(ref, device=device)
        pt.render(1)
        flows.append(gpu_flow(pt))
        pt.close_engine()
    assert np.abs(flows[0]).max() > 1.0
    assert np.array_equal(_bits(flows[0]), _bits(flows[1]))


# ------------------------------------------------------------------ 6. PUPIL_VERTS_REBUILD
@pytest.mark.parametrize("accel", ["flat", "two_level_world"])
def test_rebuild_keeps_the_snapshot(accel, monkeypatch):
    _accel(monkeypatch, accel)
    ref = _single()
    o, d = centre_rays(ref["cam"][0], ref["cam"][1], WIDTH, HEIGHT)
    flows, prims = [], []
    for rebuild in (False, True):
        w, pt = _deformed_pass(ref, rebuild=rebuild)
        pt.render(1)
        flows.append(gpu_flow(pt))
        prims.append(trace(pt, o, d)[3])
        pt.close_engine()
    compare("rebuild " + accel, flows[1], ref["flow"], np.ones(len(o), bool), TOL)
    assert np.abs(flows[1] - flows[0]).max() <= TOL
    assert np.array_equal(prims[0], prims[1])
    assert (prims[1] != ref["tri"]).sum() <= 2  # instance 0's faces are global primitives 0..127


# ------------------------------------------------------------------ 7. lifecycle
def test_lifecycle():
    import torch

    ref = _single()
    moved_cam = _explicit(_single(moved_camera=True))[0]
    # a pass that never asks for it: the camera's flow and nothing else
    w, pt = _deformed_pass(ref, keep=False)
    pt.render(1)
    assert not pt._snapshots
    plain = gpu_flow(pt)
    plain_cam = gpu_flow(pt, moved_cam)
    compare("no keyword", plain, np.zeros_like(plain), np.ones(len(plain), bool), TOL)
    pt.close_engine()

    # two kept updates before one render: the first "before" (the flat grid) stays
    w = _world()
    pt = _pass(w)
    pt.render(1)
    w.set_mesh_vertices(0, deform(ref["pos"], 0.4))
    pt.update_shape(w, 0, keep_previous=True)
    with pytest.raises(RuntimeError):
        pt.motion_vectors()  # the engine holds vertices no render has used
    w.set_mesh_vertices(0, ref["cur"])
    pt.update_shape(w, 0, keep_previous=True)
    with pytest.raises(RuntimeError):
        pt.motion_vectors()
    pt.render(1)
    got = gpu_flow(pt)
    compare("two kept updates", got, ref["flow"], np.ones(len(got), bool), TOL)
    pt.render(1)  # nothing deformed between the last two renders
    torch.cuda.synchronize()
    got = gpu_flow(pt)
    compare("render without a deformation", got, np.zeros_like(got), np.ones(len(got), bool), TOL)
    # the next kept update starts from the vertices of the render before it
    half = _single(amount=0.4)
    w.set_mesh_vertices(0, half["cur"])
    pt.update_shape(w, 0, keep_previous=True)
    pt.render(1)
    got = gpu_flow(pt)
    back, _, _, _ = reference(ref["cam"], ref["cam"], [("mesh", ref["tw_now"][0], half["cur"], ref["idx"])],
                              [(ref["tw_prev"][0], ref["cur"])])
    assert np.abs(back).max() > 0.5
    compare("second frame", got, back, np.ones(len(got), bool), TOL)
    # an update without the keyword after all that: bit for bit the flow of the pass that never used it
    w.set_mesh_vertices(0, ref["cur"])
    pt.update_shape(w, 0)
    pt.render(1)
    assert not pt._snapshots
    assert np.array_equal(_bits(gpu_flow(pt)), _bits(plain))
    assert np.array_equal(_bits(gpu_flow(pt, moved_cam)), _bits(plain_cam))
    assert np.abs(plain_cam).max() > 0.3
    pt.set_scene(w)  # a new engine holds no snapshot
    assert not pt._kept and not pt._snapshots
    pt.close_engine()


# ------------------------------------------------------------------ 8. tiling
def test_tiled_ranks_equal_full_image():
    import torch

    ref = _single(moved_instance=True, moved_camera=True)
    cam, ptw = _explicit(ref)
    w, pt = _deformed_pass(ref)
    full = pt.motion_vectors(cam, ptw).cpu().numpy().copy()
    assert np.abs(full - ref["flow"]).max() < 1e-2
    stitched = np.full_like(full, np.inf)
    for rank in range(2):
        pt.set_tiling(32, rank, 2)
        part = pt.motion_vectors(cam, ptw)
        torch.cuda.synchronize()
        px = pt.local_pixels()
        assert part.shape[0] == len(px)
        stitched[px] = part.cpu().numpy()
    assert np.array_equal(stitched.view(np.uint32), full.view(np.uint32))
    pt.close_engine()


# ------------------------------------------------------------------ 9. no side effects
def test_snapshot_and_flow_have_no_side_effects():
    import torch

    ref = _single()
    out = []
    for keep in (True, False):
        w, pt = _deformed_pass(ref, keep=keep)
        if keep:
            pt.motion_vectors(_explicit(ref)[0])
        pt.mark_dirty()
        pt.render(2)
        torch.cuda.synchronize()
        st = pt.stats()
        out.append(({k: pt.buffers.get(k).cpu().numpy().copy() for k in KEYS}, st["rays_traced_total"], st["accel_refits"]))
        pt.close_engine()
    for k in KEYS:
        assert np.array_equal(out[0][0][k].view(np.uint32), out[1][0][k].view(np.uint32)), k
    assert out[0][1] == out[1][1] > 0 and out[0][2] == out[1][2] == 1


# ------------------------------------------------------------------ 10. the C entry on a live engine
def test_c_entry_on_a_live_engine():
    import torch

    ref = _single()
    w = _world("shared")  # shape 0 the grid, 1 the sphere, 2 the small mesh, 3 the light's rectangle
    pt = _pass(w)
    lib = pt._lib
    cam = (ref["cam"][0].astype(np.float32), ref["cam"][1].astype(np.float32))

    def render():
        pt.mark_dirty()
        pt.render(2)
        torch.cuda.synchronize()
        return {k: pt.buffers.get(k).cpu().numpy().copy() for k in KEYS}

    before = render()
    stats = pt.stats()
    assert lib.pupil_pt_snapshot_shape_vertices(pt._pt, 1) == abi.ERR_INVALID  # the sphere
    assert b"mesh" in lib.pupil_last_error()
    assert lib.pupil_pt_snapshot_shape_vertices(pt._pt, w.desc().num_shapes) == abi.ERR_INVALID
    assert b"range" in lib.pupil_last_error()
    after = render()
    for k in KEYS:
        assert np.array_equal(before[k].view(np.uint32), after[k].view(np.uint32)), k
    rigid = gpu_flow(pt, cam)
    assert lib.pupil_pt_snapshot_shape_vertices(pt._pt, 0) == abi.OK  # a valid call after the failed ones
    assert lib.pupil_pt_snapshot_shape_vertices(pt._pt, 0) == abi.OK  # overwrites
    after = render()  # a snapshot alone changes no pixel and is no refit
    for k in KEYS:
        assert np.array_equal(before[k].view(np.uint32), after[k].view(np.uint32)), k
    assert pt.stats()["accel_refits"] == stats["accel_refits"]
    assert np.array_equal(_bits(gpu_flow(pt, cam)), _bits(rigid))  # nothing moved since the snapshot
    w.set_mesh_vertices(0, deform(grid()[0]))
    pt.update_shape(w, 0)  # the engine holds the snapshot the C call took
    moved = gpu_flow(pt, cam)
    assert np.abs(moved - rigid).max() > 1.0
    assert lib.pupil_pt_clear_vertex_snapshots(pt._pt) == abi.OK
    cleared = gpu_flow(pt, cam)
    assert np.abs(cleared).max() < TOL  # static camera, no snapshot: no flow
    assert lib.pupil_pt_snapshot_shape_vertices(pt._pt, 0) == abi.OK  # and again after a clear: the deformed grid
    assert np.array_equal(_bits(gpu_flow(pt, cam)), _bits(cleared))
    pt.close_engine()
