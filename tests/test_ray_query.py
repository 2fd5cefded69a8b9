"""Ray queries from device memory (pupil_pt_query_rays / _query_camera, csrc/pt_query.hip) through
PTPass.trace / primary_hits / pick.

Hits are compared bit for bit with the host entry pupil_pt_trace_rays and with the CPU oracle; the
ids with what the oracle's primitive id and the scene description's primitive offsets give; the
normal with the "normal" AOV of a render of the same camera rays; position and texcoord with a
numpy float32 restatement of reconstruct() (pt_shade.h) in its order of operations.  Only the
texcoord of a sphere passes through library functions (atan2, acos) and has a bound:

    SPHERE_UV_TOL = 4 x the largest |uv_gpu - uv_float64| measured on an MI355X over the rays of
    test_position_and_texcoord (see its docstring and profiles/ray_query_timing.txt).
"""
import contextlib
import ctypes as C
import os
import tempfile

import numpy as np
import pytest

import oracle
from pupiloptixlab_amd import World, abi, scenes

pytestmark = pytest.mark.gpu

_TMPDIR = tempfile.TemporaryDirectory(prefix="pupil_ray_query_")
TMP = _TMPDIR.name
RES = 64
SEED = 3
COUNTS = [1, 63, 64, 65, 257, 1000]  # wave and block tails of the resolve kernel and of the eight-shard split
SCENES = ["cornell", "materials", "instanced"]
ACCELS = ["flat", "two_level"]
FIELD = dict(num_instances=4, width=RES, height=RES, max_depth=4, seed=3, spheres_per_blas=2, slices=8, stacks=6)
MEASURED_SPHERE_UV = 5.41e-7  # the cornell_materials rays: 486 sphere hits, 2 of them at the seam; either accelerator
SPHERE_UV_TOL = 4 * MEASURED_SPHERE_UV  # 2.164e-6
ALL = ("hit", "instance", "primitive", "material", "position", "normal", "texcoord")


def _world(scene):
    if scene == "cornell":
        return World().load_scene(scenes.cornell_xml(os.path.join(TMP, "cb.xml"), RES, RES, 4))
    if scene == "materials":
        return World().load_scene(scenes.cornell_materials_xml(os.path.join(TMP, "cbm.xml"), RES, RES, 4))
    return scenes.instanced_field(**FIELD)


@contextlib.contextmanager
def _accel_env(accel):
    old = os.environ.get("PUPIL_ACCEL")
    os.environ["PUPIL_ACCEL"] = accel
    try:
        yield
    finally:
        if old is None:
            del os.environ["PUPIL_ACCEL"]
        else:
            os.environ["PUPIL_ACCEL"] = old


def _pass(world, accel):
    from pupiloptixlab_amd.pt_pass import PTPass

    with _accel_env(accel):
        pt = PTPass(device=0)
        pt.set_scene(world)
    assert pt.stats()["two_level"] == (0 if accel == "flat" else 1)
    return pt


def _r8(rays6):
    n = len(rays6)
    return np.ascontiguousarray(np.concatenate([rays6, np.full((n, 1), 0.001, np.float32),
                                                np.full((n, 1), 1e16, np.float32)], 1), np.float32)


class Reference:
    """What the tests of one scene share: its world, the oracle, the rays and the oracle's hits.
    Computed once per scene and left unchanged."""

    def __init__(self, scene):
        self.world = _world(scene)
        self.desc = self.world.desc()
        self.oracle = oracle.OracleScene(self.desc)
        d = self.desc
        self.camera = _r8(np.array([self.oracle.camera_ray(p, SEED) for p in range(d.width * d.height)], np.float32))
        rng = np.random.default_rng(17)
        lo, hi = ([-0.9, 0.1, -0.9], [0.9, 1.9, 0.9]) if scene != "instanced" else ([-7, 0.5, -9], [7, 13, 10])
        org = rng.uniform(lo, hi, (992, 3))
        dirs = rng.normal(size=(992, 3))
        dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
        # and 8 rays that start far above the scene and leave it: misses
        away = np.concatenate([rng.uniform(-1, 1, (8, 3)) + [0, 500, 0], np.tile([0.0, 1.0, 0.0], (8, 1))], 1)
        self.random = _r8(np.concatenate([np.concatenate([org, dirs], 1), away]).astype(np.float32))
        assert len(self.random) == 1000
        self.ref = {"camera": self.oracle.closest(self.camera), "random": self.oracle.closest(self.random)}
        # the scene description's primitive offsets: a mesh instance holds its shape's faces, a sphere one
        counts = [d.shapes[d.instances[i].shape].num_faces if d.shapes[d.instances[i].shape].kind == abi.SHAPE_MESH
                  else 1 for i in range(d.num_instances)]
        self.offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        self.is_sphere = np.array([d.shapes[d.instances[i].shape].kind == abi.SHAPE_SPHERE
                                   for i in range(d.num_instances)])
        self.materials = np.array([d.instances[i].material for i in range(d.num_instances)], np.int64)

    def rays(self, which):
        return self.camera if which == "camera" else self.random

    def ids(self, which):
        """instance, primitive, material (-1 on a miss) from the oracle's primitive ids."""
        prim = self.ref[which][:, 3].copy().view(np.uint32).astype(np.int64)
        miss = prim == 0xFFFFFFFF
        inst = np.searchsorted(self.offsets, np.where(miss, 0, prim), side="right") - 1
        local = np.where(miss, 0, prim) - self.offsets[inst]
        return (np.where(miss, -1, inst), np.where(miss, -1, local), np.where(miss, -1, self.materials[inst]), miss)


_REFS, _PASSES = {}, {}


def reference(scene):
    if scene not in _REFS:
        _REFS[scene] = Reference(scene)
    return _REFS[scene]


def shared_pass(scene, accel):
    """An engine the tests only query (renders and queries leave what a query returns alone)."""
    if (scene, accel) not in _PASSES:
        _PASSES[scene, accel] = _pass(reference(scene).world, accel)
    return _PASSES[scene, accel]


@pytest.fixture(scope="module", autouse=True)
def _close_engines():
    yield
    for pt in _PASSES.values():
        pt.close_engine()
    _PASSES.clear()
    _REFS.clear()


def dev(pt, a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).to(pt.device)


def host(d):
    return {k: v.cpu().numpy() for k, v in d.items()}


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same(a, b, what=""):
    assert a.shape == b.shape, (what, a.shape, b.shape)
    bad = bits(a) != bits(b)
    assert not bad.any(), f"{what}: {int(bad.reshape(len(a), -1).any(axis=1).sum())} of {len(a)} rays differ"


def host_trace(pt, r8, any_hit=0):
    out = np.zeros((len(r8), 4), np.float32)
    abi.check(pt._lib.pupil_pt_trace_rays(pt._pt, len(r8), r8.ctypes.data_as(abi.f32p), out.ctypes.data_as(abi.f32p),
                                          any_hit))
    return out


# ------------------------------------------------------------------ 1. hits
@pytest.mark.parametrize("accel", ACCELS)
@pytest.mark.parametrize("scene", SCENES)
def test_hits_equal_host_entry_and_oracle(scene, accel):
    ref = reference(scene)
    pt = shared_pass(scene, accel)
    for which in ("random", "camera"):
        r8 = ref.rays(which)
        counts = COUNTS if which == "random" else [len(r8)]
        for n in counts:
            got = pt.trace(dev(pt, r8[:n]), want=("hit",))["hit"].cpu().numpy()
            same(got, host_trace(pt, r8[:n]), f"{scene} {accel} {which} n={n} vs pupil_pt_trace_rays")
            same(got, ref.ref[which][:n], f"{scene} {accel} {which} n={n} vs oracle")
            occ = pt.trace(dev(pt, r8[:n]), any_hit=True)
            assert set(occ) == {"hit"}
            occ = occ["hit"].cpu().numpy()
            same(occ, host_trace(pt, r8[:n], 1), f"{scene} {accel} {which} n={n} any hit")
            assert np.array_equal(occ[:, 0] > 0, ref.ref[which][:n, 0] > 0)
            assert set(np.unique(occ[:, 0])) <= {1.0, -1.0}


# ------------------------------------------------------------------ 2. ids
@pytest.mark.parametrize("accel", ACCELS)
@pytest.mark.parametrize("scene", SCENES)
def test_ids_follow_the_scene_description(scene, accel):
    ref = reference(scene)
    pt = shared_pass(scene, accel)
    sphere_hits = misses = 0
    for which in ("random", "camera"):
        inst, local, mat, miss = ref.ids(which)
        r8 = ref.rays(which)
        for n in (COUNTS if which == "random" else [len(r8)]):
            # ids alone (the kernel without the geometry) and with everything else
            for want in (("instance", "primitive", "material"), ALL):
                got = host(pt.trace(dev(pt, r8[:n]), want=want))
                assert np.array_equal(got["instance"], inst[:n]), (scene, accel, which, n, want)
                assert np.array_equal(got["primitive"], local[:n]), (scene, accel, which, n, want)
                assert np.array_equal(got["material"], mat[:n]), (scene, accel, which, n, want)
        on_sphere = ~miss & ref.is_sphere[np.where(miss, 0, inst)]
        assert (local[on_sphere] == 0).all()
        sphere_hits += int(on_sphere.sum())
        misses += int(miss.sum())
        full = host(pt.trace(dev(pt, r8), want=ALL))
        for k in ("position", "normal", "texcoord"):
            assert (bits(full[k][miss]) == 0).all(), k  # exactly +0
        assert (full["hit"][miss, 0] == -1).all() and (bits(full["hit"][miss, 3]) == 0xFFFFFFFF).all()
    assert misses >= 8
    if scene == "materials":
        assert sphere_hits > 100


# ------------------------------------------------------------------ 3. normal against the renderer
@pytest.mark.parametrize("accel", ACCELS)
@pytest.mark.parametrize("scene", SCENES)
def test_normal_equals_the_normal_aov(scene, accel):
    import torch

    ref = reference(scene)
    pt = shared_pass(scene, accel)
    pt.dirty = False
    pt.random_seed, pt.sample_cnt = SEED, 0
    pt.render(1)
    torch.cuda.synchronize()
    aov = pt.buffers.get("normal").cpu().numpy()
    got = pt.trace(dev(pt, ref.camera), want=("normal",))["normal"].cpu().numpy()
    same(got, aov, f"{scene} {accel} normal vs AOV")
    miss = ref.ids("camera")[3]
    assert (bits(got[miss]) == 0).all()
    assert (np.abs(np.linalg.norm(got[~miss], axis=1) - 1) < 1e-5).all()


# ------------------------------------------------------------------ 4. position and texcoord
def _f32(a):
    return np.asarray(a, np.float32)


def _shape_arrays(d, s):
    sh = d.shapes[s]
    nv, nf = sh.num_vertices, sh.num_faces
    pos = np.ctypeslib.as_array(sh.positions, (nv * 3,)).reshape(nv, 3).copy()
    idx = np.ctypeslib.as_array(sh.indices, (nf * 3,)).reshape(nf, 3).copy()
    tex = np.ctypeslib.as_array(sh.texcoords, (nv * 2,)).reshape(nv, 2).copy() if sh.texcoords else None
    return pos, idx, tex


def _xform_point(m, p):
    """pt_math.h xform_point in float32, left to right."""
    m = _f32(m)
    return np.stack([m[4 * r] * p[:, 0] + m[4 * r + 1] * p[:, 1] + m[4 * r + 2] * p[:, 2] + m[4 * r + 3]
                     for r in range(3)], 1)


def restate_triangles(ref, which, hit):
    """reconstruct()'s position and texcoord of the triangle hits, float32 in its order: the
    barycentric sum w p0 + u p1 + v p2 with w = 1 - u - v, then the instance transform."""
    d = ref.desc
    inst, local, _, miss = ref.ids(which)
    pos = np.zeros((len(hit), 3), np.float32)
    uv = np.zeros((len(hit), 2), np.float32)
    tri = ~miss & ~ref.is_sphere[np.where(miss, 0, inst)]
    for i in np.unique(inst[tri]):
        sel = tri & (inst == i)
        ins = d.instances[int(i)]
        p, idx, tex = _shape_arrays(d, ins.shape)
        f = idx[local[sel]]
        u, v = hit[sel, 1:2], hit[sel, 2:3]
        w = np.float32(1.0) - u - v
        obj = w * p[f[:, 0]] + u * p[f[:, 1]] + v * p[f[:, 2]]
        pos[sel] = _xform_point(list(ins.to_world), obj)
        if tex is not None:
            t = w * tex[f[:, 0]] + u * tex[f[:, 1]] + v * tex[f[:, 2]]
            if ins.flip_tex_coords:
                t[:, 1] = np.float32(1.0) - t[:, 1]
            uv[sel] = t
    return pos, uv, tri


@pytest.mark.parametrize("accel", ACCELS)
@pytest.mark.parametrize("scene", SCENES)
def test_position_and_texcoord(scene, accel):
    """Triangles: bit for bit the float32 restatement.  Spheres: position = o + t d in float32 bit
    for bit; texcoord against float64 within SPHERE_UV_TOL = 4 x MEASURED_SPHERE_UV = 2.164e-6,
    MEASURED_SPHERE_UV = 5.41e-7 being the largest deviation measured on an MI355X over these rays
    (u within 1e-3 of the seam left out: 2 of the 486 sphere hits)."""
    ref = reference(scene)
    pt = shared_pass(scene, accel)
    d = ref.desc
    worst, seam, spheres = 0.0, 0, 0
    for which in ("random", "camera"):
        r8 = ref.rays(which)
        got = host(pt.trace(dev(pt, r8), want=ALL))
        hit = got["hit"]
        pos, uv, tri = restate_triangles(ref, which, hit)
        assert tri.sum() > 100
        same(got["position"][tri], pos[tri], f"{scene} {accel} {which} triangle position")
        same(got["texcoord"][tri], uv[tri], f"{scene} {accel} {which} triangle texcoord")
        inst, _, _, miss = ref.ids(which)
        sph = ~miss & ~tri
        if not sph.any():
            continue
        o, dd, t = r8[sph, 0:3], r8[sph, 3:6], hit[sph, 0:1]
        same(got["position"][sph], o + t * dd, f"{scene} {accel} {which} sphere position")
        p64 = got["position"][sph].astype(np.float64)
        to_obj = np.array([list(d.instances[int(i)].to_object) for i in inst[sph]], np.float64).reshape(-1, 3, 4)
        lp = np.einsum("nij,nj->ni", to_obj[:, :, :3], p64) + to_obj[:, :, 3]
        lp /= np.linalg.norm(lp, axis=1, keepdims=True)
        phi = np.arctan2(lp[:, 1], lp[:, 0])
        phi = np.where(phi < 0, phi + 2 * np.pi, phi)
        ref_uv = np.stack([phi / (2 * np.pi), np.arccos(np.clip(lp[:, 2], -1, 1)) / np.pi], 1)
        near = (ref_uv[:, 0] < 1e-3) | (ref_uv[:, 0] > 1 - 1e-3)
        seam += int(near.sum())
        spheres += int(sph.sum())
        err = np.abs(got["texcoord"][sph].astype(np.float64) - ref_uv)[~near]
        worst = max(worst, float(err.max()))
    if scene == "materials":
        assert spheres > 100
    if spheres:
        print(f"sphere texcoord {scene} {accel}: {spheres} hits, {seam} at the seam, max |uv - float64| {worst:.3e}")
        assert seam <= 0.02 * spheres, (seam, spheres)
        assert worst <= SPHERE_UV_TOL, worst


# ------------------------------------------------------------------ 5. G-buffer
def centre_rays64(s2c, c2w, width, height):
    """tests/test_motion_vectors.py centre_rays: the pixel-centre camera rays in float64."""
    yy, xx = np.mgrid[0:height, 0:width]
    film = np.stack([(xx + 0.5) / width, (yy + 0.5) / height, np.zeros_like(xx, float), np.ones_like(xx, float)], -1)
    d4 = film.reshape(-1, 4) @ s2c.T
    d = d4[:, :3] / d4[:, 3:4]
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d = d @ c2w[:3, :3].T
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return np.broadcast_to(c2w[:3, 3], d.shape), d


@pytest.mark.parametrize("accel", ACCELS)
@pytest.mark.parametrize("scene", SCENES)
def test_primary_hits_is_trace_of_the_centre_rays(scene, accel):
    import torch

    ref = reference(scene)
    d = ref.desc
    pt = _pass(ref.world, accel)  # its own engine: the tiling changes
    try:
        g = pt.primary_hits(jitter=(0.5, 0.5), return_rays=True)
        rays = g.pop("rays")
        r = rays.cpu().numpy()
        s2c = np.array(list(d.sample_to_camera), np.float64).reshape(4, 4)
        c2w = np.array(list(d.camera_to_world), np.float64).reshape(4, 4)
        o, dirs = centre_rays64(s2c, c2w, d.width, d.height)
        assert np.array_equal(r[:, 0:3], o.astype(np.float32))
        assert (r[:, 6] == np.float32(0.001)).all() and (r[:, 7] == np.float32(1e16)).all()
        # a float32 unit vector behind two 4-term matrix products, a divide and two normalisations:
        # under 16 roundings of 2^-24 relative on components of magnitude <= 1
        assert np.abs(r[:, 3:6] - dirs).max() < 16 * 2.0 ** -24
        t = pt.trace(rays, want=ALL)
        full = host(g)
        for k in ALL:
            same(full[k], t[k].cpu().numpy(), f"{scene} {accel} primary_hits {k}")
        # hit only: the same hits, no scratch
        same(pt.primary_hits(want=("hit",))["hit"].cpu().numpy(), full["hit"], "hit only")
        # a jitter of the render's own draws is not the centre
        assert not np.array_equal(pt.primary_hits(jitter=(0.25, 0.75), want=("hit",))["hit"].cpu().numpy(), full["hit"])
        pt.set_tiling(32, 1, 2)
        local = pt.local_pixels()
        assert 0 < len(local) < d.width * d.height
        part = host(pt.primary_hits(return_rays=True))
        same(part.pop("rays"), r[local], "tiled rays")
        for k in ALL:
            same(part[k], full[k][local], f"{scene} {accel} tiled {k}")
        # the same rank in the frame's index space (not compact): its pixels are written in place
        n = d.width * d.height
        sentinel = torch.full((n, 4), 7.0, device=pt.device)
        inst = torch.full((n,), -9, dtype=torch.int32, device=pt.device)
        nrm = torch.full((n, 3), 7.0, device=pt.device)
        hits = abi.RayHits()
        hits.hit, hits.instance, hits.normal = sentinel.data_ptr(), inst.data_ptr(), nrm.data_ptr()
        s = torch.cuda.current_stream(0)
        abi.check(pt._lib.pupil_pt_query_camera(pt._pt, 0.5, 0.5, 0, 32, 1, 2, None, C.byref(hits),
                                                C.c_void_p(s.cuda_stream)))
        torch.cuda.synchronize()
        other = np.setdiff1d(np.arange(n), local)
        same(sentinel.cpu().numpy()[local], full["hit"][local], "scattered hit")
        same(nrm.cpu().numpy()[local], full["normal"][local], "scattered normal")
        assert np.array_equal(inst.cpu().numpy()[local], full["instance"][local])
        assert (sentinel.cpu().numpy()[other] == 7.0).all() and (inst.cpu().numpy()[other] == -9).all()
    finally:
        pt.close_engine()


# ------------------------------------------------------------------ 6. visibility
@pytest.mark.parametrize("accel", ACCELS)
def test_hidden_instances_are_hit_by_no_query(accel):
    w = _world("materials")
    pt = _pass(w, accel)
    try:
        rays = dev(pt, reference("materials").camera)
        first = host(pt.trace(rays, want=ALL))
        inst, t = first["instance"], first["hit"][:, 0]
        # the nearest object that covers at least 50 pixels: something lies behind it
        cands = [i for i in np.unique(inst[inst >= 0]) if (inst == i).sum() >= 50]
        victim = int(min(cands, key=lambda i: t[inst == i].mean()))
        w.set_instance_visibility(victim, 0)
        pt.update_instances(w, [victim])
        hidden = host(pt.trace(rays, want=ALL))
        assert not (hidden["instance"] == victim).any()
        was = inst == victim
        behind = hidden["hit"][was, 0]
        assert ((behind == -1) | (behind > t[was])).all()
        assert (hidden["instance"][was] >= 0).sum() > 25  # what lies behind it is reported
        for k in ALL:  # the rays that never met it are untouched
            same(hidden[k][~was], first[k][~was], f"{accel} hidden, other rays, {k}")
        occ = pt.trace(rays, any_hit=True)["hit"].cpu().numpy()
        assert np.array_equal(occ[:, 0] > 0, hidden["hit"][:, 0] > 0)
        w.set_instance_visibility(victim, 255)
        pt.update_instances(w, [victim])
        again = host(pt.trace(rays, want=ALL))
        for k in ALL:
            same(again[k], first[k], f"{accel} shown again, {k}")
    finally:
        pt.close_engine()


# ------------------------------------------------------------------ 7. deformation
@pytest.mark.parametrize("accel", ACCELS)
def test_deformed_mesh_equals_a_fresh_engine(accel):
    ref = reference("instanced")
    w = scenes.instanced_field(**FIELD)
    pt = _pass(w, accel)
    try:
        pos, _, _ = _shape_arrays(w.desc(), 0)
        rays = np.concatenate([ref.random, ref.camera])
        before = host(pt.trace(dev(pt, rays), want=ALL))
        for scale, rebuild in ((0.75, False), (0.5, True)):  # a refit, then a rebuild (the flat records move)
            moved = (pos * np.float32(scale)).astype(np.float32)
            pt.update_shape_device(0, dev(pt, moved), rebuild=rebuild)
            got = host(pt.trace(dev(pt, rays), want=ALL))
            w2 = scenes.instanced_field(**FIELD)
            w2.set_mesh_vertices(0, moved)
            fresh = _pass(w2, accel)
            try:
                want = host(fresh.trace(dev(fresh, rays), want=ALL))
            finally:
                fresh.close_engine()
            for k in ALL:
                same(got[k], want[k], f"{accel} scale {scale} rebuild {rebuild} {k}")
            assert not np.array_equal(bits(got["hit"]), bits(before["hit"]))
    finally:
        pt.close_engine()


# ------------------------------------------------------------------ 8. no side effects
RAY_TOTALS = ("primary_rays", "extension_rays", "shadow_rays", "path_samples", "rays_traced_total",
              "shadow_rays_reference", "terminal_rays_culled")


@pytest.mark.parametrize("accel", ACCELS)
def test_a_query_changes_nothing_a_render_produces(accel):
    import torch

    ref = reference("materials")
    rays = ref.random

    def two_renders(query):
        pt = _pass(_world("materials"), accel)
        try:
            pt.render(2, continues=True)
            if query:
                stats = pt.stats()
                mv = pt.motion_vectors().clone()
                pt.trace(dev(pt, rays), want=ALL)
                pt.primary_hits()
                assert np.array_equal(bits(pt.motion_vectors().cpu().numpy()), bits(mv.cpu().numpy()))
                after = pt.stats()
                for k in RAY_TOTALS:
                    assert after[k] == stats[k], k
            pt.render(2)
            torch.cuda.synchronize()
            out = {k: pt.buffers.get(k).cpu().numpy() for k in ("pt accum buffer", "final result", "normal", "albedo")}
            return out, pt.sample_cnt, pt.stats()
        finally:
            pt.close_engine()

    plain, cnt0, st0 = two_renders(False)
    mixed, cnt1, st1 = two_renders(True)
    assert cnt0 == cnt1 == 4
    for k in plain:
        same(mixed[k], plain[k], f"{accel} {k} with a query between the renders")
    for k in RAY_TOTALS:
        assert st0[k] == st1[k], k


# ------------------------------------------------------------------ 9. steady state
@pytest.mark.parametrize("accel", ACCELS)
def test_steady_state_allocates_nothing(accel):
    ref = reference("cornell")
    pt = _pass(ref.world, accel)
    try:
        assert pt.query_info() == {"queries": 0, "rays": 0, "scratch_grows": 0, "last_ms": 0.0}
        rays = dev(pt, ref.random)
        pt.trace(rays, want=("hit",))  # the caller's hit array and no resolved output: no scratch
        pt.trace(rays, want=("hit", "instance"))
        pt.trace(rays, any_hit=True)
        assert pt.query_info()["scratch_grows"] == 0
        pt.trace(rays, want=("instance", "normal"))  # no hit array: the engine's scratch
        info = pt.query_info()
        assert info["scratch_grows"] >= 1 and info["queries"] == 4 and info["rays"] == 4000
        assert info["last_ms"] > 0
        for n in COUNTS:
            pt.trace(rays[:n], want=("position", "texcoord", "material"))
            pt.trace(rays[:n], want=ALL)
        after = pt.query_info()
        assert after["scratch_grows"] == info["scratch_grows"]
        assert after["queries"] == 4 + 2 * len(COUNTS) and after["rays"] == 4000 + 2 * sum(COUNTS)
        assert after["last_ms"] > 0
        # out= reuses the tensors of an earlier call
        first = pt.trace(rays, want=ALL)
        ptrs = {k: v.data_ptr() for k, v in first.items()}
        keep = host(first)
        for v in first.values():
            v.zero_()
        second = pt.trace(rays, want=ALL, out=first)
        assert {k: v.data_ptr() for k, v in second.items()} == ptrs
        for k in ALL:
            same(second[k].cpu().numpy(), keep[k], k)
    finally:
        pt.close_engine()


# ------------------------------------------------------------------ 10. another stream
@pytest.mark.parametrize("accel", ACCELS)
def test_query_on_another_stream_after_a_render(accel):
    import torch

    ref = reference("materials")
    pt = shared_pass("materials", accel)
    rays = dev(pt, ref.camera)
    want = host(pt.trace(rays, want=ALL))
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=0)
    pt.render(4)  # on the default stream; the query shares its overflow stacks
    # the outputs are allocated on the current (default) stream and written on the side one
    got = pt.trace(rays, want=ALL, stream=side)
    g = pt.primary_hits(want=("hit",), return_rays=True, stream=side)
    pt.render(1)  # and a render behind the queries, back on the default stream
    side.synchronize()
    torch.cuda.synchronize()
    got = host(got)
    for k in ALL:
        same(got[k], want[k], f"{accel} side stream {k}")
    same(g["hit"].cpu().numpy(), pt.primary_hits(want=("hit",))["hit"].cpu().numpy(), f"{accel} side stream G-buffer")
    with torch.cuda.stream(side):  # and with the side stream current
        inside = pt.trace(rays, want=ALL)
    side.synchronize()
    for k in ALL:
        same(inside[k].cpu().numpy(), want[k], f"{accel} current side stream {k}")


# ------------------------------------------------------------------ 11. arguments
def test_argument_errors():
    import torch

    ref = reference("cornell")
    pt = shared_pass("cornell", "flat")
    rays = dev(pt, ref.random)
    before = pt.query_info()["queries"]
    with pytest.raises(abi.PupilError) as e:
        pt.trace(rays, any_hit=True, want=("hit", "position"))
    assert e.value.code == abi.ERR_INVALID
    with pytest.raises(abi.PupilError) as e:
        pt.trace(rays, want=())
    assert e.value.code == abi.ERR_INVALID
    with pytest.raises(abi.PupilError) as e:
        pt.primary_hits(want=())
    assert e.value.code == abi.ERR_INVALID
    with pytest.raises(ValueError, match="unknown query output 'depth'"):
        pt.trace(rays, want=("hit", "depth"))
    # device tensors the kernels would read out of bounds: refused by the check that names them
    wide = torch.zeros((1000, 16), dtype=torch.float32, device=pt.device)
    for bad, message in ((rays.double(), r"needs float32 rays, got torch\.float64"),
                         (rays[:, :7], r"needs an \(n, 8\) tensor of rays, got \(1000, 7\)"),
                         (rays[:, :7].contiguous(), r"needs an \(n, 8\) tensor of rays, got \(1000, 7\)"),
                         (rays.reshape(-1), r"needs an \(n, 8\) tensor of rays, got \(8000,\)"),
                         (wide[:, ::2], r"needs contiguous rays"),
                         (rays.cpu(), r"needs rays on cuda:0, got a cpu tensor")):
        with pytest.raises(ValueError, match=message):
            pt.trace(bad)
    assert tuple(wide[:, ::2].shape) == (1000, 8) and not wide[:, ::2].is_contiguous()
    assert pt.query_info()["queries"] == before  # nothing was enqueued
    # out= tensors that do not fit the query: a wrong one would be written out of bounds
    good = pt.trace(rays, want=("hit", "instance", "normal"))
    torch.cuda.synchronize()
    before = pt.query_info()["queries"]
    for name, bad in (("hit", torch.zeros((999, 4), device=pt.device)),                       # too short
                      ("hit", torch.zeros((1000, 3), device=pt.device)),                      # too narrow
                      ("hit", torch.zeros((1000, 4), dtype=torch.float64, device=pt.device)),
                      ("hit", torch.zeros((1000, 8), device=pt.device)[:, ::2]),              # strided
                      ("hit", torch.zeros((1000, 4))),                                        # on the CPU
                      ("hit", np.zeros((1000, 4), np.float32)),                               # not a tensor
                      ("instance", torch.zeros(1000, device=pt.device)),                      # float32 ids
                      ("instance", torch.zeros((1000, 1), dtype=torch.int32, device=pt.device)),
                      ("normal", torch.zeros((1000, 4), device=pt.device))):
        with pytest.raises(ValueError, match=rf"out\['{name}'\] must be a contiguous"):
            pt.trace(rays, want=("hit", "instance", "normal"), out={**good, name: bad})
    assert pt.query_info()["queries"] == before  # nothing was enqueued
    # misaligned pointers, straight at the ABI: the hit array and the ray list need 16 B
    s = C.c_void_p(torch.cuda.current_stream(0).cuda_stream)
    buf = torch.zeros(16 * 1000 + 16, dtype=torch.uint8, device=pt.device)
    hits = abi.RayHits()
    hits.hit = buf.data_ptr() + 4
    assert pt._lib.pupil_pt_query_rays(pt._pt, 1000, C.c_void_p(rays.data_ptr()), 0, C.byref(hits), s) == abi.ERR_INVALID
    hits.hit = buf.data_ptr()
    assert pt._lib.pupil_pt_query_rays(pt._pt, 999, C.c_void_p(rays.data_ptr() + 4), 0, C.byref(hits), s) == abi.ERR_INVALID
    assert pt._lib.pupil_pt_query_rays(pt._pt, 1 << 31, C.c_void_p(rays.data_ptr()), 0, C.byref(hits), s) == abi.ERR_INVALID
    assert pt._lib.pupil_pt_query_rays(pt._pt, 1000, C.c_void_p(rays.data_ptr()), 0, None, s) == abi.ERR_INVALID
    assert pt._lib.pupil_pt_query_rays(pt._pt, 1000, C.c_void_p(rays.data_ptr()), 2, C.byref(hits), s) == abi.ERR_INVALID
    assert pt.query_info()["queries"] == before  # nothing was enqueued
    empty = pt.trace(rays[:0])
    assert set(empty) == set(ALL)
    assert tuple(empty["hit"].shape) == (0, 4) and tuple(empty["instance"].shape) == (0,)
    assert tuple(empty["position"].shape) == (0, 3) and tuple(empty["texcoord"].shape) == (0, 2)
    assert pt._lib.pupil_pt_query_rays(pt._pt, 0, None, 0, C.byref(hits), s) == abi.OK
    assert pt.query_info()["queries"] == before


def test_pick_names_what_a_pixel_shows():
    ref = reference("materials")
    pt = shared_pass("materials", "flat")
    g = host(pt.primary_hits(want=("hit", "instance", "primitive", "material")))
    d = ref.desc
    seen_hit = seen_miss = False
    for x, y in ((RES // 2, RES // 2), (5, 5), (RES - 3, 20), (0, RES - 1), (RES // 3, RES // 4)):
        i = y * d.width + x
        got = pt.pick(x, y)
        if g["instance"][i] < 0:
            assert got is None
            seen_miss = True
            continue
        seen_hit = True
        assert got is not None and isinstance(got["instance"], int) and isinstance(got["t"], float)
        assert (got["instance"], got["primitive"], got["material"]) == (
            int(g["instance"][i]), int(g["primitive"][i]), int(g["material"][i]))
        assert got["t"] == pytest.approx(float(g["hit"][i, 0]), rel=1e-5)
    assert seen_hit
    with pytest.raises(ValueError):
        pt.pick(RES, 0)
