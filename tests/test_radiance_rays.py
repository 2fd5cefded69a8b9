"""Path-traced radiance along rays from device memory (pupil_pt_radiance_rays, csrc/pt_radiance.hip)
through PTPass.radiance.

Every comparison is of bits, with no tolerance: a path started from a caller's ray runs the render's
own stages, so where the ray is the camera ray a render draws for a pixel the outputs are that
render's pixel -- the CPU oracle's and PTPass.render's.  Scenes, rays and engines are built as in
tests/test_ray_query.py."""
import contextlib
import ctypes as C
import os
import tempfile

import numpy as np
import pytest

import oracle
from pupiloptixlab_amd import World, abi, scenes
from pupiloptixlab_amd import world as W

pytestmark = pytest.mark.gpu

_TMPDIR = tempfile.TemporaryDirectory(prefix="pupil_radiance_rays_")
TMP = _TMPDIR.name
RES = 64
SEED = 3
COUNTS = [1, 63, 64, 65, 257, 1000]  # wave and block tails of the generate kernel and of the eight-shard split
SCENES = ["cornell", "materials", "instanced"]
ACCELS = ["flat", "two_level"]
FIELD = dict(num_instances=4, width=RES, height=RES, max_depth=4, seed=3, spheres_per_blas=2, slices=8, stacks=6)
OUTPUTS = ("radiance", "albedo", "normal")
# the moved and turned view of test_not_the_engines_camera: (fov, axis, origin, target)
MOVED = {"cornell": (24.0, "x", (0.6, 1.4, 5.5), (-0.1, 0.8, 0.0)),
         "materials": (24.0, "x", (0.6, 1.4, 5.5), (-0.1, 0.8, 0.0)),
         "instanced": (55.0, "y", (3.0, 7.0, 12.0), (-1.0, 4.0, 0.0))}


def _world(scene):
    if scene == "cornell":
        return World().load_scene(scenes.cornell_xml(os.path.join(TMP, "cb.xml"), RES, RES, 4))
    if scene == "materials":
        return World().load_scene(scenes.cornell_materials_xml(os.path.join(TMP, "cbm.xml"), RES, RES, 4))
    return scenes.instanced_field(**FIELD)


@contextlib.contextmanager
def _env(**values):
    old = {k: os.environ.get(k) for k in values}
    os.environ.update(values)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def _pass(world, accel, **env):
    from pupiloptixlab_amd.pt_pass import PTPass

    with _env(PUPIL_ACCEL=accel, **env):
        pt = PTPass(device=0)
        pt.set_scene(world)
    assert pt.stats()["two_level"] == (0 if accel == "flat" else 1)
    return pt


def _r8(rays6):
    n = len(rays6)
    return np.ascontiguousarray(np.concatenate([rays6, np.full((n, 1), 0.001, np.float32),
                                                np.full((n, 1), 1e16, np.float32)], 1), np.float32)


def _camera_rays(orc, desc, seed):
    return _r8(np.array([orc.camera_ray(p, seed) for p in range(desc.width * desc.height)], np.float32))


def _image(orc, **kw):
    r = orc.render(**kw)
    return {"radiance": r["accum"], "albedo": r["albedo"], "normal": r["normal"]}


class Reference:
    """What the tests of one scene share: its world, the oracle, the rays and the oracle's images.
    Computed once per scene and left unchanged."""

    def __init__(self, scene):
        self.world = _world(scene)
        self.desc = self.world.desc()
        self.oracle = oracle.OracleScene(self.desc)
        self.camera = _camera_rays(self.oracle, self.desc, SEED)
        self.image = _image(self.oracle, spp=1, random_seed=SEED, accumulate=False)
        rng = np.random.default_rng(17)
        lo, hi = ([-0.9, 0.1, -0.9], [0.9, 1.9, 0.9]) if scene != "instanced" else ([-7, 0.5, -9], [7, 13, 10])
        org = rng.uniform(lo, hi, (992, 3))
        dirs = rng.normal(size=(992, 3))
        dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
        # and 8 rays that start far above the scene and leave it: misses
        away = np.concatenate([rng.uniform(-1, 1, (8, 3)) + [0, 500, 0], np.tile([0.0, 1.0, 0.0], (8, 1))], 1)
        self.random = _r8(np.concatenate([np.concatenate([org, dirs], 1), away]).astype(np.float32))
        assert len(self.random) == 1000


_REFS, _PASSES = {}, {}


def reference(scene):
    if scene not in _REFS:
        _REFS[scene] = Reference(scene)
    return _REFS[scene]


def shared_pass(scene, accel):
    """An engine whose camera stays the scene's (radiance calls and renders leave each other alone)."""
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


def same(got, want, what):
    """got: dict of arrays; each equals want's of that name bit for bit."""
    for k, a in got.items():
        b = want[k]
        assert a.shape == b.shape, (what, k, a.shape, b.shape)
        bad = bits(a) != bits(b)
        assert not bad.any(), f"{what}: {k} differs on {int(bad.reshape(len(a), -1).any(axis=1).sum())} of {len(a)} rays"


def render_at(pt, seed):
    """PTPass.render(1) at `seed` from a fresh accumulation: accum, albedo and normal buffers."""
    import torch

    pt.dirty = False
    pt.random_seed, pt.sample_cnt = seed, 0
    pt.render(1)
    torch.cuda.synchronize()
    return {"radiance": pt.buffers.get("pt accum buffer").cpu().numpy(),
            "albedo": pt.buffers.get("albedo").cpu().numpy(), "normal": pt.buffers.get("normal").cpu().numpy()}


# ------------------------------------------------------------------ 1. camera parity
@pytest.mark.parametrize("accel", ACCELS)
@pytest.mark.parametrize("scene", SCENES)
def test_camera_rays_give_the_render(scene, accel):
    ref = reference(scene)
    pt = shared_pass(scene, accel)
    got = host(pt.radiance(dev(pt, ref.camera), spp=1, seed=SEED, want=OUTPUTS))
    assert (got["radiance"][:, 3] == 1).all()
    assert got["radiance"][:, :3].max() > 0
    same(got, ref.image, f"{scene} {accel} vs oracle")
    same(got, render_at(pt, SEED), f"{scene} {accel} vs PTPass.render")
    only = host(pt.radiance(dev(pt, ref.camera), spp=1, seed=SEED))
    assert set(only) == {"radiance"}
    same(only, ref.image, f"{scene} {accel} radiance alone")


# ------------------------------------------------------------------ 2. not the engine's camera
@pytest.mark.parametrize("accel", ACCELS)
@pytest.mark.parametrize("scene", SCENES)
def test_not_the_engines_camera(scene, accel):
    ref = reference(scene)
    fov, axis, origin, target = MOVED[scene]
    moved = _world(scene)
    moved.set_sensor(fov, W.look_at_mitsuba(origin, target, (0, 1, 0)), fov_axis=axis)
    md = moved.desc()
    assert list(md.camera_to_world) != list(ref.desc.camera_to_world)
    assert [md.camera_to_world[k] for k in (3, 7, 11)] != [ref.desc.camera_to_world[k] for k in (3, 7, 11)]
    orc = oracle.OracleScene(md)
    rays = _camera_rays(orc, md, SEED)
    want = _image(orc, spp=1, random_seed=SEED, accumulate=False)
    assert not np.array_equal(bits(want["radiance"]), bits(ref.image["radiance"]))
    pt = shared_pass(scene, accel)  # keeps the scene's own camera
    got = host(pt.radiance(dev(pt, rays), spp=1, seed=SEED, want=OUTPUTS))
    same(got, want, f"{scene} {accel} moved camera")
    orc.close()


# ------------------------------------------------------------------ 3. subsets, order and tails
@pytest.mark.parametrize("accel", ACCELS)
@pytest.mark.parametrize("scene", SCENES)
def test_subsets_in_any_order(scene, accel):
    ref = reference(scene)
    pt = shared_pass(scene, accel)
    rng = np.random.default_rng(23)
    for n in COUNTS:
        pixels = rng.permutation(RES * RES)[:n]
        got = host(pt.radiance(dev(pt, ref.camera[pixels]), spp=1, seed=SEED, want=OUTPUTS,
                               stream_ids=dev(pt, pixels.astype(np.int32))))
        same(got, {k: v[pixels] for k, v in ref.image.items()}, f"{scene} {accel} n={n}")


# ------------------------------------------------------------------ 4. samples
@pytest.mark.parametrize("accel", ACCELS)
@pytest.mark.parametrize("scene", SCENES)
def test_samples_accumulate_like_frames(scene, accel):
    ref = reference(scene)
    pt = shared_pass(scene, accel)
    rays = dev(pt, ref.random)
    once = pt.radiance(rays, spp=3, seed=SEED, accumulate=True, want=OUTPUTS)
    out = None
    for f in range(3):
        out = pt.radiance(rays, spp=1, seed=SEED + f, sample_cnt=f, accumulate=True, want=OUTPUTS, out=out)
    same(host(once), host(out), f"{scene} {accel} spp=3 vs 3 x spp=1")
    # the frames of a progressive render: each call is fed the camera rays of its own seed
    out = None
    for f in range(3):
        cam = ref.camera if f == 0 else _camera_rays(ref.oracle, ref.desc, SEED + f)
        out = pt.radiance(dev(pt, cam), spp=1, seed=SEED + f, sample_cnt=f, accumulate=True, want=OUTPUTS, out=out)
    want = _image(ref.oracle, spp=3, random_seed=SEED, accumulate=True)
    same(host(out), want, f"{scene} {accel} three frames vs oracle spp=3")


# ------------------------------------------------------------------ 5. chunks
@pytest.mark.parametrize("accel", ACCELS)
@pytest.mark.parametrize("scene", SCENES)
def test_chunk_size_changes_nothing(scene, accel):
    ref = reference(scene)
    pt = shared_pass(scene, accel)
    small = _pass(ref.world, accel, PUPIL_RADIANCE_CHUNK="256")
    try:
        ids = dev(pt, np.arange(1000, dtype=np.int32)[::-1].copy())
        kw = dict(spp=3, seed=SEED, accumulate=True, want=OUTPUTS)
        want = host(pt.radiance(dev(pt, ref.random), stream_ids=ids, **kw))
        assert small.radiance_info()["scratch_grows"] == 0
        got = host(small.radiance(dev(small, ref.random), stream_ids=ids, **kw))
        same(got, want, f"{scene} {accel} chunk 256 vs default")
        grows = small.radiance_info()["scratch_grows"]
        assert grows >= 1
        again = host(small.radiance(dev(small, ref.random), stream_ids=ids, **kw))
        same(again, want, f"{scene} {accel} chunk 256, second call")
        info = small.radiance_info()
        assert info["scratch_grows"] == grows
        assert info["calls"] == 2 and info["rays"] == 2000
        assert info["shadow_rays"] > 0 and info["extension_rays"] > 0
    finally:
        small.close_engine()


@pytest.mark.parametrize("accel", ACCELS)
def test_more_samples_than_a_chunk(accel):
    """spp above the chunk: the samples are cut into ranges that continue each other's mean."""
    ref = reference("cornell")
    pt = shared_pass("cornell", accel)
    small = _pass(ref.world, accel, PUPIL_RADIANCE_CHUNK="64")
    try:
        rays = ref.random[:33]
        for accumulate in (True, False):
            kw = dict(spp=70, seed=SEED, sample_cnt=2 if accumulate else 0, accumulate=accumulate, want=OUTPUTS)
            start = np.full((33, 4), 0.25, np.float32)
            want = host(pt.radiance(dev(pt, rays), out={"radiance": dev(pt, start)}, **kw))
            got = host(small.radiance(dev(small, rays), out={"radiance": dev(small, start)}, **kw))
            same(got, want, f"cornell {accel} spp=70 in chunks of 64, accumulate={accumulate}")
    finally:
        small.close_engine()


# ------------------------------------------------------------------ 6. rays from anywhere
@pytest.mark.parametrize("accel", ACCELS)
@pytest.mark.parametrize("scene", SCENES)
def test_rays_from_anywhere(scene, accel):
    ref = reference(scene)
    pt = shared_pass(scene, accel)
    rays = dev(pt, ref.random)
    got = host(pt.radiance(rays, spp=1, seed=SEED, want=OUTPUTS))
    normal = pt.trace(rays, want=("normal",))["normal"].cpu().numpy()
    same({"normal": got["normal"]}, {"normal": normal}, f"{scene} {accel} normal vs trace")
    assert (bits(got["albedo"][-8:]) == 0).all() and (bits(got["normal"][-8:]) == 0).all()
    assert np.isfinite(got["radiance"]).all() and (got["radiance"][:, 3] == 1).all()
    hit = np.linalg.norm(got["normal"], axis=1) > 0
    assert hit.any() and not hit[-8:].any() and got["radiance"][hit, :3].max() > 0


# ------------------------------------------------------------------ 7. leaves renders alone
@pytest.mark.parametrize("accel", ACCELS)
@pytest.mark.parametrize("scene", SCENES)
def test_renders_are_left_alone(scene, accel):
    import torch

    ref = reference(scene)

    def sequence(with_calls):
        pt = _pass(ref.world, accel)
        try:
            rays = dev(pt, ref.random)
            frames = []
            for f in range(6):
                pt.render(1, continues=True)
                torch.cuda.synchronize()
                frames.append(pt.buffers.get("pt accum buffer").cpu().numpy().copy())
                if with_calls and f < 5:
                    pt.radiance(rays, spp=2, seed=11 + f, accumulate=True, want=OUTPUTS)
            st = pt.stats()
            return frames, {k: st[k] for k in ("primary_rays", "extension_rays", "shadow_rays", "rays_traced_total")}
        finally:
            pt.close_engine()

    plain, plain_stats = sequence(False)
    mixed, mixed_stats = sequence(True)
    for f in range(6):
        assert np.array_equal(bits(plain[f]), bits(mixed[f])), f"{scene} {accel}: frame {f} differs"
    assert plain_stats == mixed_stats
    assert not np.array_equal(bits(plain[0]), bits(plain[5]))


# ------------------------------------------------------------------ another stream than the current one
@pytest.mark.parametrize("accel", ACCELS)
def test_side_stream_while_the_current_one_is_busy(accel):
    """Outputs that radiance() allocates itself are written by the call alone: nothing torch
    enqueues for them on the current stream may land after (or race) the call on `stream`.  The
    one fill there is (a mean continued without `out`) is ordered before the call."""
    import torch

    ref = reference("cornell")
    pt = shared_pass("cornell", accel)
    rays = dev(pt, ref.camera)
    cases = [dict(spp=1, seed=SEED), dict(spp=2, seed=SEED, accumulate=True),
             dict(spp=2, seed=SEED, sample_cnt=2, accumulate=True)]
    want = [host(pt.radiance(rays, want=OUTPUTS, **kw)) for kw in cases]
    same(want[0], ref.image, f"cornell {accel} same stream")
    side = torch.cuda.Stream(device=pt.device)
    a = torch.rand((4096, 4096), device=pt.device)
    torch.cuda.synchronize()
    for kw, w in zip(cases, want):
        for _ in range(12):  # a backlog on the current stream: whatever is enqueued there now runs late
            a = (a @ a).clamp_(0.0, 1.0)
        got = pt.radiance(rays, want=OUTPUTS, stream=side, **kw)
        side.synchronize()
        got = {k: v.clone() for k, v in got.items()}  # on the current stream, behind the backlog and any late fill
        torch.cuda.synchronize()
        same(host(got), w, f"cornell {accel} side stream {kw}")


# ------------------------------------------------------------------ 8. argument checks
def test_argument_checks():
    import torch

    ref = reference("cornell")
    pt = shared_pass("cornell", "flat")
    lib = pt._lib
    rays = dev(pt, ref.random[:16])
    ids = dev(pt, np.arange(16, dtype=np.int32))
    rad = torch.zeros((17, 4), dtype=torch.float32, device=pt.device)
    aov = torch.zeros((17, 3), dtype=torch.float32, device=pt.device)
    torch.cuda.synchronize()
    before = pt.radiance_info()

    def call(engine=True, n=16, rays_p=rays.data_ptr(), ids_p=ids.data_ptr(), launch=True, out=True, spp=1,
             radiance=rad.data_ptr(), albedo=aov.data_ptr(), normal=aov.data_ptr()):
        la = abi.Launch()
        la.spp = spp
        o = abi.RayRadiance(radiance, albedo, normal)
        return lib.pupil_pt_radiance_rays(pt._pt if engine else None, n, C.c_void_p(rays_p), C.c_void_p(ids_p),
                                          C.byref(la) if launch else None, C.byref(o) if out else None, None)

    refused = {
        "NULL pt": dict(engine=False), "NULL launch": dict(launch=False), "NULL out": dict(out=False),
        "NULL radiance": dict(radiance=None), "NULL rays": dict(rays_p=None), "spp = 0": dict(spp=0),
        "n = 2^31": dict(n=1 << 31), "rays off by 4 B": dict(rays_p=rays.data_ptr() + 4),
        "rays off by 8 B": dict(rays_p=rays.data_ptr() + 8), "radiance off by 4 B": dict(radiance=rad.data_ptr() + 4),
        "radiance off by 8 B": dict(radiance=rad.data_ptr() + 8), "ids off by 2 B": dict(ids_p=ids.data_ptr() + 2),
        "albedo off by 1 B": dict(albedo=aov.data_ptr() + 1), "normal off by 2 B": dict(normal=aov.data_ptr() + 2),
    }
    for what, kw in refused.items():
        assert call(**kw) == abi.ERR_INVALID, what
        assert lib.pupil_last_error(), what
    assert call(n=0) == abi.PUPIL_OK
    assert call(n=0, rays_p=None) == abi.PUPIL_OK
    torch.cuda.synchronize()
    assert pt.radiance_info() == before
    assert (rad == 0).all() and (aov == 0).all()
    # 4-B aligned AOVs and ids that are not 16-B aligned are fine
    assert call(ids_p=ids.data_ptr() + 4, n=15, albedo=aov.data_ptr() + 4, normal=aov.data_ptr() + 12) == abi.PUPIL_OK
    torch.cuda.synchronize()
    assert pt.radiance_info()["calls"] == before["calls"] + 1
    with pytest.raises(ValueError, match="spp >= 1"):
        pt.radiance(rays, spp=0)
    with pytest.raises(ValueError, match="unknown radiance output"):
        pt.radiance(rays, want=("radiance", "depth"))
    with pytest.raises(ValueError, match="stream_ids must be"):
        pt.radiance(rays, stream_ids=ids[:8])
    assert pt.radiance(rays[:0])["radiance"].shape == (0, 4)
