"""The deferred shadow settle of the mixed traversal launches (pt_trace4.hip trace4_body).

A lane whose shadow ray ends unoccluded no longer adds its pending NEE term to the path's
radiance at once: the wave remembers it in a ballot mask and settles all such lanes at its next
refill, on the drained path, or after the loop.  Each path still gets exactly one `rad += sh_c`,
so the accumulation buffer must equal the oracle's bit for bit, whatever iteration the settle
runs in.  The sizes are the ones where it could go wrong: fewer rays than the refill threshold
(every settle on the drained path), exactly one wave, a second wave with one lane, and a
pipelined ring in which many waves run many refill cycles.  `continues` renders go through the
stage pipeline (k_trace4 / k_trace4tl mixed launches), not the one-launch frame kernel.
"""
import os
import tempfile

import numpy as np
import pytest

import oracle
from pupiloptixlab_amd import World, scenes
from pupiloptixlab_amd import world as W

pytestmark = pytest.mark.gpu


def _cornell(width, height, depth=4):
    with tempfile.TemporaryDirectory() as tmp:  # the XML is read at load_scene and not needed after it
        return World().load_scene(scenes.cornell_xml(os.path.join(tmp, f"cb{width}x{height}.xml"), width, height,
                                                     depth)).desc()


def _render_sequence(desc, spp, renders):
    """`renders` consecutive continued renders on one engine: the accumulation buffer after each,
    and the counters after the last."""
    import torch
    from pupiloptixlab_amd.pt_pass import PTPass

    pt = PTPass(device=0)
    pt.set_scene(desc)
    frames = []
    for _ in range(renders):
        pt.render(spp, continues=True)
        torch.cuda.synchronize()
        frames.append(pt.buffers.get("pt accum buffer").cpu().numpy())
    st = pt.stats()
    pt.close_engine()
    return frames, st


def _check_sequence(desc, spp, renders, name):
    frames, st = _render_sequence(desc, spp, renders)
    assert st["frame_launches"] == 0, "the renders must run as stage launches (mixed k_trace4)"
    o = oracle.OracleScene(desc)
    for k, got in enumerate(frames):
        r = o.render(spp=spp * (k + 1))
        assert r["stats"]["shadow_rays"] > 0
        ref = r["accum"]
        bad = (got.reshape(ref.shape).view(np.uint32) != ref.view(np.uint32)).any(axis=1)
        print(f"{name} render {k}: {int(bad.sum())}/{len(ref)} pixels differ, "
              f"max|gpu-oracle| = {np.abs(got.reshape(ref.shape) - ref).max():.3g}")
        assert not bad.any(), f"{name}: render {k}: {int(bad.sum())} pixels differ from the oracle"
    return frames, st


# A: 16 paths, fewer than the refill threshold of a wave: no refill before `drained`
# B: 64 paths, exactly one wave's worth
# C: 65 paths, a second wave with a single lane
@pytest.mark.parametrize("width,height", [(4, 4), (8, 8), (13, 5)])
def test_tiny_films_match_oracle(width, height):
    _check_sequence(_cornell(width, height), 1, 2, f"cornell{width}x{height}")


# D: the pipelined ring over three continued renders; flat BVH4 (k_trace4), the two-level world
# structure (k_trace4, TOP) and the object-space two-level kernel (k_trace4tl)
@pytest.mark.parametrize("accel", ["flat", "two_level", "two_level_object"])
def test_pipelined_ring_matches_oracle(accel, monkeypatch):
    if accel != "flat":
        monkeypatch.setenv("PUPIL_ACCEL", "two_level")
    if accel == "two_level_object":
        monkeypatch.setenv("PUPIL_TL_MODE", "object")
    _, st = _check_sequence(_cornell(64, 64), 4, 3, f"cornell64x4-{accel}")
    assert st["two_level"] == (accel != "flat")


def _floor_and_light(blocker):
    """A floor, a light facing it, the camera looking down at the floor; `blocker`: a sheet wider
    than both between them, over the camera too, so that no segment from below reaches the light."""
    w = World()
    w.set_film(8, 8, 4)
    rect = w.add_builtin("rectangle")
    grey = w.add_material(W.twosided(W.diffuse((0.6, 0.6, 0.6))))
    w.add_instance(rect, grey, W.transform(scale=(4, 4, 1), rotate=((1, 0, 0), -90), translate=(0, 0, 0)))
    if blocker:
        w.add_instance(rect, grey, W.transform(scale=(8, 8, 1), rotate=((1, 0, 0), -90), translate=(0, 2.8, 0)))
    black = w.add_material(W.twosided(W.diffuse((0.0, 0.0, 0.0))))
    w.add_instance(rect, black, W.transform(scale=(0.5, 0.5, 1), rotate=((1, 0, 0), 90), translate=(0, 3, 0)),
                   emitter_radiance=(17.0, 12.0, 4.0))
    w.set_sensor(20.0, W.look_at_mitsuba((0.0, 2.5, 2.0), (0.0, 0.0, 0.0), (0, 1, 0)), fov_axis="x")
    return w.desc()


def test_all_shadow_rays_unoccluded():
    """Only a floor and the light: every shadow ray ends unoccluded, so every lane that traced one
    owes a settle, and every pixel carries direct light."""
    frames, _ = _check_sequence(_floor_and_light(False), 1, 2, "floor+light")
    assert (frames[0][:, :3].sum(axis=1) > 0).all()


def test_all_shadow_rays_occluded():
    """A blocker between the floor and the light: no shadow ray ends unoccluded, no lane owes a
    settle, and no light arrives anywhere."""
    frames, _ = _check_sequence(_floor_and_light(True), 1, 2, "floor+blocker+light")
    assert (frames[-1][:, :3] == 0).all()


def test_deferred_lanes_are_counted_once():
    """A counter render: per launch, items handed out = lanes activated = lanes retired = the
    list length (counters[20..23]), so a lane that waits for its settle is still retired once."""
    from pupiloptixlab_amd.pt_pass import PTPass

    pt = PTPass(device=0)
    pt.set_scene(_cornell(64, 64))
    pt.render(4, collect_stats=1)
    c = pt.stats()
    pt.close_engine()
    rays = c["primary_rays"] + c["extension_rays"] + c["shadow_rays"]
    print(f"rays {rays}: handed {c['queue_handed']} activated {c['queue_activated']} "
          f"retired {c['queue_retired']} listed {c['queue_listed']}")
    assert c["shadow_rays"] > 0
    assert (c["queue_handed"], c["queue_activated"], c["queue_retired"], c["queue_listed"]) == (rays,) * 4, c
