"""Everything an engine allocates goes with it: one engine life that touches every lazily sized
buffer -- the ring, the flow pass's scratch with previous transforms and a vertex snapshot, the
query scratch (grown once), the radiance block, the device move's staging block, replaced texels,
a replaced mesh -- run five times in one process, on the flattened BVH and the two-level structure.
The free device memory after lives 2 to 5 stays within one granule of its value after life 1; the
granule's upper bound is what the first engine's creation cost."""
import numpy as np
import pytest

from pupiloptixlab_amd import abi
from pupiloptixlab_amd import world as W

import owner_cases as cases
from material_cases import texels
from replace_mesh_cases import fixed_rays


def _life(tmp_path, free):
    """one engine life; returns the free memory before and after its creation"""
    import torch

    from pupiloptixlab_amd.pt_pass import PTPass

    w, box, inst, material = cases.cornell(tmp_path)
    pt = PTPass(device=0)
    before = free()
    pt.set_scene(w)
    created = free()
    try:
        pt.render(1, collect_stats=1)
        torch.cuda.synchronize()
        assert pt.stats()["path_samples"] == cases.SIZE * cases.SIZE
        # flow with previous transforms and one vertex snapshot
        abi.check(pt._lib.pupil_pt_snapshot_shape_vertices(pt._pt, box))
        mv = pt.motion_vectors(prev_camera=pt._cam, prev_to_world=pt.instance_transforms()[0])
        # resolved geometry without the hits: the engine's scratch holds them, and grows once
        rays = torch.from_numpy(fixed_rays(64)).to(pt.device)
        grows = pt.query_info()["scratch_grows"]
        for n in (8, 64):
            pt.trace(rays[:n].contiguous(), want=("position", "normal"))
        slot_map = 0 if pt.stats()["two_level"] else 1  # the flattened BVH's slot map counts as one growth
        assert pt.query_info()["scratch_grows"] == grows + 2 + slot_map
        pt.radiance(rays[:8].contiguous(), spp=1)
        tw = pt.instance_transforms()[0][inst:inst + 1].copy()
        tw[0, 3] += 0.05
        pt.update_instances_device(torch.from_numpy(tw).to(pt.device),
                                   ids=torch.tensor([inst], dtype=torch.int32, device=pt.device))
        w.set_material(material, W.twosided(W.diffuse(W.bitmap(texels(8, 8, 62), filter=1))))
        pt.update_material(w, material)
        cases.replace(pt, w, box, cases.box_meshes(w, box)[1])
        pt.render(1)
        torch.cuda.synchronize()
        d = w.desc()
        assert d.shapes[box].num_faces == 48
        assert pt.stats()["bvh_prims"] == sum(d.shapes[d.instances[i].shape].num_faces for i in range(d.num_instances))
        assert np.isfinite(pt.buffers.get("pt accum buffer").cpu().numpy()).all() and np.isfinite(mv.cpu().numpy()).any()
    finally:
        pt.close_engine()
    return before, created


@pytest.mark.gpu
@pytest.mark.parametrize("accel", ["flat", "two_level"])
def test_engine_lifecycle_holds_no_memory(accel, monkeypatch, tmp_path):
    import torch

    monkeypatch.setenv("PUPIL_ACCEL", accel)
    free = lambda: torch.cuda.mem_get_info(0)[0]  # noqa: E731
    after = []
    granule = 0
    for life in range(5):
        before, created = _life(tmp_path, free)
        torch.cuda.synchronize()
        after.append(free())
        if life == 0:
            granule = abs(before - created)
    print(f"{accel}: the first creation cost {granule} B; free after lives 1 to 5: {after}")
    assert granule > 0
    for f in after[1:]:
        assert abs(f - after[0]) <= granule, (after, granule)
