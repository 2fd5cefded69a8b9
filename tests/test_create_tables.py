"""The primitive -> instance tables pupil_pt_create builds, against their definition.  The update
tests compare an updated engine's tables with a fresh engine's, and both come from the same text
(host/scene_tables.h stage, pt_replace.hip's fill), so create needs a reference of its own: a numpy
restatement of what the tables are, compared exactly.

Scenes: replace_mesh_cases.world("cube") -- 6 instances, 109 primitives, guide shift 0 -- and
world("grid") -- 18,517 primitives, shift 2, the smallest scene of the suite past the guide's 8192
buckets.  Film 48 x 48; nothing is rendered."""
import numpy as np
import pytest

from pupiloptixlab_amd import abi

import replace_mesh_cases as cases
from test_replace_mesh import ACCELS, _accel

GUIDE_BUCKETS = 8192


def tables_by_definition(counts):
    """counts[i]: primitives of instance i.  prim_inst[p]: the instance holding global primitive p;
    inst_first: each instance's first primitive, then the total; inst_guide[k]: the instance holding
    primitive min(k << shift, P - 1), k = 0 .. ((P - 1) >> shift) + 1, with the smallest shift that
    leaves P >> shift <= 8192 (an empty scene: two zeros)"""
    counts = np.asarray(counts, np.int64)
    total = int(counts.sum())
    prim_inst = np.repeat(np.arange(len(counts)), counts).astype(np.uint32)
    inst_first = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint32)
    shift = 0
    while (total >> shift) > GUIDE_BUCKETS:
        shift += 1
    if total:
        k = np.arange(((total - 1) >> shift) + 2, dtype=np.int64)
        inst_guide = prim_inst[np.minimum(k << shift, total - 1)]
    else:
        inst_guide = np.zeros(2, np.uint32)
    return {"num_prims": total, "guide_shift": shift, "prim_inst": prim_inst, "inst_first": inst_first,
            "inst_guide": inst_guide}


def _counts(world):
    d = world.desc()
    shapes = [d.shapes[d.instances[i].shape] for i in range(d.num_instances)]
    return [1 if s.kind == abi.SHAPE_SPHERE else s.num_faces for s in shapes]


def test_restatement_on_small_counts():
    """by hand: empty instances share their first id with the next holder"""
    t = tables_by_definition([5, 0, 0, 7, 0, 3])
    assert t["num_prims"] == 15 and t["guide_shift"] == 0
    assert t["prim_inst"].tolist() == [0] * 5 + [3] * 7 + [5] * 3
    assert t["inst_first"].tolist() == [0, 5, 5, 5, 12, 12, 15]
    assert t["inst_guide"].tolist() == [0] * 5 + [3] * 7 + [5] * 3 + [5]
    assert tables_by_definition([])["inst_guide"].tolist() == [0, 0]


@pytest.mark.gpu
@pytest.mark.parametrize("accel", ACCELS)
@pytest.mark.parametrize("mesh,prims,shift", [("cube", 109, 0), ("grid", 109 - 24 + 2 * 9216, 2)])
def test_create_builds_the_tables_of_the_definition(accel, mesh, prims, shift, monkeypatch):
    from pupiloptixlab_amd.pt_pass import PTPass

    _accel(monkeypatch, accel)
    w = cases.world(mesh)
    ref = tables_by_definition(_counts(w))
    assert ref["num_prims"] == prims and ref["guide_shift"] == shift and len(ref["inst_first"]) == 7
    pt = PTPass(device=0)
    try:
        pt.set_scene(w)
        got = pt.prim_tables()
        assert got["num_prims"] == prims and got["guide_shift"] == shift
        for k in ("prim_inst", "inst_first", "inst_guide"):
            assert got[k].dtype == ref[k].dtype and np.array_equal(got[k], ref[k]), (accel, mesh, k)
    finally:
        pt.close_engine()
