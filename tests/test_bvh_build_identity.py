"""The builder's output, byte for byte, against digests recorded before bvh_build.hip was split.

The builder is deterministic (test_bvh_reinsert: two fresh engines give the same bytes), so a
restructuring that keeps every kernel and the order of launches must reproduce the recorded trees
exactly.  tests/golden/bvh4_digests.json holds, per case, what `digest(case)` below returned on the
commit named in the file (tests/golden/make_bvh_digests.py writes it; it is not regenerated when
the builder's structure changes, only when its output is meant to change):

  tree       SHA-256 of the exported node bytes and of the record words, root link, node count and
             the 4-wide depth of stats(), flat accel, for every builder path on a 2000-triangle
             soup, the default path at the root leaf (2), the smallest tree (3) and one past the
             PLOC block (257), the scan block (1025) and the sort tile (4097), default and lbvh on
             instances + spheres and on degenerate triangles, no reinsertion, leaf size 1
  reinsert   the boxes-only driver (pupil_debug_bvh_reinsert): cost by round as float64 bits
  two_level  no export there: SHA-256 of the closest-hit rows of a fixed ray list, both TL modes
"""
import hashlib
import json
import os

import numpy as np
import pytest

from test_bvh_invariants import BUILDERS, _scene, _set_builder
from test_bvh_reinsert import _costs, _desc_boxes, _field, _instanced
from test_visibility import _random_rays, _trace

DIGESTS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bvh4_digests.json")
U32 = np.uint32
KNOBS = ("PUPIL_BVH_REINSERT", "PUPIL_BVH_REINSERT_LOG", "PUPIL_LEAF_SIZE", "PUPIL_TL_MODE")

CASES = {f"soup2000-{b}": ("tree", "soup2000", b, {}) for b in BUILDERS}
CASES.update({f"soup{n}-default": ("tree", f"soup{n}", "default", {}) for n in (2, 3, 257, 1025, 4097)})
CASES.update({f"{s}-{b}": ("tree", s, b, {}) for s in ("mixed", "degenerate") for b in ("default", "lbvh")})
CASES["soup2000-default-reinsert0"] = ("tree", "soup2000", "default", {"PUPIL_BVH_REINSERT": "0"})
CASES["soup2000-default-leaf1"] = ("tree", "soup2000", "default", {"PUPIL_LEAF_SIZE": "1"})
CASES["boxes-field"] = ("reinsert",)
CASES.update({f"two_level-{m}": ("two_level", m) for m in ("world", "object")})


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def digest(case, monkeypatch):
    """What the file records for `case`, from a fresh engine under the case's environment."""
    from pupiloptixlab_amd.pt_pass import PTPass

    kind, *arg = CASES[case]
    _set_builder(monkeypatch, "default" if kind != "tree" else arg[1])
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    if kind == "reinsert":
        cost, kept, rejected = _costs(_desc_boxes(_field().desc()))
        return {"cost_bits": [f"{int(w):016x}" for w in cost.view(np.uint64)], "kept": kept, "rejected": rejected}
    if kind == "two_level":
        monkeypatch.setenv("PUPIL_ACCEL", "two_level")
        monkeypatch.setenv("PUPIL_TL_MODE", arg[0])
        desc = _instanced().desc()
    else:
        for k, v in arg[2].items():
            monkeypatch.setenv(k, v)
        desc = _scene(arg[0]).world.desc()
    pt = PTPass(device=0)
    pt.set_scene(desc)
    try:
        if kind == "two_level":
            assert pt.stats()["two_level"] == 1
            return {"hits": _sha(_trace(pt, _random_rays(4096, [-7, 0.2, -9], [7, 13, 13], 6)).view(U32))}
        nodes, recs, root = pt.export_bvh4()
        return {"nodes": _sha(nodes), "recs": _sha(recs.view(U32)), "root": int(root), "num_nodes": len(nodes),
                "depth4": int(pt.stats()["bvh_depth"])}
    finally:
        pt.close_engine()


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(CASES))
def test_build_equals_the_recorded_digest(case, monkeypatch):
    with open(DIGESTS) as f:
        recorded = json.load(f)["cases"]
    got = digest(case, monkeypatch)
    print(f"bvh identity {case}: {got}")
    assert got == recorded[case], f"{case}: the builder's output changed\n got      {got}\n recorded {recorded[case]}"
