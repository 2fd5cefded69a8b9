"""The parallel reinsertion pass over the PLOC binary tree (bvh_build.hip, PUPIL_BVH_REINSERT).

Rendering does not depend on the tree, so what is checked is the tree itself: the exported BVH4
passes the exact-bounds and coverage checks of test_bvh_invariants, two fresh engines give the
same bytes, ray-list hits equal the oracle's and those of PUPIL_BVH_REINSERT=0, the binary tree's
surface-area cost never rises from round to round (pupil_debug_bvh_reinsert), and a rebuild after
a vertex update gives the arrays of a fresh engine.  Scenes: a 4-sphere field (8 k triangles), 2 /
3 hand-placed boxes (nothing can move: the root's children stay), two 5-box layouts on which
PLOC's mutual-nearest merging is sub-optimal and one reinsertion is worth 18 % / 17 % of the
tree's cost (the smallest trees in which a move is applied), 64 identical boxes (no gain
anywhere), a 32 x 32 coplanar grid, and a two-level scene of 3 instances."""
import ctypes as C
import functools

import numpy as np
import pytest

import oracle
from pupiloptixlab_amd import abi, scenes

from test_bvh_invariants import Built, _check_hits, _leaf_size, _rays, check_bvh4
from test_visibility import _random_rays, _trace

pytestmark = pytest.mark.gpu

F32, U32 = np.float32, np.uint32
ROUNDS = 8  # rounds asked of pupil_debug_bvh_reinsert


def _env(monkeypatch, rounds=None, accel="flat"):
    monkeypatch.setenv("PUPIL_ACCEL", accel)
    for k in ("PUPIL_BVH_BUILDER", "PUPIL_BVH4_COLLAPSE", "PUPIL_SAH_LEAF", "PUPIL_FLAT_UPDATE", "PUPIL_BVH_REINSERT"):
        monkeypatch.delenv(k, raising=False)
    if rounds is not None:
        monkeypatch.setenv("PUPIL_BVH_REINSERT", str(rounds))


def _pass(world_or_desc):
    from pupiloptixlab_amd.pt_pass import PTPass

    pt = PTPass(device=0)
    pt.set_scene(world_or_desc)
    return pt


def _tri(c, e=0.05):
    c = np.asarray(c, F32)
    return np.stack([c + [-e, -e, 0], c + [e, -e, 0], c + [0, e, 0]]).astype(F32)


def _box_tri(b):
    """a triangle whose bounds are exactly the box b = (lo xyz, hi xyz)"""
    lo, hi = b[:3], b[3:]
    return np.array([[lo[0], lo[1], lo[2]], [hi[0], lo[1], hi[2]], [lo[0], hi[1], hi[2]]], F32)


# Boxes on a 1/64 grid (exact in float32), found by a search over random layouts with a host model of
# PLOC (all five boxes lie within its radius, so it is plain mutual-nearest merging whatever the
# Morton order) and of one reinsertion.  PLOC gives (((0 1) (2 3)) 4) on A and ((0 2) ((1 4) 3)) on
# B.  On A the best move takes box 0 out of (0 1) and makes it the sibling of box 4, a child of the
# root (the target's parent is the root; the removed node's grandparent is not): 18.1 % of the
# cost.  On B box 1 leaves (1 4), whose grandparent is a child of the root, for box 0 inside the
# root's other child: 16.6 %.  No move whose target is the removed node's uncle or nephew is the
# best one on any 5-box layout the search met; those relinkings occur in the larger scenes.
HAND5 = {"A": [[12, 33, 22, 14, 39, 46], [33, 27, 23, 51, 31, 27], [48, 0, 10, 60, 10, 20], [55, 9, 9, 59, 11, 23],
               [2, 50, -3, 14, 56, 19]],
         "B": [[11, 0, 45, 37, 18, 47], [16, 40, 44, 36, 52, 50], [-4, 30, 42, 14, 48, 58], [52, 5, 8, 60, 11, 10],
               [26, 41, 5, 32, 51, 15]]}
HAND5_GAIN = {"A": 0.181, "B": 0.166}  # the best single move, as a share of the PLOC tree's cost


@functools.lru_cache(maxsize=None)
def _hand(n):
    """2 / 3 small triangles; "A" / "B": the 5-box layouts above, one triangle per box"""
    if n in HAND5:
        return Built([{"tris": np.stack([_box_tri(np.array(b, F32) / 64) for b in HAND5[n]])}])
    xs = {2: [0.1, 0.9], 3: [0.1, 0.25, 0.9]}[n]
    return Built([{"tris": np.stack([_tri((x, 0.5 + 0.3 * (i % 2), 0.5)) for i, x in enumerate(xs)])}])


@functools.lru_cache(maxsize=None)
def _identical():
    return Built([{"tris": np.repeat(_tri((0.5, 0.5, 0.5), 0.2)[None], 64, axis=0)}])


@functools.lru_cache(maxsize=None)
def _grid():
    g = (np.arange(32, dtype=F32) + 0.5) / 32
    return Built([{"tris": np.stack([_tri((x, y, 0.25), 0.01) for y in g for x in g])}])


BUILT = {"hand2": lambda: _hand(2), "hand3": lambda: _hand(3), "hand5a": lambda: _hand("A"), "hand5b": lambda: _hand("B"),
         "identical64": _identical, "grid32": _grid}


def _field():
    return scenes.sphere_field(num_spheres=4, width=32, height=18, max_depth=4)


def _instanced():
    return scenes.instanced_field(num_instances=3, width=32, height=18, max_depth=4, seed=3, spheres_per_blas=4,
                                  slices=12, stacks=8)


def _desc_boxes(desc):
    """world-space boxes (n, 6) of the triangles of every mesh instance"""
    out = []
    for i in range(desc.num_instances):
        inst = desc.instances[i]
        sh = desc.shapes[inst.shape]
        if not sh.num_faces or not sh.positions or not sh.indices:
            continue
        p = np.ctypeslib.as_array(sh.positions, (sh.num_vertices, 3)).astype(np.float64)
        idx = np.ctypeslib.as_array(sh.indices, (sh.num_faces, 3))
        m = np.array(inst.to_world[:], np.float64).reshape(3, 4)
        t = (p @ m[:, :3].T + m[:, 3]).astype(F32)[idx]
        out.append(np.concatenate([t.min(axis=1), t.max(axis=1)], axis=1))
    return np.ascontiguousarray(np.concatenate(out), F32)


def _costs(boxes, rounds=ROUNDS):
    """(cost after 0 .. rounds rounds, rounds kept, rounds rejected)"""
    boxes = np.ascontiguousarray(boxes, F32)
    cost = np.zeros(rounds + 1, np.float64)
    kept, rejected = C.c_uint32(99), C.c_uint32(99)
    abi.check(abi.load_library().pupil_debug_bvh_reinsert(0, len(boxes), boxes.ctypes.data_as(abi.f32p), rounds,
                                                          cost.ctypes.data_as(C.POINTER(C.c_double)),
                                                          C.byref(kept), C.byref(rejected)))
    return cost, kept.value, rejected.value


def _export(world_or_desc):
    pt = _pass(world_or_desc)
    try:
        nodes, recs, root = pt.export_bvh4()
        return nodes.copy(), recs.copy(), root, pt.stats()
    finally:
        pt.close_engine()


def _same_tree(a, b):
    return a[2] == b[2] and np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(U32), b[1].view(U32))


# ------------------------------------------------------------------ the exported tree and the hits
@pytest.mark.parametrize("name", list(BUILT))
def test_built_scenes(name, monkeypatch):
    b = BUILT[name]()
    desc = b.world.desc()
    orc = oracle.OracleScene(desc)
    rays = _rays(b, 3, aimed=1500, random=500)
    ref = orc.closest(rays, brute_force=True)
    _env(monkeypatch, 0)
    pt0 = _pass(desc)
    try:
        hits0 = (_trace(pt0, rays), _trace(pt0, rays, any_hit=1))
        tree0 = pt0.export_bvh4()
    finally:
        pt0.close_engine()
    _env(monkeypatch)
    pt = _pass(desc)
    try:
        nodes, recs, root = pt.export_bvh4()
        check_bvh4(nodes, recs, root, orc.num_prims, _leaf_size(), stats=pt.stats())
        _check_hits(name, b, pt, rays, ref, min_unique=0.0 if name == "identical64" else 0.95)
        out = _trace(pt, rays)
        if name != "identical64":  # 64 coincident triangles tie on every hit
            assert np.array_equal(out.view(U32), hits0[0].view(U32))
        else:
            assert np.array_equal(out[:, 0].view(U32), hits0[0][:, 0].view(U32))
        occ = _trace(pt, rays, any_hit=1)
        assert np.array_equal(occ[:, [0, 3]].view(U32), hits0[1][:, [0, 3]].view(U32))
    finally:
        pt.close_engine()
    again = _export(desc)
    assert _same_tree((nodes, recs, root), again), "two fresh engines differ"
    if name == "identical64":  # all gains are zero: the tree comes back unchanged
        assert _same_tree((nodes, recs, root), tree0)


def test_sphere_field(monkeypatch):
    desc = _field().desc()
    orc = oracle.OracleScene(desc)
    rays = _random_rays(4096, [-7, 0.2, -9], [7, 13, 13], 5)
    ref, ref_any = orc.closest(rays), orc.closest(rays, any_hit=True)
    assert 0.5 < (ref[:, 0] > 0).mean()
    _env(monkeypatch, 0)
    pt0 = _pass(desc)
    try:
        hits0, occ0 = _trace(pt0, rays), _trace(pt0, rays, any_hit=1)
        tree0 = pt0.export_bvh4()
    finally:
        pt0.close_engine()
    _env(monkeypatch)
    pt = _pass(desc)
    try:
        nodes, recs, root = pt.export_bvh4()
        assert not _same_tree((nodes, recs, root), tree0), "the default rounds left the tree as PLOC built it"
        info = check_bvh4(nodes, recs, root, orc.num_prims, _leaf_size(), stats=pt.stats())
        assert info["nodes"] > 1000
        out = _trace(pt, rays)
        assert np.array_equal(out.view(U32), ref.view(U32))
        assert np.array_equal(out.view(U32), hits0.view(U32))
        occ = _trace(pt, rays, any_hit=1)
        assert np.array_equal(occ[:, [0, 3]].view(U32), ref_any[:, [0, 3]].view(U32))
        assert np.array_equal(occ[:, [0, 3]].view(U32), occ0[:, [0, 3]].view(U32))
    finally:
        pt.close_engine()
    assert _same_tree((nodes, recs, root), _export(desc)), "two fresh engines differ"


def test_two_level_three_instances(monkeypatch):
    """The two-level structure has no export: its BLAS and TLAS trees are checked through the hits
    (closest rows bit for bit against the oracle and against 0 rounds; the any-hit rows, whose
    barycentrics are those of the first occluder met and so follow the topology, between two
    fresh engines)."""
    desc = _instanced().desc()
    orc = oracle.OracleScene(desc)
    rays = _random_rays(4096, [-7, 0.2, -9], [7, 13, 13], 6)
    ref, ref_any = orc.closest(rays), orc.closest(rays, any_hit=True)

    def run():
        pt = _pass(desc)
        try:
            assert pt.stats()["two_level"] == 1
            return _trace(pt, rays), _trace(pt, rays, any_hit=1)
        finally:
            pt.close_engine()

    for mode in ("world", "object"):
        monkeypatch.setenv("PUPIL_TL_MODE", mode)
        _env(monkeypatch, 0, accel="two_level")
        out0, occ0 = run()
        _env(monkeypatch, accel="two_level")
        out, occ = run()
        out2, occ2 = run()
        assert np.array_equal(out.view(U32), ref.view(U32)), mode
        assert np.array_equal(out.view(U32), out0.view(U32)), mode
        assert np.array_equal(occ[:, [0, 3]].view(U32), ref_any[:, [0, 3]].view(U32)), mode
        assert np.array_equal(occ[:, [0, 3]].view(U32), occ0[:, [0, 3]].view(U32)), mode
        assert np.array_equal(out.view(U32), out2.view(U32)) and np.array_equal(occ.view(U32), occ2.view(U32)), mode


# ------------------------------------------------------------------ the binary tree's cost
MOVES = ("hand5a", "hand5b", "grid32", "field", "instanced")  # scenes with a positive-gain move


@pytest.mark.parametrize("name", list(BUILT) + ["field", "instanced"])
def test_cost_by_round(name):
    """The cost never rises from round to round (a round that would raise it is thrown away, and
    reported), and where a positive-gain move exists it falls strictly: the pass ran and moved
    something.  Neither is a tuned threshold.  On the 5-box layouts the first round's drop is at
    least the best single move's (the highest gain owns all of its claims), known from the host
    model to three digits; the bound leaves it 1 % of the cost of slack for float32 areas."""
    if name in BUILT:
        b = BUILT[name]()
        boxes = np.concatenate([b.lo, b.hi], axis=1)
    else:
        boxes = _desc_boxes((_field() if name == "field" else _instanced()).desc())
    cost, kept, rejected = _costs(boxes)
    print(f"reinsert {name}: n {len(boxes)} kept {kept} rejected {rejected} cost by round "
          f"{[float(f'{c:.6g}') for c in cost]}")
    assert np.isfinite(cost).all() and (cost >= 0).all()
    assert (np.diff(cost) <= 0).all(), cost
    assert rejected <= 1 and kept + rejected <= ROUNDS
    assert int((np.diff(cost) < 0).sum()) <= kept  # only a kept round changes the figure
    again = _costs(boxes)
    assert np.array_equal(cost, again[0]) and again[1:] == (kept, rejected), "the pass is not deterministic"
    assert _costs(boxes, 0)[0][0] == cost[0]
    if name in MOVES:
        assert kept >= 1 and cost[1] < cost[0], "no move was applied"
        assert cost[-1] < cost[0]
    else:
        assert kept == 0 and rejected == 0 and (cost == cost[0]).all()
    if name in ("hand5a", "hand5b"):
        assert cost[0] - cost[1] >= (HAND5_GAIN[name[-1].upper()] - 0.01) * cost[0], cost


# ------------------------------------------------------------------ rebuild after a vertex update
def test_rebuild_after_update_equals_a_fresh_engine(monkeypatch):
    _env(monkeypatch)
    w = _field()
    sh = w.desc().shapes[0]
    p = np.ctypeslib.as_array(sh.positions, (sh.num_vertices, 3)).copy()
    c = p.mean(axis=0)
    q = (c + (p - c) * np.array([1.0, 1.6, 0.7]) + [0.3, 0.0, -0.2]).astype(F32)
    pt = _pass(w)
    try:
        w.set_mesh_vertices(0, q, None)
        pt.update_shape(w, 0, rebuild=True)
        nodes, recs, root = pt.export_bvh4()
        n_prims = oracle.OracleScene(w.desc()).num_prims
        check_bvh4(nodes, recs, root, n_prims, _leaf_size(), stats=pt.stats())
    finally:
        pt.close_engine()
    w2 = _field()
    w2.set_mesh_vertices(0, q, None)
    assert _same_tree((nodes, recs, root), _export(w2)), "the rebuilt arrays differ from a fresh engine's"
