"""The two-level world structure against exact bounds, after every update path.

CPU: `check_world_bvh4` (world_bvh_cases.py) accepts a hand-built structure encoded by
bvh4_quant.h on the host and rejects each subtle mutation of it with the invariant's own tag.

GPU: one small scene (four cubes, four tessellated spheres, two built-in spheres; skew
rotations, a (3, 0.2, 1) scale, a mirror, a translation by 1e4, a coincident pair) is driven
through every update path in one chain per parameter combination; after each step the structure
is read back (PTPass.export_world_bvh4) and checked, its records against a fresh flattened engine
of the same scene.  After the last step 2 000 rays are compared with the oracle's brute force.
"""
import contextlib
import os
import time

import numpy as np
import pytest

import oracle
from pupiloptixlab_amd import abi
from test_bvh_invariants import EMPTY_LINK, F32, U32, BvhViolation, _check_hits, _leaf_size, _rays, _run_quantiser, make_leaf
from world_bvh_cases import T, VERT, WorldScene, check_world_bvh4, hand_world, icosahedron


# ------------------------------------------------------------------ CPU: the checker on a hand-built structure
def _host_encoder(tmp_path):
    """encode(list of (child boxes, links)) -> 16-word nodes, each axis by bvh4_quant.h on the host"""

    def encode(nodes):
        cases = []
        for boxes, _ in nodes:
            lo = np.min([b[0] for b in boxes], axis=0).astype(F32)
            hi = np.max([b[1] for b in boxes], axis=0).astype(F32)
            for a in range(3):
                cases.append((4, lo[a], hi[a], np.array([b[0][a] for b in boxes], F32), np.array([b[1][a] for b in boxes], F32)))
        got = _run_quantiser(tmp_path, cases)
        out = []
        for j, (boxes, links) in enumerate(nodes):
            w = np.zeros(16, U32)
            for a in range(3):
                org, e, qa, qb = got[3 * j + a]
                w[a] = np.array([org], F32).view(U32)[0]
                w[(3, 14, 15)[a]] = e << 23
                w[8 + a] = sum(q << (8 * k) for k, q in enumerate(qa))
                w[11 + a] = sum(q << (8 * k) for k, q in enumerate(qb))
            for k in range(4):
                w[4 + k] = (links[k] if k < len(links) else EMPTY_LINK) & 0xFFFFFFFF
            out.append(w)
        return out

    return encode


@pytest.fixture(scope="module")
def hand(tmp_path_factory):
    enc = _host_encoder(tmp_path_factory.mktemp("quant"))
    return {(mode, hid): hand_world(enc, hidden_b=hid, mode=mode)
            for mode, hid in (("built", False), ("refit", False), ("refit", True))}


def _copy(h):
    exp, insts, stats = h
    exp = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in exp.items()}
    return exp, [dict(i) for i in insts], dict(stats)


def test_checker_accepts_the_hand_built_structure(hand):
    for (mode, hid), h in hand.items():
        exp, insts, stats = _copy(h)
        info = check_world_bvh4(exp, insts, tlas=mode, stats=stats, max_leaf=1)
        assert info["nodes"] == 3 and info["leaves"] == 5 and info["unreached"] == 1
        assert 0 < info["slack_s"] <= 2.0
        if mode == "built":  # the decoded entry boxes sit up to 2 s of the copy node outside the exact ones
            assert info["tlas_slack_exact_s"] > 0


def _words(exp):
    return exp["nodes"].view("<u4").reshape(-1, 16)


def _set_planes(w, node, k, src=None):
    """child k of `node` gets the planes of child `src`, or the empty bytes lo 255 / hi 0"""
    for a in range(3):
        for word, empty in ((8 + a, 255), (11 + a, 0)):
            v = int(w[node, word])
            q = empty if src is None else (v >> (8 * src)) & 255
            w[node, word] = (v & ~(255 << (8 * k)) & 0xFFFFFFFF) | (q << (8 * k))


def _scale_records(exp, inst, f):
    r = exp["recs"]
    rows = np.nonzero(r.view(U32)[:, 7] == inst)[0]
    rows = rows[r.view(U32)[rows, 3] != 0xFFFFFFFF]
    v = r[rows][:, VERT].reshape(-1, 3).astype(np.float64)
    c = v.mean(axis=0)
    r[np.ix_(rows, VERT)] = ((v - c) * f + c).astype(F32).reshape(len(rows), 9)


def _mutants():
    def hi_plane_down(exp, insts):
        w = _words(exp)
        assert (w[4, 11] & 255) > 0
        w[4, 11] -= 1  # B's copy node, child 0, x hi plane: the smallest q that encloses, one quantum down

    def records_grown(exp, insts):
        _scale_records(exp, 1, 1.5)  # B moved (scaled about its centre), every box left alone

    def records_shrunk(exp, insts):
        _scale_records(exp, 1, 0.5)

    def leaf_of_the_other_instance(exp, insts):
        _words(exp)[3, 4] = make_leaf(4, 1) & 0xFFFFFFFF  # A's copy node names B's first record
        _words(exp)[1, 4] = make_leaf(4, 1) & 0xFFFFFFFF  # and so does the entry the TLAS holds for it

    def reserve_linked(exp, insts):
        w = _words(exp)
        w[0, 6] = 2
        _set_planes(w, 0, 2, src=0)  # planes of child 0 for the new child, so that only the link is wrong

    def duplicated_id(exp, insts):
        exp["recs"].view(U32)[2, 3] = 0  # A's second triangle carries the first one's global id

    def hidden_but_finite(exp, insts):
        insts[1]["hidden"] = True

    def unowned_slot(exp, insts):
        w = _words(exp)
        w[1, 5] = EMPTY_LINK  # the entry for A's second leaf is gone
        _set_planes(w, 1, 1)

    def entry_reached_twice(exp, insts):
        w = _words(exp)
        w[0, 6] = 4  # B's copy root, also under node 1
        _set_planes(w, 0, 2, src=0)

    return [(hi_plane_down, "enclosure"), (records_grown, "enclosure"), (records_shrunk, "tightness"),
            (leaf_of_the_other_instance, "leaves"), (reserve_linked, "reachability"), (duplicated_id, "leaves"),
            (hidden_but_finite, "hidden"), (unowned_slot, "leaves"), (entry_reached_twice, "reachability")]


@pytest.mark.parametrize("mode", ["built", "refit"])
@pytest.mark.parametrize("mutate,invariant", _mutants(), ids=[m.__name__ for m, _ in _mutants()])
def test_checker_rejects_each_mutation(hand, mutate, invariant, mode):
    exp, insts, stats = _copy(hand[(mode, False)])
    mutate(exp, insts)
    with pytest.raises(BvhViolation) as e:
        check_world_bvh4(exp, insts, tlas=mode, max_leaf=1)
    assert f"[{invariant}]" in str(e.value), str(e.value)


def test_checker_rejects_a_hidden_instance_that_widens_a_plane(hand):
    """B hidden: its planes 255 / 0 in node 1 pass; any other byte there, or a finite origin kept in
    its own emptied copy node, is rejected, and so are wrong statistics."""
    exp, insts, stats = _copy(hand[("refit", True)])
    _words(exp)[1, 11] |= 1 << 16  # child 2 (B) of node 1: x hi plane 1 instead of 0
    with pytest.raises(BvhViolation, match=r"\[hidden\]"):
        check_world_bvh4(exp, insts, tlas="refit", max_leaf=1)
    exp, insts, stats = _copy(hand[("refit", True)])
    _words(exp)[4, 0] = np.array([1.0], F32).view(U32)[0]
    with pytest.raises(BvhViolation, match=r"\[hidden\]"):
        check_world_bvh4(exp, insts, tlas="refit", max_leaf=1)
    exp, insts, stats = _copy(hand[("refit", False)])
    for key, val in (("bvh_nodes", 5), ("node_bound", [stats["node_bound"][0] * 2.0] + stats["node_bound"][1:])):
        with pytest.raises(BvhViolation, match=r"\[statistics\]"):
            check_world_bvh4(exp, insts, tlas="refit", stats=dict(stats, **{key: val}), max_leaf=1)


def test_checker_ends_on_cyclic_links_among_unreached_nodes(hand):
    """Copy nodes a refit never wrote hold whatever the allocation held: links that form cycles
    must be reported as orphans, not followed forever."""
    exp, insts, stats = _copy(hand[("built", False)])
    nodes = np.concatenate([exp["nodes"]] + [exp["nodes"][3:4]] * 40)  # 40 more unreached copy nodes
    w = nodes.view("<u4").reshape(-1, 16)
    for j in range(5, len(w)):
        w[j, 4:8] = [5 + (j - 5 + d) % 40 for d in (0, 1, 7, 13)]  # every node links four of them, itself included
    exp["nodes"] = nodes
    with pytest.raises(BvhViolation, match=r"\[reachability\]"):
        check_world_bvh4(exp, insts, tlas="built", max_leaf=1)


def test_checker_compares_records_with_the_flat_export(hand):
    exp, insts, stats = _copy(hand[("refit", False)])
    flat = exp["recs"][[6, 0, 4, 2, 8]].copy()  # any slot order: matched by global id
    check_world_bvh4(exp, insts, flat_recs=flat, tlas="refit", max_leaf=1)
    flat[1, 5] = np.nextafter(flat[1, 5], F32(9.0))
    with pytest.raises(BvhViolation, match=r"\[records\]"):
        check_world_bvh4(exp, insts, flat_recs=flat, tlas="refit", max_leaf=1)


# ------------------------------------------------------------------ GPU: every update path
@contextlib.contextmanager
def _env(**kv):
    old = {k: os.environ.get(k) for k in kv}
    try:
        for k, v in kv.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _flat_records(world):
    """the record slots of a fresh flattened engine of the world as it is now"""
    from pupiloptixlab_amd.pt_pass import PTPass

    with _env(PUPIL_ACCEL="flat", PUPIL_FLAT_UPDATE=None):
        pt = PTPass(device=0)
        pt.set_scene(world.desc())
        try:
            return pt.export_bvh4()[1]
        finally:
            pt.close_engine()


class Chain:
    """One two-level engine on the WorldScene; check() after each step collects the violations, so
    that one run shows every step that fails."""

    def __init__(self, monkeypatch, braid, leaf, update):
        from pupiloptixlab_amd.pt_pass import PTPass

        monkeypatch.setenv("PUPIL_ACCEL", "two_level")
        monkeypatch.setenv("PUPIL_TL_BRAID", str(braid))
        monkeypatch.setenv("PUPIL_TL_UPDATE", update)
        for k in ("PUPIL_TL_MODE", "PUPIL_TL_BUILDER", "PUPIL_DEBUG_TL_FALLBACK", "PUPIL_LEAF_SIZE"):
            monkeypatch.delenv(k, raising=False)
        if leaf:
            monkeypatch.setenv("PUPIL_LEAF_SIZE", str(leaf))
        self.after_update = "refit" if update == "refit" else "built"
        self.sc = WorldScene()
        self.pt = PTPass(device=0)
        self.pt.set_scene(self.sc.world.desc())
        self.failed = []
        self.tag = f"braid {braid} leaf {leaf or 'default'} {update}"

    def check(self, step, tlas):
        exp = self.pt.export_world_bvh4()
        assert exp is not None, "the engine did not build the world-mode two-level structure"
        try:
            info = check_world_bvh4(exp, self.sc.table(self.pt), flat_recs=_flat_records(self.sc.world), tlas=tlas,
                                    stats=self.pt.stats(), max_leaf=_leaf_size())
            print(f"world bvh4 [{self.tag}] {step}: tlas {tlas} nodes {info['nodes']} leaves {info['leaves']} "
                  f"unreached {info['unreached']} slack {info['slack_s']:.3f} s, built TLAS to exact {info['tlas_slack_exact_s']:.3f} s")
        except BvhViolation as e:
            print(f"world bvh4 [{self.tag}] {step}: {e}")
            self.failed.append(f"{step}: {e}")

    def finish(self):
        assert not self.failed, f"{len(self.failed)} step(s) failed:\n" + "\n".join(self.failed)

    # the update paths
    def host(self, ids):
        self.pt.update_instances(self.sc.world, ids)

    def device(self, ids, xfs):
        """ids may repeat (each repeat with the same matrix)"""
        import torch

        for k, x in zip(ids, xfs):
            self.sc.move(k, x)
        tw = torch.tensor(np.stack([np.asarray(x, F32)[:3].reshape(12) for x in xfs]), device="cuda:0")
        self.pt.update_instances_device(tw, torch.tensor(ids, dtype=torch.int32, device="cuda:0"))

    def show(self, ids, vis):
        for k in ids:
            self.sc.show(k, vis)
        self.host(ids)


PARAMS = [(b, l, u) for b in (0, 2, 10) for l in (1, None) for u in ("refit", "rebuild")]


@pytest.mark.gpu
@pytest.mark.parametrize("braid,leaf,update", PARAMS, ids=[f"braid{b}-leaf{l or 'default'}-{u}" for b, l, u in PARAMS])
def test_every_update_path_keeps_the_world_structure_exact(braid, leaf, update, monkeypatch):
    import torch

    t0 = time.perf_counter()
    c = Chain(monkeypatch, braid, leaf, update)
    sc, pt, U = c.sc, c.pt, c.after_update
    try:
        # 1. fresh build
        c.check("1 fresh build", "built")
        # 2. host updates: one instance, then all in one call
        sc.move(1, T(scale=(3.0, 0.2, 1.0), rotate=((1, 0, 2), 110.0), translate=(5.0, -1.0, 2.0)))
        c.host([1])
        c.check("2a host update of one instance", U)
        for k in range(len(sc.inst)):
            kk = 4 if k == 5 else k  # 4 and 5 stay coincident
            sc.move(k, T(rotate=((2, 3, -1), 17.0 + 5.0 * kk), translate=(0.5, 0.25 * kk, -0.5)) @ sc.inst[k]["xf"])
        c.host(list(range(len(sc.inst))))
        c.check("2b host update of all instances", U)
        home = [i["xf"].copy() for i in sc.inst]
        # 3. device update with a repeated id, then the same instances back
        there = [T(rotate=((1, 1, 0), 80.0), translate=(-4.0, 0.0, 3.0)) @ home[k] for k in (2, 5, 8)]
        c.device([2, 5, 8, 2], there + [there[0]])
        c.check("3a device update, id list with a repeat", U)
        c.device([2, 5, 8], [home[2], home[5], home[8]])
        c.check("3b device update back", U)
        # 4. shrink, then grow
        small = home[6] @ T(scale=(0.05, 0.05, 0.05))
        sc.move(6, small)
        c.host([6])
        c.check("4a instance shrunk by 0.05", U)
        sc.move(6, small @ T(scale=(20.0, 20.0, 20.0)))
        c.host([6])
        c.check("4b instance grown by 20", U)
        # 5. visibility
        c.show([0], False)
        c.check("5a one instance hidden", U)
        cubes = sc.of_shape("cube")
        c.show(cubes, False)
        c.check("5b every instance of one shape hidden", U)
        c.show(cubes, True)
        c.check("5c shown again", U)
        c.show([6], False)
        sc.move(6, T(translate=(0.0, 6.0, 0.0)) @ home[6])
        c.host([6])
        c.check("5d hidden instance moved", U)
        c.show([6], True)
        c.check("5e moved instance shown", U)
        c.show([7], False)
        pt.update_shape(sc.world, sc.shape["tess"], rebuild=True)  # builds the TLAS topology without instance 7
        c.check("5f structure rebuilt with an instance hidden", "built")
        c.show([7], True)  # not in the topology: a build, whatever PUPIL_TL_UPDATE says
        c.check("5g instance shown that the topology lacked", "built")
        # 6. the instance table as a whole: two added, three removed, then a reorder
        sc.add("tess", T(scale=(0.5, 0.5, 0.5), rotate=((0, 1, 1), 15.0), translate=(3.0, 3.0, -3.0)))
        sc.add("sphere", T(scale=(0.4, 0.4, 0.9), rotate=((1, 0, 1), 70.0), translate=(-4.0, 1.0, 1.0)))
        pt.set_instances(sc.world)
        c.check("6a two instances added", "built")
        for k in (8, 2, 0):
            sc.remove(k)
        pt.set_instances(sc.world)
        c.check("6b three instances removed", "built")
        moved = sc.remove(1)
        sc.add(moved["shape"], moved["xf"])
        first = sc.remove(0)
        sc.add(first["shape"], first["xf"])
        pt.set_instances(sc.world)
        c.check("6c instances reordered", "built")
        # 7. deform the tessellated shape: from host memory, then from device memory with a larger vmax
        p0 = sc.mesh["tess"][0]
        sc.set_vertices("tess", p0 * F32(0.8) + F32(0.1) * np.sin(7.0 * p0[:, [1, 2, 0]]).astype(F32))
        pt.update_shape(sc.world, sc.shape["tess"])
        c.check("7a vertices from host memory", U)
        big = (p0 * np.array([2.5, 1.0, 0.6], F32) + np.array([0.0, 3.0, 0.0], F32)).astype(F32)
        sc.set_vertices("tess", big)
        pt.update_shape_device(sc.shape["tess"], torch.tensor(big, device="cuda:0").contiguous())
        c.check("7b vertices from device memory, vmax enlarged", U)
        # 8. the cube replaced by a mesh of other topology
        sc.set_mesh("cube", *icosahedron())
        pt.replace_shape(sc.shape["cube"], *icosahedron())
        c.check("8 cube replaced by 20 triangles", "built")
        # 9. stale entries, then a forced TLAS build
        lacking = sc.of_shape("cube")[0]
        mover = sc.of_shape("tess")[1]
        c.show([lacking], False)
        pt.update_shape(sc.world, sc.shape["tess"], rebuild=True)  # a topology without `lacking`
        c.device([mover], [T(rotate=((3, -1, 1), 45.0), translate=(-2.0, 2.0, 5.0)) @ sc.inst[mover]["xf"]])
        c.check("9a device move leaves its entries stale", U)
        c.show([lacking], True)
        c.check("9b instance shown that the topology lacked: a build over the stale entries", "built")
        c.finish()
        # rays after the most-mutated state, against brute force
        b = sc.built()
        rays = _rays(b, 9, 1500, 500)
        ref = oracle.OracleScene(sc.world.desc()).closest(rays, brute_force=True)
        hits, share = _check_hits("world chain", b, pt, rays, ref, min_unique=0.0)
        assert hits > 700
        print(f"world bvh4 [{c.tag}]: {hits} hits, {share:.3f} unique, {time.perf_counter() - t0:.2f} s")
    finally:
        pt.close_engine()


@pytest.mark.gpu
def test_world_export_error_handling(monkeypatch):
    """UNSUPPORTED for the flattened BVH and for object mode, INVALID for NULL count pointers, and
    the counts-only call agrees with the full one."""
    import ctypes as C

    from pupiloptixlab_amd.pt_pass import PTPass

    sc = WorldScene()
    lib = abi.load_library()
    for env in ({"PUPIL_ACCEL": "flat"}, {"PUPIL_ACCEL": "two_level", "PUPIL_TL_MODE": "object"},
                {"PUPIL_ACCEL": "two_level", "PUPIL_TL_MODE": "world"}):
        for k in ("PUPIL_ACCEL", "PUPIL_TL_MODE", "PUPIL_TL_BRAID"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        pt = PTPass(device=0)
        pt.set_scene(sc.world.desc())
        try:
            nn, nr, ni = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
            counts = (C.byref(nn), None, C.byref(nr), None, C.byref(ni), None, None, None, None, None)
            rc = lib.pupil_debug_export_world_bvh4(pt._pt, *counts)
            if env.get("PUPIL_TL_MODE") != "world":
                assert rc == abi.ERR_UNSUPPORTED and pt.export_world_bvh4() is None
                continue
            assert rc == 0
            assert pt.export_bvh4() is None  # pupil_pt_export_bvh4 still declines the two-level structure
            for k in (0, 2, 4):
                args = list(counts)
                args[k] = None
                assert lib.pupil_debug_export_world_bvh4(pt._pt, *args) == abi.ERR_INVALID
            exp = pt.export_world_bvh4()
            assert (len(exp["nodes"]), len(exp["recs"]), len(exp["boxes"])) == (nn.value, nr.value, ni.value)
            assert ni.value == len(sc.inst) and exp["tlas_nodes"] <= exp["tlas_cap"] <= nn.value and exp["braid"] == 10
            small = C.c_uint32(nn.value - 1)  # an array shorter than the count is refused, nothing written
            buf = np.zeros((nn.value, 64), np.uint8)
            assert lib.pupil_debug_export_world_bvh4(pt._pt, C.byref(small), buf.ctypes.data_as(C.c_void_p), C.byref(nr), None,
                                                     C.byref(ni), None, None, None, None, None) == abi.ERR_INVALID
            assert not buf.any()
        finally:
            pt.close_engine()
