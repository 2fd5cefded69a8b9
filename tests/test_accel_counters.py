"""What pupil_pt_stats reports about the acceleration structure after every update path, in flat,
two-level world and two-level object mode: instance move (refit / rebuild), hide then show, shape
update (refit / PUPIL_VERTS_REBUILD).

Scene: test_deform's shared_world (two instances of one 12 x 8 UV sphere, a cube, a floor).

After every call: accel_refits advanced by exactly one, build_ms > 0, node_bound finite and
non-negative, and, after a render, 256 fixed random rays trace bit for bit like a fresh engine
created in the final state.  A refit keeps bvh_nodes / bvh_depth / two_level; a rebuild (no
instance hidden) reports those and node_bound like that fresh engine."""
import functools
import math

import numpy as np
import pytest

from pupiloptixlab_amd import world as W

from test_deform import ACCELS, _accel, _deform, _pass, shared_world, state
from test_visibility import _random_rays, _trace

pytestmark = pytest.mark.gpu

PATHS = ["move_refit", "move_rebuild", "hide_show", "shape_refit", "shape_rebuild"]
FINAL = {"move_refit": "moved", "move_rebuild": "moved", "hide_show": "none", "shape_refit": "bulge",
         "shape_rebuild": "bulge"}
TREE = ("bvh_nodes", "bvh_depth", "two_level")
MOVED = dict(scale=(0.7, 1.0, 0.9), rotate=((0, 1, 1), 55), translate=(1.1, 0.9, -0.4))


def _rays():
    return _random_rays(256, [-4, -2, -5], [4, 3, 4], 29)


def _world(final):
    w = shared_world(*state("shared", "bulge" if final == "bulge" else "none", "new"))
    if final == "moved":
        w.set_instance_transform(1, W.transform(**MOVED))
    return w


@functools.lru_cache(maxsize=None)
def _fresh(accel, final):
    """stats and hits of an engine created in the final state (the caller has set the accel mode)"""
    pt = _pass(_world(final))
    try:
        st = pt.stats()
        pt.render(1)
        return st, _trace(pt, _rays())
    finally:
        pt.close_engine()


def _steps(path, pt, w):
    """the path's update calls, one per yield"""
    if path.startswith("move"):
        w.set_instance_transform(1, W.transform(**MOVED))
        pt.update_instances(w, [1])
        yield "move"
    elif path == "hide_show":
        for mask in (0, 1):
            w.set_instance_visibility(0, mask)
            pt.update_instances(w, [0])
            yield "hide" if mask == 0 else "show"
    else:
        _deform(pt, w, "shared", "bulge", "new", rebuild=path == "shape_rebuild")
        yield "deform"


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("accel", ACCELS)
def test_counters_after_update(accel, path, monkeypatch):
    _accel(monkeypatch, accel)
    fresh_st, fresh_hits = _fresh(accel, FINAL[path])
    if path == "move_rebuild":  # the switches are read per update, not at create
        monkeypatch.setenv("PUPIL_FLAT_UPDATE", "rebuild")
        monkeypatch.setenv("PUPIL_TL_UPDATE", "rebuild")
    w = _world("none")
    pt = _pass(w)
    try:
        st0 = pt.stats()
        before = st0
        for step in _steps(path, pt, w):
            st = pt.stats()
            print(accel, path, step, {k: st[k] for k in TREE + ("node_bound", "build_ms", "accel_refits")},
                  "before", {k: st0[k] for k in TREE}, "fresh", {k: fresh_st[k] for k in TREE + ("node_bound",)})
            assert st["accel_refits"] == before["accel_refits"] + 1, step
            assert st["build_ms"] > 0.0, step
            assert all(math.isfinite(b) and b >= 0.0 for b in st["node_bound"]), (step, st["node_bound"])
            # (object mode rebuilds its TLAS over the visible instances on every instance update:
            # with instance 0 hidden it has 40 nodes on 5 levels instead of 41 on 6)
            if not path.endswith("rebuild") and (accel, step) != ("two_level_object", "hide"):
                assert [st[k] for k in TREE] == [st0[k] for k in TREE], step
            before = st
        if path.endswith("rebuild"):
            assert [st[k] for k in TREE] == [fresh_st[k] for k in TREE]
            assert st["node_bound"] == fresh_st["node_bound"]
        pt.render(1)
        out = _trace(pt, _rays())
        assert (fresh_hits[:, 0] > 0).mean() > 0.1
        assert np.array_equal(out.view(np.uint32), fresh_hits.view(np.uint32))
    finally:
        pt.close_engine()
