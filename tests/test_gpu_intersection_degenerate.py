"""The BVH4 traversal kernels at degenerate rays (tests/intersection_cases.py): direction components
of +-0 (idir = +-1e30 in visit4 and in the two-level object-space ray), rays lying in box face
planes, rays through shared edges and vertices, equal-t ties, and tmin / tmax windows between hits.

The same rays as test_intersection_degenerate.py go through pupil_pt_trace_rays, closest and any
hit, on the flattened BVH (default traversal, refill after one idle lane, refill only by whole
waves) and on the two-level structure.  The engine must equal the oracle bit for bit in all four
outputs, and -- directly, not through the oracle, which restates the same intersection routines
line by line -- agree with the float64 references; any hit must equal "a closest hit exists" under the same window.
"""
import numpy as np
import pytest

import intersection_cases as ic
import oracle
from pupiloptixlab_amd import abi

pytestmark = pytest.mark.gpu

# PUPIL_ACCEL, (PUPIL_REFILL, PUPIL_NODE_MIN) or None for the defaults
CONFIGS = [("flat", None), ("flat", ("1", "8")), ("flat", ("64", "8")), ("two_level", None)]
_IDS = ["flat", "flat-refill1", "flat-refill64", "two_level"]


def _trace_both(desc, rays):
    """Closest and any hits of rays (n, 8) on an engine of this call's own."""
    from pupiloptixlab_amd.pt_pass import PTPass

    r8 = np.ascontiguousarray(rays, np.float32).reshape(-1, 8)
    pt = PTPass(device=0)
    pt.set_scene(desc)
    outs = []
    for any_hit in (0, 1):
        out = np.full((len(r8), 4), 7.0, np.float32)
        abi.check(pt._lib.pupil_pt_trace_rays(pt._pt, len(r8), r8.ctypes.data_as(abi.f32p),
                                              out.ctypes.data_as(abi.f32p), any_hit))
        outs.append(out)
    pt.close_engine()
    return outs


_ORACLE = {}


def _oracle_answers(family):
    """The oracle's closest and any hits of a family, computed once."""
    if family not in _ORACLE:
        cs = ic.case(family)
        orc = oracle.OracleScene(cs.desc)
        _ORACLE[family] = (orc.closest(cs.rays), orc.closest(cs.rays, any_hit=True))
        orc.close()
    return _ORACLE[family]


@pytest.mark.parametrize("accel,traversal", CONFIGS, ids=_IDS)
@pytest.mark.parametrize("family", ic.FAMILIES)
def test_engine_equals_oracle_and_float64(family, accel, traversal, monkeypatch):
    monkeypatch.setenv("PUPIL_ACCEL", accel)
    if traversal:
        monkeypatch.setenv("PUPIL_REFILL", traversal[0])
        monkeypatch.setenv("PUPIL_NODE_MIN", traversal[1])
    cs = ic.case(family)
    ref, ref_any = _oracle_answers(family)
    out, occ = _trace_both(cs.desc, cs.rays)
    bad = np.flatnonzero((out.view(np.uint32) != ref.view(np.uint32)).any(axis=1))
    miss = int(((out[:, 0] > 0) != (ref[:, 0] > 0)).sum())
    print(f"{family} {accel} {traversal}: {cs.n} rays, {len(bad)} differ from the oracle ({miss} in hit / miss)")
    assert len(bad) == 0, (f"{len(bad)} of {cs.n} rays differ from the oracle ({miss} in hit / miss), e.g. ray {bad[0]} "
                           f"[{cs.tags[bad[0]]}] {cs.rays[bad[0]]}: {out[bad[0]]} vs {ref[bad[0]]}")
    assert np.array_equal(occ.view(np.uint32), ref_any.view(np.uint32)), "any-hit output differs from the oracle"
    assert np.array_equal(occ[:, 0] > 0, out[:, 0] > 0), "any-hit differs from closest under the same window"
    ic.check_closest(family, out)
    ic.check_any(family, occ)


@pytest.mark.parametrize("accel", ["flat", "two_level"])
def test_empty_and_single_ray_calls_return_cleanly(accel, monkeypatch):
    from pupiloptixlab_amd.pt_pass import PTPass

    monkeypatch.setenv("PUPIL_ACCEL", accel)
    cs = ic.case("single")
    pt = PTPass(device=0)
    pt.set_scene(cs.desc)
    empty, none = np.zeros((0, 8), np.float32), np.zeros((1, 4), np.float32)  # n = 0 reads and writes nothing
    for any_hit in (0, 1):
        abi.check(pt._lib.pupil_pt_trace_rays(pt._pt, 0, empty.ctypes.data_as(abi.f32p), none.ctypes.data_as(abi.f32p),
                                              any_hit))
        assert not none.any()
    out = np.zeros((1, 4), np.float32)
    abi.check(pt._lib.pupil_pt_trace_rays(pt._pt, 1, cs.rays.ctypes.data_as(abi.f32p), out.ctypes.data_as(abi.f32p), 0))
    pt.close_engine()
    ref, _ = _oracle_answers("single")
    assert np.array_equal(out.view(np.uint32), ref.view(np.uint32))
    ic.check_closest("single", out)
