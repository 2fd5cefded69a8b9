"""The oracle's ray-scene intersection at degenerate rays (tests/intersection_cases.py): direction
components of +-0, rays in box face planes, rays through shared edges and vertices, equal-t ties
and tmin / tmax windows between hits.

For every family the oracle's BVH traversal must equal its own brute force bit for bit (closest
hits do not depend on the tree, and at a bit-equal t the lowest primitive id wins), and both must
agree with the float64 references: the same hit / miss, t within rtol 3e-5 / atol 1e-6, the
barycentrics within 1e-4, the primitive equal where the strict set has one member and inside
the tied set otherwise.  No ray is skipped; only the "equal" windows (tmax = fl(t1)) accept
either outcome for that one hit.  Test infrastructure only; CPU.
"""
import numpy as np
import pytest

import intersection_cases as ic
import oracle


@pytest.fixture(scope="module")
def oracles():
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = oracle.OracleScene(ic.case(name).desc)
        return cache[name]

    yield get
    for o in cache.values():
        o.close()


def test_case_sizes():
    """Small scenes, about 5,000 rays at most, two ray counts that are no multiple of 64, one n = 1."""
    n = {f: ic.case(f).n for f in ic.FAMILIES}
    assert max(n.values()) <= 6000, n
    assert sum(1 for v in n.values() if v % 64) >= 2 and n["single"] == 1, n
    for f in ic.FAMILIES:
        assert len(ic.case(f).tris) + len(ic.case(f).spheres) <= 1200


def test_references_are_unambiguous():
    """Hit or miss must not hang on the reference's own tolerance: every ray of the tied set has a
    member whose barycentrics are >= -1e-12 (float64 rounding of an exact edge hit), and no sphere
    root lies within a relative 1e-4 of a window edge or of tangency by less than the +-1e-3 offset."""
    for f in ic.FAMILIES:
        cs, ref = ic.case(f), ic.reference(f)
        r = cs.rays.astype(np.float64)
        if len(cs.tris):
            T, U, V, _ = ic.mt_reference(r[:, :3], r[:, 3:6], r[:, 6:8], cs.tris)
            inside = np.isfinite(T) & (np.minimum(np.minimum(U, V), 1 - U - V) >= -1e-12)
            assert np.array_equal(inside.any(1), np.isfinite(T).any(1)), f
        assert ref.hit.any() and (f in ("no_leak", "single") or (~ref.hit).any()), f


def test_every_family_has_its_cases():
    ax = ic.case("axis")
    d = ax.rays[:, 3:6]
    for k in range(3):  # both signs of zero on every axis, all six axis directions
        z = d[:, k] == 0
        assert (np.signbit(d[z, k])).any() and (~np.signbit(d[z, k])).any()
        assert (d[:, k] == 1).any() and (d[:, k] == -1).any()
    o = ax.rays[:, :3]
    on_plane = ((np.abs(o[:, 0]) == 1) & (d[:, 0] == 0)) | ((np.abs(o[:, 1]) == 1) & (d[:, 1] == 0))
    assert (on_plane & ic.reference("axis").hit).sum() > 100  # hits of rays lying in an outer bounding plane
    ties = (np.isfinite(ic.reference("axis").T) & (ic.reference("axis").T == ic.reference("axis").tmin[:, None])).sum(1)
    assert (ties >= 2).sum() > 500 and (ties == 6).sum() > 50  # shared edges and vertices
    assert ic.reference("no_leak").hit.all()
    assert set(np.unique(ic.case("window").tags)) >= {"tmax_below", "equal", "tmax_above", "tmin_between", "empty"}
    sp = ic.case("sphere")
    for pid in (0, 1):  # the answers the rays were built for, on the sphere they are aimed at
        hit = np.isfinite(ic.reference("sphere").T[:, pid])
        assert hit[sp.tags == f"graze_hit:{pid}"].all() and not hit[sp.tags == f"graze_miss:{pid}"].any()
        assert not hit[sp.tags == f"surface_out:{pid}"].any() and hit[sp.tags == f"surface_in:{pid}"].all()
        assert hit[sp.tags == f"far:{pid}"].all() and hit[sp.tags == f"centre:{pid}"].all()


@pytest.mark.parametrize("family", ic.FAMILIES)
def test_bvh_equals_brute_force_bit_for_bit(family, oracles):
    cs, orc = ic.case(family), oracles(family)
    assert orc.num_prims == len(cs.tris) + len(cs.spheres)
    bvh = orc.closest(cs.rays)
    brute = orc.closest(cs.rays, brute_force=True)
    bad = np.flatnonzero((bvh.view(np.uint32) != brute.view(np.uint32)).any(axis=1))
    miss = int(((bvh[:, 0] > 0) != (brute[:, 0] > 0)).sum())
    assert len(bad) == 0, (f"{family}: {len(bad)} of {cs.n} rays differ between the BVH and brute force "
                           f"({miss} in hit / miss), e.g. ray {bad[0]} [{cs.tags[bad[0]]}] {cs.rays[bad[0]]}: "
                           f"{bvh[bad[0]]} vs {brute[bad[0]]}")
    occ = orc.closest(cs.rays, any_hit=True)
    occ_brute = orc.closest(cs.rays, brute_force=True, any_hit=True)
    assert np.array_equal(occ.view(np.uint32), occ_brute.view(np.uint32))
    assert np.array_equal(occ[:, 0] > 0, bvh[:, 0] > 0), f"{family}: any-hit differs from closest under the same window"


@pytest.mark.parametrize("family", ic.FAMILIES)
@pytest.mark.parametrize("brute", [False, True])
def test_oracle_matches_float64(family, brute, oracles):
    cs, orc = ic.case(family), oracles(family)
    took_alt = ic.check_closest(family, orc.closest(cs.rays, brute_force=brute))
    ic.check_any(family, orc.closest(cs.rays, brute_force=brute, any_hit=True))
    assert took_alt <= int((cs.tags == "equal").sum())


def test_six_float_rays_keep_the_default_window(oracles):
    """(n, 6) rays mean tmin 0.001, tmax 1e16, as before the window argument existed."""
    cs, orc = ic.case("axis"), oracles("axis")
    assert np.all(cs.rays[:, 6] == np.float32(0.001)) and np.all(cs.rays[:, 7] == np.float32(1e16))
    assert np.array_equal(orc.closest(cs.rays[:, :6]).view(np.uint32), orc.closest(cs.rays).view(np.uint32))
    assert orc.closest(np.zeros((0, 8), np.float32)).shape == (0, 4)
