"""The exported BVH4 against an exact bounds reference, on every builder path.

A BVH is correct only if every child box encloses everything under it.  `check_bvh4` decodes the
arrays of `PTPass.export_bvh4()` (pt_scene.h Bvh4Node, kRecF4 record slots) in numpy and checks,
with no tolerance anywhere:

  1. topology     every node but the root referenced once, leaves own disjoint even-aligned slot
                  ranges, every primitive id in exactly one leaf, empty slots carry the empty bytes
  2. enclosure    float32(o + q s) brackets the min/max of the record vertices under each child
  3. origin/scale o is the float32 minimum of the children's lows bit for bit; s is a normal power
                  of two with s <= 4 ext / 254 (ceil(log2) < 2x, one retry doubling).  A normal
                  float cannot be smaller than 2^-126, so the bound is max(4 ext / 254, 2^-126).
  4. tightness    every decoded plane within 2 s + one ulp (of the plane value) of its bound
  5. statistics   bvh_nodes, bvh_depth (4-wide levels; 1 when the root is a leaf) and node_bound

The CPU tests mutate a hand-built tree to show the checker rejects a subtly wrong builder, and
run bvh4_quant.h on the host.  The GPU tests build awkward scenes on every builder path, check the
exported arrays and compare traced hits with the oracle's brute force (no BVH of its own).

Hit ties: where several primitives hit at the reference t (duplicates, coplanar overlaps) only t is
compared bit for bit; the id and barycentrics are compared where the reference hit is unique, which
a float64 restatement decides from the scene geometry alone (`_unique_hits`).  The coincident case
(300 copies of one triangle) has no unique hit by construction and is exempt from the 95 % share.
"""
import functools
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import oracle
from pupiloptixlab_amd import World, abi
from pupiloptixlab_amd import world as world_mod

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pupiloptixlab_amd", "csrc")
F32, F64, U32 = np.float32, np.float64, np.uint32
EMPTY_LINK = 0x7FFFFFFF
TRAVERSE_DONE = 0x76543210
HOLE = 0xFFFFFFFF
SPHERE_BIT = 0x80000000
S_MIN = 2.0 ** -126
AXES = "xyz"


class BvhViolation(AssertionError):
    pass


def _bits(x):
    return np.ascontiguousarray(x, F32).view(U32)


def _ulp(x):
    return np.spacing(np.abs(np.asarray(x, F32))).astype(F64)


def make_leaf(first, count):
    return ~((first << 3) | (count - 1))


def _decode_nodes(nodes):
    w = np.ascontiguousarray(nodes, np.uint8).reshape(-1, 64).view("<u4").reshape(-1, 16)
    o = np.ascontiguousarray(w[:, 0:3]).view(F32)
    s = np.ascontiguousarray(w[:, [3, 14, 15]]).view(F32)
    child = np.ascontiguousarray(w[:, 4:8]).view(np.int32)
    sh = (8 * np.arange(4, dtype=U32))[None, None, :]
    qlo = (w[:, 8:11, None] >> sh) & 255  # (n, axis, child)
    qhi = (w[:, 11:14, None] >> sh) & 255
    return o, s, child, qlo, qhi


def _record_boxes(recs):
    rf = np.ascontiguousarray(recs, F32).reshape(-1, 12)
    rw = rf.view(U32)
    ids = rw[:, 3].copy()
    live = ids != HOLE
    with np.errstate(invalid="ignore"):
        v = rf[:, [0, 1, 2, 4, 5, 6, 8, 9, 10]].reshape(-1, 3, 3)
        lo, hi = v.min(axis=1), v.max(axis=1)
        sph = live & ((ids & SPHERE_BIT) != 0)
        lo[sph] = rf[sph, 0:3] - rf[sph, 4:7]  # float32, as k_refit_level evaluates c -+ e
        hi[sph] = rf[sph, 0:3] + rf[sph, 4:7]
    return ids, live, lo, hi


def _check_planes(idx, o, s, qlo, qhi, used, clo, chi, nlo, nhi, fail, info, scale_bound=True,
                  parts=("enclosure", "origin/scale", "tightness")):
    """Invariants 2-4 of check_bvh4 on decoded nodes, one row per node; idx names the rows in the
    messages.  used (n, 4) marks the children to check, clo / chi (n, 3, 4) are their reference
    boxes and nlo / nhi (n, 3) the nodes'.  Updates info's slack_s / excess_s."""
    u = used[:, None, :] & np.ones((1, 3, 1), bool)
    with np.errstate(invalid="ignore", over="ignore"):
        dlo = o[:, :, None] + qlo.astype(F32) * s[:, :, None]  # float32: q s exact, one rounding
        dhi = o[:, :, None] + qhi.astype(F32) * s[:, :, None]
    assert dlo.dtype == F32 and dhi.dtype == F32

    def where(m):
        j, a, k = (int(x[0]) for x in np.nonzero(m))
        return j, a, k, f"node {idx[j]} child {k} axis {AXES[a]} (o {o[j, a]!r}, s {s[j, a]!r}, q {qlo[j, a, k]}..{qhi[j, a, k]})"

    if "enclosure" in parts:  # ---- 2. enclosure
        m = u & ~(dlo <= clo)
        if m.any():
            j, a, k, w = where(m)
            fail("enclosure", f"{w}: decoded lo {dlo[j, a, k]!r} > reference {clo[j, a, k]!r}; {m.sum()} planes")
        m = u & ~(dhi >= chi)
        if m.any():
            j, a, k, w = where(m)
            fail("enclosure", f"{w}: decoded hi {dhi[j, a, k]!r} < reference {chi[j, a, k]!r}; {m.sum()} planes")
    if "origin/scale" in parts:  # ---- 3. origin and scale
        m = _bits(o) != _bits(nlo)
        if m.any():
            j, a = (int(x[0]) for x in np.nonzero(m))
            fail("origin/scale", f"node {idx[j]} axis {AXES[a]}: origin {o[j, a]!r} is not the children's minimum "
                                 f"{nlo[j, a]!r}; {m.sum()} origins")
        sb = _bits(s)
        ex = (sb >> 23) & 0xFF
        m = ((sb & 0x807FFFFF) != 0) | (ex == 0) | (ex == 255)
        if m.any():
            j, a = (int(x[0]) for x in np.nonzero(m))
            fail("origin/scale", f"node {idx[j]} axis {AXES[a]}: scale bits {sb[j, a]:#010x} are no normal power of two")
        with np.errstate(invalid="ignore"):
            ext = nhi.astype(F64) - nlo.astype(F64)
        if scale_bound:
            m = (ext > 0) & (s.astype(F64) > np.maximum(4.0 * ext / 254.0, S_MIN))
            if m.any():
                j, a = (int(x[0]) for x in np.nonzero(m))
                fail("origin/scale", f"node {idx[j]} axis {AXES[a]}: scale {s[j, a]!r} > 4 ext / 254 with ext {ext[j, a]!r} "
                                     f"(ratio {s[j, a] * 254.0 / ext[j, a]:.3f}); {m.sum()} scales")
    if "tightness" in parts:  # ---- 4. tightness
        s3 = s.astype(F64)[:, :, None] * np.ones((1, 1, 4))
        with np.errstate(invalid="ignore", over="ignore"):
            for dec, ref, side in ((dlo, clo, "lo"), (dhi, chi, "hi")):
                slack = np.abs(ref.astype(F64) - dec.astype(F64))
                ulp = _ulp(np.maximum(np.abs(dec), np.abs(ref)))
                ok = u & np.isfinite(slack)
                if ok.any():
                    info["slack_s"] = max(info["slack_s"], float((slack[ok] / s3[ok]).max()))
                    info["excess_s"] = max(info["excess_s"], float(((slack[ok] - ulp[ok]) / s3[ok]).max()))
                m = u & ~(slack <= 2.0 * s3 + ulp)
                if m.any():
                    j, a, k, w = where(m)
                    fail("tightness", f"{w}: decoded {side} {dec[j, a, k]!r} is {slack[j, a, k] / s3[j, a, k]:.3f} s from "
                                      f"{ref[j, a, k]!r} (limit 2 s + ulp {ulp[j, a, k]!r}); {m.sum()} planes")


def check_bvh4(nodes, recs, root, n_prims, leaf_size, sah_leaf=None, refit=False, stats=None):
    """Raises BvhViolation naming the invariant; returns dict(nodes, depth, leaves, slack_s, excess_s):
    slack_s the largest plane-to-bound distance in units of s, excess_s the same after one ulp."""
    max_leaf = max(int(leaf_size), int(sah_leaf or 0))
    n = len(nodes)
    o, s, child, qlo, qhi = _decode_nodes(nodes) if n else (np.zeros((0, 3), F32),) * 2 + (np.zeros((0, 4), np.int32),) * 3
    ids, live, rlo, rhi = _record_boxes(recs)
    nrec = len(ids) if n_prims else 0
    bad = []

    def fail(kind, msg):
        bad.append(f"[{kind}] {msg}")

    def done():
        if bad:
            raise BvhViolation(f"{len(bad)} violation(s):\n" + "\n".join(bad[:12]))

    # ---- 1. topology
    owned = np.zeros(max(nrec, 1), bool)
    seen = []

    def leaf(link, where):
        v = (~int(link)) & 0xFFFFFFFF
        first, count = v >> 3, (v & 7) + 1
        span = (count + 1) & ~1
        if first % 2 or first + span > nrec:
            return fail("topology", f"{where}: leaf slots [{first}, {first + span}) odd or beyond {nrec} records")
        if count > max_leaf:
            fail("topology", f"{where}: leaf of {count} primitives, limit {max_leaf}")
        if owned[first:first + span].any():
            fail("topology", f"{where}: leaf slots [{first}, {first + span}) overlap another leaf")
        owned[first:first + span] = True
        if not live[first:first + count].all():
            fail("topology", f"{where}: leaf range [{first}, {first + count}) covers a hole slot")
        if live[first + count:first + span].any():
            fail("topology", f"{where}: padding slot of leaf [{first}, {first + count}) holds a primitive")
        seen.extend(int(i) for i in ids[first:first + count][live[first:first + count]] & 0x7FFFFFFF)
        return first, count

    refs = np.zeros(n, np.int64)
    level = np.zeros(n, np.int64)
    order = []
    depth = 0
    if n_prims == 0:
        if root != TRAVERSE_DONE:
            fail("topology", f"empty scene with root link {root:#x}")
    elif root < 0:
        if n:
            fail("topology", f"leaf root with {n} nodes")
        leaf(root, "root")
        depth = 1
    elif root >= n:
        fail("topology", f"root link {root} outside [0, {n})")
    else:
        level[root] = 1
        stack = [root]
        while stack:
            j = stack.pop()
            order.append(j)
            for k in range(4):
                l = int(child[j, k])
                if l == EMPTY_LINK:
                    if (qlo[j, :, k] != 255).any() or (qhi[j, :, k] != 0).any():
                        fail("topology", f"node {j} slot {k}: empty link without the empty bytes (lo 255, hi 0)")
                elif l < 0:
                    leaf(l, f"node {j} child {k}")
                elif l >= n:
                    fail("topology", f"node {j} child {k}: inner link {l} outside [0, {n})")
                else:
                    refs[l] += 1
                    if refs[l] == 1 and l != root:
                        level[l] = level[j] + 1
                        stack.append(l)
        if refs[root]:
            fail("topology", f"the root is referenced {refs[root]} times (cycle)")
        for j in np.nonzero((refs != 1) & (np.arange(n) != root))[0][:4]:
            fail("topology", f"node {j} is referenced {refs[j]} times (a tree references it once)")
        depth = int(level.max())
    if n_prims:
        sn = np.asarray(seen, np.int64)
        if (sn >= n_prims).any():
            fail("topology", f"primitive id {sn.max()} beyond the scene's {n_prims} primitives")
        cnt = np.bincount(sn[sn < n_prims], minlength=n_prims)
        for p in np.nonzero(cnt[:n_prims] != 1)[0][:4]:
            fail("topology", f"primitive id {p} appears in {cnt[p]} leaves (exactly one expected)")
        stray = np.nonzero(live[:nrec] & ~owned[:nrec])[0]
        if len(stray):
            fail("topology", f"record slot {stray[0]} holds a primitive but belongs to no leaf")
    done()

    # ---- reference boxes, bottom up
    clo = np.full((n, 3, 4), np.inf, F32)
    chi = np.full((n, 3, 4), -np.inf, F32)
    used = child != EMPTY_LINK
    nlo = np.zeros((n, 3), F32)
    nhi = np.zeros((n, 3), F32)
    for j in reversed(order):
        for k in range(4):
            l = int(child[j, k])
            if l == EMPTY_LINK:
                continue
            if l < 0:
                v = (~l) & 0xFFFFFFFF
                first, count = v >> 3, (v & 7) + 1
                clo[j, :, k] = rlo[first:first + count].min(axis=0)
                chi[j, :, k] = rhi[first:first + count].max(axis=0)
            else:
                clo[j, :, k], chi[j, :, k] = nlo[l], nhi[l]
        nlo[j], nhi[j] = clo[j].min(axis=1), chi[j].max(axis=1)
    info = {"nodes": n, "depth": depth, "leaves": int((child < 0).sum()) + (1 if root < 0 else 0),
            "slack_s": 0.0, "excess_s": 0.0}
    if n:
        _check_planes(np.arange(n), o, s, qlo, qhi, used, clo, chi, nlo, nhi, fail, info, scale_bound=not refit)
    # ---- 5. statistics
    if stats is not None:
        if stats["bvh_nodes"] != n:
            fail("statistics", f"bvh_nodes {stats['bvh_nodes']} != {n} exported nodes")
        if stats["bvh_depth"] != depth:
            fail("statistics", f"bvh_depth {stats['bvh_depth']} != {depth} levels walked from the root")
        with np.errstate(over="ignore"):
            nb = (np.abs(o) + F32(512.0) * s).max(axis=0) if n else np.zeros(3, F32)
        got = np.asarray(stats["node_bound"], F32)
        if not np.array_equal(_bits(got), _bits(nb)):
            fail("statistics", f"node_bound {got.tolist()} != max |o| + 512 s = {nb.tolist()}")
    done()
    return info


# ------------------------------------------------------------------ checker self-test (CPU)
def _quantize_axis(lo, hi, clo, chi, n=4):
    """bvh4_quant.h quantize_axis_n restated in numpy float32: (origin, scale, qlo[n], qhi[n])."""
    lo, hi = F32(lo), F32(hi)
    ext = hi - lo
    smin, smax = F32(S_MIN), F32(2.0 ** 127)
    if not ext > 0:
        s = smin
    else:
        s = F32(2.0 ** math.ceil(math.log2(float(ext / F32(254.0)))))
        s = min(max(s, smin), smax)
    dec = lambda q: lo + F32(q) * s  # noqa: E731
    for _ in range(8):
        ok, qa, qb = True, [255] * n, [0] * n
        for k in range(len(clo)):
            c0, c1 = F32(clo[k]), F32(chi[k])
            a = int(min(max(math.floor(float((c0 - lo) / s)), 0), 255))
            b = int(min(max(math.ceil(float((c1 - lo) / s)), 0), 255))
            while a > 0 and dec(a) > c0:
                a -= 1
            while b < 255 and dec(b) < c1:
                b += 1
            ok = ok and dec(a) <= c0 and dec(b) >= c1
            qa[k], qb[k] = a, b
        if ok:
            break
        s = s * F32(2.0) if s < smax else s
    return lo, s, qa, qb


def _encode_node(boxes, links):
    """One 64-byte node from <= 4 child boxes ((lo3, hi3) float32) and links."""
    w = np.zeros(16, U32)
    f = w.view(F32)
    lo = np.min([b[0] for b in boxes], axis=0).astype(F32)
    hi = np.max([b[1] for b in boxes], axis=0).astype(F32)
    for a in range(3):
        org, s, qa, qb = _quantize_axis(lo[a], hi[a], [b[0][a] for b in boxes], [b[1][a] for b in boxes])
        f[a] = org
        f[(3, 14, 15)[a]] = s
        w[8 + a] = sum(q << (8 * k) for k, q in enumerate(qa))
        w[11 + a] = sum(q << (8 * k) for k, q in enumerate(qb))
    for k in range(4):
        w[4 + k] = (links[k] if k < len(links) else EMPTY_LINK) & 0xFFFFFFFF
    return w, (lo, hi)


def _hand_tree():
    """Ten triangles, leaf size 2: root -> [node 1, (5, 6), (7, 8), (9)], node 1 -> [(0, 1), (2, 3), (4)]."""
    rng = np.random.default_rng(1)
    tri = (rng.uniform(0, 1, (10, 1, 3)) + rng.uniform(-0.07, 0.07, (10, 3, 3))).astype(F32)
    leaves = [(0, [0, 1]), (2, [2, 3]), (4, [4]), (6, [5, 6]), (8, [7, 8]), (10, [9])]
    recs = np.full((12, 12), np.nan, F32)
    recs.view(U32)[:] = HOLE
    boxes = []
    for first, prims in leaves:
        for i, p in enumerate(prims):
            recs[first + i, [0, 1, 2, 4, 5, 6, 8, 9, 10]] = tri[p].reshape(9)
            recs.view(U32)[first + i, [3, 7, 11]] = [p, 0, 1]
        boxes.append((tri[prims].reshape(-1, 3).min(0), tri[prims].reshape(-1, 3).max(0)))
    links = [make_leaf(first, len(prims)) for first, prims in leaves]
    n1, b1 = _encode_node(boxes[:3], links[:3])
    n0, _ = _encode_node([b1] + boxes[3:], [1] + links[3:])
    nodes = np.stack([n0, n1]).view(np.uint8).reshape(2, 64)
    o, s, *_ = _decode_nodes(nodes)
    stats = {"bvh_nodes": 2, "bvh_depth": 2,
             "node_bound": [float(max(abs(o[j, a]) + F32(512) * s[j, a] for j in range(2))) for a in range(3)]}
    return nodes, recs, 0, stats


def _mutants():
    def qlo_up(w, r):
        w[0, 8] += 1 << 8  # child 1's x lo plane one step up

    def qhi_down(w, r):
        w[1, 12] -= 1  # node 1 child 0's y hi plane one step down

    def dup_link(w, r):
        w[0, 5] = 1  # node 1 referenced by two slots

    def leaf_over_hole(w, r):
        w[1, 6] = make_leaf(4, 2) & 0xFFFFFFFF  # slot 5 is a hole

    def prim_twice(w, r):
        r.view(U32)[6, 3] = 7  # primitive 7 in two leaves, 5 in none

    def scale_mantissa(w, r):
        w[0, 14] |= 1

    def origin_up(w, r):
        w[1, 2] += 1  # oz of node 1 (positive) one ulp up

    return [(qlo_up, "enclosure"), (qhi_down, "enclosure"), (dup_link, "topology"), (leaf_over_hole, "topology"),
            (prim_twice, "topology"), (scale_mantissa, "origin/scale"), (origin_up, "origin/scale")]


def test_checker_accepts_a_hand_built_tree():
    nodes, recs, root, stats = _hand_tree()
    info = check_bvh4(nodes, recs, root, 10, 2, stats=stats)
    assert info["nodes"] == 2 and info["depth"] == 2 and info["leaves"] == 6
    assert 0 < info["slack_s"] <= 2.0
    # a leaf root (the builder's num_nodes4 == 0) and an empty scene
    r2 = recs[:2].copy()
    check_bvh4(np.zeros((0, 64), np.uint8), r2, make_leaf(0, 2), 2, 2,
               stats={"bvh_nodes": 0, "bvh_depth": 1, "node_bound": [0.0, 0.0, 0.0]})


@pytest.mark.parametrize("mutate,invariant", _mutants(), ids=[m.__name__ for m, _ in _mutants()])
def test_checker_rejects_each_mutation(mutate, invariant):
    nodes, recs, root, stats = _hand_tree()
    w = nodes.view("<u4").reshape(2, 16).copy()
    r = recs.copy()
    mutate(w, r)
    with pytest.raises(BvhViolation) as e:
        check_bvh4(w.view(np.uint8).reshape(2, 64), r, root, 10, 2)
    assert f"[{invariant}]" in str(e.value), str(e.value)


def test_checker_rejects_wrong_statistics():
    nodes, recs, root, stats = _hand_tree()
    for key, val in (("bvh_nodes", 3), ("bvh_depth", 0),
                     ("node_bound", [float(np.nextafter(F32(stats["node_bound"][0]), F32(0)))] + stats["node_bound"][1:])):
        with pytest.raises(BvhViolation, match=r"\[statistics\]"):
            check_bvh4(nodes, recs, root, 10, 2, stats=dict(stats, **{key: val}))


# ------------------------------------------------------------------ bvh4_quant.h on the host (CPU)
QUANT_MAIN = r"""
#include <cstdio>
#include <cstdlib>
#include "bvh4_quant.h"
// stdin: N nk lo hi clo[0] chi[0] ... (floats as hex words); stdout: origin ebyte qlo[N/4] qhi[N/4]
template <int N>
static void run(int nk, float lo, float hi, const float *clo, const float *chi) {
    float origin;
    uint32_t e, qlo[N / 4], qhi[N / 4];
    pupil::quantize_axis_n<N>(lo, hi, clo, chi, nk, origin, e, qlo, qhi);
    printf("%08x %u", pupil::qbits(origin), e);
    for (int w = 0; w < N / 4; w++) printf(" %08x", qlo[w]);
    for (int w = 0; w < N / 4; w++) printf(" %08x", qhi[w]);
    printf("\n");
}
int main() {
    int n, nk;
    while (scanf("%d %d", &n, &nk) == 2) {
        uint32_t w[18];
        for (int i = 0; i < 2 + 2 * nk; i++)
            if (scanf("%x", &w[i]) != 1) return 2;
        float clo[8] = {0}, chi[8] = {0};
        for (int k = 0; k < nk; k++) clo[k] = pupil::qfloat(w[2 + 2 * k]), chi[k] = pupil::qfloat(w[3 + 2 * k]);
        if (n == 4) run<4>(nk, pupil::qfloat(w[0]), pupil::qfloat(w[1]), clo, chi);
        else if (n == 8) run<8>(nk, pupil::qfloat(w[0]), pupil::qfloat(w[1]), clo, chi);
        else return 3;
    }
    return 0;
}
"""


def _quant_cases():
    """(N, lo, hi, clo[nk], chi[nk]) float32 interval sets; children lie inside [lo, hi]."""
    rng = np.random.default_rng(7)
    cases = []

    def add(n, lo, hi, c):
        c = np.asarray(c, F32).reshape(-1, 2)
        cases.append((n, F32(lo), F32(hi), c[:, 0].copy(), c[:, 1].copy()))

    for i in range(10000):  # magnitudes 1e-6 .. 1e6 for the position and for the extent
        n = 4 if i % 2 == 0 else 8
        nk = 1 + (i // 2) % n
        lo = F32(rng.choice([-1.0, 1.0]) * 10.0 ** rng.uniform(-6, 6))
        hi = F32(F64(lo) + 10.0 ** rng.uniform(-6, 6))
        c = np.sort(rng.uniform(F64(lo), F64(hi), (nk, 2)), axis=1).astype(F32).clip(lo, hi)
        if i % 3:  # as in a real node: some child touches each end
            c[0, 0], c[-1, 1] = lo, hi
        add(n, lo, hi, c)
    for n in (4, 8):
        for nk in range(1, n + 1):
            for lo in (0.0, -3.5, 1e-3, 12345.678):
                add(n, lo, lo, [[lo, lo]] * nk)  # hi == lo
                add(n, lo, lo + 2.5, [[lo, lo + 2.5]] * nk)  # children equal to the parent
                add(n, lo, lo + 2.5, ([[lo, lo], [lo + 2.5, lo + 2.5]] * nk)[:nk])  # zero width at both ends
        g = 0.0625  # the float32 grid at 1e6: hi = 1e6 + 2^-10 rounds to lo, the next extents are grid steps
        add(n, 1e6, 1e6 + 2.0 ** -10, [[1e6, 1e6 + 2.0 ** -10]] * 2)
        add(n, 1e6, 1e6 + g, [[1e6, 1e6 + g], [1e6, 1e6], [1e6 + g, 1e6 + g]])
        add(n, 1e6, 1e6 + 5 * g, [[1e6, 1e6 + g], [1e6 + 2 * g, 1e6 + 3 * g], [1e6 + 4 * g, 1e6 + 5 * g]])
        add(n, -1e6 - 3 * g, -1e6, [[-1e6 - 3 * g, -1e6 - 2 * g], [-1e6 - g, -1e6]])
        for lo, hi in ((0.0, 1e-40), (1e-39, 2e-39), (-3e-45, 3e-45), (0.0, 1.4e-45), (1.0, 1.0 + 2.0 ** -23),
                       (0.0, 254 * S_MIN), (0.0, 253 * S_MIN)):  # denormal extents and the smallest normal scale
            mid = F32(0.5 * (F64(F32(lo)) + F64(F32(hi))))
            add(n, lo, hi, [[lo, mid], [mid, hi], [lo, hi]])
    return cases


def _run_quantiser(tmp_path, cases):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    src, exe = tmp_path / "quant_main.cpp", tmp_path / "quant_main"
    src.write_text(QUANT_MAIN)
    # pt_scene.h uses float4, so plain g++ cannot compile it: hipcc's host-only pass
    subprocess.run([hipcc, "-x", "hip", "--cuda-host-only", "-std=c++17", "-O1", "-ffp-contract=off", "-I", CSRC,
                    str(src), "-o", str(exe)], check=True)
    hx = lambda v: f"{int(_bits(v).reshape(-1)[0]):08x}"  # noqa: E731
    text = "\n".join(" ".join([str(n), str(len(clo)), hx(lo), hx(hi)] + [hx(x) for k in range(len(clo))
                                                                      for x in (clo[k], chi[k])])
                     for n, lo, hi, clo, chi in cases)
    r = subprocess.run([str(exe)], input=text + "\n", capture_output=True, text=True, check=True)
    lines = r.stdout.split("\n")[:-1]
    assert len(lines) == len(cases)
    out = []
    for (n, *_), line in zip(cases, lines):
        t = line.split()
        org = np.array([int(t[0], 16)], U32).view(F32)[0]
        words = [int(x, 16) for x in t[2:]]
        qlo = [(words[k // 4] >> (8 * (k % 4))) & 255 for k in range(n)]
        qhi = [(words[n // 4 + k // 4] >> (8 * (k % 4))) & 255 for k in range(n)]
        out.append((org, int(t[1]), qlo, qhi))
    return out


def test_host_quantiser_invariants(tmp_path):
    """bvh4_quant.h (N = 4 and 8) keeps invariants 2-4 on 10^4 random interval sets over 1e-6..1e6 and on
    the edge inputs of _quant_cases.  For children inside [lo, hi] plane 0 decodes to lo and, once the
    scale is a normal float, plane 255 reaches hi after at most one doubling, so the retry loop
    (attempt < 8) ends with ok true on every input here; it can store a node with ok false only
    for children outside [lo, hi] or NaN inputs."""
    cases = _quant_cases()
    worst = 0.0
    for (n, lo, hi, clo, chi), (org, e, qlo, qhi) in zip(cases, _run_quantiser(tmp_path, cases)):
        tag = f"N={n} nk={len(clo)} lo={lo!r} hi={hi!r} -> e={e} qlo={qlo} qhi={qhi}"
        assert _bits(org)[0] == _bits(lo)[0], f"[origin/scale] {tag}"
        assert 1 <= e <= 254, f"[origin/scale] exponent byte: {tag}"
        s = F32(2.0 ** (e - 127))
        ext = F64(hi) - F64(lo)
        if ext > 0:
            assert F64(s) <= max(4.0 * ext / 254.0, S_MIN), f"[origin/scale] s = {s!r}: {tag}"
        for k in range(n):
            if k >= len(clo):
                assert (qlo[k], qhi[k]) == (255, 0), f"empty slot {k}: {tag}"
                continue
            dlo, dhi = org + F32(qlo[k]) * s, org + F32(qhi[k]) * s
            assert dlo <= clo[k] and dhi >= chi[k], f"[enclosure] child {k} [{clo[k]!r}, {chi[k]!r}]: {tag}"
            for dec, ref in ((dlo, clo[k]), (dhi, chi[k])):
                slack = abs(F64(ref) - F64(dec))
                assert slack <= 2.0 * F64(s) + _ulp(max(abs(dec), abs(ref))), \
                    f"[tightness] child {k}: {dec!r} is {slack / F64(s):.3f} s from {ref!r}: {tag}"
                worst = max(worst, slack / F64(s))
    print(f"host quantiser: {len(cases)} cases, largest slack {worst:.3f} s")


def test_host_quantiser_overflowing_extent(tmp_path):
    """lo = -3e38, hi = 3e38: hi - lo is infinite.  The encoder used to store the scale inf, whose
    plane 0 decodes to NaN.  Pinned now: the scale is clamped to the largest finite power of two,
    2^127; planes that would lie more than FLT_MAX above the origin decode to +inf (q * scale itself
    overflows, so no 8-bit q places a finite plane there), which still encloses; nothing is NaN and
    the low planes stay finite."""
    lo, hi = F32(-3e38), F32(3e38)
    kids = [(lo, F32(-1e38)), (F32(-1e38), F32(1e38)), (F32(1e38), hi), (lo, hi)]
    cases = [(n, lo, hi, np.array([k[0] for k in kids[:nk]], F32), np.array([k[1] for k in kids[:nk]], F32))
             for n in (4, 8) for nk in (1, 4)]
    for (n, _, _, clo, chi), (org, e, qlo, qhi) in zip(cases, _run_quantiser(tmp_path, cases)):
        assert _bits(org)[0] == _bits(lo)[0] and e == 254, (org, e)
        s = F32(2.0 ** 127)
        with np.errstate(over="ignore"):
            for k in range(len(clo)):
                dlo, dhi = org + F32(qlo[k]) * s, org + F32(qhi[k]) * s
                assert np.isfinite(dlo) and dlo <= clo[k], (k, qlo[k], dlo)
                assert not np.isnan(dhi) and dhi >= chi[k], (k, qhi[k], dhi)


# ------------------------------------------------------------------ scenes for the GPU cases
class Built:
    """A scene as a list of instances ({"tris": (k, 3, 3) object space, "xf": 4x4} or {"sphere": 4x4})
    with its world-space geometry by global primitive id (float64, for aiming rays and for ties)."""

    def __init__(self, instances, aim=None, res=(16, 16)):
        self.instances = instances
        self.aim = aim  # per-primitive weight of the aimed rays (None: uniform)
        w = World()
        mat = w.add_material(world_mod.diffuse((0.5, 0.5, 0.5)))
        sph = None
        for inst in instances:
            if "sphere" in inst:
                sph = w.add_builtin("sphere") if sph is None else sph
                w.add_instance(sph, mat, inst["sphere"])
            else:
                t = np.ascontiguousarray(inst["tris"], F32)
                s = w.add_mesh(t.reshape(-1, 3), np.arange(3 * len(t), dtype=U32).reshape(-1, 3))
                w.add_instance(s, mat, inst.get("xf"))
        w.set_film(res[0], res[1], 2)
        w.set_sensor(40.0, world_mod.look_at_mitsuba((0.5, 0.5, -3), (0.5, 0.5, 0.5), (0, 1, 0)))
        self.world = w
        self.refresh()

    def set_transform(self, i, xf):
        self.instances[i]["sphere" if "sphere" in self.instances[i] else "xf"] = xf
        self.world.set_instance_transform(i, xf)
        self.refresh()

    def refresh(self):
        tri, lo, hi, inst_of, inv = [], [], [], [], {}
        for i, inst in enumerate(self.instances):
            if "sphere" in inst:
                m = np.asarray(inst["sphere"], F64)
                e = np.linalg.norm(m[:3, :3], axis=1) * 1.001
                tri.append(np.full((1, 3, 3), np.nan))
                inv[len(inst_of)] = np.linalg.inv(m[:3, :3])
                lo.append((m[:3, 3] - e)[None])
                hi.append((m[:3, 3] + e)[None])
                inst_of.append([i])
            else:
                t = np.asarray(inst["tris"], F32).astype(F64)
                if inst.get("xf") is not None:
                    m = np.asarray(inst["xf"], F32).astype(F64)
                    t = t @ m[:3, :3].T + m[:3, 3]
                t = t.astype(F32).astype(F64)  # world vertices are float32 in the engine and the oracle
                tri.append(t)
                lo.append(t.min(axis=1))
                hi.append(t.max(axis=1))
                inst_of.append([i] * len(t))
        self.tri, self.lo, self.hi = np.concatenate(tri), np.concatenate(lo), np.concatenate(hi)
        self.inst_of = np.concatenate(inst_of)
        self.to_object = np.zeros((len(self.lo), 3, 3))  # spheres: world -> unit sphere (linear part)
        first = np.cumsum([0] + [len(i) for i in inst_of])
        for i, m in inv.items():
            self.to_object[first[i]] = m
        self.sphere = np.isnan(self.tri[:, 0, 0])
        e1, e2 = self.tri[:, 1] - self.tri[:, 0], self.tri[:, 2] - self.tri[:, 0]
        self.normal = np.cross(e1, e2)
        self.edge = np.maximum(np.linalg.norm(e1, axis=1), np.maximum(
            np.linalg.norm(e2, axis=1), np.linalg.norm(self.tri[:, 2] - self.tri[:, 1], axis=1)))
        with np.errstate(invalid="ignore"):
            self.zero_area = ~self.sphere & ~(np.linalg.norm(self.normal, axis=1) > 1e-9 * self.edge ** 2)
        self.centre = np.where(self.sphere[:, None], 0.5 * (self.lo + self.hi), np.nan_to_num(self.tri).mean(axis=1))
        self.size = np.maximum((self.hi - self.lo).max(axis=1), 1e-30)


def _soup(n, seed, size=0.05, lo=0.0, hi=1.0):
    rng = np.random.default_rng(seed)
    return (rng.uniform(lo, hi, (n, 1, 3)) + rng.uniform(-size, size, (n, 3, 3))).astype(F32)


def _xf(rng, spread=1.0, smin=0.4, smax=2.0):
    axis = rng.normal(size=3)
    return world_mod.transform(scale=tuple(rng.uniform(smin, smax, 3)), rotate=(axis, rng.uniform(0, 360)),
                               translate=tuple(rng.uniform(0, spread, 3)))


def _mixed():
    rng = np.random.default_rng(21)
    inst = [{"tris": _soup(75, 30 + i, 0.08, -0.5, 0.5), "xf": _xf(rng, 2.0)} for i in range(4)]
    inst += [{"sphere": _xf(rng, 2.5, 0.05, 0.3)} for _ in range(40)]
    return Built(inst, res=(48, 32))


@functools.lru_cache(maxsize=None)
def _scene(name):
    if name.startswith("soup"):  # soup<N>: random small triangles in a unit cube
        n = int(name[4:])
        return Built([{"tris": _soup(n, n)}])
    if name == "coincident":
        return Built([{"tris": np.repeat(_soup(1, 5, 0.3), 300, axis=0)}])
    if name.startswith("coplanar"):
        t = _soup(1000, 11, 0.003)  # small: few of the coplanar triangles overlap (hit ties)
        t[:, :, AXES.index(name[-1])] = 0.25
        return Built([{"tris": t}])
    if name == "degenerate":
        rng = np.random.default_rng(12)
        good = _soup(500, 12, 0.04)
        two = _soup(50, 13, 0.04)
        two[:, 2] = two[:, 1]  # two equal vertices
        c0 = rng.integers(0, 1024, (50, 3))  # collinear, exactly: v0, v0 + d, v0 + 2 d on a 2^-10 grid
        step = rng.integers(1, 40, (50, 3))
        col = (np.stack([c0, c0 + step, c0 + 2 * step], axis=1) / 1024.0).astype(F32)
        dup_of = rng.choice(500, 50, replace=False)
        aim = np.ones(650)
        aim[dup_of] = aim[600:] = 0.05  # tied pairs: few aimed rays, so that >= 95 % of the hits are unique
        aim[500:600] = 0.5
        return Built([{"tris": np.concatenate([good, two, col, good[dup_of]])}], aim=aim)
    if name == "far":
        return Built([{"tris": _soup(1000, 15, 1e-2),
                       "xf": world_mod.transform(translate=(1e5, -2e5, 3e5))}])
    if name == "decades":
        rng = np.random.default_rng(16)
        n = 1500
        c = rng.choice([-1.0, 1.0], (n, 1, 3)) * 10.0 ** rng.uniform(-4, 4, (n, 1, 3))
        return Built([{"tris": (c + 10.0 ** rng.uniform(-4, 4, (n, 1, 1)) * rng.uniform(-1, 1, (n, 3, 3))).astype(F32)}])
    if name == "mixed":
        return _mixed()
    raise KeyError(name)


def _rays(b, seed, aimed=5000, random=2000, only=None):
    """`aimed` rays at jittered primitive centres from nearby origins (near relative to the primitive,
    so that the small ones of a wide-ranging scene are hit too) and `random` rays through the bounds."""
    rng = np.random.default_rng(seed)
    p = np.ones(len(b.centre)) if b.aim is None else b.aim.copy()
    if only is not None:
        p = p * only
    pick = rng.choice(len(p), aimed, p=p / p.sum())
    tgt = b.centre[pick] + rng.normal(0, 0.15, (aimed, 3)) * b.size[pick, None]
    d = rng.normal(size=(aimed, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    org = tgt - d * (b.size[pick] * 10.0 ** rng.uniform(0.5, 2.0, aimed))[:, None]
    lo, hi = b.lo.min(axis=0), b.hi.max(axis=0)
    pad = 0.25 * (hi - lo).max() + 1e-3
    o2 = rng.uniform(lo - pad, hi + pad, (random, 3))
    d2 = rng.normal(size=(random, 3))
    d2 /= np.linalg.norm(d2, axis=1, keepdims=True)
    return np.concatenate([np.concatenate([org, d], 1), np.concatenate([o2, d2], 1)]).astype(F32)


def _unique_hits(b, rays, ref):
    """Mask of rays whose reference hit is unique: no other primitive passes through the hit point
    x = o + t d (float64 restatement on the scene's geometry alone).  The intersection works on
    vertices relative to the ray origin, so its rounding scales with max(t, |v - o|): a primitive
    ties if x lies within 64 float32 ulps of that magnitude of it (for a sphere: within a 0.1 %
    shell of its surface, conservative).  Zero-area triangles cannot be hit and never tie."""
    ids = np.ascontiguousarray(ref).view(U32)[:, 3] & 0x7FFFFFFF
    hit = ref[:, 0] > 0
    o, d, t = rays[:, :3].astype(F64), rays[:, 3:6].astype(F64), ref[:, 0].astype(F64)
    x = o + t[:, None] * d
    unique = np.ones(len(rays), bool)
    idx = np.nonzero(hit)[0]
    cand = ~b.zero_area
    slo, shi = b.lo.min(axis=0), b.hi.max(axis=0)
    for c in np.array_split(idx, max(1, len(idx) * len(b.lo) // 1_000_000)):
        xc = x[c][:, None, :]
        far = np.maximum(np.abs(slo - o[c]), np.abs(shi - o[c])).max(axis=1)
        e = (64.0 * _ulp(np.maximum(far, t[c])))[:, None, None]  # prefilter: the scene's largest |v - o|
        inside = ((xc >= b.lo[None] - e) & (xc <= b.hi[None] + e)).all(axis=2) & cand[None]
        inside[np.arange(len(c)), ids[c]] = False
        r, p = np.nonzero(inside)
        oc = o[c][r]
        er = 64.0 * _ulp(np.maximum(np.maximum(np.abs(b.lo[p] - oc), np.abs(b.hi[p] - oc)).max(axis=1), t[c][r]))
        tie = np.zeros(len(r), bool)
        m = b.sphere[p]
        y = np.einsum("nij,nj->ni", b.to_object[p[m]], x[c][r[m]] - b.centre[p[m]])
        tie[m] = np.abs(np.linalg.norm(y, axis=1) - 1.0) <= 1e-3 + er[m] * np.abs(b.to_object[p[m]]).sum(axis=(1, 2))
        m = ~m
        rr, pp = r[m], p[m]
        n = b.normal[pp]
        nn = np.linalg.norm(n, axis=1)
        v = x[c][rr] - b.tri[pp, 0]
        near = np.abs((n * v).sum(axis=1)) <= er[m] * nn
        e1, e2 = b.tri[pp, 1] - b.tri[pp, 0], b.tri[pp, 2] - b.tri[pp, 0]
        bu = (np.cross(v, e2) * n).sum(axis=1) / nn ** 2
        bv = (np.cross(e1, v) * n).sum(axis=1) / nn ** 2
        tol = er[m] * b.edge[pp] / nn
        tie[m] = near & (bu >= -tol) & (bv >= -tol) & (1.0 - bu - bv >= -tol)
        unique[c[np.unique(r[tie])]] = False
    return unique


def _leaf_size():
    return min(8, max(1, int(os.environ.get("PUPIL_LEAF_SIZE", "2"))))


def _trace(pt, rays, any_hit=0):
    r8 = np.ascontiguousarray(np.concatenate([rays, np.full((len(rays), 1), 0.001, F32),
                                              np.full((len(rays), 1), 1e16, F32)], 1), F32)
    out = np.zeros((len(rays), 4), F32)
    abi.check(pt._lib.pupil_pt_trace_rays(pt._pt, len(rays), r8.ctypes.data_as(abi.f32p), out.ctypes.data_as(abi.f32p),
                                          any_hit))
    return out


def _check_hits(name, b, pt, rays, ref, min_unique=0.95):
    """Closest and any hits of the engine against the brute-force reference."""
    unique = _unique_hits(b, rays, ref)
    hit = ref[:, 0] > 0
    share = unique[hit].mean() if hit.any() else 1.0
    if min_unique:
        assert share >= min_unique, f"{name}: only {share:.3f} of the reference hits are unique"
    out = _trace(pt, rays)
    ow, rw = out.view(U32), ref.view(U32)
    bad = ow[:, 0] != rw[:, 0]
    assert not bad.any(), f"{name}: t differs on {bad.sum()} rays, first {np.nonzero(bad)[0][:5]}: {out[bad][:3]} vs {ref[bad][:3]}"
    bad = unique & (ow != rw).any(axis=1)
    assert not bad.any(), f"{name}: {bad.sum()} unique hits differ: {ow[bad][:3]} vs {rw[bad][:3]}"
    got = ow[hit, 3] & 0x7FFFFFFF
    assert (got < len(b.lo)).all() and not b.zero_area[got].any(), f"{name}: a zero-area triangle or no primitive reported"
    assert not b.zero_area[rw[hit, 3] & 0x7FFFFFFF].any(), f"{name}: the reference hit a zero-area triangle"
    occ = _trace(pt, rays, any_hit=1)
    assert np.array_equal(occ[:, 0] > 0, hit), f"{name}: any-hit differs on {((occ[:, 0] > 0) != hit).sum()} rays"
    return int(hit.sum()), float(share)


def _run_case(name, seed=3, sah_leaf=None, min_unique=0.95):
    """One engine on scene `name` under the current environment: exported arrays checked, hits compared."""
    from pupiloptixlab_amd.pt_pass import PTPass

    b = _scene(name)
    desc = b.world.desc()
    orc = oracle.OracleScene(desc)
    rays = _rays(b, seed)
    ref = orc.closest(rays, brute_force=True)
    pt = PTPass(device=0)
    pt.set_scene(desc)
    try:
        nodes, recs, root = pt.export_bvh4()
        info = check_bvh4(nodes, recs, root, orc.num_prims, _leaf_size(), sah_leaf=sah_leaf, stats=pt.stats())
        hits, share = _check_hits(name, b, pt, rays, ref, min_unique)
    finally:
        pt.close_engine()
    print(f"bvh4 {name}: prims {orc.num_prims} nodes {info['nodes']} depth {info['depth']} leaves {info['leaves']} "
          f"slack {info['slack_s']:.3f} s (past one ulp {info['excess_s']:.3f} s) hits {hits} unique {share:.3f}")
    return info


BUILDERS = {"default": {}, "lbvh": {"PUPIL_BVH_BUILDER": "lbvh"}, "greedy": {"PUPIL_BVH4_COLLAPSE": "greedy"},
            "parity": {"PUPIL_BVH4_COLLAPSE": "parity"}, "sah_leaf8": {"PUPIL_SAH_LEAF": "8"}}


def _set_builder(monkeypatch, builder):
    monkeypatch.setenv("PUPIL_ACCEL", "flat")
    for k in ("PUPIL_BVH_BUILDER", "PUPIL_BVH4_COLLAPSE", "PUPIL_SAH_LEAF", "PUPIL_FLAT_UPDATE"):
        monkeypatch.delenv(k, raising=False)
    for k, v in BUILDERS[builder].items():
        monkeypatch.setenv(k, v)


@pytest.mark.gpu
@pytest.mark.parametrize("builder", list(BUILDERS))
def test_builder_paths_on_a_triangle_soup(builder, monkeypatch):
    _set_builder(monkeypatch, builder)
    info = _run_case("soup2000", sah_leaf=8 if builder == "sah_leaf8" else None)
    assert info["nodes"] > 100


@pytest.mark.gpu
@pytest.mark.parametrize("counts", [(2, 3, 255, 256, 257), (1023, 1024, 1025), (4095, 4096, 4097)],
                         ids=["ploc_block", "scan_block", "sort_tile"])
def test_primitive_counts_at_the_tile_edges(counts, monkeypatch):
    """N - 1 / N / N + 1 of the PLOC block (256), kScanBlock (1024) and kSortTile (4096), and the
    smallest scenes: 2 primitives are one root leaf, 3 the smallest tree."""
    _set_builder(monkeypatch, "default")
    for n in counts:
        info = _run_case(f"soup{n}")
        assert (info["nodes"] == 0) == (n <= _leaf_size())


@pytest.mark.gpu
@pytest.mark.parametrize("builder", ["default", "lbvh"])
@pytest.mark.parametrize("name", ["coincident", "coplanar_z", "coplanar_x", "coplanar_y", "degenerate", "far",
                                  "decades", "mixed"])
def test_awkward_geometry(name, builder, monkeypatch):
    _set_builder(monkeypatch, builder)
    _run_case(name, min_unique=0.0 if name == "coincident" else 0.95)


# ------------------------------------------------------------------ refit
def _records_by_id(recs):
    w = np.ascontiguousarray(recs, F32).view(U32).reshape(-1, 12)
    w = w[w[:, 3] != HOLE]
    return w[np.argsort(w[:, 3] & 0x7FFFFFFF)]


@pytest.mark.gpu
def test_refit_keeps_the_invariants(monkeypatch):
    """A mesh instance moved 50 scene diameters away (non-uniform scale, rotation) and a moved sphere,
    one refit: the boxes are loose against the old topology but legal, the records equal a fresh
    engine's, hits equal brute force; then the same after moving both back."""
    import torch
    from pupiloptixlab_amd.pt_pass import PTPass

    _set_builder(monkeypatch, "default")
    b = _mixed()
    w = b.world
    home = [b.instances[1]["xf"].copy(), b.instances[10]["sphere"].copy()]
    diam = float(np.linalg.norm(b.hi.max(axis=0) - b.lo.min(axis=0)))
    pt = PTPass(device=0)
    pt.set_scene(w.desc())
    try:
        pt.render(1)
        torch.cuda.synchronize()
        n_prims = len(b.lo)
        n0 = pt.stats()
        check_bvh4(*pt.export_bvh4(), n_prims, _leaf_size(), stats=n0)
        away = [world_mod.transform(scale=(1.8, 0.5, 1.2), rotate=((1, 2, 3), 75), translate=(50 * diam, -20 * diam, 5.0)),
                world_mod.transform(scale=(0.3, 0.15, 0.2), rotate=((0, 1, 1), 40), translate=(1.0, 3.5, -1.0))]
        for step, xfs in (("moved", away), ("back", home)):
            b.set_transform(1, xfs[0])
            b.set_transform(10, xfs[1])
            before = pt.stats()["accel_refits"]
            pt.update_instances(w, [1, 10])
            stats = pt.stats()
            assert stats["accel_refits"] == before + 1
            nodes, recs, root = pt.export_bvh4()
            info = check_bvh4(nodes, recs, root, n_prims, _leaf_size(), refit=True, stats=stats)
            assert info["nodes"] == n0["bvh_nodes"]  # a refit keeps the topology
            desc = w.desc()
            moved = np.isin(b.inst_of, [1, 10]).astype(F64)
            rays = np.concatenate([_rays(b, 5, 3000, 0, only=moved), _rays(b, 6, 1500, 1500)])
            ref = oracle.OracleScene(desc).closest(rays, brute_force=True)
            hits, share = _check_hits(f"refit {step}", b, pt, rays, ref)
            fresh = PTPass(device=0)
            fresh.set_scene(desc)
            f_nodes, f_recs, f_root = fresh.export_bvh4()
            fresh.close_engine()
            assert np.array_equal(_records_by_id(recs), _records_by_id(f_recs)), f"{step}: records differ from a fresh engine's"
            print(f"bvh4 refit {step}: nodes {info['nodes']} depth {info['depth']} slack {info['slack_s']:.3f} s "
                  f"hits {hits} unique {share:.3f}")
    finally:
        pt.close_engine()


@pytest.mark.gpu
def test_update_of_a_root_leaf_scene(monkeypatch):
    """Two triangles in one instance: the root is a leaf (no 4-wide node), refit_bvh4 declines and
    pupil_pt_update_instances rebuilds.  Hits equal brute force and the render the oracle's."""
    import torch
    from pupiloptixlab_amd.pt_pass import PTPass

    _set_builder(monkeypatch, "default")
    tri = np.array([[[-1, -1, 0], [1, -1, 0], [0, 1, 0]], [[-1, -1, 0.4], [1, -1, 0.4], [0, 1, 0.6]]], F32)
    b = Built([{"tris": tri, "xf": world_mod.transform()}], res=(32, 32))
    w = b.world
    w.set_sensor(40.0, world_mod.look_at_mitsuba((0, 0, -4), (0, 0, 0), (0, 1, 0)))
    w.add_const_env((1.0, 1.0, 1.0))
    pt = PTPass(device=0)
    pt.set_scene(w.desc())
    try:
        pt.render(1)
        torch.cuda.synchronize()
        nodes, recs, root = pt.export_bvh4()
        assert len(nodes) == 0 and root < 0
        check_bvh4(nodes, recs, root, 2, _leaf_size(), stats=pt.stats())
        b.set_transform(0, world_mod.transform(scale=(0.8, 1.3, 1.0), rotate=((0, 0, 1), 25), translate=(0.3, -0.2, 0.5)))
        pt.update_instances(w, [0])
        stats = pt.stats()
        assert stats["accel_refits"] == 1
        nodes, recs, root = pt.export_bvh4()
        check_bvh4(nodes, recs, root, 2, _leaf_size(), stats=stats)
        desc = w.desc()
        orc = oracle.OracleScene(desc)
        rays = _rays(b, 8, 1500, 500)
        ref = orc.closest(rays, brute_force=True)
        assert (ref[:, 0] > 0).sum() > 300
        _check_hits("root leaf", b, pt, rays, ref)
        pt.render(1)
        torch.cuda.synchronize()
        gpu = pt.buffers.get("pt accum buffer").cpu().numpy()
        assert np.array_equal(gpu.view(U32), orc.render(spp=1)["accum"].view(U32))
    finally:
        pt.close_engine()
