"""The two-level world structure (PUPIL_TL_MODE=world) against exact bounds: the checker, a
hand-built structure for its self-test, and the scene the GPU tests drive through every update.

`check_world_bvh4` takes what `PTPass.export_world_bvh4()` returns -- one node array (the TLAS in
[0, tlas_nodes), its never-written reserve up to tlas_cap, then a world-space copy of its shape's
BLAS per mesh instance), the world record slots (flat record format; one two-slot leaf per sphere
at the end), the per-instance world boxes -- and the instance table (prim offset and count, sphere,
hidden, to_world).  Pure numpy, no tolerance: every comparison is exact or a bound derived from
the code, stated where it is asserted.  It raises BvhViolation naming the invariant:

  reachability  the walk from the root stays in [0, tlas_nodes) + [tlas_cap, n), reaches no node
                twice; a copy node it does not reach lies above the braid level: each of its
                children is an entry the TLAS links, or such a node itself (or its instance is hidden)
  leaves        every live slot of a visible instance in exactly one reached leaf, every global
                id of an instance exactly once, b.w the owning instance and its prim range holding
                the id, padding slots holes, a sphere one record in a leaf the TLAS links
  hidden        a hidden instance's vertices are NaN (id words as ever), a visible one's finite;
                a child with nothing visible under it carries the planes lo 255 / hi 0, and a node
                with no visible child origin 0, scale 1 and those planes for every child: what
                bvh4_quant.h quantize_axis_n stores for a node box with lo > hi and what its
                clamps make of a child interval (+inf, -inf).  No ancestor plane moves for hidden
                geometry: the reference boxes below leave it out, and tightness is exact
  instance box  d_boxes: a visible mesh's is the min / max of its world records bit for bit (every
                vertex of the test meshes is referenced), a hidden instance's (+inf, -inf), a
                sphere's encloses c_a +- |row a of the linear part| evaluated in float64
  enclosure     float32(o + q s) brackets the vertices under every child of every reached TLAS
                node and every copy node; a sphere child encloses the true sphere (float64)
  records       (flat_recs given) the nine vertex floats of every visible mesh primitive equal the
                flattened engine's record of the same global id bit for bit
  origin/scale, tightness   invariants 3 and 4 of check_bvh4 against the reference boxes
  statistics    bvh_nodes = tlas_nodes + (n - tlas_cap); node_bound = max |o| + 512 s over the
                live nodes that are not empty (pt_trace4.hip k_node_bound)

Reference boxes.  A copy node is always written by k_world_refit / k_world_refit_batch from the
exact float32 min / max of the records under it, so it is held to those.  A TLAS node is written
either by k_tlas_refit (tlas="refit": the same exact boxes, a sphere child by its instance box) or
by a build (tlas="built": rebuild_tlas over `entries`).  A built node is legitimately looser, and by
a known amount: world_entries (accel_two_level.hip) gives an entry the box DECODED from its
parent's quantised planes in the instance's copy -- qdecode(org, q, sc) per plane -- or the
instance box for a copy's root and for a sphere; build_tlas_node / build_bvh4_over_boxes take exact
float unions of those and encode_bvh4 quantises once more.  So a built TLAS child is held, with
the same exact origin and 2 s + ulp, to the union of its entries' decoded boxes, which this
checker recomputes from the exported copy nodes; `tlas_slack_exact_s` reports how far that leaves
the planes from the true bounds.
"""
import numpy as np

from test_bvh_invariants import (EMPTY_LINK, F32, F64, HOLE, SPHERE_BIT, TRAVERSE_DONE, U32, BvhViolation, _bits,
                                 _check_planes, _decode_nodes, _record_boxes, _records_by_id, make_leaf)
from pupiloptixlab_amd import world as world_mod

INF = F32(np.inf)
VERT = [0, 1, 2, 4, 5, 6, 8, 9, 10]


def leaf_range(link):
    v = (~int(link)) & 0xFFFFFFFF
    return v >> 3, (v & 7) + 1


def sphere_extent(to_world):
    """c_a +- |row a of the linear part| of a unit sphere's to_world (12 floats), in float64."""
    m = np.asarray(to_world, F32).astype(F64).reshape(3, 4)
    r = np.sqrt((m[:, :3] ** 2).sum(axis=1))
    return m[:, 3] - r, m[:, 3] + r


def check_world_bvh4(exp, insts, flat_recs=None, tlas="refit", stats=None, max_leaf=8):
    """exp: PTPass.export_world_bvh4(); insts: per instance dict(first, count, sphere, hidden, to_world).
    Returns dict(nodes, leaves, slack_s, excess_s, tlas_slack_exact_s, unreached)."""
    assert tlas in ("refit", "built")
    nodes, recs, boxes = exp["nodes"], exp["recs"], np.asarray(exp["boxes"], F32).reshape(-1, 6)
    root, tn, tc = int(exp["root"]), int(exp["tlas_nodes"]), int(exp["tlas_cap"])
    n, ni = len(nodes), len(insts)
    o, s, child, qlo, qhi = _decode_nodes(nodes) if n else (np.zeros((0, 3), F32),) * 2 + (np.zeros((0, 4), np.int32),) * 3
    ids, live, _, _ = _record_boxes(recs)
    rf = np.ascontiguousarray(recs, F32).reshape(-1, 12)
    rw = rf.view(U32)
    nrec = len(ids)
    first = np.array([i["first"] for i in insts], np.int64)
    count = np.array([i["count"] for i in insts], np.int64)
    sphere = np.array([bool(i["sphere"]) for i in insts], bool)
    hidden = np.array([bool(i["hidden"]) for i in insts], bool)
    bad = []

    def fail(kind, msg):
        bad.append(f"[{kind}] {msg}")

    def done():
        if bad:
            raise BvhViolation(f"{len(bad)} violation(s):\n" + "\n".join(bad[:12]))

    if not (tn <= tc <= n):
        fail("reachability", f"tlas_nodes {tn}, tlas_cap {tc}, {n} nodes: not ordered")
        done()

    # ---- a. reachability
    refs = np.zeros(n, np.int64)
    order, leaves = [], []  # reached nodes; reached leaves (link, where, linked from the TLAS)
    entry_links = set()     # links held by TLAS nodes (or the root link): the braided entries

    def visit(l, where, from_tlas):
        if l == EMPTY_LINK:
            return
        if from_tlas and not 0 <= l < tn:
            entry_links.add(l)
        if l < 0:
            leaves.append((l, where, from_tlas))
        elif l >= n or tn <= l < tc:
            fail("reachability", f"{where}: link {l} into the reserve [{tn}, {tc}) or beyond {n} nodes")
        else:
            refs[l] += 1
            if refs[l] == 1:
                stack.append(l)

    stack = []
    if root != TRAVERSE_DONE:
        visit(root, "root", True)
    while stack:
        j = stack.pop()
        order.append(j)
        for k in range(4):
            l = int(child[j, k])
            if l == EMPTY_LINK and ((qlo[j, :, k] != 255).any() or (qhi[j, :, k] != 0).any()):
                fail("reachability", f"node {j} slot {k}: empty link without the empty bytes (lo 255, hi 0)")
            visit(l, f"node {j} child {k}", j < tn)
    for j in np.nonzero(refs > 1)[0][:4]:
        fail("reachability", f"node {j} is reached {refs[j]} times (a tree reaches it once)")
    reached = refs > 0

    # instance of every copy node (from the b.w word of the first record under it) and of every leaf
    node_inst = np.full(n, -1, np.int64)

    def leaf_inst(l):
        f, _ = leaf_range(l)
        return int(rw[f, 7]) if f < nrec else -1

    def inst_of(j, depth=0):
        if node_inst[j] < 0 and depth < 64:
            for k in range(4):
                l = int(child[j, k])
                if l == EMPTY_LINK:
                    continue
                node_inst[j] = leaf_inst(l) if l < 0 else (inst_of(l, depth + 1) if tc <= l < n else -1)
                break
        return node_inst[j]

    parent_of = {}  # link -> (unreached copy node, slot): where world_entries decoded the entry's box
    fine = {}

    def above_braid(j, depth=0):
        if j in fine:
            return fine[j]
        fine[j] = False  # while it is being walked: a cycle among unreached nodes ends here, as an orphan
        ok = depth < 64
        for k in range(4):
            l = int(child[j, k])
            if l == EMPTY_LINK:
                continue
            parent_of[l] = (j, k)
            if l in entry_links:
                continue
            ok = ok and l >= 0 and tc <= l < n and not reached[l] and above_braid(l, depth + 1)
        fine[j] = ok
        return ok

    for j in range(tc, n):
        if reached[j]:
            continue
        i = inst_of(j)
        if not above_braid(j) and not (0 <= i < ni and hidden[i]):
            fail("reachability", f"copy node {j} (instance {i}) is not reached and is no ancestor of reached entries alone")

    # ---- b. leaves
    owned = np.zeros(nrec, np.int64)
    leaf_of_slot = {}
    for l, where, from_tlas in leaves:
        f, c = leaf_range(l)
        span = (c + 1) & ~1
        if f % 2 or f + span > nrec:
            fail("leaves", f"{where}: leaf slots [{f}, {f + span}) odd or beyond {nrec} records")
            continue
        if c > max_leaf:
            fail("leaves", f"{where}: leaf of {c} primitives, limit {max_leaf}")
        owned[f:f + span] += 1
        if not live[f:f + c].all():
            fail("leaves", f"{where}: leaf range [{f}, {f + c}) covers a hole slot")
        if live[f + c:f + span].any():
            fail("leaves", f"{where}: padding slot of leaf [{f}, {f + c}) holds a primitive")
        for r in range(f, f + c):
            leaf_of_slot[r] = (where, from_tlas)
    for r in np.nonzero(owned > 1)[0][:4]:
        fail("leaves", f"record slot {r} lies in {owned[r]} reached leaves")
    rinst = rw[:, 7].astype(np.int64)
    gid = (ids & 0x7FFFFFFF).astype(np.int64)
    lv = np.nonzero(live)[0]
    m = rinst[lv] >= ni
    if m.any():
        fail("leaves", f"record slot {lv[m][0]} names instance {rinst[lv[m][0]]} of {ni}")
        done()
    ri = rinst[lv]
    m = (gid[lv] < first[ri]) | (gid[lv] >= first[ri] + count[ri])
    for r in lv[m][:4]:
        fail("leaves", f"record slot {r}: id {gid[r]} outside the prim range of its instance {rinst[r]}")
    m = ((ids[lv] & SPHERE_BIT) != 0) != sphere[ri]
    for r in lv[m][:4]:
        fail("leaves", f"record slot {r}: the sphere bit disagrees with instance {rinst[r]}")
    total = int((first + count).max()) if ni else 0
    cnt = np.bincount(gid[lv][gid[lv] < total], minlength=total)
    for i in range(ni):
        c = cnt[first[i]:first[i] + count[i]]
        for p in np.nonzero(c != 1)[0][:2]:
            fail("leaves", f"global id {first[i] + p} of instance {i} is held by {c[p]} live record slots (exactly one)")
    vis_slot = live & ~np.append(hidden, False)[np.minimum(rinst, ni)]
    for r in np.nonzero(vis_slot & (owned == 0))[0][:4]:
        fail("leaves", f"record slot {r} (instance {rinst[r]}, id {gid[r]}) is live but in no reached leaf")
    for r in lv[sphere[ri] & ~hidden[ri]]:
        if r in leaf_of_slot and not leaf_of_slot[r][1]:
            fail("leaves", f"sphere record {r} hangs under {leaf_of_slot[r][0]}, not under a TLAS node")
    if tlas == "built":
        for r in np.nonzero(live & ~vis_slot & (owned > 0))[0][:2]:
            fail("hidden", f"record slot {r} of hidden instance {rinst[r]} is reached in a freshly built TLAS")

    # ---- c. hidden instances: records
    mesh = live & ((ids & SPHERE_BIT) == 0)
    nan = np.isnan(rf[:, VERT])
    fin = np.isfinite(rf[:, VERT])
    hid_slot = mesh & ~vis_slot
    for r in np.nonzero(hid_slot & ~nan.all(axis=1))[0][:4]:
        fail("hidden", f"record slot {r} of hidden instance {rinst[r]} holds vertices that are not NaN")
    for r in np.nonzero(mesh & vis_slot & ~fin.all(axis=1))[0][:4]:
        fail("hidden", f"record slot {r} of visible instance {rinst[r]} holds vertices that are not finite")
    done()

    # ---- reference boxes: per record, then bottom up
    with np.errstate(invalid="ignore"):
        v = rf[:, VERT].reshape(-1, 3, 3)
        rlo = np.fmin.reduce(v, axis=1)  # fminf / fmaxf drop NaN, as the refit kernels do
        rhi = np.fmax.reduce(v, axis=1)
    rlo[np.isnan(rlo)] = INF
    rhi[np.isnan(rhi)] = -INF
    sph_slot = live & ((ids & SPHERE_BIT) != 0)
    rlo[sph_slot] = boxes[rinst[sph_slot], 0:3]  # k_tlas_refit bounds a sphere record by its instance box
    rhi[sph_slot] = boxes[rinst[sph_slot], 3:6]
    # instance boxes
    for i in range(ni):
        mine = live & (rinst == i)
        if hidden[i]:
            want = np.concatenate([np.full(3, INF), np.full(3, -INF)])
        elif sphere[i]:
            lo64, hi64 = sphere_extent(insts[i]["to_world"])
            if not ((boxes[i, 0:3].astype(F64) <= lo64).all() and (boxes[i, 3:6].astype(F64) >= hi64).all()):
                fail("instance box", f"sphere instance {i}: box {boxes[i].tolist()} does not enclose [{lo64}, {hi64}]")
            continue
        elif not mine.any():
            continue
        else:
            want = np.concatenate([rlo[mine].min(axis=0), rhi[mine].max(axis=0)])
        if not np.array_equal(_bits(boxes[i]), _bits(want)):
            fail("instance box", f"instance {i}: box {boxes[i].tolist()} != {want.tolist()}")

    clo = np.full((n, 3, 4), INF, F32)
    chi = np.full((n, 3, 4), -INF, F32)
    nlo = np.full((n, 3), INF, F32)
    nhi = np.full((n, 3), -INF, F32)
    have = np.zeros(n, bool)

    def leaf_box(l):
        f, c = leaf_range(l)
        if f + c > nrec:
            return np.full(3, INF), np.full(3, -INF)
        return rlo[f:f + c].min(axis=0), rhi[f:f + c].max(axis=0)

    def node_box(j, depth=0):
        if have[j] or depth > 64:
            return
        have[j] = True
        for k in range(4):
            l = int(child[j, k])
            if l == EMPTY_LINK:
                continue
            if l < 0:
                clo[j, :, k], chi[j, :, k] = leaf_box(l)
            elif l < n and not tn <= l < tc:
                node_box(l, depth + 1)
                clo[j, :, k], chi[j, :, k] = nlo[l], nhi[l]
        nlo[j], nhi[j] = clo[j].min(axis=1), chi[j].max(axis=1)

    checked = np.zeros(n, bool)
    checked[tc:] = True
    checked[[j for j in order]] = True
    for j in np.nonzero(checked)[0]:
        node_box(int(j))
    with np.errstate(invalid="ignore", over="ignore"):
        dlo = o[:, :, None] + qlo.astype(F32) * s[:, :, None]
        dhi = o[:, :, None] + qhi.astype(F32) * s[:, :, None]
    used = child != EMPTY_LINK

    # ---- c. hidden instances: planes
    empty_child = used & (clo[:, 0, :] > chi[:, 0, :])
    empty_node = checked & ~(nlo[:, 0] <= nhi[:, 0]) & used.any(axis=1)
    for j in np.nonzero(checked)[0]:
        for k in np.nonzero(empty_child[j])[0]:
            if (qlo[j, :, k] != 255).any() or (qhi[j, :, k] != 0).any():
                fail("hidden", f"node {j} child {k}: nothing visible under it, planes {qlo[j, :, k]}..{qhi[j, :, k]} "
                               "instead of lo 255 / hi 0")
        if empty_node[j] and not (np.array_equal(_bits(o[j]), _bits(np.zeros(3, F32))) and
                                  np.array_equal(_bits(s[j]), _bits(np.ones(3, F32)))):
            fail("hidden", f"node {j}: no visible child, origin {o[j].tolist()} scale {s[j].tolist()} instead of 0 / 1")

    # ---- d. enclosure, f. origin, scale and tightness
    info = {"nodes": len(order), "leaves": len(leaves), "slack_s": 0.0, "excess_s": 0.0, "tlas_slack_exact_s": 0.0,
            "unreached": int((~reached[tc:]).sum())}
    u = used & ~empty_child
    sel = np.nonzero(checked & ~empty_node)[0]
    is_tlas = sel < tn
    exact = sel if tlas == "refit" else sel[~is_tlas]

    def planes(rows, lo, hi, blo, bhi, parts):
        if len(rows):
            _check_planes(rows, o[rows], s[rows], qlo[rows], qhi[rows], u[rows], lo[rows], hi[rows], blo[rows], bhi[rows],
                          fail, info, parts=parts)

    planes(exact, clo, chi, nlo, nhi, ("enclosure", "origin/scale", "tightness"))
    if tlas == "built":
        rows = sel[is_tlas]
        planes(rows, clo, chi, nlo, nhi, ("enclosure",))
        # the entries' boxes as world_entries decodes them, united upwards as the builders do
        mlo, mhi = clo.copy(), chi.copy()
        bl, bh = nlo.copy(), nhi.copy()
        done_t = set()

        def model(j, depth=0):
            if j in done_t or depth > 64:
                return
            done_t.add(j)
            for k in range(4):
                l = int(child[j, k])
                if l == EMPTY_LINK:
                    continue
                if 0 <= l < tn:
                    model(l, depth + 1)
                    mlo[j, :, k], mhi[j, :, k] = bl[l], bh[l]
                elif l in parent_of:
                    p, pk = parent_of[l]
                    mlo[j, :, k], mhi[j, :, k] = dlo[p, :, pk], dhi[p, :, pk]
                else:  # a copy's root or a sphere: the instance box
                    i = leaf_inst(l) if l < 0 else inst_of(l)
                    if 0 <= i < ni:
                        mlo[j, :, k], mhi[j, :, k] = boxes[i, 0:3], boxes[i, 3:6]
            bl[j], bh[j] = mlo[j].min(axis=1), mhi[j].max(axis=1)

        for j in rows:
            model(int(j))
        planes(rows, mlo, mhi, bl, bh, ("origin/scale", "tightness"))
        with np.errstate(invalid="ignore", over="ignore"):
            s3 = s[rows].astype(F64)[:, :, None]
            uu = u[rows][:, None, :] & np.ones((1, 3, 1), bool)
            for dec, ref in ((dlo[rows], clo[rows]), (dhi[rows], chi[rows])):
                d = np.abs(ref.astype(F64) - dec.astype(F64)) / s3
                ok = uu & np.isfinite(d)
                if ok.any():
                    info["tlas_slack_exact_s"] = max(info["tlas_slack_exact_s"], float(d[ok].max()))
    # a sphere child encloses the true sphere, whatever box the kernels took for it
    for j in order:
        for k in range(4):
            l = int(child[j, k])
            if l >= 0 or l == EMPTY_LINK:
                continue
            f, c = leaf_range(l)
            if f < nrec and sph_slot[f] and not hidden[rinst[f]]:
                lo64, hi64 = sphere_extent(insts[rinst[f]]["to_world"])
                if not ((dlo[j, :, k].astype(F64) <= lo64).all() and (dhi[j, :, k].astype(F64) >= hi64).all()):
                    fail("enclosure", f"node {j} child {k}: [{dlo[j, :, k]}, {dhi[j, :, k]}] does not enclose the sphere "
                                      f"[{lo64}, {hi64}] of instance {rinst[f]}")

    # ---- e. the records are the flattened engine's
    if flat_recs is not None:
        fw = _records_by_id(flat_recs)
        fid = (fw[:, 3] & 0x7FFFFFFF).astype(np.int64)
        mine = np.nonzero(mesh & vis_slot)[0]
        mine = mine[np.argsort(gid[mine], kind="stable")]
        pos = np.searchsorted(fid, gid[mine])
        okp = (pos < len(fid)) & (fid[np.minimum(pos, len(fid) - 1)] == gid[mine])
        if not okp.all():
            fail("records", f"global id {gid[mine][~okp][0]} is not in the flattened engine's records")
        else:
            diff = (rw[mine][:, VERT] != fw[pos][:, VERT]).any(axis=1)
            for r in mine[diff][:4]:
                fail("records", f"record slot {r} (instance {rinst[r]}, id {gid[r]}): vertices {rf[r, VERT].tolist()} "
                                "differ from the flattened engine's")
            if diff.any():
                fail("records", f"{diff.sum()} of {len(mine)} visible mesh records differ from the flattened engine's")

    # ---- g. statistics
    if stats is not None:
        if stats["bvh_nodes"] != tn + (n - tc):
            fail("statistics", f"bvh_nodes {stats['bvh_nodes']} != tlas_nodes {tn} + copies {n - tc}")
        livem = np.zeros(n, bool)
        livem[:tn] = True
        livem[tc:] = True
        w = nodes.view("<u4").reshape(-1, 16) if n else np.zeros((0, 16), U32)
        livem &= ~((w[:, 8] == 0xFFFFFFFF) & (w[:, 11] == 0))  # k_node_bound skips empty nodes
        with np.errstate(over="ignore"):
            nb = (np.abs(o[livem]) + F32(512.0) * s[livem]).max(axis=0) if livem.any() else np.zeros(3, F32)
        got = np.asarray(stats["node_bound"], F32)
        if not np.array_equal(_bits(got), _bits(nb)):
            fail("statistics", f"node_bound {got.tolist()} != max |o| + 512 s = {nb.tolist()} over the live nodes")
    done()
    return info


# ------------------------------------------------------------------ a hand-built structure (CPU self-test)
QUAD = np.array([[[0, 0, 0], [1, 0, 0], [1, 1, 0]], [[0, 0, 0], [1, 1, 0], [0, 1, 0]]], F64)


def hand_world(encode, hidden_b=False, mode="built"):
    """Two instances A, B of a two-triangle quad (leaf size 1: one copy node with two leaves each)
    and one sphere.  Nodes: 0 the TLAS root -> [node 1, the sphere's leaf]; 1 a TLAS node ->
    [A's two leaves, B's copy root]; 2 the reserve (never written: garbage bytes); 3 A's copy node,
    above the braid level and not reached; 4 B's.  tlas_nodes 2, tlas_cap 3.  `encode` turns a
    list of (child boxes, links) into 16-word nodes (bvh4_quant.h on the host).  mode "built":
    the TLAS boxes are the entries' decoded boxes, as rebuild_tlas builds; "refit": exact, as
    k_tlas_refit leaves them, with B's planes emptied when hidden_b.
    Returns (exp, insts, stats)."""
    xf = [world_mod.transform(scale=(1.5, 0.7, 1.0), rotate=((1, 2, 3), 37.0), translate=(0.3, -0.2, 0.5)),
          world_mod.transform(scale=(0.8, 1.2, 1.0), rotate=((2, -1, 1), 63.0), translate=(4.0, 0.5, -1.0)),
          world_mod.transform(scale=(0.5, 0.5, 0.5), translate=(2.0, 3.0, 0.0))]
    recs = np.zeros((10, 12), F32)
    rw = recs.view(U32)
    rw[:] = HOLE
    for i in range(2):
        m = xf[i].astype(F64)
        for t in range(2):
            r = 4 * i + 2 * t
            wv = (QUAD[t] @ m[:3, :3].T + m[:3, 3]).astype(F32)
            recs[r, VERT] = np.nan if (hidden_b and i == 1) else wv.reshape(9)
            rw[r, [3, 7, 11]] = [2 * i + t, i, 0]
    recs[8] = 0.0
    rw[8, [3, 7, 11]] = [4 | SPHERE_BIT, 2, 0]
    m = xf[2]
    e = np.array([np.sqrt(F32(m[a, 0] * m[a, 0] + m[a, 1] * m[a, 1] + m[a, 2] * m[a, 2])) * F32(1.001) for a in range(3)], F32)
    boxes = np.zeros((3, 6), F32)
    boxes[2] = np.concatenate([m[:3, 3] - e, m[:3, 3] + e])
    empty = (np.full(3, INF), np.full(3, -INF))

    def rec_box(r):
        if np.isnan(recs[r, 0]):
            return empty
        v = recs[r, VERT].reshape(3, 3)
        return v.min(axis=0), v.max(axis=0)

    def union(bs):
        return np.min([b[0] for b in bs], axis=0).astype(F32), np.max([b[1] for b in bs], axis=0).astype(F32)

    lb = [rec_box(r) for r in (0, 2, 4, 6)]
    ll = [make_leaf(r, 1) for r in (0, 2, 4, 6)]
    ibox = [union(lb[0:2]), union(lb[2:4])]
    for i in range(2):
        boxes[i] = np.concatenate(ibox[i])
    n3, n4 = encode([(lb[0:2], ll[0:2]), (lb[2:4], ll[2:4])])
    if mode == "built":
        o, s, _, qlo, qhi = _decode_nodes(np.stack([n3]).view(np.uint8).reshape(1, 64))
        ea = [((o[0] + qlo[0, :, k].astype(F32) * s[0]).astype(F32), (o[0] + qhi[0, :, k].astype(F32) * s[0]).astype(F32))
              for k in range(2)]
    else:
        ea = lb[0:2]
    kids1 = ea + [ibox[1]]
    sph = (boxes[2, 0:3], boxes[2, 3:6])
    n1, n0 = encode([(kids1, ll[0:2] + [4]), ([union(kids1), sph], [1, make_leaf(8, 1)])])
    nodes = np.stack([n0, n1, np.full(16, 0xCDCDCDCD, U32), n3, n4]).astype(U32)
    nodes8 = nodes.view(np.uint8).reshape(5, 64)
    o, s, *_ = _decode_nodes(nodes8)
    livem = np.array([True, True, False, True, not hidden_b])
    stats = {"bvh_nodes": 4, "node_bound": [float((np.abs(o[livem, a]) + F32(512) * s[livem, a]).max()) for a in range(3)]}
    exp = {"nodes": nodes8, "recs": recs, "boxes": boxes, "root": 0, "tlas_nodes": 2, "tlas_cap": 3, "braid": 1}
    insts = [{"first": 2 * i, "count": 2, "sphere": False, "hidden": hidden_b and i == 1, "to_world": xf[i][:3].reshape(12)}
             for i in range(2)]
    insts.append({"first": 4, "count": 1, "sphere": True, "hidden": False, "to_world": xf[2][:3].reshape(12)})
    return exp, insts, stats


# ------------------------------------------------------------------ the scene of the GPU tests
def cube_mesh():
    p = np.array([[x, y, z] for x in (-0.5, 0.5) for y in (-0.5, 0.5) for z in (-0.5, 0.5)], F32)
    f = np.array([[0, 1, 3], [0, 3, 2], [4, 6, 7], [4, 7, 5], [0, 4, 5], [0, 5, 1], [2, 3, 7], [2, 7, 6],
                  [0, 2, 6], [0, 6, 4], [1, 5, 7], [1, 7, 3]], U32)
    return p, f


def tess_sphere(slices=12, stacks=8):
    """168 triangles: two fans of `slices` at the poles and stacks - 2 bands of 2 * slices."""
    p = [[0.0, 1.0, 0.0]]
    for i in range(1, stacks):
        th = np.pi * i / stacks
        for j in range(slices):
            ph = 2.0 * np.pi * j / slices
            p.append([np.sin(th) * np.cos(ph), np.cos(th), np.sin(th) * np.sin(ph)])
    p.append([0.0, -1.0, 0.0])
    ring = lambda i, j: 1 + (i - 1) * slices + j % slices  # noqa: E731
    f = [[0, ring(1, j + 1), ring(1, j)] for j in range(slices)]
    for i in range(1, stacks - 1):
        for j in range(slices):
            f += [[ring(i, j), ring(i, j + 1), ring(i + 1, j + 1)], [ring(i, j), ring(i + 1, j + 1), ring(i + 1, j)]]
    f += [[len(p) - 1, ring(stacks - 1, j), ring(stacks - 1, j + 1)] for j in range(slices)]
    return np.array(p, F32), np.array(f, U32)


def icosahedron():
    g = (1.0 + 5.0 ** 0.5) / 2.0
    p = np.array([[-1, g, 0], [1, g, 0], [-1, -g, 0], [1, -g, 0], [0, -1, g], [0, 1, g], [0, -1, -g], [0, 1, -g],
                  [g, 0, -1], [g, 0, 1], [-g, 0, -1], [-g, 0, 1]], F32) * F32(0.4)
    f = np.array([[0, 11, 5], [0, 5, 1], [0, 1, 7], [0, 7, 10], [0, 10, 11], [1, 5, 9], [5, 11, 4], [11, 10, 2],
                  [10, 7, 6], [7, 1, 8], [3, 9, 4], [3, 4, 2], [3, 2, 6], [3, 6, 8], [3, 8, 9], [4, 9, 5], [2, 4, 11],
                  [6, 2, 10], [8, 6, 7], [9, 8, 1]], U32)
    return p, f


T = world_mod.transform


def start_instances():
    """Eight mesh instances and two spheres: rotations about skew axes, the non-uniform scale
    (3, 0.2, 1), a mirror, a translation by 1e4, and an exactly coincident pair (4, 5)."""
    pair = T(scale=(1.1, 0.9, 1.3), rotate=((1, -2, 1), 51.0), translate=(1.5, -2.0, 2.0))
    return [{"shape": "cube", "xf": T(rotate=((1, 2, 3), 37.0))},
            {"shape": "cube", "xf": T(scale=(3.0, 0.2, 1.0), rotate=((2, -1, 1), 63.0), translate=(4.0, 1.0, 0.0))},
            {"shape": "cube", "xf": T(scale=(-1.0, 1.0, 1.0), rotate=((1, 1, -2), 25.0), translate=(-3.0, 2.0, 1.0))},
            {"shape": "tess", "xf": T(rotate=((3, 1, 2), 71.0), translate=(1e4, -1e4, 1e4))},
            {"shape": "tess", "xf": pair},
            {"shape": "tess", "xf": pair.copy()},
            {"shape": "tess", "xf": T(scale=(3.0, 0.2, 1.0), rotate=((1, 3, -1), 140.0), translate=(-2.0, -3.0, 0.0))},
            {"shape": "cube", "xf": T(scale=(0.6, 0.6, 0.6), rotate=((-1, 2, 2), 200.0), translate=(0.0, 4.0, -2.0))},
            {"shape": "sphere", "xf": T(scale=(0.5, 0.8, 0.3), rotate=((1, 1, 1), 33.0), translate=(2.0, 2.0, 2.0))},
            {"shape": "sphere", "xf": T(scale=(0.7, 0.7, 0.7), translate=(-1.0, -1.0, 3.0))}]


class WorldScene:
    """The world of the GPU tests and what the checker needs of it, kept in step through every
    update: the instance list (shape, transform, visibility) and the meshes of the two shapes."""

    def __init__(self):
        from pupiloptixlab_amd import World

        w = World()
        self.mat = w.add_material(world_mod.diffuse((0.5, 0.5, 0.5)))
        self.mesh = {"cube": cube_mesh(), "tess": tess_sphere()}
        self.shape = {k: w.add_mesh(*self.mesh[k]) for k in ("cube", "tess")}
        self.shape["sphere"] = w.add_builtin("sphere")
        self.inst = start_instances()
        for i in self.inst:
            i["vis"] = True
            w.add_instance(self.shape[i["shape"]], self.mat, i["xf"])
        w.set_film(16, 16, 2)
        w.set_sensor(40.0, world_mod.look_at_mitsuba((0.5, 0.5, -12), (0.5, 0.5, 0.5), (0, 1, 0)))
        self.world = w

    def of_shape(self, name):
        return [k for k, i in enumerate(self.inst) if i["shape"] == name]

    def move(self, k, xf):
        self.inst[k]["xf"] = np.asarray(xf, F32)
        self.world.set_instance_transform(k, xf)

    def show(self, k, vis):
        self.inst[k]["vis"] = bool(vis)
        self.world.set_instance_visibility(k, 0xFF if vis else 0)

    def add(self, shape, xf):
        self.inst.append({"shape": shape, "xf": np.asarray(xf, F32), "vis": True})
        self.world.add_instance(self.shape[shape], self.mat, xf)

    def remove(self, k):
        self.world.remove_instance(k)
        return self.inst.pop(k)

    def set_vertices(self, name, p):
        self.mesh[name] = (np.asarray(p, F32), self.mesh[name][1])
        self.world.set_mesh_vertices(self.shape[name], self.mesh[name][0])

    def set_mesh(self, name, p, f):
        self.mesh[name] = (np.asarray(p, F32), np.asarray(f, U32))
        self.world.set_mesh(self.shape[name], *self.mesh[name])

    def table(self, pt):
        """the checker's instance table, prim offsets and transforms as the engine holds them"""
        first = pt.prim_tables()["inst_first"]
        tw = pt.instance_transforms()[0]
        assert len(first) == len(self.inst) + 1 and len(tw) == len(self.inst)
        return [{"first": int(first[k]), "count": int(first[k + 1] - first[k]), "sphere": i["shape"] == "sphere",
                 "hidden": not i["vis"], "to_world": tw[k]} for k, i in enumerate(self.inst)]

    def built(self):
        """the same geometry as test_bvh_invariants.Built (rays, hit ties)"""
        from test_bvh_invariants import Built

        out = []
        for i in self.inst:
            if i["shape"] == "sphere":
                out.append({"sphere": i["xf"]})
            else:
                p, f = self.mesh[i["shape"]]
                out.append({"tris": p[f], "xf": i["xf"]})
        return Built(out)
