// pt_accel.hip — SceneAccel: builds, updates and publishes the engine's acceleration structure.
#include "pt_accel.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>

namespace pupil {
namespace {

// A builder's return code (build_bvh_bounded, build_two_level, rebuild_tlas) as an ABI error;
// `other`: the message of a failure that is no limit.
int builder_error(int rc, bool two_level, const char *other) {
    if (rc == -3)
        return fail(PUPIL_ERR_UNSUPPORTED, two_level ? "TLAS + BLAS deeper than the traversal stacks hold"
                                                     : "BVH deeper than the traversal stacks hold");
    if (rc == -4) return fail(PUPIL_ERR_UNSUPPORTED, "two-level record slots beyond the 28-bit leaf links");
    return fail(PUPIL_ERR_HIP, other);
}

// of a structure just built, before it is used (create) or swapped in (the rebuilds)
int node_limit(uint64_t nodes4) {
    return nodes4 > kMaxNodes4 ? fail(PUPIL_ERR_UNSUPPORTED, "BVH4 larger than 2^26 nodes (32-bit node offsets)") : PUPIL_OK;
}

uint64_t nodes4_of(const TwoLevelAccel &a) { return a.world ? a.num_wnodes : a.num_nodes4; }

// PUPIL_FLAT_UPDATE / PUPIL_TL_UPDATE, read per update
bool is_rebuild(const char *v) { return v && std::strcmp(v, "rebuild") == 0; }

}  // namespace

uint64_t SceneAccel::nodes4_count() const { return two_level ? nodes4_of(tl) : bvh.num_nodes4; }

void SceneAccel::free() {
    free_lbvh(bvh);
    free_two_level(tl);
    for (void *p : {(void *)d_moved, (void *)refit_box, (void *)node_bound})
        if (p) (void)hipFree(p);
    d_moved = nullptr, refit_box = nullptr, node_bound = nullptr;
}

int SceneAccel::build(const Tables &tables, const pupil_scene_desc *scene, const std::vector<ShapeDev> &shapes) {
    t = tables;
    leaf_size = 2u;  // with the 7-wave traversal: 2 beats 3 by 2 %, 1 and 4 are slower (config 4)
    if (const char *ls = std::getenv("PUPIL_LEAF_SIZE")) leaf_size = (uint32_t)std::min(8, std::max(1, std::atoi(ls)));
    // Flattened (default: on config 5 it traces 1.08x faster than the two-level world mode) or
    // two-level (PUPIL_ACCEL=two_level, which bench.py selects for config 5: cheaper instance
    // updates; automatic when the flattened primitive count would pass the flat build's 2^27
    // limit).
    std::vector<uint32_t> uses(scene->num_shapes, 0);
    inst_shape.resize(scene->num_instances);
    uint64_t flat_prims = 0;
    for (uint32_t i = 0; i < scene->num_instances; i++) {
        inst_shape[i] = scene->instances[i].shape;
        uses[inst_shape[i]]++;
        const pupil_shape &sh = scene->shapes[inst_shape[i]];
        flat_prims += sh.kind == PUPIL_SHAPE_SPHERE ? 1u : sh.num_faces;
    }
    // leaf links hold 28-bit record slots, up to two per primitive (pt_scene.h kRecF4)
    two_level = flat_prims >= (1ull << 27);
    if (const char *a = std::getenv("PUPIL_ACCEL")) {
        if (std::strcmp(a, "flat") == 0) two_level = false;
        if (std::strcmp(a, "two_level") == 0) two_level = true;
    }
    if (!two_level && flat_prims >= (1ull << 27))
        return fail(PUPIL_ERR_UNSUPPORTED, "flattened BVH limited to 2^27 primitives");
    if (two_level) {
        tl_shapes.assign(scene->num_shapes, TwoLevelShape{});
        for (uint32_t k = 0; k < scene->num_shapes; k++) {
            const pupil_shape &sh = scene->shapes[k];
            TwoLevelShape &ts = tl_shapes[k];
            if (sh.kind != PUPIL_SHAPE_MESH || !uses[k]) continue;
            ts.num_faces = sh.num_faces;
            ts.num_vertices = sh.num_vertices;
            ts.positions = shapes[k].pos.get();
            ts.normals = shapes[k].nrm.get();
            ts.texcoords = shapes[k].tex.get();
            ts.indices = shapes[k].idx.get();
            float vmax = 0.f;
            for (size_t v = 0; v < 3 * (size_t)sh.num_vertices; v++) vmax = std::max(vmax, std::fabs(sh.positions[v]));
            ts.vmax = vmax;
        }
        const int rc = build_two_level(tl_shapes, inst_shape, g().mirror, g().insts.get(), t.materials->device(), leaf_size, t.stream, tl);
        if (rc != 0) return builder_error(rc, true, "two-level acceleration build failed");
        ms = tl.build_ms;
    } else {
        const BvhBuildInput bin{g().num_prims, g().prim_inst.get(), g().insts.get(), t.materials->device()};
        const int rc = build_bvh_bounded(bin, bvh, leaf_size, t.stream, &ms, 0);
        if (rc != 0) return builder_error(rc, false, "LBVH build failed");
    }
    return node_limit(nodes4_count());
}

// Writes what the traversal and pupil_pt_stats see of the structure as it is now, and
// DeviceScene::node_bound of its BVH4 arrays (one 12-B read back, the traversal kernels take it
// by value; synchronises the stream).  Live nodes only: in the two-level layouts the TLAS reserve
// [tlas_nodes, tlas_cap) is never written, and whatever an earlier allocation left there must
// not loosen the bound of every ray.
int SceneAccel::publish() {
    DeviceScene &sc = *t.sc;
    pupil_pt_counters &totals = *t.totals;
    sc.two_level = two_level ? 1u : 0u;
    sc.tl_world = two_level && tl.world ? 1u : 0u;
    sc.nodes4 = !two_level ? bvh.nodes4 : tl.world ? tl.wnodes : tl.nodes4;
    sc.prims = !two_level ? bvh.prims : tl.world ? tl.wprims : tl.prims;
    sc.wprims = tl.wprims;
    sc.attrs = two_level ? tl.attrs : bvh.attrs;
    sc.root_link4 = two_level ? tl.root_link4 : bvh.root_link4;
    totals.two_level = sc.two_level;
    totals.bvh_nodes = two_level ? two_level_nodes(tl) : bvh.num_nodes4;
    totals.bvh_depth = two_level ? tl.tlas_depth + tl.blas_depth : bvh.depth4;
    sc.node_bound[0] = sc.node_bound[1] = sc.node_bound[2] = 0.f;
    const uint64_t n = nodes4_count();
    {  // LDS-resident top of the tree (pt_scene.h top_nodes) for the world-mode two-level structure, whose
       // braided TLAS every ray crosses first: -1.3 % per config-5 step; the flat trees of configs 3 / 4
       // pay 1.1 % per launch for the per-visit branch and run the kernel without it
       // (profiles/r05_top_nodes_bisect.txt; PUPIL_TOP_NODES=k forces k nodes, 0 off)
        const char *e = std::getenv("PUPIL_TOP_NODES");
        const uint32_t want = e ? (uint32_t)std::min<long>(kTopNodes, std::max(0L, std::atol(e)))
                                : (sc.tl_world ? kTopNodes : 0u);
        uint64_t live = sc.nodes4 ? n : 0;
        if (two_level) live = std::min<uint64_t>(live, tl.tlas_nodes);
        sc.top_nodes = (uint32_t)std::min<uint64_t>(want, live);
    }
    if (!sc.nodes4 || n == 0) return PUPIL_OK;
    if (!node_bound) HIP_TRY(hipMalloc((void **)&node_bound, 3 * sizeof(uint32_t)));
    if (two_level) {
        const uint64_t tlas = std::min<uint64_t>(tl.tlas_nodes, n), cap = std::min<uint64_t>(tl.tlas_cap, n);
        launch_node_bound(sc.nodes4, tlas, node_bound, t.stream, true);
        launch_node_bound(sc.nodes4 + cap, n - cap, node_bound, t.stream, false);
        counts.launches += (tlas ? 1u : 0u) + (n - cap ? 1u : 0u);
    } else {
        launch_node_bound(sc.nodes4, n, node_bound, t.stream, true);
        counts.launches++;
    }
    counts.syncs++;
    uint32_t b[3];
    HIP_TRY(hipMemcpyAsync(b, node_bound, sizeof(b), hipMemcpyDeviceToHost, t.stream));
    HIP_TRY(hipStreamSynchronize(t.stream));
    std::memcpy(sc.node_bound, b, sizeof(b));
    return PUPIL_OK;
}

// the flags of the instances whose records a refit rewrites (`changed`, or null: the hidden
// ones) on the device, and the node-box scratch of a tree of `nodes` nodes
int SceneAccel::flag_instances(const std::vector<uint32_t> *changed, uint32_t nodes) {
    const std::vector<DevInstance> &insts = g().mirror;
    if (!d_moved) HIP_TRY(hipMalloc((void **)&d_moved, std::max<size_t>(1, insts.size())));
    if (!refit_box) HIP_TRY(hipMalloc((void **)&refit_box, sizeof(float) * 6 * (size_t)std::max(1u, nodes)));
    h_moved.assign(insts.size(), 0);
    if (changed) {
        for (uint32_t id : *changed) h_moved[id] = 1;
    } else {
        for (size_t i = 0; i < insts.size(); i++) h_moved[i] = insts[i].hidden ? 1 : 0;
    }
    HIP_TRY(hipMemcpyAsync(d_moved, h_moved.data(), h_moved.size(), hipMemcpyHostToDevice, t.stream));
    return PUPIL_OK;
}

// The flattened BVH after the instances in `changed` moved, were hidden or shown, or had their
// shape's vertices replaced (attrs: their shading records are rewritten too): one refit in
// place, or a rebuild with the masks applied to the new tree before it replaces the old one
// (refit = false, PUPIL_FLAT_UPDATE=rebuild, a tree without a level order).
int SceneAccel::update_flat(const std::vector<uint32_t> &changed, bool refit, bool attrs, bool flagged) {
    const BvhBuildInput bin{g().num_prims, g().prim_inst.get(), g().insts.get(), t.materials->device()};
    if (refit && !is_rebuild(std::getenv("PUPIL_FLAT_UPDATE"))) {
        if (!flagged)
            if (const int rc = flag_instances(&changed, bvh.num_nodes4)) return rc;
        if (refit_bvh4(bin, bvh, d_moved, refit_box, t.stream, &ms) == 0) {
            // refit_bvh4: the records, one launch per level, one event synchronisation
            counts.launches += (bvh.num_records ? 1u : 0u) +
                               (bvh.level_start.size() >= 2 ? (uint32_t)bvh.level_start.size() - 1u : 0u);
            counts.syncs++;
            // deformed meshes: the shading records follow (publish synchronises the stream)
            if (attrs) launch_refresh_attrs(bin, bvh, d_moved, t.stream);
            return publish();
        }
    }
    BvhBuildOutput nb{};
    double bms = 0.0, hms = 0.0;
    int rc = build_bvh_bounded(bin, nb, leaf_size, t.stream, &bms, 0);
    rc = rc != 0 ? builder_error(rc, false, "LBVH rebuild failed") : node_limit(nb.num_nodes4);
    if (rc == PUPIL_OK && refit_box) {  // sized for the old tree
        (void)hipFree(refit_box);
        refit_box = nullptr;
    }
    bool any_hidden = false;
    for (const DevInstance &d : g().mirror) any_hidden = any_hidden || d.hidden != 0u;
    if (rc == PUPIL_OK && any_hidden) {  // the build covered every instance: the masks go on like a refit's
        rc = flag_instances(nullptr, nb.num_nodes4);
        const int hrc = rc ? 0 : refit_bvh4(bin, nb, d_moved, refit_box, t.stream, &hms, true);
        if (hrc == -1) rc = fail(PUPIL_ERR_UNSUPPORTED, "hidden instances need the BVH4 level order");
        else if (hrc != 0) rc = fail(PUPIL_ERR_HIP, "applying the visibility masks failed");
    }
    if (rc != PUPIL_OK) {  // the old tree stays
        free_lbvh(nb);
        return rc;
    }
    free_lbvh(bvh);
    bvh = nb;
    ms = bms + hms;
    return publish();
}

// The TLAS after the world boxes, world records and world BLAS copies of `changed` were
// regenerated: world mode refits it like the reference's IAS update, object mode rebuilds it
// (PUPIL_TL_UPDATE=rebuild: full build in both).
int SceneAccel::update_tlas(const std::vector<uint32_t> &changed) {
    const int rc = rebuild_tlas(tl, g().mirror, g().insts.get(), changed, t.stream, !is_rebuild(std::getenv("PUPIL_TL_UPDATE")),
                                &counts.launches, &counts.syncs);
    return rc != 0 ? builder_error(rc, true, "TLAS rebuild failed") : publish();
}

int SceneAccel::update_instances(const std::vector<uint32_t> &changed) {
    if (!two_level) return update_flat(changed, true, false);
    const auto t0 = std::chrono::steady_clock::now();
    if (const int rc = update_tlas(changed)) return rc;
    ms = ms_since(t0);
    return PUPIL_OK;
}

int SceneAccel::move_begin(uint32_t **list, uint8_t **moved) {
    *list = nullptr, *moved = nullptr;
    if (two_level) {
        if (tl.world) *list = tl.d_list;
        return PUPIL_OK;
    }
    if (is_rebuild(std::getenv("PUPIL_FLAT_UPDATE"))) return PUPIL_OK;  // a rebuild reads no flag
    const size_t n = std::max<size_t>(1, g().mirror.size());
    if (!d_moved) HIP_TRY(hipMalloc((void **)&d_moved, n));
    if (!refit_box) HIP_TRY(hipMalloc((void **)&refit_box, sizeof(float) * 6 * (size_t)std::max(1u, bvh.num_nodes4)));
    HIP_TRY(hipMemsetAsync(d_moved, 0, n, t.stream));
    *moved = d_moved;
    return PUPIL_OK;
}

void SceneAccel::move_boxes(uint32_t count, float *box, uint32_t stride) {
    if (!two_level || !tl.world || count == 0) return;
    instance_boxes_device(tl, g().insts.get(), count, box, stride, t.stream);
    counts.launches += 2;
}

int SceneAccel::move_finish(const std::vector<uint32_t> &changed, uint32_t count) {
    if (!two_level) return update_flat(changed, true, false, d_moved != nullptr && !is_rebuild(std::getenv("PUPIL_FLAT_UPDATE")));
    if (!tl.world) return update_instances(changed);  // the host's TLAS build, from the mirror
    const auto t0 = std::chrono::steady_clock::now();
    const int rc = move_world_instances(tl, g().mirror, g().insts.get(), changed, count, t.stream,
                                        !is_rebuild(std::getenv("PUPIL_TL_UPDATE")), &counts.launches, &counts.syncs);
    if (rc != 0) return builder_error(rc, true, "TLAS rebuild failed");
    if (const int prc = publish()) return prc;
    ms = ms_since(t0);
    return PUPIL_OK;
}

// The records that carry a bin word: the flattened BVH's, or the two-level world records (world
// mode: with one two-slot leaf per sphere appended; object mode traverses with the instances'
// own bins, its world records are kept consistent all the same).
uint32_t SceneAccel::world_record_slots() const {
    uint64_t slots = two_level ? tl.num_wprims : bvh.num_records;
    if (two_level && tl.world)
        for (const DevInstance &d : g().mirror) slots += d.kind == PUPIL_SHAPE_SPHERE ? 2u : 0u;
    return (uint32_t)slots;
}

void SceneAccel::update_bins() {
    launch_record_bins(two_level ? tl.wprims : bvh.prims, world_record_slots(), g().insts.get(), (uint32_t)g().mirror.size(),
                       t.stream);
}

// Flattened BVH: the shape's instances are flagged moved, refit_bvh4 rewrites their world records
// (a hidden instance's stay NaN) and refits every node, launch_refresh_attrs rewrites their
// shading records.  Two-level: update_shape_blas rewrites the object-space BLAS records, refits
// the BLAS and refreshes its shading records, the instances get the new vmax and margins, and
// rebuild_tlas regenerates their world boxes, world records and world BLAS copies and refits
// (world mode) or rebuilds (object mode) the TLAS.  rebuild: everything anew with the create-time
// builders, the masks put back on, swapped in once it is complete.
int SceneAccel::update_shape(uint32_t shape, const std::vector<uint32_t> &changed, bool rebuild) {
    if (!two_level) return update_flat(changed, !rebuild, true);
    TwoLevelShape &ts = tl_shapes[shape];
    float vmax = 0.f;
    if (!rebuild) {
        if (update_shape_blas(tl, shape, ts, &vmax, t.stream) != 0) return fail(PUPIL_ERR_HIP, "BLAS refit failed");
        ts.vmax = vmax;
        for (uint32_t id : changed) {
            g().mirror[id].vmax = vmax;
            refresh_instance_margins(g().mirror[id]);
        }
        return update_tlas(changed);
    }
    // vmax as at create, from the engine's own device copy by a device reduction (the same
    // maximum the host loop at create finds): host and device vertices take one path, and
    // device vertices never come back to the host
    if (shape_abs_max(tl, ts, &vmax, t.stream) != 0) return fail(PUPIL_ERR_HIP, "vertex reduction failed");
    ts.vmax = vmax;
    std::vector<DevInstance> insts = g().mirror;  // build_two_level refills the two-level fields
    TwoLevelAccel ntl{};
    int rc = build_two_level(tl_shapes, inst_shape, insts, g().insts.get(), t.materials->device(), leaf_size, t.stream, ntl);
    rc = rc != 0 ? builder_error(rc, true, "two-level acceleration rebuild failed") : node_limit(nodes4_of(ntl));
    if (rc != PUPIL_OK) {  // the old structure stays
        free_two_level(ntl);
        return rc;
    }
    free_two_level(tl);
    tl = ntl;
    g().mirror = insts;
    return publish();
}

int SceneAccel::replace_shape(uint32_t shape, const ShapeDev &mesh, bool used, Generation &staged) {
    const BuildOver scope(*this, staged);
    if (!used) {  // no instance shows the shape: no structure holds it (the two-level build skips it too)
        HIP_TRY(hipStreamSynchronize(t.stream));
        return PUPIL_OK;
    }
    TwoLevelShape old_shape{};
    if (two_level) {
        TwoLevelShape &ts = tl_shapes[shape];
        old_shape = ts;
        ts.num_faces = mesh.num_faces;
        ts.num_vertices = mesh.num_vertices;
        ts.positions = mesh.pos.get();
        ts.normals = mesh.nrm.get();
        ts.texcoords = mesh.tex.get();
        ts.indices = mesh.idx.get();  // vmax: update_shape reduces it from the new array
    }
    // both rebuilds build aside and swap on success: flat over the staged tables, two-level over
    // tl_shapes and a copy of the staged mirror, uploaded to the staged instance table
    const int rc = update_shape(shape, {}, true);
    if (rc != PUPIL_OK && two_level) tl_shapes[shape] = old_shape;
    return rc;
}

int SceneAccel::set_instances(Generation &staged, std::vector<uint32_t> &shape_of, const std::vector<ShapeDev> &shapes) {
    const BuildOver scope(*this, staged);
    const std::vector<TwoLevelShape> old_shapes = tl_shapes;
    inst_shape.swap(shape_of);
    auto undo = [&](int rc) {  // of the structure's own inputs; the tables: `scope`
        inst_shape.swap(shape_of);
        tl_shapes = old_shapes;
        return rc;
    };
    if (d_moved) {  // sized by the instance count; the next refit allocates
        (void)hipFree(d_moved);
        d_moved = nullptr;
    }
    last_blas_builds = 0;
    last_whole_rebuild = 1;
    if (!two_level) {
        const int rc = update_flat({}, false, true);
        return rc != PUPIL_OK ? undo(rc) : rc;
    }
    const uint32_t n = (uint32_t)g().mirror.size();
    std::vector<uint8_t> used(tl_shapes.size(), 0);
    for (uint32_t i = 0; i < n; i++)
        if (g().mirror[i].kind != PUPIL_SHAPE_SPHERE) used[inst_shape[i]] = 1;
    // built with every instance shown, as create builds; the masks follow
    std::vector<DevInstance> copy = g().mirror;
    std::vector<uint32_t> hidden;
    for (uint32_t i = 0; i < n; i++)
        if (copy[i].hidden) {
            hidden.push_back(i);
            copy[i].hidden = 0u;
        }
    TwoLevelAccel ntl{};
    int rc = -5;
    const bool stage_only = tl.world && used == tl.shape_used;
    if (stage_only) rc = set_two_level_instances(tl_shapes, inst_shape, copy, g().insts.get(), t.stream, tl, ntl);
    if (rc == 0) {
        last_whole_rebuild = 0;
    } else if (rc == -5) {
        // A shape without a BLAS in tl gains its first instance: its arrays as they are now, and vmax
        // as at create.  While no instance showed it, a vertex update or a replacement left no
        // trace here, so nothing an earlier use left in tl_shapes[k] may be trusted.
        for (size_t k = 0; k < tl_shapes.size(); k++) {
            TwoLevelShape &ts = tl_shapes[k];
            if (!used[k] || (k < tl.shape_used.size() && tl.shape_used[k])) continue;
            ts = TwoLevelShape{};
            ts.num_faces = shapes[k].num_faces;
            ts.num_vertices = shapes[k].num_vertices;
            ts.positions = shapes[k].pos.get();
            ts.normals = shapes[k].nrm.get();
            ts.texcoords = shapes[k].tex.get();
            ts.indices = shapes[k].idx.get();
            if (shape_abs_max(tl, ts, &ts.vmax, t.stream) != 0) return undo(fail(PUPIL_ERR_HIP, "vertex reduction failed"));
        }
        copy = g().mirror;
        for (uint32_t id : hidden) copy[id].hidden = 0u;
        rc = build_two_level(tl_shapes, inst_shape, copy, g().insts.get(), t.materials->device(), leaf_size, t.stream, ntl);
    }
    auto drop = [&]() {
        if (last_whole_rebuild) free_two_level(ntl);
        else free_instance_stage(ntl);
    };
    if (rc == 0 && !hidden.empty()) {  // the masks, as pupil_pt_update_instances_masked puts them on a fresh engine
        std::vector<DevInstance> staged;
        staged.reserve(hidden.size());
        for (uint32_t id : hidden) {
            copy[id].hidden = 1u;
            staged.push_back(device_instance(copy[id]));
            if (hipMemcpyAsync(g().insts.get() + id, &staged.back(), sizeof(DevInstance), hipMemcpyHostToDevice, t.stream) != hipSuccess)
                rc = -1;
        }
        if (rc == 0)
            rc = rebuild_tlas(ntl, copy, g().insts.get(), hidden, t.stream, !is_rebuild(std::getenv("PUPIL_TL_UPDATE")));
        if (rc != 0) (void)hipStreamSynchronize(t.stream);  // `staged` outlives its copies
    }
    rc = rc != 0 ? builder_error(rc, true, "two-level acceleration rebuild failed") : node_limit(nodes4_of(ntl));
    if (rc != PUPIL_OK) {  // the old structure stays
        drop();
        return undo(rc);
    }
    last_blas_builds = ntl.blas_builds;
    for (size_t k = 0; k < tl_shapes.size(); k++)  // a shape that lost its last instance is forgotten
        if (!used[k]) tl_shapes[k] = TwoLevelShape{};
    if (last_whole_rebuild) free_two_level(tl);
    else free_instance_stage(tl);
    tl = ntl;
    g().mirror = copy;
    ms = tl.build_ms;
    return publish();
}

}  // namespace pupil
