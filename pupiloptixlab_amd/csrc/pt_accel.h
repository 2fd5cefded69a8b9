// pt_accel.h — SceneAccel, the one owner of the engine's acceleration structure (pt_accel.hip),
// and what the engine's host code shares with it.
#pragma once

#include <chrono>
#include <string>

#include "../../include/pupil_pt.h"
#include "accel_two_level.h"
#include "host/emitter_tables.h"
#include "host/material_tables.h"
#include "host/scene_tables.h"

namespace pupil {

// the ABI code, with msg left for pupil_last_error (engine.hip)
int fail(int code, const std::string &msg);

#define HIP_TRY(expr)                                                                                     \
    do {                                                                                                  \
        hipError_t _e = (expr);                                                                           \
        if (_e != hipSuccess)                                                                             \
            return fail(_e == hipErrorOutOfMemory ? PUPIL_ERR_OOM : PUPIL_ERR_HIP,                        \
                        std::string(#expr) + ": " + hipGetErrorString(_e));                               \
    } while (0)

// the host clock: milliseconds since t0
inline double ms_since(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

// After the first enqueue of an update that builds aside: the stream passes what it holds before
// the call's own buffers go with the return.
inline int drained(hipStream_t stream, int rc) {
    (void)hipStreamSynchronize(stream);
    return rc;
}
#define HIP_TRY_DRAINED(stream, expr)                                                                     \
    do {                                                                                                  \
        hipError_t _e = (expr);                                                                           \
        if (_e != hipSuccess)                                                                             \
            return drained(stream, fail(_e == hipErrorOutOfMemory ? PUPIL_ERR_OOM : PUPIL_ERR_HIP,        \
                                        std::string(#expr) + ": " + hipGetErrorString(_e)));              \
    } while (0)

// the device of the engine's tables (host/scene_tables.h, host/emitter_tables.h, host/material_tables.h),
// of its shapes and of every scratch
struct HipDevice {
    using Stream = hipStream_t;
    static hipError_t alloc(void **p, size_t bytes) {
        const hipError_t e = hipMalloc(p, bytes);
        if (e != hipSuccess) (void)hipGetLastError();
        return e;
    }
    static void free(void *p) { (void)hipFree(p); }
    static void destroy(hipEvent_t e) { (void)hipEventDestroy(e); }
    static void destroy(hipStream_t s) { (void)hipStreamDestroy(s); }
    static int fill(const TableGeneration<HipDevice> &g, hipStream_t stream) {
        HIP_TRY(hipMemcpyAsync(g.inst_first.get(), g.first.data(), sizeof(uint32_t) * g.first.size(), hipMemcpyHostToDevice,
                               stream));
        launch_prim_tables(g.inst_first.get(), g.num_instances, g.num_prims, g.guide_shift, g.guide_entries,
                           g.prim_inst.get(), g.inst_guide.get(), stream);
        return PUPIL_OK;
    }
    static hipError_t upload(void *dst, const void *src, size_t bytes) { return hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice); }
    static hipError_t download(void *dst, const void *src, size_t bytes) { return hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost); }
    static hipError_t copy(void *dst, const void *src, size_t bytes) {  // device to device, complete on return
        const hipError_t e = hipMemcpy(dst, src, bytes, hipMemcpyDeviceToDevice);
        return e == hipSuccess ? hipStreamSynchronize(nullptr) : e;
    }
    static int failed(hipError_t e, const char *what) {  // what HIP_TRY(what) returns
        if (e == hipSuccess) return PUPIL_OK;
        return fail(e == hipErrorOutOfMemory ? PUPIL_ERR_OOM : PUPIL_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
    }
    static int write(void *dst, const void *src, size_t bytes, hipStream_t stream) {
        return failed(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, stream), "hipMemcpyAsync");
    }
    static int sync(hipStream_t stream) { return failed(hipStreamSynchronize(stream), "hipStreamSynchronize"); }
    static int env_tables(const DevEmitter &e, const void *rgba, float *sums, DevEmitter *env, hipStream_t stream) {
        HIP_TRY(hipMemcpyAsync((void *)e.radiance.data, rgba, sizeof(float4) * (size_t)e.map_w * e.map_h,
                               hipMemcpyDeviceToDevice, stream));
        launch_env_tables({e.radiance.data, e.map_w, e.map_h, const_cast<float *>(e.col_cdf), const_cast<float *>(e.row_cdf),
                           e.row_weight, sums, env},
                          stream);
        return failed(hipGetLastError(), "hipGetLastError()");
    }
};
using EngineTables = SceneTables<HipDevice>;
using EngineEmitters = EmitterTables<HipDevice>;
using EngineMaterials = MaterialTables<HipDevice>;

// a shape and its device arrays (those the instances point at), a value: moving one over another
// frees the old arrays
struct ShapeDev {
    uint32_t kind = PUPIL_SHAPE_MESH, num_vertices = 0, num_faces = 0;
    ScopedBuffer<float, HipDevice> pos, nrm, tex;
    ScopedBuffer<uint32_t, HipDevice> idx;
    // pupil_pt_snapshot_shape_vertices: the vertices from before an update (allocated on the
    // first snapshot and kept), and whether the flow pass uses them
    ScopedBuffer<float, HipDevice> prev;
    bool prev_valid = false;
};

// Acceleration structure (replaces the GAS + IAS builds): one flattened BVH over world-space
// primitives, or a TLAS over per-shape BLASes (accel_two_level.hip).  Both give bit-identical
// hits.  Everything that builds, refits, rebuilds or frees it is here; publish() is the only
// writer of the structure's fields of DeviceScene and of totals.bvh_nodes / bvh_depth /
// two_level, and every update ends in it.
struct SceneAccel {
    // What the structure is built over and publishes to, valid for the engine's life.  The
    // instance and primitive tables are read through their owner, never copied: before an update
    // its current generation (mirror and device table) already holds the new transforms and
    // masks, and the shapes' device arrays the new vertices.
    // The hand-off of an update that resizes a table (replace_shape, set_instances), in one place:
    // the engine stages a generation aside (SceneTables::stage) and fills its instance table and
    // mirror; for the length of the call the structure reads that generation instead of the
    // current one and builds over it; on success the engine adopts it (SceneTables::adopt), on
    // failure the current tables and the old structure are untouched and the staged generation
    // goes with the engine's call.
    using Generation = EngineTables::Generation;
    struct Tables {
        hipStream_t stream;  // the engine's own
        EngineTables *tables;
        const EngineMaterials *materials;
        DeviceScene *sc;
        pupil_pt_counters *totals;
    };
    // Chooses flat or two-level and builds it.  publish() is left to the end of create: the
    // ring budget is read between the two, before the engine's first kernel launch.
    int build(const Tables &tables, const pupil_scene_desc *scene, const std::vector<ShapeDev> &shapes);
    // the instances in `changed` moved, were hidden or shown
    int update_instances(const std::vector<uint32_t> &changed);
    // the vertices of mesh shape `shape`, shown by the instances in `changed`, were replaced;
    // rebuild: PUPIL_VERTS_REBUILD
    int update_shape(uint32_t shape, const std::vector<uint32_t> &changed, bool rebuild);
    // Mesh shape `shape` got new topology (pupil_pt_replace_shape_mesh).  The engine has built
    // aside, on the stream: `mesh`, the shape's new arrays and counts, and `staged`, whose
    // instance table and mirror carry the new prim offsets and array pointers.  When an instance
    // shows the shape (`used`), the structure is rebuilt over `staged` as by update_shape(rebuild)
    // and published.
    int replace_shape(uint32_t shape, const ShapeDev &mesh, bool used, Generation &staged);
    // The instance table was replaced as a whole (pupil_pt_set_instances).  The engine has built
    // aside, on the stream: `staged` (its instance table by k_fill_instances) and `shape_of`, the
    // shape of each new instance.  The structure is built over `staged` and published.  Flattened: one
    // build, as update_shape(rebuild).  Two-level, world mode, the set of mesh shapes shown by at
    // least one instance unchanged: the instance stage alone (set_two_level_instances) on freshly
    // sized per-instance arrays -- no BLAS builder runs.  Two-level otherwise -- the set changed,
    // so a BLAS is missing or left over, or object mode, whose BLASes lie behind a TLAS reserve of
    // one node per instance and whose links move with the instance count -- the whole structure is
    // built anew.  Both two-level paths fill the instances' two-level fields in the host mirror and
    // upload the table again, as create does.  A shape that gains its first instance takes its
    // arrays and vmax from `shapes` as they are now; one that loses its last is forgotten.
    // Masks go on after the build, as a fresh engine's do after create.  On success `shape_of`
    // holds the previous shapes.
    // last_blas_builds / last_whole_rebuild: what the last call ran (flattened: 0 / 1).
    int set_instances(Generation &staged, std::vector<uint32_t> &shape_of, const std::vector<ShapeDev> &shapes);
    uint32_t last_blas_builds = 0, last_whole_rebuild = 0;
    // Instances moved on the device (pupil_pt_update_instances_device), in three steps whose kernel
    // launches and synchronisations do not depend on how many moved (flattened BVH, two-level world
    // mode; object mode rebuilds its TLAS through update_instances, correct and no more).
    // move_begin: what the transform kernel writes besides the instance table -- the id list of the
    // structure kernels (two-level; null otherwise) and the cleared moved flags (flattened; null
    // otherwise).  move_boxes (two-level, `count` list entries written): the instances' world
    // boxes, also to box[stride * k] on the device.  move_finish, once insts holds what the device
    // computed for `changed` (the ids of the list in range): the structure follows, then publish().
    int move_begin(uint32_t **list, uint8_t **moved);
    void move_boxes(uint32_t count, float *box, uint32_t stride);
    int move_finish(const std::vector<uint32_t> &changed, uint32_t count);
    // kernel launches and stream / event synchronisations of the structure's own code since the
    // caller cleared them, counted where they are made, on the paths the device move takes
    struct Counts {
        uint32_t launches = 0, syncs = 0;
    } counts;
    // the material bins of instances changed (insts / d_insts hold the new ones): the bin words of
    // the record slots follow, enqueued on the stream.  No box or link changes: not a refit
    void update_bins();
    // slots of the world-space records update_bins walks (the flattened BVH's, or the two-level
    // world records; world mode: with the spheres' leaves), the array the terminal-ray cull set
    // indexes when the traversal reads it (DeviceScene::prims: flat and world mode)
    uint32_t world_record_slots() const;
    int publish();
    // BVH4 node array the traversal walks (its size bounds the 32-bit node offsets, kMaxNodes4)
    uint64_t nodes4_count() const;
    void free();

    bool two_level = false;  // TLAS + per-shape BLAS instead of one flattened BVH
    BvhBuildOutput bvh{};
    TwoLevelAccel tl{};
    std::vector<TwoLevelShape> tl_shapes;  // the two-level build's input (PUPIL_VERTS_REBUILD)
    std::vector<uint32_t> inst_shape;      // shape of each instance
    uint32_t leaf_size = 2;                // primitives per BVH leaf (PUPIL_LEAF_SIZE)
    // build_ms, one rule: the structure's own time is `ms` -- the builder's timer at create and
    // the refit's or rebuild's after a flattened update; the two-level updates have no timer, so
    // an instance update takes the host clock around the TLAS update and publish().  The entry
    // points report `ms`, except pupil_pt_update_shape_vertices, which reports the host clock
    // around its whole call (vertex copies included) in every mode.
    double ms = 0.0;
    uint64_t refits = 0;  // accel_refits; ticked by the entry points, not here

private:
    // flagged: d_moved already holds the flags of `changed` (move_begin + the transform kernel)
    int update_flat(const std::vector<uint32_t> &changed, bool refit, bool attrs, bool flagged = false);
    int update_tlas(const std::vector<uint32_t> &changed);
    int flag_instances(const std::vector<uint32_t> *changed, uint32_t nodes);
    Tables t{};
    // the generation the structure reads: the current one, or `over` for the length of a hand-off
    Generation *over = nullptr;
    Generation &g() const { return over ? *over : t.tables->cur(); }
    struct BuildOver {  // scope of a hand-off
        SceneAccel &a;
        BuildOver(SceneAccel &accel, Generation &staged) : a(accel) { a.over = &staged; }
        ~BuildOver() { a.over = nullptr; }
    };
    // flattened-BVH refits: per-instance moved flags and the node-box scratch
    uint8_t *d_moved = nullptr;
    std::vector<uint8_t> h_moved;
    float *refit_box = nullptr;
    uint32_t *node_bound = nullptr;  // launch_node_bound's result (3 floats as bits)
};

}  // namespace pupil
