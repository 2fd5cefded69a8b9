// accel_two_level.h — two-level acceleration structure (TLAS over instances,
// one object-space BLAS per mesh shape); see accel_two_level.hip.
#pragma once

#include <array>
#include <utility>
#include <vector>

#include "pt_kernels.h"  // host/instance_record.h: instance_margin_values

namespace pupil {

struct TwoLevelShape {  // one mesh shape (device arrays, object space)
    uint32_t num_faces, num_vertices;
    const float *positions, *normals, *texcoords;
    const uint32_t *indices;
    float vmax;  // largest |coordinate| of its vertices (host-computed; for the box margin)
};

struct TwoLevelAccel {
    Bvh4Node *nodes4 = nullptr;  // [0, tlas_cap) TLAS, then the rebased BLASes
    float4 *prims = nullptr;     // 3 float4 per BLAS primitive, object space, BLAS leaf order; w of [0] = local id
    float4 *attrs = nullptr;     // kAttrStride float4 per BLAS primitive, the mesh's own primitive order
    float4 *wprims = nullptr;    // 3 float4 per (mesh instance, BLAS primitive): world vertices fl(to_world * v),
                                 // instance-major, BLAS leaf order; w of [0] = global primitive id
    uint32_t num_wprims = 0;
    float *d_boxes = nullptr;    // 6 floats per instance: world box
    uint32_t *d_list = nullptr, *d_verts = nullptr;  // scratch: instance list, vertices per instance
    uint32_t *d_faces = nullptr;                     // BLAS primitives per instance (world records)
    uint32_t tlas_cap = 0, tlas_nodes = 0, num_nodes4 = 0, num_prims = 0;
    uint32_t tlas_depth = 0, blas_depth = 0;  // BVH4 levels (deepest BLAS); see kTraceStackEntries
    uint32_t sah_splits = 0;  // TLAS nodes of the last build placed by an SAH (GPU collapse, or host binned splits)
    // "world" mode (PUPIL_TL_MODE, default): every mesh instance gets a world-space copy of
    // its shape's BLAS (child boxes transformed and re-quantised conservatively) and the
    // TLAS is built over the nodes `braid` levels below each instance root, so the whole
    // structure is one BVH4 the flat traversal kernels walk (no ray transform, no
    // return markers, the flat kernel's occupancy).  HBM pays one BLAS copy per instance.
    bool world = false;
    uint32_t braid = 10;  // PUPIL_TL_BRAID
    Bvh4Node *wnodes = nullptr;  // [0, tlas_cap) TLAS, then the per-instance world BLAS copies
    float *d_wbox = nullptr;     // world box of every copied node (6 floats)
    uint32_t num_wnodes = 0;
    std::vector<std::vector<std::pair<int, std::array<float, 6>>>> entries;  // per instance: TLAS entries
    std::vector<uint32_t> inst_shape;                  // shape of each instance (0xFFFFFFFF: sphere)
    std::vector<uint8_t> in_tlas;  // world mode: the instance was visible when the TLAS topology was built
    // world mode: entries[i] is older than the instance's world copy (move_world_instances refits
    // the TLAS and needs no entry); whatever BUILDS a TLAS recomputes the stale ones first
    std::vector<uint8_t> entries_stale;
    // world-mode TLAS refits (GPU, one launch per level, deepest first): the TLAS node ids
    // ordered by level from the deepest (d_tlas_order) and where each level starts in it
    uint32_t *d_tlas_order = nullptr;
    std::vector<uint32_t> tlas_level_start;
    std::vector<std::vector<uint32_t>> shape_levels;   // per shape: BVH4 level starts of its BLAS (+ end)
    // per shape, for vertex updates (update_shape_blas): BLAS record slots (0 = no BLAS), first node /
    // record slot / shading record in the combined arrays, and whether the BLAS is one root leaf
    std::vector<uint32_t> shape_slots, shape_node_base, shape_rec_base, shape_attr_base;
    std::vector<uint8_t> shape_root_leaf;
    // per shape, what the instance stage takes from the shape stage (set_two_level_instances runs
    // it without the BLAS builders): whether the shape has a BLAS, its node count and its root
    // link before rebasing; blas_builds: BLAS builder runs of the build that made this structure
    std::vector<uint8_t> shape_used;
    std::vector<uint32_t> shape_nodes;
    std::vector<int32_t> shape_root;
    uint32_t blas_builds = 0;
    float *d_objbox = nullptr;     // exact box of every object-space node (6 floats), scratch of the BLAS refits
    uint32_t *d_vmax = nullptr;    // update_shape_blas: the max |coordinate| reduction's result
    uint32_t root_link4 = (uint32_t)kTraverseDone;
    double build_ms = 0.0;
};

// Link of a node or leaf of one BLAS after it is copied to node_base / prim_base.
PT_HD int rebase_link(int link, uint32_t node_base, uint32_t prim_base) {
    if (link == kEmptyLink || link == kTraverseDone) return link;
    if (link >= 0) return link + (int)node_base;
    return make_leaf(leaf_first(link) + prim_base, leaf_count(link));
}

// Builds the BLASes, fills the two-level fields of every instance (host copy
// `insts`, uploaded to d_insts), their world boxes and the TLAS.
// inst_shape[i] = shape index of instance i (ignored for spheres).  Returns 0, -1 on a HIP
// error, -3 when the TLAS + BLAS depth exceeds the traversal stacks, -4 when the BLAS record
// slots or instances exceed the 28-bit leaf links (accel_limits.h; past the world-mode limit
// alone the build falls back to object mode instead).
int build_two_level(const std::vector<TwoLevelShape> &shapes, const std::vector<uint32_t> &inst_shape,
                    std::vector<DevInstance> &insts, DevInstance *d_insts, const DevMaterial *d_mats,
                    uint32_t leaf_size, hipStream_t s, TwoLevelAccel &acc);
// build_two_level is two stages (accel_two_level.hip): the shape stage builds the BLASes, the
// object nodes, prims, attrs and the shape_* vectors; the instance stage the instances' fields,
// the world records and world BLAS copies, the boxes, the braided entries, the TLAS and its level
// order.  set_two_level_instances (world mode; pupil_pt_set_instances) runs the instance stage
// alone for a new instance table whose mesh instances show only shapes that have a BLAS in acc:
// `out` shares acc's shape-stage arrays and gets per-instance arrays of its own, built aside.  On
// success the caller frees acc's per-instance arrays (free_instance_stage) and takes out; on
// failure out is empty and acc untouched.  Returns as build_two_level, and -5 when the new table
// does not fit world mode (the caller builds the whole structure instead).
int set_two_level_instances(const std::vector<TwoLevelShape> &shapes, const std::vector<uint32_t> &inst_shape,
                            std::vector<DevInstance> &insts, DevInstance *d_insts, hipStream_t s,
                            const TwoLevelAccel &acc, TwoLevelAccel &out);
void free_instance_stage(TwoLevelAccel &acc);
// Recomputes the world boxes of the `changed` instances (transforms already in
// insts / d_insts) and rebuilds the TLAS.  -3: the TLAS + BLAS depth exceeds the
// traversal stacks (kTraceStackEntries).
// refit (world mode): keep the TLAS topology and refit its boxes instead of rebuilding.
// launches / syncs (or null): the kernels launched and the stream synchronisations made up to the
// refit's are added (a build's own are not counted).
int rebuild_tlas(TwoLevelAccel &acc, std::vector<DevInstance> &insts, DevInstance *d_insts,
                 const std::vector<uint32_t> &changed, hipStream_t s, bool refit = false, uint32_t *launches = nullptr,
                 uint32_t *syncs = nullptr);
// Instances moved on the device (pupil_pt_update_instances_device): acc.d_list holds `count` ids in
// range (repeats allowed) and d_insts their new transforms and margins.
// instance_boxes_device: their world boxes into acc.d_boxes and the device instances' wlo / whi,
// and, box (or null), 6 floats each at box[stride * k] for list entry k.  Two launches.
void instance_boxes_device(TwoLevelAccel &acc, DevInstance *d_insts, uint32_t count, float *box, uint32_t stride,
                           hipStream_t s);
// move_world_instances (world mode; insts already hold what the device computed, the boxes
// included): world records, then the world BLAS copies with ONE launch per BLAS level of each
// moved shape (grid.y over the list; the node arithmetic is k_world_refit's), then the TLAS refit.
// The braided entries of `changed` are only marked stale.  Launches and synchronisations do not
// depend on count.  A TLAS that must be built (PUPIL_TL_UPDATE=rebuild, an instance shown that
// the topology does not hold, no level order) goes through rebuild_tlas.  launches (or null): the
// kernels launched are added.  Returns as rebuild_tlas.
int move_world_instances(TwoLevelAccel &acc, std::vector<DevInstance> &insts, DevInstance *d_insts,
                         const std::vector<uint32_t> &changed, uint32_t count, hipStream_t s, bool refit,
                         uint32_t *launches, uint32_t *syncs);
// Deformed mesh: shape `shape` (its device arrays in `sh` hold the new vertices) gets its
// object-space BLAS records rewritten in place, its BLAS boxes refitted bottom up and its
// shading records refreshed; topology, record slots and id words stay.  vmax (or null):
// receives the new largest |coordinate|, reduced on the device (synchronises s).  The
// instances' margins and rebuild_tlas over the shape's instances follow at the caller.
int update_shape_blas(TwoLevelAccel &acc, uint32_t shape, const TwoLevelShape &sh, float *vmax, hipStream_t s);
// Largest |coordinate| of the shape's device vertices as they are now, reduced on the device
// (4 bytes come back; synchronises s): what TwoLevelShape::vmax holds, without the vertices
// passing through the host.
int shape_abs_max(TwoLevelAccel &acc, const TwoLevelShape &sh, float *vmax, hipStream_t s);
void free_two_level(TwoLevelAccel &acc);
// BLAS box margins of an instance after its transform changed (uses its stored vmax)
void refresh_instance_margins(DevInstance &d);
// nodes of the traversed structure (object mode: TLAS + shared BLASes; world mode: TLAS + copies)
inline uint64_t two_level_nodes(const TwoLevelAccel &a) {
    return a.tlas_nodes + ((a.world ? a.num_wnodes : a.num_nodes4) - a.tlas_cap);
}

}  // namespace pupil
