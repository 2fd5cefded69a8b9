// scene_tables.h — SceneTables, the one owner of the tables the acceleration structure and the
// shading are built over: the instance table, its host mirror and the three primitive -> instance
// tables (pt_scene.h DeviceScene::instances / prim_inst / inst_first / inst_guide).
// Plain C++ (no HIP): the device is a policy, so the ownership paths run on the host under a
// sanitizer (tests/scene_tables_driver.cpp).
//   Dev::alloc / Dev::free: as host/scoped_buffer.h          Dev::Stream: what work is enqueued on
//   Dev::fill(g, stream) -> ABI code: g.first goes up to g.inst_first, and g.prim_inst and
//       g.inst_guide are filled from it on the device (pt_replace.hip), enqueued on the stream
#pragma once

#include <string>
#include <utility>
#include <vector>

#include "../pt_scene.h"
#include "prim_tables.h"
#include "scoped_buffer.h"

namespace pupil {

int fail(int code, const std::string &msg);  // engine.hip: the code, msg left for pupil_last_error

// One generation of the tables, a value: moving one over another frees the old device arrays.
template <typename Dev>
struct TableGeneration {
    ScopedBuffer<DevInstance, Dev> insts;                        // num_instances records
    ScopedBuffer<uint32_t, Dev> prim_inst, inst_first, inst_guide;  // num_prims, num_instances + 1, guide_entries
    uint32_t num_instances = 0, num_prims = 0, guide_shift = 0, guide_entries = 2;
    std::vector<DevInstance> mirror;  // the host's copy of insts (a hidden sphere keeps its real to_object here)
    std::vector<uint32_t> first;      // the host's copy of inst_first: each instance's prim_offset, then num_prims
};

template <typename Dev>
class SceneTables {
public:
    using Generation = TableGeneration<Dev>;

    // The "aside" step of create and of every update that resizes a table.  counts[i]: primitives
    // of instance i.  `out` gets the four arrays, the counts and `first`; inst_first, prim_inst and
    // inst_guide are written on the stream, insts and the mirror (n value-initialised records) are
    // the caller's to fill.  Nothing the engine reads changes.  flat: the flattened BVH's limit
    // applies.  After a failure `out` may own arrays the stream still writes: the caller lets the
    // stream pass before `out` goes.
    static int stage(const uint32_t *counts, uint32_t n, bool flat, typename Dev::Stream stream, Generation &out) {
        PrimTables tab;
        if (!prim_tables(counts, n, &tab)) return fail(PUPIL_ERR_UNSUPPORTED, "more than 2^31 primitives");
        if (flat && tab.num_prims >= (1u << 27))
            return fail(PUPIL_ERR_UNSUPPORTED, "flattened BVH limited to 2^27 primitives");
        if (out.insts.alloc(n) || out.prim_inst.alloc(tab.num_prims) || out.inst_first.alloc(tab.inst_first.size()) ||
            out.inst_guide.alloc(tab.guide_entries))
            return fail(PUPIL_ERR_OOM, "scene tables: allocation failed");
        out.num_instances = n;
        out.num_prims = tab.num_prims;
        out.guide_shift = tab.guide_shift;
        out.guide_entries = tab.guide_entries;
        out.first = std::move(tab.inst_first);
        out.mirror.assign(n, DevInstance{});
        return Dev::fill(out, stream);
    }

    // The swap: `staged` becomes the current generation, the previous one's arrays are freed (no
    // stream may still read them), and the scene and the totals follow.  The only writer of these
    // fields of DeviceScene and of totals.bvh_prims.
    void adopt(Generation &&staged, DeviceScene &sc, pupil_pt_counters &totals) {
        cur_ = std::move(staged);
        sc.instances = cur_.insts.get();
        sc.num_instances = cur_.num_instances;
        sc.prim_inst = cur_.prim_inst.get();
        sc.inst_first = cur_.inst_first.get();
        sc.inst_guide = cur_.inst_guide.get();
        sc.inst_guide_shift = cur_.guide_shift;
        sc.num_prims = cur_.num_prims;
        totals.bvh_prims = cur_.num_prims;
    }

    // the current generation: readers, and the updates that rewrite records in place
    Generation &cur() { return cur_; }
    const Generation &cur() const { return cur_; }

private:
    Generation cur_;
};

}  // namespace pupil
