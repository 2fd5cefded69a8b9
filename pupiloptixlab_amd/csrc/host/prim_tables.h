// prim_tables.h — the geometry of the primitive -> instance tables (pt_scene.h DeviceScene::
// prim_inst / inst_first / inst_guide) from the instances' primitive counts: what the host
// computes when a mesh is replaced (pupil_pt_replace_shape_mesh), num_instances numbers, while
// the per-primitive tables are filled on the device (pt_replace.hip) by the lookup below.
// Host-only C++ but for that one function, which the fill kernel shares.
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

#if defined(__HIPCC__)
#define PUPIL_PRIM_HD __host__ __device__ inline
#else
#define PUPIL_PRIM_HD inline
#endif

namespace pupil {

// most buckets of the guide table before its shift goes up (a few kB that stay in the L1 / L2)
constexpr uint32_t kGuideBuckets = 8192u;

// the guide's shift for num_prims primitives: the smallest with num_prims >> shift <= kGuideBuckets
inline uint32_t prim_guide_shift(uint64_t num_prims) {
    uint32_t shift = 0;
    while ((num_prims >> shift) > kGuideBuckets) shift++;
    return shift;
}

struct PrimTables {
    std::vector<uint32_t> inst_first;  // num_instances + 1: each instance's first global primitive id, then num_prims
    uint32_t num_prims = 0;
    uint32_t guide_shift = 0;
    uint32_t guide_entries = 2;  // entries of inst_guide: buckets + 1 (an empty scene: two zeros)
};

// counts[i]: primitives of instance i (a mesh's faces, 1 for a sphere).  false: 2^31 primitives
// or more (global primitive ids keep their top bit for the sphere flag), *out is left unspecified
inline bool prim_tables(const uint32_t *counts, size_t num_instances, PrimTables *out) {
    out->inst_first.resize(num_instances + 1);
    uint64_t sum = 0;
    for (size_t i = 0; i < num_instances; i++) {
        out->inst_first[i] = (uint32_t)sum;
        sum += counts[i];
        if (sum >= (1ull << 31)) return false;
    }
    out->inst_first[num_instances] = (uint32_t)sum;
    out->num_prims = (uint32_t)sum;
    out->guide_shift = prim_guide_shift(sum);
    out->guide_entries = sum ? (uint32_t)(((sum - 1) >> out->guide_shift) + 1) + 1u : 2u;
    return true;
}

// the instance that holds primitive p < inst_first[num_instances]: the last i with
// inst_first[i] <= p (an instance without primitives shares its first id with the next one,
// which is the one that holds it) -- what prim_inst[p] is
PUPIL_PRIM_HD uint32_t prim_holder(const uint32_t *inst_first, uint32_t num_instances, uint32_t p) {
    uint32_t lo = 0, hi = num_instances;  // inst_first[lo] <= p < inst_first[hi]
    while (hi - lo > 1u) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (inst_first[mid] <= p) lo = mid;
        else hi = mid;
    }
    return lo;
}

// inst_guide[k] for k < guide_entries: the instance holding prim min(k << shift, num_prims - 1)
PUPIL_PRIM_HD uint32_t prim_guide_entry(const uint32_t *inst_first, uint32_t num_instances, uint32_t num_prims,
                                        uint32_t shift, uint32_t k) {
    if (num_prims == 0) return 0u;
    const uint64_t p = (uint64_t)k << shift;
    return prim_holder(inst_first, num_instances, p < num_prims ? (uint32_t)p : num_prims - 1u);
}

}  // namespace pupil
