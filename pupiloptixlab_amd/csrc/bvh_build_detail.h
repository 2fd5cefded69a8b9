// bvh_build_detail.h — what the builder's files share (bvh_build.hip, bvh_sort.hip, bvh_ploc.hip,
// bvh_reinsert.hip, bvh_collapse.hip, bvh_refit.hip).  Internal: nothing outside the builder
// includes it; the public entry points are declared in pt_kernels.h.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "bvh4_quant.h"
#include "host/scoped_buffer.h"
#include "pt_kernels.h"

namespace pupil::bvh {

constexpr int kBlock = 256;
inline dim3 grid_for(int m) { return dim3((unsigned)((m + kBlock - 1) / kBlock)); }

struct Aabb {
    float lo[3];
    float hi[3];
};

__device__ __forceinline__ Aabb merge(const Aabb &a, const Aabb &b) {
    Aabb r;
    for (int k = 0; k < 3; k++) {
        r.lo[k] = fminf(a.lo[k], b.lo[k]);
        r.hi[k] = fmaxf(a.hi[k], b.hi[k]);
    }
    return r;
}

__device__ __forceinline__ float half_area(const Aabb &b) {
    const float dx = b.hi[0] - b.lo[0], dy = b.hi[1] - b.lo[1], dz = b.hi[2] - b.lo[2];
    return dx * dy + dy * dz + dz * dx;
}

// ---------------------------------------------------------------- device scratch
// One hipMalloc per buffer, freed when the holder goes out of scope; release() hands a pointer
// on to BvhBuildOutput.
struct HipAlloc {
    static hipError_t alloc(void **p, size_t bytes) { return hipMalloc(p, bytes); }
    static void free(void *p) { (void)hipFree(p); }
};
template <typename T>
using DevBuf = ScopedBuffer<T, HipAlloc>;

// Allocates unless an earlier allocation of the same sequence failed (err is set already), so a
// block of declarations reads top to bottom and is followed by one `if (err) return err;`.
template <typename T>
DevBuf<T> scratch(hipError_t &err, size_t count) {
    DevBuf<T> b;
    if (!err) err = b.alloc(count);
    return b;
}

// ---------------------------------------------------------------- options
// Everything the environment decides about a build, read once at the entry points
// (read_build_options, bvh_build.hip) and passed down.
struct BuildOptions {
    enum class Builder { Ploc, Karras };
    enum class Collapse { Sah, Greedy, Parity };
    Builder builder = Builder::Ploc;    // PUPIL_BVH_BUILDER=lbvh: Karras
    Collapse collapse = Collapse::Sah;  // PUPIL_BVH4_COLLAPSE=greedy | parity
    uint32_t sah_leaf = 0;              // PUPIL_SAH_LEAF, clamped to [leaf_size, 8]; default leaf_size
    int reinsert_rounds = 0;            // PUPIL_BVH_REINSERT, clamped to [0, 64]; default 2
    bool reinsert_log = false;          // PUPIL_BVH_REINSERT_LOG: one line per build on stderr
};

// ---------------------------------------------------------------- 64-bit exclusive scan
constexpr int kScanBlock = 1024;
constexpr int kScanItems = 4;
constexpr int kScanPer = kScanBlock * kScanItems;  // items per block of the block pass
inline int scan64_blocks(int n) { return (n + kScanPer - 1) / kScanPer; }
// In-place exclusive scan of n 64-bit counts (block pass, block-sum pass, add pass).  sums:
// scan64_blocks(n) entries, total: one entry, both device scratch of the caller; the grand total
// is left in *total.  host_total (optional): a copy of the total is queued right behind the
// scan, valid after the caller's next synchronisation.  hipErrorInvalidValue, before anything
// is launched, when the block sums do not fit one block (n > 16.7 M).
hipError_t scan64(unsigned long long *data, int n, unsigned long long *sums, unsigned long long *total,
                  hipStream_t s, unsigned long long *host_total = nullptr);

// In-place exclusive scan of `count` 32-bit counts by one block (bvh_sort.hip: the radix sort's
// histogram scan; the parity collapse numbers its nodes with it).
void scan32(uint32_t *data, uint32_t count, hipStream_t s);

// ---------------------------------------------------------------- stages
// The arrays the front end (Morton order, binary tree) keeps on the device for n boxes; both
// drivers allocate them through this, in this order.
struct BinaryTree;
struct FrontEnd {
    DevBuf<Aabb> boxes, node_boxes;
    DevBuf<uint32_t> bounds, keys, vals, keys2, vals2, hist;
    DevBuf<uint32_t> refit_flags;  // arrival counters of the Karras refit (build_lbvh only)
    DevBuf<int2> children, ranges;
    DevBuf<int> parent_internal, parent_leaf;
    // morton_order: the sorted keys / values and the sort's other pair of buffers;
    // binary_tree: sorted_vals is the tree's final primitive order (PLOC writes a new one)
    uint32_t *sorted_keys = nullptr, *sorted_vals = nullptr, *spare_keys = nullptr, *spare_vals = nullptr;

    FrontEnd(hipError_t &err, int n, bool with_refit_flags);
    BinaryTree tree(int n) const;
};

// Binary tree over n primitives: root 0, child >= 0 internal node, < 0 leaf ~position in
// prim_order; ranges[i] the positions under node i (contiguous).
struct BinaryTree {
    int n;
    const uint32_t *prim_order;
    const Aabb *prim_boxes;
    const int2 *children, *ranges;
    const Aabb *node_boxes;
    const int *parent_internal;
};

// Stage 1 (bvh_sort.hip): centroid bounds, 30-bit Morton codes of fe.boxes, four radix passes.
void morton_order(FrontEnd &fe, int n, hipStream_t s);

// Stage 2 (bvh_ploc.hip), n >= 2: Karras hierarchy + bottom-up boxes, or PLOC with the
// reinsertion rounds inside.  Fills children / ranges / node_boxes / parents.
hipError_t binary_tree(FrontEnd &fe, int n, const BuildOptions &opts, hipStream_t s, ReinsertLog *log = nullptr);

// Parallel reinsertion over the PLOC creation-id tree, in place (bvh_reinsert.hip).  Out of
// memory for its scratch leaves the tree as it is and is no error.
hipError_t reinsert_ploc(int n, const BuildOptions &opts, const uint32_t *vals_in, const Aabb *prim_boxes,
                         int2 *node_child, Aabb *node_box, int *node_count, ReinsertLog *log, hipStream_t s);

// Stage 3 (bvh_collapse.hip): the 4-wide quantized tree by opts.collapse.  level_start: first
// node of each level and the end (breadth first); the parity collapse leaves it empty.
// spare_a / spare_b: n words each of scratch the caller can spare (the parity collapse keeps its
// depths and flags there; the others do not touch them).
struct Collapsed {
    DevBuf<Bvh4Node> nodes4;
    uint32_t num_nodes4 = 0, depth4 = 0;
    std::vector<uint32_t> level_start;
};
hipError_t collapse_bvh4(const BinaryTree &t, uint32_t leaf_size, const BuildOptions &opts, uint32_t *spare_a,
                         uint32_t *spare_b, hipStream_t s, Collapsed &out);

}  // namespace pupil::bvh
