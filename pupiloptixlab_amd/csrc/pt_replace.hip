// pt_replace.hip — the device side of pupil_pt_replace_shape_mesh: what hangs off a shape's
// primitive count is rewritten from the engine's own arrays, so that a mesh given in device
// memory never passes through the host.
//
//   k_index_max      the largest of the new mesh's indices (the call refuses one >= num_vertices):
//                    grid-stride, wave reduction, one atomic per block; 4 bytes come back
//   k_prim_tables    prim_inst and inst_guide from the new inst_first (host/prim_tables.h: the
//                    host sums num_instances counts, the per-primitive tables are filled here)
//   k_patch_instances  the new instance table: every instance's prim_offset, and the array
//                    pointers of the instances that show the replaced shape
//
// All three are bound by their stores or loads; nothing here is tuned beyond coalescing.
#include <hip/hip_runtime.h>

#include "host/prim_tables.h"
#include "pt_kernels.h"

namespace pupil {
namespace {

constexpr uint32_t kBlock = 256;

__global__ __launch_bounds__(kBlock) void k_index_max(const uint32_t *idx, size_t n, uint32_t *out) {
    __shared__ uint32_t wave_max[kBlock / 64];
    uint32_t m = 0;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
        m = max(m, idx[i]);
    for (int s = 32; s > 0; s >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, s));
    if ((threadIdx.x & 63u) == 0u) wave_max[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (uint32_t w = 1; w < kBlock / 64; w++) m = max(m, wave_max[w]);
        atomicMax(out, m);
    }
}

// threads [0, num_prims): prim_inst; the next guide_entries threads: inst_guide
__global__ __launch_bounds__(kBlock) void k_prim_tables(const uint32_t *inst_first, uint32_t num_instances,
                                                        uint32_t num_prims, uint32_t shift, uint32_t guide_entries,
                                                        uint32_t *prim_inst, uint32_t *inst_guide) {
    const uint64_t total = (uint64_t)num_prims + guide_entries;
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < total; i += (uint64_t)gridDim.x * blockDim.x) {
        if (i < num_prims)
            prim_inst[i] = prim_holder(inst_first, num_instances, (uint32_t)i);
        else
            inst_guide[i - num_prims] = prim_guide_entry(inst_first, num_instances, num_prims, shift, (uint32_t)(i - num_prims));
    }
}

__global__ __launch_bounds__(kBlock) void k_patch_instances(ReplaceMeshJob j) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= j.num_instances) return;
    DevInstance &d = j.instances[i];
    d.prim_offset = j.inst_first[i];
    if (j.emitter_offsets) d.emitter_offset = j.emitter_offsets[i];
    // a shape's instances all point at the shape's one position array, and no other shape's do
    if (d.kind == PUPIL_SHAPE_MESH && d.positions == j.old_positions) {
        d.positions = j.positions;
        d.normals = j.normals;
        d.texcoords = j.texcoords;
        d.indices = j.indices;
    }
}

uint32_t blocks_for(uint64_t n, uint32_t cap) {
    const uint64_t b = (n + kBlock - 1) / kBlock;
    return (uint32_t)(b < 1 ? 1 : b > cap ? cap : b);
}

}  // namespace

void launch_index_max(const uint32_t *idx, size_t n, uint32_t *out, hipStream_t s) {
    hipLaunchKernelGGL(k_index_max, dim3(blocks_for(n, 1024u)), dim3(kBlock), 0, s, idx, n, out);
}

void launch_prim_tables(const uint32_t *inst_first, uint32_t num_instances, uint32_t num_prims, uint32_t shift,
                        uint32_t guide_entries, uint32_t *prim_inst, uint32_t *inst_guide, hipStream_t s) {
    hipLaunchKernelGGL(k_prim_tables, dim3(blocks_for((uint64_t)num_prims + guide_entries, 1u << 16)), dim3(kBlock), 0, s,
                       inst_first, num_instances, num_prims, shift, guide_entries, prim_inst, inst_guide);
}

void launch_patch_instances(const ReplaceMeshJob &job, hipStream_t s) {
    if (job.num_instances)
        hipLaunchKernelGGL(k_patch_instances, dim3((job.num_instances + kBlock - 1) / kBlock), dim3(kBlock), 0, s, job);
}

}  // namespace pupil
