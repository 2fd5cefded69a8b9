// pt_instance_set.hip — the device side of pupil_pt_set_instances: a new instance table filled
// from what each instance binds, so that transforms given in device memory never pass through the
// host on their way into the table.
//
//   k_fill_instances  one thread per new instance assembles its whole 224-byte DevInstance
//                     (host/instance_record.h, the text the host mirror and create's tables share):
//                     the shape's arrays from a small per-shape table, the bindings the host
//                     uploaded, prim_offset from inst_first, the transform from the caller's block
//                     with its inverse (pt_invert.h) or both from the host's upload, and the NaN
//                     to_object of a hidden sphere's device copy.  The two-level fields are left as
//                     create's upload leaves them; the structure's instance stage fills them.
//
// Bound by its stores: the record is built in registers and leaves as fourteen 16-byte stores.
#include <hip/hip_runtime.h>

#include "pt_kernels.h"

namespace pupil {
namespace {

constexpr uint32_t kBlock = 256;
constexpr uint32_t kRecordVecs = sizeof(DevInstance) / sizeof(uint4);
static_assert(sizeof(DevInstance) % sizeof(uint4) == 0, "the record leaves as whole 16-byte stores");

__global__ __launch_bounds__(kBlock) void k_fill_instances(FillInstancesJob j) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= j.n) return;
    const InstBinding b = j.bindings[i];
    const InstShape sh = j.shapes[b.shape];  // b.shape < num_shapes: the host checked every binding
    float tw[12], to[12];
    for (int c = 0; c < 12; c++) tw[c] = j.to_world[12 * (size_t)i + c];
    if (j.to_object)
        for (int c = 0; c < 12; c++) to[c] = j.to_object[12 * (size_t)i + c];
    union {
        DevInstance d;
        uint4 v[kRecordVecs];
    } rec;
    fill_instance_record(rec.d, sh, b, j.inst_first[i], tw, j.to_object ? to : nullptr, true);
    uint4 *out = reinterpret_cast<uint4 *>(j.out + i);  // 224-byte stride from a hipMalloc base: 16-byte aligned
#pragma unroll
    for (uint32_t k = 0; k < kRecordVecs; k++) out[k] = rec.v[k];
}

}  // namespace

void launch_fill_instances(const FillInstancesJob &job, hipStream_t s) {
    if (job.n) hipLaunchKernelGGL(k_fill_instances, dim3((job.n + kBlock - 1) / kBlock), dim3(kBlock), 0, s, job);
}

}  // namespace pupil
