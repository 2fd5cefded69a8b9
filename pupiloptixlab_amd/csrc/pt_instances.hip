// pt_instances.hip — instance transforms from device memory (pupil_pt_update_instances_device):
// the kernel that takes a list of ids and matrices and writes the engine's instance table.
//
// One thread per list entry does what the host entry does per instance before it uploads it:
// the inverse when the caller gave none (pt_invert.h, the world's own expression in double), the
// two-level box margins (accel_two_level.h instance_margin_values), the NaN to_object of a hidden
// sphere's device copy (pt_scene.h device_instance).  It also leaves the plain values in a staging
// block the host reads back in one copy, the id list the structure kernels take, and the moved
// flags of the flattened refit.  fp64 on a few thousand threads: nothing here is tuned.
#include <hip/hip_runtime.h>

#include "pt_accel.h"
#include "pt_invert.h"
#include "pt_kernels.h"

namespace pupil {
namespace {

__global__ __launch_bounds__(256) void k_move_instances(MoveInstancesJob j) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= j.n) return;
    const uint32_t id = j.ids ? j.ids[k] : k;
    if (id >= j.num_instances) {  // nothing of the entry is read or written
        atomicAdd(j.skipped, 1u);
        if (j.list) j.list[k] = j.fallback;  // an id in range that the list holds anyway
        return;
    }
    DevInstance &d = j.instances[id];
    float tw[12], to[12], margin[2] = {d.margin[0], d.margin[1]};
    for (int c = 0; c < 12; c++) tw[c] = j.to_world[12 * (size_t)k + c];
    if (j.to_object) {
        for (int c = 0; c < 12; c++) to[c] = j.to_object[12 * (size_t)k + c];
    } else {
        invert_affine3x4(tw, to);
    }
    if (j.margins && d.kind != PUPIL_SHAPE_SPHERE) instance_margin_values(tw, to, d.vmax, margin);
    const bool nan_object = d.hidden && d.kind == PUPIL_SHAPE_SPHERE;
    float *st = j.stage + (size_t)kMoveStageFloats * k;
    for (int c = 0; c < 12; c++) {
        d.to_world[c] = tw[c];
        d.to_object[c] = nan_object ? __builtin_nanf("") : to[c];
        st[c] = tw[c];
        st[12 + c] = to[c];
    }
    for (int c = 0; c < 2; c++) {
        d.margin[c] = margin[c];
        st[24 + c] = margin[c];
    }
    if (j.list) j.list[k] = id;
    if (j.moved) j.moved[id] = 1;
}

}  // namespace

void launch_move_instances(const MoveInstancesJob &job, hipStream_t s) {
    if (job.n) hipLaunchKernelGGL(k_move_instances, dim3((job.n + 255u) / 256u), dim3(256), 0, s, job);
}

}  // namespace pupil

extern "C" int pupil_debug_invert3x4(const float m[12], float out[12]) {
    if (!m || !out) return pupil::fail(PUPIL_ERR_INVALID, "null argument");
    pupil::invert_affine3x4(m, out);
    return PUPIL_OK;
}
