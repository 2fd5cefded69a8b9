// pt_materials.hip — what a material update leaves to the device (pupil_pt_update_materials,
// pupil_pt_update_texture_device).
//
// k_specular_weight: a plastic's specular_sampling_weight depends on the pixel averages of its
// diffuse and specular reflectance (optix_material.cpp:106-116, GetPixelAverage :15-42).  The host
// sums a bitmap's r, g and b in float over the texels in row-major order, and float addition is
// not associative, so after the texels of a slot were replaced on the device the sums are chained
// here in that order: the weight is bit for bit what convert_materials (engine.hip) computes from
// the same texels (-ffp-contract=off on both sides; / is correctly rounded on both).  One block
// of two waves, wave 0 on the diffuse slot and wave 1 on the specular one.  A wave loads 64
// texels per step, one float4 per lane (coalesced, 1 KB), and stages them in the LDS; its lanes
// 0, 1 and 2 then add the step's r, g and b in texel order, three independent chains in one
// instruction stream, while the loads of the next step are already in flight.  A slot without
// texels (rgb, checkerboard) contributes its constant average and its wave only keeps the
// barriers.
//
// k_record_bins: a material whose type changed moves its instances to another material bin; the
// bin word every record slot carries (flat and two-level world records, c.w) follows
// DevInstance::bin.  Nothing else of the acceleration structure depends on a material.
#include <hip/hip_runtime.h>

#include "pt_kernels.h"

namespace pupil {
namespace {

constexpr uint32_t kAvgStep = 64;  // texels per step: one per lane of the wave

__device__ __forceinline__ uint64_t bitmap_texels(const DevTexture &t) {
    return t.type == PUPIL_TEX_BITMAP && t.data && t.width && t.height ? (uint64_t)t.width * t.height : 0ull;
}

__global__ __launch_bounds__(128) void k_specular_weight(DevMaterial *mat) {
    // per wave two stages: step s + 2 overwrites the stage of step s only after the barrier of
    // step s + 1, which every read of step s precedes
    __shared__ float4 stage[2][2][kAvgStep];
    __shared__ float sums[2][3];
    const uint32_t type = mat->type;
    if (type != PUPIL_MAT_PLASTIC && type != PUPIL_MAT_ROUGH_PLASTIC) return;  // the whole block
    const uint32_t first = type == PUPIL_MAT_PLASTIC ? 0u : 1u;  // diffuse slot; specular = first + 1
    const uint32_t wave = threadIdx.x / 64u, lane = threadIdx.x % 64u;
    const DevTexture &t = mat->tex[first + wave];
    const uint64_t n = bitmap_texels(t);
    // both waves run the steps of the longer slot: the barriers stay uniform
    const uint64_t n_max = max(bitmap_texels(mat->tex[first]), bitmap_texels(mat->tex[first + 1u]));
    const uint64_t steps = (n_max + kAvgStep - 1u) / kAvgStep;
    const float4 *data = t.data;
    float sum = 0.f;  // lanes 0..2: the running r, g, b
    float4 next = make_float4(0.f, 0.f, 0.f, 0.f);
    if (lane < n) next = data[lane];
    for (uint64_t step = 0; step < steps; step++) {
        const uint64_t base = step * kAvgStep;
        float4 *st = stage[wave][step & 1u];
        st[lane] = next;
        const uint64_t k = base + kAvgStep + lane;  // the next step's texel, in flight during the adds
        if (k < n) next = data[k];
        __syncthreads();
        if (lane < 3u && base < n) {
            const float *f = reinterpret_cast<const float *>(st) + lane;
            if (n - base >= kAvgStep) {
#pragma unroll
                for (uint32_t j = 0; j < kAvgStep; j++) sum = sum + f[4u * j];
            } else {  // the last step of a size that is no multiple of 64
                const uint32_t len = (uint32_t)(n - base);
                for (uint32_t j = 0; j < len; j++) sum = sum + f[4u * j];
            }
        }
    }
    if (lane < 3u) sums[wave][lane] = sum;
    __syncthreads();
    if (threadIdx.x == 0u) {
        vec3 average[2];
        for (uint32_t s = 0; s < 2u; s++) {
            const DevTexture &ts = mat->tex[first + s];
            average[s] = bitmap_texels(ts) ? bitmap_average(v3(sums[s][0], sums[s][1], sums[s][2]), ts.width, ts.height)
                                           : texture_const_average(ts.type, ts.c0, ts.c1);
        }
        mat->specular_sampling_weight = specular_sampling_weight(average[0], average[1]);
    }
}

__global__ __launch_bounds__(256) void k_record_bins(float4 *recs, uint32_t slots, const DevInstance *instances,
                                                     uint32_t num_instances) {
    const uint32_t r = blockIdx.x * 256u + threadIdx.x;
    if (r >= slots) return;
    float4 *rec = recs + (size_t)kRecF4 * r;
    const uint32_t id = __float_as_uint(rec[1].w);
    if (id >= num_instances) return;  // a hole slot (kRecHole)
    rec[2].w = __uint_as_float(instances[id].bin);
}

}  // namespace

void launch_specular_weight(DevMaterial *mat, hipStream_t s) {
    hipLaunchKernelGGL(k_specular_weight, dim3(1), dim3(128), 0, s, mat);
}

void launch_record_bins(float4 *recs, uint32_t slots, const DevInstance *instances, uint32_t num_instances,
                        hipStream_t s) {
    if (!recs || slots == 0u) return;
    hipLaunchKernelGGL(k_record_bins, dim3((slots + 255u) / 256u), dim3(256), 0, s, recs, slots, instances, num_instances);
}

}  // namespace pupil
