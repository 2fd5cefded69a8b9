// pt_radiance.hip — the generate stage of path-traced radiance along a caller's rays
// (pupil_pt_radiance_rays): sample s of ray i is one path of __raygen__main (main.cu:36-194) whose
// first ray is ray i instead of the camera's.  Everything after the generate is the wavefront
// pipeline as it stands (engine.hip radiance_chunk): the queue form of the primary extend, which
// takes each path's origin from PathState::ray_o, then partition, mixed traversal and shade per
// bounce with fresh = false, then k_accumulate into the caller's arrays.
//
// k_generate_rays writes the full record of k_generate (full = 1) -- origin, direction,
// throughput 1, radiance 0, RNG -- one path per lane, sample-major within the chunk (path
// p = sample * num_local + ray, the layout k_accumulate reads): 32 B of ray in (two 16-B loads;
// the 64 lanes of a wave cover 2 KB of contiguous rays, each load instruction every second
// quarter line, both from the same lines) and five 16-B non-temporal record stores out.  The RNG
// is rng_init(id, seed + sample) followed by the two film-jitter draws a camera path makes
// (main.cu:53-55), so a ray that is the camera ray of pixel `id` continues that pixel's stream.
// Neither the ray index nor the id is chunk-local: the results do not depend on the chunk size.
// The direction is used as given (unit length is the caller's contract); floats 6 and 7 of a ray
// are not read: every segment of a path uses the path tracer's window [0.001, kMaxDistance].
#include <hip/hip_runtime.h>

#include "pt_shade.h"

namespace pupil {
namespace {

constexpr int kRadianceBlock = 256;

__global__ __launch_bounds__(kRadianceBlock) void k_generate_rays(RayGenJob job, PathState ps) {
    const uint32_t p = blockIdx.x * kRadianceBlock + threadIdx.x;
    if (p >= job.num_paths) return;
    const uint32_t s = p / job.num_local;
    const uint32_t l = p - s * job.num_local;
    const size_t i = (size_t)job.ray_base + l;  // the ray's index in the caller's list
    const float4 r0 = job.rays[2 * i], r1 = job.rays[2 * i + 1];
    const uint32_t id = job.stream_ids ? job.stream_ids[i] : (uint32_t)i;
    uint32_t rng = rng_init(id, job.seed0 + s);  // main.cu:53
    (void)rng_next(rng);                         // main.cu:55: the film jitter of a camera path
    (void)rng_next(rng);
    st_ps(ps.ray_o + p, make_float4(r0.x, r0.y, r0.z, 0.f));
    st_ps(ps.ray_d + p, make_float4(r0.w, r1.x, r1.y, 0.f));
    st_ps(ps.thr + p, make_float4(1.f, 1.f, 1.f, 0.f));
    st_ps(ps.rad + p, make_float4(0.f, 0.f, 0.f, 0.f));
    st_ps(ps.misc + p, make_uint4(rng, 0u, 0u, 0u));
}

__global__ __launch_bounds__(kRadianceBlock) void k_identity_ids(uint32_t *ids, uint32_t n) {
    const uint32_t i = blockIdx.x * kRadianceBlock + threadIdx.x;
    if (i < n) ids[i] = i;
}

}  // namespace

void launch_generate_rays(const RayGenJob &job, const PathState &ps, hipStream_t s) {
    if (job.num_paths == 0) return;
    hipLaunchKernelGGL(k_generate_rays, dim3((job.num_paths + kRadianceBlock - 1) / kRadianceBlock),
                       dim3(kRadianceBlock), 0, s, job, ps);
}

void launch_identity_ids(uint32_t *ids, uint32_t n, hipStream_t s) {
    if (n == 0) return;
    hipLaunchKernelGGL(k_identity_ids, dim3((n + kRadianceBlock - 1) / kRadianceBlock), dim3(kRadianceBlock), 0, s, ids,
                       n);
}

}  // namespace pupil
