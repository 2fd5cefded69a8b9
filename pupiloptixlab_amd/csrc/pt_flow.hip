// pt_flow.hip — screen-space flow AOV (pupil_pt_motion_vectors), the guide the reference's
// temporal denoiser takes as OptixDenoiserGuideLayer::flow (framework/optix/denoiser.cpp:203-209).
//
// Three steps on one stream: k_flow_rays writes the camera ray through every local pixel's
// centre into a ray list, the production traversal (launch_trace_debug, kModeRays) finds the
// primary hits, k_flow_project carries every hit point back to where it was under the previous
// instance transforms, projects it through the previous camera and writes
//     flow = (x + 0.5 - u, y + 0.5 - v)     (pixels; (u, v) = the previous continuous pixel position).
// An environment miss is the point at infinity (the direction with w = 0), so a pure camera
// translation leaves the background still.  A point at or behind the previous camera plane has
// no previous pixel: (NaN, NaN), which the denoiser reads as "no history".
//
// Both kernels are one pixel per lane and stream: 32 B of ray record out (two 16-B stores), then
// 48 B in and 8 B out (one float2 store); the instance tables stay in the L2.  While a shape holds
// a vertex snapshot (pupil_pt_snapshot_shape_vertices) the projection also undoes the vertex
// motion: a pixel on such a shape gathers 12 B of indices and 2 x 36 B of vertices, which
// neighbouring pixels share (they hit the same or neighbouring triangles).
#include <hip/hip_runtime.h>

#include "pt_kernels.h"

namespace pupil {
namespace {

constexpr int kFlowBlock = 256;

// The camera ray of camera_path (pt_shade.h) with the film jitter given instead of drawn: the
// same operations in the same order, so the ray is the one a render would trace for a jitter of
// exactly (jx, jy) -- the pixel centre (0.5, 0.5) for the flow pass.
__device__ __forceinline__ vec3 jittered_ray(const Camera &cam, uint32_t width, uint32_t height, uint32_t x, uint32_t y,
                                             float jx, float jy) {
    const vec4 film = v4(((float)x + jx) / (float)width, ((float)y + jy) / (float)height, 0.f, 1.f);
    const float *m = cam.s2c;
    vec4 d = v4(dot(v4(m[0], m[1], m[2], m[3]), film), dot(v4(m[4], m[5], m[6], m[7]), film),
                dot(v4(m[8], m[9], m[10], m[11]), film), dot(v4(m[12], m[13], m[14], m[15]), film));
    const float inv_w = 1.0f / d.w;
    d = v4(d.x * inv_w, d.y * inv_w, d.z * inv_w, d.w * inv_w);
    d.w = 0.f;
    d = normalize(d);
    const float *c = cam.c2w;
    return normalize(v3(dot(v4(c[0], c[1], c[2], c[3]), d), dot(v4(c[4], c[5], c[6], c[7]), d),
                        dot(v4(c[8], c[9], c[10], c[11]), d)));
}

// ray l = (o, d, tmin, tmax) of local pixel l, the 8-float format of the kModeRays traversal;
// tmin / tmax are the render's camera-ray interval
__global__ __launch_bounds__(kFlowBlock) void k_flow_rays(Camera cam, uint32_t width, uint32_t height,
                                                          const uint32_t *pixel_map, uint32_t n, float jx, float jy,
                                                          float4 *rays) {
    const uint32_t l = blockIdx.x * kFlowBlock + threadIdx.x;
    if (l >= n) return;
    const uint32_t pixel = pixel_map ? pixel_map[l] : l;
    const uint32_t y = pixel / width;
    const uint32_t x = pixel - y * width;
    const vec3 d = jittered_ray(cam, width, height, x, y, jx, jy);
    rays[2 * (size_t)l] = make_float4(cam.c2w[3], cam.c2w[7], cam.c2w[11], d.x);
    rays[2 * (size_t)l + 1] = make_float4(d.y, d.z, 0.001f, kMaxDistance);
}

__device__ __forceinline__ vec3 vertex3(const float *v, uint32_t i) {
    return v3(v[3 * (size_t)i], v[3 * (size_t)i + 1], v[3 * (size_t)i + 2]);
}

// Object-space displacement (now minus before) of the point with barycentrics (b1, b2) on face
// f of instance `in`, whose shape's vertices were prevv before the update: the weights are
// reconstruct()'s (pt_shade.h), 1 - b1 - b2 on the face's first vertex.  Exactly 0 where the three
// vertices did not move.  The 3 index loads go out together, then the 18 vertex loads.
__device__ __forceinline__ vec3 vertex_displacement(const DevInstance &in, const float *prevv, uint32_t f, float b1,
                                                    float b2) {
    const uint32_t i0 = in.indices[3 * (size_t)f], i1 = in.indices[3 * (size_t)f + 1], i2 = in.indices[3 * (size_t)f + 2];
    const vec3 c0 = vertex3(in.positions, i0), c1 = vertex3(in.positions, i1), c2 = vertex3(in.positions, i2);
    const vec3 v0 = vertex3(prevv, i0), v1 = vertex3(prevv, i1), v2 = vertex3(prevv, i2);
    const float w = 1.f - b1 - b2;
    return w * (c0 - v0) + b1 * (c1 - v1) + b2 * (c2 - v2);
}

// DEFORM = false is the pass without vertex snapshots: prev_verts is not read.  DEFORM = true
// (prev_verts: per instance the snapshot of its shape or null) runs the same arithmetic on the
// pixels of instances without a snapshot, and takes the object-space displacement d of the hit
// point off it on the others before the previous transform goes on:
//     p' = prev_to_world (to_object p - d),   or   p' = p - L d   (L = the linear part of to_world)
// when no instance moved.  The displacement form, not the re-interpolated previous position: where
// d = 0 (the unmoved part of a mesh that deforms in part) p' is bit for bit the rigid pass's.
template <bool DEFORM>
__device__ __forceinline__ void flow_project(const DeviceScene &sc, const FlowJob &job, const float4 *rays,
                                             const float4 *hits, float2 *flow, const float *const *prev_verts) {
    const uint32_t l = blockIdx.x * kFlowBlock + threadIdx.x;
    if (l >= job.n) return;
    const uint32_t pixel = job.pixel_map ? job.pixel_map[l] : l;
    const uint32_t y = pixel / job.width;
    const uint32_t x = pixel - y * job.width;
    const float4 r0 = rays[2 * (size_t)l], r1 = rays[2 * (size_t)l + 1];
    const float4 h = hits[l];
    const vec3 d = v3(r0.w, r1.x, r1.y);
    const uint32_t prim = __float_as_uint(h.w);  // global primitive id, kMissIndex = environment
    vec4 q = v4(d.x, d.y, d.z, 0.f);
    if (prim != kMissIndex) {
        vec3 p = v3(r0.x, r0.y, r0.z) + h.x * d;
        const float *prevv = nullptr;
        uint32_t inst = 0;
        if (DEFORM) {
            inst = inst_of_prim(sc, prim);
            prevv = prev_verts[inst];
        }
        if (DEFORM && prevv) {  // a deformed mesh: the point the hit was on before the update
            const DevInstance &in = sc.instances[inst];
            const vec3 dv = vertex_displacement(in, prevv, prim - in.prim_offset, h.y, h.z);
            if (job.prev_to_world)
                p = xform_point(job.prev_to_world + 12 * (size_t)inst, xform_point(in.to_object, p) - dv);
            else
                p = p - xform_vector(in.to_world, dv);
        } else if (job.prev_to_world) {  // the same object-space point under the instance's previous transform
            if (!DEFORM) inst = inst_of_prim(sc, prim);
            p = xform_point(job.prev_to_world + 12 * (size_t)inst, xform_point(sc.instances[inst].to_object, p));
        }
        q = v4(p.x, p.y, p.z, 1.f);
    }
    const float *m = job.world_to_sample;
    const float hx = dot(v4(m[0], m[1], m[2], m[3]), q), hy = dot(v4(m[4], m[5], m[6], m[7]), q);
    const float hw = dot(v4(m[12], m[13], m[14], m[15]), q);
    float2 f = make_float2(__builtin_nanf(""), __builtin_nanf(""));
    if (hw > 0.f) {
        const float u = hx / hw * (float)job.width, v = hy / hw * (float)job.height;
        f = make_float2(((float)x + 0.5f) - u, ((float)y + 0.5f) - v);
    }
    flow[job.compact ? l : pixel] = f;
}

__global__ __launch_bounds__(kFlowBlock) void k_flow_project(DeviceScene sc, FlowJob job, const float4 *rays,
                                                             const float4 *hits, float2 *flow) {
    flow_project<false>(sc, job, rays, hits, flow, nullptr);
}

__global__ __launch_bounds__(kFlowBlock) void k_flow_project_deform(DeviceScene sc, FlowJob job, const float4 *rays,
                                                                    const float4 *hits, float2 *flow,
                                                                    const float *const *prev_verts) {
    flow_project<true>(sc, job, rays, hits, flow, prev_verts);
}

}  // namespace

void launch_flow_rays(const DeviceScene &sc, uint32_t width, uint32_t height, const uint32_t *pixel_map, uint32_t n,
                      float jitter_x, float jitter_y, float4 *rays, hipStream_t s) {
    hipLaunchKernelGGL(k_flow_rays, dim3((n + kFlowBlock - 1) / kFlowBlock), dim3(kFlowBlock), 0, s, sc.camera, width,
                       height, pixel_map, n, jitter_x, jitter_y, rays);
}

void launch_flow_project(const DeviceScene &sc, const FlowJob &job, const float4 *rays, const float4 *hits,
                         float2 *flow, hipStream_t s, const float *const *prev_verts) {
    const dim3 grid((job.n + kFlowBlock - 1) / kFlowBlock);
    if (prev_verts)
        hipLaunchKernelGGL(k_flow_project_deform, grid, dim3(kFlowBlock), 0, s, sc, job, rays, hits, flow, prev_verts);
    else
        hipLaunchKernelGGL(k_flow_project, grid, dim3(kFlowBlock), 0, s, sc, job, rays, hits, flow);
}

}  // namespace pupil
