// pt_emitters.hip — the area-emitter table rebuilt on the device (pupil_pt_enable_device_emitters).
//
// The host derives the table in world.cpp (AddAreaEmitter, ComputeProbability) and host/emitter_tables.h
// (emitter_tables).  The five stages here restate those operations in the host's order, so the
// table is bit for bit the host's for the same vertices and transforms (the build has
// -ffp-contract=off on both sides; / and sqrtf are correctly rounded on both):
//   1. k_emit_geometry  per emitter: world vertices, normals, area (or centre, radius, area of a
//                       sphere) into its DevEmitter, weight = select_weight * area into scratch
//   2. k_emit_chain     the weight sum: ComputeProbability adds the weights in emitter order in
//                       float, and float addition is not associative, so ONE lane chains the adds
//   3. k_emit_select    select_probability = weight / sum * count, then / emitter_num
//   4. k_emit_chain     cdf[e] = cdf[e - 1] + select_probability[e]: the same chain
//   5. k_emit_guide     guide[k] = first i with cdf[i] >= k / m: a lower-bound binary search per
//                       k, equal to the host's linear walk on a non-decreasing CDF
// Stages 2 and 4 are one wave: its 64 lanes stage kChainChunk values in the LDS with coalesced
// loads (and, for the CDF, store the chunk's results the same way), lane 0 reads them back four
// per LDS load and adds.  Nothing else of a DevEmitter is written (type, radiance, tex, the env).
// The delta lights (point, spot, directional) follow the area emitters in the table and have no
// geometry to rebuild: stages 1 and 2 run over the area emitters alone (`count` in stage 3 is the
// true area count), stage 3 rewrites a delta light's select_probability = 1 / emitter_num and
// stages 4 and 5 span the whole table, as the host's CDF does.
//
// A table of a new size (an emissive mesh replaced, emissive instances added or removed) has no
// records yet: k_emit_fill runs in front of the five stages and writes, per triangle or sphere
// emitter, the whole DevEmitter that EmitterTables::convert_emitter writes from the world's
// AddAreaEmitter record -- zero but for type, the instance's radiance and a triangle's texcoords
// -- and emit_inst[e], the emitter's instance: a search over the emissive instances' offsets, so
// no per-face array comes from the host.
#include <hip/hip_runtime.h>

#include "pt_kernels.h"

namespace pupil {
namespace {

constexpr int kEmitBlock = 256;
constexpr uint32_t kChainChunk = 1024;  // values per LDS stage: 16 coalesced loads per lane

// TransformPoint (transform.cpp:123-130; world.cpp) by the 3x4 the engine holds: the 4x4's last
// row is 0 0 0 1, so w is exactly 1 for finite p -- computed and divided by all the same, which
// keeps the host's result for non-finite coordinates too
__device__ __forceinline__ vec3 emit_point(const float *m, float px, float py, float pz) {
    const float x = m[0] * px + m[1] * py + m[2] * pz + m[3];
    const float y = m[4] * px + m[5] * py + m[6] * pz + m[7];
    const float z = m[8] * px + m[9] * py + m[10] * pz + m[11];
    const float w = 0.f * px + 0.f * py + 0.f * pz + 1.f;
    return v3(x / w, y / w, z / w);
}

// TransformNormal (transform.cpp:138-146) by Inverse().Transpose(): row r of the transposed 3x3 is
// column r of to_object
__device__ __forceinline__ vec3 emit_normal(const float *o, float nx, float ny, float nz) {
    const float x = o[0] * nx + o[4] * ny + o[8] * nz;
    const float y = o[1] * nx + o[5] * ny + o[9] * nz;
    const float z = o[2] * nx + o[6] * ny + o[10] * nz;
    const float len = sqrtf(x * x + y * y + z * z);
    return v3(x / len, y / len, z / len);
}

// stage 1: EmitterHelper::SetMeshAreaEmitter / SetSphereAreaEmitter (world.cpp AddAreaEmitter)
__global__ __launch_bounds__(kEmitBlock) void k_emit_geometry(EmitterJob job) {
    const uint32_t e = blockIdx.x * kEmitBlock + threadIdx.x;
    if (e >= job.count) return;
    const uint32_t inst = job.emit_inst[e];
    const DevInstance &in = job.instances[inst];
    const float select_weight = job.inst_weight[inst];
    DevEmitter &d = job.areas[e];
    float area;
    if (in.kind == PUPIL_SHAPE_SPHERE) {
        const vec3 o = emit_point(in.to_world, 0.f, 0.f, 0.f);
        const vec3 p = emit_point(in.to_world, 0.f + 1.f, 0.f, 0.f);
        const float dx = o.x - p.x, dy = o.y - p.y, dz = o.z - p.z;
        const float radius = sqrtf(dx * dx + dy * dy + dz * dz);
        area = 4.f * 3.14159265358979323846f * radius * radius;
        d.center = o;
        d.radius = radius;
    } else {
        const uint32_t f = e - (uint32_t)in.emitter_offset;
        vec3 p[3];
        for (int v = 0; v < 3; v++) {
            const uint32_t idx = in.indices[3 * (size_t)f + v];
            p[v] = emit_point(in.to_world, in.positions[3 * (size_t)idx], in.positions[3 * (size_t)idx + 1],
                              in.positions[3 * (size_t)idx + 2]);
            float nx = 0.f, ny = 0.f, nz = 1.f;
            if (in.normals) {
                nx = in.normals[3 * (size_t)idx];
                ny = in.normals[3 * (size_t)idx + 1];
                nz = in.normals[3 * (size_t)idx + 2];
            }
            d.pos[v] = p[v];
            d.nrm[v] = emit_normal(in.to_object, nx, ny, nz);
        }
        const float v1x = p[1].x - p[0].x, v1y = p[1].y - p[0].y, v1z = p[1].z - p[0].z;
        const float v2x = p[2].x - p[0].x, v2y = p[2].y - p[0].y, v2z = p[2].z - p[0].z;
        const float cx = v1y * v2z - v1z * v2y, cy = v1z * v2x - v1x * v2z, cz = v1x * v2y - v1y * v2x;
        area = sqrtf(cx * cx + cy * cy + cz * cz) * 0.5f;
    }
    d.area = area;
    job.weight[e] = select_weight * area;
}

// In front of stage 1 for a table of a new size.  sources[k].offset increases with k from 0, so the
// emitter's instance is the last source whose offset is <= e.
__global__ __launch_bounds__(kEmitBlock) void k_emit_fill(EmitterFillJob job) {
    const uint32_t e = blockIdx.x * kEmitBlock + threadIdx.x;
    if (e >= job.count) return;
    uint32_t lo = 0, hi = job.num_sources;  // the first source whose offset is > e, in [1, num_sources]
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (job.sources[mid].offset <= e) lo = mid + 1u;
        else hi = mid;
    }
    const DevEmitSource &src = job.sources[lo - 1u];
    const DevInstance &in = job.instances[src.inst];
    DevEmitter d;
    __builtin_memset(&d, 0, sizeof(d));
    d.radiance = src.radiance;
    if (in.kind == PUPIL_SHAPE_SPHERE) {
        d.type = PUPIL_EMITTER_SPHERE;
    } else {
        d.type = PUPIL_EMITTER_TRI_AREA;
        if (in.texcoords) {  // AddAreaEmitter: the shape's own, no flip
            const uint32_t f = e - src.offset;
            for (int v = 0; v < 3; v++) {
                const uint32_t idx = in.indices[3 * (size_t)f + v];
                d.tex[v] = v2(in.texcoords[2 * (size_t)idx], in.texcoords[2 * (size_t)idx + 1]);
            }
        }
    }
    job.areas[e] = d;
    job.emit_inst[e] = src.inst;
}

// stages 2 and 4: out = the running sum of in[0..n) in index order, starting from 0.f.  SCAN:
// every partial sum goes to out[0..n) (the CDF); else only the total, to out[0].  One wave.
template <bool SCAN>
__global__ __launch_bounds__(64) void k_emit_chain(const float *in, uint32_t n, float *out) {
    __shared__ float4 stage[kChainChunk / 4];
    float *stage_f = reinterpret_cast<float *>(stage);
    const uint32_t lane = threadIdx.x;
    float sum = 0.f;  // lane 0's
    for (uint32_t base = 0; base < n; base += kChainChunk) {
        const uint32_t len = min(kChainChunk, n - base);
        for (uint32_t k = lane; k < len; k += 64u) stage_f[k] = in[base + k];
        __syncthreads();
        if (lane == 0) {
            uint32_t k = 0;
            for (; k + 4 <= len; k += 4) {
                float4 v = stage[k / 4];
                sum = sum + v.x, v.x = sum;
                sum = sum + v.y, v.y = sum;
                sum = sum + v.z, v.z = sum;
                sum = sum + v.w, v.w = sum;
                if (SCAN) stage[k / 4] = v;
            }
            for (; k < len; k++) {
                sum = sum + stage_f[k];
                if (SCAN) stage_f[k] = sum;
            }
        }
        __syncthreads();
        if (SCAN)
            for (uint32_t k = lane; k < len; k += 64u) out[base + k] = stage_f[k];
        __syncthreads();  // the next chunk overwrites the stage
    }
    if (!SCAN && lane == 0) out[0] = sum;
}

// stage 3: ComputeProbability's two roundings (count and emitter_num converted as the host's
// size_t values are)
__global__ __launch_bounds__(kEmitBlock) void k_emit_select(EmitterJob job) {
    const uint32_t e = blockIdx.x * kEmitBlock + threadIdx.x;
    if (e >= job.total) return;
    float p;
    if (e < job.count) {
        p = job.weight[e] / job.sum[0] * (float)job.count;
        p = p / (float)job.emitter_num;
    } else {
        p = 1.f / (float)job.emitter_num;  // a delta light: weight 1 (emitter.cpp:334-335)
    }
    job.areas[e].select_probability = p;
    job.select[e] = p;
}

// stage 5: emitter_tables' guide, k = 0..m (m = 2^guide_bits)
__global__ __launch_bounds__(kEmitBlock) void k_emit_guide(EmitterJob job) {
    const uint32_t k = blockIdx.x * kEmitBlock + threadIdx.x;
    const uint32_t m = 1u << job.guide_bits;
    if (k > m) return;
    const float t = (float)k / (float)m;
    uint32_t lo = 0, hi = job.total;  // first i in [0, total] with cdf[i] >= t (total = none)
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (job.cdf[mid] < t) lo = mid + 1u;
        else hi = mid;
    }
    job.guide[k] = lo;
}

// The terminal-ray cull set's scan (engine.hip derive_cull_set): the record slots whose instance
// carries emitters.  A hole slot names no instance (kRecHole); a hidden instance's slots are
// listed too -- their NaN vertices fail the cull's test exactly as they fail the traversal's.
__global__ __launch_bounds__(kEmitBlock) void k_cull_scan(const float4 *recs, uint32_t slots,
                                                          const DevInstance *instances, uint32_t num_instances,
                                                          uint32_t *out, uint32_t cap) {
    const uint32_t r = blockIdx.x * kEmitBlock + threadIdx.x;
    if (r >= slots) return;
    const uint32_t id = __float_as_uint(recs[(size_t)kRecF4 * r + 1].w);
    if (id >= num_instances || instances[id].emitter_offset < 0) return;
    const uint32_t k = atomicAdd(out, 1u);
    if (k < cap) out[1u + k] = r;
}

}  // namespace

uint32_t launch_emitter_rebuild(const EmitterJob &job, hipStream_t s) {
    if (job.total == 0) return 0u;
    uint32_t launches = 2u;
    const dim3 grid_all((job.total + kEmitBlock - 1) / kEmitBlock);
    if (job.count) {  // none: delta lights alone, whose select probability needs no weight
        const dim3 grid((job.count + kEmitBlock - 1) / kEmitBlock);
        hipLaunchKernelGGL(k_emit_geometry, grid, dim3(kEmitBlock), 0, s, job);
        hipLaunchKernelGGL(k_emit_chain<false>, dim3(1), dim3(64), 0, s, (const float *)job.weight, job.count, job.sum);
        launches += 2u;
    }
    hipLaunchKernelGGL(k_emit_select, grid_all, dim3(kEmitBlock), 0, s, job);
    hipLaunchKernelGGL(k_emit_chain<true>, dim3(1), dim3(64), 0, s, (const float *)job.select, job.total, job.cdf);
    if (job.guide) {
        const uint32_t entries = (1u << job.guide_bits) + 1u;
        hipLaunchKernelGGL(k_emit_guide, dim3((entries + kEmitBlock - 1) / kEmitBlock), dim3(kEmitBlock), 0, s, job);
        launches++;
    }
    return launches;
}

void launch_emitter_fill(const EmitterFillJob &job, hipStream_t s) {
    if (job.count == 0 || job.num_sources == 0) return;
    hipLaunchKernelGGL(k_emit_fill, dim3((job.count + kEmitBlock - 1) / kEmitBlock), dim3(kEmitBlock), 0, s, job);
}

void launch_cull_scan(const float4 *recs, uint32_t slots, const DevInstance *instances, uint32_t num_instances,
                      uint32_t *out, uint32_t cap, hipStream_t s) {
    if (!recs || slots == 0u) return;
    hipLaunchKernelGGL(k_cull_scan, dim3((slots + kEmitBlock - 1) / kEmitBlock), dim3(kEmitBlock), 0, s, recs, slots,
                       instances, num_instances, out, cap);
}

}  // namespace pupil
