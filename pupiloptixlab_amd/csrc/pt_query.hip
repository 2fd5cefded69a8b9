// pt_query.hip — ray queries from device memory (pupil_pt_query_rays / _query_camera): what the
// production traversal found for a ray list, resolved into what a caller can use without the
// engine's private tables -- instance, face within the shape, material, and
// Geometry::GetHitLocalGeometry's position, normal and texcoord (render/geometry.h:272-320).
//
// The traversal is the kModeRays launch as it stands (launch_trace_debug): it writes the compact
// hit (t, b1, b2, global primitive id).  k_query_resolve then runs one ray per lane: 32 B of ray
// and 16 B of hit in (three 16-B loads; a sphere hit reads the ray's first quarter once more
// inside reconstruct(), as its origin record, from the line it just loaded; ids alone read only
// the hit), the arrays asked for out.  The ids are three 4-B stores,
// position and normal one 12-B store each (global_store_dwordx3: the 64 lanes of a wave cover 768
// contiguous bytes, so every 128-B line but the two at the ends of the wave's span is written
// whole by one instruction), the texcoord one 8-B store.  Full output set: 48 B in and 44 B out
// per ray, 60 B out with the 16 B of hit the traversal wrote; the shading record of a hit (one
// 128-B line) and the instance and material tables come through the L2 as in the shade stage.
//
// Which arrays are written is decided per launch: GEO (any of position / normal / texcoord) is a
// template parameter, because without it neither the shading record nor the material is read;
// within an instance each array is a test of a kernel-argument pointer, which the compiler keeps
// in SGPRs (s_cmp_eq_u64 + s_cbranch_scc1 around each store in the gfx950 ISA, no VALU work and
// no divergence; 66 VGPRs with GEO, 12 without, no spills).  A template mask over the six arrays
// would be 64 instances to save those scalar pairs.
//
// Flat scenes: the ray-list traversal reports the global primitive id, and reconstruct() wants the
// record slot its shading record lives in (the flat BVH orders records by leaf).  prim_slot, built
// by k_query_prim_slots from the records themselves, is that map; two-level scenes shade by the
// global id and need none.
#include <hip/hip_runtime.h>

#include "pt_shade.h"

namespace pupil {
namespace {

constexpr int kQueryBlock = 256;

struct f3s {
    float x, y, z;
};

// record slot i of a flat BVH -> prim_slot[global primitive id] = i (holes are skipped; every
// primitive has exactly one record, so no two slots write one entry)
__global__ __launch_bounds__(kQueryBlock) void k_query_prim_slots(const float4 *recs, uint32_t slots,
                                                                  uint32_t num_prims, uint32_t *prim_slot) {
    const uint32_t i = blockIdx.x * kQueryBlock + threadIdx.x;
    if (i >= slots) return;
    const uint32_t ref = __float_as_uint(recs[(size_t)kRecF4 * i].w);
    if (ref == kRecHole) return;
    const uint32_t prim = ref & ~kPrimSphereBit;
    if (prim < num_prims) prim_slot[prim] = i;
}

template <bool GEO>
__global__ __launch_bounds__(kQueryBlock) void k_query_resolve(DeviceScene sc, QueryJob job) {
    const uint32_t l = blockIdx.x * kQueryBlock + threadIdx.x;
    if (l >= job.n) return;
    const float4 h = job.hits[l];
    const uint32_t prim = __float_as_uint(h.w);  // global primitive id, kMissIndex = nothing hit
    int32_t inst = -1, local = -1, material = -1;
    vec3 pos = v3(0.f), nrm = v3(0.f);
    vec2 uv = v2(0.f, 0.f);
    // the hit as the shade stage reads it: flat scenes name the record slot (a slot past the
    // records, which no map built from them holds, resolves as a miss instead of being read)
    uint32_t slot = 0;
    if (GEO && !sc.two_level && prim < sc.num_prims) slot = job.prim_slot[prim];
    if (prim < sc.num_prims && slot < job.slots) {
        if (GEO) {
            const float4 r0 = job.rays[2 * (size_t)l], r1 = job.rays[2 * (size_t)l + 1];
            const vec3 rd = v3(r0.w, r1.x, r1.y);
            float4 hr = h;
            if (!sc.two_level) hr.w = __uint_as_float(slot);
            HitGeo hg = reconstruct(sc, hr, job.rays + 2 * (size_t)l, false, rd, v2(0.f, 0.f));
            const DevInstance &in = sc.instances[hg.inst];
            const DevMaterial &mat = sc.materials[in.material];
            if (mat.twosided && dot(-rd, hg.g.normal) < 0.f) hg.g.normal = -hg.g.normal;  // geometry.h:316-320
            inst = (int32_t)hg.inst;
            local = (int32_t)(prim - in.prim_offset);  // a sphere is its instance's one primitive: 0
            material = (int32_t)in.material;
            pos = hg.g.position;
            nrm = hg.g.normal;
            uv = hg.g.texcoord;
        } else {
            const uint32_t id = inst_of_prim(sc, prim);
            const DevInstance &in = sc.instances[id];
            inst = (int32_t)id;
            local = (int32_t)(prim - in.prim_offset);  // a sphere is its instance's one primitive: 0
            material = (int32_t)in.material;
        }
    }
    const size_t o = job.out_index ? job.out_index[l] : l;
    if (job.hit_out) job.hit_out[o] = h;
    if (job.instance) job.instance[o] = inst;
    if (job.primitive) job.primitive[o] = local;
    if (job.material) job.material[o] = material;
    if (GEO) {
        if (job.position) reinterpret_cast<f3s *>(job.position)[o] = f3s{pos.x, pos.y, pos.z};
        if (job.normal) reinterpret_cast<f3s *>(job.normal)[o] = f3s{nrm.x, nrm.y, nrm.z};
        if (job.texcoord) job.texcoord[o] = make_float2(uv.x, uv.y);
    }
}

}  // namespace

void launch_query_prim_slots(const float4 *recs, uint32_t slots, uint32_t num_prims, uint32_t *prim_slot,
                             hipStream_t s) {
    if (slots == 0) return;
    hipLaunchKernelGGL(k_query_prim_slots, dim3((slots + kQueryBlock - 1) / kQueryBlock), dim3(kQueryBlock), 0, s, recs,
                       slots, num_prims, prim_slot);
}

void launch_query_resolve(const DeviceScene &sc, const QueryJob &job, hipStream_t s) {
    if (job.n == 0) return;
    const dim3 grid((job.n + kQueryBlock - 1) / kQueryBlock);
    if (job.position || job.normal || job.texcoord)
        hipLaunchKernelGGL(k_query_resolve<true>, grid, dim3(kQueryBlock), 0, s, sc, job);
    else
        hipLaunchKernelGGL(k_query_resolve<false>, grid, dim3(kQueryBlock), 0, s, sc, job);
}

}  // namespace pupil
