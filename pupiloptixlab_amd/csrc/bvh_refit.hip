// bvh_refit.hip — updates of a built BVH4 without a rebuild: moved / hidden instances
// (refit_bvh4: records rewritten, boxes refitted bottom up over the collapse's level order) and
// deformed meshes (launch_refit_levels, launch_refresh_attrs*).
#include "bvh_build_detail.h"

#include <algorithm>

namespace pupil {

using bvh::kBlock;

// ------------------------------------------------------------------ refit (RenderInstanceUpdate)
namespace {

// Records of the moved instance (b.w = instance) get its new world vertices, written
// exactly as k_prim_setup writes them (global id in a.w: sphere bit + id).
__global__ void k_refit_records(BvhBuildInput in, uint32_t n, float4 *recs_base, const uint8_t *moved) {
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    float4 *recs = recs_base + (size_t)kRecF4 * r;
    const uint32_t id = __float_as_uint(recs[1].w);
    if (id == kRecHole || !moved[id]) return;  // a hole slot, or an unmoved instance
    const uint32_t gid = __float_as_uint(recs[0].w) & ~kPrimSphereBit;
    const DevInstance &inst = in.instances[id];
    if (inst.hidden) {
        // visibilityMask 0 (ias_manager.cpp:174,192): vertices no ray hits (intersect_triangle's
        // range test fails on NaN; a sphere is rejected through the NaN to_object of its instance's
        // device copy, pt_scene.h device_instance: its record only has to stay out of the boxes)
        // and that k_refit_level's fminf / fmaxf leave out of every box.  The id words stay:
        // showing the instance again flags it moved and the branches below restore the record.
        const float q = __builtin_nanf("");
        recs[0] = make_float4(q, q, q, recs[0].w);
        recs[1] = make_float4(q, q, q, recs[1].w);
        if (inst.kind != PUPIL_SHAPE_SPHERE) recs[2] = make_float4(q, q, q, recs[2].w);
        return;
    }
    if (inst.kind == PUPIL_SHAPE_SPHERE) {
        const float *m = inst.to_world;
        const vec3 c = v3(m[3], m[7], m[11]);
        const float ex = sqrtf(m[0] * m[0] + m[1] * m[1] + m[2] * m[2]) * 1.001f;
        const float ey = sqrtf(m[4] * m[4] + m[5] * m[5] + m[6] * m[6]) * 1.001f;
        const float ez = sqrtf(m[8] * m[8] + m[9] * m[9] + m[10] * m[10]) * 1.001f;
        recs[0] = make_float4(c.x, c.y, c.z, recs[0].w);
        recs[1] = make_float4(ex, ey, ez, recs[1].w);
        return;
    }
    const uint32_t local = gid - inst.prim_offset;
    const uint32_t i0 = inst.indices[3 * local], i1 = inst.indices[3 * local + 1], i2 = inst.indices[3 * local + 2];
    const float *P = inst.positions;
    const vec3 w0 = xform_point(inst.to_world, v3(P[3 * i0], P[3 * i0 + 1], P[3 * i0 + 2]));
    const vec3 w1 = xform_point(inst.to_world, v3(P[3 * i1], P[3 * i1 + 1], P[3 * i1 + 2]));
    const vec3 w2 = xform_point(inst.to_world, v3(P[3 * i2], P[3 * i2 + 1], P[3 * i2 + 2]));
    recs[0] = make_float4(w0.x, w0.y, w0.z, recs[0].w);
    recs[1] = make_float4(w1.x, w1.y, w1.z, recs[1].w);
    recs[2] = make_float4(w2.x, w2.y, w2.z, recs[2].w);
}

// One BVH4 level, bottom up: child boxes from the records under a leaf (exact; a
// sphere's padded box) or from the child's box of the previous launch; re-quantised.
__global__ void k_refit_level(Bvh4Node *nodes, uint32_t lo, uint32_t hi, const float4 *recs, float *nbox) {
    for (uint32_t j = lo + blockIdx.x * blockDim.x + threadIdx.x; j < hi; j += gridDim.x * blockDim.x) {
        const Bvh4Node n = nodes[j];
        float clo[3][4], chi[3][4];
        float nlo[3] = {__builtin_huge_valf(), __builtin_huge_valf(), __builtin_huge_valf()};
        float nhi[3] = {-__builtin_huge_valf(), -__builtin_huge_valf(), -__builtin_huge_valf()};
        int link[4];
        int nk = 0;
        for (int k = 0; k < 4; k++) {
            const int l = n.child[k];
            if (l == kEmptyLink) continue;
            float bl[3] = {__builtin_huge_valf(), __builtin_huge_valf(), __builtin_huge_valf()};
            float bh[3] = {-__builtin_huge_valf(), -__builtin_huge_valf(), -__builtin_huge_valf()};
            if (l >= 0) {
                for (int a = 0; a < 3; a++) {
                    bl[a] = nbox[6 * (size_t)l + a];
                    bh[a] = nbox[6 * (size_t)l + 3 + a];
                }
            } else {
                for (uint32_t r = leaf_first(l); r < leaf_first(l) + leaf_count(l); r++) {
                    const float4 a = recs[kRecF4 * r], b = recs[kRecF4 * r + 1], c = recs[kRecF4 * r + 2];
                    if (__float_as_uint(a.w) & kPrimSphereBit) {
                        bl[0] = fminf(bl[0], a.x - b.x);
                        bl[1] = fminf(bl[1], a.y - b.y);
                        bl[2] = fminf(bl[2], a.z - b.z);
                        bh[0] = fmaxf(bh[0], a.x + b.x);
                        bh[1] = fmaxf(bh[1], a.y + b.y);
                        bh[2] = fmaxf(bh[2], a.z + b.z);
                    } else {
                        bl[0] = fminf(bl[0], fminf(fminf(a.x, b.x), c.x));
                        bl[1] = fminf(bl[1], fminf(fminf(a.y, b.y), c.y));
                        bl[2] = fminf(bl[2], fminf(fminf(a.z, b.z), c.z));
                        bh[0] = fmaxf(bh[0], fmaxf(fmaxf(a.x, b.x), c.x));
                        bh[1] = fmaxf(bh[1], fmaxf(fmaxf(a.y, b.y), c.y));
                        bh[2] = fmaxf(bh[2], fmaxf(fmaxf(a.z, b.z), c.z));
                    }
                }
            }
            for (int a = 0; a < 3; a++) {
                clo[a][nk] = bl[a];
                chi[a][nk] = bh[a];
                nlo[a] = fminf(nlo[a], bl[a]);
                nhi[a] = fmaxf(nhi[a], bh[a]);
            }
            link[nk++] = l;
        }
        nodes[j] = encode_bvh4(nlo, nhi, clo, chi, link, nk);
        for (int a = 0; a < 3; a++) {
            nbox[6 * (size_t)j + a] = nlo[a];
            nbox[6 * (size_t)j + 3 + a] = nhi[a];
        }
    }
}

// The object-space part of a shading record (k_attrs: p0 p1 p2, n0 n1 n2) from the shape's
// vertex arrays as they are now; the id words r[0].w / r[1].w and the texcoords stay.
__device__ __forceinline__ void write_attr_geometry(float4 *r, const float *P, const float *N, const uint32_t *idx,
                                                    uint32_t local) {
    const uint32_t i0 = idx[3 * local], i1 = idx[3 * local + 1], i2 = idx[3 * local + 2];
    float nn[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (N) {
        const uint32_t id[3] = {i0, i1, i2};
        for (int v = 0; v < 3; v++)
            for (int c = 0; c < 3; c++) nn[3 * v + c] = N[3 * id[v] + c];
    }
    r[0] = make_float4(P[3 * i0], P[3 * i0 + 1], P[3 * i0 + 2], r[0].w);
    r[1] = make_float4(P[3 * i1], P[3 * i1 + 1], P[3 * i1 + 2], r[1].w);
    r[2] = make_float4(P[3 * i2], P[3 * i2 + 1], P[3 * i2 + 2], nn[0]);
    r[3] = make_float4(nn[1], nn[2], nn[3], nn[4]);
    r[4] = make_float4(nn[5], nn[6], nn[7], nn[8]);
}

// Deformed meshes, flattened BVH: the shading record of every record slot whose instance is
// flagged in `moved` is rewritten from the instance's vertex arrays, exactly as k_attrs wrote
// it.  The slot's primitive and instance are read from the traversal record beside it (the
// same words as the shading record's r[0].w / r[1].w; a hole slot has no shading record).
__global__ void k_refresh_attrs(BvhBuildInput in, uint32_t n, const float4 *recs_base, float4 *attrs,
                                const uint8_t *moved) {
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    const float4 *recs = recs_base + (size_t)kRecF4 * r;
    const uint32_t id = __float_as_uint(recs[1].w);
    if (id == kRecHole || !moved[id]) return;
    const uint32_t w0 = __float_as_uint(recs[0].w);
    if (w0 & kPrimSphereBit) return;
    const DevInstance &inst = in.instances[id];
    write_attr_geometry(attrs + (size_t)kAttrStride * r, inst.positions, inst.normals, inst.indices,
                        w0 - inst.prim_offset);
}

// ... a two-level BLAS: the n shading records of one shape, in the mesh's own primitive order
__global__ void k_refresh_attrs_shape(uint32_t n, float4 *attrs, const float *P, const float *N,
                                      const uint32_t *idx) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    float4 *r = attrs + (size_t)kAttrStride * p;
    write_attr_geometry(r, P, N, idx, __float_as_uint(r[0].w));
}

}  // namespace

void launch_refit_levels(Bvh4Node *nodes, const std::vector<uint32_t> &level_start, uint32_t node_base,
                         const float4 *recs, float *nbox, hipStream_t s) {
    for (size_t L = level_start.size() < 2 ? 0 : level_start.size() - 1; L-- > 0;) {
        const uint32_t lo = node_base + level_start[L], hi = node_base + level_start[L + 1];
        if (hi <= lo) continue;
        const uint32_t g = std::max(1u, std::min(4096u, (hi - lo + kBlock - 1) / kBlock));
        hipLaunchKernelGGL(k_refit_level, dim3(g), dim3(kBlock), 0, s, nodes, lo, hi, recs, nbox);
    }
}

void launch_refresh_attrs(const BvhBuildInput &in, const BvhBuildOutput &out, const uint8_t *moved, hipStream_t s) {
    const uint32_t n = out.num_records;
    if (n && out.attrs)
        hipLaunchKernelGGL(k_refresh_attrs, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, s, in, n, out.prims,
                           out.attrs, moved);
}

void launch_refresh_attrs_shape(float4 *attrs, uint32_t n, const float *positions, const float *normals,
                                const uint32_t *indices, hipStream_t s) {
    if (n)
        hipLaunchKernelGGL(k_refresh_attrs_shape, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, s, n, attrs,
                           positions, normals, indices);
}

int refit_bvh4(const BvhBuildInput &in, BvhBuildOutput &out, const uint8_t *moved, float *nbox, hipStream_t s,
               double *ms, bool records_only) {
    const bool levels = out.level_start.size() >= 2 && out.nodes4 && out.num_nodes4 != 0;
    if (!levels && !(records_only && out.num_nodes4 == 0 && out.prims)) return -1;
    hipEvent_t e0, e1;
    (void)hipEventCreate(&e0);
    (void)hipEventCreate(&e1);
    (void)hipEventRecord(e0, s);
    hipError_t err = hipSuccess;
    {
        const uint32_t n = out.num_records;  // record slots (holes are skipped)
        if (n) hipLaunchKernelGGL(k_refit_records, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, s, in, n, out.prims, moved);
        for (size_t L = levels ? out.level_start.size() - 1 : 0; L-- > 0;) {
            const uint32_t lo = out.level_start[L], hi = out.level_start[L + 1];
            const uint32_t g = std::max(1u, std::min(4096u, (hi - lo + kBlock - 1) / kBlock));
            hipLaunchKernelGGL(k_refit_level, dim3(g), dim3(kBlock), 0, s, out.nodes4, lo, hi, out.prims, nbox);
        }
        err = hipGetLastError();
    }
    (void)hipEventRecord(e1, s);
    if (!err) err = hipEventSynchronize(e1);
    float t = 0.f;
    (void)hipEventElapsedTime(&t, e0, e1);
    if (ms) *ms = t;
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    return err == hipSuccess ? 0 : -2;
}

}  // namespace pupil
