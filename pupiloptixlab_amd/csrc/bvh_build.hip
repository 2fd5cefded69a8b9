// bvh_build.hip — GPU BVH builder (replaces optixAccelBuild for the GAS/IAS,
// framework/world/gas_manager.cpp:130-173, ias_manager.cpp:54-96): the drivers.
//
// Pipeline (all on device, one stream; the default path first, the knob that selects another
// after it; every knob is read once per build, by read_build_options below):
//   0. k_prim_setup    object-space meshes -> world-space primitive records + AABBs (instances
//                      flattened; spheres keep their instance).  build_bvh4_over_boxes starts
//                      from uploaded boxes instead.
//   1. Morton order    bvh_sort.hip: centroid bounds, 30-bit Morton codes, stable LSD radix sort
//   2. binary tree     bvh_ploc.hip: PLOC (nearest-neighbour clustering over the Morton order),
//                      then PUPIL_BVH_REINSERT (default 2) rounds of parallel reinsertion over
//                      its tree (bvh_reinsert.hip; PUPIL_BVH_REINSERT_LOG=1 prints what they
//                      did).  PUPIL_BVH_BUILDER=lbvh: the Karras 2012 hierarchy with a bottom-up
//                      refit, which build_bvh_bounded also falls back to when the PLOC tree is
//                      too deep for the traversal stacks.
//   3. collapse        bvh_collapse.hip: 4-wide quantized nodes, breadth first, by the
//                      SAH-optimal slot distribution; subtrees of <= leaf_size (PUPIL_LEAF_SIZE,
//                      read by the engine) primitives become one leaf, up to PUPIL_SAH_LEAF
//                      where the SAH prefers it.  PUPIL_BVH4_COLLAPSE=greedy: greedy
//                      surface-area opening; =parity: binary nodes at even depth (no level
//                      order, so no refit).
//   4. leaf slots      each leaf's records on a 128-B line: k_leaf_marks, scan, k_leaf_slots
//      and records     k_reorder (primitive records into their slots) and k_attrs (shading
//                      records in the same order).  build_lbvh only.
// Updates of a built tree (refit, deformed meshes) are in bvh_refit.hip.
#include "bvh_build_detail.h"

#include <algorithm>
#include <cstdlib>
#include <cstring>

namespace pupil {

using namespace bvh;

namespace {

__global__ void k_prim_setup(BvhBuildInput in, float4 *recs, Aabb *boxes) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= in.num_prims) return;
    const uint32_t inst_id = in.prim_inst[i];
    const DevInstance &inst = in.instances[inst_id];
    const uint32_t mtype = in.materials[inst.material].type;
    const uint32_t bin = (mtype >= 1u && mtype <= 7u) ? mtype : 8u;
    Aabb b;
    if (inst.kind == PUPIL_SHAPE_SPHERE) {
        const float *m = inst.to_world;
        const vec3 c = v3(m[3], m[7], m[11]);
        // exact extents of an affinely transformed unit sphere, padded
        const float ex = sqrtf(m[0] * m[0] + m[1] * m[1] + m[2] * m[2]) * 1.001f;
        const float ey = sqrtf(m[4] * m[4] + m[5] * m[5] + m[6] * m[6]) * 1.001f;
        const float ez = sqrtf(m[8] * m[8] + m[9] * m[9] + m[10] * m[10]) * 1.001f;
        b.lo[0] = c.x - ex; b.lo[1] = c.y - ey; b.lo[2] = c.z - ez;
        b.hi[0] = c.x + ex; b.hi[1] = c.y + ey; b.hi[2] = c.z + ez;
        recs[3 * i + 0] = make_float4(c.x, c.y, c.z, __uint_as_float(i | kPrimSphereBit));
        recs[3 * i + 1] = make_float4(ex, ey, ez, __uint_as_float(inst_id));
        recs[3 * i + 2] = make_float4(0.f, 0.f, 0.f, __uint_as_float(bin));
    } else {
        const uint32_t local = i - inst.prim_offset;
        const uint32_t i0 = inst.indices[3 * local], i1 = inst.indices[3 * local + 1], i2 = inst.indices[3 * local + 2];
        const float *P = inst.positions;
        // world-space vertices: the CPU oracle applies the same row-major 3x4 product
        // (object_space: a BLAS keeps the input vertices untouched)
        vec3 w0 = v3(P[3 * i0], P[3 * i0 + 1], P[3 * i0 + 2]);
        vec3 w1 = v3(P[3 * i1], P[3 * i1 + 1], P[3 * i1 + 2]);
        vec3 w2 = v3(P[3 * i2], P[3 * i2 + 1], P[3 * i2 + 2]);
        if (!in.object_space) {
            w0 = xform_point(inst.to_world, w0);
            w1 = xform_point(inst.to_world, w1);
            w2 = xform_point(inst.to_world, w2);
        }
        b.lo[0] = fminf(fminf(w0.x, w1.x), w2.x);
        b.lo[1] = fminf(fminf(w0.y, w1.y), w2.y);
        b.lo[2] = fminf(fminf(w0.z, w1.z), w2.z);
        b.hi[0] = fmaxf(fmaxf(w0.x, w1.x), w2.x);
        b.hi[1] = fmaxf(fmaxf(w0.y, w1.y), w2.y);
        b.hi[2] = fmaxf(fmaxf(w0.z, w1.z), w2.z);
        recs[3 * i + 0] = make_float4(w0.x, w0.y, w0.z, __uint_as_float(i));
        recs[3 * i + 1] = make_float4(w1.x, w1.y, w1.z, __uint_as_float(inst_id));
        recs[3 * i + 2] = make_float4(w2.x, w2.y, w2.z, __uint_as_float(bin));
    }
    boxes[i] = b;
}

// Shading record of each primitive in traversal (Morton) order, kAttrStride
// float4 per primitive: everything the hit reconstruction of
// Geometry::GetHitLocalGeometry (render/geometry.h:48-96) gathers from the
// object-space mesh, in one 128-B line instead of index + 3 x position / normal /
// uv gathers:  [0] p0 | global id (+ sphere bit)  [1] p1 | instance  [2] p2 | n0.x
// [3] n0.yz n1.xy  [4] n1.z n2.xyz  [5] t0 t1  [6] t2 | 0 0  [7] unused
__global__ void k_attrs(int n, const uint32_t *sorted_vals, const uint32_t *slot, BvhBuildInput in, float4 *attrs) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t prim = sorted_vals[i];
    const uint32_t inst_id = in.prim_inst[prim];
    const DevInstance &inst = in.instances[inst_id];
    // object_space (BLAS): records in the mesh's own primitive order, found by primitive id;
    // flattened: by record slot (the hit index)
    float4 *r = attrs + (size_t)kAttrStride * (in.object_space ? prim : slot[i]);
    const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
    if (inst.kind == PUPIL_SHAPE_SPHERE) {
        r[0] = make_float4(0.f, 0.f, 0.f, __uint_as_float(prim | kPrimSphereBit));
        r[1] = make_float4(0.f, 0.f, 0.f, __uint_as_float(inst_id));
        r[2] = r[3] = r[4] = r[5] = r[6] = r[7] = z;
        return;
    }
    const uint32_t local = prim - inst.prim_offset;
    const uint32_t i0 = inst.indices[3 * local], i1 = inst.indices[3 * local + 1], i2 = inst.indices[3 * local + 2];
    const float *P = inst.positions;
    r[0] = make_float4(P[3 * i0], P[3 * i0 + 1], P[3 * i0 + 2], __uint_as_float(prim));
    r[1] = make_float4(P[3 * i1], P[3 * i1 + 1], P[3 * i1 + 2], __uint_as_float(inst_id));
    float nn[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (inst.normals) {
        const float *N = inst.normals;
        const uint32_t id[3] = {i0, i1, i2};
        for (int v = 0; v < 3; v++)
            for (int c = 0; c < 3; c++) nn[3 * v + c] = N[3 * id[v] + c];
    }
    r[2] = make_float4(P[3 * i2], P[3 * i2 + 1], P[3 * i2 + 2], nn[0]);
    r[3] = make_float4(nn[1], nn[2], nn[3], nn[4]);
    r[4] = make_float4(nn[5], nn[6], nn[7], nn[8]);
    if (inst.texcoords) {
        const float *T = inst.texcoords;
        r[5] = make_float4(T[2 * i0], T[2 * i0 + 1], T[2 * i1], T[2 * i1 + 1]);
        r[6] = make_float4(T[2 * i2], T[2 * i2 + 1], 0.f, 0.f);
    } else {
        r[5] = r[6] = z;
    }
    r[7] = z;
}

__global__ void k_reorder(int n, const uint32_t *sorted_vals, const uint32_t *slot, const float4 *recs_in,
                          float4 *recs_out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t src = sorted_vals[i];
    float4 *o = recs_out + (size_t)kRecF4 * slot[i];
    o[0] = recs_in[3 * src + 0];
    o[1] = recs_in[3 * src + 1];
    o[2] = recs_in[3 * src + 2];
}

// Record slots (kRecF4): every leaf's slot count 2 ceil(c / 2) at its first primitive,
// scanned, gives each leaf a first slot on a 128-B line
__global__ void k_leaf_marks(const Bvh4Node *nodes, uint32_t m, unsigned long long *lsz) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= m) return;
    const Bvh4Node nd = nodes[j];
    for (int k = 0; k < 4; k++) {
        const int l = nd.child[k];
        if (l != kEmptyLink && l < 0) lsz[leaf_first(l)] = leaf_slots(leaf_count(l));
    }
}
// each leaf's primitives -> their slots; its link now names its first slot
__global__ void k_leaf_slots(Bvh4Node *nodes, uint32_t m, const unsigned long long *first_slot, uint32_t *slot) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= m) return;
    Bvh4Node nd = nodes[j];
    for (int k = 0; k < 4; k++) {
        const int l = nd.child[k];
        if (l == kEmptyLink || l >= 0) continue;
        const uint32_t f = leaf_first(l), c = leaf_count(l), fs = (uint32_t)first_slot[f];
        for (uint32_t q = 0; q < c; q++) slot[f + q] = fs + q;
        nd.child[k] = make_leaf(fs, c);
    }
    nodes[j] = nd;
}

constexpr int kReinsDefault = 2;  // PUPIL_BVH_REINSERT

// The one place the builder reads its environment.  leaf_size: already clamped to [1, kLeafMax].
BuildOptions read_build_options(uint32_t leaf_size) {
    BuildOptions o;
    const char *e = std::getenv("PUPIL_BVH_BUILDER");
    if (e && std::strcmp(e, "lbvh") == 0) o.builder = BuildOptions::Builder::Karras;
    e = std::getenv("PUPIL_BVH4_COLLAPSE");
    if (e && std::strcmp(e, "parity") == 0) o.collapse = BuildOptions::Collapse::Parity;
    else if (e && std::strcmp(e, "greedy") == 0) o.collapse = BuildOptions::Collapse::Greedy;
    o.sah_leaf = leaf_size;  // larger leaves where the SAH prefers them (<= 8)
    if ((e = std::getenv("PUPIL_SAH_LEAF"))) o.sah_leaf = (uint32_t)std::min(8, std::max((int)leaf_size, std::atoi(e)));
    o.reinsert_rounds = kReinsDefault;  // 0: the PLOC tree as built
    if ((e = std::getenv("PUPIL_BVH_REINSERT"))) o.reinsert_rounds = std::min(64, std::max(0, std::atoi(e)));
    o.reinsert_log = std::getenv("PUPIL_BVH_REINSERT_LOG") != nullptr;
    return o;
}

// Stage 4.  Record slots: each leaf on a 128-B line (kRecF4), the links of out.nodes4 rewritten
// to slots; then the primitive records (recs, in primitive order) and the shading records in
// slot order.  order: the tree's primitive order.  Fills out.prims / attrs / num_records.
hipError_t leaf_slots_and_records(const BvhBuildInput &in, const uint32_t *order, const float4 *recs, bool leaf_root,
                                  BvhBuildOutput &out, hipStream_t s) {
    const uint32_t nrec = in.num_prims;
    const uint32_t g = (nrec + kBlock - 1) / kBlock;
    hipError_t err = hipSuccess;
    auto slot = scratch<uint32_t>(err, nrec);
    auto lsz = scratch<unsigned long long>(err, nrec);
    auto ssum = scratch<unsigned long long>(err, scan64_blocks((int)nrec));
    auto stot = scratch<unsigned long long>(err, 1);
    if (err) return err;
    const uint32_t m = leaf_root ? 0u : out.num_nodes4;
    const uint32_t gm = (m + kBlock - 1) / kBlock;
    err = hipMemsetAsync(lsz.get(), 0, sizeof(unsigned long long) * nrec, s);
    if (leaf_root && !err) {
        const unsigned long long v = leaf_slots(nrec);
        err = hipMemcpyAsync(lsz.get(), &v, sizeof(v), hipMemcpyHostToDevice, s);
    }
    if (err) return err;
    if (m) hipLaunchKernelGGL(k_leaf_marks, dim3(gm), dim3(kBlock), 0, s, out.nodes4, m, lsz.get());
    err = scan64(lsz.get(), (int)nrec, ssum.get(), stot.get(), s);
    if (err) return err;
    if (m) hipLaunchKernelGGL(k_leaf_slots, dim3(gm), dim3(kBlock), 0, s, out.nodes4, m, lsz.get(), slot.get());
    if (leaf_root) {  // the root leaf: slots 0 .. n-1
        std::vector<uint32_t> id(nrec);
        for (uint32_t q = 0; q < nrec; q++) id[q] = q;
        err = hipMemcpyAsync(slot.get(), id.data(), sizeof(uint32_t) * nrec, hipMemcpyHostToDevice, s);
        if (!err) err = hipStreamSynchronize(s);
    }
    unsigned long long tot = 0;
    if (!err) err = hipMemcpyAsync(&tot, stot.get(), sizeof(tot), hipMemcpyDeviceToHost, s);
    if (!err) err = hipStreamSynchronize(s);
    const uint32_t nslots = (uint32_t)tot;
    if (!err && tot >= (1ull << 28)) err = hipErrorInvalidValue;  // leaf links hold 28-bit slots
    auto prims = scratch<float4>(err, (size_t)kRecF4 * nslots);
    if (!err) err = hipMemsetAsync(prims.get(), 0xFF, sizeof(float4) * kRecF4 * (size_t)std::max(1u, nslots), s);
    const size_t nattr = in.object_space ? (size_t)nrec : (size_t)nslots;
    auto attrs = scratch<float4>(err, (size_t)kAttrStride * nattr);
    if (err) return err;
    hipLaunchKernelGGL(k_reorder, dim3(g), dim3(kBlock), 0, s, (int)nrec, order, slot.get(), recs, prims.get());
    hipLaunchKernelGGL(k_attrs, dim3(g), dim3(kBlock), 0, s, (int)nrec, order, slot.get(), in, attrs.get());
    err = hipStreamSynchronize(s);
    if (err) return err;
    out.prims = prims.release();
    out.attrs = attrs.release();
    out.num_records = nslots;
    return hipSuccess;
}

// build_lbvh between its timing events: primitive setup and the four stages.  recs: 3 float4
// per primitive of scratch; fe: the front end's arrays for in.num_prims boxes.
hipError_t build_stages(const BvhBuildInput &in, BvhBuildOutput &out, uint32_t leaf_size, const BuildOptions &opts,
                        float4 *recs, FrontEnd &fe, hipStream_t s) {
    const int n = (int)in.num_prims;
    hipLaunchKernelGGL(k_prim_setup, grid_for(n), dim3(kBlock), 0, s, in, recs, fe.boxes.get());
    morton_order(fe, n, s);
    Collapsed c4;
    hipError_t err = hipSuccess;
    if (n > 1) {
        err = binary_tree(fe, n, opts, s);
        if (!err) err = collapse_bvh4(fe.tree(n), leaf_size, opts, fe.spare_keys, fe.spare_vals, s, c4);
    } else {
        c4.nodes4 = scratch<Bvh4Node>(err, 1);
    }
    if (err) return err;
    out.nodes4 = c4.nodes4.release();
    out.num_nodes4 = c4.num_nodes4;
    out.depth4 = c4.depth4;
    out.level_start = std::move(c4.level_start);
    const bool leaf_root = (uint32_t)n <= leaf_size;
    err = leaf_slots_and_records(in, fe.sorted_vals, recs, leaf_root, out, s);
    if (err) return err;
    if (n == 1 || leaf_root) out.depth4 = 1;  // the root is a leaf
    out.root_link4 = leaf_root ? (uint32_t)make_leaf(0u, (uint32_t)n) : 0u;
    if (leaf_root && !in.object_space) {
        // the root leaf is the whole tree: the 4-wide root the collapse emitted for 1 < n <= leaf_size
        // is referenced by nothing, so it is not counted, exported, refitted or part of the node
        // bound (a two-level BLAS keeps its count, which the combined node array is laid out by)
        out.num_nodes4 = 0;
        out.level_start.clear();
    }
    return hipGetLastError();
}

}  // namespace

void free_lbvh(BvhBuildOutput &out) {
    if (out.nodes4) (void)hipFree(out.nodes4);
    if (out.prims) (void)hipFree(out.prims);
    if (out.attrs) (void)hipFree(out.attrs);
    out.nodes4 = nullptr;
    out.prims = nullptr;
    out.attrs = nullptr;
}

int build_lbvh(const BvhBuildInput &in, BvhBuildOutput &out, uint32_t leaf_size, hipStream_t s, double *build_ms,
               bool force_lbvh) {
    const int n = (int)in.num_prims;
    if (n <= 0) {  // empty scene: every ray misses
        out = BvhBuildOutput{};
        out.root_link4 = (uint32_t)kTraverseDone;
        if (build_ms) *build_ms = 0.0;
        return 0;
    }
    if (leaf_size < 1) leaf_size = 1;
    if (leaf_size > (uint32_t)kLeafMax) leaf_size = kLeafMax;
    BuildOptions opts = read_build_options(leaf_size);
    if (force_lbvh) opts.builder = BuildOptions::Builder::Karras;
    out.depth4 = 0;
    out.level_start.clear();
    hipEvent_t e0, e1;
    (void)hipEventCreate(&e0);
    (void)hipEventCreate(&e1);
    (void)hipEventRecord(e0, s);

    // the scratch that spans the stages is freed after the timing, on return
    hipError_t err = hipSuccess;
    auto recs = scratch<float4>(err, 3 * (size_t)n);
    FrontEnd fe(err, n, true);
    if (!err) err = build_stages(in, out, leaf_size, opts, recs.get(), fe, s);
    if (err) free_lbvh(out);

    (void)hipEventRecord(e1, s);
    (void)hipEventSynchronize(e1);
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, e0, e1);
    if (build_ms) *build_ms = ms;
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    return err == hipSuccess ? 0 : -2;
}

// BVH4 over n boxes (lo xyz, hi xyz; the world-mode TLAS over braided entries,
// accel_two_level.hip): Morton order, PLOC and the SAH-optimal collapse of the flattened
// build with one box per leaf.  On return `nodes` holds the 4-wide nodes (root 0,
// breadth first: parents before children) whose leaf links make_leaf(p, 1) name the
// box order[p].  n >= 2.
int build_bvh4_over_boxes(const float *h_boxes, uint32_t n, std::vector<Bvh4Node> &nodes, std::vector<uint32_t> &order,
                          uint32_t *depth, hipStream_t s, int rounds, ReinsertLog *log) {
    if (n < 2) return -1;
    BuildOptions opts = read_build_options(1u);
    opts.builder = BuildOptions::Builder::Ploc;  // always the default tree, whatever the flat build is told
    opts.collapse = BuildOptions::Collapse::Sah;
    if (rounds >= 0) opts.reinsert_rounds = rounds;  // < 0: the environment's value or its default
    const int m = (int)n;
    hipError_t err = hipSuccess;
    FrontEnd fe(err, m, false);
    Collapsed c4;
    if (!err) err = hipMemcpyAsync(fe.boxes.get(), h_boxes, sizeof(Aabb) * n, hipMemcpyHostToDevice, s);
    if (!err) {
        morton_order(fe, m, s);
        err = binary_tree(fe, m, opts, s, log);
    }
    if (!err) err = collapse_bvh4(fe.tree(m), 1u, opts, fe.spare_keys, fe.spare_vals, s, c4);
    if (!err) {
        nodes.resize(c4.num_nodes4);
        order.resize(n);
        err = hipMemcpyAsync(nodes.data(), c4.nodes4.get(), sizeof(Bvh4Node) * c4.num_nodes4, hipMemcpyDeviceToHost, s);
        if (!err) err = hipMemcpyAsync(order.data(), fe.sorted_vals, sizeof(uint32_t) * n, hipMemcpyDeviceToHost, s);
        if (!err) err = hipStreamSynchronize(s);
    }
    if (depth) *depth = c4.depth4;
    return err == hipSuccess ? 0 : -2;
}

int build_bvh_bounded(const BvhBuildInput &in, BvhBuildOutput &out, uint32_t leaf_size, hipStream_t s,
                      double *build_ms, uint32_t reserve) {
    const auto fits = [&](const BvhBuildOutput &o) {
        return o.depth4 == 0 || 3u * o.depth4 + reserve <= (uint32_t)kTraceStackEntries;
    };
    int rc = build_lbvh(in, out, leaf_size, s, build_ms);
    if (rc != 0 || fits(out)) return rc;
    // PLOC merges nearest neighbours bottom-up and can chain a skewed primitive
    // distribution into a deep tree; the Karras LBVH splits on Morton bits.
    free_lbvh(out);
    double ms2 = 0.0;
    rc = build_lbvh(in, out, leaf_size, s, &ms2, true);
    if (build_ms) *build_ms += ms2;
    if (rc != 0) return rc;
    if (!fits(out)) {
        free_lbvh(out);
        return -3;
    }
    return 0;
}

}  // namespace pupil
