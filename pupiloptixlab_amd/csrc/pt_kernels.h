// pt_kernels.h — host-visible declarations of the wavefront stages and the
// LBVH builder (implemented in pt_kernels.hip / bvh_build.hip).
#pragma once

#include <vector>

#include <hip/hip_runtime.h>

#include "pt_scene.h"
#include "host/instance_record.h"

namespace pupil {

constexpr int kTraceBlock = 128;
// persistent BVH4 kernels: occupancy target (<= 72 VGPRs; 6 waves: 3 % slower, 8 waves at <= 64 VGPRs:
// 8-11 % slower, r03 / r05 A/B, profiles/r05_stack_ab.txt)
constexpr int kTraceWavesPerSimd = 7;
constexpr int kTraceWavesPerSimdTL = 5;  // two-level variant (<= 96 VGPRs; A/B r02 on config 5: 4 waves 688, 5: 743, 6: 716 Mrays/s)
constexpr int kStackOvf = 160;  // per-thread global overflow entries
constexpr int kRing = 16;       // persistent BVH4 kernels: per-lane LDS ring entries (spills to the overflow column)
// Stack entries a traversal may need: 3 per BVH4 level (4 children, one taken), plus
// 2 per instance entry in two-level mode.  Builds whose trees need more are rejected
// (or rebuilt with the depth-bounded Karras LBVH) at create time, so no kernel ever
// overwrites a live entry.
constexpr int kTraceStackEntries = kRing + kStackOvf;
constexpr int kShadeBlock = 256;
constexpr uint32_t kShadeMaxBlocks = 16384;  // largest shade grid (pt_kernels.hip shade_blocks)
constexpr uint32_t kMaxDepth = 128;  // PTPass inspector range (pt_pass.cpp:225-237)
constexpr uint32_t kNumQueues = 9;  // 0 = miss, 1..7 = EMatType, 8 = unknown material
constexpr uint32_t kMissIndex = 0xFFFFFFFFu;

// Path state in HBM, structure of arrays indexed by path id
// p = sample * num_local_pixels + local_pixel.
struct PathState {
    float4 *ray_o;      // xyz origin of the current ray (and of its shadow ray: w = the shadow ray's tmax)
    float4 *ray_d;      // xyz direction
    float4 *hit;        // t, b1, b2, sorted primitive index (bits) or kMissIndex
    float4 *thr;        // xyz throughput, w = pdf of the BSDF sample that spawned the ray
    float4 *rad;        // xyz radiance
    uint4 *misc;        // x rng, y bounce (bits 0..23) | delta << 31, z/w texcoord (stale semantics, geometry.h:298-304)
    float4 *sh_d;       // shadow ray direction
    float4 *sh_c;       // pending NEE contribution
    uint8_t *mbin;      // extend -> material bin of the hit (0 miss, 1..7 EMatType, 8 unknown), 0xFF = not traced
    uint8_t *sflags;    // shade -> bit 0: extension ray spawned, bit 1: shadow ray spawned, bits 2..7: bounce tag
};

// Bounce tag of the shade flags byte: the flags partition after bounce b lists
// only bytes carrying tag(b), so the flags a path left when it died are never
// listed again and no per-bounce clear is needed.  Depths above 63 would alias
// the 6-bit tag: there the tag is 0 and the engine clears the bytes per bounce.
__host__ __device__ inline uint32_t sflag_tag(uint32_t max_depth, uint32_t bounce) {
    return max_depth <= 63u ? bounce % 63u + 1u : 0u;
}

// Queues are rebuilt by a stable partition (queue_partition.hip) after each
// stage, so every queue lists path ids in increasing order.
constexpr int kPartMaxBins = 9;
// counts[] slots
constexpr uint32_t kCntNext = 9, kCntShadow = 10;                      // queue lengths
// persistent-kernel work counters: per kind kWorkShards dequeue heads (one per
// XCD), one final exit counter and kWorkShards exit sub-counters, each on its
// own 128-B line.  Zero at allocation; the last wave of every persistent launch
// puts them back to zero.
constexpr uint32_t kWorkShards = 8, kWorkStride = 32, kWorkKind = (2 * kWorkShards + 1) * kWorkStride;
// slot 1 * kWorkKind is unused (it served the separate any-hit launch, retired in r01)
constexpr uint32_t kWorkExtend = 0, kWorkRays = 2 * kWorkKind, kWorkFrame = 3 * kWorkKind;
constexpr uint32_t kWorkFlow = 4 * kWorkKind;  // the flow pass's traversal (pupil_pt_motion_vectors)
constexpr uint32_t kWorkQuery = 5 * kWorkKind;  // ray queries from device memory (pupil_pt_query_rays / _query_camera)
// path-traced radiance along rays (pupil_pt_radiance_rays): the work pointer of its own Queues, whose
// launches add kWorkExtend like every other
constexpr uint32_t kWorkRadiance = 6 * kWorkKind;
constexpr uint32_t kWorkSlots = 7 * kWorkKind;
constexpr uint32_t kStartBins = 16;                                    // [16..24] material bin starts
constexpr uint32_t kStartNext = 25, kStartShadow = 26;                 // next / shadow regions of nxsh
constexpr uint32_t kScratch = 27;
constexpr uint32_t kCountSlots = 32;

// Terminal-ray cull: the largest cull set (DeviceScene::cull_set; the engine's cap is
// PUPIL_TERMINAL_CULL_K, 8 unless set) and the sharded counter of culled rays
constexpr uint32_t kCullSetMax = 32;
constexpr uint32_t kCullShards = 64, kCullStride = 16;  // counters, and 64-bit words between two

struct Queues {
    uint32_t *bins;      // capacity: material bin b occupies [counts[kStartBins + b], + counts[b])
    uint32_t *nxsh;      // 2 * capacity: next ids from counts[kStartNext] (= 0), shadow ids from counts[kStartShadow]
    uint32_t *counts;    // kCountSlots entries, see above
    uint32_t *hist;      // partition scratch, partition_hist_entries(capacity)
    uint32_t *work;      // kWorkSlots persistent-kernel work heads (see kWorkExtend)
    uint32_t capacity;
};

// partition key modes (queue_partition.hip)
enum PartMode : int {
    kPartExclusive = 0,  // bin = key >> shift (0xFF = none)
    kPartFlags = 1,      // bin b <=> bit b of the key, if key >> 2 == tag (passed as `shift`)
};

struct FrameParams {
    uint32_t width, height;
    uint32_t num_local;    // local pixels
    uint32_t num_paths;    // num_local * spp
    uint32_t spp;
    uint32_t seed0;
    uint32_t cnt0;
    uint32_t accumulate;
    uint32_t max_depth;
    uint32_t compact;
    const uint32_t *pixel_map;  // local -> global pixel (null = identity)
    float4 *accum;
    float4 *frame;
    float *albedo;  // 3 floats per pixel
    float *normal;
    float *test;
    unsigned long long *nee_count;  // collect_stats: paths that reached the shadow test (main.cu:113-123)
    // terminal-ray cull (pt_shade.h terminal_ray_culled): running total of the extension rays the
    // emitter test resolved, kCullShards counters one 128-B line apart (a wave adds to the one of
    // its block); null = the cull is off for this render
    unsigned long long *cull_cum;
    // shade: the AOV pointers above are indexed by the local pixel (compact output, or the
    // per-slot AOV scratch of a frame that completes in a later render); else by y*w+x
    uint32_t aov_local;
    // pipelined frame groups (engine.hip render_pipelined): a ring slot holds `group` frames of
    // spp samples; frame f of a slot writes its AOVs at + f * aov_frame_stride floats (0: one
    // frame per slot, or the render's own buffers)
    uint32_t group;
    uint32_t aov_frame_stride;
};

// Path-state records are streamed with non-temporal loads / stores (r03), so the GBs of path state a step moves do not push BVH nodes and primitive records out of
// the L2s and the Infinity Cache.
__device__ __forceinline__ float4 ld_ps(const float4 *a) {
    typedef float v4f __attribute__((ext_vector_type(4)));
    const v4f v = __builtin_nontemporal_load(reinterpret_cast<const v4f *>(a));
    return make_float4(v.x, v.y, v.z, v.w);
}
__device__ __forceinline__ uint4 ld_ps(const uint4 *a) {
    typedef unsigned v4u __attribute__((ext_vector_type(4)));
    const v4u v = __builtin_nontemporal_load(reinterpret_cast<const v4u *>(a));
    return make_uint4(v.x, v.y, v.z, v.w);
}
__device__ __forceinline__ void st_ps(float4 *a, float4 v) {
    typedef float v4f __attribute__((ext_vector_type(4)));
    v4f w = {v.x, v.y, v.z, v.w};
    __builtin_nontemporal_store(w, reinterpret_cast<v4f *>(a));
}
__device__ __forceinline__ void st_ps(uint4 *a, uint4 v) {
    typedef unsigned v4u __attribute__((ext_vector_type(4)));
    v4u w = {v.x, v.y, v.z, v.w};
    __builtin_nontemporal_store(w, reinterpret_cast<v4u *>(a));
}

// The instance holding global primitive `idx`: the last instance i in the guide's range with
// inst_first[i] <= idx (an instance without primitives shares its first id with the next one,
// which is the one that holds it), i.e. exactly prim_inst[idx].
#ifndef PUPIL_INST_GUIDE
#define PUPIL_INST_GUIDE 1
#endif
__device__ __forceinline__ uint32_t inst_of_prim(const DeviceScene &sc, uint32_t idx) {
    if (!PUPIL_INST_GUIDE) return sc.prim_inst[idx];
    const uint32_t k = idx >> sc.inst_guide_shift;
    uint32_t lo = sc.inst_guide[k], hi = sc.inst_guide[k + 1];
    while (lo < hi) {
        const uint32_t mid = (lo + hi + 1u) >> 1;
        if (sc.inst_first[mid] <= idx) lo = mid;
        else hi = mid - 1u;
    }
    return lo;
}

struct TraceStats {
    unsigned long long *counters;  // [0..1] closest-hit nodes/prims, [14..15] shadow, [2..13] diagnostics,
                                   // [16] reference shadow rays, [18] distinct node fetches,
                                   // [20..23] queue accounting (handed, activated, retired, listed),
                                   // [24..25] occluded shadow rays: their node visits, their number
    // PUPIL_TRACE_TAIL diagnostics (STATS kernels only, else null): per wave of the
    // persistent launch, s_memrealtime (100 MHz) at start, when its dequeue found
    // the work list drained, at exit, and the rays it took
    unsigned long long *wave_times = nullptr;
};

// wavefront stages
// full = false: only the camera rays (the list shade then treats the batch as fresh paths)
void launch_generate(const DeviceScene &sc, const FrameParams &fp, const PathState &ps, hipStream_t s, bool full);
// interleave_spp / num_local (primary extend, queue == null): dequeue the spp samples of
// a pixel on consecutive lanes (TraceJob::spp); 0 = path order
void launch_extend(const DeviceScene &sc, const PathState &ps, const Queues &q, const uint32_t *queue,
                   const uint32_t *queue_count, uint32_t static_count, int *ovf, uint32_t ovf_threads,
                   const TraceStats *stats, hipStream_t s, uint32_t interleave_spp = 0, uint32_t num_local = 0);
// which paths a shade launch walks: the material-bin partition (q.bins), a range of path
// ids (every path of a batch after its primary extend), the previous bounce's next list
// (q.nxsh), or that next list followed by a range (pipelined frames: the extension rays of
// the frames in flight, then the camera rays of the frame started in the same launch).
// Each path's bounce is read from its state (PathState::misc.y), so one launch may shade
// paths of several frames at different bounces; `tag` is the bounce tag the launch writes
// into the flags bytes (sflag_tag, or the pipeline's generation tag).
// fresh_range (list modes): the range is a batch whose k_generate stored only its camera rays
// (full = false), first frame seed fresh_seed0; its bounce-0 shade derives throughput 1,
// radiance 0 and the camera RNG instead of reading them.
enum ShadeList : int { kShadeBins = 0, kShadeAll = 1, kShadeNext = 2, kShadeNextRange = 3 };
void launch_shade(const DeviceScene &sc, const FrameParams &fp, const PathState &ps, const Queues &q, uint32_t tag,
                  hipStream_t s, ShadeList list, uint32_t range_base, uint32_t range_n, uint32_t max_count,
                  bool fresh_range = false, uint32_t fresh_seed0 = 0);
// The shade kernels' block-resident scene tables (pt_shade.h BlockTables).  shade_table_caps: the
// entry caps of the instance, material, area-emitter and cull-set copies, in that order;
// shade_tables_fit: bit k set = table k of `sc` is within its cap and is read from the LDS copy
void shade_table_caps(uint32_t caps[4]);
uint32_t shade_tables_fit(const DeviceScene &sc);
// one persistent launch over the next + shadow lists of a bounce (BVH4 persistent path only)
// ahead_count > 0 (render-ahead, BVH4 kernels only): the launch also traces the camera
// rays of the next render.  `ps` is then the base of both buffer halves: this render's
// listed paths are at list_base + id, the next render's camera rays (generated there)
// at ahead_base + [0, ahead_count), dequeued pixel-major when ahead_spp > 1 (as the
// primary extend)
// any_overlap: the any-hit lanes' child order (pt_traverse.h visit4)
void launch_trace_mixed(const DeviceScene &sc, const PathState &ps, const Queues &q, int *ovf, uint32_t ovf_threads,
                        const TraceStats *stats, hipStream_t s, uint32_t ahead_count = 0, uint32_t list_base = 0,
                        uint32_t ahead_base = 0, uint32_t ahead_spp = 0, uint32_t ahead_local = 0,
                        uint32_t any_overlap = 0);
// small frames (pt_frame.hip): every path of the frame -- camera ray, bounces, shadow rays --
// in one persistent launch (no partitions, one drain); the accumulate follows.  Flat BVH4 and
// two-level world mode only.  ray_cum: running totals of extension [0] and shadow [1] rays.
bool frame_kernel_supported(const DeviceScene &sc);
void launch_frame(const DeviceScene &sc, const FrameParams &fp, const PathState &ps, uint32_t *work,
                  unsigned long long *ray_cum, int *ovf, uint32_t ovf_threads, uint32_t interleave_spp, hipStream_t s);
// running mean of the batch's frames into fp.accum / fp.frame; aov_src (or null): the
// frame's AOVs from the slot scratch (3n albedo, 3n normal, n test floats) copied to the
// outputs; clear_flags: zero the frame's flags bytes (its ring slot is free again)
// per axis max of |o| + 512 s over n BVH4 nodes into out[0..2] (float bits; clear: out is
// zeroed first, else the max also covers what it holds), the bound DeviceScene::node_bound holds
void launch_node_bound(const Bvh4Node *nodes, uint64_t n, uint32_t *out, hipStream_t s, bool clear = true);
void launch_accumulate(const FrameParams &fp, const PathState &ps, const float *aov_src, bool clear_flags,
                       hipStream_t s);
uint32_t trace_grid_blocks();
// stats (or null): the persistent kernels' counter variants (queue accounting, node visits)
void launch_trace_debug(const DeviceScene &sc, const float *rays, float *out, uint32_t n, int any, int *ovf,
                        uint32_t ovf_threads, uint32_t *work, hipStream_t s, const TraceStats *stats = nullptr,
                        uint32_t any_overlap = 0);
// flow AOV (pt_flow.hip): the camera rays through the centres of the n local pixels as a
// kModeRays ray list (2 float4 per ray), and the projection of their hits (launch_trace_debug's
// 4 floats per ray) through the previous camera into flow[compact ? local pixel : y*w+x]
struct FlowJob {
    float world_to_sample[16];   // previous camera: sample <- world, row-major (inverted in double on the host)
    const float *prev_to_world;  // device, 12 floats per instance (row-major 3x4), null = no instance moved
    const uint32_t *pixel_map;   // local -> global pixel (null = identity)
    uint32_t width, height;
    uint32_t n;                  // local pixels
    uint32_t compact;
};
// (jitter_x, jitter_y): the film jitter of every ray, camera_path's (jx, jy); the flow pass passes
// the pixel centre (0.5, 0.5)
void launch_flow_rays(const DeviceScene &sc, uint32_t width, uint32_t height, const uint32_t *pixel_map, uint32_t n,
                      float jitter_x, float jitter_y, float4 *rays, hipStream_t s);
// prev_verts (deforming meshes, pupil_pt_snapshot_shape_vertices): device, per instance the
// vertices its shape had before the update (3 floats per vertex) or null.  null = no shape holds
// a snapshot: the kernel and its arguments are then those of the rigid-only pass.
void launch_flow_project(const DeviceScene &sc, const FlowJob &job, const float4 *rays, const float4 *hits,
                         float2 *flow, hipStream_t s, const float *const *prev_verts = nullptr);
// ray queries (pt_query.hip): the compact hits of a kModeRays launch (launch_trace_debug's 4 floats
// per ray) resolved into the arrays that are not null -- instance, face within its shape, material
// (-1 on a miss), and reconstruct()'s position, normal (two-sided flip applied) and texcoord (0 on
// a miss).  rays: the list the hits were traced from, 2 float4 per ray.  prim_slot / slots (flat
// scenes with a position, normal or texcoord wanted): global primitive id -> record slot, as
// launch_query_prim_slots derives it from the `slots` record slots of DeviceScene::prims;
// two-level scenes pass null and any slots > 0
struct QueryJob {
    const float4 *rays;
    const float4 *hits;
    uint32_t n;
    uint32_t slots;
    const uint32_t *prim_slot;
    int32_t *instance, *primitive, *material;
    float *position, *normal;  // 3 floats per ray
    float2 *texcoord;
    // a tiled camera query in the frame's index space: ray l's outputs go to element out_index[l]
    // (null = l), and its hit is copied to hit_out there (null = the hits are where they belong)
    const uint32_t *out_index;
    float4 *hit_out;
};
void launch_query_prim_slots(const float4 *recs, uint32_t slots, uint32_t num_prims, uint32_t *prim_slot,
                             hipStream_t s);
void launch_query_resolve(const DeviceScene &sc, const QueryJob &job, hipStream_t s);
// radiance along rays (pt_radiance.hip): the full path records (k_generate's, full = 1) of a chunk
// of a caller's ray list -- path sample * num_local + l is sample `sample` of ray ray_base + l,
// its origin and direction the ray's (2 float4 per ray; floats 6 and 7 are not read), its RNG
// rng_init(id, seed0 + sample) after two discarded draws, id = stream_ids[ray_base + l] or, when
// null, ray_base + l.  launch_identity_ids: ids[i] = i, the queue that makes launch_extend read
// each path's origin from its state
struct RayGenJob {
    const float4 *rays;
    const uint32_t *stream_ids;
    uint32_t ray_base;
    uint32_t num_local;  // rays of the chunk
    uint32_t num_paths;  // num_local * samples of the chunk
    uint32_t seed0;      // seed of the chunk's first sample
};
void launch_generate_rays(const RayGenJob &job, const PathState &ps, hipStream_t s);
void launch_identity_ids(uint32_t *ids, uint32_t n, hipStream_t s);
// the area-emitter table rebuilt in place from the engine's own arrays (pt_emitters.hip): in every
// DevEmitter pos, nrm, area and select_probability (a sphere: center, radius, area and
// select_probability), the selection CDF and, unless null, its guide table
struct EmitterJob {
    DevEmitter *areas;
    float *cdf;
    uint32_t *guide;       // null = the table has none
    uint32_t guide_bits;
    uint32_t count;        // triangle and sphere emitters: table entries [0, count)
    uint32_t total;        // + the delta lights, entries [count, total): cdf, select and the guide span these
    uint32_t emitter_num;  // total + 1 with an env emitter
    const DevInstance *instances;
    const uint32_t *emit_inst;  // per emitter: its instance
    const float *inst_weight;   // per instance: GetWeight of its radiance (0 where not emissive)
    float *weight, *select;     // scratch, one float per table entry
    float *sum;                 // scratch, one float
};
// returns the kernels it launched.  No triangle or sphere emitter (count == 0) but delta lights:
// the stages from the select probabilities on still run, over the delta lights alone
uint32_t launch_emitter_rebuild(const EmitterJob &job, hipStream_t s);
// A table of a new size (pt_emitters.hip k_emit_fill): every byte of areas[0, count) that the
// rebuild above does not write -- zero but for type, radiance and a triangle's tex -- and
// emit_inst[0, count), from the emissive instances' emitter ranges.  sources: num_sources entries
// in instance order, their offsets increasing from 0; count = the end of the last range
struct EmitterFillJob {
    DevEmitter *areas;
    uint32_t *emit_inst;
    uint32_t count;
    const DevEmitSource *sources;
    uint32_t num_sources;
    const DevInstance *instances;
};
void launch_emitter_fill(const EmitterFillJob &job, hipStream_t s);
// the cull set's scan (pt_emitters.hip): out[0] (zero at launch) counts the record slots of `recs`
// whose instance is emissive, out[1 + k] holds the k-th found for k < cap, in no order
void launch_cull_scan(const float4 *recs, uint32_t slots, const DevInstance *instances, uint32_t num_instances,
                      uint32_t *out, uint32_t cap, hipStream_t s);
// Material updates (pt_materials.hip).  launch_specular_weight: mat->specular_sampling_weight of a
// plastic or rough_plastic recomputed from the texels its diffuse and specular slots hold on the
// device now, bit for bit the host's value (other types: nothing is launched by the caller, and
// the kernel writes nothing).  launch_record_bins: the material-bin word (c.w) of every record
// slot follows DevInstance::bin of the slot's instance (b.w); hole slots stay.
void launch_specular_weight(DevMaterial *mat, hipStream_t s);
void launch_record_bins(float4 *recs, uint32_t slots, const DevInstance *instances, uint32_t num_instances,
                        hipStream_t s);
// The env map's tables rebuilt in place from the engine's own texels (pt_envmap.hip): col_cdf
// ((w + 1) * h), row_cdf (h + 1) and env->normalization, bit for bit what convert_emitter
// (host/emitter_tables.h) derives from the same texels.  row_weight (h, the host's std::sin) is read only;
// col_sum: scratch, h floats.  kEnvStage: the values a wave stages in the LDS per chunk of a chain.
constexpr uint32_t kEnvStage = 1024;
struct EnvTablesJob {
    const float4 *texels;  // w * h, row-major
    uint32_t w, h;
    float *col_cdf, *row_cdf;
    const float *row_weight;
    float *col_sum;
    DevEmitter *env;
};
void launch_env_tables(const EnvTablesJob &job, hipStream_t s);
// Instance transforms from device memory (pt_instances.hip): entry k of the list moves instance
// ids[k] (null: k) to to_world[12k..], with to_object[12k..] or, null, the inverse computed on the
// device.  An id >= num_instances is skipped and counted in *skipped, a running total.  stage:
// kMoveStageFloats floats per entry for the host mirror -- to_world, to_object (the real one, also
// where the device copy of a hidden sphere gets NaN), the two margins, then six floats the box
// gather fills (two-level).  list (or null): the ids as the structure kernels take them, `fallback`
// (an id in range that the list holds anyway) in place of a skipped one.  moved (or null): the
// flattened refit's flags, cleared by the caller.  margins: recompute the two-level box margins.
constexpr uint32_t kMoveStageFloats = 32;
constexpr uint32_t kMoveStageBox = 26;
struct MoveInstancesJob {
    DevInstance *instances;
    uint32_t num_instances, n;
    const uint32_t *ids;
    const float *to_world, *to_object;
    uint32_t margins, fallback;
    float *stage;
    uint32_t *list;
    uint8_t *moved;
    uint32_t *skipped;
};
void launch_move_instances(const MoveInstancesJob &job, hipStream_t s);
// A mesh replaced in place (pt_replace.hip, pupil_pt_replace_shape_mesh).
// launch_index_max: atomicMax of the n indices into *out, which the caller has cleared.
// launch_prim_tables: prim_inst (num_prims entries) and inst_guide (guide_entries entries) from
// inst_first (num_instances + 1 entries), all device arrays (host/prim_tables.h: the geometry).
// launch_patch_instances: instances[i].prim_offset = inst_first[i], and the mesh instances whose
// positions are old_positions get the four new array pointers; with emitter_offsets (one per
// instance, or null) instances[i].emitter_offset = emitter_offsets[i] as well.
void launch_index_max(const uint32_t *idx, size_t n, uint32_t *out, hipStream_t s);
void launch_prim_tables(const uint32_t *inst_first, uint32_t num_instances, uint32_t num_prims, uint32_t shift,
                        uint32_t guide_entries, uint32_t *prim_inst, uint32_t *inst_guide, hipStream_t s);
struct ReplaceMeshJob {
    DevInstance *instances;
    uint32_t num_instances;
    const uint32_t *inst_first;
    const float *old_positions;
    const float *positions, *normals, *texcoords;
    const uint32_t *indices;
    const int32_t *emitter_offsets;
};
void launch_patch_instances(const ReplaceMeshJob &job, hipStream_t s);
// A new instance table (pt_instance_set.hip, pupil_pt_set_instances): out[i] for i < n from
// shapes[bindings[i].shape], bindings[i], inst_first[i] and the transform at to_world + 12 i;
// to_object: the inverses beside them, or null: each is computed (pt_invert.h).  A hidden sphere
// gets the NaN to_object of its device copy.  All device arrays; every bindings[i].shape indexes
// shapes.
struct FillInstancesJob {
    DevInstance *out;
    uint32_t n;
    const InstShape *shapes;
    const InstBinding *bindings;
    const uint32_t *inst_first;
    const float *to_world, *to_object;
};
void launch_fill_instances(const FillInstancesJob &job, hipStream_t s);
void launch_debug_math(const float *x, const float *y2, float *out, uint32_t n, hipStream_t s);
// device emitter selection for n random numbers: area index, -1 env, -2 none
void launch_debug_select(const DeviceScene &sc, const float *p, int *out, uint32_t n, hipStream_t s);
// the env emitter's emitter_sample_direct (mode 0, in = xi) or env_eval (mode 1, in = ray
// direction) on n device inputs of 3 floats; pos_nrm: 6 host floats; out: 8 floats per input
void launch_debug_env(const DeviceScene &sc, const float *in, const float *pos_nrm, uint32_t mode, float *out, uint32_t n,
                      hipStream_t s);
// emitter_sample_direct of the device emitter *e with xi = in.xy on n device inputs of 3 floats;
// pos_nrm: 6 host floats; out: 8 floats per input (wi, pdf, distance, radiance)
void launch_debug_emitter_sample(const DevEmitter *e, const float *in, const float *pos_nrm, float *out, uint32_t n,
                                 hipStream_t s);
// tex_sample of materials[material].tex[slot] on n device uv pairs; out: 3 floats per input
void launch_debug_tex(const DeviceScene &sc, uint32_t material, uint32_t slot, const float *uv, float *out, uint32_t n,
                      hipStream_t s);

// stable partition of path ids 0..n-1 by a key byte (queue_partition.hip)
uint32_t partition_hist_entries(uint32_t n);
// the tile geometry launch_partition uses for n paths: rounds of 64 paths per wave and the
// number of blocks (0 for n = 0: the launch is a few memsets)
void partition_geometry(uint32_t n, uint32_t *rounds, uint32_t *blocks);
// log_out (or null): the nbins counts; cum_out (or null): the counts are added to these
// nbins running 64-bit totals (rays traced since the engine was created); snap_out (or
// null): receives the totals as they were before this partition added to them -- it requires
// cum_out and is left unwritten without it; bin_mask (or 0 = every bin below nbins; bits at or
// above nbins are ignored): the bins a key can name -- the others are reported empty without
// being ranked (the material partition of a scene with few materials).  A key that names a
// masked-out bin or a bin at or above nbins is dropped: its path is in no list.
// (tests/test_queue_partition.py pins both.)
void launch_partition(const uint8_t *keys, uint32_t n, uint32_t nbins, PartMode mode, uint32_t shift, uint32_t *out,
                      uint32_t *hist, uint32_t *counts_out, uint32_t *starts_out, uint32_t *total_out, uint32_t *log_out,
                      hipStream_t s, unsigned long long *cum_out = nullptr, unsigned long long *snap_out = nullptr,
                      uint32_t bin_mask = 0u);

// BVH builder (bvh_build.hip and the bvh_*.hip stage files; refit_bvh4 and the launch_*
// updates: bvh_refit.hip)
struct BvhBuildInput {
    uint32_t num_prims;
    const uint32_t *prim_inst;      // device, global prim -> instance
    const DevInstance *instances;   // device
    const DevMaterial *materials;   // device
    uint32_t object_space;          // 1: BLAS build (vertices untransformed, shading records in primitive order)
};
struct BvhBuildOutput {
    Bvh4Node *nodes4;   // device, collapsed 4-wide quantized tree
    float4 *prims;      // device, kRecF4 * num_records (record slots, pt_scene.h)
    float4 *attrs;      // device, kAttrStride * n shading records (same order)
    uint32_t root_link4;      // link of the root (internal 0 or a leaf)
    uint32_t num_nodes4;
    uint32_t depth4;    // levels of the BVH4 (1 = root only); 0 = not measured (A/B collapse)
    uint32_t num_records = 0; // record slots (leaves on even slots; holes between)
    // first node of each BVH4 level (breadth-first collapse order) and the end; empty when
    // not measured.  Children always lie on a later level (bottom-up refits walk it backwards).
    std::vector<uint32_t> level_start;
};
int build_lbvh(const BvhBuildInput &in, BvhBuildOutput &out, uint32_t leaf_size, hipStream_t s, double *build_ms,
               bool force_lbvh = false);
// build_lbvh whose BVH4 fits the traversal stacks with `reserve` entries to spare:
// PLOC first, the Karras LBVH (depth bounded by the 30-bit Morton codes) when the
// PLOC tree is too deep.  Returns 0, -2 on a HIP error, -3 when no tree fits.
int build_bvh_bounded(const BvhBuildInput &in, BvhBuildOutput &out, uint32_t leaf_size, hipStream_t s,
                      double *build_ms, uint32_t reserve);
void free_lbvh(BvhBuildOutput &out);
// RenderInstanceUpdate without a rebuild: the records of the instances flagged in
// `moved` (device, one byte per instance) get their new world vertices and every BVH4 node
// box is refitted bottom up (topology kept, like the reference's IAS update); nbox: device
// scratch of 6 floats per node.  Needs the breadth-first level order; -1 when unavailable.
// The records of a hidden instance (DevInstance::hidden) get NaN vertices instead, which no
// ray hits and no box includes; a node with nothing visible under it is encoded empty
// (bvh4_quant.h).  records_only: a tree that is one root leaf (no nodes) is accepted too and
// only its records are rewritten (applying the masks to a fresh build).
int refit_bvh4(const BvhBuildInput &in, BvhBuildOutput &out, const uint8_t *moved, float *nbox, hipStream_t s,
               double *ms, bool records_only = false);
// Deformed meshes (pupil_pt_update_shape_vertices).  launch_refit_levels: the bottom-up box
// refit of refit_bvh4 over one tree inside a larger node array -- level_start is relative to
// node_base, the links and nbox (6 floats per node of the array) are absolute.
// launch_refresh_attrs: the shading records of the instances flagged in `moved` (flattened
// BVH) get the object-space positions and normals their shapes hold now;
// launch_refresh_attrs_shape: the same for the n records of one two-level BLAS shape.  The id
// words and texcoords of a record stay.
void launch_refit_levels(Bvh4Node *nodes, const std::vector<uint32_t> &level_start, uint32_t node_base,
                         const float4 *recs, float *nbox, hipStream_t s);
void launch_refresh_attrs(const BvhBuildInput &in, const BvhBuildOutput &out, const uint8_t *moved, hipStream_t s);
void launch_refresh_attrs_shape(float4 *attrs, uint32_t n, const float *positions, const float *normals,
                                const uint32_t *indices, hipStream_t s);
// BVH4 over n >= 2 boxes (6 floats each: lo xyz, hi xyz) with the flattened build's PLOC +
// SAH collapse, one box per leaf: nodes (root 0, parents first) and, for leaf link
// make_leaf(p, 1), the box order[p]; depth = 4-wide levels.  rounds: reinsertion rounds over
// the PLOC tree (< 0: PUPIL_BVH_REINSERT or its default); log (optional): what the pass did
struct ReinsertLog {
    std::vector<double> costs;  // the binary tree's surface-area cost (sum of the internal nodes' half
                                // areas) before the pass and after each round it kept
    int kept = 0;               // rounds committed
    int rejected = 0;           // rounds thrown away because the cost rose (the pass ends there)
};
int build_bvh4_over_boxes(const float *h_boxes, uint32_t n, std::vector<Bvh4Node> &nodes,
                          std::vector<uint32_t> &order, uint32_t *depth, hipStream_t s, int rounds = -1,
                          ReinsertLog *log = nullptr);

}  // namespace pupil
