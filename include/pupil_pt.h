/*
 * pupil_pt.h — C ABI of the MI355X wavefront path tracer (libpupil_pt.so).
 *
 * This is the drop-in boundary for the reference's OptiX path-tracing pass
 * (example/path_tracer).  Every entry point below replaces one piece of the
 * reference's launch surface:
 *
 *   pupil_pt_create          — optix::Pass::InitPipeline + PTPass::SetScene + World::GetIASHandle
 *                              (example/path_tracer/pt_pass.cpp:29-37,107-209;
 *                               framework/world/gas_manager.cpp:61-185, ias_manager.cpp:29-114)
 *   pupil_pt_set_camera      — CameraHelper::GetCudaMemory upload (framework/world/camera.cpp:72-91)
 *   pupil_pt_update_instance — IASManager::UpdateInstance + IAS::Update
 *                              (framework/world/ias_manager.cpp:116-151,187-211); the engine
 *                              refits its BVH over the moved primitives (topology kept, like
 *                              IAS::Update; PUPIL_FLAT_UPDATE / PUPIL_TL_UPDATE=rebuild rebuild it)
 *   pupil_pt_update_emitters — EmitterHelper reset on RenderInstanceUpdate (world/world.cpp:45-54)
 *   pupil_pt_render          — PTPass::OnRun: optixLaunch(w,h,1) + sync, repeated spp times
 *                              with random_seed++ / sample_cnt += accumulate
 *                              (example/path_tracer/pt_pass.cpp:39-57, main.cu:36-194)
 *   pupil_pt_stats           — no reference equivalent (ray / traversal counters)
 *   pupil_pt_destroy         — pass + world GPU resource teardown
 *
 * The scene crosses the boundary as plain arrays (pupil_scene_desc).  The C++
 * host layer (Pupil::world::World, Pupil::resource::Scene, see
 * pupiloptixlab_amd/csrc/host) produces it from mitsuba-style XML exactly as
 * the reference's World::LoadScene does (framework/world/world.cpp:101-139).
 *
 * Error convention (the reference logs then asserts, framework/cuda/util.h:15-26):
 * every function returns PUPIL_OK (0) or a negative PUPIL_ERR_* code; no C++
 * exception crosses this boundary; pupil_last_error() returns the message of
 * the last failure on the calling thread.
 *
 * Threading: an engine may be driven from any thread (the device is set on
 * every call); calls on one engine must not overlap (the reference serialises
 * SetScene and OnRun under System::m_render_system_mutex, system.cpp:93-173).
 */
#pragma once
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PUPIL_OK 0
#define PUPIL_ERR_INVALID -1
#define PUPIL_ERR_HIP -2
#define PUPIL_ERR_OOM -3
#define PUPIL_ERR_IO -4
#define PUPIL_ERR_UNSUPPORTED -5

/* util::ETextureType (framework/util/texture.h:22-26) */
#define PUPIL_TEX_RGB 0u
#define PUPIL_TEX_BITMAP 1u
#define PUPIL_TEX_CHECKERBOARD 2u

/* EMatType order = framework/decl/material_decl.inl:3-11 (Unknown = 0) */
#define PUPIL_MAT_UNKNOWN 0u
#define PUPIL_MAT_DIFFUSE 1u
#define PUPIL_MAT_DIELECTRIC 2u
#define PUPIL_MAT_ROUGH_DIELECTRIC 3u
#define PUPIL_MAT_CONDUCTOR 4u
#define PUPIL_MAT_ROUGH_CONDUCTOR 5u
#define PUPIL_MAT_PLASTIC 6u
#define PUPIL_MAT_ROUGH_PLASTIC 7u
#define PUPIL_MAT_COUNT 8u

/* optix::EEmitterType (framework/render/emitter/types.h:7-14) */
#define PUPIL_EMITTER_NONE 0u
#define PUPIL_EMITTER_TRI_AREA 1u
#define PUPIL_EMITTER_SPHERE 2u
#define PUPIL_EMITTER_CONST_ENV 3u
#define PUPIL_EMITTER_ENV_MAP 4u
/* Delta emitters (types.h:13-14 reserves Point and DistDir; the reference parses `point`,
 * scene.cpp:194-202, and stops at AddEmitter's "TODO case Point", world/emitter.cpp:314).  They
 * reuse pupil_emitter's fields; every field a type does not name is zero.
 *
 * Table order.  Delta emitters travel in pupil_scene_desc::area_emitters after every triangle and
 * sphere emitter: point and spot lights first (the reference's EmitterGroup::points) in the order
 * they were added, then the directional lights (EmitterGroup::directionals) -- the scan order of
 * SelectOneEmiiter (render/emitter.h:110-135).  num_area_emitters counts them; no instance's
 * emitter_offset range reaches them, and no ray can hit one (Eval: pdf 0).
 *
 * Weights and probabilities (EmitterHelper::ComputeProbability, world/emitter.cpp:321-337):
 * weight = 1, as the env has (:300), and select_probability = weight / emitter_num (:334-335) with
 * emitter_num = true area emitters + delta emitters + (env ? 1 : 0) (:331-332).  The areas'
 * weight / area_weight_sum * m_areas.size() (:328) uses the true area count only, then / emitter_num
 * (:333).  Every emissive triangle counts as one emitter: a point light beside a two-triangle lamp
 * is picked one time in three.
 *
 * Sampling (EmitterSampleRecord with is_delta = true): pdf = 1, MIS weight 1 (main.cu:135), the
 * two xi are drawn and ignored.
 *   point:       wi = normalize(center - hit), distance = |center - hit|, radiance = color / distance^2
 *   spot:        the point light times Mitsuba's falloff of a = acos(clamp(dot(-wi, axis), -1, 1)):
 *                1 for a <= beam, 0 for a >= cutoff, (cutoff - a) / (cutoff - beam) between
 *                (beam == cutoff: a hard edge)
 *   directional: wi = -direction, distance = 1e16 (as the constant env), radiance = color */
#define PUPIL_EMITTER_POINT 5u       /* center = position, color = intensity (per steradian) */
#define PUPIL_EMITTER_SPOT 6u        /* + nrm[0] = unit axis, light towards the scene; pos[0][0] = cutoff
                                      * angle, pos[0][1] = beam width (radians, 0 < beam <= cutoff <= pi) */
#define PUPIL_EMITTER_DIRECTIONAL 7u /* nrm[0] = unit direction of travel, color = irradiance on a facing plane */

#define PUPIL_SHAPE_MESH 0u
#define PUPIL_SHAPE_SPHERE 1u

/* cuda::Texture (framework/cuda/texture.h:10-57): rgb colour, checkerboard
 * patches, or an RGBA float bitmap; `transform` is the row-major 4x4 to_uv
 * matrix whose rows 0 and 1 map (u, v, 0, 1). */
typedef struct pupil_texture {
    uint32_t type;
    float c0[3];          /* RGB colour, or checkerboard patch1 */
    float c1[3];          /* checkerboard patch2 */
    float transform[16];  /* row-major */
    uint32_t width, height;
    uint32_t filter;      /* BITMAP: 0 point, 1 bilinear (util::ETextureFilterMode) */
    uint32_t pad;
    const float *rgba;    /* host pointer, width*height*4 floats (BITMAP only) */
} pupil_texture;

/* resource::Material (framework/resource/material.h:60-77) flattened.
 * Texture slot meaning per type (same order as the reference's loaders,
 * framework/resource/material.cpp:26-147):
 *   diffuse:          tex[0]=reflectance
 *   dielectric:       tex[0]=specular_reflectance tex[1]=specular_transmittance
 *   rough_dielectric: tex[0]=alpha tex[1]=specular_reflectance tex[2]=specular_transmittance
 *   conductor:        tex[0]=eta tex[1]=k tex[2]=specular_reflectance
 *   rough_conductor:  tex[0]=alpha tex[1]=eta tex[2]=k tex[3]=specular_reflectance
 *   plastic:          tex[0]=diffuse_reflectance tex[1]=specular_reflectance
 *   rough_plastic:    tex[0]=alpha tex[1]=diffuse_reflectance tex[2]=specular_reflectance */
typedef struct pupil_material {
    uint32_t type;
    uint32_t twosided;
    float int_ior, ext_ior;
    uint32_t nonlinear;
    pupil_texture tex[4];
} pupil_material;

/* resource::Shape (framework/resource/shape.h:34-60): object-space mesh or the
 * unit sphere (centre 0, radius 1; radius/centre live in the instance transform,
 * shape.cpp:106-125,196-197). */
typedef struct pupil_shape {
    uint32_t kind;
    uint32_t num_vertices, num_faces;
    const float *positions;  /* 3 * num_vertices */
    const float *normals;    /* 3 * num_vertices or NULL */
    const float *texcoords;  /* 2 * num_vertices or NULL */
    const uint32_t *indices; /* 3 * num_faces */
} pupil_shape;

/* world::RenderObject + pt::HitGroupData (render_object.cpp:10-38, type.h:35-39).
 * to_world/to_object are the row-major 3x4 instance matrix and its inverse
 * (OptixInstance::transform = Transform.matrix.e[0..11], ias_manager.cpp:171). */
typedef struct pupil_instance {
    uint32_t shape;
    uint32_t material;
    float to_world[12];
    float to_object[12];
    uint32_t flip_normals;
    uint32_t flip_tex_coords;
    int32_t emitter_offset; /* first area-emitter index of this instance, -1 if not emissive */
    uint32_t pad;
} pupil_instance;

/* optix::Emitter (framework/render/emitter.h:13-24 + emitter/{area,sphere,env}.h) */
typedef struct pupil_emitter {
    uint32_t type;
    float weight;
    float select_probability;
    float area;
    pupil_texture radiance;
    float pos[3][3];   /* TriArea: world-space vertices; Spot: pos[0][0] = cutoff, pos[0][1] = beam (radians) */
    float nrm[3][3];   /* TriArea: world-space vertex normals; Spot / Directional: nrm[0] = axis / direction */
    float tex[3][2];   /* TriArea: vertex texcoords */
    float center[3];   /* Sphere centre / env centre; Point / Spot: position */
    float radius;      /* Sphere radius */
    float color[3];    /* ConstEnv colour; Point / Spot: intensity; Directional: irradiance */
    /* EnvMap: radiance.type == BITMAP; the CDF tables are built by the engine */
    float to_world[9]; /* EnvMap: rows of the 3x3 rotation */
    float to_local[9];
    float scale;
} pupil_emitter;

typedef struct pupil_scene_desc {
    uint32_t width, height;    /* film (scene.cpp:86-95) */
    uint32_t max_depth;        /* integrator (scene.cpp:79-82) */
    uint32_t pad0;
    float sample_to_camera[16]; /* optix::Camera (render/camera.h:7-10), row-major */
    float camera_to_world[16];
    uint32_t num_shapes;
    uint32_t num_materials;
    uint32_t num_instances;
    uint32_t num_area_emitters;
    const pupil_shape *shapes;
    const pupil_material *materials;
    const pupil_instance *instances;
    const pupil_emitter *area_emitters; /* EmitterGroup::areas, then points, then directionals
                                         * (PUPIL_EMITTER_POINT above); select_probability filled */
    const pupil_emitter *env;           /* EmitterGroup::env or NULL */
} pupil_scene_desc;

/* Output views: caller-owned device buffers (BufferManager in the reference,
 * framework/system/buffer.h:44-63).  Any pointer except accum may be NULL.
 * If `compact` is non-zero, buffers are indexed by the rank-local pixel index
 * (see pupil_pt_launch.tile_*), otherwise by y*width+x. */
typedef struct pupil_pt_frame {
    void *accum;  /* float4 "pt accum buffer" */
    void *frame;  /* float4 "final result" */
    void *albedo; /* float3 "albedo" */
    void *normal; /* float3 "normal" */
    void *test;   /* float  "test" */
    uint32_t compact;
    uint32_t pad;
} pupil_pt_frame;

/* One call renders `spp` consecutive frames exactly as spp calls of
 * PTPass::OnRun would (pt_pass.cpp:51-56): frame i uses
 * random_seed = random_seed + i and sample_cnt = sample_cnt + i*accumulate.
 * Tile sharding: the image is cut into tile_size x tile_size tiles numbered
 * row-major; this call renders the tiles t with t % tile_world == tile_rank.
 * tile_world = 1 renders the whole image. */
typedef struct pupil_pt_launch {
    uint32_t random_seed;
    uint32_t sample_cnt;
    uint32_t spp;
    uint32_t max_depth; /* 0 = scene value */
    uint32_t accumulate;
    uint32_t tile_size;
    uint32_t tile_rank;
    uint32_t tile_world;
    /* bit 0 (PUPIL_STATS_COUNTERS): count node visits / primitive tests and the
     * reference's shadow-ray count (slower kernels); bit 1 (PUPIL_STATS_TIMING): HIP
     * events around every stage launch for pupil_pt_stats' per-stage times (each
     * event costs ~6 us of stream gap, so production frames leave it off) */
    /* bit 2 (PUPIL_STATS_TRACE_TIMING): events around the traversal launches only (two
     * per launch); their times are summed over every render since pupil_pt_stats last
     * read them, so a timed sequence of renders reports its own traversal time */
    uint32_t collect_stats;
    /* bit 0 (PUPIL_HINT_CONTINUE): the next renders continue this one (random_seed +
     * spp each, same camera, scene, tiling, spp and max_depth), as consecutive
     * PTPass::OnRun calls do (pt_pass.cpp:55-56).  The engine then pipelines frames:
     * this render's launches also start the frames of the renders after it (camera
     * rays and first bounces, up to max_depth frames in flight), so a continued
     * sequence costs one traversal launch per render.  The render's own frame is
     * complete when its work has run, as without the hint; single-spp renders
     * pipeline without it.  Output is bit-identical either way; a render that does not
     * continue drops the frames ahead and renders its own.  (Was a padding word.) */
    uint32_t hints;
} pupil_pt_launch;

#define PUPIL_STATS_COUNTERS 1u
#define PUPIL_STATS_TIMING 2u
#define PUPIL_STATS_TRACE_TIMING 4u
#define PUPIL_HINT_CONTINUE 1u

typedef struct pupil_pt_counters {
    uint64_t primary_rays;
    uint64_t extension_rays;
    uint64_t shadow_rays;
    uint64_t path_samples;
    uint64_t node_visits;    /* only when collect_stats */
    uint64_t prim_tests;     /* only when collect_stats */
    uint64_t bvh_nodes;
    uint64_t bvh_prims;
    double build_ms;
    double last_render_ms;   /* device time of the last pupil_pt_render (events), recorded only for
                              * renders that set collect_stats or request stage times; 0 otherwise */
    double trace_ms;         /* device time of the traversal kernels in the last render (collect_stats
                              * bit 1), or in every PUPIL_STATS_TRACE_TIMING render since the last read */
    double trace_bytes;      /* algorithmic bytes of the traversal kernels (collect_stats) */
    uint64_t trace_launches;
    /* the dominant kernel (closest-hit extend) on its own: device time, launches,
     * and with collect_stats its node visits / primitive tests / algorithmic bytes */
    double extend_ms;
    uint64_t extend_launches;
    uint64_t extend_node_visits;
    uint64_t extend_prim_tests;
    double extend_bytes;
    double shade_ms;         /* device time of the shade stages (all materials) */
    uint64_t two_level;      /* 1: TLAS over instances + per-shape BLAS; 0: one flattened BVH */
    /* collect_stats: loop iterations that reached the shadow test (main.cu:113-123),
     * i.e. the shadow rays the reference traces unconditionally.  shadow_rays counts
     * only the traced ones: the engine (and the oracle) test occlusion only when
     * f * pdf_L != 0 and NoL > 0, which cannot change the radiance because
     * Eval draws no random numbers (optix_material.h:57-62). */
    uint64_t shadow_rays_reference;
    /* BVH4 levels of the acceleration structure (two-level: TLAS + deepest BLAS); at
     * create, trees needing more than the traversal stacks hold are rebuilt with the
     * Karras LBVH or rejected with PUPIL_ERR_UNSUPPORTED */
    uint64_t bvh_depth;
    /* collect_stats: node fetches counted once per distinct node per wave step (the
     * lanes of a wave on the same node share one fetch) -- the gather rate the memory
     * system serves, comparable with independent random gathers */
    uint64_t unique_node_fetches;
    /* ABI 3.  Rays (camera + extension + shadow) traced since the engine was created, by
     * every render: the exact work of a timed sequence of pipelined renders, whose
     * launches also trace rays of the frames ahead of them */
    uint64_t rays_traced_total;
    /* frames started ahead of the next render (pipelined frames) and the ring size */
    uint64_t frames_in_flight;
    uint64_t pipeline_slots;
    /* two-level structure: TLAS nodes placed by an SAH at the last TLAS build -- every node
     * of a GPU-built TLAS (world mode above 64 entries: PLOC + SAH-optimal collapse), or the
     * host builder's binned-SAH splits (entry ranges above 1024, accel_two_level.hip) */
    uint64_t tlas_sah_splits;
    /* collect_stats, persistent traversal kernels: list items the dequeue heads handed
     * out, lanes activated with them, lanes retired, and the launches' list lengths --
     * all four equal when no ray is lost or traced twice */
    uint64_t queue_handed;
    uint64_t queue_activated;
    uint64_t queue_retired;
    uint64_t queue_listed;
    /* ABI 4.  HBM held by the pipelined-frame ring (path state, queues, AOV scratch) and
     * the budget it may grow to (PUPIL_PIPE_GB, default a quarter of the device memory
     * free at pupil_pt_create) */
    uint64_t ring_bytes;
    uint64_t ring_budget_bytes;
    /* acceleration structure refits / rebuilds done for instance updates since creation:
     * one per pupil_pt_update_instances call, however many instances it moves */
    uint64_t accel_refits;
    /* DeviceScene::node_bound, the per-axis max of |o| + 512 s over the live BVH4 nodes
     * (the slab test's rounding bound is taken per ray from it) */
    float node_bound[3];
    uint32_t pad_counters;
    /* ABI 5.  collect_stats, persistent traversal kernels: SIMD efficiency -- node-loop wave
     * iterations and the lanes active in them, leaf-loop wave iterations and their active
     * lanes, refills and the lanes they activated (active lanes / (64 x iterations) = the
     * fraction of a wave's lanes doing useful work in that loop) */
    uint64_t node_loop_iters;
    uint64_t node_loop_lanes;
    uint64_t leaf_loop_iters;
    uint64_t leaf_loop_lanes;
    uint64_t refills;
    uint64_t refill_lanes;
    /* renders run as one persistent launch per frame (renders that start no frame ahead and
     * have at most PUPIL_FRAME_PATHS paths: the moving-camera OnRun, one rank's tiles) */
    uint64_t frame_launches;
    /* ABI 6.  Device time of those one-launch frames (collect_stats bit 1 / 2): the frame kernel
     * traces and shades, so it is kept out of trace_ms */
    double frame_ms;
    /* Terminal extension rays (those feeding the last shade of a path, which can only add the
     * emission of the primitive it hits) resolved by the emitter test instead of a BVH walk,
     * since the engine was created (a running total, like rays_traced_total).  They stay counted
     * in extension_rays and rays_traced_total: those count rays resolved.  It does not grow while the
     * scene has no cull set (environment map, more emissive primitives than the cap, object-mode
     * two-level structure, PUPIL_TERMINAL_CULL=0) and keeps its value when a set goes away: 0
     * only for an engine that never had one.  In the slot that was reserved as coop_dma
     * (always 0 until now): the struct keeps its size and no ABI bump is needed */
    uint64_t terminal_rays_culled;
    uint64_t coop_slots; /* reserved, always 0 */
    /* instances whose visibility mask hides them now (pupil_pt_update_instances_masked);
     * appended without an ABI bump: detect the entry by its symbol */
    uint64_t hidden_instances;
} pupil_pt_counters;

typedef struct pupil_pt pupil_pt;

const char *pupil_last_error(void);
int pupil_abi_version(void);

int pupil_pt_create(const pupil_scene_desc *scene, int device, pupil_pt **out);
int pupil_pt_set_camera(pupil_pt *pt, const float sample_to_camera[16], const float camera_to_world[16]);
/* instance = index into pupil_scene_desc.instances; to_world / to_object row-major 3x4.
 * Must not overlap a render in flight (the reference serialises both under its render mutex). */
int pupil_pt_update_instance(pupil_pt *pt, uint32_t instance, const float to_world[12], const float to_object[12]);
/* n instances at once: ids[k] gets to_world[12k..12k+11] / to_object[12k..]; ONE refit of
 * the acceleration structure covers them all (the reference refits its IAS once per OnRun,
 * however many RenderInstanceUpdate events marked it dirty: pt_pass.cpp:46,216-218).
 * Ordered after every render enqueued so far (stream events, no device-wide sync); returns
 * when the structure is updated.  pupil_pt_update_instance = n = 1. */
int pupil_pt_update_instances(pupil_pt *pt, uint32_t n, const uint32_t *ids, const float *to_world,
                              const float *to_object);
/* IASManager::UpdateInstance (ias_manager.cpp:187-197; SetInstance :174): transform and
 * visibilityMask of n instances, ONE refit.  to_world/to_object NULL = transforms kept;
 * visibility_mask NULL = masks kept (then identical to pupil_pt_update_instances).  Both NULL,
 * or an id out of range: PUPIL_ERR_INVALID.  Every instance is visible at create.
 *
 * RenderObject::visibility_mask (world/render_object.h:16; the inspector's checkbox,
 * gui.cpp:780-784, fires RenderInstanceUpdate).  An instance is visible iff (mask & 0xFF) != 0:
 * every optixTrace of the reference passes mask 255 (main.cu:77-82,158-163, emitter.h:95-98),
 * so rays carry no mask of their own.  A hidden instance is hit by no ray: camera, extension
 * and shadow rays, pupil_pt_trace_rays, and pupil_pt_motion_vectors, which reports the flow
 * of what lies behind it.  The structure is refitted, not rebuilt, and showing the instance
 * again restores it bit for bit.
 *
 * The emitter table does NOT change: the reference resets its emitters only on
 * RenderInstanceTransform (world/world.cpp:45-54), and a visibility change goes straight to
 * RenderInstanceUpdate.  A hidden emissive instance is therefore still picked by next-event
 * estimation, and its own hidden geometry does not block the shadow ray, so it still lights
 * the scene; camera and BSDF-sampled rays never see it.
 *
 * Instances are added and removed with pupil_pt_set_instances below, which replaces the table as
 * a whole (the reference's path tracer never binds RenderInstanceRemove, and its SBT offsets go
 * stale after a removal). */
int pupil_pt_update_instances_masked(pupil_pt *pt, uint32_t n, const uint32_t *ids,
                                     const float *to_world, const float *to_object,
                                     const uint32_t *visibility_mask);
/* Instances moved from device memory: the update above for callers whose transforms are produced
 * on the GPU (a rigid-body step, a particle system, a pose optimiser).  No matrix passes through
 * the host on its way in, and in the flattened BVH and in world-mode two-level the kernel
 * launches and stream synchronisations of one call do not depend on n.  No ABI bump: detect the
 * symbols.
 *
 * pupil_pt_update_instances_device: list entry k moves instance ids_device[k] (NULL: instance k)
 * to to_world_device[12k..12k+11], row-major 3x4.  ids must be distinct; with a repeated id it
 * is unspecified which entry wins, but every write stays in bounds.
 *   Ordering, caller's stream: the three arrays are read in place, after the work enqueued so far
 *     on hip_stream (a hipStream_t, NULL = the null stream), by an event as PUPIL_VERTS_DEVICE
 *     does; no device-wide sync.  They must stay valid and unchanged until the call returns.
 *   Ordering, engine's stream: after every render, flow pass, ray query and radiance call enqueued
 *     so far.  Frames in flight are dropped.  Returns once the structure is updated;
 *     accel_refits + 1, build_ms = the call's time.
 *   Result: the next render, query and flow pass equal those of an engine created on a world with
 *     these transforms, bit for bit.
 *   to_object_device NULL: the engine inverts on the device.  Each to_world is completed with the
 *     row (0, 0, 0, 1) and inverted in double by the cofactor expansion the world uses (the same
 *     terms in the same order, det == 0 gives all zeros, 1.0 / det, one rounding to float): bit
 *     for bit the to_object pupil_world_get_desc produces for an affine matrix.  Otherwise n x 12
 *     floats that must be that inverse, as for the host entry.
 *   Two-level box margins are recomputed on the device for every moved mesh instance, in the
 *     host's order of operations.
 *   Visibility does not change: a hidden instance takes the new transform and stays hidden, and
 *     pupil_pt_update_instances_masked shows it later at the new transform.
 *   An id >= num_instances writes nothing and reads nothing out of bounds: the kernel skips it
 *     and counts it; the call returns PUPIL_OK with a message in pupil_last_error(), and the
 *     running total is `skipped` of pupil_pt_instances_device_info.
 *   n == 0: PUPIL_OK, nothing enqueued.  PUPIL_ERR_INVALID, before anything is enqueued: pt or
 *     to_world_device NULL, n > num_instances, a pointer not 4-byte aligned.
 *   Host mirror: the call reads back 4n bytes of ids before it changes anything, and after the
 *     kernels one contiguous staging block of the moved instances' to_world, to_object, margins
 *     and world boxes; no other transfer depends on n.  Every later host-path call sees the move.
 *   Emissive instances: with the device-side emitter table off (pupil_pt_enable_device_emitters),
 *     a moved id that is emissive returns PUPIL_ERR_UNSUPPORTED before anything changes, as
 *     PUPIL_VERTS_DEVICE does on an emissive shape; with it on, the table is rebuilt before the
 *     call returns.
 *   Two-level object mode (PUPIL_TL_MODE=object) rebuilds its TLAS on the host on every update:
 *     there the call is correct and no more, it goes through the host path after the readback.
 *
 * pupil_pt_get_instance_transforms: the engine's host mirror of instances [first, first + n),
 * whichever path wrote it, 12 floats each; either out pointer may be NULL.  PUPIL_ERR_INVALID:
 * pt NULL or the range out of bounds.
 *
 * pupil_pt_instances_device_info: successful device calls and instances moved by them since
 * create; the skipped ids; the kernel launches and hipStreamSynchronize / hipEventSynchronize
 * calls of the LAST call, counted by the host code where it makes them; the host's time around
 * it.  Any out pointer may be NULL.
 *
 * pupil_debug_invert3x4: the inverse above on the host, from the text the kernel compiles; no GPU
 * is touched.  PUPIL_ERR_INVALID: a NULL argument. */
int pupil_pt_update_instances_device(pupil_pt *pt, uint32_t n, const uint32_t *ids_device,
                                     const void *to_world_device, const void *to_object_device, void *hip_stream);
int pupil_pt_get_instance_transforms(pupil_pt *pt, uint32_t first, uint32_t n, float *to_world, float *to_object);
int pupil_pt_instances_device_info(pupil_pt *pt, uint64_t *updates, uint64_t *instances, uint64_t *skipped,
                                   uint32_t *last_launches, uint32_t *last_syncs, double *last_ms);
int pupil_debug_invert3x4(const float m[12], float out[12]);
/* Kernel launches and stream / event synchronisations of the last instance update, by the host
 * entries or the device entry, counted by the host code where it makes them, up to the TLAS refit
 * (a TLAS or BVH that is built anew adds its own, uncounted).  For tools that compare the two
 * paths; either out pointer may be NULL. */
int pupil_debug_update_counts(pupil_pt *pt, uint32_t *launches, uint32_t *syncs);
/* Deformable meshes: new vertices for mesh shape `shape` (index into pupil_scene_desc.shapes),
 * the geometry-AS counterpart (OPTIX_BUILD_OPERATION_UPDATE) of the instance update above.
 * positions: 3 * num_vertices floats as at create; normals: the same count, or NULL = the
 * normals stay.  Vertex count, indices and texcoords never change.  Every instance of the
 * shape follows with ONE refit (accel_refits + 1, build_ms = the call's time): records, node
 * boxes and shading records are rewritten in place, hidden instances stay hidden and show the
 * new vertices when shown.  The next render equals, bit for bit, a render of an engine created
 * on the deformed mesh.
 *   PUPIL_VERTS_DEVICE   positions / normals are device pointers: the copy (device to device,
 *                        into the engine's own arrays) is ordered after the work enqueued so far
 *                        on hip_stream (a hipStream_t, NULL = the null stream) by an event; the
 *                        vertices never pass through the host.  hip_stream is ignored without it.
 *   PUPIL_VERTS_REBUILD  rebuild the whole acceleration structure with the builders of
 *                        pupil_pt_create instead of refitting: for deformations so large that
 *                        the refitted tree traces badly.  There is no per-BLAS rebuild.
 * PUPIL_ERR_INVALID: pt or positions NULL, shape out of range or a PUPIL_SHAPE_SPHERE, normals
 * for a shape created without them, unknown flags.  If an instance of the shape is emissive
 * (emitter_offset >= 0) its area emitters must follow through pupil_pt_update_emitters, as after
 * a transform (pupil_world_set_mesh_vertices + pupil_world_get_desc produce them); without the
 * device-side emitter table the engine cannot derive that table from device vertices, so
 * PUPIL_VERTS_DEVICE on such a shape returns PUPIL_ERR_UNSUPPORTED.  That applies only while
 * pupil_pt_enable_device_emitters (below) is off: with it on, this call rebuilds the table itself
 * after the refit, from host or device vertices alike, and PUPIL_VERTS_DEVICE is accepted.  Ordered after every render enqueued so far; frames in flight are
 * dropped; returns once the structure is updated.  accel_refits counts successful calls only.  If
 * the call fails after the argument checks (PUPIL_ERR_HIP / _OOM / _UNSUPPORTED from the refit or
 * the builders), the engine's vertex arrays already hold the new vertices while the acceleration
 * structure still bounds the old ones: do not render until a later call for this shape succeeds
 * (PUPIL_VERTS_REBUILD is the one that depends on nothing left behind).  pupil_pt_motion_vectors
 * sees the vertex motion of an update that pupil_pt_snapshot_shape_vertices preceded (below);
 * without a snapshot it reports camera and rigid instance motion only.  No ABI bump: detect the
 * symbol. */
#define PUPIL_VERTS_DEVICE 1u
#define PUPIL_VERTS_REBUILD 2u
int pupil_pt_update_shape_vertices(pupil_pt *pt, uint32_t shape, const float *positions, const float *normals,
                                   uint32_t flags, void *hip_stream);
/* Flow for deforming meshes.  pupil_pt_snapshot_shape_vertices keeps the vertices mesh shape
 * `shape` has NOW as its "previous" vertices, for the flow of the update that follows: call it
 * before pupil_pt_update_shape_vertices.  While a shape holds a snapshot, pupil_pt_motion_vectors
 * carries every hit on an instance of it back by the displacement of the hit point (barycentric
 * blend of the three vertices' now-minus-snapshot displacements) before the previous instance
 * transform and camera go on; hits on other shapes, and on triangles whose vertices did not move,
 * get bit for bit the flow they get without a snapshot.  The copy is device to device from the
 * engine's own array into a per-shape array allocated on first use, on the engine's stream after
 * every render and flow pass enqueued so far; every later flow pass is ordered after it.  A second
 * call for the shape overwrites the snapshot.  Works for emissive shapes, hidden instances and
 * shapes no instance shows, and survives PUPIL_VERTS_REBUILD (vertex count, indices and global
 * primitive ids never change).  Drops no frame in flight, is no refit (accel_refits and build_ms
 * stay) and changes no pixel of any render.  PUPIL_ERR_INVALID: pt NULL, shape out of range or a
 * PUPIL_SHAPE_SPHERE; PUPIL_ERR_OOM: the 12 B x num_vertices array could not be allocated (the
 * shape then holds no snapshot).
 * pupil_pt_clear_vertex_snapshots forgets every snapshot (the allocations are kept): flow is
 * camera and rigid instance motion again, by the same kernel with the same arguments as before
 * the first snapshot.  PUPIL_ERR_INVALID: pt NULL.  No ABI bump: detect the symbols. */
int pupil_pt_snapshot_shape_vertices(pupil_pt *pt, uint32_t shape);
int pupil_pt_clear_vertex_snapshots(pupil_pt *pt);
/* New topology for mesh shape `shape`, in place: *mesh is a PUPIL_SHAPE_MESH with its own
 * num_vertices, num_faces, positions, indices and optional normals / texcoords, each present or
 * absent whatever the old mesh had.  The arrays are copied into arrays the engine owns.  Every
 * instance of the shape shows the new mesh (a hidden one when it is shown again), and the next
 * render, ray query, radiance call and flow pass equal, bit for bit, those of an engine created on
 * the same scene description.  Everything that hangs off the primitive count follows: the
 * instances' prim_offset and array pointers, the primitive -> instance table and its lookup
 * tables (filled on the device, pt_replace.hip), the cull set, the query scratch; the whole
 * acceleration structure is rebuilt with the builders of pupil_pt_create, as PUPIL_VERTS_REBUILD
 * does (there is no rebuild of one BLAS inside the two-level arrays).  accel_refits + 1; bvh_prims,
 * bvh_nodes and bvh_depth follow; build_ms = the call's time.  The shape's vertex snapshot is
 * dropped: the next flow pass treats it as having none.
 *   flags: 0, or PUPIL_VERTS_DEVICE = all the pointers of *mesh are device pointers, read in
 *   place after the work enqueued so far on hip_stream (a hipStream_t, NULL = the null stream) by
 *   an event; no vertex or index passes through the host (the index check is a reduction on the
 *   device, 4 bytes come back).  hip_stream is ignored without it.
 * Ordered after every render enqueued so far; frames in flight are dropped; returns once the
 * structure is published.
 * A failed call leaves the engine as it was (the next render equals the render before the call):
 * everything is validated, allocated and built aside -- new shape arrays, tables, instance table
 * and structure -- and swapped in together once the structure is complete.
 * PUPIL_ERR_INVALID: NULL pt / mesh / positions / indices, shape out of range or a
 * PUPIL_SHAPE_SPHERE, mesh->kind not PUPIL_SHAPE_MESH, num_faces or num_vertices 0, unknown flags,
 * an index >= num_vertices.  PUPIL_ERR_UNSUPPORTED: an instance of the shape is emissive
 * (emitter_offset >= 0) while the device-side emitter table is off -- its emitter count would
 * change and with it every later instance's emitter_offset, which only the device-side mode
 * follows (below) -- or a limit of the builders (2^31
 * primitives, 2^27 flattened primitives, the 28-bit leaf links, the node limit, the traversal
 * stacks).  PUPIL_ERR_OOM: the new arrays could not be allocated.
 * Emissive shapes, with the device-side emitter table on (pupil_pt_enable_device_emitters): the
 * shape's emissive instances get one emitter per new face.  The engine assigns every emissive
 * instance its emitter_offset anew in instance order, as pupil_world_get_desc does, keeps each
 * one's radiance (bitmap texels are moved into the new table, not uploaded again) and select
 * weight, and rebuilds the area-emitter table at its new size on the device (pt_emitters.hip: the
 * records with type, radiance and texcoords, then geometry, select probabilities, CDF and guide)
 * inside the same transaction: the table is staged aside and adopted in the swap.  Afterwards the
 * table equals, bit for bit, that of an engine created on the world's description of the new
 * scene (pupil_world_replace_mesh with PUPIL_WORLD_MESH_EMISSIVE_OK keeps the world in step).
 * Delta lights keep their records under their new indices; the env emitter carries over.
 * pupil_pt_replace_info: successful calls since create and the host clock around the last one;
 * either out pointer may be NULL.  No ABI bump: detect the symbols. */
int pupil_pt_replace_shape_mesh(pupil_pt *pt, uint32_t shape, const pupil_shape *mesh, uint32_t flags,
                                void *hip_stream);
int pupil_pt_replace_info(pupil_pt *pt, uint64_t *replacements, double *last_ms);
/* The instance table replaced as a whole: instances added, removed, or bound to another shape or
 * material slot of the engine, in place.  The table becomes instances[0..n); shapes, materials,
 * emitters, camera and film stay.  shape and material index the engine's existing ones.  After
 * the call the next render, pupil_pt_query_rays / _query_camera, pupil_pt_radiance_rays and
 * pupil_pt_motion_vectors equal, bit for bit, those of an engine freshly created on the scene
 * whose instance list is the new one, with the same masks applied; everything sized or indexed by
 * the instance or primitive count follows (the primitive tables, the material bins, the cull set,
 * the query, flow and device-move scratch).  Vertex snapshots of shapes stay.
 * visibility_mask: n masks as in pupil_pt_update_instances_masked, or NULL: all visible.
 * flags == 0: transforms from instances[k].to_world / to_object; to_world_device must be NULL.
 * PUPIL_INSTANCES_DEVICE: the transforms are the n x 12 floats at to_world_device, read in place
 * behind hip_stream (an event, as PUPIL_VERTS_DEVICE; no device-wide sync) and inverted on the
 * device as pupil_world_get_desc inverts them; the host structs' to_world / to_object are ignored,
 * their shape, material, flips and emitter_offset are used.  The engine's host mirror is filled
 * from one readback of the new table.  On the flattened BVH nothing else grows with n beyond the
 * upload of the bindings.  In the two-level modes the structure's per-instance stage then fills
 * the instances' BLAS fields, margins and boxes in the mirror and uploads the table once more
 * (224 bytes per instance), as pupil_pt_create does.
 * Ordered after every render, query, radiance call and flow pass enqueued so far; frames in
 * flight are dropped; returns once the structure is published; accel_refits + 1.
 * Transactional: everything is validated, allocated and built aside, then swapped in.  A failed
 * call leaves the engine untouched.
 * Structure: the flattened BVH is built once.  Two-level world mode, when the set of mesh shapes
 * shown by at least one instance is unchanged: only the per-instance stage runs (world records,
 * world BLAS copies, boxes, TLAS) -- no BLAS is built.  When that set changes (a shape gains its
 * first instance or loses its last), and in two-level object mode (PUPIL_TL_MODE=object, whose
 * BLAS links depend on the instance count), the whole structure is built.
 * Emissive instances: the emitter table is not touched, so the emissive instances of the new table
 * must be the old ones in the same relative order, each with its shape, material, flips and
 * emitter_offset, and -- unless the device-side emitter table is on
 * (pupil_pt_enable_device_emitters) -- its transform bit for bit.  Their indices may change; with
 * the device-side table on it is refreshed before the call returns.  Anything else (an emissive
 * instance added, removed, reordered, rebound, or moved with the device-side table off) returns
 * PUPIL_ERR_UNSUPPORTED before anything changes; pupil_pt_set_instances_emitters (below) lifts
 * this with the device-side table on.
 * PUPIL_ERR_INVALID: NULL pt or instances, n == 0 (as pupil_pt_create on a scene without
 * instances), a shape, material or emitter range out of range, unknown flags, the device pointer
 * missing or present without the flag, or not 4-byte aligned.  PUPIL_ERR_UNSUPPORTED: the
 * builders' limits as pupil_pt_replace_shape_mesh lists them.  PUPIL_ERR_OOM: an allocation failed.
 * pupil_pt_set_instances_info: successful calls since create; of the last one the BLAS builds it
 * ran, whether the whole structure was built (flattened: always 1) and the host clock around it;
 * any out pointer may be NULL.  No ABI bump: detect the symbols. */
#define PUPIL_INSTANCES_DEVICE 1u
int pupil_pt_set_instances(pupil_pt *pt, uint32_t n, const pupil_instance *instances,
                           const uint32_t *visibility_mask /* n, or NULL = all visible */,
                           const void *to_world_device /* n x 12 floats, or NULL */, uint32_t flags,
                           void *hip_stream);
int pupil_pt_set_instances_info(pupil_pt *pt, uint64_t *calls, uint32_t *last_blas_builds,
                                uint32_t *last_whole_rebuild, double *last_ms);
/* pupil_pt_set_instances with a free emissive set, for the device-side emitter table
 * (pupil_pt_enable_device_emitters; PUPIL_ERR_UNSUPPORTED while it is off).  The instance list is
 * scene->instances[0..num_instances); `material` names the engine's slots, as above.  Emissive
 * instances may be added, removed, reordered, rebound to another shape or radiance, and moved:
 * the area-emitter table is rebuilt at its new size on the device, inside the same transaction
 * (staged aside, adopted with the instance table and the structure), and afterwards equals, bit
 * for bit, that of an engine created on the scene.  Of scene->area_emitters the call reads, per
 * emissive instance, the radiance of the first record of its range (descriptor, host texels of a
 * bitmap -- uploaded once per instance -- and the select weight, as
 * pupil_pt_enable_device_emitters reads it) and the delta-light records behind the ranges, whole;
 * geometry, area, weight and select_probability of the triangle and sphere emitters are not read:
 * they are derived on the device, with PUPIL_INSTANCES_DEVICE from transforms that never reach
 * the host.  Everything else is pupil_pt_set_instances: flags, masks, ordering, accel_refits + 1,
 * no BLAS build in two-level world mode while the set of shown shapes stays, and, with an
 * unchanged emissive set, the same engine state.
 * PUPIL_ERR_INVALID, before anything changes: a NULL pt, scene or instance list; emitter ranges
 * that do not follow each other in instance order or are not the shape's face count (a sphere: 1)
 * of the matching type; num_area_emitters that is not the ranges plus the delta lights; a table
 * out of the order areas, point / spot, directional; an env emitter present in one of scene and
 * engine only (the env changes through pupil_pt_update_emitters); everything
 * pupil_pt_set_instances rejects.
 * pupil_pt_emitter_resize_info: tables rebuilt at a new size since create (by this call and by
 * pupil_pt_replace_shape_mesh on an emissive shape; successes only), the triangle and sphere
 * emitters of the last one and the host clock around its call; any out pointer may be NULL.  A
 * resize that leaves a triangle or sphere emitter in the table also counts as a rebuild in
 * pupil_pt_device_emitters_info, as the refresh of pupil_pt_set_instances does.
 * Out of scope: the mode-off path (both calls refuse as before), a single BLAS rebuilt alone, area
 * radiance texels from device memory.  No ABI bump: detect the symbols. */
int pupil_pt_set_instances_emitters(pupil_pt *pt, const pupil_scene_desc *scene,
                                    const uint32_t *visibility_mask /* num_instances, or NULL */,
                                    const void *to_world_device /* num_instances x 12 floats, or NULL */,
                                    uint32_t flags, void *hip_stream);
int pupil_pt_emitter_resize_info(pupil_pt *pt, uint64_t *resizes, uint32_t *last_true_areas, double *last_ms);
/* The shape of the emitter table the engine holds now: its entries (delta lights included), the
 * triangle and sphere emitters in front, and whether there is an env emitter -- what a caller
 * compares a scene description with before pupil_pt_set_instances_emitters.  Any out pointer may
 * be NULL.  No ABI bump: detect the symbol. */
int pupil_pt_emitter_table_info(pupil_pt *pt, uint32_t *emitters, uint32_t *true_areas, uint32_t *has_env);
/* Shadow rays of the last render with PUPIL_STATS_COUNTERS (zeros otherwise), beside
 * pupil_pt_counters: those that found an occluder and the node visits they took; the others took
 * node_visits - extend_node_visits minus these.  overlap_order: 1 when the engine's any-hit rays
 * (shadow rays, PUPIL_QUERY_ANY_HIT queries) descend the child with the longest overlap first, 0
 * when PUPIL_SHADOW_ORDER=0 at create keeps them near to far; results do not depend on it.  Any
 * out pointer may be NULL.  No ABI bump: detect the symbol. */
int pupil_pt_shadow_info(pupil_pt *pt, uint64_t *occluded_rays, uint64_t *occluded_visits, uint32_t *overlap_order);
/* (tests) the primitive -> instance tables as the device holds them: the primitive count, the
 * guide's shift and its entries ((num_prims - 1 >> shift) + 2), and, each unless NULL, prim_inst
 * (num_prims words), inst_first (num_instances + 1) and inst_guide (guide_entries). */
int pupil_debug_read_prim_tables(pupil_pt *pt, uint32_t *num_prims, uint32_t *guide_shift, uint32_t *guide_entries,
                                 uint32_t *prim_inst, uint32_t *inst_first, uint32_t *inst_guide);
/* replaces the area-emitter table (delta lights included), selection CDF and env emitter (after an
 * emissive instance moved, or a point, spot or directional light was moved, recoloured, added or
 * removed); rewritten in place on the engine's stream when their shapes -- the emitter count, each
 * entry's type, the env -- are unchanged.  PUPIL_ERR_INVALID for a table that is not in the order
 * areas, point / spot lights, directional lights. */
int pupil_pt_update_emitters(pupil_pt *pt, const pupil_scene_desc *scene);
/* Engine-owned area-emitter table.  The engine holds everything the table is derived from
 * (vertices, indices, normals, to_world / to_object, each instance's emitter_offset), so with
 * this mode on it rebuilds the table on the device instead of taking it from the host.  Opt-in;
 * with the mode off every call behaves as it did before the mode existed.  No ABI bump: detect
 * the symbols.
 *
 * pupil_pt_enable_device_emitters: `scene` is the description the engine renders now (the one of
 * pupil_pt_create, or the latest given to pupil_pt_update_emitters); NULL switches the mode off.
 * From it the engine takes one value per emissive instance, the select weight of its radiance
 * texture (the reference's GetWeight, world/emitter.cpp:73-101; a bitmap is summed on the host,
 * now, from the scene's texel pointer), builds its bookkeeping (per emitter its instance, per
 * instance the weight) and runs one rebuild.  After it the table equals the one `scene` describes
 * bit for bit, provided `scene` was produced by pupil_world_get_desc: a caller who filled
 * select_probability by another rule than the reference's (weight = select weight x area,
 * normalised over the area emitters, then divided by the emitter count with the env) gets the
 * reference's rule from then on.  PUPIL_ERR_INVALID, with the mode and the table unchanged: pt
 * NULL; the scene's instance count, area-emitter count or any emitter_offset differs from the
 * engine's; an emissive mesh instance's emitter range is not its face count (a sphere's: one).
 *
 * While the mode is on, pupil_pt_update_shape_vertices on a shape with an emissive instance (host
 * vertices, PUPIL_VERTS_DEVICE, either with PUPIL_VERTS_REBUILD) and
 * pupil_pt_update_instances[_masked] that give an emissive instance a transform rebuild the table
 * before they return; a call that changes visibility masks only leaves it alone (a hidden
 * emitter stays in the table, above).  pupil_pt_update_emitters still replaces everything, the
 * env included; the mode stays on if the new scene still matches the engine's counts and offsets
 * (its radiance weights are taken anew), otherwise it goes off and pupil_last_error() says so
 * while the call returns PUPIL_OK.
 *
 * The rebuild rewrites, in place, pos / nrm / area / select_probability of every triangle
 * emitter (center / radius / area / select_probability of a sphere), the selection CDF and its
 * guide table, and nothing else: counts, guide_bits, radiance textures, texcoords and the env
 * emitter (whose select probability depends on the emitter count only) cannot change.  Delta
 * lights may be present: the ranges cover the triangle and sphere emitters in front of them, the
 * scene's delta entries must be the engine's type for type, and the rebuild leaves a delta entry
 * untouched but for its select_probability (1 / emitter count, as before) and its CDF entry.  Every
 * stage restates the host's operations in the host's order (pt_emitters.hip), so the result is
 * bit-identical to pupil_world_get_desc + pupil_pt_update_emitters for the same vertices and
 * transforms; to_object must be the inverse the world computes.  Precondition, as for the host
 * path's guide table: the weights are finite and >= 0, so the CDF is non-decreasing.
 *
 * pupil_pt_refresh_emitters runs the rebuild now, on the engine's stream after every render
 * enqueued so far, drops frames in flight and returns when the table is written
 * (PUPIL_ERR_INVALID with the mode off): for callers who write the engine's arrays by other
 * means, and for timing.  pupil_pt_device_emitters_info: whether the mode is on, rebuilds since
 * create, and the host's time around the last one (as build_ms is taken); any out pointer may be
 * NULL. */
int pupil_pt_enable_device_emitters(pupil_pt *pt, const pupil_scene_desc *scene);
int pupil_pt_refresh_emitters(pupil_pt *pt);
int pupil_pt_device_emitters_info(pupil_pt *pt, uint32_t *enabled, uint64_t *refreshes, double *last_ms);
/* Materials and textures updated in place.  The reference fixes them at SetScene
 * (optix_material.cpp runs once per scene load, and its inspector edits no material): there is no
 * reference event behind these entries.  No ABI bump: detect the symbols.
 *
 * pupil_pt_update_materials replaces materials ids[k] (indices into pupil_scene_desc.materials)
 * by materials[k]; an id named twice takes its last entry.  Any field may change: type, twosided,
 * the IORs, nonlinear and all four texture slots, a slot's kind and a bitmap's size included.  The
 * host precompute is that of pupil_pt_create, so the next render equals, bit for bit, a render of
 * an engine created with the new materials.  Everything is checked before anything changes
 * (PUPIL_ERR_INVALID: pt NULL, ids / materials NULL with n > 0, an id out of range, an unknown
 * texture type, a bitmap without texels or with a zero side; PUPIL_ERR_OOM: new texels could not
 * be allocated): a refused call leaves the engine rendering exactly as before.  Ordered on the
 * engine's stream after every render enqueued so far; frames in flight are dropped; returns once
 * the copies have run.  Only the named DevMaterial entries are written.  A bitmap slot whose
 * width * height is unchanged keeps its allocation; otherwise new texels are allocated and the
 * old ones freed before the call returns, so repeated updates hold no more memory than the
 * materials in use.  When a type changes, the material bin of every instance that uses the
 * material follows (instance table and record slots), and with it the shading schedule
 * (PUPIL_SHADE_LIST is honoured as at create).  No box or link of the acceleration structure
 * depends on a material: it is not refitted and accel_refits stays.  Emitter radiance is not a
 * material: pupil_pt_update_emitters changes it.
 *
 * pupil_pt_update_texture_device replaces the texels of bitmap slot `slot` (0..3) of `material`
 * from device memory: width * height float4, row-major, the layout of pupil_texture::rgba.  The
 * slot must already be a bitmap of exactly width x height (PUPIL_ERR_INVALID otherwise, the
 * message says to set the size with pupil_pt_update_materials first; also for pt or rgba_device
 * NULL, a material out of range, slot > 3).  As with PUPIL_VERTS_DEVICE the copy, device to
 * device into the engine's own texels, is ordered after the work enqueued so far on hip_stream
 * (a hipStream_t, NULL = the null stream) by an event: no device-wide sync, and the texels never
 * pass through the host.  For a plastic or rough_plastic whose diffuse or specular reflectance
 * slot is updated, specular_sampling_weight is recomputed on the device from the texels the two
 * slots then hold, in the host's summation order, so it is bit for bit the weight
 * pupil_pt_create would compute from them (pt_materials.hip); one serial pass over the bitmap.
 * Frames in flight are dropped; returns once the engine's stream has passed the copy.
 *
 * pupil_pt_material_info: successful calls of either entry since create, and the host's time
 * around the last one (as build_ms is taken); either out pointer may be NULL. */
int pupil_pt_update_materials(pupil_pt *pt, uint32_t n, const uint32_t *ids, const pupil_material *materials);
int pupil_pt_update_texture_device(pupil_pt *pt, uint32_t material, uint32_t slot, const void *rgba_device,
                                   uint32_t width, uint32_t height, void *hip_stream);
int pupil_pt_material_info(pupil_pt *pt, uint64_t *updates, double *last_ms);
/* The env map updated in place, its texels from device memory.  The reference builds the map's
 * tables once per scene load (BuildEnvMapCdfTable, world/emitter.cpp:107-149): there is no
 * reference event behind these entries.  No ABI bump: detect the symbols.
 *
 * pupil_pt_update_env_device replaces the texels of the env map: width * height float4, row-major,
 * the layout of pupil_texture::rgba.  The engine's env emitter must be a PUPIL_EMITTER_ENV_MAP of
 * exactly width x height.  PUPIL_ERR_INVALID otherwise -- no env emitter, a constant env, another
 * size (the message says to set the size with pupil_pt_update_emitters first), pt or rgba_device
 * NULL -- and PUPIL_ERR_OOM when the first call cannot allocate its scratch (height floats, owned
 * by the engine until pupil_pt_destroy; no later call of the same size allocates).  Everything is
 * checked before anything changes: a refused call leaves the engine rendering exactly as before.
 * As with pupil_pt_update_texture_device the copy, device to device into the engine's own texels,
 * is ordered after the work enqueued so far on hip_stream (a hipStream_t, NULL = the null stream)
 * by an event, with no device-wide sync, and after every render enqueued so far; frames in flight
 * are dropped.  The tables col_cdf, row_cdf and the normalization are then rebuilt on the engine's
 * stream, in place, in the host's summation order (pt_envmap.hip), so they are bit for bit what
 * pupil_pt_create would derive from the same texels; row_weight depends on the height only and
 * stays.  Nothing else of the emitter is written.  Returns once the engine's stream has passed
 * the kernels.  Precondition, as for the host path: the texels are finite and every row's
 * luminance sum is > 0 (the host's tables hold NaN otherwise, whose bits the device need not
 * match).
 *
 * pupil_pt_update_env_params rewrites scale, to_world and to_local (row-major 3x3; to_local must
 * be the inverse the world computes, pupil_world_invert3x3) of the device's env map, whether its
 * texels came from the host or the device: no table is built and no texel copied.  Ordered after
 * every render enqueued so far; frames in flight are dropped; returns once the copies have run.
 * PUPIL_ERR_INVALID: pt or a matrix NULL, no env map.
 *
 * After either call the engine's env no longer equals the pupil_emitter it was created from.  A
 * later pupil_pt_update_emitters therefore never takes its in-place path on the strength of an
 * unchanged env: it rebuilds the env from the scene it is given (host texels, host tables), even
 * when that scene's env is byte for byte the one given before.
 *
 * pupil_pt_env_info: successful calls of the two entries since create, and the host's time around
 * the last one (as build_ms is taken); either out pointer may be NULL. */
int pupil_pt_update_env_device(pupil_pt *pt, const void *rgba_device, uint32_t width, uint32_t height,
                               void *hip_stream);
int pupil_pt_update_env_params(pupil_pt *pt, float scale, const float to_world[9], const float to_local[9]);
int pupil_pt_env_info(pupil_pt *pt, uint64_t *updates, double *last_ms);
/* Asynchronous on hip_stream (a hipStream_t; NULL = the default null stream): the
 * output buffers are complete once work later enqueued on that stream runs.  Exception:
 * with max_depth > 64 the call synchronises hip_stream every 16 bounces to read the list
 * lengths back and stops once no path is left. */
int pupil_pt_render(pupil_pt *pt, const pupil_pt_frame *out, const pupil_pt_launch *launch, void *hip_stream);
int pupil_pt_stats(pupil_pt *pt, pupil_pt_counters *out);
int pupil_pt_local_pixels(uint32_t width, uint32_t height, uint32_t tile_size, uint32_t tile_rank,
                          uint32_t tile_world, uint32_t *out_pixels, uint32_t *inout_count);
void pupil_pt_destroy(pupil_pt *pt);
/* ABI 7.  Screen-space flow for OptixDenoiserGuideLayer::flow (denoiser.cpp:207): for every pixel
 * i = y*width + x, out[2i..2i+1] = (cur_x - prev_x, cur_y - prev_y) in pixels, in the index
 * space of the frame buffers (compact = rank-local pixel order, as pupil_pt_frame.compact),
 * of the surface point seen through the pixel centre now, against where that point was
 * under the previous camera and the previous instance transforms.  An environment miss is the
 * point at infinity along the ray; a point at or behind the previous camera plane has no
 * previous pixel and gets (NaN, NaN).  Flow is that of the primary hit (nothing is followed
 * through reflections or refractions).  Rigid instance motion is covered through prev_to_world,
 * vertex motion of the shapes that hold a snapshot (pupil_pt_snapshot_shape_vertices) through
 * the snapshots: p' = prev_to_world (to_object p - d), d = the object-space displacement of the
 * hit point since the snapshot.
 * prev_to_world: num_instances * 12 floats (row-major 3x4, host) or NULL = no instance moved.
 * Asynchronous on hip_stream, ordered after every render enqueued so far; the current camera
 * and instance transforms are the engine's (pupil_pt_set_camera / pupil_pt_update_instances).
 * Adds nothing to the ray counters of pupil_pt_stats. */
int pupil_pt_motion_vectors(pupil_pt *pt, const float prev_sample_to_camera[16],
                            const float prev_camera_to_world[16], const float *prev_to_world,
                            void *out_flow /* device float2 per pixel */, uint32_t compact,
                            uint32_t tile_size, uint32_t tile_rank, uint32_t tile_world,
                            void *hip_stream);

/* Ray queries from device memory: what does this ray hit.  The engine's production traversal over
 * a ray list that is already on the device, and the hits resolved into ids and hit geometry that
 * mean something without the engine's tables (picking, depth / position / instance-id maps,
 * line-of-sight tests, range scans).  The reference has no such entry (its inspector works on
 * the selected RenderObject): no ABI bump, detect the symbols.
 *
 * pupil_ray_hits: device pointers to n elements each, NULL = not wanted.  On a miss t = -1, the
 * prim id bits are 0xFFFFFFFF, the ids are -1 and position, normal and texcoord are exactly 0
 * (what a render writes to the normal AOV on a miss).  Alignment: hit 16 B, texcoord 8 B,
 * everything else 4 B; the ray list 16 B (the resolve kernel loads rays and hits as float4 and
 * stores a texcoord as one float2; ids, positions and normals are stored by dwords).
 *
 * pupil_pt_query_rays: n rays (ox, oy, oz, dx, dy, dz, tmin, tmax), read in place from
 * rays_device.  Closest hit unless PUPIL_QUERY_ANY_HIT; `hit` is bit for bit what
 * pupil_pt_trace_rays returns for the same rays (same kernel), degenerate rays included.  With
 * PUPIL_QUERY_ANY_HIT only `hit` may be set (t = 1 occluded, -1 not).  A hidden instance is hit by
 * no ray.  n = 0: PUPIL_OK, nothing is enqueued.  PUPIL_ERR_INVALID, before anything is
 * enqueued: pt, out or (n > 0) rays_device NULL, every field of out NULL, n >= 2^31, an unknown
 * flag, any hit with a resolved output, a misaligned pointer.
 * Asynchronous on hip_stream (NULL = the null stream), with no device-wide sync: ordered by stream
 * events after every render, flow pass and query enqueued so far (they share the traversal's
 * overflow stacks), and later ones order themselves behind it.  The outputs are complete once
 * work later enqueued on hip_stream runs.  Adds nothing to the ray counters of pupil_pt_stats and
 * touches neither the accumulation, the sample count nor the frames in flight.  When `hit` is NULL
 * but resolved outputs are wanted the hits go to engine-owned scratch, which grows geometrically
 * and never shrinks; a flat (one-level) acceleration structure also keeps 4 B per primitive for
 * the resolve of position, normal or texcoord, allocated by the first query that wants one.  A
 * call that fits what is there allocates nothing and synchronises nothing; a growth waits for
 * the queries in flight.
 *
 * pupil_pt_query_camera: the G-buffer form.  One camera ray per local pixel of the tiling -- the
 * ray a render traces for film jitter (jitter_x, jitter_y), (0.5, 0.5) = the pixel centre -- then
 * the same trace and resolve.  Outputs are indexed like the frame buffers (compact = rank-local
 * order; else y*width + x, where a rank writes only its own pixels); tile_* as in
 * pupil_pt_motion_vectors.  rays_out_device (optional, 16-B aligned): receives the rays, 8 floats
 * per local pixel in rank-local order; NULL = they stay in the engine's scratch (the flow pass's).
 *
 * pupil_pt_query_info: queries and rays since create, growths of the engine-owned scratch, and
 * the device time of the last query from events around it (the call waits for that query); any
 * out pointer may be NULL. */
typedef struct pupil_ray_hits {
    void *hit;       /* float4: t, b1, b2, prim id bits -- pupil_pt_trace_rays' layout and values */
    void *instance;  /* int32: index into pupil_scene_desc.instances */
    void *primitive; /* int32: face index within the instance's shape (0 for a sphere) */
    void *material;  /* int32: the instance's material index */
    void *position;  /* float3, world space */
    void *normal;    /* float3: GetHitLocalGeometry's normal (geometry.h:272-320), flip_normals and
                        the two-sided flip towards the ray included: the value of the "normal" AOV */
    void *texcoord;  /* float2 */
} pupil_ray_hits;
enum { PUPIL_QUERY_ANY_HIT = 1 };
int pupil_pt_query_rays(pupil_pt *pt, uint32_t n, const void *rays_device /* 8 floats per ray */, uint32_t flags,
                        const pupil_ray_hits *out, void *hip_stream);
int pupil_pt_query_camera(pupil_pt *pt, float jitter_x, float jitter_y, uint32_t compact, uint32_t tile_size,
                          uint32_t tile_rank, uint32_t tile_world, void *rays_out_device, const pupil_ray_hits *out,
                          void *hip_stream);
int pupil_pt_query_info(pupil_pt *pt, uint64_t *queries, uint64_t *rays, uint64_t *scratch_grows, double *last_ms);

/* Path-traced radiance along rays from device memory: what does this ray see.  The integrator of
 * pupil_pt_render (MIS, every BSDF, area and env emitters) over a ray list that is already on the
 * device instead of the scene's pinhole camera: training batches of rays from many cameras,
 * light-probe and lightmap baking, panoramic / fisheye / orthographic / thin-lens cameras, a second
 * view.  The reference has no such entry: no ABI bump, detect the symbols.
 *
 * Rays: the layout of pupil_pt_query_rays (ox, oy, oz, dx, dy, dz, tmin, tmax), 16-B aligned, read in
 * place.  The direction must be unit length; it is used as given, not re-normalised.  Floats 6 and
 * 7 are IGNORED: every segment of a path, the first included, uses the path tracer's window
 * [0.001, 1e16], so one tensor serves both entries.
 *
 * Launch: random_seed, sample_cnt, spp, accumulate and max_depth (0 = the scene's) mean what they
 * mean for pupil_pt_render; tile_*, collect_stats and hints are ignored.
 *
 * Sample s of ray i is one path of __raygen__main (main.cu:36-194) whose first ray is ray i.  Its
 * RNG is rng_init(id_i, random_seed + s) followed by two discarded draws (the film jitter a camera
 * path draws), id_i = stream_ids_device[i], or i when that is NULL.  The path's radiance enters
 * radiance[i] by the render's running mean, the count being sample_cnt + s when accumulate is set
 * (main.cu:187-191); without accumulate the last sample stays, as in a frame.  So if ray i is the
 * camera ray a render of seed random_seed draws for pixel id_i, radiance[i], albedo[i] and
 * normal[i] equal that render's pixel bit for bit.  The result does not depend on how the call is
 * cut into chunks.
 *
 * Asynchronous on hip_stream (NULL = the null stream), with no device-wide sync: ordered by stream
 * events after every render, flow pass, query and radiance call enqueued so far (they share the
 * traversal's overflow stacks), and later ones order themselves behind it.  Adds nothing to the
 * ray counters of pupil_pt_stats, touches neither any frame's accumulation, the sample count nor
 * the frames in flight, and reads the engine's camera nowhere.
 *
 * Scratch: paths are processed in chunks of at most PUPIL_RADIANCE_CHUNK paths (environment, read
 * at pupil_pt_create; default 16777216, at least 64), 146 B each, so the scratch is bounded
 * whatever n * spp is.  It grows geometrically up to that bound and never shrinks; a growth waits
 * for the calls in flight.  A call that fits allocates nothing and synchronises nothing (depths
 * above 64 read the list lengths back every 16 bounces, as a render of such a depth does).
 * Memory budget: the scratch an engine holds is 146 B x min(PUPIL_RADIANCE_CHUNK, the largest
 * n * spp of any call so far; up to twice that after a growth), kept until pupil_pt_destroy: with
 * the default, at most 2.4 GB, reached by the first call of 16.8 M paths or more (1920x1080 rays at
 * 8 spp is 16.6 M) and held from then on.  PUPIL_RADIANCE_CHUNK=4194304 caps it at 0.6 GB; such a
 * call then runs as four chunks and takes about 1.15 times as long (every stage drains four launch
 * tails instead of one).
 *
 * n = 0: PUPIL_OK, nothing is enqueued.  PUPIL_ERR_INVALID, before anything is enqueued: pt, launch,
 * out, out->radiance or (n > 0) rays_device NULL, spp = 0, n >= 2^31, a misaligned pointer
 * (radiance and the rays 16 B, everything else 4 B).
 *
 * pupil_pt_radiance_info: calls and rays since create, the extension and shadow rays their paths
 * cast (the first ray of a path is not among them; totals of the radiance calls' own), growths of
 * the scratch, and the device time of the last call from events around it.  Asking for the ray
 * totals or the time waits for the last call; any out pointer may be NULL. */
typedef struct pupil_ray_radiance {
    void *radiance; /* float4 per ray, required: rgb + 1, the running mean exactly as the frame's accum buffer */
    void *albedo;   /* float3 per ray, optional: the first hit's albedo AOV (0 on a miss) */
    void *normal;   /* float3 per ray, optional: the first hit's normal AOV (0 on a miss) */
} pupil_ray_radiance;
int pupil_pt_radiance_rays(pupil_pt *pt, uint32_t n, const void *rays_device /* 8 floats per ray */,
                           const uint32_t *stream_ids_device /* n, or NULL = the ray's index */,
                           const pupil_pt_launch *launch, const pupil_ray_radiance *out, void *hip_stream);
int pupil_pt_radiance_info(pupil_pt *pt, uint64_t *calls, uint64_t *rays, uint64_t *extension_rays,
                           uint64_t *shadow_rays, uint64_t *scratch_grows, double *last_ms);

/* ---- verification entry points (used by the parity tests) ----
 * closest (any_hit = 0) or any hit (any_hit = 1) for n host rays packed as
 * (ox, oy, oz, dx, dy, dz, tmin, tmax); out (host) = (t, b1, b2, prim id bits)
 * per ray, prim id = 0xFFFFFFFF and t = -1 on a miss (any hit: t = 1 if occluded).
 * Synchronises the device and allocates per call: production code traces rays that are on
 * the device with pupil_pt_query_rays, which returns the same hits. */
int pupil_pt_trace_rays(pupil_pt *pt, uint32_t n, const float *rays, float *out, int any_hit);
/* copies the flattened BVH4 the traversal kernels read (64-B quantized nodes, 12-float
 * world-space primitive records, root link) to host memory, for the CPU baseline that
 * traverses the same arrays.  Records are the device's record slots (leaf
 * links name slots; every leaf starts on an even slot), 12 floats each; a hole slot between
 * leaves has all bits of its first record's w set.  Call with nodes = records = NULL for the
 * counts.  PUPIL_ERR_UNSUPPORTED for the two-level structure. */
int pupil_pt_export_bvh4(pupil_pt *pt, uint32_t *num_nodes, void *nodes, uint32_t *num_records, float *records,
                         int32_t *root_link);
/* (tests; callers detect the symbol, the ABI version does not count it) copies the two-level
 * structure of world mode (PUPIL_TL_MODE) to host memory, after everything enqueued so far: the
 * node array [0, num_nodes) -- the TLAS in [0, tlas_nodes), its never-written reserve up to
 * tlas_cap, then the per-instance world BLAS copies --, the world record slots as 12 floats each
 * (the mesh instances' records, then one two-slot leaf per sphere), the per-instance world boxes
 * (6 floats each: lo, hi), the root link and the braid depth.  Call with nodes = records =
 * inst_boxes = NULL for the counts; the scalar out pointers after inst_boxes may be NULL.
 * PUPIL_ERR_UNSUPPORTED for the flattened BVH and for object mode, PUPIL_ERR_INVALID for a NULL
 * count pointer or arrays smaller than the counts. */
int pupil_debug_export_world_bvh4(pupil_pt *pt, uint32_t *num_nodes, void *nodes, uint32_t *num_records, float *records,
                                  uint32_t *num_instances, float *inst_boxes, int32_t *root_link, uint32_t *tlas_nodes,
                                  uint32_t *tlas_cap, uint32_t *braid);
/* evaluates the device's sin, cos, acos, atan2(x, y2), sqrt, 1/x on n inputs:
 * out[6*i + k] for k in that order (bit-exactness probe for the CPU oracle) */
int pupil_debug_math(int device, uint32_t n, const float *x, const float *y2, float *out);
/* the device's emitter pick (EmitterGroup::SelectOneEmiiter, render/emitter.h:110-135)
 * for n random numbers p: out[i] = area emitter index, -1 = env, -2 = none */
int pupil_debug_select_emitter(pupil_pt *pt, uint32_t n, const float *p, int32_t *out);
/* the device's area-emitter table, emitters [first, first + n): 24 floats each --
 * select_probability, area, cdf, the type word's bits, pos[3][3], nrm[3][3], 0, 0.
 * PUPIL_ERR_INVALID when the range is out of bounds.  Works with the device-side emitter mode
 * on or off.  For a delta entry (PUPIL_EMITTER_POINT / _SPOT / _DIRECTIONAL) the nine pos floats
 * are center, color, (cutoff, beam, 0); nrm[0] is the axis or direction; area is 0. */
int pupil_debug_read_emitters(pupil_pt *pt, uint32_t first, uint32_t n, float *out);
/* the device's Emitter::SampleDirect (emitter_sample_direct) of table entry `emitter`
 * (== the table's count, delta emitters included: the env emitter) on n inputs xi of 3 floats
 * (x, y used), from the shading point pos_nrm = (position xyz, normal xyz).  out: 8 floats per
 * input, as pupil_debug_env mode 0 -- wi(3), pdf, distance, radiance(3).  The sample is returned
 * as the function gives it: the integrator's gates (NoL > 0, f * pdf != 0) are not applied.
 * PUPIL_ERR_INVALID: a NULL argument, an index beyond the env's, the env's without an env. */
int pupil_debug_emitter_sample(pupil_pt *pt, uint32_t emitter, uint32_t n, const float *xi, const float *pos_nrm,
                               float *out);
/* the CDF's guide table: *bits = guide_bits, guide = its 2^bits + 1 entries.  Call with guide =
 * NULL for the count; a count of 0 means the table has none (fewer than two emitters, or
 * PUPIL_EMITTER_SELECT=binary). */
int pupil_debug_read_emitter_guide(pupil_pt *pt, uint32_t *bits, uint32_t *guide, uint32_t *inout_count);
/* the shade kernels keep copies of the scene's small tables in each block's LDS: caps = the entry
 * caps of the instance, material, area-emitter (delta lights included) and cull-set copies, and
 * *fit (pt may be NULL: then only the caps) has bit k set when table k of the engine's scene is
 * within its cap now; a table over its cap is read from global memory.  Either pointer may be NULL. */
int pupil_debug_shade_tables(pupil_pt *pt, uint32_t caps[4], uint32_t *fit);
/* the device's env emitter on n inputs of 3 floats, from the shading point pos_nrm =
 * (position xyz, normal xyz); out: 8 floats per input.
 * mode 0: Emitter::SampleDirect (render/emitter/env.h:23-49, 70-79) with xi = (in.x, in.y),
 *         both in [0, 1]: out = wi(3), pdf, distance, radiance(3);
 * mode 1: Emitter::Eval as __miss__default reaches it (main.cu:196-212) for a ray from the
 *         position along in.xyz: out = radiance(3), pdf, 0, 0, 0, 0.
 * PUPIL_ERR_INVALID without an env emitter. */
int pupil_debug_env(pupil_pt *pt, uint32_t n, const float *xi_or_dir, const float *pos_nrm, uint32_t mode, float *out);
/* the device's env-map tables, read back after everything enqueued so far: col_cdf
 * ((*width + 1) * *height floats), row_cdf (*height + 1), row_weight (*height) and the
 * normalization.  The size comes back through width and height; call with the four out pointers
 * NULL to size the arrays, and any of them may be NULL.  PUPIL_ERR_INVALID without an env map. */
int pupil_debug_read_env_tables(pupil_pt *pt, uint32_t *width, uint32_t *height, float *col_cdf, float *row_cdf,
                                float *row_weight, float *normalization);
/* the device's cuda::Texture::Sample (framework/cuda/texture.h:33-57) of texture `slot`
 * (0..3) of a material on n (u, v) pairs: out = rgb per input */
int pupil_debug_tex_sample(pupil_pt *pt, uint32_t material, uint32_t slot, uint32_t n, const float *uv, float *out);
/* the device's copy of a material, read back after everything enqueued so far: *type, and
 * out = eta, int_fdr, specular_sampling_weight */
int pupil_debug_read_material(pupil_pt *pt, uint32_t material, uint32_t *type, float out[3]);
/* two-level structure: fills the never-written TLAS reserve [tlas_nodes, tlas_cap) of the
 * node array with nodes whose every float is `value`, then recomputes node_bound (test of
 * the bound's live-node ranges); PUPIL_ERR_UNSUPPORTED for the flattened BVH */
int pupil_debug_fill_tlas_reserve(pupil_pt *pt, float value);
/* the builder's binary tree over n >= 2 boxes (6 floats each: lo xyz, hi xyz) with `rounds`
 * (<= 64) reinsertion rounds: cost[r] = the tree's surface-area cost (sum of the internal
 * nodes' half areas) after r rounds, r = 0 .. rounds; a round the pass did not keep, or did
 * not run because nothing was left to move, repeats the figure before it.  *kept = rounds that
 * moved something and were committed, *rejected = rounds thrown away because they raised the
 * cost (0 or 1: the pass ends at the first); kept + rejected < rounds means a round found
 * nothing to move.  Either may be NULL. */
int pupil_debug_bvh_reinsert(int device, uint32_t n, const float *boxes, uint32_t rounds, double *cost,
                             uint32_t *kept, uint32_t *rejected);
/* the wavefront stages' stable partition of the path ids 0 .. n-1 by a key byte, launched as the
 * engine launches it, on scratch sized for `capacity` >= n paths (at most 2^28) that is filled
 * with the word 0xA5A5A5A5 beforehand.  All pointers are host memory.
 * mode 0 (exclusive): nbins in 1..9, bin = key >> shift_or_tag, the key 0xFF is in no bin; out
 * has n ids.  mode 1 (flags): nbins = 2, bit b of the key puts the path in bin b when key >> 2 ==
 * shift_or_tag; out has 2n ids.  bin_mask: 0 = every bin.  The ids of bin b are
 * out[starts[b] .. starts[b] + counts[b]); the entries of out after *total keep the fill word.
 * counts, starts: nbins each; total (or NULL): one; log (or NULL): nbins, the counts again.
 * cum_in (or NULL): nbins running totals the counts are added to -- cum_out (or NULL) receives
 * the sums and snap (or NULL: the partition gets no snapshot pointer) the totals as they were;
 * cum_out and snap need cum_in.
 * info (or NULL): the rounds and blocks of the tile geometry used (blocks = 0 for n = 0), the
 * histogram entries allocated for the capacity, and 1 when the scratch was written nowhere it
 * should not be: 64 guard words after the histogram and after the id list, the histogram past
 * nbins * blocks entries and the id list past n (2n) ids all still hold the fill word.
 * PUPIL_ERR_INVALID, before the device is touched: keys NULL with n > 0; out, counts or starts
 * NULL; nbins outside 1..9; mode > 1; mode 1 with nbins != 2; n > capacity; capacity > 2^28;
 * cum_out or snap without cum_in. */
int pupil_debug_partition(int device, uint32_t n, uint32_t capacity, const uint8_t *keys, uint32_t nbins,
                          uint32_t mode, uint32_t shift_or_tag, uint32_t bin_mask, const uint64_t *cum_in,
                          uint32_t *out, uint32_t *counts, uint32_t *starts, uint32_t *total, uint32_t *log,
                          uint64_t *cum_out, uint64_t *snap, uint32_t *info);

/* ---- image output (util::BitmapTexture::Save, framework/util/texture.cpp:12-85,152-160) ----
 * rgba: width*height float4, row 0 = image bottom (the "final result" order).
 * EXR: uncompressed FLOAT B,G,R, top row first; HDR: Radiance RGBE, top row first;
 * PFM: float RGB, bottom row first.  format PUPIL_IMAGE_AUTO picks by extension. */
enum { PUPIL_IMAGE_AUTO = 0, PUPIL_IMAGE_EXR = 1, PUPIL_IMAGE_HDR = 2, PUPIL_IMAGE_PFM = 3 };
int pupil_image_save(const char *path, uint32_t width, uint32_t height, const float *rgba, uint32_t format);

/* ---- image input (util::BitmapTexture::Load, framework/util/texture.cpp:87-174) ----
 * Decodes an EXR (by the exact extension ".exr": tinyexr LoadEXR semantics), a
 * Radiance HDR (by signature), a PNG or baseline JPEG (stbi_load semantics with the
 * reference's pow(v / 255, 2.2) mapping) or a PFM file into float RGBA, row 0 = image
 * top (the texture order).  Call with rgba = NULL to get the size, then with a
 * buffer of width*height*4 floats.  PUPIL_ERR_IO with pupil_last_error() when the
 * file is unreadable or its format is not supported. */
int pupil_image_load(const char *path, uint32_t *width, uint32_t *height, float *rgba);

/* ---- denoiser (substitute for optix::Denoiser, framework/optix/denoiser.h:7-66) ----
 * The OptiX AI denoiser has no ROCm equivalent; this is an edge-avoiding
 * a-trous wavelet filter (Dammertz et al. 2010): five passes of a 5x5 B3-spline
 * kernel at strides 1, 2, 4, 8, 16, each tap weighted by colour, normal and
 * albedo similarity.  Mode bits and Execute's data follow the reference:
 * UseAlbedo / UseNormal select the guides, UseTemporal blends with prev_output:
 * without motion_vector the fixed blend out = prev + 0.2 (filtered - prev) of a
 * static camera; with motion_vector (pupil_pt_motion_vectors' flow) the history is
 * fetched where each pixel's surface point was in the previous frame (bilinear, each
 * tap weighted by the similarity of the previous call's guides to this call's),
 * rejected where it is disoccluded (summed tap weight <= 0.05, non-finite flow or a
 * source outside the image) and blended with a per-pixel history length,
 * alpha = max(0.2, 1 / (n + 1)).  The denoiser keeps the previous call's guides and
 * the history length between calls; pupil_denoiser_setup with a new size and
 * pupil_denoiser_reset_history forget them.  Tiled is accepted (the whole frame is
 * filtered at once), ApplyToAOV and UseUpscale2X return PUPIL_ERR_UNSUPPORTED.
 * Buffers are device pointers: input/output/prev_output float4 per pixel,
 * albedo/normal float3 per pixel (the "albedo"/"normal" AOVs), motion_vector float2
 * per pixel. */
enum {
    PUPIL_DENOISE_USE_ALBEDO = 1,
    PUPIL_DENOISE_USE_NORMAL = 1 << 1,
    PUPIL_DENOISE_APPLY_TO_AOV = 1 << 2,
    PUPIL_DENOISE_USE_TEMPORAL = 1 << 3,
    PUPIL_DENOISE_USE_UPSCALE_2X = 1 << 4,
    PUPIL_DENOISE_TILED = 1 << 5
};
typedef struct pupil_denoise_data {
    const void *input;        /* float4 */
    void *output;             /* float4 (may equal input) */
    const void *prev_output;  /* float4, UseTemporal only (NULL: first frame) */
    const void *albedo;       /* float3, UseAlbedo */
    const void *normal;       /* float3, UseNormal */
    const void *motion_vector; /* float2 (cur - prev, pixels), UseTemporal with prev_output: reprojected
                                * history; NULL = fixed blend.  output must then not alias prev_output */
} pupil_denoise_data;
typedef struct pupil_denoiser pupil_denoiser;
/* Denoiser(mode, stream) (denoiser.h:20-21) */
int pupil_denoiser_create(int device, uint32_t mode, pupil_denoiser **out);
/* SetMode / Setup(w, h) (denoiser.h:24-25); sigma_color scales the colour edge-stopping term (0 = 1.0) */
int pupil_denoiser_setup(pupil_denoiser *d, uint32_t mode, uint32_t width, uint32_t height, float sigma_color);
/* Execute(ExecutionData) (denoiser.h:31-40); asynchronous on hip_stream */
int pupil_denoiser_execute(pupil_denoiser *d, const pupil_denoise_data *data, void *hip_stream);
/* ABI 7.  Forgets the temporal history (previous guides, history length): the next reprojecting
 * execute behaves as a first frame (a scene load or a camera cut) */
int pupil_denoiser_reset_history(pupil_denoiser *d);
void pupil_denoiser_destroy(pupil_denoiser *d);

/* ---- host world (the reference's resource::Scene + world::World, C++ inside) ---- */
typedef struct pupil_world pupil_world;

int pupil_world_create(pupil_world **out);
/* mitsuba-3 XML subset, resource/scene.cpp:27-227 semantics */
int pupil_world_load_xml(pupil_world *w, const char *path);
/* programmatic scene building (procedural benchmark scenes) */
int pupil_world_set_film(pupil_world *w, uint32_t width, uint32_t height, uint32_t max_depth);
/* sensor: fov in degrees along fov_axis ('x' or 'y'), to_world row-major 4x4 in mitsuba convention */
int pupil_world_set_sensor(pupil_world *w, float fov, char fov_axis, float near_clip, float far_clip,
                           const float to_world[16]);
int pupil_world_add_mesh(pupil_world *w, uint32_t num_vertices, uint32_t num_faces, const float *positions,
                         const float *normals, const float *texcoords, const uint32_t *indices, uint32_t *out_shape);
int pupil_world_add_builtin_shape(pupil_world *w, const char *name /* rectangle|cube|sphere */, uint32_t *out_shape);
int pupil_world_add_material(pupil_world *w, const pupil_material *m, uint32_t *out_material);
/* is_emitter: area emitter with the given radiance texture */
int pupil_world_add_instance(pupil_world *w, uint32_t shape, uint32_t material, const float to_world[16],
                             uint32_t flip_normals, uint32_t flip_tex_coords, uint32_t is_emitter,
                             const pupil_texture *radiance, uint32_t *out_instance);
/* Removes an instance; later instances shift down by one.  The description afterwards is that of
 * a world built without the instance: emitter offsets and select probabilities included. */
int pupil_world_remove_instance(pupil_world *w, uint32_t instance);
int pupil_world_add_const_env(pupil_world *w, const float radiance[3]);
/* Delta lights (PUPIL_EMITTER_POINT / _SPOT / _DIRECTIONAL above).  Both calls read only e->type
 * and the fields that type names (center and color; for a spot nrm[0], pos[0][0], pos[0][1]; for a
 * directional light nrm[0] and color); the world normalises the axis / direction, and
 * pupil_world_get_desc fills weight (1) and select_probability.
 * *out_light (may be NULL) and `light` number the delta lights in order of addition, whatever their
 * types (lights loaded from XML come first, in file order).  In the desc's table light k is entry
 *   A + (point and spot lights among lights 0 .. k-1)                          for a point or spot,
 *   A + (all point and spot lights) + (directional lights among 0 .. k-1)      for a directional,
 * with A the number of triangle and sphere emitters.
 * pupil_world_set_delta_emitter replaces light `light`; a point may become a spot and back.
 * PUPIL_ERR_INVALID, with the world unchanged: a NULL argument (out_light excepted); a type that is
 * not 5, 6 or 7; a zero or non-finite axis or direction; spot angles outside
 * 0 < beam <= cutoff <= pi (or non-finite); a light index out of range; a type change between
 * point / spot and directional, which would move the light across that boundary of the table. */
int pupil_world_add_delta_emitter(pupil_world *w, const pupil_emitter *e, uint32_t *out_light);
int pupil_world_set_delta_emitter(pupil_world *w, uint32_t light, const pupil_emitter *e);
/* light `light` as the world holds it (axis normalised, weight 1, select_probability 0: that one
 * is the desc's to fill), for callers that change one field.  PUPIL_ERR_INVALID: a NULL argument,
 * a light index out of range. */
int pupil_world_get_delta_emitter(pupil_world *w, uint32_t light, pupil_emitter *out);
/* the inverse of a row-major 3x3 by the routine pupil_world_get_desc derives an env emitter's
 * to_local from its to_world with (the 4x4 inverse in double of the matrix without translation):
 * what pupil_pt_update_env_params needs to match a freshly loaded scene bit for bit.
 * PUPIL_ERR_INVALID: a NULL argument or a singular matrix. */
int pupil_world_invert3x3(const float m[9], float out[9]);
/* RenderInstanceUpdate on the host side: new to_world (row-major 4x4) of instance `instance`
 * (index into pupil_scene_desc.instances); the next pupil_world_get_desc has the new
 * instance matrices and area emitters (world/world.cpp:45-54) */
int pupil_world_set_instance_transform(pupil_world *w, uint32_t instance, const float to_world[16]);
/* RenderObject::visibility_mask (world/render_object.h:16; 1 at creation) of instance `instance`:
 * the world remembers it for the passes, which hand it to pupil_pt_update_instances_masked
 * (visible iff (mask & 0xFF) != 0).  pupil_world_get_desc does not change: a hidden emitter
 * stays in the emitter table, as in the reference. */
int pupil_world_set_instance_visibility(pupil_world *w, uint32_t instance, uint32_t visibility_mask);
int pupil_world_get_instance_visibility(pupil_world *w, uint32_t instance, uint32_t *visibility_mask);
/* Deformable meshes on the host side: new vertices of mesh shape `shape` (index into
 * pupil_scene_desc.shapes), copied into the world's own mesh.  positions: 3 floats per vertex,
 * the vertex count the shape has; normals: the same count, or NULL = kept (PUPIL_ERR_INVALID
 * for a mesh without normals, a sphere, a shape out of range, a null argument).  The next
 * pupil_world_get_desc has the new vertices and, for emissive instances of the shape, the new
 * area emitters (world-space triangles, areas, select probabilities) that
 * pupil_pt_update_emitters takes after pupil_pt_update_shape_vertices. */
int pupil_world_set_mesh_vertices(pupil_world *w, uint32_t shape, const float *positions, const float *normals);
/* the world-side half of pupil_pt_replace_shape_mesh: mesh shape `shape` gets new counts and
 * arrays (copied; normals / texcoords may be NULL), its instances keep material, transform and
 * flags, and pupil_world_get_desc afterwards describes the scene a fresh engine is created from.
 * PUPIL_ERR_INVALID: NULL arguments, a count of 0, shape out of range or not a mesh, an index
 * >= num_vertices; PUPIL_ERR_UNSUPPORTED: an emissive instance shows the shape. */
int pupil_world_set_mesh(pupil_world *w, uint32_t shape, uint32_t num_vertices, uint32_t num_faces,
                         const float *positions, const float *normals, const float *texcoords,
                         const uint32_t *indices);
/* pupil_world_set_mesh with flags: 0 = the same call; PUPIL_WORLD_MESH_EMISSIVE_OK = a shape that
 * emissive instances show is accepted, and pupil_world_get_desc afterwards describes the re-meshed
 * emitter: one area emitter per new face, later instances' emitter_offset shifted, the select
 * probabilities of the new table (the world-side half of pupil_pt_replace_shape_mesh with the
 * device-side emitter table on).  PUPIL_ERR_INVALID for unknown flags. */
#define PUPIL_WORLD_MESH_EMISSIVE_OK 1u
int pupil_world_replace_mesh(pupil_world *w, uint32_t shape, uint32_t num_vertices, uint32_t num_faces,
                             const float *positions, const float *normals, const float *texcoords,
                             const uint32_t *indices, uint32_t flags);
/* A material replaced on the host side: `material` is an index into pupil_scene_desc.materials
 * (the world flattens one material per instance, in instance order, so it is the material of
 * desc instance `material`); the next pupil_world_get_desc carries *m there, and
 * pupil_pt_update_materials takes it from that desc.  Bitmap texels are copied into the world, as
 * by pupil_world_add_material: the caller's array is free once the call returns.  The table of
 * pupil_world_add_material is not changed (instances added later take what they were given).
 * PUPIL_ERR_INVALID, with the world unchanged: a null argument, a material out of range, an
 * unknown texture type, a bitmap without texels or with a zero side. */
int pupil_world_set_material(pupil_world *w, uint32_t material, const pupil_material *m);
/* resolves emitters (EmitterHelper), camera matrices (CameraHelper) and fills desc;
 * pointers stay valid until the world is modified or destroyed */
int pupil_world_get_desc(pupil_world *w, pupil_scene_desc *desc);
void pupil_world_destroy(pupil_world *w);

#ifdef __cplusplus
}
#endif
