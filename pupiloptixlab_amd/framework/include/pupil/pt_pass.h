// pt_pass.h — the path-tracing pass (example/path_tracer/pt_pass.h:20-43),
// rendering with the HIP wavefront engine through the C ABI instead of an
// OptiX pipeline + SBT.  Same constructor, OnRun, Inspector, SetScene and
// event bindings; same buffers ("pt accum buffer", "albedo", "normal",
// "test", writing "final result").
#pragma once

#include <atomic>
#include <mutex>
#include <string_view>
#include <vector>

#include "framework.h"
#include "world.h"

namespace Pupil::pt {

class PTPass : public Pass {
public:
    PTPass(std::string_view name = "Path Tracing") noexcept;
    ~PTPass() noexcept override;

    void OnRun() noexcept override;
    void Inspector() noexcept override;
    void SetScene(world::World *world) noexcept;

    // headless accessors (the reference shows these in its ImGui inspector)
    uint32_t SampleCount() const noexcept { return m_sample_cnt; }
    int MaxDepth() const noexcept { return m_max_depth; }
    void SetMaxDepth(int depth) noexcept;
    void SetAccumulate(bool on) noexcept;
    bool Stats(pupil_pt_counters &out) noexcept;
    // Deformed mesh: the next OnRun hands the vertices the world holds for `shape` to the engine
    // (pupil_pt_update_shape_vertices, then the emitter table if an instance of it emits) and
    // restarts accumulation.  World::SetMeshVertices calls this through its event; several
    // updates of a shape before one OnRun cost one refit.
    void UpdateShape(uint32_t shape) noexcept;
    // Flow for deforming meshes (default off): OnRun keeps a pending shape's vertices from before
    // its update (pupil_pt_snapshot_shape_vertices), so ComputeMotionVectors covers the
    // deformation, and forgets the snapshots on an OnRun that applies no shape update.
    void SetKeepPreviousVertices(bool on) noexcept;
    // Engine-owned area-emitter table (pupil_pt_enable_device_emitters; default off): call after
    // SetScene.  While on, the engine rebuilds the table on the device after every update of an
    // emissive shape or instance, and OnRun's update handlers upload no host emitter table.
    // SetScene switches it off (a new engine).  False: no scene, or the engine refused.
    bool SetDeviceEmitters(bool on) noexcept;
    // Materials and textures in place (pupil_pt_update_materials / _update_texture_device), applied
    // now: call them from the thread that runs OnRun, between OnRuns, like SetDeviceEmitters.
    // UpdateMaterials: Desc().materials[i] of the scene's world for every i in ids
    // (World::SetMaterial), in one engine call.  UpdateTextureDevice: width x height float4 texels
    // in device memory for bitmap slot `slot` of `material`, copied after the work enqueued so far
    // on `stream`.  Both restart accumulation at the next OnRun, as an instance update does.
    // False: no scene, or the engine refused (the log has pupil_last_error).
    bool UpdateMaterials(const std::vector<uint32_t> &ids) noexcept;
    // Point, spot and directional lights added or changed on the scene's world (World::AddPointLight,
    // SetLight, ...): hands Desc()'s emitter table to the engine (pupil_pt_update_emitters; in place
    // when no light was added or changed its type), under the same threading rule.  Restarts
    // accumulation at the next OnRun.  False: no scene, or the engine refused.
    bool UpdateLights() noexcept;
    bool UpdateTextureDevice(uint32_t material, uint32_t slot, const void *rgba_device, uint32_t width, uint32_t height,
                             hipStream_t stream) noexcept;
    // The env map in place (pupil_pt_update_env_device / _update_env_params), applied now, under the
    // same threading rule: between OnRuns, from OnRun's thread.  UpdateEnvDevice: width x height
    // float4 texels in device memory for the scene's env map of that size, copied after the work
    // enqueued so far on `stream` (a hipStream_t); the map's CDF tables follow on the device.
    // UpdateEnvParams: scale and rotation (row-major 3x3) of the env map; to_local is the world's
    // own inverse of to_world (pupil_world_invert3x3), as a freshly loaded scene's is.  Both
    // restart accumulation at the next OnRun.  False: no scene, or the engine refused.
    bool UpdateEnvDevice(const void *rgba_device, uint32_t width, uint32_t height, void *stream) noexcept;
    bool UpdateEnvParams(float scale, const float to_world[9]) noexcept;
    // Instances moved from device memory (pupil_pt_update_instances_device), applied now, under the
    // same threading rule: entry k moves instance ids_device[k] (NULL: instance k) to the row-major
    // 3x4 at to_world_device + 12k floats; to_object_device NULL = the engine inverts on the device.
    // The arrays are read after the work enqueued so far on `stream` (a hipStream_t).  Visibility
    // stays; an emissive instance needs SetDeviceEmitters(true).  ComputeMotionVectors after the
    // next OnRun covers the move, which also restarts accumulation.  False: no scene, or the engine
    // refused.
    bool UpdateInstancesDevice(uint32_t n, const uint32_t *ids_device, const void *to_world_device,
                               const void *to_object_device, void *stream) noexcept;
    // A mesh of new topology in place (pupil_pt_replace_shape_mesh), applied now, under the same
    // threading rule: mesh shape `shape` gets the counts and arrays of `mesh` (host pointers, or,
    // with `device`, device pointers read after the work enqueued so far on `stream`, a
    // hipStream_t).  The whole acceleration structure is rebuilt; a pending UpdateShape of the
    // shape is dropped (the world's vertices it would hand over have the old count until
    // pupil_world_set_mesh brings the world in step) and so is the shape's vertex snapshot.
    // Restarts accumulation at the next OnRun.  False: no scene, or the engine refused -- a sphere,
    // a shape an emissive instance shows while SetDeviceEmitters is off (on: the engine rebuilds its
    // emitter table at the new size; World::SetMesh(..., true) keeps the world in step), an index
    // out of range -- and then nothing has changed.
    bool ReplaceShapeMesh(uint32_t shape, const pupil_shape &mesh, bool device = false, void *stream = nullptr) noexcept;
    // The instance table as a whole (pupil_pt_set_instances), applied now, under the same threading
    // rule: the engine's instances become instances[0..n) -- added, removed, or bound to another
    // shape or material slot of the scene the pass was set on -- with visibility_mask (n masks, or
    // null: all visible).  Transforms from the structs, or, with to_world_device, from n x 12
    // device floats read after the work enqueued so far on `stream` (a hipStream_t) and inverted
    // on the device.  With SetDeviceEmitters(true) the call goes to pupil_pt_set_instances_emitters
    // with the world's Desc() (its radiances and delta lights): emissive instances may be added,
    // removed, reordered, rebound or moved.  Otherwise they must stay the old ones, in order.  The pass's own
    // per-instance state follows: recorded instance updates are dropped, and the flow of the next
    // ComputeMotionVectors covers the camera only.  Restarts accumulation at the next OnRun.
    // False: no scene, or the engine refused (pupil_last_error()) -- then nothing has changed.
    bool SetInstances(uint32_t n, const pupil_instance *instances, const uint32_t *visibility_mask = nullptr,
                      const void *to_world_device = nullptr, void *stream = nullptr) noexcept;
    // Screen-space flow since the previous OnRun (pupil_pt_motion_vectors: the camera of that
    // OnRun, and the instance transforms it rendered with if this OnRun moved any), written to
    // the "motion vector" buffer (float2 per pixel, allocated on first use; this rank's tiles in
    // compact order when the frame is gathered) for optix::Denoiser::ExecutionData::motion_vector.
    // Synchronised like OnRun.  After a single OnRun the flow is zero on every surface.
    bool ComputeMotionVectors() noexcept;
    // Ray queries from device memory (pupil_pt_query_rays / _query_camera): what n device rays
    // (8 floats each: origin, direction, tmin, tmax) hit, or what the camera ray through every
    // pixel of this rank's tiles hits at film jitter (jitter_x, jitter_y), into the device arrays
    // of `out` that are not null.  Enqueued on `stream` (a hipStream_t; QueryCamera: the pass's
    // own), ordered after every OnRun enqueued so far; the caller synchronises before reading.
    // Between OnRuns, from OnRun's thread.  Nothing the pass renders changes.  False: no scene,
    // or the engine refused (pupil_last_error()).
    bool QueryRays(uint32_t n, const void *rays_device, const pupil_ray_hits &out, bool any_hit = false,
                   void *stream = nullptr) noexcept;
    bool QueryCamera(const pupil_ray_hits &out, float jitter_x = 0.5f, float jitter_y = 0.5f,
                     void *rays_out_device = nullptr) noexcept;
    // Path-traced radiance along rays from device memory (pupil_pt_radiance_rays): what the n rays
    // at rays_device see (QueryRays' layout; unit directions, tmin and tmax ignored), spp samples
    // each, into out.radiance (float4 per ray, required) and the optional first-hit AOVs.  Sample
    // s of ray i draws from the RNG of pixel stream_ids_device[i] (null: i) at seed + s, so a
    // pixel's camera ray reproduces an OnRun's pixel; sample_cnt and accumulate as in OnRun,
    // max_depth 0 = the scene's.  The pass's camera plays no part, and nothing it renders
    // changes.  Enqueued on `stream`, ordered after every OnRun enqueued so far; the caller
    // synchronises before reading.  False: no scene, or the engine refused (pupil_last_error()).
    bool RadianceRays(uint32_t n, const void *rays_device, const pupil_ray_radiance &out, uint32_t spp = 1,
                      uint32_t seed = 0, const uint32_t *stream_ids_device = nullptr, uint32_t sample_cnt = 0,
                      bool accumulate = false, uint32_t max_depth = 0, void *stream = nullptr) noexcept;

private:
    void BindingEventCallback() noexcept;

    pupil_pt *m_engine = nullptr;
    hipStream_t m_stream = nullptr;
    world::World *m_world = nullptr;
    pupil_pt_frame m_frame{};
    void *m_full_result = nullptr;  // System's full-frame "final result" (the gather target)
    uint32_t m_random_seed = 0;
    uint32_t m_sample_cnt = 0;
    uint32_t m_frame_max_depth = 1;  // value in effect for the running accumulation
    int m_max_depth = 1;
    bool m_accumulated_flag = true;
    std::atomic_bool m_dirty = true;
    // instances moved since the last OnRun (RenderInstanceUpdate only records them, as the
    // reference's handler only sets m_dirty, pt_pass.cpp:216-218; OnRun refits once)
    std::mutex m_pending_mutex;
    std::vector<uint32_t> m_pending;
    std::vector<uint32_t> m_pending_shapes;  // shapes deformed since the last OnRun (same mutex)
    // what ComputeMotionVectors compares against: the cameras of the last two OnRuns, the
    // instance transforms now in the engine and those before the last OnRun's update
    float m_cam[2][2][16] = {};  // [0] last OnRun, [1] the one before; [.][0] sample_to_camera, [.][1] camera_to_world
    bool m_have_cam = false;
    std::vector<float> m_to_world, m_prev_to_world;  // 12 floats per instance
    bool m_instances_moved = false;                 // by the last OnRun
    bool m_device_moved = false;                    // UpdateInstancesDevice since the last OnRun
    std::atomic_bool m_keep_prev_verts = false;     // SetKeepPreviousVertices
    bool m_snapshots = false;                       // the engine holds vertex snapshots
    bool m_device_emitters = false;                 // SetDeviceEmitters
};

}  // namespace Pupil::pt
