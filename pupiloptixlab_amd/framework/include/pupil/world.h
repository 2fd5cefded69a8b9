// world.h — host scene of the C++ layer (framework/world/world.h:25-70 names).
// Wraps the engine's pupil_world (XML loader, programmatic builder, emitter
// table, camera matrices) and exposes the fields PTPass reads in the
// reference: world->scene->sensor.film.{w,h}, world->scene->integrator.max_depth,
// world->camera (CameraHelper, world/camera.h).
#pragma once

#include <filesystem>
#include <memory>

#include "framework.h"

namespace Pupil::world {

struct SceneInfo {
    struct {
        struct {
            int w = 0, h = 0;
        } film;
    } sensor;
    struct {
        int max_depth = 1;
    } integrator;
};

class CameraHelper {
public:
    // Unsynchronised views (single-threaded use); a render thread takes Snapshot().
    const float *SampleToCamera() const noexcept { return m_s2c; }
    const float *CameraToWorld() const noexcept { return m_c2w; }
    // Replace the camera-to-world matrix (row-major 4x4) and fire
    // EWorldEvent::CameraChange, like CameraHelper's setters (world/camera.cpp).
    // Safe from any thread (the World's mutex guards the matrices).
    void SetCameraToWorld(const float c2w[16]) noexcept;
    void Snapshot(float s2c[16], float c2w[16]) const noexcept;
    void Load(const pupil_scene_desc &d) noexcept;

private:
    friend class World;
    std::mutex *m_lock = nullptr;  // the owning World's mutex
    float m_s2c[16] = {};
    float m_c2w[16] = {};
};

class World;
// payload of EWorldEvent::RenderInstanceUpdate
struct InstanceUpdate {
    World *world;
    uint32_t instance;  // index into Desc().instances
    // World::SetMeshVertices: the mesh shape (index into Desc().shapes) whose vertices changed;
    // `instance` is unused then
    uint32_t shape = 0xFFFFFFFFu;
};

class World {
public:
    std::unique_ptr<SceneInfo> scene;
    std::unique_ptr<CameraHelper> camera;

    World() noexcept;
    ~World() noexcept;
    World(const World &) = delete;
    World &operator=(const World &) = delete;

    bool LoadScene(const std::filesystem::path &xml) noexcept;
    // Programmatic scenes: the caller filled `handle()` through pupil_world_*.
    bool Finalize() noexcept;
    // Moves instance `instance` (row-major 4x4), refreshes Desc() (instance
    // matrices, area emitters) and fires EWorldEvent::RenderInstanceUpdate.  Safe from
    // any thread: the edit happens under Mutex(), the event is fired after it.
    bool SetInstanceTransform(uint32_t instance, const float to_world[16]) noexcept;
    // RenderObject::visibility_mask (world/render_object.h:16; the inspector's checkbox,
    // gui.cpp:780-784): visible iff mask & 0xFF.  Fires EWorldEvent::RenderInstanceUpdate; the
    // pass picks the mask up at the top of its next OnRun.  Desc() does not change: a hidden
    // emitter stays in the emitter table, as in the reference (world/world.cpp:45-54).
    bool SetInstanceVisibility(uint32_t instance, uint32_t mask) noexcept;
    uint32_t InstanceVisibility(uint32_t instance) noexcept;
    // Deformable meshes: new vertices of mesh shape `shape` (3 floats per vertex, the count the
    // shape has; normals null = kept), copied into the world.  Refreshes Desc() (vertices, the
    // area emitters of emissive instances) and fires EWorldEvent::RenderInstanceUpdate with
    // InstanceUpdate::shape set; the pass refits once at the top of its next OnRun.
    bool SetMeshVertices(uint32_t shape, const float *positions, const float *normals = nullptr) noexcept;
    // New topology for mesh shape `shape` (pupil_world_set_mesh / _replace_mesh): the arrays are
    // copied, *mesh is a PUPIL_SHAPE_MESH as PTPass::ReplaceShapeMesh takes it.  allow_emissive: a
    // shape emissive instances show is accepted, and Desc() then carries the re-meshed emitter (new
    // ranges, later offsets shifted, new probabilities), which a pass with SetDeviceEmitters(true)
    // follows in place.  Refreshes Desc() and fires no event: PTPass::ReplaceShapeMesh hands the
    // mesh to the engine.
    bool SetMesh(uint32_t shape, const pupil_shape &mesh, bool allow_emissive = false) noexcept;
    // Replaces material `material` (index into Desc().materials: one per instance, in instance
    // order) and refreshes Desc().  The reference has no event for a material edit and fires
    // none: PTPass::UpdateMaterials hands the material to the engine.
    bool SetMaterial(uint32_t material, const pupil_material &m) noexcept;
    // Delta lights (pupil_world_add_delta_emitter / _set_delta_emitter; PUPIL_EMITTER_POINT in
    // pupil_pt.h has the table order, the selection rule and the sampling).  The adders return the
    // light's number (lights count in order of addition, those of the XML file first) or -1;
    // directions need not be unit length, angles are in degrees (beam_deg < 0: 3/4 of the
    // cutoff, mitsuba's default).  SetLight replaces light `light` by *e as the C entry reads it
    // (angles in radians).  All refresh Desc() and fire no event: PTPass::UpdateLights hands the
    // table to the engine.
    int AddPointLight(const float position[3], const float intensity[3]) noexcept;
    int AddSpotLight(const float position[3], const float direction[3], const float intensity[3],
                     float cutoff_deg = 20.f, float beam_deg = -1.f) noexcept;
    int AddDirectionalLight(const float direction[3], const float irradiance[3]) noexcept;
    bool SetLight(uint32_t light, const pupil_emitter &e) noexcept;

    pupil_world *handle() noexcept { return m_world; }
    // Flattened scene for pupil_pt_create (valid until the world changes); a thread
    // reading it while another may edit the world holds Mutex().
    const pupil_scene_desc &Desc() const noexcept { return m_desc; }
    std::mutex &Mutex() noexcept { return m_mutex; }

private:
    int AddLight(const pupil_emitter &e) noexcept;
    pupil_world *m_world = nullptr;
    pupil_scene_desc m_desc{};
    std::mutex m_mutex;
};

}  // namespace Pupil::world
