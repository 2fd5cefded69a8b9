// world.cpp — World / CameraHelper over the engine's pupil_world.
#include "pupil/world.h"

#include <cstring>

namespace Pupil::world {

void CameraHelper::Load(const pupil_scene_desc &d) noexcept {
    std::memcpy(m_s2c, d.sample_to_camera, sizeof(m_s2c));
    std::memcpy(m_c2w, d.camera_to_world, sizeof(m_c2w));
}

void CameraHelper::SetCameraToWorld(const float c2w[16]) noexcept {
    {
        std::unique_lock<std::mutex> lock;
        if (m_lock) lock = std::unique_lock<std::mutex>(*m_lock);
        std::memcpy(m_c2w, c2w, sizeof(m_c2w));
    }
    EventDispatcher<EWorldEvent::CameraChange>(this);
}

void CameraHelper::Snapshot(float s2c[16], float c2w[16]) const noexcept {
    std::unique_lock<std::mutex> lock;
    if (m_lock) lock = std::unique_lock<std::mutex>(*m_lock);
    std::memcpy(s2c, m_s2c, sizeof(m_s2c));
    std::memcpy(c2w, m_c2w, sizeof(m_c2w));
}

World::World() noexcept {
    if (pupil_world_create(&m_world) != PUPIL_OK) {
        Log("world creation failed: %s", pupil_last_error());
        m_world = nullptr;
    }
    scene = std::make_unique<SceneInfo>();
    camera = std::make_unique<CameraHelper>();
    camera->m_lock = &m_mutex;
}

World::~World() noexcept {
    if (m_world) pupil_world_destroy(m_world);
}

bool World::LoadScene(const std::filesystem::path &xml) noexcept {
    if (!m_world) return false;
    if (pupil_world_load_xml(m_world, xml.string().c_str()) != PUPIL_OK) {
        Log("scene '%s': %s", xml.string().c_str(), pupil_last_error());
        return false;
    }
    return Finalize();
}

bool World::Finalize() noexcept {
    if (!m_world || pupil_world_get_desc(m_world, &m_desc) != PUPIL_OK) {
        Log("scene description failed: %s", pupil_last_error());
        return false;
    }
    scene->sensor.film.w = (int)m_desc.width;
    scene->sensor.film.h = (int)m_desc.height;
    scene->integrator.max_depth = (int)m_desc.max_depth;
    camera->Load(m_desc);
    return true;
}

bool World::SetInstanceTransform(uint32_t instance, const float to_world[16]) noexcept {
    {
        std::scoped_lock lock(m_mutex);
        if (!m_world || pupil_world_set_instance_transform(m_world, instance, to_world) != PUPIL_OK) {
            Log("instance update failed: %s", pupil_last_error());
            return false;
        }
        // the desc only: the camera keeps any SetCameraToWorld made since the load
        if (pupil_world_get_desc(m_world, &m_desc) != PUPIL_OK) {
            Log("scene description failed: %s", pupil_last_error());
            return false;
        }
    }
    InstanceUpdate u{this, instance};
    EventDispatcher<EWorldEvent::RenderInstanceUpdate>(&u);
    return true;
}

bool World::SetInstanceVisibility(uint32_t instance, uint32_t mask) noexcept {
    {
        std::scoped_lock lock(m_mutex);
        if (!m_world || pupil_world_set_instance_visibility(m_world, instance, mask) != PUPIL_OK) {
            Log("instance visibility failed: %s", pupil_last_error());
            return false;
        }
    }
    InstanceUpdate u{this, instance};
    EventDispatcher<EWorldEvent::RenderInstanceUpdate>(&u);
    return true;
}

bool World::SetMeshVertices(uint32_t shape, const float *positions, const float *normals) noexcept {
    {
        std::scoped_lock lock(m_mutex);
        if (!m_world || pupil_world_set_mesh_vertices(m_world, shape, positions, normals) != PUPIL_OK) {
            Log("mesh vertex update failed: %s", pupil_last_error());
            return false;
        }
        if (pupil_world_get_desc(m_world, &m_desc) != PUPIL_OK) {
            Log("scene description failed: %s", pupil_last_error());
            return false;
        }
    }
    InstanceUpdate u{this, 0u, shape};
    EventDispatcher<EWorldEvent::RenderInstanceUpdate>(&u);
    return true;
}

bool World::SetMesh(uint32_t shape, const pupil_shape &mesh, bool allow_emissive) noexcept {
    std::scoped_lock lock(m_mutex);
    if (!m_world || pupil_world_replace_mesh(m_world, shape, mesh.num_vertices, mesh.num_faces, mesh.positions, mesh.normals,
                                             mesh.texcoords, mesh.indices,
                                             allow_emissive ? (uint32_t)PUPIL_WORLD_MESH_EMISSIVE_OK : 0u) != PUPIL_OK) {
        Log("mesh replacement failed: %s", pupil_last_error());
        return false;
    }
    if (pupil_world_get_desc(m_world, &m_desc) != PUPIL_OK) {
        Log("scene description failed: %s", pupil_last_error());
        return false;
    }
    return true;
}

bool World::SetMaterial(uint32_t material, const pupil_material &m) noexcept {
    std::scoped_lock lock(m_mutex);
    if (!m_world || pupil_world_set_material(m_world, material, &m) != PUPIL_OK) {
        Log("material update failed: %s", pupil_last_error());
        return false;
    }
    if (pupil_world_get_desc(m_world, &m_desc) != PUPIL_OK) {
        Log("scene description failed: %s", pupil_last_error());
        return false;
    }
    return true;
}

namespace {
pupil_emitter DeltaLight(uint32_t type, const float *position, const float *direction, const float color[3]) {
    pupil_emitter e;
    std::memset(&e, 0, sizeof(e));
    e.type = type;
    for (int k = 0; k < 3; k++) {
        e.color[k] = color[k];
        if (position) e.center[k] = position[k];
        if (direction) e.nrm[0][k] = direction[k];
    }
    return e;
}
}  // namespace

int World::AddLight(const pupil_emitter &e) noexcept {
    std::scoped_lock lock(m_mutex);
    uint32_t light = 0;
    if (!m_world || pupil_world_add_delta_emitter(m_world, &e, &light) != PUPIL_OK) {
        Log("light not added: %s", pupil_last_error());
        return -1;
    }
    // a world without a shape yet has no desc: Finalize() fills it once there is one
    (void)pupil_world_get_desc(m_world, &m_desc);
    return (int)light;
}

int World::AddPointLight(const float position[3], const float intensity[3]) noexcept {
    return AddLight(DeltaLight(PUPIL_EMITTER_POINT, position, nullptr, intensity));
}

int World::AddSpotLight(const float position[3], const float direction[3], const float intensity[3], float cutoff_deg,
                        float beam_deg) noexcept {
    pupil_emitter e = DeltaLight(PUPIL_EMITTER_SPOT, position, direction, intensity);
    const float deg = 3.14159265358979323846f / 180.f;
    e.pos[0][0] = cutoff_deg * deg;
    e.pos[0][1] = (beam_deg < 0.f ? cutoff_deg * 0.75f : beam_deg) * deg;
    return AddLight(e);
}

int World::AddDirectionalLight(const float direction[3], const float irradiance[3]) noexcept {
    return AddLight(DeltaLight(PUPIL_EMITTER_DIRECTIONAL, nullptr, direction, irradiance));
}

bool World::SetLight(uint32_t light, const pupil_emitter &e) noexcept {
    std::scoped_lock lock(m_mutex);
    if (!m_world || pupil_world_set_delta_emitter(m_world, light, &e) != PUPIL_OK) {
        Log("light update failed: %s", pupil_last_error());
        return false;
    }
    if (pupil_world_get_desc(m_world, &m_desc) != PUPIL_OK) {
        Log("scene description failed: %s", pupil_last_error());
        return false;
    }
    return true;
}

// the caller holds Mutex() where another thread may edit the world
uint32_t World::InstanceVisibility(uint32_t instance) noexcept {
    uint32_t mask = 1u;
    if (m_world) (void)pupil_world_get_instance_visibility(m_world, instance, &mask);
    return mask;
}

}  // namespace Pupil::world
