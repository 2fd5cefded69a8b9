// pt_pass.cpp — PTPass over the HIP engine (example/path_tracer/pt_pass.cpp).
#include "pupil/pt_pass.h"

#include <algorithm>
#include <cstring>

namespace Pupil::pt {

PTPass::PTPass(std::string_view name) noexcept : Pass(name) {
    if (hipStreamCreateWithFlags(&m_stream, hipStreamNonBlocking) != hipSuccess) {
        Log("%s: stream creation failed", this->name.c_str());
        m_stream = nullptr;
    }
    BindingEventCallback();
}

PTPass::~PTPass() noexcept {
    if (m_engine) pupil_pt_destroy(m_engine);
    if (m_stream) (void)hipStreamDestroy(m_stream);
}

// pt_pass.cpp:39-57: refresh on dirty (camera, instances moved since the last frame,
// depth, accumulation reset), one 1-spp frame, synchronise, advance seed and sample
// count.  Runs on the render thread; events may arrive from any other thread.
void PTPass::OnRun() noexcept {
    if (!m_engine) return;
    std::memcpy(m_cam[1], m_cam[0], sizeof(m_cam[0]));  // the previous OnRun's view, for ComputeMotionVectors
    m_instances_moved = m_device_moved;  // UpdateInstancesDevice since the last OnRun: its "before" stays
    m_device_moved = false;
    if (m_snapshots) {  // the vertex snapshots of the OnRun before are a frame old
        pupil_pt_clear_vertex_snapshots(m_engine);
        m_snapshots = false;
    }
    if (m_dirty) {
        m_dirty = false;  // an event after this point marks the next frame dirty again
        std::vector<uint32_t> moved, deformed;
        {
            std::scoped_lock lock(m_pending_mutex);
            moved.swap(m_pending);
            deformed.swap(m_pending_shapes);
        }
        float s2c[16], c2w[16];
        m_world->camera->Snapshot(s2c, c2w);
        pupil_pt_set_camera(m_engine, s2c, c2w);
        std::memcpy(m_cam[0][0], s2c, sizeof(s2c));
        std::memcpy(m_cam[0][1], c2w, sizeof(c2w));
        if (!m_have_cam) std::memcpy(m_cam[1], m_cam[0], sizeof(m_cam[0]));  // first frame: no motion
        m_have_cam = true;
        if (!moved.empty() || !deformed.empty()) {
            std::scoped_lock lock(m_world->Mutex());
            const pupil_scene_desc &d = m_world->Desc();
            // the desc's emitter table describes the whole scene as it is now: it goes up ONCE, after
            // every geometry and instance update of this OnRun that changed an emitter and succeeded
            bool emitters = false;
            // deformed shapes first (one geometry refit each), so that the instance refit below and the
            // emitter table meet the vertices they were made from
            for (uint32_t shape : deformed) {
                if (shape >= d.num_shapes) continue;
                const pupil_shape &sh = d.shapes[shape];
                if (m_keep_prev_verts && sh.kind == PUPIL_SHAPE_MESH) {  // the "before" of ComputeMotionVectors
                    if (pupil_pt_snapshot_shape_vertices(m_engine, shape) == PUPIL_OK) m_snapshots = true;
                    else Log("%s: vertex snapshot failed: %s", name.c_str(), pupil_last_error());
                }
                if (pupil_pt_update_shape_vertices(m_engine, shape, sh.positions, sh.normals, 0u, nullptr) != PUPIL_OK) {
                    Log("%s: shape update failed: %s", name.c_str(), pupil_last_error());
                    continue;  // the other shapes and their emitters still follow
                }
                for (uint32_t i = 0; i < d.num_instances; i++)
                    emitters = emitters || (d.instances[i].shape == shape && d.instances[i].emitter_offset >= 0);
            }
            if (!moved.empty()) {  // m_world->GetIASHandle(2, true) + the emitter group (pt_pass.cpp:46-47)
                std::vector<float> tw(12 * moved.size()), to(12 * moved.size());
                std::vector<uint32_t> vis(moved.size());  // ias_manager.cpp:187-197: transform and mask together
                bool emissive = false;
                for (size_t k = 0; k < moved.size(); k++) {
                    const pupil_instance &ins = d.instances[moved[k]];
                    vis[k] = m_world->InstanceVisibility(moved[k]);
                    std::memcpy(&tw[12 * k], ins.to_world, sizeof(ins.to_world));
                    std::memcpy(&to[12 * k], ins.to_object, sizeof(ins.to_object));
                    emissive = emissive || ins.emitter_offset >= 0;
                }
                if (!m_instances_moved) m_prev_to_world = m_to_world;
                for (size_t k = 0; k < moved.size(); k++)
                    if (12 * (size_t)moved[k] + 12 <= m_to_world.size())
                        std::memcpy(&m_to_world[12 * (size_t)moved[k]], &tw[12 * k], 12 * sizeof(float));
                m_instances_moved = true;
                if (pupil_pt_update_instances_masked(m_engine, (uint32_t)moved.size(), moved.data(), tw.data(), to.data(),
                                                     vis.data()) != PUPIL_OK)
                    Log("%s: instance update failed: %s", name.c_str(), pupil_last_error());
                else
                    emitters = emitters || emissive;
            }
            // with the engine-owned emitter table on, the update calls above have rebuilt it
            if (emitters && !m_device_emitters && pupil_pt_update_emitters(m_engine, &d) != PUPIL_OK)
                Log("%s: emitter update failed: %s", name.c_str(), pupil_last_error());
        }
        m_frame_max_depth = (uint32_t)m_max_depth;
        m_sample_cnt = 0;
        m_random_seed = 0;
    }
    pupil_pt_launch launch{};
    launch.random_seed = m_random_seed;
    launch.sample_cnt = m_sample_cnt;
    launch.spp = 1;
    launch.max_depth = m_frame_max_depth;
    launch.accumulate = m_accumulated_flag ? 1u : 0u;
    FrameGather *gather = util::Singleton<System>::instance()->Gather();
    if (gather) {  // this rank's tiles only (dist.h)
        launch.tile_size = gather->Info().tile;
        launch.tile_rank = (uint32_t)gather->Info().rank;
        launch.tile_world = (uint32_t)gather->Info().world;
    }
    if (pupil_pt_render(m_engine, &m_frame, &launch, m_stream) != PUPIL_OK) {
        Log("%s: render failed: %s", name.c_str(), pupil_last_error());
        return;
    }
    if (gather && !gather->Gather(m_frame.frame, m_full_result, m_stream)) {
        Log("%s: tile gather failed", name.c_str());
        return;
    }
    (void)hipStreamSynchronize(m_stream);
    m_sample_cnt += m_accumulated_flag ? 1u : 0u;
    ++m_random_seed;
}

void PTPass::SetScene(world::World *world) noexcept {
    if (!world) return;
    m_world = world;
    {
        std::scoped_lock lock(m_pending_mutex);  // moves of the previous world
        m_pending.clear();
        m_pending_shapes.clear();
    }
    if (m_engine) {
        pupil_pt_destroy(m_engine);
        m_engine = nullptr;
    }
    m_snapshots = false;  // they went with the engine
    m_device_emitters = false;  // and so did the engine-owned emitter table: a new engine
    int w = world->scene->sensor.film.w, h = world->scene->sensor.film.h;
    m_max_depth = world->scene->integrator.max_depth;
    m_accumulated_flag = true;
    auto *bm = BufferManager::instance();
    Buffer *final_result = bm->GetBuffer(BufferManager::DEFAULT_FINAL_RESULT_BUFFER_NAME);
    m_full_result = final_result ? final_result->cuda_ptr : nullptr;
    FrameGather *gather = util::Singleton<System>::instance()->Gather();
    if (gather) {  // multi-GPU: the pass's buffers hold this rank's tiles, compact (dist.h)
        w = (int)std::max(1u, gather->LocalPixels());
        h = 1;
        BufferDesc tiles;
        tiles.name = "final result (local tiles)";
        tiles.width = (uint32_t)w;
        tiles.height = 1;
        tiles.stride_in_byte = sizeof(float) * 4;
        final_result = bm->AllocBuffer(tiles);
    }
    BufferDesc desc;
    desc.width = (uint32_t)w;
    desc.height = (uint32_t)h;
    desc.name = "pt accum buffer";
    desc.stride_in_byte = sizeof(float) * 4;
    Buffer *accum = bm->AllocBuffer(desc);
    desc.name = "albedo";
    desc.flag = EBufferFlag::AllowDisplay;
    desc.stride_in_byte = sizeof(float) * 3;
    Buffer *albedo = bm->AllocBuffer(desc);
    desc.name = "normal";
    Buffer *normal = bm->AllocBuffer(desc);
    desc.name = "test";
    desc.stride_in_byte = sizeof(float);
    Buffer *test = bm->AllocBuffer(desc);
    if (!final_result || !accum || !albedo || !normal || !test) {
        Log("%s: output buffers unavailable", name.c_str());
        return;
    }
    m_frame = pupil_pt_frame{accum->cuda_ptr, final_result->cuda_ptr, albedo->cuda_ptr, normal->cuda_ptr,
                             test->cuda_ptr, gather ? 1u : 0u, 0u};
    int dev = 0;
    (void)hipGetDevice(&dev);
    if (pupil_pt_create(&world->Desc(), dev, &m_engine) != PUPIL_OK) {
        Log("%s: engine creation failed: %s", name.c_str(), pupil_last_error());
        m_engine = nullptr;
        return;
    }
    const pupil_scene_desc &sd = world->Desc();
    m_to_world.resize(12 * (size_t)sd.num_instances);
    for (uint32_t i = 0; i < sd.num_instances; i++)
        std::memcpy(&m_to_world[12 * (size_t)i], sd.instances[i].to_world, 12 * sizeof(float));
    m_prev_to_world.clear();
    m_instances_moved = m_device_moved = false;
    m_have_cam = false;
    m_dirty = true;
    // the engine creates every instance visible: instances hidden before the scene was set
    std::vector<uint32_t> hidden, zero;
    for (uint32_t i = 0; i < sd.num_instances; i++)
        if ((world->InstanceVisibility(i) & 0xFFu) == 0u) hidden.push_back(i);
    zero.assign(hidden.size(), 0u);
    if (!hidden.empty() && pupil_pt_update_instances_masked(m_engine, (uint32_t)hidden.size(), hidden.data(), nullptr,
                                                            nullptr, zero.data()) != PUPIL_OK)
        Log("%s: instance visibility failed: %s", name.c_str(), pupil_last_error());
}

bool PTPass::ComputeMotionVectors() noexcept {
    if (!m_engine || !m_have_cam) return false;
    auto *bm = BufferManager::instance();
    Buffer *mv = bm->GetBuffer("motion vector");
    FrameGather *gather = util::Singleton<System>::instance()->Gather();
    if (!mv) {
        BufferDesc desc;
        desc.name = "motion vector";
        desc.width = gather ? std::max(1u, gather->LocalPixels()) : (uint32_t)m_world->scene->sensor.film.w;
        desc.height = gather ? 1u : (uint32_t)m_world->scene->sensor.film.h;
        desc.stride_in_byte = sizeof(float) * 2;
        mv = bm->AllocBuffer(desc);
        if (!mv) return false;
    }
    const float *prev_tw = m_instances_moved && m_prev_to_world.size() == m_to_world.size() && !m_to_world.empty()
                               ? m_prev_to_world.data()
                               : nullptr;
    const uint32_t tile = gather ? gather->Info().tile : 0u, rank = gather ? (uint32_t)gather->Info().rank : 0u,
                   world = gather ? (uint32_t)gather->Info().world : 1u;
    if (pupil_pt_motion_vectors(m_engine, m_cam[1][0], m_cam[1][1], prev_tw, mv->cuda_ptr, gather ? 1u : 0u, tile,
                                rank, world, m_stream) != PUPIL_OK) {
        Log("%s: motion vectors failed: %s", name.c_str(), pupil_last_error());
        return false;
    }
    return hipStreamSynchronize(m_stream) == hipSuccess;
}

bool PTPass::QueryRays(uint32_t n, const void *rays_device, const pupil_ray_hits &out, bool any_hit,
                       void *stream) noexcept {
    if (!m_engine) return false;
    if (pupil_pt_query_rays(m_engine, n, rays_device, any_hit ? (uint32_t)PUPIL_QUERY_ANY_HIT : 0u, &out, stream) !=
        PUPIL_OK) {
        Log("%s: ray query failed: %s", name.c_str(), pupil_last_error());
        return false;
    }
    return true;
}

bool PTPass::RadianceRays(uint32_t n, const void *rays_device, const pupil_ray_radiance &out, uint32_t spp,
                          uint32_t seed, const uint32_t *stream_ids_device, uint32_t sample_cnt, bool accumulate,
                          uint32_t max_depth, void *stream) noexcept {
    if (!m_engine) return false;
    pupil_pt_launch launch{};
    launch.random_seed = seed;
    launch.sample_cnt = sample_cnt;
    launch.spp = spp;
    launch.max_depth = max_depth;
    launch.accumulate = accumulate ? 1u : 0u;
    if (pupil_pt_radiance_rays(m_engine, n, rays_device, stream_ids_device, &launch, &out, stream) != PUPIL_OK) {
        Log("%s: radiance along rays failed: %s", name.c_str(), pupil_last_error());
        return false;
    }
    return true;
}

bool PTPass::QueryCamera(const pupil_ray_hits &out, float jitter_x, float jitter_y, void *rays_out_device) noexcept {
    if (!m_engine) return false;
    FrameGather *gather = util::Singleton<System>::instance()->Gather();
    const uint32_t tile = gather ? gather->Info().tile : 0u, rank = gather ? (uint32_t)gather->Info().rank : 0u,
                   world = gather ? (uint32_t)gather->Info().world : 1u;
    if (pupil_pt_query_camera(m_engine, jitter_x, jitter_y, gather ? 1u : 0u, tile, rank, world, rays_out_device, &out,
                              m_stream) != PUPIL_OK) {
        Log("%s: camera query failed: %s", name.c_str(), pupil_last_error());
        return false;
    }
    return true;
}

void PTPass::SetMaxDepth(int depth) noexcept {
    depth = std::clamp(depth, 1, 128);  // Inspector clamp, pt_pass.cpp:229
    if (depth != m_max_depth) {
        m_max_depth = depth;
        m_dirty = true;
    }
}

void PTPass::SetAccumulate(bool on) noexcept {
    if (on != m_accumulated_flag) {
        m_accumulated_flag = on;
        m_dirty = true;
    }
}

void PTPass::UpdateShape(uint32_t shape) noexcept {
    {
        std::scoped_lock lock(m_pending_mutex);
        if (std::find(m_pending_shapes.begin(), m_pending_shapes.end(), shape) == m_pending_shapes.end())
            m_pending_shapes.push_back(shape);
    }
    m_dirty = true;
}

void PTPass::SetKeepPreviousVertices(bool on) noexcept { m_keep_prev_verts = on; }

bool PTPass::SetDeviceEmitters(bool on) noexcept {
    if (!m_engine || !m_world) return false;
    std::scoped_lock lock(m_world->Mutex());
    if (pupil_pt_enable_device_emitters(m_engine, on ? &m_world->Desc() : nullptr) != PUPIL_OK) {
        Log("%s: device emitters: %s", name.c_str(), pupil_last_error());
        return false;
    }
    m_device_emitters = on;
    m_dirty = true;
    return true;
}

bool PTPass::UpdateLights() noexcept {
    if (!m_engine || !m_world) return false;
    std::scoped_lock lock(m_world->Mutex());
    if (pupil_pt_update_emitters(m_engine, &m_world->Desc()) != PUPIL_OK) {
        Log("%s: light update failed: %s", name.c_str(), pupil_last_error());
        return false;
    }
    m_dirty = true;
    return true;
}

bool PTPass::UpdateMaterials(const std::vector<uint32_t> &ids) noexcept {
    if (!m_engine || !m_world) return false;
    if (ids.empty()) return true;
    std::scoped_lock lock(m_world->Mutex());
    const pupil_scene_desc &d = m_world->Desc();
    std::vector<pupil_material> mats;
    mats.reserve(ids.size());
    for (uint32_t id : ids) {
        if (id >= d.num_materials) {
            Log("%s: material update failed: material index out of range", name.c_str());
            return false;
        }
        mats.push_back(d.materials[id]);
    }
    if (pupil_pt_update_materials(m_engine, (uint32_t)ids.size(), ids.data(), mats.data()) != PUPIL_OK) {
        Log("%s: material update failed: %s", name.c_str(), pupil_last_error());
        return false;
    }
    m_dirty = true;
    return true;
}

bool PTPass::UpdateTextureDevice(uint32_t material, uint32_t slot, const void *rgba_device, uint32_t width,
                                 uint32_t height, hipStream_t stream) noexcept {
    if (!m_engine) return false;
    if (pupil_pt_update_texture_device(m_engine, material, slot, rgba_device, width, height, stream) != PUPIL_OK) {
        Log("%s: texture update failed: %s", name.c_str(), pupil_last_error());
        return false;
    }
    m_dirty = true;
    return true;
}

bool PTPass::UpdateEnvDevice(const void *rgba_device, uint32_t width, uint32_t height, void *stream) noexcept {
    if (!m_engine) return false;
    if (pupil_pt_update_env_device(m_engine, rgba_device, width, height, stream) != PUPIL_OK) {
        Log("%s: env map update failed: %s", name.c_str(), pupil_last_error());
        return false;
    }
    m_dirty = true;
    return true;
}

bool PTPass::UpdateInstancesDevice(uint32_t n, const uint32_t *ids_device, const void *to_world_device,
                                   const void *to_object_device, void *stream) noexcept {
    if (!m_engine) return false;
    if (pupil_pt_update_instances_device(m_engine, n, ids_device, to_world_device, to_object_device, stream) != PUPIL_OK) {
        Log("%s: device instance update failed: %s", name.c_str(), pupil_last_error());
        return false;
    }
    if (n && !m_to_world.empty()) {  // the flow of the next OnRun covers the move: the first "before" stays
        if (!m_device_moved) m_prev_to_world = m_to_world;
        m_device_moved = true;
        pupil_pt_get_instance_transforms(m_engine, 0, (uint32_t)(m_to_world.size() / 12), m_to_world.data(), nullptr);
    }
    m_dirty = true;
    return true;
}

bool PTPass::ReplaceShapeMesh(uint32_t shape, const pupil_shape &mesh, bool device, void *stream) noexcept {
    if (!m_engine) return false;
    if (pupil_pt_replace_shape_mesh(m_engine, shape, &mesh, device ? (uint32_t)PUPIL_VERTS_DEVICE : 0u, stream) !=
        PUPIL_OK) {
        Log("%s: mesh replacement failed: %s", name.c_str(), pupil_last_error());
        return false;
    }
    {
        std::scoped_lock lock(m_pending_mutex);
        m_pending_shapes.erase(std::remove(m_pending_shapes.begin(), m_pending_shapes.end(), shape), m_pending_shapes.end());
    }
    m_dirty = true;
    return true;
}

bool PTPass::SetInstances(uint32_t n, const pupil_instance *instances, const uint32_t *visibility_mask,
                          const void *to_world_device, void *stream) noexcept {
    if (!m_engine) return false;
    const uint32_t flags = to_world_device ? (uint32_t)PUPIL_INSTANCES_DEVICE : 0u;
    int rc;
    uint32_t has_env = 0;
    std::unique_lock<std::mutex> lock;
    if (m_world) lock = std::unique_lock<std::mutex>(m_world->Mutex());
    // the emissive set is free when the world describes the engine's emitter table (the same env
    // presence); else -- the emitters were set from another description -- the old entry keeps it
    if (m_device_emitters && m_world && pupil_pt_emitter_table_info(m_engine, nullptr, nullptr, &has_env) == PUPIL_OK &&
        (has_env != 0u) == (m_world->Desc().env != nullptr && m_world->Desc().env->type != PUPIL_EMITTER_NONE)) {
        pupil_scene_desc d = m_world->Desc();
        d.instances = instances;
        d.num_instances = n;
        rc = pupil_pt_set_instances_emitters(m_engine, &d, visibility_mask, to_world_device, flags, stream);
    } else {
        rc = pupil_pt_set_instances(m_engine, n, instances, visibility_mask, to_world_device, flags, stream);
    }
    if (rc != PUPIL_OK) {
        Log("%s: instance table update failed: %s", name.c_str(), pupil_last_error());
        return false;
    }
    {
        std::scoped_lock lock(m_pending_mutex);  // recorded moves name instances of the old table
        m_pending.clear();
    }
    m_to_world.assign(12 * (size_t)n, 0.f);
    pupil_pt_get_instance_transforms(m_engine, 0, n, m_to_world.data(), nullptr);
    m_prev_to_world.clear();
    m_instances_moved = false;
    m_device_moved = false;
    m_dirty = true;
    return true;
}

bool PTPass::UpdateEnvParams(float scale, const float to_world[9]) noexcept {
    if (!m_engine || !to_world) return false;
    float to_local[9];
    if (pupil_world_invert3x3(to_world, to_local) != PUPIL_OK ||
        pupil_pt_update_env_params(m_engine, scale, to_world, to_local) != PUPIL_OK) {
        Log("%s: env parameter update failed: %s", name.c_str(), pupil_last_error());
        return false;
    }
    m_dirty = true;
    return true;
}

bool PTPass::Stats(pupil_pt_counters &out) noexcept { return m_engine && pupil_pt_stats(m_engine, &out) == PUPIL_OK; }

void PTPass::BindingEventCallback() noexcept {
    EventBinder<EWorldEvent::CameraChange>([this](void *) { m_dirty = true; });
    EventBinder<EWorldEvent::RenderInstanceUpdate>([this](void *p) {
        // only recorded: the next OnRun refits once for every instance moved since the last
        // (ias_manager.cpp:116-151, world.cpp:45-54) and restarts accumulation
        const auto *u = static_cast<const world::InstanceUpdate *>(p);
        if (u && u->world == m_world && u->shape != 0xFFFFFFFFu) {
            UpdateShape(u->shape);
            return;
        }
        if (u && u->world == m_world) {
            std::scoped_lock lock(m_pending_mutex);
            if (std::find(m_pending.begin(), m_pending.end(), u->instance) == m_pending.end())
                m_pending.push_back(u->instance);
        }
        m_dirty = true;
    });
    EventBinder<ESystemEvent::SceneLoad>([this](void *p) { SetScene(static_cast<world::World *>(p)); });
}

void PTPass::Inspector() noexcept {
    Pass::Inspector();
    Log("  sample count: %u, max trace depth: %d, accumulate radiance: %s", m_sample_cnt + 1, m_max_depth,
        m_accumulated_flag ? "on" : "off");
}

}  // namespace Pupil::pt
