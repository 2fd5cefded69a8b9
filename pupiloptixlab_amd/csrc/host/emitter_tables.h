// emitter_tables.h — EmitterTables, the one owner of the emitter state.  Plain C++ (no
// HIP): the device is a policy, as in host/scene_tables.h, so the ownership paths run on the host under
// a sanitizer (tests/emitter_tables_driver.cpp).  Dev::alloc / free / Stream, and, each -> ABI code,
//   Dev::upload(dst, src, bytes) -> status: a synchronous copy      Dev::failed(status, what): HIP_TRY's text
//   Dev::write(dst, src, bytes, stream): an enqueued copy           Dev::sync(stream): the stream passed
//   Dev::env_tables(h_env, rgba, sums, d_env, stream): the env map's texels and tables (pt_envmap.hip), enqueued
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "../pt_scene.h"
#include "scoped_buffer.h"

namespace pupil {

int fail(int code, const std::string &msg);  // engine.hip: the code, msg left for pupil_last_error

// everything of a texture but its texels (data stays null); refuses what no engine can sample
inline int texture_desc(const pupil_texture &t, DevTexture &d) {
    std::memset(&d, 0, sizeof(d));
    d.type = t.type;
    d.width = t.width;
    d.height = t.height;
    d.filter = t.filter;
    for (int k = 0; k < 3; k++) {
        d.c0[k] = t.c0[k];
        d.c1[k] = t.c1[k];
    }
    for (int k = 0; k < 4; k++) {
        d.r0[k] = t.transform[k];
        d.r1[k] = t.transform[4 + k];
    }
    if (t.type == PUPIL_TEX_BITMAP) {
        if (!t.rgba || !t.width || !t.height) return fail(PUPIL_ERR_INVALID, "bitmap texture without texels");
    } else if (t.type > PUPIL_TEX_CHECKERBOARD) {
        return fail(PUPIL_ERR_INVALID, "unknown texture type");
    }
    return PUPIL_OK;
}

// EnvMap::Eval (env.h:58-62) lerps row_weight[row], row_weight[row + 1] with row <= h - 2,
// and SampleDirect's column walk ends at w - 1: neither is defined for a one-texel side
inline bool env_map_size_ok(uint32_t w, uint32_t h) { return w >= 2 && h >= 2; }

// The table's shape: each entry's type, and the number of triangle and sphere emitters in front, in
// SelectOneEmiiter's scan order (render/emitter.h:110-135): areas, points (point and spot), directionals.
inline int emitter_table_shape(const pupil_scene_desc *scene, std::vector<uint32_t> &types, uint32_t &true_areas) {
    types.resize(scene->num_area_emitters);
    true_areas = 0;
    uint32_t stage = 0;  // 0 areas, 1 points, 2 directionals
    for (uint32_t e = 0; e < scene->num_area_emitters; e++) {
        const uint32_t t = scene->area_emitters[e].type;
        uint32_t s;
        if (t == PUPIL_EMITTER_TRI_AREA || t == PUPIL_EMITTER_SPHERE) s = 0;
        else if (t == PUPIL_EMITTER_POINT || t == PUPIL_EMITTER_SPOT) s = 1;
        else if (t == PUPIL_EMITTER_DIRECTIONAL) s = 2;
        else return fail(PUPIL_ERR_INVALID, "emitter table entry of an unknown or env type");
        if (s < stage) return fail(PUPIL_ERR_INVALID, "emitter table out of order: areas, point / spot, directional");
        stage = s;
        true_areas += s == 0 ? 1u : 0u;
        types[e] = t;
    }
    return PUPIL_OK;
}

// One generation of the tables, a value: moving one over another frees what the old one owned.
template <typename Dev>
struct EmitterGeneration {
    ScopedBuffer<DevEmitter, Dev> areas, env;  // types.size() records; the env record or none
    ScopedBuffer<float, Dev> cdf;
    ScopedBuffer<uint32_t, Dev> guide;  // 2^guide_bits + 1 entries, or none (plain binary search)
    std::vector<ScopedBuffer<float, Dev>> texels;  // what the records point at: bitmap radiances, the env block
    // each entry's type: the triangle and sphere emitters [0, num_true_areas), then the delta lights
    std::vector<uint32_t> types;
    uint32_t guide_bits = 0, num_true_areas = 0;
    pupil_emitter env_src{};  // the env emitter the tables were built from
    DevEmitter h_env{};       // the host mirror of *env as staged
    bool env_src_valid = false, env_stale = false;  // env_stale: write_env_* ran, env_src no longer describes the device
};

// The device-side mode's bookkeeping (pupil_pt_enable_device_emitters), a value of the same kind: per
// emitter its instance, per instance its radiance's select weight, the rebuild's scratch (pt_emitters.hip)
template <typename Dev>
struct EmitterBookkeeping {
    ScopedBuffer<uint32_t, Dev> emit_inst;                      // count entries, the true areas' filled
    ScopedBuffer<float, Dev> inst_weight, weight, select, sum;  // instances, count, count, 1
    std::vector<uint32_t> h_emit_inst;  // the host's copies, which a new instance table re-indexes
    std::vector<float> h_inst_weight;
    bool enabled = false;
    uint32_t count = 0;  // emitters the arrays were sized for: the whole table, delta lights too

    // the "aside" step: after a failure `out` frees what it took, nothing else has changed
    static int stage(std::vector<uint32_t> emit_inst, std::vector<float> inst_weight, uint32_t count, EmitterBookkeeping &out,
                     const char *oom = "emitter bookkeeping allocation failed") {
        if (out.emit_inst.alloc(count) || out.weight.alloc(count) || out.select.alloc(count) ||
            out.inst_weight.alloc(inst_weight.size()) || out.sum.alloc(1))
            return fail(PUPIL_ERR_OOM, oom);
        if (!emit_inst.empty())
            if (const auto e = Dev::upload(out.emit_inst.get(), emit_inst.data(), sizeof(uint32_t) * emit_inst.size()))
                return Dev::failed(e, "hipMemcpy(pt->d_emit_inst, emit_inst.data(), sizeof(uint32_t) * emit_inst.size(), hipMemcpyHostToDevice)");
        if (const auto e = Dev::upload(out.inst_weight.get(), inst_weight.data(), sizeof(float) * inst_weight.size()))
            return Dev::failed(e, "hipMemcpy(pt->d_inst_weight, inst_weight.data(), sizeof(float) * inst_weight.size(), hipMemcpyHostToDevice)");
        out.h_emit_inst = std::move(emit_inst);
        out.h_inst_weight = std::move(inst_weight);
        out.count = count;
        return PUPIL_OK;
    }
    // this bookkeeping under a new table of n instances, where emissive instance from[k] is to[k]
    int restage(const std::vector<uint32_t> &from, const std::vector<uint32_t> &to, uint32_t n, EmitterBookkeeping &out,
                const char *oom) const {
        std::vector<uint32_t> to_new(h_inst_weight.size(), 0u), emit = h_emit_inst;
        std::vector<float> w(n, 0.f);
        for (size_t k = 0; k < from.size(); k++) to_new[from[k]] = to[k], w[to[k]] = h_inst_weight[from[k]];
        for (uint32_t &e : emit) e = to_new[e];
        out.enabled = enabled;
        return stage(std::move(emit), std::move(w), count, out, oom);
    }
};

// One emissive instance of a table that is being resized (EmitterTables::stage_resize), in instance
// order: its index in the new instance table, its emitter range, the select weight of its radiance,
// and the radiance itself -- that of record `kept` of the current table (its texels are moved, not
// uploaded again), or, kept < 0, `radiance`, whose bitmap is uploaded once
struct EmitterSource {
    uint32_t inst = 0, offset = 0, range = 0;
    uint32_t type = PUPIL_EMITTER_TRI_AREA;  // or PUPIL_EMITTER_SPHERE (range 1)
    float weight = 0.f;
    int64_t kept = -1;
    pupil_texture radiance{};
};

// A resized table, staged: the generation and the bookkeeping sized for the new count, built aside.
// The records of gen.areas are filled on the device (pt_emitters.hip: k_emit_fill from `sources`,
// then the five stages) but for the delta lights' at [num_true_areas, total), which are staged here.
template <typename Dev>
struct EmitterResize {
    EmitterGeneration<Dev> gen;
    EmitterBookkeeping<Dev> book;
    ScopedBuffer<DevEmitSource, Dev> sources;  // the fill kernel's input; goes with the call
    uint32_t num_sources = 0;
    std::vector<const float *> moved;  // texels of the current generation that gen's records point at: they move at adoption
};

template <typename Dev>
class EmitterTables {
public:
    using Generation = EmitterGeneration<Dev>;
    using Bookkeeping = EmitterBookkeeping<Dev>;
    using Resize = EmitterResize<Dev>;
    using Texels = std::vector<ScopedBuffer<float, Dev>>;

    // The "aside" step of a resize (device-side mode).  sources: the emissive instances of the new
    // table of n_instances, their ranges following each other from 0.  deltas: the delta lights
    // behind them, or, keep_deltas: those of the current generation, copied on the device.  The env record
    // carries over (its own copy, with the select probability of the new count); its texels and
    // tables move at adoption.  Also needs Dev::download(dst, src, bytes) and Dev::copy(dst, src,
    // bytes), synchronous like Dev::upload.  After a failure `out` frees what it took; nothing the
    // engine reads has changed, and no texel has left the current generation.
    int stage_resize(const std::vector<EmitterSource> &sources, uint32_t n_instances, const pupil_emitter *deltas,
                     uint32_t num_deltas, bool keep_deltas, Resize &out) {
        Generation &g = out.gen;
        std::vector<DevEmitSource> dev(sources.size());
        std::vector<float> inst_weight(n_instances, 0.f);
        std::vector<uint32_t> emit_inst;
        g.types.clear();
        for (size_t k = 0; k < sources.size(); k++) {
            const EmitterSource &s = sources[k];
            if (s.offset != g.types.size() || s.range == 0 || s.inst >= n_instances)
                return fail(PUPIL_ERR_INVALID, "emitter ranges do not follow each other in instance order");
            DevEmitter rec{};
            if (s.kept >= 0) {
                if ((uint64_t)s.kept >= cur_.num_true_areas) return fail(PUPIL_ERR_INVALID, "kept emitter out of range");
                if (const auto e = Dev::download(&rec, cur_.areas.get() + s.kept, sizeof(rec)))
                    return Dev::failed(e, "download(record, areas + kept, sizeof(DevEmitter))");
                if (rec.radiance.data && !keep(reinterpret_cast<const float *>(rec.radiance.data), out.moved))
                    return fail(PUPIL_ERR_INVALID, "kept emitter's texels are not the current generation's");
            } else {
                if (const int rc = texture_desc(s.radiance, rec.radiance)) return rc;
                if (s.radiance.type == PUPIL_TEX_BITMAP) {
                    g.texels.emplace_back();
                    if (const auto e = put(g.texels.back(), s.radiance.rgba, 4 * (size_t)s.radiance.width * s.radiance.height))
                        return Dev::failed(e, "upload(texels, t.rgba, 4 * t.width * t.height)");
                    rec.radiance.data = reinterpret_cast<const float4 *>(g.texels.back().get());
                }
            }
            dev[k] = DevEmitSource{s.inst, s.offset, rec.radiance};
            inst_weight[s.inst] = s.weight;
            g.types.insert(g.types.end(), s.range, s.type);
            emit_inst.insert(emit_inst.end(), s.range, s.inst);
        }
        g.num_true_areas = (uint32_t)g.types.size();
        const uint32_t old_deltas = (uint32_t)cur_.types.size() - cur_.num_true_areas;
        if (!keep_deltas) {
            for (uint32_t k = 0; k < num_deltas; k++) g.types.push_back(deltas[k].type);
        } else {
            num_deltas = old_deltas;
            g.types.insert(g.types.end(), cur_.types.begin() + cur_.num_true_areas, cur_.types.end());
        }
        const uint32_t total = (uint32_t)g.types.size();
        g.guide_bits = 0;
        while ((1u << g.guide_bits) < total && g.guide_bits < 20) g.guide_bits++;
        const char *sel = std::getenv("PUPIL_EMITTER_SELECT");
        const bool guide = total > 1 && !(sel && std::strcmp(sel, "binary") == 0);  // as emitter_tables()
        if (g.areas.alloc(total) || g.cdf.alloc(total) || (guide && g.guide.alloc((1u << g.guide_bits) + 1u)))
            return fail(PUPIL_ERR_OOM, "emitter table allocation failed");
        if (out.sources.alloc(dev.size())) return fail(PUPIL_ERR_OOM, "emitter table allocation failed");
        out.num_sources = (uint32_t)dev.size();
        if (!dev.empty())
            if (const auto e = Dev::upload(out.sources.get(), dev.data(), sizeof(DevEmitSource) * dev.size()))
                return Dev::failed(e, "upload(sources, dev.data(), sizeof(DevEmitSource) * dev.size())");
        if (!keep_deltas && num_deltas) {
            std::vector<DevEmitter> recs(num_deltas);
            for (uint32_t k = 0; k < num_deltas; k++)
                if (const int rc = convert_emitter(deltas[k], recs[k], g.texels)) return rc;
            if (const auto e = Dev::upload(g.areas.get() + g.num_true_areas, recs.data(), sizeof(DevEmitter) * num_deltas))
                return Dev::failed(e, "upload(areas + num_true_areas, recs.data(), sizeof(DevEmitter) * num_deltas)");
        } else if (num_deltas) {
            if (const auto e = Dev::copy(g.areas.get() + g.num_true_areas, cur_.areas.get() + cur_.num_true_areas,
                                         sizeof(DevEmitter) * num_deltas))
                return Dev::failed(e, "copy(areas + num_true_areas, cur.areas + cur.num_true_areas, sizeof(DevEmitter) * num_deltas)");
        }
        if (cur_.env.get()) {  // its own record: ComputeProbability's env weight / emitter_num under the new count
            g.h_env = cur_.h_env;
            g.env_src = cur_.env_src;
            g.env_src_valid = cur_.env_src_valid, g.env_stale = cur_.env_stale;
            g.h_env.select_probability = g.env_src.select_probability = 1.f / (float)((size_t)total + 1);
            if (g.env.alloc(1)) return fail(PUPIL_ERR_OOM, "env allocation failed");
            // from the device: the table kernels write the env map's normalization there, not into h_env
            if (const auto e = Dev::copy(g.env.get(), cur_.env.get(), sizeof(DevEmitter)))
                return Dev::failed(e, "copy(env, cur.env, sizeof(DevEmitter))");
            if (const auto e = Dev::upload(&g.env.get()->select_probability, &g.h_env.select_probability, sizeof(float)))
                return Dev::failed(e, "upload(&env->select_probability, &h_env.select_probability, sizeof(float))");
            keep(reinterpret_cast<const float *>(g.h_env.radiance.data), out.moved);
            keep(g.h_env.col_cdf, out.moved);
        }
        g.texels.reserve(g.texels.size() + out.moved.size());  // adoption allocates nothing
        out.book.enabled = true;
        if (const int rc = Bookkeeping::stage({}, std::move(inst_weight), total, out.book)) return rc;
        out.book.h_emit_inst = std::move(emit_inst);  // the device's copy is k_emit_fill's
        return PUPIL_OK;
    }

    // the swap of a resize: the texels the staged records share with the current generation move
    // over, everything else of the current generation and the old bookkeeping is freed
    void adopt_resize(Resize &&staged, DeviceScene &sc) {
        for (const float *p : staged.moved)
            for (auto &t : cur_.texels)
                if (t.get() == p) staged.gen.texels.push_back(std::move(t));
        adopt(std::move(staged.gen), sc);
        book_ = std::move(staged.book);
    }

    // The "aside" step: the tables derived once, into the staging vectors, and uploaded into `out`, which
    // frees what it took after a failure; nothing the engine reads changes.  With `fits`: tables that keep
    // the current shape (entry types, no bitmap radiance, the env, the guide) stay in the staging vectors.
    int stage(const pupil_scene_desc *scene, Generation &out, bool *fits = nullptr) {
        if (const int rc = emitter_table_shape(scene, out.types, out.num_true_areas)) return rc;
        const bool env = scene->env && scene->env->type != PUPIL_EMITTER_NONE;
        bool same = fits && cur_.areas.get() && out.types == cur_.types && env == cur_.env_src_valid && !cur_.env_stale &&
                    (!env || std::memcmp(&cur_.env_src, scene->env, sizeof(pupil_emitter)) == 0);
        for (uint32_t e = 0; same && e < scene->num_area_emitters; e++)
            same = scene->area_emitters[e].radiance.type != PUPIL_TEX_BITMAP;
        if (const int rc = emitter_tables(scene, out.texels, h_areas_, h_cdf_, h_guide_, out.guide_bits)) return rc;
        if (same && h_guide_.empty() == !cur_.guide.get() && out.guide_bits == cur_.guide_bits) {
            *fits = true;
            return PUPIL_OK;
        }
        if (put(out.areas, h_areas_.data(), h_areas_.size()) || put(out.cdf, h_cdf_.data(), h_cdf_.size()))
            return fail(PUPIL_ERR_OOM, "emitter upload failed");
        if (!h_guide_.empty() && put(out.guide, h_guide_.data(), h_guide_.size()))
            return fail(PUPIL_ERR_OOM, "emitter guide upload failed");
        if (env) {
            if (const int rc = convert_emitter(*scene->env, out.h_env, out.texels)) return rc;
            if (put(out.env, &out.h_env, 1)) return fail(PUPIL_ERR_OOM, "env upload failed");
            out.env_src = *scene->env;
            out.env_src_valid = true;
        }
        return PUPIL_OK;
    }

    // the swap, and the only writer of these fields of DeviceScene: the previous generation is freed
    void adopt(Generation &&staged, DeviceScene &sc) {
        cur_ = std::move(staged);
        sc.areas = cur_.areas.get();
        sc.area_cdf = cur_.cdf.get();
        sc.area_guide = cur_.guide.get();
        sc.guide_bits = cur_.guide_bits;
        sc.num_areas = (uint32_t)cur_.types.size();
        sc.has_env = cur_.env.get() ? 1u : 0u;
        sc.env = cur_.env.get();
    }

    // the tables written through the current generation behind the stream when they fit, else staged and
    // adopted once the stream has passed what reads the old one; a refusal changes nothing
    int update(const pupil_scene_desc *scene, typename Dev::Stream stream, DeviceScene &sc) {
        Generation staged;
        bool fits = false;
        int rc = stage(scene, staged, &fits);
        if (!rc && fits) rc = Dev::write(cur_.areas.get(), h_areas_.data(), sizeof(DevEmitter) * h_areas_.size(), stream);
        if (!rc && fits) rc = Dev::write(cur_.cdf.get(), h_cdf_.data(), sizeof(float) * h_cdf_.size(), stream);
        if (!rc && fits && cur_.guide.get()) rc = Dev::write(cur_.guide.get(), h_guide_.data(), sizeof(uint32_t) * h_guide_.size(), stream);
        if (!rc) rc = Dev::sync(stream);
        if (!rc && !fits) adopt(std::move(staged), sc);
        return rc;
    }

    const Generation &cur() const { return cur_; }
    Bookkeeping &book() { return book_; }  // replaced as a whole: book() = std::move(staged)

    // the engine holds an env map (not a constant env, not none) the two writers below can rewrite
    int env_map_held() const {
        const DevEmitter &e = cur_.h_env;
        if (!cur_.env.get() || e.type != PUPIL_EMITTER_ENV_MAP || !e.radiance.data || !e.col_cdf)
            return fail(PUPIL_ERR_INVALID, "the scene has no env map: give it one with pupil_pt_update_emitters first");
        return PUPIL_OK;
    }
    // everything that can refuse new texels, the row-sum scratch (first call, or the map grew) included
    int reserve_env_texels(uint32_t width, uint32_t height) {
        if (const int rc = env_map_held()) return rc;
        const DevEmitter &e = cur_.h_env;
        if (e.map_w != width || e.map_h != height)
            return fail(PUPIL_ERR_INVALID, "the env map is " + std::to_string(e.map_w) + " x " + std::to_string(e.map_h) +
                                               ": set the size with pupil_pt_update_emitters first");
        if (env_sums_cap_ < height) {  // no kernel reads the old one: every call returns behind its own
            env_sums_cap_ = 0;
            if (env_sums_.alloc(height)) return fail(PUPIL_ERR_OOM, "env scratch allocation failed");
            env_sums_cap_ = height;
        }
        return PUPIL_OK;
    }
    // the reserved texels from device memory, behind the stream: the tables are rewritten in place
    int write_env_texels(const void *rgba_device, typename Dev::Stream stream) {
        cur_.env_stale = true;
        const int rc = Dev::env_tables(cur_.h_env, rgba_device, env_sums_.get(), cur_.env.get(), stream);
        return rc ? rc : Dev::sync(stream);
    }
    // scale, to_world and to_local of the device's env emitter: two small copies, no table, no texel
    int write_env_params(float scale, const float to_world[9], const float to_local[9], typename Dev::Stream stream) {
        static_assert(offsetof(DevEmitter, to_local) == offsetof(DevEmitter, to_world) + 9 * sizeof(float), "one copy");
        cur_.env_stale = true;
        DevEmitter &e = cur_.h_env, *d = cur_.env.get();  // e outlives the copies
        e.scale = scale;
        std::memcpy(e.to_world, to_world, sizeof(e.to_world));
        std::memcpy(e.to_local, to_local, sizeof(e.to_local));
        int rc = Dev::write(&d->scale, &e.scale, sizeof(float), stream);
        if (!rc) rc = Dev::write(d->to_world, e.to_world, sizeof(e.to_world) + sizeof(e.to_local), stream);
        return rc ? rc : Dev::sync(stream);
    }

    // EmitterGroup (render/emitter.h:110-135): the area emitters, their sequential selection CDF and its
    // guide (pt_scene.h area_guide; <= 2^20 buckets; none for PUPIL_EMITTER_SELECT=binary or < 2 emitters)
    static int emitter_tables(const pupil_scene_desc *scene, Texels &texels, std::vector<DevEmitter> &areas,
                              std::vector<float> &cdf, std::vector<uint32_t> &guide, uint32_t &bits) {
        areas.assign(scene->num_area_emitters, DevEmitter{});
        cdf.assign(scene->num_area_emitters, 0.f);
        float sum_p = 0.f;
        for (uint32_t e = 0; e < scene->num_area_emitters; e++) {
            if (const int rc = convert_emitter(scene->area_emitters[e], areas[e], texels)) return rc;
            cdf[e] = sum_p + areas[e].select_probability;
            sum_p = cdf[e];
        }
        bits = 0;
        while ((1u << bits) < scene->num_area_emitters && bits < 20) bits++;
        const char *sel = std::getenv("PUPIL_EMITTER_SELECT");
        guide.clear();
        if (scene->num_area_emitters > 1 && !(sel && std::strcmp(sel, "binary") == 0)) {
            const uint32_t m = 1u << bits;
            guide.resize(m + 1);
            uint32_t i = 0;
            for (uint32_t k = 0; k <= m; k++) {
                const float t = (float)k / (float)m;
                while (i < cdf.size() && cdf[i] < t) i++;
                guide[k] = i;
            }
        }
        return PUPIL_OK;
    }

private:
    // p is an allocation of the current generation's texels: listed once in `moved`
    bool keep(const float *p, std::vector<const float *> &moved) const {
        for (const auto &t : cur_.texels)
            if (p && t.get() == p) {
                if (std::find(moved.begin(), moved.end(), p) == moved.end()) moved.push_back(p);
                return true;
            }
        return false;
    }

    template <typename T>
    static auto put(ScopedBuffer<T, Dev> &b, const T *src, size_t count) {
        auto e = b.alloc(count);
        if (!e && count) e = Dev::upload(b.get(), src, sizeof(T) * count);
        return e;
    }

    static int convert_emitter(const pupil_emitter &e, DevEmitter &d, Texels &texels) {
        std::memset(&d, 0, sizeof(d));
        d.type = e.type;
        d.select_probability = e.select_probability;
        d.area = e.area;
        d.radius = e.radius;
        const pupil_texture &t = e.radiance;
        if (const int rc = texture_desc(t, d.radiance)) return rc;
        if (t.type == PUPIL_TEX_BITMAP) {
            texels.emplace_back();
            if (const auto s = put(texels.back(), t.rgba, 4 * (size_t)t.width * t.height))
                return Dev::failed(s, "upload(texels, t.rgba, 4 * t.width * t.height)");
            d.radiance.data = reinterpret_cast<const float4 *>(texels.back().get());
        }
        for (int k = 0; k < 3; k++) {
            d.pos[k] = v3(e.pos[k][0], e.pos[k][1], e.pos[k][2]);
            d.nrm[k] = v3(e.nrm[k][0], e.nrm[k][1], e.nrm[k][2]);
            d.tex[k] = v2(e.tex[k][0], e.tex[k][1]);
        }
        d.center = v3(e.center[0], e.center[1], e.center[2]);
        d.color = v3(e.color[0], e.color[1], e.color[2]);
        d.scale = e.scale;
        for (int k = 0; k < 9; k++) {
            d.to_world[k] = e.to_world[k];
            d.to_local[k] = e.to_local[k];
        }
        if (e.type == PUPIL_EMITTER_ENV_MAP) {
            // BuildEnvMapCdfTable (world/emitter.cpp:107-149)
            if (t.type != PUPIL_TEX_BITMAP || !t.rgba) return fail(PUPIL_ERR_INVALID, "env map needs a bitmap");
            const size_t w = t.width, h = t.height;
            if (!env_map_size_ok(t.width, t.height)) return fail(PUPIL_ERR_INVALID, "env map smaller than 2 x 2 texels");
            // col_cdf | row_cdf | row_weight | 0.0f (pt_scene.h DevEmitter), the tail >= one column walk
            const size_t tail = std::max((h + 1) + h + 1, w);
            std::vector<float> tables((w + 1) * h + tail, 0.f);
            float *col_cdf = tables.data(), *row_cdf = col_cdf + (w + 1) * h, *row_weight = row_cdf + (h + 1);
            size_t ci = 0, ri = 0;
            float row_sum = 0.f;
            row_cdf[ri++] = 0.f;
            for (size_t y = 0; y < h; ++y) {
                float col_sum = 0.f;
                col_cdf[ci++] = 0.f;
                for (size_t x = 0; x < w; ++x) {
                    const size_t pix = y * w + x;
                    col_sum += luminance(v3(t.rgba[pix * 4 + 0], t.rgba[pix * 4 + 1], t.rgba[pix * 4 + 2]));
                    col_cdf[ci++] = col_sum;
                }
                for (size_t x = 1; x < w; ++x) col_cdf[ci - x - 1] /= col_sum;
                col_cdf[ci - 1] = 1.f;
                const float weight = std::sin((y + 0.5f) * kPi / h);
                row_weight[y] = weight;
                row_sum += col_sum * weight;
                row_cdf[ri++] = row_sum;
            }
            for (size_t y = 1; y < h; ++y) row_cdf[ri - y - 1] /= row_sum;
            row_cdf[ri - 1] = 1.f;
            d.normalization = 1.f / (row_sum * (2.f * kPi / w) * (kPi / h));
            d.map_w = (uint32_t)w;
            d.map_h = (uint32_t)h;
            texels.emplace_back();
            if (const auto s = put(texels.back(), tables.data(), tables.size()))
                return Dev::failed(s, "upload(block, tables.data(), tables.size())");
            const float *block = texels.back().get();
            d.col_cdf = block;
            d.row_cdf = block + (row_cdf - col_cdf);
            d.row_weight = block + (row_weight - col_cdf);
        }
        return PUPIL_OK;
    }

    Generation cur_;
    Bookkeeping book_;
    std::vector<DevEmitter> h_areas_;  // host sources of rewrite's copies
    std::vector<float> h_cdf_;
    std::vector<uint32_t> h_guide_;
    ScopedBuffer<float, Dev> env_sums_;  // the row sums the env table kernels pass between their stages
    uint32_t env_sums_cap_ = 0;
};

}  // namespace pupil
