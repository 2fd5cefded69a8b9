// emitter_tables_driver.cpp — csrc/host/emitter_tables.h on the host: the ownership paths of the
// engine's emitter tables and of the device-side mode's bookkeeping (stage, adopt, the in-place
// writers, the failures and refusals between) with a counting allocator in place of the device,
// and the staged CDF and guide against their definition restated below.
// Built with -fsanitize=address,undefined by test_emitter_tables_host.py: every array is sized
// exactly, so a leak, a double free, a use after free or an index past an end fails the run.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

// the engine's headers name HIP's vector types in structs this driver never touches
struct float2 { float x, y; };
struct float4 { float x, y, z, w; };

#include "host/emitter_tables.h"

using namespace pupil;

static std::string g_error;
int pupil::fail(int code, const std::string &msg) {
    g_error = msg;
    return code;
}

namespace {

std::map<void *, size_t> live;  // allocation -> bytes
int allocs = 0, frees = 0, fail_at = -1, syncs = 0;

#define REQUIRE(c)                                                      \
    do {                                                                \
        if (!(c)) {                                                     \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);  \
            std::exit(1);                                               \
        }                                                               \
    } while (0)

size_t live_bytes() {
    size_t b = 0;
    for (const auto &a : live) b += a.second;
    return b;
}

struct CountingDevice {
    using Stream = int;
    static int alloc(void **p, size_t bytes) {
        if (allocs == fail_at) return 2;  // like hipErrorOutOfMemory: nothing allocated
        *p = std::malloc(bytes);
        live[*p] = bytes;
        allocs++;
        return 0;
    }
    static void free(void *p) {
        REQUIRE(live.erase(p) == 1);  // a pointer that is not live: a double free
        std::free(p);
        frees++;
    }
    static int failed(int, const char *what) { return fail(PUPIL_ERR_OOM, what); }
    static int upload(void *dst, const void *src, size_t bytes) {
        std::memcpy(dst, src, bytes);
        return 0;
    }
    static int write(void *dst, const void *src, size_t bytes, Stream) {
        std::memcpy(dst, src, bytes);
        return PUPIL_OK;
    }
    static int sync(Stream) {
        syncs++;
        return PUPIL_OK;
    }
    // the texel copy of the engine's device; the table stages are kernels, not ownership
    static int env_tables(const DevEmitter &e, const void *rgba, float *sums, DevEmitter *env, Stream) {
        std::memcpy((void *)e.radiance.data, rgba, sizeof(float4) * (size_t)e.map_w * e.map_h);
        for (uint32_t y = 0; y < e.map_h; y++) sums[y] = (float)y;  // sized for the map's rows
        env->normalization = 7.f;
        return PUPIL_OK;
    }
};
using Tables = EmitterTables<CountingDevice>;
using Generation = Tables::Generation;
using Book = Tables::Bookkeeping;

// ---- scenes: a two-triangle lamp, a sphere emitter, a point light; an env or none
const float kLamp[16] = {4.f, 3.f, 2.f, 1.f, 0.5f, 6.f, 1.f, 1.f, 2.f, 2.f, 2.f, 1.f, 0.25f, 1.f, 8.f, 1.f};  // 2 x 2
float g_env_texels[4 * 3 * 4];                                                                              // 4 x 3

pupil_texture constant(float r, float g, float b) {
    pupil_texture t{};
    t.type = PUPIL_TEX_RGB;
    t.c0[0] = r, t.c0[1] = g, t.c0[2] = b;
    return t;
}
pupil_texture bitmap(const float *rgba, uint32_t w, uint32_t h) {
    pupil_texture t{};
    t.type = PUPIL_TEX_BITMAP;
    t.width = w, t.height = h;
    t.rgba = rgba;
    return t;
}

struct Scene {
    std::vector<pupil_emitter> areas;
    pupil_emitter env{};
    pupil_scene_desc desc{};
    const pupil_scene_desc *get() {
        desc.num_area_emitters = (uint32_t)areas.size();
        desc.area_emitters = areas.data();
        desc.env = env.type != PUPIL_EMITTER_NONE ? &env : nullptr;
        return &desc;
    }
};

Scene make_scene(bool bitmap_lamp, bool env_map, float lamp_shift = 0.f) {
    Scene s;
    const uint32_t types[4] = {PUPIL_EMITTER_TRI_AREA, PUPIL_EMITTER_TRI_AREA, PUPIL_EMITTER_SPHERE, PUPIL_EMITTER_POINT};
    const float prob[4] = {0.3f, 0.2f, 0.4f, 0.1f};
    for (int k = 0; k < 4; k++) {
        pupil_emitter e{};
        e.type = types[k];
        e.weight = 1.f;
        e.select_probability = prob[k];
        e.area = 1.f + k;
        e.radiance = (k < 2 && bitmap_lamp) ? bitmap(kLamp, 2, 2) : constant(4.f, 3.f, 2.f);
        e.pos[1][0] = 1.f + lamp_shift, e.pos[2][1] = 1.f;
        e.center[0] = (float)k;
        e.radius = 0.5f;
        s.areas.push_back(e);
    }
    if (env_map) {
        s.env.type = PUPIL_EMITTER_ENV_MAP;
        s.env.weight = 1.f;
        s.env.scale = 1.f;
        s.env.radiance = bitmap(g_env_texels, 4, 3);
        s.env.to_world[0] = s.env.to_world[4] = s.env.to_world[8] = 1.f;
        s.env.to_local[0] = s.env.to_local[4] = s.env.to_local[8] = 1.f;
    }
    return s;
}

// what the engine's pupil_pt_update_emitters does with the owner
int update(Tables &t, DeviceScene &sc, const pupil_scene_desc *scene, bool *replaced = nullptr) {
    const int before = allocs;
    const int rc = t.update(scene, 0, sc);
    if (replaced) *replaced = allocs != before;  // in place: nothing is allocated
    return rc;
}

// the staged tables against their definition: the sequential CDF of select_probability, and
// guide[k] = the first i with cdf[i] >= k / 2^bits
void check_tables(const pupil_scene_desc *scene, const Generation &g) {
    const uint32_t n = scene->num_area_emitters;
    REQUIRE(g.types.size() == n && live.at(g.areas.get()) == sizeof(DevEmitter) * n && live.at(g.cdf.get()) == sizeof(float) * n);
    float sum = 0.f;
    for (uint32_t e = 0; e < n; e++) {
        sum = sum + scene->area_emitters[e].select_probability;
        REQUIRE(g.cdf.get()[e] == sum && g.types[e] == scene->area_emitters[e].type);
        const DevEmitter &d = g.areas.get()[e];
        REQUIRE(d.type == g.types[e] && d.area == scene->area_emitters[e].area);
        const pupil_texture &tex = scene->area_emitters[e].radiance;
        if (tex.type == PUPIL_TEX_BITMAP) {  // its own texels, owned by the generation
            REQUIRE(live.at((void *)d.radiance.data) == sizeof(float) * 4 * tex.width * tex.height);
            REQUIRE(std::memcmp(d.radiance.data, tex.rgba, sizeof(float) * 4 * tex.width * tex.height) == 0);
        } else {
            REQUIRE(d.radiance.data == nullptr);
        }
    }
    uint32_t bits = 0;
    while ((1u << bits) < n) bits++;
    REQUIRE(g.guide_bits == bits && g.guide.get() && live.at(g.guide.get()) == sizeof(uint32_t) * ((1u << bits) + 1u));
    for (uint32_t k = 0; k <= (1u << bits); k++) {
        uint32_t i = 0;
        while (i < n && !(g.cdf.get()[i] >= (float)k / (float)(1u << bits))) i++;
        REQUIRE(g.guide.get()[k] == i);
    }
    if (scene->env) {
        const DevEmitter &h = g.h_env;
        REQUIRE(g.env.get() && g.env_src_valid && std::memcmp(&g.env_src, scene->env, sizeof(pupil_emitter)) == 0);
        REQUIRE(std::memcmp(g.env.get(), &h, sizeof(h)) == 0 && !g.env_stale);
        if (h.type == PUPIL_EMITTER_ENV_MAP) {
            const size_t w = h.map_w, hh = h.map_h;
            REQUIRE(w == 4 && hh == 3 && live.at((void *)h.radiance.data) == sizeof(float4) * w * hh);
            REQUIRE(live.at((void *)h.col_cdf) == sizeof(float) * ((w + 1) * hh + (hh + 1) + hh + 1));
            REQUIRE(h.row_cdf == h.col_cdf + (w + 1) * hh && h.row_weight == h.row_cdf + (hh + 1));
            REQUIRE(h.row_cdf[0] == 0.f && h.row_cdf[hh] == 1.f && h.row_weight[hh] == 0.f);
        }
    } else {
        REQUIRE(!g.env.get() && !g.env_src_valid);
    }
}

// what adopt published is the generation `t` holds now
void check_published(const Tables &t, const DeviceScene &sc) {
    const Generation &g = t.cur();
    REQUIRE(sc.areas == g.areas.get() && sc.area_cdf == g.cdf.get() && sc.area_guide == g.guide.get());
    REQUIRE(sc.guide_bits == g.guide_bits && sc.num_areas == g.types.size() && sc.env == g.env.get());
    REQUIRE(sc.has_env == (g.env.get() ? 1u : 0u));
}

// a copy of everything a generation holds, the contents of its device arrays included
struct Snapshot {
    std::map<void *, std::string> memory;  // every live allocation, byte for byte
    std::vector<const void *> pointers;
    std::vector<uint32_t> types;
    uint32_t guide_bits, num_true_areas;
    std::string env_src, h_env;
    bool env_src_valid, env_stale;
    DeviceScene sc;
    bool operator==(const Snapshot &o) const {
        return memory == o.memory && pointers == o.pointers && types == o.types && guide_bits == o.guide_bits &&
               num_true_areas == o.num_true_areas && env_src == o.env_src && h_env == o.h_env &&
               env_src_valid == o.env_src_valid && env_stale == o.env_stale && std::memcmp(&sc, &o.sc, sizeof(sc)) == 0;
    }
};
Snapshot snapshot(const Generation &g, const DeviceScene &sc) {
    Snapshot s;
    for (const auto &a : live) s.memory[a.first] = std::string((const char *)a.first, a.second);
    s.pointers = {g.areas.get(), g.env.get(), g.cdf.get(), g.guide.get()};
    for (const auto &t : g.texels) s.pointers.push_back(t.get());
    s.types = g.types;
    s.guide_bits = g.guide_bits, s.num_true_areas = g.num_true_areas;
    s.env_src.assign((const char *)&g.env_src, sizeof(g.env_src));
    s.h_env.assign((const char *)&g.h_env, sizeof(g.h_env));
    s.env_src_valid = g.env_src_valid, s.env_stale = g.env_stale;
    s.sc = sc;
    return s;
}

struct BookSnapshot {
    std::vector<const void *> pointers;
    std::vector<uint32_t> emit_inst;
    std::vector<float> inst_weight;
    bool enabled;
    uint32_t count;
    bool operator==(const BookSnapshot &o) const {
        return pointers == o.pointers && emit_inst == o.emit_inst && inst_weight == o.inst_weight && enabled == o.enabled &&
               count == o.count;
    }
};
BookSnapshot snapshot(const Book &b) {
    return {{b.emit_inst.get(), b.inst_weight.get(), b.weight.get(), b.select.get(), b.sum.get()},
            b.h_emit_inst, b.h_inst_weight, b.enabled, b.count};
}

void check_book(const Book &b, const std::vector<uint32_t> &emit_inst, const std::vector<float> &inst_weight, uint32_t count) {
    REQUIRE(b.count == count && b.h_emit_inst == emit_inst && b.h_inst_weight == inst_weight);
    REQUIRE(live.at(b.emit_inst.get()) == sizeof(uint32_t) * count && live.at(b.weight.get()) == sizeof(float) * count);
    REQUIRE(live.at(b.select.get()) == sizeof(float) * count && live.at(b.sum.get()) == sizeof(float));
    REQUIRE(live.at(b.inst_weight.get()) == sizeof(float) * inst_weight.size());
    REQUIRE(std::memcmp(b.emit_inst.get(), emit_inst.data(), sizeof(uint32_t) * emit_inst.size()) == 0);
    REQUIRE(std::memcmp(b.inst_weight.get(), inst_weight.data(), sizeof(float) * inst_weight.size()) == 0);
}

}  // namespace

int main() {
    for (int i = 0; i < 48; i++) g_env_texels[i] = 0.25f + (float)((i * 7) % 11);
    Scene plain = make_scene(false, false), textured = make_scene(true, true), constant_env = make_scene(false, true);
    {  // stage then drop: everything is freed once
        Generation g;
        REQUIRE(Tables().stage(textured.get(), g) == PUPIL_OK);
        check_tables(textured.get(), g);
        REQUIRE(live.size() == 8 && g.texels.size() == 4);  // 2 lamp bitmaps, areas, cdf, guide, env texels, env block, env
    }
    REQUIRE(live.empty() && allocs == 8 && frees == 8);
    {
        Tables t;
        DeviceScene sc{};
        sc.num_materials = 77u;  // not the emitters': adopt leaves it
        {  // stage then adopt: the new generation is owned, the (empty) old one frees nothing
            Generation g;
            REQUIRE(t.stage(plain.get(), g) == PUPIL_OK);
            check_tables(plain.get(), g);
            REQUIRE(live.size() == 3 && g.texels.empty());
            t.adopt(std::move(g), sc);
            REQUIRE(g.areas.get() == nullptr && g.cdf.get() == nullptr);  // moved from: it owns nothing
        }
        check_published(t, sc);
        REQUIRE(live.size() == 3 && frees == 8 && sc.num_areas == 4 && sc.has_env == 0 && sc.num_materials == 77u);
        REQUIRE(t.env_map_held() == PUPIL_ERR_INVALID);
        // three replacing adoptions in a row: the texels and the env block go with their generation
        size_t count1 = 0, bytes1 = 0;
        for (int round = 0; round < 3; round++) {
            bool replaced = false;
            REQUIRE(update(t, sc, textured.get(), &replaced) == PUPIL_OK && replaced);  // a bitmap radiance: never in place
            check_published(t, sc);
            check_tables(textured.get(), t.cur());
            if (round == 0) count1 = live.size(), bytes1 = live_bytes();
            REQUIRE(live.size() == count1 && live_bytes() == bytes1 && count1 == 8);
        }
        // back to constant radiance with the same env: the shape stays, so in place, and again; the
        // generation keeps the texels it no longer points at until it goes
        bool replaced = true;
        REQUIRE(update(t, sc, constant_env.get(), &replaced) == PUPIL_OK && !replaced && live.size() == 8);
        check_tables(constant_env.get(), t.cur());
        const int allocs_before = allocs, syncs_before = syncs;
        Scene moved = make_scene(false, true, 0.5f);
        REQUIRE(update(t, sc, moved.get(), &replaced) == PUPIL_OK && !replaced && allocs == allocs_before && syncs == syncs_before + 1);
        check_published(t, sc);
        check_tables(moved.get(), t.cur());
        REQUIRE(t.cur().areas.get()[0].pos[1].x == 1.5f);

        // an allocation failing at each position of stage: nothing leaks, nothing changes
        const Snapshot before = snapshot(t.cur(), sc);
        int positions = 0;
        for (;; positions++) {
            Generation g;
            fail_at = allocs + positions;
            const int rc = t.stage(textured.get(), g);
            fail_at = -1;
            if (rc == PUPIL_OK) break;
            REQUIRE(rc == PUPIL_ERR_OOM && live.size() == 8u + (size_t)positions);
            g = Generation{};
            REQUIRE(live.size() == 8 && snapshot(t.cur(), sc) == before);
        }
        REQUIRE(positions == 8 && live.size() == 8 && snapshot(t.cur(), sc) == before);

        // the refusals, each twice in a row: refused both times, nothing changes
        Scene no_bitmap = make_scene(false, true);  // an env map whose radiance is no bitmap
        no_bitmap.env.radiance = constant(1.f, 1.f, 1.f);
        Scene disorder = make_scene(false, true), unknown = make_scene(false, true);
        std::swap(disorder.areas[2], disorder.areas[3]);  // a point light in front of a sphere
        unknown.areas[1].type = PUPIL_EMITTER_ENV_MAP;
        for (int twice = 0; twice < 2; twice++) {
            REQUIRE(update(t, sc, no_bitmap.get()) == PUPIL_ERR_INVALID && g_error == "env map needs a bitmap");
            REQUIRE(live.size() == 8 && snapshot(t.cur(), sc) == before);
            REQUIRE(update(t, sc, disorder.get()) == PUPIL_ERR_INVALID &&
                    g_error == "emitter table out of order: areas, point / spot, directional");
            REQUIRE(update(t, sc, unknown.get()) == PUPIL_ERR_INVALID && g_error == "emitter table entry of an unknown or env type");
            REQUIRE(live.size() == 8 && snapshot(t.cur(), sc) == before);
        }

        // the env writers go through the current generation; an update with the old desc then replaces
        float texels[48];
        for (int i = 0; i < 48; i++) texels[i] = (float)i;
        REQUIRE(t.reserve_env_texels(4, 4) == PUPIL_ERR_INVALID && live.size() == 8);
        REQUIRE(t.reserve_env_texels(4, 3) == PUPIL_OK && live.size() == 9);  // the row sums
        REQUIRE(t.write_env_texels(texels, 0) == PUPIL_OK && t.cur().env_stale);
        REQUIRE(std::memcmp(t.cur().h_env.radiance.data, texels, sizeof(texels)) == 0 && t.cur().env.get()->normalization == 7.f);
        REQUIRE(t.reserve_env_texels(4, 3) == PUPIL_OK && live.size() == 9);  // sized once
        const float rot[9] = {0.f, 1.f, 0.f, -1.f, 0.f, 0.f, 0.f, 0.f, 1.f};
        REQUIRE(t.write_env_params(2.f, rot, rot, 0) == PUPIL_OK);
        REQUIRE(t.cur().env.get()->scale == 2.f && std::memcmp(t.cur().env.get()->to_local, rot, sizeof(rot)) == 0);
        REQUIRE(update(t, sc, moved.get(), &replaced) == PUPIL_OK && replaced && !t.cur().env_stale && live.size() == 7);
        check_tables(moved.get(), t.cur());

        // ---- the device-side mode's bookkeeping: 6 instances, the lamp is 1, the sphere 4
        const std::vector<uint32_t> emit_inst = {1u, 1u, 4u};
        const std::vector<float> inst_weight = {0.f, 3.f, 0.f, 0.f, 2.f, 0.f};
        {  // stage then drop
            Book b;
            REQUIRE(Book::stage(emit_inst, inst_weight, 4, b) == PUPIL_OK);
            check_book(b, emit_inst, inst_weight, 4);
            REQUIRE(live.size() == 12);
        }
        REQUIRE(live.size() == 7 && t.book().emit_inst.get() == nullptr);
        {  // stage then adopt, twice: the second frees the first
            for (int twice = 0; twice < 2; twice++) {
                Book b;
                REQUIRE(Book::stage(emit_inst, inst_weight, 4, b) == PUPIL_OK);
                b.enabled = true;
                t.book() = std::move(b);
                REQUIRE(live.size() == 12);
            }
            check_book(t.book(), emit_inst, inst_weight, 4);
        }
        // an allocation failing at each position of the bookkeeping's staging, plain and re-indexed
        const std::vector<uint32_t> old_em = {1u, 4u}, new_em = {2u, 5u};
        const BookSnapshot book_before = snapshot(t.book());
        const Snapshot tables_before = snapshot(t.cur(), sc);
        for (int reindex = 0; reindex < 2; reindex++) {
            for (positions = 0;; positions++) {
                Book b;
                fail_at = allocs + positions;
                const int rc = reindex ? t.book().restage(old_em, new_em, 7, b, "emitter bookkeeping allocation failed") : Book::stage(emit_inst, inst_weight, 4, b);
                fail_at = -1;
                if (rc == PUPIL_OK) break;
                REQUIRE(rc == PUPIL_ERR_OOM && g_error == "emitter bookkeeping allocation failed");
                REQUIRE(live.size() == 12u + (size_t)positions);
                b = Book{};
                REQUIRE(live.size() == 12 && snapshot(t.book()) == book_before && snapshot(t.cur(), sc) == tables_before);
            }
            REQUIRE(positions == 5 && live.size() == 12 && snapshot(t.book()) == book_before);
        }
        {  // the re-index under a new instance table of 7: instance 1 is 2 there, 4 is 5
            Book b;
            REQUIRE(t.book().restage(old_em, new_em, 7, b, "emitter bookkeeping allocation failed") == PUPIL_OK && b.enabled);
            check_book(b, {2u, 2u, 5u}, {0.f, 0.f, 3.f, 0.f, 0.f, 2.f, 0.f}, 4);
            t.book() = std::move(b);
            REQUIRE(live.size() == 12);
        }
        t.book() = Book{};  // switched off: dropped
        REQUIRE(live.size() == 7 && !t.book().enabled && t.book().count == 0);
        REQUIRE(update(t, sc, plain.get(), &replaced) == PUPIL_OK && replaced && live.size() == 4 && sc.has_env == 0 && !sc.env);
    }
    REQUIRE(live.empty() && allocs == frees);  // the owner's destructor freed the last generation and the scratch
    std::printf("ok %d allocations\n", allocs);
    return 0;
}
