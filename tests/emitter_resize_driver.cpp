// emitter_resize_driver.cpp — the staged resize of csrc/host/emitter_tables.h on the host:
// EmitterTables::stage_resize / adopt_resize with a counting allocator in place of the device.  The
// records themselves are the device's work (pt_emitters.hip); here: what is sized, owned, moved
// and freed.  Texel buffers of kept emitters move and are not duplicated, those of emitters that
// went are freed exactly once, new bitmaps are uploaded once per instance, the env record and its
// texels carry over, an allocation failing at each staging step leaves cur() and book() untouched,
// and the table grows, shrinks, goes to zero and comes back.
// Built with -fsanitize=address,undefined by test_emitter_resize_host.py: every array is sized
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
int allocs = 0, frees = 0, fail_at = -1;

#define REQUIRE(c)                                                      \
    do {                                                                \
        if (!(c)) {                                                     \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);  \
            std::exit(1);                                               \
        }                                                               \
    } while (0)

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
    static int download(void *dst, const void *src, size_t bytes) { return upload(dst, src, bytes); }
    static int copy(void *dst, const void *src, size_t bytes) { return upload(dst, src, bytes); }
    static int write(void *dst, const void *src, size_t bytes, Stream) { return upload(dst, src, bytes); }
    static int sync(Stream) { return PUPIL_OK; }
    static int env_tables(const DevEmitter &, const void *, float *, DevEmitter *, Stream) { return PUPIL_OK; }
};
using Tables = EmitterTables<CountingDevice>;
using Generation = Tables::Generation;
using Resize = Tables::Resize;

const float kLampA[16] = {4.f, 3.f, 2.f, 1.f, 0.5f, 6.f, 1.f, 1.f, 2.f, 2.f, 2.f, 1.f, 0.25f, 1.f, 8.f, 1.f};  // 2 x 2
const float kLampB[16] = {1.f, 1.f, 1.f, 1.f, 2.f, 2.f, 2.f, 1.f, 3.f, 3.f, 3.f, 1.f, 4.f, 4.f, 4.f, 1.f};
float g_env_texels[4 * 3 * 4];

pupil_texture constant(float r, float g, float b) {
    pupil_texture t{};
    t.type = PUPIL_TEX_RGB;
    t.c0[0] = r, t.c0[1] = g, t.c0[2] = b;
    return t;
}
pupil_texture bitmap(const float *rgba) {
    pupil_texture t{};
    t.type = PUPIL_TEX_BITMAP;
    t.width = t.height = 2;
    t.rgba = rgba;
    return t;
}

// the first scene, from the host: a two-triangle lamp with a bitmap (instance 1), a sphere with a
// constant radiance (instance 3), a point light; an env map or none
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
Scene make_scene(bool env_map) {
    Scene s;
    const uint32_t types[4] = {PUPIL_EMITTER_TRI_AREA, PUPIL_EMITTER_TRI_AREA, PUPIL_EMITTER_SPHERE, PUPIL_EMITTER_POINT};
    for (int k = 0; k < 4; k++) {
        pupil_emitter e{};
        e.type = types[k];
        e.weight = 1.f;
        e.select_probability = 0.25f;
        e.area = 1.f + k;
        e.radiance = k < 2 ? bitmap(kLampA) : constant(4.f, 3.f, 2.f);
        e.center[0] = (float)k;
        s.areas.push_back(e);
    }
    if (env_map) {
        s.env.type = PUPIL_EMITTER_ENV_MAP;
        s.env.weight = 1.f;
        s.env.scale = 1.f;
        s.env.select_probability = 0.2f;
        pupil_texture t{};
        t.type = PUPIL_TEX_BITMAP;
        t.width = 4, t.height = 3;
        t.rgba = g_env_texels;
        s.env.radiance = t;
        s.env.to_world[0] = s.env.to_world[4] = s.env.to_world[8] = 1.f;
        s.env.to_local[0] = s.env.to_local[4] = s.env.to_local[8] = 1.f;
    }
    return s;
}

EmitterSource source(uint32_t inst, uint32_t offset, uint32_t range, float weight, int64_t kept, pupil_texture radiance = {},
                     uint32_t type = PUPIL_EMITTER_TRI_AREA) {
    EmitterSource s;
    s.inst = inst, s.offset = offset, s.range = range, s.weight = weight, s.kept = kept, s.radiance = radiance, s.type = type;
    return s;
}

// every live allocation byte for byte, the pointers the owner holds and what it published
struct Snapshot {
    std::map<void *, std::string> memory;
    std::vector<const void *> pointers;
    std::vector<uint32_t> types, emit_inst;
    std::vector<float> inst_weight;
    uint32_t guide_bits, num_true_areas, count;
    bool enabled;
    std::string sc;
    bool operator==(const Snapshot &o) const {
        return memory == o.memory && pointers == o.pointers && types == o.types && emit_inst == o.emit_inst &&
               inst_weight == o.inst_weight && guide_bits == o.guide_bits && num_true_areas == o.num_true_areas &&
               count == o.count && enabled == o.enabled && sc == o.sc;
    }
};
Snapshot snapshot(Tables &t, const DeviceScene &sc) {
    Snapshot s;
    for (const auto &a : live) s.memory[a.first] = std::string((const char *)a.first, a.second);
    const Generation &g = t.cur();
    s.pointers = {g.areas.get(), g.env.get(), g.cdf.get(), g.guide.get(), t.book().emit_inst.get(), t.book().inst_weight.get(),
                  t.book().weight.get(), t.book().select.get(), t.book().sum.get()};
    for (const auto &x : g.texels) s.pointers.push_back(x.get());
    s.types = g.types, s.guide_bits = g.guide_bits, s.num_true_areas = g.num_true_areas;
    s.emit_inst = t.book().h_emit_inst, s.inst_weight = t.book().h_inst_weight;
    s.count = t.book().count, s.enabled = t.book().enabled;
    s.sc.assign((const char *)&sc, sizeof(sc));
    return s;
}

// the published tables are the current generation's, sized for `types`; the bookkeeping matches
void check_current(Tables &t, const DeviceScene &sc, const std::vector<uint32_t> &types, uint32_t true_areas, uint32_t instances,
                   bool env) {
    const Generation &g = t.cur();
    const uint32_t total = (uint32_t)types.size();
    REQUIRE(g.types == types && g.num_true_areas == true_areas);
    REQUIRE(sc.areas == g.areas.get() && sc.area_cdf == g.cdf.get() && sc.area_guide == g.guide.get());
    REQUIRE(sc.num_areas == total && sc.guide_bits == g.guide_bits && sc.env == g.env.get() && sc.has_env == (env ? 1u : 0u));
    REQUIRE(live.at(g.areas.get()) == sizeof(DevEmitter) * (total ? total : 1u));
    REQUIRE(live.at(g.cdf.get()) == sizeof(float) * (total ? total : 1u));
    uint32_t bits = 0;
    while ((1u << bits) < total) bits++;
    REQUIRE(g.guide_bits == bits);
    if (total >= 2) REQUIRE(g.guide.get() && live.at(g.guide.get()) == sizeof(uint32_t) * ((1u << bits) + 1u));
    else REQUIRE(!g.guide.get());  // none below two emitters, as emitter_tables() decides
    const auto &b = t.book();
    REQUIRE(b.enabled && b.count == total && b.h_emit_inst.size() == true_areas && b.h_inst_weight.size() == instances);
    REQUIRE(live.at(b.emit_inst.get()) == sizeof(uint32_t) * (total ? total : 1u));
    REQUIRE(live.at(b.weight.get()) == sizeof(float) * (total ? total : 1u) && live.at(b.select.get()) == live.at(b.weight.get()));
    REQUIRE(live.at(b.inst_weight.get()) == sizeof(float) * instances && live.at(b.sum.get()) == sizeof(float));
    REQUIRE(std::memcmp(b.inst_weight.get(), b.h_inst_weight.data(), sizeof(float) * instances) == 0);
    if (env) {
        REQUIRE(g.env.get() && g.env_src_valid);
        const float p = 1.f / (float)(total + 1);
        REQUIRE(g.env.get()->select_probability == p && g.h_env.select_probability == p && g.env_src.select_probability == p);
        REQUIRE(live.count((void *)g.h_env.radiance.data) == 1 && live.count((void *)g.h_env.col_cdf) == 1);
        REQUIRE(g.env.get()->radiance.data == g.h_env.radiance.data && g.env.get()->col_cdf == g.h_env.col_cdf);
    } else {
        REQUIRE(!g.env.get());
    }
}

// a resize that must succeed, with an allocation failing at each of its staging steps first:
// every failure frees what the staging took and leaves the owner as it was
void resize(Tables &t, DeviceScene &sc, const std::vector<EmitterSource> &sources, uint32_t instances,
            const pupil_emitter *deltas, uint32_t num_deltas, bool keep_deltas, int *steps = nullptr) {
    const Snapshot before = snapshot(t, sc);
    const size_t live_before = live.size();
    int positions = 0;
    for (;; positions++) {
        Resize r;
        fail_at = allocs + positions;
        const int rc = t.stage_resize(sources, instances, deltas, num_deltas, keep_deltas, r);
        fail_at = -1;
        if (rc == PUPIL_OK) {
            REQUIRE(snapshot(t, sc).pointers == before.pointers);  // staged: nothing has moved yet
            t.adopt_resize(std::move(r), sc);
            break;
        }
        REQUIRE(rc == PUPIL_ERR_OOM);
        r = Resize{};
        REQUIRE(live.size() == live_before && snapshot(t, sc) == before);
    }
    REQUIRE(positions >= 6);  // areas, cdf, sources and the bookkeeping's five at the least
    if (steps) *steps = positions;
}

const void *texels_of(Tables &t, uint32_t record) { return t.cur().areas.get()[record].radiance.data; }

// the fill kernel's work, stood in for: records [first, last) name the texels their source carried
void stand_in(Tables &t, uint32_t first, uint32_t last, const void *texels) {
    for (uint32_t e = first; e < last; e++) {
        DevEmitter &d = t.cur().areas.get()[e];
        std::memset(&d, 0, sizeof(d));
        d.type = PUPIL_EMITTER_TRI_AREA;
        d.radiance.type = PUPIL_TEX_BITMAP;
        d.radiance.width = d.radiance.height = 2;
        d.radiance.data = (const float4 *)texels;
    }
}

}  // namespace

int main() {
    for (int i = 0; i < 48; i++) g_env_texels[i] = 0.25f + (float)((i * 7) % 11);
    const uint32_t TRI = PUPIL_EMITTER_TRI_AREA, SPH = PUPIL_EMITTER_SPHERE, PNT = PUPIL_EMITTER_POINT, DIR = PUPIL_EMITTER_DIRECTIONAL;
    for (int with_env = 0; with_env < 2; with_env++) {
        Tables t;
        DeviceScene sc{};
        Scene first = make_scene(with_env != 0);
        REQUIRE(t.update(first.get(), 0, sc) == PUPIL_OK);
        // the host path uploads one texel copy per record: the lamp's two triangles hold two
        const void *lamp0 = texels_of(t, 0), *lamp1 = texels_of(t, 1);
        REQUIRE(lamp0 && lamp1 && lamp0 != lamp1 && live.at((void *)lamp0) == sizeof(kLampA));
        const size_t env_allocs = with_env ? 3 : 0;  // the record, its texels, its tables
        REQUIRE(live.size() == 2 + 3 + env_allocs);

        // grow: the lamp re-meshed to five faces keeps its radiance, the sphere stays, the point light is kept.
        // The lamp's first texel buffer moves; the per-record duplicate goes with the old generation.
        {
            auto &sphere_rec = t.cur().areas.get()[2];
            REQUIRE(sphere_rec.radiance.data == nullptr);
            std::vector<EmitterSource> src = {source(1, 0, 5, 3.f, 0), source(3, 5, 1, 2.f, 2, {}, SPH)};
            resize(t, sc, src, 6, nullptr, 0, true);
            check_current(t, sc, {TRI, TRI, TRI, TRI, TRI, SPH, PNT}, 6, 6, with_env != 0);
            REQUIRE(live.count((void *)lamp0) == 1 && live.count((void *)lamp1) == 0);  // moved; freed once
            REQUIRE(t.cur().texels.size() == 1 + (with_env ? 2u : 0u));
            // the kept point light under its new index, whole
            REQUIRE(t.cur().areas.get()[6].type == PNT && t.cur().areas.get()[6].center.x == 3.f);
            REQUIRE(t.book().h_emit_inst == std::vector<uint32_t>({1u, 1u, 1u, 1u, 1u, 3u}));
            REQUIRE(t.book().h_inst_weight == std::vector<float>({0.f, 3.f, 0.f, 2.f, 0.f, 0.f}));
            REQUIRE(live.size() == 3 + 5 + 1 + env_allocs);  // areas, cdf, guide; the bookkeeping; the lamp's texels
        }
        stand_in(t, 0, 5, lamp0);

        // a second bitmap lamp comes (uploaded once, whatever its range), the first stays: its buffer
        // moves again and is not duplicated; delta lights from a scene: a point and a directional
        pupil_emitter deltas[2]{};
        deltas[0].type = PNT, deltas[0].center[0] = 7.f;
        deltas[1].type = DIR, deltas[1].nrm[0][1] = -1.f;
        const void *second = nullptr;
        {
            const int allocs_before = allocs;
            std::vector<EmitterSource> src = {source(0, 0, 3, 1.5f, -1, bitmap(kLampB)), source(2, 3, 5, 3.f, 0)};
            int steps = 0;
            resize(t, sc, src, 4, deltas, 2, false, &steps);
            check_current(t, sc, {TRI, TRI, TRI, TRI, TRI, TRI, TRI, TRI, PNT, DIR}, 8, 4, with_env != 0);
            REQUIRE(live.count((void *)lamp0) == 1);
            REQUIRE(t.cur().texels.size() == 2 + (with_env ? 2u : 0u));
            second = t.cur().texels[0].get();
            REQUIRE(second != lamp0 && live.at((void *)second) == sizeof(kLampB) && std::memcmp(second, kLampB, sizeof(kLampB)) == 0);
            REQUIRE(t.cur().areas.get()[8].center.x == 7.f && t.cur().areas.get()[9].nrm[0].y == -1.f);
            // one staging allocates: one bitmap, areas, cdf, guide, sources, the env record, the bookkeeping's five
            REQUIRE(steps == 1 + 3 + 1 + (with_env ? 1 : 0) + 5);
            REQUIRE(allocs - allocs_before == steps * (steps + 1) / 2);  // the failing rounds and the one that passed
            REQUIRE(live.size() == 3 + 5 + 2 + env_allocs);
        }
        stand_in(t, 0, 3, second);
        stand_in(t, 3, 8, lamp0);

        // shrink: the first lamp goes -- its texels are freed exactly once -- the second stays; no delta light
        {
            const int frees_before = frees;
            std::vector<EmitterSource> src = {source(0, 0, 1, 1.5f, 0)};
            resize(t, sc, src, 2, nullptr, 0, false);
            check_current(t, sc, {TRI}, 1, 2, with_env != 0);  // one emitter: no guide
            REQUIRE(live.count((void *)lamp0) == 0 && live.count((void *)second) == 1);
            REQUIRE(frees - frees_before >= 1 && live.size() == 2 + 5 + 1 + env_allocs);
        }
        stand_in(t, 0, 1, second);

        // to zero: an empty table; the last bitmap is freed
        {
            resize(t, sc, {}, 2, nullptr, 0, false);
            check_current(t, sc, {}, 0, 2, with_env != 0);
            REQUIRE(live.count((void *)second) == 0 && t.cur().texels.size() == (with_env ? 2u : 0u));
            REQUIRE(live.size() == 2 + 5 + env_allocs);
        }
        // zero true areas, delta lights alone
        {
            resize(t, sc, {}, 2, deltas, 2, false);
            check_current(t, sc, {PNT, DIR}, 0, 2, with_env != 0);
        }
        // from zero: a sphere and a lamp come back, the delta lights are kept under new indices
        {
            std::vector<EmitterSource> src = {source(0, 0, 1, 2.f, -1, constant(1.f, 2.f, 3.f), SPH),
                                              source(1, 1, 2, 1.f, -1, bitmap(kLampA))};
            resize(t, sc, src, 2, nullptr, 0, true);
            check_current(t, sc, {SPH, TRI, TRI, PNT, DIR}, 3, 2, with_env != 0);
            REQUIRE(t.cur().areas.get()[3].center.x == 7.f && t.cur().areas.get()[4].nrm[0].y == -1.f);
            REQUIRE(t.cur().texels.size() == 1 + (with_env ? 2u : 0u));
        }
        // refusals change nothing: ranges out of order, a kept record that is none, a bitmap without texels
        {
            const Snapshot before = snapshot(t, sc);
            Resize r;
            REQUIRE(t.stage_resize({source(0, 1, 2, 1.f, -1, constant(1.f, 1.f, 1.f))}, 2, nullptr, 0, true, r) == PUPIL_ERR_INVALID);
            REQUIRE(t.stage_resize({source(0, 0, 2, 1.f, 3)}, 2, nullptr, 0, true, r) == PUPIL_ERR_INVALID);
            pupil_texture broken = bitmap(nullptr);
            REQUIRE(t.stage_resize({source(0, 0, 2, 1.f, -1, broken)}, 2, nullptr, 0, true, r) == PUPIL_ERR_INVALID);
            r = Resize{};
            REQUIRE(snapshot(t, sc) == before);
        }
        // the host path takes over again: pupil_pt_update_emitters replaces the resized generation whole
        REQUIRE(t.update(first.get(), 0, sc) == PUPIL_OK && sc.num_areas == 4);
    }
    REQUIRE(live.empty() && allocs == frees);
    std::printf("ok %d allocations\n", allocs);
    return 0;
}
