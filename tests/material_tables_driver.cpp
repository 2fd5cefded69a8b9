// material_tables_driver.cpp — csrc/host/material_tables.h on the host: the ownership paths of the
// engine's materials (create, stage, commit, the failures and refusals between) with a counting
// allocator in place of the device.
// Built with -fsanitize=address,undefined by test_material_tables_host.py: every array is sized
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

#include "host/material_tables.h"

using namespace pupil;

static std::string g_error;
int pupil::fail(int code, const std::string &msg) {
    g_error = msg;
    return code;
}

namespace {

std::map<void *, size_t> live;  // allocation -> bytes
int allocs = 0, frees = 0, fail_at = -1, writes = 0, write_fail_at = -1;

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
    static int write(void *dst, const void *src, size_t bytes, Stream) {
        if (writes == write_fail_at) return fail(PUPIL_ERR_HIP, "write failed");
        writes++;
        std::memcpy(dst, src, bytes);
        return PUPIL_OK;
    }
};
using Tables = MaterialTables<CountingDevice>;

// ---- materials: texels of w x h whose values name the bitmap, so a copy is told from another's
std::vector<float> texels(uint32_t w, uint32_t h, float tag) {
    std::vector<float> t(4 * (size_t)w * h);
    for (size_t i = 0; i < t.size(); i++) t[i] = tag + 0.001f * (float)i;
    return t;
}
pupil_texture constant(float r, float g, float b) {
    pupil_texture t{};
    t.type = PUPIL_TEX_RGB;
    t.c0[0] = r, t.c0[1] = g, t.c0[2] = b;
    return t;
}
pupil_texture bitmap(const std::vector<float> &rgba, uint32_t w, uint32_t h) {
    REQUIRE(rgba.size() == 4 * (size_t)w * h);
    pupil_texture t{};
    t.type = PUPIL_TEX_BITMAP;
    t.width = w, t.height = h;
    t.rgba = rgba.data();
    return t;
}
pupil_material diffuse(const pupil_texture &reflectance) {
    pupil_material m{};
    m.type = PUPIL_MAT_DIFFUSE;
    m.int_ior = 1.5f, m.ext_ior = 1.f;
    m.tex[0] = reflectance;
    return m;
}
pupil_material plastic(const pupil_texture &diffuse_reflectance, const pupil_texture &specular) {
    pupil_material m = diffuse(diffuse_reflectance);
    m.type = PUPIL_MAT_PLASTIC;
    m.tex[1] = specular;
    return m;
}

// the tables against the materials they should hold now: the mirror is convert_material's record with
// each bitmap slot pointing at texels the tables own, sized exactly and holding the source's; the device
// array equals the mirror; nothing else is live but `extra` allocations (staged or replaced texels)
void check(const Tables &t, const DeviceScene &sc, const std::vector<pupil_material> &want, size_t extra = 0) {
    REQUIRE(t.count() == want.size() && t.mirror().size() == want.size());
    REQUIRE(sc.materials == t.device() && sc.num_materials == t.count());
    REQUIRE(live.at(t.device()) == sizeof(DevMaterial) * want.size());
    size_t bitmaps = 0;
    for (size_t m = 0; m < want.size(); m++) {
        DevMaterial d;
        REQUIRE(convert_material(want[m], d) == PUPIL_OK);
        const DevMaterial &h = t.mirror()[m];
        for (int s = 0; s < 4; s++) {
            const pupil_texture &src = want[m].tex[s];
            if (src.type == PUPIL_TEX_BITMAP) {
                const size_t bytes = sizeof(float) * 4 * src.width * src.height;
                REQUIRE(live.at((void *)h.tex[s].data) == bytes && std::memcmp(h.tex[s].data, src.rgba, bytes) == 0);
                bitmaps++;
            } else {
                REQUIRE(h.tex[s].data == nullptr);
            }
            d.tex[s].data = h.tex[s].data;
        }
        REQUIRE(std::memcmp(&d, &h, sizeof(d)) == 0);
        REQUIRE(std::memcmp(t.device() + m, &h, sizeof(h)) == 0);
    }
    REQUIRE(live.size() == 1 + bitmaps + extra);
}

// every live allocation byte for byte, and the mirror
struct Snapshot {
    std::map<void *, std::string> memory;
    std::string mirror;
    bool operator==(const Snapshot &o) const { return memory == o.memory && mirror == o.mirror; }
};
Snapshot snapshot(const Tables &t) {
    Snapshot s;
    for (const auto &a : live) s.memory[a.first] = std::string((const char *)a.first, a.second);
    s.mirror.assign((const char *)t.mirror().data(), sizeof(DevMaterial) * t.mirror().size());
    return s;
}

// what pupil_pt_update_materials does with the owner: stage, commit, drop the replaced texels
int update(Tables &t, const std::vector<uint32_t> &ids, const std::vector<pupil_material> &mats, size_t *replaced_count = nullptr) {
    Tables::Staged st;
    if (const int rc = t.stage((uint32_t)ids.size(), ids.data(), mats.data(), st)) return rc;
    std::vector<Tables::Texels> replaced;
    bool type_changed = false;
    const int rc = t.commit(st, 0, replaced, type_changed);
    if (replaced_count) *replaced_count = replaced.size();
    return rc;
}

}  // namespace

int main() {
    const std::vector<float> a22 = texels(2, 2, 1.f), b32 = texels(3, 2, 2.f), c33 = texels(3, 3, 3.f), d33 = texels(3, 3, 4.f),
                             e51 = texels(5, 1, 5.f), f14 = texels(1, 4, 6.f), g22 = texels(2, 2, 7.f);
    std::vector<pupil_material> scene = {diffuse(bitmap(a22, 2, 2)), plastic(bitmap(b32, 3, 2), constant(0.9f, 0.9f, 0.9f)),
                                         diffuse(constant(0.2f, 0.3f, 0.4f))};
    {  // create then drop
        Tables t;
        DeviceScene sc{};
        REQUIRE(t.create(scene.data(), 3, sc) == PUPIL_OK);
        check(t, sc, scene);
        REQUIRE(live.size() == 3 && t.mirror()[1].specular_sampling_weight > 0.f);
    }
    REQUIRE(live.empty() && allocs == 3 && frees == 3);
    {  // a scene with no materials: one zeroed material, a valid pointer
        Tables t;
        DeviceScene sc{};
        REQUIRE(t.create(nullptr, 0, sc) == PUPIL_OK && t.count() == 1 && sc.num_materials == 1 && sc.materials == t.device());
        const DevMaterial zero{};
        REQUIRE(live.size() == 1 && live.at(t.device()) == sizeof(DevMaterial));
        REQUIRE(std::memcmp(t.device(), &zero, sizeof(zero)) == 0 && std::memcmp(t.mirror().data(), &zero, sizeof(zero)) == 0);
    }
    REQUIRE(live.empty());
    for (int position = 0; position < 3; position++) {  // create failing at each allocation: what it took goes with it
        Tables t;
        DeviceScene sc{};
        fail_at = allocs + position;
        REQUIRE(t.create(scene.data(), 3, sc) == PUPIL_ERR_OOM && live.size() == (size_t)position);
        fail_at = -1;
    }
    REQUIRE(live.empty());
    {
        Tables t;
        DeviceScene sc{};
        REQUIRE(t.create(scene.data(), 3, sc) == PUPIL_OK);
        std::vector<pupil_material> now = scene;
        {  // stage then drop: the fresh texels go with the stage, nothing changed
            const Snapshot before = snapshot(t);
            Tables::Staged st;
            const uint32_t id = 2;
            const pupil_material m = diffuse(bitmap(c33, 3, 3));
            REQUIRE(t.stage(1, &id, &m, st) == PUPIL_OK && st.size() == 1 && live.size() == 4);
            st = Tables::Staged{};
            REQUIRE(live.size() == 3 && snapshot(t) == before);
        }
        {  // stage, commit, then drop the replaced texels: a size change (2 x 2 -> 3 x 3)
            Tables::Staged st;
            const uint32_t id = 0;
            now[0] = diffuse(bitmap(c33, 3, 3));
            const void *old = t.mirror()[0].tex[0].data;
            REQUIRE(t.stage(1, &id, &now[0], st) == PUPIL_OK && live.size() == 4);
            std::vector<Tables::Texels> replaced;
            bool type_changed = false;
            REQUIRE(t.commit(st, 0, replaced, type_changed) == PUPIL_OK && !type_changed);
            REQUIRE(replaced.size() == 1 && replaced[0].get() == old && live.count((void *)old));  // still live: the stream may read it
            check(t, sc, now, 1);
            replaced.clear();
            check(t, sc, now);
        }
        {  // a bitmap of the same size reuses its texels: nothing allocated, nothing replaced
            const int allocs_before = allocs;
            const void *kept = t.mirror()[0].tex[0].data;
            size_t replaced = 7;
            now[0] = diffuse(bitmap(d33, 3, 3));
            REQUIRE(update(t, {0}, {now[0]}, &replaced) == PUPIL_OK && replaced == 0 && allocs == allocs_before);
            REQUIRE(t.mirror()[0].tex[0].data == kept);
            check(t, sc, now);
        }
        {  // bitmap to constant and back; the type change is reported
            size_t replaced = 0;
            now[0] = diffuse(constant(0.5f, 0.5f, 0.5f));
            REQUIRE(update(t, {0}, {now[0]}, &replaced) == PUPIL_OK && replaced == 1);
            check(t, sc, now);
            const int allocs_before = allocs;
            now[0] = plastic(bitmap(e51, 5, 1), constant(0.8f, 0.8f, 0.8f));
            Tables::Staged st;
            const uint32_t id = 0;
            REQUIRE(t.stage(1, &id, &now[0], st) == PUPIL_OK);
            std::vector<Tables::Texels> none;
            bool type_changed = false;
            REQUIRE(t.commit(st, 0, none, type_changed) == PUPIL_OK && type_changed && none.empty() && allocs == allocs_before + 1);
            check(t, sc, now);
        }
        {  // one id named twice, both bitmaps, of different sizes: the last one counts, exactly one survives
            const int allocs_before = allocs;
            size_t replaced = 7;
            now[2] = diffuse(bitmap(f14, 1, 4));
            REQUIRE(update(t, {2, 2}, {diffuse(bitmap(a22, 2, 2)), now[2]}, &replaced) == PUPIL_OK);
            REQUIRE(replaced == 0 && allocs == allocs_before + 1);
            check(t, sc, now);
            // and over a slot whose bitmap has the size of the entry that does not count: replaced, not reused
            now[2] = diffuse(bitmap(c33, 3, 3));
            REQUIRE(update(t, {2, 2}, {diffuse(bitmap(f14, 1, 4)), now[2]}, &replaced) == PUPIL_OK && replaced == 1);
            check(t, sc, now);
        }
        // a three-bitmap update with an allocation failing at each position: nothing leaks, nothing changes
        const std::vector<uint32_t> all = {0, 1, 2};
        const std::vector<pupil_material> three = {diffuse(bitmap(g22, 2, 2)), plastic(bitmap(c33, 3, 3), constant(0.9f, 0.9f, 0.9f)),
                                                   diffuse(bitmap(b32, 3, 2))};
        {
            const Snapshot before = snapshot(t);
            const size_t live_before = live.size();
            int positions = 0;
            for (;; positions++) {
                Tables::Staged st;
                fail_at = allocs + positions;
                const int rc = t.stage(3, all.data(), three.data(), st);
                fail_at = -1;
                if (rc == PUPIL_OK) break;
                REQUIRE(rc == PUPIL_ERR_OOM && g_error == "texel allocation failed" && live.size() == live_before + (size_t)positions);
                st = Tables::Staged{};
                REQUIRE(live.size() == live_before && snapshot(t) == before);
                check(t, sc, now);
            }
            REQUIRE(positions == 3 && live.size() == live_before && snapshot(t) == before);
        }
        {  // a write failing between two materials: the first is in place, the second untouched, nothing leaks
            const size_t live_before = live.size();
            Tables::Staged st;
            REQUIRE(t.stage(3, all.data(), three.data(), st) == PUPIL_OK && live.size() == live_before + 3);
            std::vector<Tables::Texels> replaced;
            bool type_changed = false;
            write_fail_at = writes + 2;  // material 0: its texels and its record; then material 1's texels
            REQUIRE(t.commit(st, 0, replaced, type_changed) == PUPIL_ERR_HIP && g_error == "write failed" && replaced.size() == 1);
            write_fail_at = -1;
            now[0] = three[0];
            check(t, sc, now, 3);  // the replaced texels of 0, the fresh ones of 1 and 2
            replaced.clear();
            st = Tables::Staged{};
            check(t, sc, now);
            REQUIRE(live.size() == live_before);
            REQUIRE(update(t, all, three) == PUPIL_OK);  // the same update again succeeds
            now = three;
            check(t, sc, now);
        }
        {  // a write failing within one material, after a slot reused in place was written: those texels hold
           // the new content, the mirror, the record and the owners are what they were, nothing leaks
            const size_t live_before = live.size();
            const std::string mirror_before = snapshot(t).mirror;
            const void *kept = t.mirror()[1].tex[0].data;
            const pupil_material two = plastic(bitmap(d33, 3, 3), bitmap(a22, 2, 2));
            Tables::Staged st;
            const uint32_t id = 1;
            REQUIRE(t.stage(1, &id, &two, st) == PUPIL_OK && live.size() == live_before + 1);
            std::vector<Tables::Texels> replaced;
            bool type_changed = false;
            write_fail_at = writes + 1;  // slot 0's texels are written, slot 1's are not
            REQUIRE(t.commit(st, 0, replaced, type_changed) == PUPIL_ERR_HIP && replaced.empty());
            write_fail_at = -1;
            st = Tables::Staged{};
            REQUIRE(live.size() == live_before && snapshot(t).mirror == mirror_before && t.mirror()[1].tex[0].data == kept);
            REQUIRE(std::memcmp(kept, d33.data(), sizeof(float) * d33.size()) == 0);
            REQUIRE(std::memcmp(t.device() + 1, &t.mirror()[1], sizeof(DevMaterial)) == 0);
            REQUIRE(update(t, {1}, {now[1]}) == PUPIL_OK);  // the old material again: its texels are rewritten
            check(t, sc, now);
        }
        {  // the refusals change nothing
            const Snapshot before = snapshot(t);
            pupil_material empty = diffuse(constant(0.f, 0.f, 0.f));
            empty.tex[0].type = PUPIL_TEX_BITMAP;
            empty.tex[0].width = empty.tex[0].height = 2;  // rgba stays null
            pupil_material unknown = diffuse(constant(0.f, 0.f, 0.f));
            unknown.tex[3].type = 3u;
            REQUIRE(update(t, {0, 3}, {now[0], now[1]}) == PUPIL_ERR_INVALID && g_error == "material index out of range");
            REQUIRE(update(t, {0, 1}, {diffuse(bitmap(a22, 2, 2)), empty}) == PUPIL_ERR_INVALID && g_error == "bitmap texture without texels");
            REQUIRE(update(t, {1}, {unknown}) == PUPIL_ERR_INVALID && g_error == "unknown texture type");
            REQUIRE(snapshot(t) == before);
            check(t, sc, now);
        }
    }
    REQUIRE(live.empty() && allocs == frees);  // the owner's destructor freed the array and every slot's texels
    std::printf("ok %d allocations\n", allocs);
    return 0;
}
