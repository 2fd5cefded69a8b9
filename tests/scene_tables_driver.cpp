// scene_tables_driver.cpp — csrc/host/scene_tables.h on the host: the ownership paths of the
// engine's instance and primitive tables (stage, adopt, the failures between) with a counting
// allocator in place of the device, and the staged tables against the definition restated below.
// Built with -fsanitize=address,undefined by test_scene_tables_host.py: every array is sized
// exactly, so a leak, a double free, a use after free or an index past an end fails the run.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <string>
#include <vector>

// the engine's headers name HIP's vector types in structs this driver never touches
struct float2 { float x, y; };
struct float4 { float x, y, z, w; };

#include "host/scene_tables.h"

using namespace pupil;

static std::string g_error;
int pupil::fail(int code, const std::string &msg) {
    g_error = msg;
    return code;
}

namespace {

std::set<void *> live;
int allocs = 0, frees = 0, fail_at = -1, fills = 0;

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
        live.insert(*p);
        allocs++;
        return 0;
    }
    static void free(void *p) {
        REQUIRE(live.erase(p) == 1);  // a pointer that is not live: a double free
        std::free(p);
        frees++;
    }
    // what the engine's device does: inst_first goes up, the fill kernel's threads write the rest
    static int fill(const TableGeneration<CountingDevice> &g, Stream) {
        REQUIRE(g.first.size() == (size_t)g.num_instances + 1);
        std::memcpy(g.inst_first.get(), g.first.data(), sizeof(uint32_t) * g.first.size());
        for (uint32_t p = 0; p < g.num_prims; p++) g.prim_inst.get()[p] = prim_holder(g.inst_first.get(), g.num_instances, p);
        for (uint32_t k = 0; k < g.guide_entries; k++)
            g.inst_guide.get()[k] = prim_guide_entry(g.inst_first.get(), g.num_instances, g.num_prims, g.guide_shift, k);
        fills++;
        return PUPIL_OK;
    }
};
using Tables = SceneTables<CountingDevice>;
using Generation = Tables::Generation;

// the specification of the three tables, from an explicit prim_inst array
void reference(const std::vector<uint32_t> &counts, std::vector<uint32_t> &prim_inst, std::vector<uint32_t> &inst_first,
               std::vector<uint32_t> &inst_guide, uint32_t &shift) {
    prim_inst.clear();
    inst_first.resize(counts.size() + 1);
    for (size_t i = 0; i < counts.size(); i++) {
        inst_first[i] = (uint32_t)prim_inst.size();
        prim_inst.insert(prim_inst.end(), counts[i], (uint32_t)i);
    }
    inst_first[counts.size()] = (uint32_t)prim_inst.size();
    shift = 0;
    while ((prim_inst.size() >> shift) > 8192u) shift++;
    if (!prim_inst.empty()) {
        const size_t nb = ((prim_inst.size() - 1) >> shift) + 1;
        inst_guide.resize(nb + 1);
        for (size_t k = 0; k <= nb; k++) inst_guide[k] = prim_inst[std::min(k << shift, prim_inst.size() - 1)];
    } else {
        inst_guide.assign(2, 0u);
    }
}

int stage(const std::vector<uint32_t> &counts, Generation &out, bool flat = true) {
    return Tables::stage(counts.data(), (uint32_t)counts.size(), flat, 0, out);
}

// a staged generation holds exactly the reference's tables, a zeroed mirror and four live arrays
void check_staged(const std::vector<uint32_t> &counts, const Generation &g) {
    std::vector<uint32_t> prim_inst, inst_first, inst_guide;
    uint32_t shift = 0;
    reference(counts, prim_inst, inst_first, inst_guide, shift);
    REQUIRE(g.num_instances == counts.size() && g.num_prims == prim_inst.size());
    REQUIRE(g.guide_shift == shift && g.guide_entries == inst_guide.size());
    REQUIRE(g.first == inst_first);
    REQUIRE(std::equal(inst_first.begin(), inst_first.end(), g.inst_first.get()));
    REQUIRE(std::equal(prim_inst.begin(), prim_inst.end(), g.prim_inst.get()));
    REQUIRE(std::equal(inst_guide.begin(), inst_guide.end(), g.inst_guide.get()));
    REQUIRE(g.mirror.size() == counts.size());
    const DevInstance zero{};
    for (const DevInstance &d : g.mirror) REQUIRE(std::memcmp(&d, &zero, sizeof(d)) == 0);
    for (void *p : {(void *)g.insts.get(), (void *)g.prim_inst.get(), (void *)g.inst_first.get(), (void *)g.inst_guide.get()})
        REQUIRE(live.count(p) == 1);
    std::memset(g.insts.get(), 0xAB, sizeof(DevInstance) * g.num_instances);  // the caller's to fill: sized for it
}

// what adopt published is the generation `t` holds now
void check_published(const Tables &t, const DeviceScene &sc, const pupil_pt_counters &totals) {
    const Generation &g = t.cur();
    REQUIRE(sc.instances == g.insts.get() && sc.num_instances == g.num_instances);
    REQUIRE(sc.prim_inst == g.prim_inst.get() && sc.inst_first == g.inst_first.get() && sc.inst_guide == g.inst_guide.get());
    REQUIRE(sc.inst_guide_shift == g.guide_shift && sc.num_prims == g.num_prims && totals.bvh_prims == g.num_prims);
}

}  // namespace

int main() {
    const std::vector<uint32_t> scene = {12, 12, 1, 80, 2}, gaps = {5, 0, 0, 7, 0, 3};
    {  // stage then drop: everything is freed once
        Generation g;
        REQUIRE(stage(scene, g) == PUPIL_OK);
        check_staged(scene, g);
        REQUIRE(live.size() == 4 && allocs == 4 && fills == 1);
    }
    REQUIRE(live.empty() && frees == 4);
    {
        Tables t;
        DeviceScene sc{};
        pupil_pt_counters totals{};
        sc.num_materials = 77u;  // not the tables': adopt leaves it
        {  // stage then adopt: the new generation is owned, the (empty) old one frees nothing
            Generation g;
            REQUIRE(stage(scene, g) == PUPIL_OK);
            const DevInstance *insts = g.insts.get();
            const uint32_t *prim_inst = g.prim_inst.get(), *inst_first = g.inst_first.get(), *inst_guide = g.inst_guide.get();
            g.mirror[3].material = 9u;
            t.adopt(std::move(g), sc, totals);
            REQUIRE(sc.instances == insts && sc.prim_inst == prim_inst && sc.inst_first == inst_first && sc.inst_guide == inst_guide);
            REQUIRE(sc.num_instances == 5 && sc.num_prims == 107 && sc.inst_guide_shift == 0 && totals.bvh_prims == 107);
            REQUIRE(g.insts.get() == nullptr && g.prim_inst.get() == nullptr);  // moved from: it owns nothing
        }
        check_published(t, sc, totals);
        REQUIRE(live.size() == 4 && frees == 4 && t.cur().mirror[3].material == 9u && sc.num_materials == 77u);
        {  // adopt twice in a row: each frees the generation before it, once
            Generation g, h;
            REQUIRE(stage(gaps, g) == PUPIL_OK && stage({2, 18432, 18432, 1, 80, 2}, h) == PUPIL_OK);
            check_staged(gaps, g);
            REQUIRE(live.size() == 12);
            t.adopt(std::move(g), sc, totals);
            REQUIRE(live.size() == 8 && frees == 8);
            check_published(t, sc, totals);
            REQUIRE(sc.num_instances == 6 && sc.num_prims == 15);
            t.adopt(std::move(h), sc, totals);
            REQUIRE(live.size() == 4 && frees == 12);
            check_published(t, sc, totals);
            REQUIRE(sc.num_prims == 36949 && sc.inst_guide_shift == 3);
        }
        REQUIRE(live.size() == 4);
        // an allocation that fails at each of the four positions: nothing leaks, the current
        // generation and what was published stay
        const DeviceScene before = sc;
        const std::set<void *> held = live;
        for (int pos = 0; pos < 4; pos++) {
            const int fills_before = fills;
            {
                Generation g;
                fail_at = allocs + pos;
                REQUIRE(stage(scene, g) == PUPIL_ERR_OOM && g_error == "scene tables: allocation failed");
                fail_at = -1;
                REQUIRE(live.size() == 4u + (size_t)pos && fills == fills_before);  // nothing was enqueued
            }
            REQUIRE(live == held && std::memcmp(&before, &sc, sizeof(sc)) == 0);
            check_published(t, sc, totals);
            REQUIRE(t.cur().num_prims == 36949 && t.cur().mirror.size() == 6);
        }
        {  // the refusals: nothing is allocated
            const int allocs_before = allocs;
            Generation g;
            REQUIRE(stage({0x7FFFFFFFu, 1u}, g) == PUPIL_ERR_UNSUPPORTED && g_error == "more than 2^31 primitives");
            REQUIRE(stage({0xFFFFFFFFu, 0xFFFFFFFFu, 2u}, g) == PUPIL_ERR_UNSUPPORTED && g_error == "more than 2^31 primitives");
            REQUIRE(stage({1u << 26, 1u << 26}, g) == PUPIL_ERR_UNSUPPORTED && g_error == "flattened BVH limited to 2^27 primitives");
            REQUIRE(allocs == allocs_before && g.insts.get() == nullptr && live == held);
            REQUIRE(stage({(1u << 13) + 1u}, g, false) == PUPIL_OK);  // below every limit, either mode
            check_staged({(1u << 13) + 1u}, g);
        }
        REQUIRE(live == held);
    }
    REQUIRE(live.empty() && allocs == frees);  // the owner's destructor freed the last generation
    std::printf("ok %d allocations\n", allocs);
    return 0;
}
