// prim_tables_driver.cpp — csrc/host/prim_tables.h on the host: the prefix sums, the guide's
// geometry and the lookup the fill kernel runs per primitive (pt_replace.hip), against the
// tables' specification, restated below from an explicit prim_inst array.  Built with
// -fsanitize=address,undefined by test_prim_tables_host.py: every table is sized exactly, so
// an index past an end fails the run.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "host/prim_tables.h"

using namespace pupil;

namespace {

int g_cases = 0;

#define REQUIRE(c)                                                      \
    do {                                                                \
        if (!(c)) {                                                     \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);  \
            std::exit(1);                                               \
        }                                                               \
    } while (0)

// the specification: what every engine's tables must be, at create and after an update
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

void check(const std::vector<uint32_t> &counts) {
    std::vector<uint32_t> prim_inst, inst_first, inst_guide;
    uint32_t shift = 0;
    reference(counts, prim_inst, inst_first, inst_guide, shift);
    PrimTables t;
    REQUIRE(prim_tables(counts.data(), counts.size(), &t));
    REQUIRE(t.inst_first == inst_first);
    REQUIRE(t.num_prims == prim_inst.size());
    REQUIRE(t.guide_shift == shift);
    REQUIRE(t.guide_entries == inst_guide.size());
    // the fill, as the kernel's threads do it, into exactly sized arrays
    std::vector<uint32_t> filled(t.num_prims), guide(t.guide_entries);
    const uint32_t ni = (uint32_t)counts.size();
    for (uint32_t p = 0; p < t.num_prims; p++) filled[p] = prim_holder(t.inst_first.data(), ni, p);
    for (uint32_t k = 0; k < t.guide_entries; k++)
        guide[k] = prim_guide_entry(t.inst_first.data(), ni, t.num_prims, t.guide_shift, k);
    REQUIRE(filled == prim_inst);
    REQUIRE(guide == inst_guide);
    g_cases++;
}

}  // namespace

int main() {
    check({1});
    check({12, 12, 1, 80, 2});                  // the test scene's shape
    check({2, 12, 12, 1, 80, 2});
    check({2, 18432, 18432, 1, 80, 2});         // past 8192 primitives: shift 2
    check({8192});                              // the last count at shift 0
    check({8193});                              // the first at shift 1
    check({8191, 1, 1});
    check({1, 16384, 1});                       // 16386 primitives: shift 2, by one
    check({16383, 1});                          // 16384: shift 1, exactly
    check({5, 0, 0, 7, 0, 3});                  // empty instances share their first id with the next holder
    check({0, 0, 4});
    check({100000, 1, 120000, 3, 1});
    std::vector<uint32_t> many(5000);
    uint32_t x = 12345u;
    for (uint32_t &c : many) {
        x = x * 1664525u + 1013904223u;
        c = 1u + (x >> 24);                      // 1 .. 256
    }
    check(many);
    {  // 2^31 primitives or more are refused, without a wrap of the 32-bit sums
        const std::vector<uint32_t> big = {0x7FFFFFFFu, 1u};
        PrimTables t;
        REQUIRE(!prim_tables(big.data(), big.size(), &t));
        const std::vector<uint32_t> wrap = {0xFFFFFFFFu, 0xFFFFFFFFu, 2u};
        REQUIRE(!prim_tables(wrap.data(), wrap.size(), &t));
        const std::vector<uint32_t> most = {0x7FFFFFFEu, 1u};
        REQUIRE(prim_tables(most.data(), most.size(), &t));
        REQUIRE(t.num_prims == 0x7FFFFFFFu && t.guide_shift == 18 && t.guide_entries == 8193u);
        REQUIRE(prim_holder(t.inst_first.data(), 2, 0x7FFFFFFEu) == 1u && prim_holder(t.inst_first.data(), 2, 0x7FFFFFFDu) == 0u);
        REQUIRE(prim_guide_entry(t.inst_first.data(), 2, t.num_prims, t.guide_shift, 8192u) == 1u);
    }
    REQUIRE(prim_guide_shift(0) == 0 && prim_guide_shift(8192) == 0 && prim_guide_shift(8193) == 1);
    std::printf("ok %d cases\n", g_cases);
    return 0;
}
