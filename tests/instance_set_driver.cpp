// instance_set_driver.cpp — csrc/host/instance_record.h on the host: the record assembly that
// pupil_pt_create, pupil_pt_set_instances' host mirror and the fill kernel (pt_instance_set.hip)
// share, against the record's specification (restated below, field by field) with the prim
// offsets of host/prim_tables.h; the two-level fields stay zero for the structure's instance stage.
// Built with -fsanitize=address,undefined by test_instance_set_host.py: every table is sized
// exactly, so an index past an end fails the run.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

// the engine's headers name HIP's vector types in structs this driver never touches
struct float2 { float x, y; };
struct float4 { float x, y, z, w; };

#include "host/instance_record.h"
#include "host/prim_tables.h"

using namespace pupil;

namespace {

#define REQUIRE(c)                                                      \
    do {                                                                \
        if (!(c)) {                                                     \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);  \
            std::exit(1);                                               \
        }                                                               \
    } while (0)

struct Source {  // what a pupil_instance and its mask carry
    uint32_t shape, material, flip_n, flip_t;
    int32_t emitter_offset;
    uint32_t mask;
    float to_world[12];
};

// the specification: the record of instance `src`, all zero outside the fields named here
DevInstance reference(const Source &src, const InstShape &sh, uint32_t bin, uint32_t prim_offset, const float *to_object) {
    DevInstance d;
    std::memset(&d, 0, sizeof(d));
    std::memcpy(d.to_world, src.to_world, sizeof(d.to_world));
    std::memcpy(d.to_object, to_object, sizeof(d.to_object));
    d.kind = sh.kind;
    d.material = src.material;
    d.prim_offset = prim_offset;
    d.emitter_offset = src.emitter_offset;
    d.flip_normals = src.flip_n;
    d.flip_tex_coords = src.flip_t;
    d.bin = bin;
    d.blas_root = kTraverseDone;
    d.positions = sh.positions;
    d.normals = sh.normals;
    d.texcoords = sh.texcoords;
    d.indices = sh.indices;
    d.hidden = (src.mask & 0xFFu) == 0u ? 1u : 0u;
    return d;
}

}  // namespace

int main() {
    static const float pos[9] = {0, 0, 0, 1, 0, 0, 0, 1, 0};
    static const uint32_t idx[6] = {0, 1, 2, 0, 2, 1};
    // shapes: a 2-face mesh, a sphere, a 7-face mesh
    std::vector<InstShape> shapes(3);
    std::memset(shapes.data(), 0, sizeof(InstShape) * shapes.size());
    shapes[0] = InstShape{PUPIL_SHAPE_MESH, 2u, pos, nullptr, pos, idx};
    shapes[1] = InstShape{PUPIL_SHAPE_SPHERE, 0u, nullptr, nullptr, nullptr, nullptr};
    shapes[2] = InstShape{PUPIL_SHAPE_MESH, 7u, pos, pos, nullptr, idx};
    const std::vector<Source> src = {
        {0, 1, 0, 0, -1, 1, {2, 0, 0, 1, 0, 3, 0, -2, 0, 0, 0.5f, 4}},
        {1, 0, 1, 0, -1, 0, {0.5f, 0, 0, 1, 0, 0.5f, 0, 2, 0, 0, 0.5f, 3}},  // a hidden sphere
        {2, 2, 0, 1, 0, 0x100, {0, -1, 0, 0, 1, 0, 0, 0, 0, 0, 1, 7}},        // mask & 0xFF == 0: hidden
        {0, 3, 0, 0, -1, 0xFF, {1, 0.25f, 0, 0, 0, 1, 0.5f, 0, 0, 0, 1, 0}},
        {2, 1, 1, 1, -1, 1, {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0}},
    };
    const uint32_t n = (uint32_t)src.size();
    std::vector<uint32_t> counts(n);
    for (uint32_t i = 0; i < n; i++) counts[i] = shapes[src[i].shape].kind == PUPIL_SHAPE_SPHERE ? 1u : shapes[src[i].shape].num_faces;
    PrimTables tab;
    REQUIRE(prim_tables(counts.data(), n, &tab));
    REQUIRE(tab.num_prims == 2u + 1u + 7u + 2u + 7u && tab.inst_first.size() == n + 1);
    int cases = 0;
    std::vector<InstBinding> bind(n);
    for (uint32_t i = 0; i < n; i++)
        bind[i] = InstBinding{src[i].shape, src[i].material, src[i].flip_n, src[i].flip_t, src[i].emitter_offset,
                              (src[i].mask & 0xFFu) == 0u ? 1u : 0u, 1u + src[i].material};
    for (int with_inverse = 0; with_inverse < 2; with_inverse++)
        for (int nan_hidden = 0; nan_hidden < 2; nan_hidden++) {
            std::vector<DevInstance> table(n);  // exactly n records
            for (uint32_t i = 0; i < n; i++) {
                float inv[12];
                invert_affine3x4(src[i].to_world, inv);
                std::memset(&table[i], 0xAB, sizeof(DevInstance));  // every byte of the record must be written
                fill_instance_record(table[i], shapes[bind[i].shape], bind[i], tab.inst_first[i], src[i].to_world,
                                     with_inverse ? inv : nullptr, nan_hidden != 0);
                DevInstance ref = reference(src[i], shapes[src[i].shape], bind[i].bin, tab.inst_first[i], inv);
                const bool nan_object = nan_hidden && ref.hidden && ref.kind == PUPIL_SHAPE_SPHERE;
                if (nan_object) {  // pt_scene.h device_instance
                    const DevInstance dev = device_instance(ref);
                    REQUIRE(std::memcmp(&dev, &ref, sizeof(ref)) != 0);
                    for (float x : table[i].to_object) REQUIRE(std::isnan(x));
                    std::memcpy(table[i].to_object, ref.to_object, sizeof(ref.to_object));
                }
                REQUIRE(std::memcmp(&table[i], &ref, sizeof(DevInstance)) == 0);
                REQUIRE(table[i].prim_offset + counts[i] == tab.inst_first[i + 1]);
                cases++;
            }
        }
    std::printf("ok %d records\n", cases);
    return 0;
}
