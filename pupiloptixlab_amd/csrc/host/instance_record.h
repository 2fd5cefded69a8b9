// instance_record.h — one instance's 224-byte DevInstance record from what it binds: one text for
// pupil_pt_create, for pupil_pt_set_instances' host mirror, for the kernel that fills a new
// instance table on the device (pt_instance_set.hip k_fill_instances) and for the stand-alone host
// driver of the tests.  The two-level fields (BLAS root and bases, margins, world box) are left
// empty: build_two_level's instance stage fills them in the host mirror and uploads the table
// again, at create and after pupil_pt_set_instances alike.
#pragma once

#include <math.h>

#include "../pt_invert.h"
#include "../pt_scene.h"

namespace pupil {

// The two margin terms of an instance (accel_two_level.hip instance_margin derives them), one text
// for the host and for the kernels that write instances on the device (pt_instances.hip,
// pt_instance_set.hip): infinity norms of the 3x3 parts and of the translations, in this order of
// operations.
PT_HD void instance_margin_values(const float *to_world, const float *to_object, float vmax, float *margin) {
    auto mx = [](float a, float b) { return a < b ? b : a; };  // std::max
    float anorm = 0.f, at = 0.f, mnorm = 0.f, mt = 0.f;
    for (int r = 0; r < 3; r++) {
        anorm = mx(anorm, fabsf(to_object[4 * r]) + fabsf(to_object[4 * r + 1]) + fabsf(to_object[4 * r + 2]));
        mnorm = mx(mnorm, fabsf(to_world[4 * r]) + fabsf(to_world[4 * r + 1]) + fabsf(to_world[4 * r + 2]));
        at = mx(at, fabsf(to_object[4 * r + 3]));
        mt = mx(mt, fabsf(to_world[4 * r + 3]));
    }
    const float c = 0x1p-18f;
    margin[0] = c * anorm;
    margin[1] = c * (anorm * (mnorm * vmax + mt) + at);
}

// What an instance takes from its shape: the engine-owned arrays.
struct InstShape {
    uint32_t kind, num_faces;
    const float *positions, *normals, *texcoords;
    const uint32_t *indices;
};

// What the caller binds per instance (pupil_instance's small integers and the mask) and the bin
// of its material.
struct InstBinding {
    uint32_t shape, material, flip_normals, flip_tex_coords;
    int32_t emitter_offset;
    uint32_t hidden, bin;
};

// to_object null: the inverse of to_world (pt_invert.h).  nan_hidden: the device copy of a hidden
// sphere, whose to_object is NaN (pt_scene.h device_instance); the host mirror keeps the real one.
PT_HD void fill_instance_record(DevInstance &d, const InstShape &sh, const InstBinding &b, uint32_t prim_offset,
                                const float *to_world, const float *to_object, bool nan_hidden) {
    float inv[12];
    if (!to_object) {
        invert_affine3x4(to_world, inv);
        to_object = inv;
    }
    const bool nan_object = nan_hidden && b.hidden && sh.kind == PUPIL_SHAPE_SPHERE;
    for (int c = 0; c < 12; c++) {
        d.to_world[c] = to_world[c];
        d.to_object[c] = nan_object ? __builtin_nanf("") : to_object[c];
    }
    d.kind = sh.kind;
    d.material = b.material;
    d.prim_offset = prim_offset;
    d.emitter_offset = b.emitter_offset;
    d.flip_normals = b.flip_normals;
    d.flip_tex_coords = b.flip_tex_coords;
    d.positions = sh.positions;
    d.normals = sh.normals;
    d.texcoords = sh.texcoords;
    d.indices = sh.indices;
    // the two-level fields, empty: the structure's instance stage fills them
    d.blas_root = kTraverseDone;
    d.attr_base = 0u;
    d.bin = b.bin;
    d.margin[0] = d.margin[1] = 0.f;
    for (int c = 0; c < 3; c++) d.wlo[c] = d.whi[c] = 0.f;
    d.wrec_delta = 0;
    d.rec_base = d.obj_nbase = d.obj_ncount = d.wnode_base = 0u;
    d.vmax = 0.f;
    d.hidden = b.hidden;
}

}  // namespace pupil
