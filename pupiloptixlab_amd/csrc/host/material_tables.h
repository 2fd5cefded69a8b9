// material_tables.h — MaterialTables, the one owner of the materials: the device material
// array, its host mirror and each bitmap slot's texels.  Plain C++ (no HIP): the device is a policy, as in
// host/emitter_tables.h, so the ownership paths run on the host under a sanitizer
// (tests/material_tables_driver.cpp).  Dev::alloc / free / Stream / upload / failed / write: as there.
#pragma once

#include <array>
#include <cmath>  // pt_math.h's host branch calls sqrtf before it includes <math.h>
#include <cstring>
#include <utility>
#include <vector>

#include "../pt_scene.h"
#include "emitter_tables.h"
#include "scoped_buffer.h"

namespace pupil {

// fresnel::DiffuseReflectance (render/material/fresnel.h:67-94)
inline float diffuse_reflectance(float eta) {
    if (eta < 1) {
        return -1.4399f * (eta * eta) + 0.7099f * eta + 0.6681f + 0.0636f / eta;
    }
    const float inv_eta = 1.0f / eta;
    const float inv_eta2 = inv_eta * inv_eta;
    const float inv_eta3 = inv_eta2 * inv_eta;
    const float inv_eta4 = inv_eta3 * inv_eta;
    const float inv_eta5 = inv_eta4 * inv_eta;
    return 0.919317f - 3.4793f * inv_eta + 6.75335f * inv_eta2 - 7.80989f * inv_eta3 + 4.98554f * inv_eta4 -
           1.36881f * inv_eta5;
}

// GetPixelAverage (optix_material.cpp:15-42)
// (the two halves, pt_scene.h, are the ones the device restates after a texel update)
inline vec3 pixel_average(const pupil_texture &t) {
    if (t.type == PUPIL_TEX_BITMAP && t.rgba && t.width && t.height) {
        float r = 0.f, g = 0.f, b = 0.f;
        for (size_t i = 0, idx = 0; i < t.height; ++i)
            for (size_t j = 0; j < t.width; ++j) {
                r += t.rgba[idx++];
                g += t.rgba[idx++];
                b += t.rgba[idx++];
                idx++;
            }
        return bitmap_average(v3(r, g, b), t.width, t.height);
    }
    return texture_const_average(t.type, t.c0, t.c1);
}

// one material (optix_material.cpp:39-132 host precompute) with its texture descriptors; the
// texels are placed by the owner below.  Touches nothing of an engine: it is also the validation
// of an update
inline int convert_material(const pupil_material &src, DevMaterial &d) {
    std::memset(&d, 0, sizeof(d));
    d.type = src.type <= 7u ? src.type : 0u;
    d.twosided = src.twosided;
    d.nonlinear = src.nonlinear;
    if (d.type == PUPIL_MAT_DIELECTRIC || d.type == PUPIL_MAT_ROUGH_DIELECTRIC || d.type == PUPIL_MAT_PLASTIC ||
        d.type == PUPIL_MAT_ROUGH_PLASTIC)
        d.eta = src.int_ior / src.ext_ior;
    for (int k = 0; k < 4; k++)
        if (const int rc = texture_desc(src.tex[k], d.tex[k])) return rc;
    if (d.type == PUPIL_MAT_PLASTIC || d.type == PUPIL_MAT_ROUGH_PLASTIC) {
        const pupil_texture &dt = d.type == PUPIL_MAT_PLASTIC ? src.tex[0] : src.tex[1];
        const pupil_texture &stx = d.type == PUPIL_MAT_PLASTIC ? src.tex[1] : src.tex[2];
        d.specular_sampling_weight = specular_sampling_weight(pixel_average(dt), pixel_average(stx));
        d.int_fdr = diffuse_reflectance(1.f / d.eta);
    }
    return PUPIL_OK;
}

template <typename Dev>
class MaterialTables {
public:
    using Texels = ScopedBuffer<float4, Dev>;
    // An update staged aside, a value: dropped before its commit it frees the texels it allocated.
    struct Entry {
        uint32_t id;
        DevMaterial conv;      // each bitmap slot's data: the slot's own texels (reused) or `fresh`
        const float *rgba[4];  // the caller's texels of each bitmap slot
        bool replace[4];       // the slot's texels are not reused: `fresh` (or none) takes their place
        std::array<Texels, 4> fresh;
    };
    using Staged = std::vector<Entry>;  // one entry per id, in the order of the call

    // The scene's materials and their bitmap texels, uploaded; the only writer of sc.materials and
    // sc.num_materials.  A scene without materials gets one zeroed material: a valid pointer for its instances
    int create(const pupil_material *materials, uint32_t n, DeviceScene &sc) {
        mirror_.resize(n ? n : 1);
        std::memset(mirror_.data(), 0, sizeof(DevMaterial) * mirror_.size());
        texels_ = std::vector<std::array<Texels, 4>>(mirror_.size());
        for (uint32_t m = 0; m < n; m++) {
            if (const int rc = convert_material(materials[m], mirror_[m])) return rc;
            for (int k = 0; k < 4; k++) {
                const pupil_texture &t = materials[m].tex[k];
                if (t.type != PUPIL_TEX_BITMAP) continue;
                const size_t count = (size_t)t.width * t.height;
                auto e = texels_[m][k].alloc(count);
                if (!e) e = Dev::upload(texels_[m][k].get(), t.rgba, sizeof(float4) * count);
                if (e) return Dev::failed(e, "upload(texels, t.rgba, t.width * t.height)");
                mirror_[m].tex[k].data = texels_[m][k].get();
            }
        }
        if (mats_.alloc(mirror_.size()) || Dev::upload(mats_.get(), mirror_.data(), sizeof(DevMaterial) * mirror_.size()))
            return fail(PUPIL_ERR_OOM, "scene upload failed");
        sc.materials = mats_.get();
        sc.num_materials = count();
        return PUPIL_OK;
    }

    // The "aside" step of pupil_pt_update_materials: everything that can refuse the call, then per slot
    // whether its texels are reused (a bitmap of an unchanged texel count), replaced or dropped, with the
    // fresh texels allocated into `out`.  An id named twice: its last material is the one that counts.
    // Nothing of the tables changes.
    int stage(uint32_t n, const uint32_t *ids, const pupil_material *materials, Staged &out) const {
        std::vector<DevMaterial> conv(n);
        for (uint32_t k = 0; k < n; k++) {
            if (ids[k] >= count()) return fail(PUPIL_ERR_INVALID, "material index out of range");
            if (const int rc = convert_material(materials[k], conv[k])) return rc;
        }
        for (uint32_t k = 0; k < n; k++) {
            bool last = true;
            for (uint32_t j = k + 1; j < n && last; j++) last = ids[j] != ids[k];
            if (!last) continue;
            out.emplace_back();
            Entry &e = out.back();
            e.id = ids[k];
            e.conv = conv[k];
            for (int s = 0; s < 4; s++) {
                DevTexture &nt = e.conv.tex[s];
                const DevTexture &ot = mirror_[e.id].tex[s];
                const bool bitmap = nt.type == PUPIL_TEX_BITMAP;
                const size_t texel_count = (size_t)nt.width * nt.height;
                e.rgba[s] = bitmap ? materials[k].tex[s].rgba : nullptr;
                e.replace[s] = !(bitmap && texels_[e.id][s].get() && (size_t)ot.width * ot.height == texel_count);
                if (!e.replace[s]) nt.data = ot.data;
                if (!e.replace[s] || !bitmap) continue;
                if (e.fresh[s].alloc(texel_count)) return fail(PUPIL_ERR_OOM, "texel allocation failed");
                nt.data = e.fresh[s].get();
            }
        }
        return PUPIL_OK;
    }

    // The staged update written behind the stream, entry by entry: texels, then the mirror and the slots'
    // owners, then the record.  `replaced` receives the texels that lost their slot: the caller drops them,
    // and `st`, once the stream has passed.  After a failed write the entries before it are in place; of the
    // others the mirror, records and owners are untouched (texels reused in place may hold new content).
    int commit(Staged &st, typename Dev::Stream stream, std::vector<Texels> &replaced, bool &type_changed) {
        for (Entry &e : st) {
            for (int s = 0; s < 4; s++) {
                const DevTexture &t = e.conv.tex[s];
                if (t.type != PUPIL_TEX_BITMAP) continue;
                if (const int rc = Dev::write((void *)t.data, e.rgba[s], sizeof(float4) * (size_t)t.width * t.height, stream))
                    return rc;
            }
            DevMaterial &h = mirror_[e.id];
            type_changed = type_changed || h.type != e.conv.type;
            h = e.conv;
            for (int s = 0; s < 4; s++) {
                if (!e.replace[s]) continue;
                if (texels_[e.id][s].get()) replaced.push_back(std::move(texels_[e.id][s]));
                texels_[e.id][s] = std::move(e.fresh[s]);
            }
            if (const int rc = Dev::write(mats_.get() + e.id, &h, sizeof(DevMaterial), stream)) return rc;
        }
        return PUPIL_OK;
    }

    DevMaterial *device() const { return mats_.get(); }
    // descriptors and texel pointers as the device holds them, but for one field: after a device texel
    // update of a plastic (pupil_pt_update_texture_device) its specular_sampling_weight is stale here
    const std::vector<DevMaterial> &mirror() const { return mirror_; }
    uint32_t count() const { return (uint32_t)mirror_.size(); }

private:
    ScopedBuffer<DevMaterial, Dev> mats_;
    std::vector<DevMaterial> mirror_;
    std::vector<std::array<Texels, 4>> texels_;  // per material, per slot: the bitmap's texels or none
};

}  // namespace pupil
