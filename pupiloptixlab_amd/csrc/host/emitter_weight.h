// emitter_weight.h — the select weight of an area emitter's radiance texture, the one
// definition the host world (world.cpp AddAreaEmitter) and the engine's device-side emitter
// table (engine.hip pupil_pt_enable_device_emitters) share.
#pragma once

#include <cstddef>

#include "../../../include/pupil_pt.h"

namespace Pupil {
namespace world {

// emitter.cpp:73-101 GetWeight: the largest channel of an RGB colour, the mean of the two
// patches' largest channels of a checkerboard, the mean over a bitmap's texels of their largest
// channel.  The bitmap walk is the reference's, bug for bug: it indexes texel (i * width + j) for
// i < width, j < height and skips what falls outside the width * height * 4 floats.
inline float GetWeight(const pupil_texture &t) {
    auto mx = [](float r, float g, float b) { return r > g ? (r > b ? r : b) : (g > b ? g : b); };
    if (t.type == PUPIL_TEX_RGB) return mx(t.c0[0], t.c0[1], t.c0[2]);
    if (t.type == PUPIL_TEX_CHECKERBOARD) return (mx(t.c0[0], t.c0[1], t.c0[2]) + mx(t.c1[0], t.c1[1], t.c1[2])) * 0.5f;
    if (t.type == PUPIL_TEX_BITMAP && t.rgba) {
        float w = 0.f;
        const float *d = t.rgba;
        const size_t size = (size_t)t.width * t.height * 4;
        for (size_t i = 0; i < t.width; i++)
            for (size_t j = 0; j < t.height; j++) {
                const size_t k = (i * t.width + j) * 4;
                if (k + 2 < size) w += mx(d[k], d[k + 1], d[k + 2]);
            }
        return w / (1.f * t.width * t.height);
    }
    return 0.f;
}

}  // namespace world
}  // namespace Pupil
