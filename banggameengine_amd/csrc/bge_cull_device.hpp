// bge_cull_device.hpp — the visibility rule of include/bge_world.h as device code, shared by the passes that apply it
// (bge_cull.hip bge_world_visible*, bge_batch.hip bge_world_draw_batches*).  Files that include it are built with -ffp-contract=off.
#pragma once

#include <hip/hip_runtime.h>

#include "bge_cull.hpp"
#include "bge_device_math.hpp"
#include "bge_flatten.hpp"

namespace bge {

__device__ __forceinline__ bool finite_f(float v) { return __builtin_fabsf(v) < __builtin_inff(); } // false for NaN

// the rule of include/bge_world.h, operation for operation (the file is built with -ffp-contract=off)
__device__ __forceinline__ bool entity_visible(const CullParams& p, uint64_t e)
{
    if (!p.bounds) return false;
    const uint32_t s = p.slot_of_entity[e];
    if (s == kNone || s >= p.n_slots) return false;
    const uint32_t f = p.flag_words[s];
    const bool composed = dev::row3_deferred(s, p.row3.rs_word, p.row3.epoch); // (asked for with the flag word: one round trip)
    if (!(f & kValid) || (f & kTDirty)) return false; // no Transform here (a body kept without one), or limbo / not ticked yet
    const float* b = p.bounds + 6ull * e;
    const float cx = b[0], cy = b[1], cz = b[2], hx = b[3], hy = b[4], hz = b[5];
    if (!(hx >= 0.0f && hy >= 0.0f && hz >= 0.0f && finite_f(hx) && finite_f(hy) && finite_f(hz))) return false;
    if (!(finite_f(cx) && finite_f(cy) && finite_f(cz))) return false;
    const float4* world = reinterpret_cast<const float4*>(p.world);
    const float4* m = world + 4ull * s;
    const float4 r0 = m[0], r1 = m[1], r2 = m[2], r3 = dev::world_row3(world, s, p.row3.pos, composed);
    const float wx = ((cx * r0.x + cy * r1.x) + cz * r2.x) + r3.x;
    const float wy = ((cx * r0.y + cy * r1.y) + cz * r2.y) + r3.y;
    const float wz = ((cx * r0.z + cy * r1.z) + cz * r2.z) + r3.z;
    bool vis = true;
    for (uint32_t k = 0; k < p.n_planes; ++k) {
        const float a = p.planes[k][0], bb = p.planes[k][1], c4 = p.planes[k][2], d = p.planes[k][3];
        const float e0 = (a * r0.x + bb * r0.y) + c4 * r0.z;
        const float e1 = (a * r1.x + bb * r1.y) + c4 * r1.z;
        const float e2 = (a * r2.x + bb * r2.y) + c4 * r2.z;
        const float r = (__builtin_fabsf(e0) * hx + __builtin_fabsf(e1) * hy) + __builtin_fabsf(e2) * hz;
        const float sd = ((a * wx + bb * wy) + c4 * wz) + d;
        vis = vis && (sd >= -r); // false for a NaN on either side
    }
    return vis;
}

} // namespace bge
