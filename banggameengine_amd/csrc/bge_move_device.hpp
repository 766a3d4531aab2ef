// bge_move_device.hpp — the arithmetic of one slide round (include/bge_world.h "Sphere moves", rounds 2-7) and the cast record a
// mover asks, shared by the plain moves (bge_move.hip) and the step moves (bge_step.hip) so that both run the same expressions,
// operation for operation (the build's -ffp-contract=off keeps one rounding each).  Device code only.
#pragma once

#include <hip/hip_runtime.h>

#include "../../include/bge_world.h"

namespace bge {
namespace slide {

// bits of a lane's word (bge_move.hpp plane 3): flags in 0..7, n_hits in 8..15, last hit kind in 16..17, then these
constexpr uint32_t kHasPrev = 1u << 24, kFinished = 1u << 25;
constexpr float kRestSq = 1e-12f;       // squared length below which nothing is left to spend
constexpr float kMinApproach = 0.0625f; // the clamp of the approach cosine: bounds the back-off at grazing angles

__device__ __forceinline__ float dot3(float ax, float ay, float az, float bx, float by, float bz) { return (ax * bx + ay * by) + az * bz; }

// The cast record at index i: p.w is the radius; mask = 0 asks nothing
__device__ __forceinline__ void write_cast(void* casts, uint64_t i, const float4& p, float dx, float dy, float dz, float max_distance, uint32_t mask)
{
    uint32_t* c = static_cast<uint32_t*>(casts) + 10ull * i;
    c[0] = __float_as_uint(p.x);
    c[1] = __float_as_uint(p.y);
    c[2] = __float_as_uint(p.z);
    c[3] = __float_as_uint(dx);
    c[4] = __float_as_uint(dy);
    c[5] = __float_as_uint(dz);
    c[6] = __float_as_uint(max_distance);
    c[7] = __float_as_uint(p.w); // radius
    c[8] = mask;
    c[9] = 0u;
}

// Step 1 of the next round, taken where r is made: nothing left to spend finishes the mover
__device__ __forceinline__ bool spent(const float4& r) { return !(dot3(r.x, r.y, r.z, r.x, r.y, r.z) > kRestSq); }

// One round of a lane that is not finished, from the hit record h (bge_ray_hit, word by word) of its cast {pos, r, 1}: steps 2-7.
// pos.w is the radius, r.w the skin, prev.xyz the previous normal (valid with kHasPrev); bits is updated (n_hits, kind, kHasPrev,
// kFinished, and BGE_MOVE_OUT_OF_SLIDES when last and something is left).  Returns whether the round hit; lasthit (normal, entity)
// is written only then.
__device__ __forceinline__ bool one_round(float4& pos, float4& r, const float4& d0, float4& prev, uint32_t& bits, float4& lasthit, const uint32_t* h,
                                          bool last)
{
    const uint32_t kind = h[0];
    if (kind == BGE_RAY_MISS) { // step 2: the way is free
        pos.x = pos.x + r.x;
        pos.y = pos.y + r.y;
        pos.z = pos.z + r.z;
        r.x = r.y = r.z = 0.0f;
        bits |= kFinished;
        return false;
    }
    const float f = __uint_as_float(h[2]);
    const float nx = __uint_as_float(h[7]), ny = __uint_as_float(h[8]), nz = __uint_as_float(h[9]);
    // step 3: up to the touch, less the skin along the approach
    const float len = __builtin_sqrtf(dot3(r.x, r.y, r.z, r.x, r.y, r.z));
    float a = -(dot3(r.x, r.y, r.z, nx, ny, nz) / len);
    if (!(a >= kMinApproach)) a = kMinApproach;
    float g = f - r.w / (a * len);
    if (!(g > 0.0f)) g = 0.0f;
    pos.x = pos.x + r.x * g;
    pos.y = pos.y + r.y * g;
    pos.z = pos.z + r.z * g;
    bits = ((bits & ~(3u << 16)) | (kind << 16)) + (1u << 8); // the last hit's kind, n_hits + 1
    lasthit = make_float4(nx, ny, nz, __uint_as_float(h[1]));
    // step 4: what is left, along the surface
    const float w = 1.0f - f;
    const float lx = r.x * w, ly = r.y * w, lz = r.z * w;
    const float dn = dot3(lx, ly, lz, nx, ny, nz);
    float sx = lx - nx * dn, sy = ly - ny * dn, sz = lz - nz * dn;
    // step 5: into the previous surface again: along the crease of the two
    if ((bits & kHasPrev) && dot3(sx, sy, sz, prev.x, prev.y, prev.z) < 0.0f) {
        const float cx = prev.y * nz - prev.z * ny, cy = prev.z * nx - prev.x * nz, cz = prev.x * ny - prev.y * nx;
        const float cc = dot3(cx, cy, cz, cx, cy, cz);
        if (!(cc > kRestSq)) {
            sx = sy = sz = 0.0f;
        } else {
            const float t = dot3(lx, ly, lz, cx, cy, cz) / cc;
            sx = cx * t;
            sy = cy * t;
            sz = cz * t;
        }
    }
    // step 6: never against the asked direction
    if (!(dot3(sx, sy, sz, d0.x, d0.y, d0.z) > 0.0f)) sx = sy = sz = 0.0f;
    // step 7
    r.x = sx;
    r.y = sy;
    r.z = sz;
    prev.x = nx;
    prev.y = ny;
    prev.z = nz;
    bits |= kHasPrev;
    if (spent(r)) {
        r.x = r.y = r.z = 0.0f;
        bits |= kFinished;
    } else if (last) {
        bits |= BGE_MOVE_OUT_OF_SLIDES;
    }
    return true;
}

} // namespace slide
} // namespace bge
